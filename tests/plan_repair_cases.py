"""Inputs for the plan repair tests (tests/test_plan_repair.py on the CPU, tests/test_gpu_plan_repair.py on the GPU): hand-made
cases on windows of 15 x 15 cells at the most, each with the rows the contract (include/smpc_plan_repair.h) gives written out,
and seeded batches. A case is what plan_repair_ref.run takes: dict(costmap, origin, res, pose, plan, plan_len, plan_start, R,
stride, clearance_d2, cost) plus, for a hand-made one, want = dict(status [B], info [B][4], rows {b: the whole new plan}).

The hand-made windows have cells of 1 m and their origin at (0, 0): cell i spans [i, i + 1) and its centre is i + 0.5, so
every expected row can be read off the picture. Free cells cost 0 (w = 50: 250 along an axis, 350 along a diagonal)."""
import numpy as np

import global_plan_ref as G
import plan_repair_ref as R

LETHAL = 254


def straight(y=7.5, x0=2.5, n=11):
    return [(x0 + k, y) for k in range(n)]


def make(costmap, pose, rows, L, radius, stride=1, clearance_d2=0.0, cost=None, start=None, plan_len=None, want=None):
    """One robot (or B with lists of poses / plans) on a window with cells of 1 m at the origin."""
    costmap = np.asarray(costmap, np.uint8)
    pose = np.asarray(pose, np.float64).reshape(-1, 2)
    B = pose.shape[0]
    rows = [rows] * B if not isinstance(rows[0], list) else rows
    plan = np.full((B, L, 2), -77.25)                      # rows beyond the plan: a sentinel the call leaves alone
    for b in range(B):
        plan[b, :len(rows[b])] = np.array(rows[b], np.float64)
    n = np.array([len(r) for r in rows] if plan_len is None else plan_len, np.int32)
    return dict(costmap=costmap, origin=np.zeros(2) if costmap.ndim == 2 else np.zeros((B, 2)), res=1.0,
                pose=np.concatenate([pose, np.full((B, 1), 0.3)], axis=1), plan=plan, plan_len=n,
                plan_start=None if start is None else np.asarray(start, np.int32), R=radius, stride=stride, clearance_d2=clearance_d2,
                cost=cost or G.Cost(), want=want)


def floor(blocked=(), size=15, value=LETHAL, fill=0):
    m = np.full((size, size), fill, np.uint8)
    for x, y in blocked:
        m[y, x] = value
    return m


# the detour of "wall" between the robot and the rejoin: up to row 9, along it over the wall, down to row 7. The diagonal from
# (5, 9) to (6, 8) would cut the corner of the blocked (5, 8), so the detour turns at (6, 9).
OVER = [(3.5, 8.5), (4.5, 9.5), (5.5, 9.5), (6.5, 9.5), (6.5, 8.5)]


def hand_cases():
    c = {}
    wall = [(5, 6), (5, 7), (5, 8)]
    line = straight()
    # a wall segment across a straight plan along y = 7.5: pose 3 (cell 5) is blocked, pose 4 is the rejoin. Two diagonal and
    # four axis steps (1700) either way round; y + 1 comes before y - 1 in the neighbour order: (2,7) (3,8) (4,9) (5,9) (6,9) (6,8) (6,7)
    c["wall"] = make(floor(wall)[None], (2.5, 7.5), line, 16, 7, want=dict(
        status=[R.REPAIRED], info=[[0, 3, 4, 6]], rows={0: [(2.5, 7.5)] + OVER + line[4:]}))
    # a wall from top to bottom but for the rows 0 and 6; next to the opening at (5, 6) the cell (4, 6) is blocked, so the
    # opening could only be entered diagonally between two blocked cells, which the rule forbids: the detour runs through row
    # 0, axis steps before diagonal ones where both cost the same
    gap = [(5, y) for y in range(1, 15) if y != 6] + [(4, 6)]
    c["diagonal_gap"] = make(floor(gap)[None], (2.5, 7.5), line, 40, 7, want=dict(
        status=[R.REPAIRED], info=[[0, 3, 4, 16]],
        rows={0: [(2.5, 7.5), (2.5, 6.5), (2.5, 5.5), (2.5, 4.5), (2.5, 3.5), (2.5, 2.5), (3.5, 1.5), (4.5, 0.5), (5.5, 0.5), (6.5, 0.5), (6.5, 1.5),
                  (6.5, 2.5), (6.5, 3.5), (6.5, 4.5), (6.5, 5.5), (6.5, 6.5)] + line[4:]}))
    # two blocked runs in view: i1 from the first, i2 from the second; row 8 passes both, and (6, 8) -> (7, 7) would cut (6, 7)
    c["two_runs"] = make(floor([(4, 7), (6, 7)])[None], (2.5, 7.5), line, 16, 7, want=dict(
        status=[R.REPAIRED], info=[[0, 2, 5, 6]], rows={0: [(2.5, 7.5), (3.5, 8.5), (4.5, 8.5), (5.5, 8.5), (6.5, 8.5), (7.5, 8.5)] + line[5:]}))
    # the rejoin pushed on by the clearance: 2 m from pose 3 (5.5) is pose 5 (7.5); (6, 8) -> (7, 7) cuts nothing
    c["clearance"] = make(floor(wall)[None], (2.5, 7.5), line, 16, 7, clearance_d2=4.0, want=dict(
        status=[R.REPAIRED], info=[[0, 3, 5, 6]], rows={0: [(2.5, 7.5)] + OVER + line[5:]}))
    # m = 0: the plan runs into a blocked cell and comes back to the robot's own cell, where it rejoins
    loop = [(6.5, 7.5), (7.5, 7.5), (6.6, 7.6), (6.5, 8.5), (6.5, 9.5)]
    c["m_zero"] = make(floor([(7, 7)])[None], (6.4, 7.4), loop, 8, 7, want=dict(
        status=[R.REPAIRED], info=[[0, 1, 2, 0]], rows={0: [(6.4, 7.4), (6.6, 7.6), (6.5, 8.5), (6.5, 9.5)]}))
    # m < stride: (2,7) (3,8) (4,8) (5,8) (5,7), no centre at all between the robot and the rejoin
    c["m_below_stride"] = make(floor([(4, 7)])[None], (2.5, 7.5), line, 16, 7, stride=5, want=dict(
        status=[R.REPAIRED], info=[[0, 2, 3, 4]], rows={0: [(2.5, 7.5)] + line[3:]}))
    # the robot's own cell impassable: pose 0 in it is not blocked, and the field starts from it all the same
    c["own_cell"] = make(floor(wall + [(2, 7)])[None], (2.5, 7.5), line, 16, 7, want=dict(
        status=[R.REPAIRED], info=[[0, 3, 4, 6]], rows={0: [(2.5, 7.5)] + OVER + line[4:]}))
    # two equally near poses (2.5 and 3.5 from x = 3, cell 3): the lower index wins, and row 0 becomes the robot's point
    c["tie"] = make(floor(wall)[None], (3.0, 7.5), line, 16, 7, want=dict(
        status=[R.REPAIRED], info=[[0, 3, 4, 6]], rows={0: [(3.0, 7.5), (3.5, 8.5)] + OVER[1:] + line[4:]}))
    # plan_start = 2 with the nearest pose of all (0) in front of it: rows 0 and 1 stay, row 2 becomes the robot's point
    c["plan_start"] = make(floor(wall)[None], (2.5, 7.5), line, 16, 7, start=[2], want=dict(
        status=[R.REPAIRED], info=[[2, 3, 4, 6]], rows={0: line[:2] + [(2.5, 7.5)] + OVER + line[4:]}))
    # NaN rows: pose 0 cannot win the arg-min, pose 6 ends the stretch in view (and stays in the tail)
    nan = straight()
    nan[0] = (np.nan, 7.5)
    nan[6] = (8.5, np.nan)
    c["nan_rows"] = make(floor(wall)[None], (2.6, 7.5), nan, 16, 7, want=dict(
        status=[R.REPAIRED], info=[[1, 3, 4, 6]], rows={0: [nan[0], (2.6, 7.5)] + OVER + nan[4:]}))
    c["nan_before_rejoin"] = make(floor(wall)[None], (2.6, 7.5), nan[:4] + [(np.nan, np.nan)] + nan[5:], 16, 7, want=dict(
        status=[R.NO_REJOIN], info=[[1, 3, -1, -1]], rows={}))
    # n' == L and n' == L + 1 ("wall" gives 13 rows)
    c["fits_exactly"] = make(floor(wall)[None], (2.5, 7.5), line, 13, 7, want=dict(
        status=[R.REPAIRED], info=[[0, 3, 4, 6]], rows={0: [(2.5, 7.5)] + OVER + line[4:]}))
    c["too_long"] = make(floor(wall)[None], (2.5, 7.5), line, 12, 7, want=dict(
        status=[R.TOO_LONG], info=[[0, 3, 4, 6]], rows={}))
    # a sealed pocket: a ring around the robot, the rejoin outside
    ring = [(x, y) for x in range(0, 5) for y in range(5, 10) if max(abs(x - 2), abs(y - 7)) == 2]
    c["sealed_pocket"] = make(floor(ring)[None], (2.5, 7.5), line, 16, 7, want=dict(
        status=[R.UNREACHABLE_CELL], info=[[0, 2, 3, -1]], rows={}))
    # blocked up to the region's edge (R = 4: cells 0 .. 6 of the row are in view)
    c["no_rejoin"] = make(floor([(x, 7) for x in range(5, 9)])[None], (2.5, 7.5), line, 16, 4, want=dict(
        status=[R.NO_REJOIN], info=[[0, 3, -1, -1]], rows={}))
    # a region clipped by the window's corner: the wall reaches the window's rim, the only way is below it
    c["corner"] = make(floor([(4, 0), (4, 1), (4, 2)])[None], (1.5, 1.5), straight(1.5, 1.5), 16, 7, want=dict(
        status=[R.REPAIRED], info=[[0, 3, 4, 6]],
        rows={0: [(1.5, 1.5), (2.5, 2.5), (3.5, 3.5), (4.5, 3.5), (5.5, 3.5), (5.5, 2.5)] + straight(1.5, 1.5)[4:]}))
    # one costmap for three robots: one repaired, one clear (it stands behind the wall), one without a cell
    c["shared"] = make(floor(wall), [(2.5, 7.5), (6.5, 7.5), (15.5, 7.5)], line, 16, 7, want=dict(
        status=[R.REPAIRED, R.CLEAR, R.NO_CELL], info=[[0, 3, 4, 6], [4, -1, -1, -1], [-1, -1, -1, -1]], rows={0: [(2.5, 7.5)] + OVER + line[4:]}))
    # allow_unknown: the plan crosses cells of 255, which are passable and cost 50 + 255 each; the wall is still a wall
    unknown = floor(wall, fill=255)
    c["allow_unknown"] = make(unknown[None], (2.5, 7.5), line, 16, 7, cost=G.Cost(allow_unknown=True), want=dict(
        status=[R.REPAIRED], info=[[0, 3, 4, 6]], rows={0: [(2.5, 7.5)] + OVER + line[4:]}))
    c["unknown_blocks"] = make(unknown[None], (2.5, 7.5), line, 16, 7, want=dict(
        status=[R.NO_REJOIN], info=[[0, 1, -1, -1]], rows={}))
    # plans that are no plans: n < 2, n > L, s < 0, s >= n; s = n - 1 is one
    c["no_plan"] = make(floor(wall), [(2.5, 7.5)] * 5, line, 16, 7, plan_len=[1, 17, 11, 11, 11], start=[0, 0, -1, 11, 10], want=dict(
        status=[R.NO_PLAN, R.NO_PLAN, R.NO_PLAN, R.NO_PLAN, R.CLEAR], info=[[-1] * 4] * 4 + [[10, -1, -1, -1]], rows={}))
    c["no_finite_distance"] = make(floor(wall)[None], (2.5, 7.5), [(np.nan, 1.0), (np.inf, 2.0), (1e200, 3.0)], 16, 7, want=dict(
        status=[R.NO_PLAN], info=[[-1] * 4], rows={}))
    return c


def check_want(case, got):
    """The outputs of a hand-made case against its written expectations."""
    want = case["want"]
    assert got["status"].tolist() == want["status"], (got["status"].tolist(), want["status"])
    assert got["info"].tolist() == want["info"], (got["info"].tolist(), want["info"])
    for b in range(len(want["status"])):
        if b in want["rows"]:
            rows = np.array(want["rows"][b], np.float64)
            assert got["plan_len"][b] == len(rows), (b, got["plan_len"][b], len(rows))
            assert G.same_bits(got["plan"][b, :len(rows)], rows), (b, got["plan"][b, :len(rows)].tolist())
            assert G.same_bits(got["plan"][b, len(rows):], case["plan"][b, len(rows):])
        else:
            assert want["status"][b] != R.REPAIRED
            assert got["plan_len"][b] == case["plan_len"][b] and G.same_bits(got["plan"][b], case["plan"][b])


# ---- seeded batches ------------------------------------------------------------------------------------------------------------
SHAPES = [(67, 9, (9, 7), 1, 1), (67, 65, (21, 21), 4, 3), (33, 130, (40, 40), 15, 2), (9, 400, (80, 80), 31, 2), (5, 400, (127, 127), 63, 1)]


def seeded_name(B, L, window, radius, stride):
    return f"B{B}_L{L}_{window[0]}x{window[1]}_R{radius}_s{stride}"


def _stamp(m, cx, cy, r, value=LETHAL, ring=False):
    H, W = m.shape
    for y in range(max(0, cy - r), min(H, cy + r + 1)):
        for x in range(max(0, cx - r), min(W, cx + r + 1)):
            d = max(abs(x - cx), abs(y - cy))
            if (d == r) if ring else ((x - cx) ** 2 + (y - cy) ** 2 <= r * r):
                m[y, x] = value


def seeded_case(B, L, window, radius, stride, seed):
    """Per robot its own window. A plan starts a little behind the robot, runs straight for a while, bends once and runs on,
    its poses 0.6 cells apart (whole cells for the smallest regions); what is put on it decides the robot's fate: nothing,
    a blob to go around, a band up to the region's edge, a ring that seals the robot in, a plan that fills its rows, a robot
    off its window, a plan that is none. Some windows carry graded costs and unknown cells as well."""
    rng = np.random.default_rng(seed)
    W, H = window
    res = 0.05
    costmap = np.zeros((B, H, W), np.uint8)
    origin = rng.uniform(-3.0, 3.0, (B, 2))
    pose = np.zeros((B, 3))
    plan = np.full((B, L, 2), np.nan)
    plan_len = np.zeros(B, np.int32)
    start = np.zeros(B, np.int32)
    small = radius <= 2
    kinds = ["blob", "blob", "blob", "clear", "band", "ring", "long", "off", "none", "blob_graded"]
    for b in range(B):
        kind = kinds[b % len(kinds)]
        if rng.random() < 0.5:
            costmap[b] = rng.integers(0, 120, (H, W)) * (rng.random((H, W)) < 0.3)
        ax, ay = int(rng.integers(W // 3, W - W // 3)), int(rng.integers(H // 3, H - H // 3))
        p = (np.array([ax, ay]) + rng.uniform(0.1, 0.9, 2)) * res + origin[b]
        pose[b] = [p[0], p[1], rng.uniform(-3, 3)]
        # the plan, in cells relative to the robot's cell centre
        step = 1.0 if small else 0.6
        theta = rng.integers(0, 8) * np.pi / 4 if small else rng.uniform(0, 2 * np.pi)
        turn = theta + rng.choice([-1, 1]) * (np.pi / 2 if small else rng.uniform(np.pi / 4, np.pi / 2))
        behind = int(rng.integers(0, 3))
        n = int(min(L, rng.integers(max(4, L // 2), L + 1))) if kind != "long" else L
        if kind not in ("long",) and not small:
            n = max(4, min(n, L - int(2.5 * radius) - 4))     # room for a detour
        bend = behind + (1 if small else int(rng.integers(max(2, radius // 2), max(3, radius))))
        pts, q = [], np.zeros(2) - behind * step * np.array([np.cos(theta), np.sin(theta)])
        for k in range(n):
            pts.append(q.copy())
            ang = theta if k < bend else turn
            q = q + step * np.array([np.cos(ang), np.sin(ang)]) / (max(abs(np.cos(ang)), abs(np.sin(ang))) if small else 1.0)
        pts = np.array(pts)
        centre = (np.array([ax, ay]) + 0.5) * res + origin[b]
        jitter = rng.uniform(-0.2, 0.2, pts.shape) * res
        plan[b, :n] = centre + pts * res + jitter
        plan_len[b] = n
        start[b] = int(rng.integers(0, behind + 1))

        def on_plan(k):
            c = G.cell_of(plan[b, min(k, n - 1)], origin[b], res, W, H)
            return c

        ahead = behind + (1 if small else int(rng.integers(2, max(3, min(bend, radius - 2)))))
        c = on_plan(ahead)
        if kind in ("blob", "blob_graded", "long") and c is not None and c != (ax, ay):
            _stamp(costmap[b], c[0], c[1], 0 if small else int(rng.integers(0, max(1, min(3, radius // 4)) + 1)))
            if kind == "blob_graded":
                _stamp(costmap[b], c[0], c[1], 0, value=255)
            if max(abs(c[0] - ax), abs(c[1] - ay)) == 0:
                costmap[b, ay, ax] = 0
        elif kind == "band" and c is not None:
            for k in range(ahead, n):
                ck = on_plan(k)
                if ck is not None and ck != (ax, ay):
                    costmap[b, ck[1], ck[0]] = LETHAL
        elif kind == "ring" and not small and c is not None:
            _stamp(costmap[b], ax, ay, max(1, min(radius - 2, max(abs(c[0] - ax), abs(c[1] - ay)))), ring=True)
        elif kind == "ring" and c is not None and c != (ax, ay):
            costmap[b, c[1], c[0]] = LETHAL                  # R = 1: the blocked pose next to the robot, and the rejoin sealed off
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    if (dx, dy) != (0, 0) and on_plan(ahead + 1) != (ax + dx, ay + dy) and 0 <= ax + dx < W and 0 <= ay + dy < H:
                        costmap[b, ay + dy, ax + dx] = LETHAL
        elif kind == "off":
            pose[b, :2] = origin[b] + (np.array([W, H]) + rng.uniform(0.5, 3.0, 2)) * res * rng.choice([-1, 1], 2)
            if rng.random() < 0.3:
                pose[b, 0] = np.nan
        elif kind == "none":
            which = int(rng.integers(0, 4))
            if which == 0:
                plan_len[b] = int(rng.integers(-2, 2))
            elif which == 1:
                plan_len[b] = L + int(rng.integers(1, 5))
            elif which == 2:
                start[b] = n + int(rng.integers(0, 3))
            else:
                plan[b, :, 0] = np.nan
        if rng.random() < 0.15:
            costmap[b, ay, ax] = LETHAL                      # the robot's own cell
        if rng.random() < 0.2 and n > 6:
            plan[b, int(rng.integers(0, n))] = np.nan         # a hole in the plan
    return dict(costmap=costmap, origin=origin, res=res, pose=pose, plan=plan, plan_len=plan_len, plan_start=start, R=radius, stride=stride,
                clearance_d2=float(np.float64(0.1) * np.float64(0.1)) if not small else 0.0, cost=G.Cost(allow_unknown=bool(seed & 1)))


def seeded_cases():
    return {seeded_name(*s): seeded_case(*s, seed=100 + i) for i, s in enumerate(SHAPES)}
