"""Cases of the plan smoothing for tests/test_plan_smoother.py and tests/test_gpu_plan_smoother.py: hand-made ones whose
expected result is written out (worked by hand from include/smpc_plan_smoother.h with dyadic numbers, so that every step is
exact), the 91-pose staircase of the issue, and seeded ones on a 96 x 64 world with discs. A case is a dict:
    plan [B,L,2], plan_len [B] int32, range None or [B,2] int32, world [H,W] (shared) or [B,H,W] uint8, origin [2] or [B,2],
    res, w_data, w_smooth, tolerance, max_its, refinement_num, lethal_min_cost, allow_unknown
and, for a hand-made one, want = dict(status [B], info [B][4], change [B], rows {(b, i): (x, y)}): the rows that moved; every
other row must come back bit for bit."""
import numpy as np

CONVERGED, MAX_ITS, TOO_SHORT, BAD_PLAN = range(4)
SENTINEL = -7.25          # rows behind plan_len in the hand-made cases


def case(rows, n=None, L=8, world=None, origin=(0.0, 0.0), res=0.5, w_data=0.25, w_smooth=0.25, tolerance=1e-10, max_its=1000,
         refinement_num=0, lethal_min_cost=253, allow_unknown=False, rng=None, want=None, tail=SENTINEL):
    """One robot on a shared map (default: 16 x 12 free cells of 0.5 m)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 2)
    plan = np.full((1, L, 2), tail, np.float64)
    plan[0, :len(rows)] = rows
    return dict(plan=plan, plan_len=np.array([len(rows) if n is None else n], np.int32),
                range=None if rng is None else np.array([rng], np.int32),
                world=np.zeros((12, 16), np.uint8) if world is None else np.asarray(world, np.uint8), origin=np.array(origin, np.float64),
                res=res, w_data=w_data, w_smooth=w_smooth, tolerance=tolerance, max_its=max_its, refinement_num=refinement_num,
                lethal_min_cost=lethal_min_cost, allow_unknown=allow_unknown, want=want)


def world_with(cells, value):
    w = np.zeros((12, 16), np.uint8)
    for x, y in cells:
        w[y, x] = value
    return w


CORNER = [(1.0, 1.0), (2.0, 1.0), (2.0, 2.0)]                                   # one movable row, (2, 1)
LINE = [(1.0, 1.0), (1.5, 1.0), (2.0, 1.0), (2.5, 1.0), (3.0, 1.0)]             # collinear, evenly spaced, dyadic
STAIRS = [(1.0, 1.0), (2.0, 1.0), (2.0, 2.0), (3.0, 2.0), (3.0, 3.0)]           # three movable rows


def hand_cases():
    """With w_data = w_smooth = 1/4 a sweep of the corner's row (2, 1) between (1, 1) and (2, 2), p = y:
    x: a = 0, b = 0, s = 2 + 1 = 3, d = 4, e = -1, f = -1/4, g = -1/4, c = 1.75;  y: s = 2 + 1 = 3, d = 2, e = 1, f = 1/4, c = 1.25.
    Its cell at 0.5 m is (3, 2). The second sweep of the same round (p = (2, 1), y = (1.75, 1.25)):
    x: a = 1/4, b = 1/16, s = 3, d = 3.5, e = -1/2, f = -1/8, g = -1/16, c = 1.6875;  y: a = -1/4, b = -1/16, s = 3, d = 2.5, e = 1/2,
    f = 1/8, g = 1/16, c = 1.3125. A refinement instead (p := y = (1.75, 1.25)): x: a = 0, e = -1/2, c = 1.625; y: e = 1/2, c = 1.375;
    and one more (p := y = (1.625, 1.375)): x: d = 3.25, e = -1/4, c = 1.5625; y: d = 2.75, e = 1/4, c = 1.4375."""
    short = lambda n: dict(status=[TOO_SHORT], info=[[0, 0, 0, n]], change=[0.0], rows={})
    one = dict(status=[MAX_ITS], info=[[1, 1, 0, 3]], change=[0.25], rows={(0, 1): (1.75, 1.25)})
    kept = dict(status=[CONVERGED], info=[[1, 1, 1, 3]], change=[0.0], rows={})          # the one candidate rejected: nothing moves
    out = {
        "n0": case(CORNER, n=0, want=short(0)),
        "n1": case(CORNER, n=1, want=short(1)),
        "n2": case(CORNER, n=2, want=short(2)),
        "n_negative": case(CORNER, n=-3, want=short(0)),
        "n3_corner_one_sweep": case(CORNER, max_its=1, want=one),
        "n_above_L": case(LINE, n=9, L=5, want=dict(status=[CONVERGED], info=[[1, 1, 0, 5]], change=[0.0], rows={})),
        "nan_in_a_row": case([(1.0, 1.0), (2.0, np.nan), (2.0, 2.0)], want=dict(status=[BAD_PLAN], info=[[0, 0, 0, 3]], change=[0.0], rows={})),
        "inf_in_a_short_plan": case([(1.0, np.inf), (2.0, 1.0)], want=dict(status=[BAD_PLAN], info=[[0, 0, 0, 2]], change=[0.0], rows={})),
        "nan_beyond_n": case(CORNER, max_its=1, tail=np.nan, want=one),
        "collinear": case(LINE, want=dict(status=[CONVERGED], info=[[1, 1, 0, 5]], change=[0.0], rows={})),
        "collinear_tolerance_zero": case(LINE, tolerance=0.0, want=dict(status=[CONVERGED], info=[[1, 1, 0, 5]], change=[0.0], rows={})),
        "collinear_refinement_2": case(LINE, refinement_num=2, want=dict(status=[CONVERGED], info=[[3, 3, 0, 5]], change=[0.0], rows={})),
        "max_its_reached": case(CORNER, max_its=2, refinement_num=2,
                                want=dict(status=[MAX_ITS], info=[[2, 1, 0, 3]], change=[0.0625], rows={(0, 1): (1.6875, 1.3125)})),
        # tolerance 1: every sweep ends its round
        "refinement_0": case(CORNER, tolerance=1.0, refinement_num=0,
                             want=dict(status=[CONVERGED], info=[[1, 1, 0, 3]], change=[0.25], rows={(0, 1): (1.75, 1.25)})),
        "refinement_1": case(CORNER, tolerance=1.0, refinement_num=1,
                             want=dict(status=[CONVERGED], info=[[2, 2, 0, 3]], change=[0.125], rows={(0, 1): (1.625, 1.375)})),
        "refinement_2": case(CORNER, tolerance=1.0, refinement_num=2,
                             want=dict(status=[CONVERGED], info=[[3, 3, 0, 3]], change=[0.0625], rows={(0, 1): (1.5625, 1.4375)})),
        "rejected_by_a_lethal_cell": case(CORNER, world=world_with([(3, 2)], 254), want=kept),
        "rejected_by_cost_253": case(CORNER, world=world_with([(3, 2)], 253), want=kept),
        "accepted_at_cost_252": case(CORNER, world=world_with([(3, 2)], 252), max_its=1, want=one),
        "rejected_by_unknown": case(CORNER, world=world_with([(3, 2)], 255), want=kept),
        "accepted_with_allow_unknown": case(CORNER, world=world_with([(3, 2)], 255), allow_unknown=True, max_its=1, want=one),
        # row (0.25, 1) between (-2, 1) and (0.5, 1): x: s = 0.5 - 2 = -1.5, d = 0.5, e = -2, f = -1/2, c = -0.25: left of the map
        "rejected_by_the_maps_edge": case([(-2.0, 1.0), (0.25, 1.0), (0.5, 1.0)], want=kept),
        # the stairs, one sweep (tolerance 1): (2, 1) -> (1.75, 1.25) as above; (2, 2) between (2, 1) and (3, 2): x: s = 5, d = 4,
        # e = 1, c = 2.25, y: s = 3, d = 4, e = -1, c = 1.75; (3, 2) between (2, 2) and (3, 3): x: s = 5, d = 6, e = -1, c = 2.75,
        # y: s = 5, d = 4, e = 1, c = 2.25
        "stairs": case(STAIRS, tolerance=1.0, want=dict(status=[CONVERGED], info=[[1, 1, 0, 5]], change=[0.25],
                                                        rows={(0, 1): (1.75, 1.25), (0, 2): (2.25, 1.75), (0, 3): (2.75, 2.25)})),
        "range_one_row": case(STAIRS, tolerance=1.0, rng=(2, 2),
                              want=dict(status=[CONVERGED], info=[[1, 1, 0, 5]], change=[0.25], rows={(0, 2): (2.25, 1.75)})),
        "range_clamped": case(STAIRS, tolerance=1.0, rng=(-5, 100),
                              want=dict(status=[CONVERGED], info=[[1, 1, 0, 5]], change=[0.25],
                                        rows={(0, 1): (1.75, 1.25), (0, 2): (2.25, 1.75), (0, 3): (2.75, 2.25)})),
        "range_first_above_last": case(STAIRS, rng=(3, 2), want=short(5)),
        "range_outside_the_rows": case(STAIRS, rng=(4, 9), want=short(5)),
    }
    # two robots with a map each: the second one's candidate cell is lethal
    a, b = out["n3_corner_one_sweep"], out["rejected_by_a_lethal_cell"]
    out["a_map_each"] = dict(a, plan=np.concatenate([a["plan"], b["plan"]]), plan_len=np.array([3, 3], np.int32), max_its=1,
                             world=np.stack([a["world"], b["world"]]), origin=np.zeros((2, 2)),
                             want=dict(status=[MAX_ITS, CONVERGED], info=[[1, 1, 0, 3], [1, 1, 1, 3]], change=[0.25, 0.0], rows={(0, 1): (1.75, 1.25)}))
    return out


def check_want(c, got):
    """got (plan, status, info, change) is what the case's want says, and every row it does not name came back bit for bit."""
    w = c["want"]
    assert got["status"].tolist() == w["status"], (got["status"], w["status"])
    assert got["info"].tolist() == w["info"], (got["info"], w["info"])
    assert got["change"].tobytes() == np.array(w["change"], np.float64).tobytes(), (got["change"], w["change"])
    want = np.array(c["plan"], np.float64)
    for (b, i), xy in w["rows"].items():
        want[b, i] = xy
    assert got["plan"].tobytes() == want.tobytes(), (got["plan"], want)


# ---- the staircase of the issue ---------------------------------------------------------------------------------------------
ZIGZAG_BLOCKED = [(31, 6), (32, 6), (33, 6), (34, 6), (35, 6)]      # on the inside of the first corner, (35, 5)


def zigzag_case(blocked=(), **kw):
    """91 poses at the centres of 0.05 m cells from cell (5, 5): 30 cells east, 20 north-east, 40 alternating east / north-east,
    on a free 110 x 60 world (blocked: cells set to 254). PlanSmootherParams' defaults."""
    res = 0.05
    steps = [(1, 0)] * 30 + [(1, 1)] * 20 + [(1, 0), (1, 1)] * 20
    cells = np.cumsum([(5, 5)] + steps, axis=0)
    assert cells.shape == (91, 2)
    rows = (cells + 0.5) * res
    world = np.zeros((60, 110), np.uint8)
    for x, y in blocked:
        world[y, x] = 254
    args = dict(L=128, world=world, res=res, w_data=0.2, w_smooth=0.3, tolerance=1e-10, max_its=1000, refinement_num=2)
    args.update(kw)
    return dict(case(rows, **args), cells=cells)


# ---- seeded cases -----------------------------------------------------------------------------------------------------------
NS = (3, 4, 63, 64, 65, 66, 127, 128, 129, 447, 448, 449, 1023, 1024)
LS = (448, 1024)                     # the two slot counts of the kernel
WORLD_X, WORLD_Y, RES = 96, 64, 0.05


def disc_world(rng):
    """96 x 64 cells: discs of lethal cells with a ring of lower costs, and a few unknown cells."""
    yy, xx = np.mgrid[0:WORLD_Y, 0:WORLD_X]
    world = np.zeros((WORLD_Y, WORLD_X), np.uint8)
    for _ in range(9):
        cx, cy, r = rng.uniform(4, WORLD_X - 4), rng.uniform(4, WORLD_Y - 4), rng.uniform(1.5, 5.0)
        d = np.hypot(xx - cx, yy - cy)
        world = np.maximum(world, np.where(d <= r, 254, np.where(d <= r + 3, (252 * (1 - (d - r) / 3)).astype(np.int64), 0)).astype(np.uint8))
    world[rng.integers(0, WORLD_Y, 12), rng.integers(0, WORLD_X, 12)] = 255
    return world


def grid_walk(rng, n, origin):
    """n rows: a point in a random start cell, then the centres of an 8-connected walk that keeps a heading for a while, turns
    by 45 degrees or starts to alternate, and turns away from the border; it does not look at the costs."""
    dirs = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
    x, y, h = int(rng.integers(2, WORLD_X - 2)), int(rng.integers(2, WORLD_Y - 2)), int(rng.integers(0, 8))
    rows = [(origin[0] + (x + rng.uniform(0.1, 0.9)) * RES, origin[1] + (y + rng.uniform(0.1, 0.9)) * RES)]
    run, zig = 0, False
    while len(rows) < n:
        if run == 0:
            h, run, zig = (h + int(rng.integers(-1, 2))) % 8, int(rng.integers(2, 24)), bool(rng.integers(0, 3) == 0)
        k = (h + (run & 1)) % 8 if zig else h
        nx, ny = x + dirs[k][0], y + dirs[k][1]
        if not (1 <= nx < WORLD_X - 1 and 1 <= ny < WORLD_Y - 1):
            h, run = (h + 3) % 8, 0
            continue
        x, y, run = nx, ny, run - 1
        rows.append((origin[0] + (x + 0.5) * RES, origin[1] + (y + 0.5) * RES))
    return np.array(rows[:n], np.float64)


def seeded_name(B, L, shared, seed):
    return f"B{B}_L{L}_{'shared' if shared else 'own'}_s{seed}"


def seeded_case(B, L, shared, seed, ns=None):
    """B robots with plans of L rows; ns: their lengths (default: drawn from NS, those that fit L). Rows behind a plan hold a
    sentinel pattern that differs from row to row. Even robots of a batch get a range."""
    rng = np.random.default_rng(seed)
    fit = [n for n in NS if n <= L]
    ns = [fit[int(rng.integers(0, len(fit)))] for _ in range(B)] if ns is None else list(ns)
    worlds = np.stack([disc_world(rng) for _ in range(1 if shared else B)])
    origins = np.stack([(-1.0 + rng.uniform(-0.3, 0.3), -0.7 + rng.uniform(-0.3, 0.3)) for _ in range(1 if shared else B)])
    plan = np.empty((B, L, 2), np.float64)
    plan[...] = -1000.0 - np.arange(B * L * 2, dtype=np.float64).reshape(B, L, 2) / 8.0
    for b, n in enumerate(ns):
        plan[b, :n] = grid_walk(rng, n, origins[0 if shared else b])
    rng_rows = None
    if B > 1:
        rng_rows = np.array([(1, n) if b % 2 else (int(rng.integers(-2, max(n // 3, 1))), int(rng.integers(n // 2, n + 3))) for b, n in enumerate(ns)], np.int32)
    return dict(plan=plan, plan_len=np.array(ns, np.int32), range=rng_rows, world=worlds[0] if shared else worlds,
                origin=origins[0] if shared else origins, res=RES, w_data=0.2, w_smooth=0.3, tolerance=3e-5, max_its=20, refinement_num=2,
                lethal_min_cost=253, allow_unknown=bool(seed & 1), want=None)


def seeded_cases():
    """Every n of NS alone (B = 1) at every L it fits, on a shared map; batches of 13 at both L on a shared map and on a map
    each, their lengths covering NS."""
    out = {}
    for L in LS:
        for j, n in enumerate(n for n in NS if n <= L):
            out[f"n{n}_L{L}"] = seeded_case(1, L, True, 100 + 17 * j + L, ns=[n])
    fit = [n for n in NS if n <= 448]
    out[seeded_name(13, 448, True, 3)] = seeded_case(13, 448, True, 3, ns=fit + [200, 391])
    out[seeded_name(13, 448, False, 4)] = seeded_case(13, 448, False, 4, ns=fit[::-1] + [17, 300])
    out[seeded_name(13, 1024, True, 5)] = seeded_case(13, 1024, True, 5, ns=list(NS[1:]))
    out[seeded_name(13, 1024, False, 6)] = seeded_case(13, 1024, False, 6, ns=list(NS[:-1])[::-1])
    return out
