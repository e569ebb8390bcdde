"""The contract of smpc_repair_plan_batch (include/smpc_plan_repair.h) as plain Python: a sequential yardstick written from the
header's text, not from csrc/smpc_plan_repair_rule.hpp, which is checked against it. A heapq Dijkstra for the region's field
(no pruning: the mask of rule 10 is applied at the end), a plain loop for everything else, numpy.float64 with one operation
per line, cell / centre / weights / steps of tests/global_plan_ref.py. check_fixed_point() is a second, independent check of
a field: every value that is not masked satisfies the Bellman equation of the rule on the region."""
import heapq

import numpy as np

import global_plan_ref as G

UNREACHABLE = G.UNREACHABLE
CLEAR, REPAIRED, NO_PLAN, NO_CELL, NO_REJOIN, UNREACHABLE_CELL, TOO_LONG, INCONSISTENT_FIELD = range(8)
STATUS = ["CLEAR", "REPAIRED", "NO_PLAN", "NO_CELL", "NO_REJOIN", "UNREACHABLE", "TOO_LONG", "INCONSISTENT_FIELD"]
MAX_RADIUS = 63


def d2(p, q):
    """(px - qx) * (px - qx) + (py - qy) * (py - qy): two products and one sum, every operation rounded on its own."""
    with np.errstate(all="ignore"):
        dx = np.float64(p[0]) - np.float64(q[0])
        dy = np.float64(p[1]) - np.float64(q[1])
        a = dx * dx
        b = dy * dy
        return a + b


def region_weights(costmap, a, R, cost):
    """[S,S] int64, region coordinates (cell (fx, fy) is window cell a - (R, R) + (fx, fy)): w of the cells that exist and are
    passable, the robot's own cell whatever its cost; 0 elsewhere."""
    Hy, Hx = costmap.shape
    S = 2 * R + 1
    w = np.zeros((S, S), np.int64)
    passable = G.passable(costmap, cost)
    for fy in range(S):
        for fx in range(S):
            x, y = a[0] - R + fx, a[1] - R + fy
            if 0 <= x < Hx and 0 <= y < Hy and (passable[y, x] or (x, y) == tuple(a)):
                w[fy, fx] = cost.neutral_cost + cost.cost_weight * int(costmap[y, x])
    return w


def region_field(w, t):
    """[S,S] uint32: the least cost from every region cell to region cell t, unmasked. Dijkstra from t over the reversed
    steps: the step c -> n is allowed exactly when n -> c is, and costs what entering n costs."""
    S = w.shape[0]
    field = np.full((S, S), UNREACHABLE, np.uint32)
    dist = {tuple(t): 0}
    heap = [(0, t[0], t[1])]
    done = set()
    while heap:
        d, x, y = heapq.heappop(heap)
        if (x, y) in done:
            continue
        done.add((x, y))
        for k, nx, ny, _ in G.steps_from(w, x, y):
            if (nx, ny) in done:
                continue
            nd = d + (5 if k < 4 else 7) * int(w[y, x])
            if nd < dist.get((nx, ny), UNREACHABLE):
                dist[(nx, ny)] = nd
                heapq.heappush(heap, (nd, nx, ny))
    for (x, y), d in dist.items():
        field[y, x] = d
    return field


def check_fixed_point(field, w, t, fa):
    """Is every value of the masked `field` the Bellman fixed point? For every cell with a value: 0 at t and nowhere else below
    its steps; otherwise the minimum over its allowed steps of F(n) + cost(n), where a masked neighbour counts as above fa.
    For every masked cell that exists: no step gives a value <= fa. Returns the number of cells with a value."""
    S = w.shape[0]
    valued = 0
    for y in range(S):
        for x in range(S):
            v = int(field[y, x])
            if w[y, x] == 0:
                assert v == UNREACHABLE, (x, y)
                continue
            cands = [int(field[ny, nx]) + c for _, nx, ny, c in G.steps_from(w, x, y) if field[ny, nx] != UNREACHABLE]
            best = min(cands, default=None)
            if (x, y) == tuple(t):
                assert v == 0
                valued += 1
            elif v != UNREACHABLE:
                assert best == v and v <= fa, (x, y, v, best)
                valued += 1
            else:
                assert best is None or best > fa, (x, y, best, fa)
    return valued


def repair_one(costmap, origin, resolution, pose_xy, plan, n, s, L, R, stride, clearance_d2, cost):
    """One robot by the header's rules 1 to 10. Returns dict(status, info [4], rows (the new plan rows, or None), field ([S,S]
    masked, or None before rule 6), cells (the walk, or None), F (the unmasked field, or None), w, t)."""
    out = dict(status=None, info=[-1, -1, -1, -1], rows=None, field=None, cells=None, F=None, w=None, t=None)
    costmap = np.asarray(costmap, np.uint8)
    Hy, Hx = costmap.shape
    x, y = np.float64(pose_xy[0]), np.float64(pose_xy[1])
    # 1
    if n < 2 or n > L or s < 0 or s >= n:
        out["status"] = NO_PLAN
        return out
    # 2
    a = G.cell_of((x, y), origin, resolution, Hx, Hy)
    if a is None:
        out["status"] = NO_CELL
        return out

    def region_cell(p):
        c = G.cell_of(p, origin, resolution, Hx, Hy)
        if c is None or max(abs(c[0] - a[0]), abs(c[1] - a[1])) > R:
            return None
        return c

    # 3
    i0, best = None, None
    for i in range(s, n):
        d = d2(plan[i], (x, y))
        if np.isfinite(d) and (best is None or d < best):
            i0, best = i, d
    if i0 is None:
        out["status"] = NO_PLAN
        return out
    out["info"][0] = i0
    # 4
    e = n
    for i in range(i0, n):
        if region_cell(plan[i]) is None:
            e = i
            break
    passable = G.passable(costmap, cost)
    blocked = []
    for i in range(i0, e):
        c = region_cell(plan[i])
        if not passable[c[1], c[0]] and c != a:
            blocked.append(i)
    if not blocked:
        out["status"] = CLEAR
        return out
    i1, i2 = blocked[0], blocked[-1]
    out["info"][1] = i1
    # 5
    j = None
    for i in range(i2 + 1, e):
        c = region_cell(plan[i])
        if passable[c[1], c[0]] and d2(plan[i], plan[i2]) >= np.float64(clearance_d2):
            j = i
            break
    if j is None:
        out["status"] = NO_REJOIN
        return out
    out["info"][2] = j
    tw = region_cell(plan[j])
    # 6
    w = region_weights(costmap, a, R, cost)
    t = (tw[0] - a[0] + R, tw[1] - a[1] + R)
    F = region_field(w, t)
    fa = int(F[R, R])
    out["F"], out["w"], out["t"] = F, w, t
    out["field"] = np.where(F <= fa, F, np.uint32(UNREACHABLE)).astype(np.uint32)
    if fa == UNREACHABLE:
        out["status"] = UNREACHABLE_CELL
        return out
    # 7
    cx, cy = R, R
    cells = [(cx, cy)]
    while F[cy, cx] != 0:
        here = int(F[cy, cx])
        nxt = None
        for k, nx, ny, c in G.steps_from(w, cx, cy):
            if F[ny, nx] != UNREACHABLE and int(F[ny, nx]) + c == here:
                nxt = (nx, ny)
                break
        if nxt is None or len(cells) - 1 >= w.size:
            out["status"] = INCONSISTENT_FIELD
            return out
        cx, cy = nxt
        cells.append(nxt)
    m = len(cells) - 1
    out["info"][3] = m
    out["cells"] = [(a[0] - R + fx, a[1] - R + fy) for fx, fy in cells]
    # 8
    rows = [np.array(plan[i], np.float64) for i in range(i0)] + [np.array([x, y])]
    rows += [G.centre_of(out["cells"][k], origin, resolution) for k in range(stride, m, stride)]
    rows += [np.array(plan[i], np.float64) for i in range(j, n)]
    if len(rows) > L:
        out["status"] = TOO_LONG
        return out
    out["status"], out["rows"] = REPAIRED, np.array(rows)
    return out


def run(case, plan=None, field=None, info=None, details=None):
    """A whole batch: case = dict(costmap [Hy,Hx] (shared) or [B,Hy,Hx], origin [2] or [B,2], res, pose [B,3], plan [B,L,2],
    plan_len [B], plan_start [B] or None, R, stride, clearance_d2, cost). `field` / `info`: the arrays before the call (default
    0 / -99; None output when given as False). Returns dict(plan, plan_len, status, info, field); details: a list that
    receives every robot's repair_one result."""
    costmap, origin = np.asarray(case["costmap"], np.uint8), np.asarray(case["origin"], np.float64)
    pose = np.asarray(case["pose"], np.float64)
    B, L = pose.shape[0], case["plan"].shape[1]
    R, S = case["R"], 2 * case["R"] + 1
    new_plan = np.array(case["plan"] if plan is None else plan, np.float64)
    plan_len = np.array(case["plan_len"], np.int32)
    status = np.zeros(B, np.int32)
    info = None if info is False else (np.full((B, 4), -99, np.int32) if info is None else np.array(info, np.int32))
    field = None if field is False else (np.zeros((B, S, S), np.uint32) if field is None else np.array(field, np.uint32))
    for b in range(B):
        s = 0 if case.get("plan_start") is None else int(case["plan_start"][b])
        r = repair_one(costmap if costmap.ndim == 2 else costmap[b], origin if origin.ndim == 1 else origin[b], case["res"], pose[b, :2],
                       case["plan"][b], int(case["plan_len"][b]), s, L, R, case["stride"], case["clearance_d2"], case["cost"])
        status[b] = r["status"]
        if info is not None:
            info[b] = r["info"]
        if field is not None and r["field"] is not None:
            field[b] = r["field"]
        if r["status"] == REPAIRED:
            new_plan[b, :len(r["rows"])] = r["rows"]
            plan_len[b] = len(r["rows"])
        if details is not None:
            details.append(r)
    return dict(plan=new_plan, plan_len=plan_len, status=status, info=info, field=field)


def same(got, want, keys=("plan", "plan_len", "status", "info", "field")):
    """Equal shapes, dtypes and bytes of the named outputs (None equals None)."""
    for k in keys:
        if (got[k] is None) != (want[k] is None):
            return False
        if got[k] is not None and not G.same_bits(got[k], want[k]):
            return False
    return True
