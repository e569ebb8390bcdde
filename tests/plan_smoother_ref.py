"""The sequential yardstick of the plan smoothing, written from include/smpc_plan_smoother.h: numpy float64, one robot after the
other, every operation of the rule a numpy operation of its own (rounded once, no fused multiply-add), in the header's order.
A sweep is Jacobi, so forming all candidates of a sweep from the previous iterate at once is the rule itself, not a shortcut.
Nothing here is shared with the library's code."""
import numpy as np

CONVERGED, MAX_ITS, TOO_SHORT, BAD_PLAN = range(4)
STATUS = ["CONVERGED", "REACHED_MAX_ITS", "TOO_SHORT", "BAD_PLAN"]
INT32_MAX = 2 ** 31 - 1


def passable_cells(world, lethal_min_cost, allow_unknown):
    world = np.asarray(world, np.uint8)
    ok = world.astype(np.int64) < int(lethal_min_cost)
    if allow_unknown:
        ok |= world == 255
    return ok


def cell_axis(c, origin, res, size):
    """Per axis: floor((c - origin) / res); (cells as int64, which of them exist)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = c - np.float64(origin)
        q = np.floor(d / np.float64(res))
        ok = (q >= 0.0) & (q < np.float64(size))          # a NaN fails both
    return np.where(ok, q, 0.0).astype(np.int64), ok


def accepted_rows(cx, cy, ok_cells, origin, res):
    """Which candidates have a cell in the map and a passable one."""
    H, W = ok_cells.shape
    ix, okx = cell_axis(cx, origin[0], res, W)
    iy, oky = cell_axis(cy, origin[1], res, H)
    inside = okx & oky
    return inside & ok_cells[iy, ix]


def candidate(p, y, ym, yp, w_data, w_smooth):
    with np.errstate(invalid="ignore", over="ignore"):
        a = p - y
        b = w_data * a
        s = yp + ym
        d = y + y
        e = s - d
        f = w_smooth * e
        g = b + f
        return y + g


def smooth_one(rows, plan_len, world, origin, res, w_data, w_smooth, tolerance, max_its, refinement_num, lethal_min_cost, allow_unknown,
               rng=None, trace=None):
    """One robot. rows [L,2] are not modified. Returns (rows after, status, info (4), change). trace: a list that receives
    (sweeps so far, rows) after every sweep."""
    rows = np.array(rows, np.float64)
    L = rows.shape[0]
    n = min(max(int(plan_len), 0), L)
    w_data, w_smooth, tolerance = np.float64(w_data), np.float64(w_smooth), np.float64(tolerance)
    if not np.isfinite(rows[:n]).all():
        return rows, BAD_PLAN, (0, 0, 0, n), np.float64(0.0)
    first, last = 1, n - 2
    if rng is not None:
        first, last = max(int(rng[0]), 1), min(int(rng[1]), n - 2)
    if n < 3 or first > last:
        return rows, TOO_SHORT, (0, 0, 0, n), np.float64(0.0)
    ok_cells = passable_cells(world, lethal_min_cost, allow_unknown)
    y = rows[:n].copy()
    mv = slice(first, last + 1)
    sweeps = rounds = rejected = 0
    change = np.float64(0.0)
    status = CONVERGED
    for r in range(int(refinement_num) + 1):
        p = y.copy()
        converged = False
        for it in range(int(max_its)):
            cx = candidate(p[mv, 0], y[mv, 0], y[first - 1:last, 0], y[first + 1:last + 2, 0], w_data, w_smooth)
            cy = candidate(p[mv, 1], y[mv, 1], y[first - 1:last, 1], y[first + 1:last + 2, 1], w_data, w_smooth)
            acc = accepted_rows(cx, cy, ok_cells, origin, res)
            rejected += int((~acc).sum())
            change = np.float64(0.0)
            if acc.any():
                hx = np.abs(cx[acc] - y[mv, 0][acc])
                hy = np.abs(cy[acc] - y[mv, 1][acc])
                change = np.float64(max(hx.max(), hy.max()))
            new = y.copy()
            new[mv, 0] = np.where(acc, cx, y[mv, 0])
            new[mv, 1] = np.where(acc, cy, y[mv, 1])
            y = new
            sweeps += 1
            if trace is not None:
                trace.append((sweeps, y.copy()))
            if change <= tolerance:
                converged = True
                break
        rounds += 1
        if not converged:
            status = MAX_ITS
            break
    rows[:n] = y
    return rows, status, (sweeps, rounds, min(rejected, INT32_MAX), n), change


def run(c, info=None, change=None):
    """A case (tests/plan_smoother_cases.py) through the rule: dict(plan, status, info, change); info / change: the arrays
    before the call (default -99 / NaN: every robot's entries are written)."""
    B = c["plan"].shape[0]
    shared = c["world"].ndim == 2
    out = dict(plan=np.array(c["plan"], np.float64), status=np.zeros(B, np.int32),
               info=np.full((B, 4), -99, np.int32) if info is None else np.array(info, np.int32),
               change=np.full(B, np.nan) if change is None else np.array(change, np.float64))
    origin = np.asarray(c["origin"], np.float64).reshape(-1, 2)
    for b in range(B):
        rows, st, inf, ch = smooth_one(c["plan"][b], c["plan_len"][b], c["world"] if shared else c["world"][b], origin[0 if shared else b],
                                       c["res"], c["w_data"], c["w_smooth"], c["tolerance"], c["max_its"], c["refinement_num"],
                                       c["lethal_min_cost"], c["allow_unknown"], None if c["range"] is None else c["range"][b])
        out["plan"][b], out["status"][b], out["info"][b], out["change"][b] = rows, st, inf, ch
    return out


OUTPUTS = ("plan", "status", "info", "change")


def same(a, b, keys=OUTPUTS):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def turning(rows):
    """The summed absolute heading change of a polyline, radians; repeated points are skipped."""
    d = np.diff(np.asarray(rows, np.float64), axis=0)
    d = d[np.hypot(d[:, 0], d[:, 1]) > 0.0]
    th = np.arctan2(d[:, 1], d[:, 0])
    dth = np.diff(th)
    dth = (dth + np.pi) % (2.0 * np.pi) - np.pi
    return float(np.abs(dth).sum())
