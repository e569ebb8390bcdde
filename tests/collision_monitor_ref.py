"""The sequential yardstick of the collision monitor (include/smpc_collision_monitor.h states the rule): one robot after the
other, one point after the other, one zone after the other and every step 0..M of every zone, numpy float64 scalars with one
operation per line; no early exit, no reach filter, nothing shared between zones. The cosines and sines of the heading and of
the simulation step's angle are handed in (step 2 of the rule: everything behind them is a pure function of the four), so a
caller compares bit for bit given what a device or a compiled rule obtained, and holds those against numpy's separately
(angles_close).

p = params(...): the call's scalars and its zones; pose [B,3], cmd [B,2], kind [B,n] uint8, cell [B,n,2] int32."""
import numpy as np

F = np.float64
CIRCLE, POLYGON = 0, 1
STOP, SLOWDOWN, LIMIT, APPROACH = 0, 1, 2, 3
FLAG_BAD_INPUT, FLAG_NO_CELL = 16, 32
KIND_NONE, KIND_WORLD, KIND_AGENT, KIND_CORNER_PAIR, KIND_INVALID, KIND_NO_ROBOT = 0, 1, 2, 3, 4, 5
HEADING_ATOL = 2.3e-16     # plant_ref.HEADING_ATOL: the bound tests/test_math.py holds sincos_tab to, 1 ulp of 1


def circle(action, radius, min_points=1, slowdown_ratio=0.5, linear_limit=0.5, angular_limit=0.5):
    return dict(shape=CIRCLE, action=int(action), n=0, min_points=int(min_points), radius=F(radius), slowdown_ratio=F(slowdown_ratio),
                linear_limit=F(linear_limit), angular_limit=F(angular_limit), vertices=np.zeros((0, 2)))


def polygon(action, vertices, min_points=1, slowdown_ratio=0.5, linear_limit=0.5, angular_limit=0.5):
    v = np.array(vertices, F).reshape(-1, 2)
    return dict(shape=POLYGON, action=int(action), n=len(v), min_points=int(min_points), radius=F(0.0), slowdown_ratio=F(slowdown_ratio),
                linear_limit=F(linear_limit), angular_limit=F(angular_limit), vertices=v)


def params(zones, M=0, sim_dt=0.1, res=0.125, origin=(0.0, 0.0)):
    return dict(zones=list(zones), M=int(M), sim_dt=F(sim_dt), res=F(res), origin=(F(origin[0]), F(origin[1])))


def robot_cell(p, x, y):
    """The robot's cell (ax, ay) as ints, or None."""
    dx = x - p["origin"][0]
    dy = y - p["origin"][1]
    qx = np.floor(dx / p["res"])
    qy = np.floor(dy / p["res"])
    if not (np.isfinite(x) and np.isfinite(y)):
        return None
    if not (abs(qx) <= 2.0 ** 30 and abs(qy) <= 2.0 ** 30):
        return None
    return int(qx), int(qy)


def rel(origin, a, off, res, x):
    i = F(int(a) + int(off))
    h = i + F(0.5)
    m = h * res
    centre = origin + m
    return centre - x


def to_frame(c, s, rx, ry):
    a = c * rx
    b = s * ry
    d = c * ry
    e = s * rx
    return a + b, d - e


def points_of(p, x, y, c, s, kind, cell):
    """The robot's points in its frame, in beam order: [(px, py)], and whether it has a cell."""
    a = robot_cell(p, x, y)
    if a is None:
        return [], False
    out = []
    for k in range(len(kind)):
        if int(kind[k]) not in (KIND_WORLD, KIND_AGENT, KIND_CORNER_PAIR):
            continue
        rx = rel(p["origin"][0], a[0], cell[k, 0], p["res"], x)
        ry = rel(p["origin"][1], a[1], cell[k, 1], p["res"], y)
        out.append(to_frame(c, s, rx, ry))
    return out, True


def inside(z, qx, qy):
    if z["shape"] == CIRCLE:
        xx = qx * qx
        yy = qy * qy
        r2 = z["radius"] * z["radius"]
        return bool(xx + yy < r2)
    n, V, par = z["n"], z["vertices"], False
    for i in range(n):
        j = (i + n - 1) % n
        vix, viy, vjx, vjy = F(V[i, 0]), F(V[i, 1]), F(V[j, 0]), F(V[j, 1])
        if (viy > qy) == (vjy > qy):
            continue
        dy = vjy - viy
        ex = vjx - vix
        ey = qy - viy
        fx = qx - vix
        a = ex * ey
        b = fx * dy
        t = a - b
        if (dy > 0.0 and t > 0.0) or (dy < 0.0 and t < 0.0):
            par = not par
    return par


def step_counts(p, z, pts, v, c1, s1, M):
    """[M + 1] the number of points inside zone z at every step 0..M of the simulated command."""
    counts = [sum(inside(z, px, py) for px, py in pts)]
    X, Y, C, S = F(0.0), F(0.0), F(1.0), F(0.0)
    for m in range(1, M + 1):
        vc = v * C
        vs = v * S
        ax = vc * p["sim_dt"]
        ay = vs * p["sim_dt"]
        X = X + ax
        Y = Y + ay
        cc = C * c1
        ss = S * s1
        sc = S * c1
        cs = C * s1
        C = cc - ss
        S = sc + cs
        n = 0
        for px, py in pts:
            dx = px - X
            dy = py - Y
            qx, qy = to_frame(C, S, dx, dy)
            n += inside(z, qx, qy)
        counts.append(n)
    return counts


def run(p, pose, cmd, kind, cell, cs, cs1=None):
    """Every robot by the rule. cs [B,2]: cosine and sine of every heading; cs1 [B,2]: of every w * sim_dt (read with M > 0);
    rows of robots with a pose or command that is not finite are not read. Returns {"cmd_out" [B,2], "action" [B,4] int32,
    "zone_points" [B,Z] int32, "ratio" [B], "finite" [B] bool (heading_cs / step_cs are written for these rows only),
    "zone_step" [B,Z] the collision step of every zone or -1, "zone_counts" [B,Z,M+1] the points inside at every step}."""
    pose, cmd = np.asarray(pose, F), np.asarray(cmd, F)
    kind, cell = np.asarray(kind), np.asarray(cell)
    B, Z, M = len(pose), len(p["zones"]), p["M"]
    out = dict(cmd_out=np.zeros((B, 2)), action=np.zeros((B, 4), np.int32), zone_points=np.zeros((B, Z), np.int32), ratio=np.zeros(B),
               finite=np.zeros(B, bool), zone_step=np.full((B, Z), -1), zone_counts=np.zeros((B, Z, M + 1), np.int64))
    with np.errstate(all="ignore"):
        for b in range(B):
            x, y, th, v, w = F(pose[b, 0]), F(pose[b, 1]), F(pose[b, 2]), F(cmd[b, 0]), F(cmd[b, 1])
            if not all(np.isfinite(a) for a in (x, y, th, v, w)):
                out["action"][b] = (FLAG_BAD_INPUT, -1, -1, 0)
                continue
            out["finite"][b] = True
            c, s = F(cs[b, 0]), F(cs[b, 1])
            c1, s1 = (F(cs1[b, 0]), F(cs1[b, 1])) if M > 0 else (F(1.0), F(0.0))
            pts, has_cell = points_of(p, x, y, c, s, kind[b], cell[b])
            best, decide, dstep, by = F(1.0), -1, -1, 0
            for zi, z in enumerate(p["zones"]):
                counts = step_counts(p, z, pts, v, c1, s1, M if z["action"] == APPROACH else 0)
                out["zone_counts"][b, zi, :len(counts)] = counts
                out["zone_points"][b, zi] = counts[0]
                hit = [m for m, n in enumerate(counts) if n >= z["min_points"]]
                step = hit[0] if hit else -1
                out["zone_step"][b, zi] = step
                ratio = F(1.0)
                if step >= 0:
                    if z["action"] == STOP:
                        ratio = F(0.0)
                    elif z["action"] == SLOWDOWN:
                        ratio = z["slowdown_ratio"]
                    elif z["action"] == LIMIT:
                        av, aw = abs(v), abs(w)
                        if av > z["linear_limit"]:
                            ratio = min(ratio, z["linear_limit"] / av)
                        if aw > z["angular_limit"]:
                            ratio = min(ratio, z["angular_limit"] / aw)
                    else:
                        ratio = F(step) / F(M)
                if ratio < best:
                    best, decide, dstep, by = ratio, zi, step, 1 << z["action"]
            if best == 1.0:
                out["cmd_out"][b] = (v, w)
            elif best == 0.0:
                out["cmd_out"][b] = (0.0, 0.0)
            else:
                out["cmd_out"][b] = (v * best, w * best)
            out["ratio"][b] = best
            out["action"][b] = (by | (0 if has_cell else FLAG_NO_CELL), decide, dstep, len(pts))
    return out


def numpy_angles(pose, cmd, sim_dt):
    """([B,2], [B,2]): cosine and sine of every heading and of every w * sim_dt by numpy."""
    with np.errstate(all="ignore"):
        th = np.asarray(pose, F)[:, 2]
        a = np.asarray(cmd, F)[:, 1] * F(sim_dt)
        return np.stack([np.cos(th), np.sin(th)], axis=1), np.stack([np.cos(a), np.sin(a)], axis=1)


def angles_close(cs, cs1, pose, cmd, sim_dt, M):
    """Is every (c, s) and, with M > 0, every (c1, s1) of a robot whose pose and command are finite within HEADING_ATOL of
    numpy's? The rows of the other robots are not looked at."""
    ok = np.isfinite(np.asarray(pose, F)).all(axis=1) & np.isfinite(np.asarray(cmd, F)).all(axis=1)
    want, want1 = numpy_angles(pose, cmd, sim_dt)
    good = bool((np.abs(np.asarray(cs)[ok] - want[ok]) <= HEADING_ATOL).all())
    if M > 0:
        good = good and bool((np.abs(np.asarray(cs1)[ok] - want1[ok]) <= HEADING_ATOL).all())
    return good


def same(got, want, keys=("cmd_out", "action", "zone_points", "ratio")):
    """Bit for bit on the call's outputs (a -0.0 is not a +0.0)."""
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
            return False
    return True
