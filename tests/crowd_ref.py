"""CPU checker of smpc_crowd_step_batch, written from the contract in include/smpc.h: a plain loop over one robot, one
person and one partner at a time with libm exp / atan2 and none of the library's code. TEST INFRASTRUCTURE ONLY.

step() advances one robot's persons, step_batch() a batch; both return new arrays and leave their inputs alone.
margins() reports how far one robot's step stays from every decision the rules take (see tests/test_crowd.py)."""
import math

import numpy as np

F_DESIRED, RELAX, F_OBSTACLE, SIGMA, F_SOCIAL, LAMBDA, GAMMA, N_, NPRIME = 2.0, 0.5, 20.0, 0.2, 2.1, 2.0, 0.35, 2.0, 3.0
TOL = 1e-9   # positions, velocities and vz * dt of the device against this checker (absolute)


def wrap(a):
    """into (-pi, pi]; non-finite values pass through"""
    if not math.isfinite(a):
        return a
    while a <= -math.pi:
        a += 2.0 * math.pi
    while a > math.pi:
        a -= 2.0 * math.pi
    return a


def heading(vx, vy):
    return 0.0 if (vx == 0.0 and vy == 0.0) else wrap(math.atan2(vy, vx))


def pair_theta(dx, dy, ux, uy):
    """(theta, diff direction, interaction direction, |interaction|, |diff|) of one partner: diff = partner - me,
    u = my velocity - the partner's, with the two conventions of the contract."""
    if dx * dx + dy * dy < 1e-12:
        dx, dy = 1e-6, 0.0
    nd = math.sqrt(dx * dx + dy * dy)
    ex, ey = dx / nd, dy / nd
    ivx, ivy = LAMBDA * ux + ex, LAMBDA * uy + ey
    il = math.sqrt(ivx * ivx + ivy * ivy)
    ix, iy = ivx / il, ivy / il
    if LAMBDA * ux == 0.0 and LAMBDA * uy == 0.0:
        theta = 0.0
    else:
        theta = wrap(wrap(math.atan2(ey, ex)) - wrap(math.atan2(iy, ix)))
    return theta, (ex, ey), (ix, iy), il, nd


def social_term(dx, dy, ux, uy):
    theta, _, (ix, iy), il, nd = pair_theta(dx, dy, ux, uy)
    Bq = GAMMA * il
    fv = -math.exp(-nd / Bq - (NPRIME * Bq * theta) ** 2)
    sign = 0.0 if theta == 0.0 else (1.0 if theta > 0.0 else -1.0)
    fa = -sign * math.exp(-nd / Bq - (N_ * Bq * theta) ** 2)
    return F_SOCIAL * (fv * ix + fa * (-iy)), F_SOCIAL * (fv * iy + fa * ix)


def obstacle_of(px, py, idx, origin, res):
    """position of the nearest obstacle of the person's cell (computeObstacle's float arithmetic), or None"""
    if idx is None:
        return None
    h, w = idx.shape
    r32 = np.float32(res)
    cx, cy = (px - origin[0]) / float(r32), (py - origin[1]) / float(r32)
    if not (math.isfinite(cx) and math.isfinite(cy)):
        return None
    cx, cy = math.floor(cx), math.floor(cy)
    if not (0 <= cx < w and 0 <= cy < h):
        return None
    ob = int(idx[cy, cx])
    if ob >= w * h:
        return None
    oyc, oxc = ob // w, ob % w
    x = np.float32(float(np.float32(oxc) * r32) + origin[0])
    y = np.float32(float(np.float32(oyc) * r32) + origin[1])
    return float(x), float(y)


def step(dt, people, cursor, pose, twist, count, waypoints, n_waypoints, goal_radius=0.25, person_radius=0.35,
         desired_speed=0.6, cyclic=True, robot_visible=True, desired_speeds=None, od_indexes=None, od_origin=None,
         od_resolution=None, events=None):
    """One robot: people [Np,5], cursor [Np], pose [3], twist [2], waypoints [Np,K,2], n_waypoints [Np]; od_indexes [h,w].
    events: a dict that receives the counts of arrivals and wraps."""
    people, cursor = np.array(people, np.float64), np.array(cursor, np.int32)
    old = people.copy()
    K = waypoints.shape[1]
    rvx, rvy = twist[0] * math.cos(pose[2]), twist[0] * math.sin(pose[2])
    for i in range(int(count)):
        px, py, vx, vy = (float(v) for v in old[i, 0:4])
        des = float(desired_speed if desired_speeds is None else desired_speeds[i])
        nwp = min(max(int(n_waypoints[i]), 0), K)
        cur = int(cursor[i])
        has_goal = 0 <= cur < nwp
        fx, fy = -vx / RELAX, -vy / RELAX
        if has_goal:
            gx, gy = (float(v) for v in waypoints[i, cur])
            d = math.sqrt((gx - px) ** 2 + (gy - py) ** 2)
            if d > goal_radius:
                fx = F_DESIRED * ((gx - px) / d * des - vx) / RELAX
                fy = F_DESIRED * ((gy - py) / d * des - vy) / RELAX
        if robot_visible:
            sx, sy = social_term(pose[0] - px, pose[1] - py, vx - rvx, vy - rvy)
            fx, fy = fx + sx, fy + sy
        for j in range(int(count)):
            if j != i:
                sx, sy = social_term(old[j, 0] - px, old[j, 1] - py, vx - old[j, 2], vy - old[j, 3])
                fx, fy = fx + sx, fy + sy
        o = obstacle_of(px, py, od_indexes, od_origin, od_resolution)
        if o is not None:
            mx, my = px - o[0], py - o[1]
            m = math.sqrt(mx * mx + my * my)
            e = F_OBSTACLE * math.exp(-(m - person_radius) / SIGMA)
            if m > 0.0:
                fx, fy = fx + e * mx / m, fy + e * my / m
        nvx, nvy = vx + fx * dt, vy + fy * dt
        sp = math.sqrt(nvx * nvx + nvy * nvy)
        if sp > des:
            nvx, nvy = nvx / sp * des, nvy / sp * des
        vz = wrap(heading(nvx, nvy) - heading(vx, vy)) / dt
        px, py = px + nvx * dt, py + nvy * dt
        if has_goal and math.sqrt((gx - px) ** 2 + (gy - py) ** 2) <= goal_radius:
            cur += 1
            if events is not None:
                events["arrived"] = events.get("arrived", 0) + 1
                if cyclic and cur >= nwp:
                    events["wrapped"] = events.get("wrapped", 0) + 1
        if cyclic and cur >= nwp:
            cur = 0
        people[i] = [px, py, nvx, nvy, vz]
        cursor[i] = cur
    return people, cursor


def step_batch(dt, people, cursor, pose, twist, count, waypoints, n_waypoints, desired_speeds=None, od_indexes=None,
               od_origin=None, od_resolution=None, events=None, **kw):
    """Batch of robots; od_indexes [h,w] with od_origin [2] (shared) or [B,h,w] with [B,2]."""
    people, cursor = np.array(people, np.float64), np.array(cursor, np.int32)
    shared = od_indexes is not None and np.ndim(od_indexes) == 2
    for b in range(people.shape[0]):
        idx = None if od_indexes is None else (od_indexes if shared else od_indexes[b])
        org = None if od_indexes is None else (np.reshape(od_origin, (-1, 2))[0] if shared else od_origin[b])
        people[b], cursor[b] = step(dt, people[b], cursor[b], pose[b], twist[b], count[b], waypoints[b], n_waypoints[b],
                                    desired_speeds=None if desired_speeds is None else desired_speeds[b], od_indexes=idx,
                                    od_origin=org, od_resolution=od_resolution, events=events, **kw)
    return people, cursor


def margins(dt, people, cursor, pose, twist, count, waypoints, n_waypoints, robot_visible=True, od_indexes=None,
            od_origin=None, od_resolution=None, goal_radius=0.25, coincident_ok=False, **kw):
    """The least distances of one robot's step from the rules' decisions: theta (of a pair with unequal velocities, from 0
    and from +-pi), pair (metres between two partners; exactly coincident ones are left out with coincident_ok), goal (of a
    person's distance to its goal after the step from goal_radius), edge (of a person from the edges of its grid cell,
    before and after the step, in metres), speed (of a moving person, before and after the step)."""
    new, _ = step(dt, people, cursor, pose, twist, count, waypoints, n_waypoints, robot_visible=robot_visible,
                  od_indexes=od_indexes, od_origin=od_origin, od_resolution=od_resolution, goal_radius=goal_radius, **kw)
    m = dict(theta=math.inf, pair=math.inf, goal=math.inf, edge=math.inf, speed=math.inf)
    n = int(count)
    rvx, rvy = twist[0] * math.cos(pose[2]), twist[0] * math.sin(pose[2])
    partners = [(people[j, 0], people[j, 1], people[j, 2], people[j, 3]) for j in range(n)]
    for i in range(n):
        px, py, vx, vy = people[i, 0:4]
        for j, (qx, qy, wx, wy) in enumerate(partners + ([(pose[0], pose[1], rvx, rvy)] if robot_visible else [])):
            if j == i:
                continue
            d = math.hypot(qx - px, qy - py)
            if not (coincident_ok and d == 0.0):
                m["pair"] = min(m["pair"], d)
            if vx != wx or vy != wy:
                th = abs(pair_theta(qx - px, qy - py, vx - wx, vy - wy)[0])
                m["theta"] = min(m["theta"], th, abs(th - math.pi))
        cur = int(cursor[i])
        if 0 <= cur < min(max(int(n_waypoints[i]), 0), waypoints.shape[1]):
            g = waypoints[i, cur]
            m["goal"] = min(m["goal"], abs(math.hypot(g[0] - new[i, 0], g[1] - new[i, 1]) - goal_radius))
        for q in (people[i], new[i]):
            sp = math.hypot(q[2], q[3])
            if sp > 0.0:
                m["speed"] = min(m["speed"], sp)
            if od_indexes is not None:
                for c, o in ((q[0], od_origin[0]), (q[1], od_origin[1])):
                    t = (c - o) / float(np.float32(od_resolution))
                    m["edge"] = min(m["edge"], abs(t - round(t)) * float(np.float32(od_resolution)))
    return m


def compare(got_people, got_cursor, want_people, want_cursor, dt, count, what=""):
    """Positions, velocities and vz * dt (difference wrapped) within TOL, cursors equal; prints the largest differences."""
    gp, wp = np.asarray(got_people), np.asarray(want_people)
    live = np.arange(gp.shape[1])[None, :] < np.asarray(count)[:, None]
    d = np.abs(gp[..., 0:4] - wp[..., 0:4])[live]
    dz = (gp[..., 4] - wp[..., 4])[live] * dt
    dz = np.abs(np.arctan2(np.sin(dz), np.cos(dz)))
    worst = (float(d.max()) if d.size else 0.0, float(dz.max()) if dz.size else 0.0)
    print(f"{what}: max |d(p, v)| = {worst[0]:.3e}, max |d vz dt| = {worst[1]:.3e}")
    assert worst[0] <= TOL and worst[1] <= TOL, (what, worst)
    assert np.array_equal(np.asarray(got_cursor)[live], np.asarray(want_cursor)[live]), what
