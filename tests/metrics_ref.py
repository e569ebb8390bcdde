"""CPU statement of smpc_episode_metrics_batch (include/smpc.h): a plain numpy loop, one robot and one sample at a time,
that follows the rules of the header in their order. The social force is restated from the reference's computeSocialForce
(critics/social_work_cost_function.hpp:164-228) with the two conventions of the device code (csrc/smpc_social_force.hpp): a
pair closer than 1e-6 m takes diff = (1e-6, 0), and exactly equal velocities take theta = 0.

A helper module for tests/test_metrics.py, tests/test_gpu_metrics.py and tests/test_gpu_episode_metrics.py; it also
holds the comparison at the tolerances those tests share, and the inspection of a sample's margins (how far every
comparison of the rules is from flipping)."""
import math

import numpy as np

COLS = ["samples", "path_length", "heading_change", "sum_speed", "people_samples", "min_person_dist", "sum_min_person_dist",
        "intimate_samples", "personal_samples", "social_samples", "person_collision_samples", "social_work", "min_clearance",
        "obstacle_collision_samples", "off_grid_samples", "time_to_goal", "goal_dist", "fallback_samples", "unusable_solves",
        "last_x", "last_y", "last_yaw", "reserved0", "reserved1"]
I = {name: i for i, name in enumerate(COLS)}
NCOLS = 24
LAMBDA, GAMMA, NPRIME, NN, FORCE_FACTOR = 2.0, 0.35, 3.0, 2.0, 2.1   # src/critics/social_work_cost_function.cpp:38-43

# How the columns are compared with the device's (compare(), below).
#   exact: counters; values copied from the inputs (last_*, min_clearance: a float widened to double); sums and
#     differences the device forms with the very same IEEE operations in the same order (sum_speed, heading_change: one
#     subtraction, additions of +-2 pi, fabs; time_to_goal: one multiplication) — no product feeds an addition there, so
#     fused multiply-adds cannot change them.
#   length: a square root of a sum of two products and a short sum of those: 1e-12 relative, a few ulp with room for the
#     compiler's contraction of dx * dx + dy * dy into one fma.
#   social_work: |got - want| / max(1, |want|) <= 1e-9, the project's gate for this force arithmetic in the sweep.
LENGTH_COLS = ("path_length", "min_person_dist", "sum_min_person_dist", "goal_dist")
WORK_COLS = ("social_work",)
EXACT_COLS = tuple(c for c in COLS if c not in LENGTH_COLS + WORK_COLS)
LENGTH_RTOL, WORK_TOL = 1e-12, 1e-9


def wrap_to_pi(a):
    """critics/social_work_cost_function.hpp:39-46: into (-pi, pi]."""
    while a > math.pi:
        a -= 2.0 * math.pi
    while a <= -math.pi:
        a += 2.0 * math.pi
    return a


def social_force(me_pos, me_vel, other_pos, other_vel):
    """computeSocialForce for one other agent: the force on `me`; also returns theta (for the margins)."""
    dx, dy = me_pos[0] - other_pos[0], me_pos[1] - other_pos[1]
    if math.sqrt(dx * dx + dy * dy) < 1e-6:
        dx, dy = 1e-6, 0.0
    dist = math.sqrt(dx * dx + dy * dy)
    ex, ey = dx / dist, dy / dist
    ux, uy = me_vel[0] - other_vel[0], me_vel[1] - other_vel[1]
    ivx, ivy = LAMBDA * ux + ex, LAMBDA * uy + ey
    il = math.sqrt(ivx * ivx + ivy * ivy)
    ix, iy = ivx / il, ivy / il
    if ux == 0.0 and uy == 0.0:
        theta = 0.0
    else:
        theta = wrap_to_pi(math.atan2(ey, ex) - math.atan2(iy, ix))
    B = GAMMA * il
    fv = -math.exp(-dist / B - (NPRIME * B * theta) ** 2)
    sign = 1.0 if theta > 0 else -1.0
    fa = -sign * math.exp(-dist / B - (NN * B * theta) ** 2)
    return np.array([FORCE_FACTOR * (fv * ix + fa * -iy), FORCE_FACTOR * (fv * iy + fa * ix)]), theta


def empty_row():
    row = np.zeros(NCOLS)
    row[I["min_person_dist"]] = row[I["min_clearance"]] = np.inf
    row[I["time_to_goal"]] = -1.0
    return row


def cell_of(x, y, origin, resolution):
    res = float(np.float32(resolution))
    return math.floor((x - origin[0]) / res), math.floor((y - origin[1]) / res)


def update_row(row, mp, dt, pose, twist, people, count, goal=None, dist_grid=None, origin=None, resolution=None, status=None,
               source=None):
    """One sample of one robot: returns the new row (the old one is left alone). mp: MetricsParams; pose (x, y, yaw);
    twist (v, w); people [Np,5]; dist_grid [h,w] float32 with origin (2,) and resolution, or None."""
    row = np.array(row, np.float64)
    if row[I["samples"]] == 0.0:
        row = empty_row()
    elif row[I["time_to_goal"]] >= 0.0:
        return row
    x, y, yaw = (float(v) for v in pose)
    v = float(twist[0])
    if row[I["samples"]] > 0:
        mx, my = x - row[I["last_x"]], y - row[I["last_y"]]
        row[I["path_length"]] += math.sqrt(mx * mx + my * my)
        row[I["heading_change"]] += abs(wrap_to_pi(yaw - row[I["last_yaw"]]))
    row[I["sum_speed"]] += v
    count = int(count)
    if count > 0:
        dmin = min(math.sqrt((x - people[i][0]) ** 2 + (y - people[i][1]) ** 2) for i in range(count))
        row[I["people_samples"]] += 1
        row[I["min_person_dist"]] = min(row[I["min_person_dist"]], dmin)
        row[I["sum_min_person_dist"]] += dmin
        row[I["intimate_samples"]] += dmin < mp.intimate_radius
        row[I["personal_samples"]] += dmin < mp.personal_radius
        row[I["social_samples"]] += dmin < mp.social_radius
        row[I["person_collision_samples"]] += dmin < mp.robot_radius + mp.person_radius
    rvel = (v * math.cos(yaw), v * math.sin(yaw))
    on_robot, wp = np.zeros(2), 0.0
    for i in range(count):
        ppos, pvel = (people[i][0], people[i][1]), (people[i][2], people[i][3])
        on_robot += social_force((x, y), rvel, ppos, pvel)[0]
        on_person = social_force(ppos, pvel, (x, y), rvel)[0]   # from the robot alone
        wp += float(on_person @ on_person)
    row[I["social_work"]] += float(on_robot @ on_robot) + wp
    if dist_grid is not None:
        cx, cy = cell_of(x, y, origin, resolution)
        h, w = dist_grid.shape
        if 0 <= cx < w and 0 <= cy < h:
            c = float(dist_grid[cy, cx])
            row[I["min_clearance"]] = min(row[I["min_clearance"]], c)
            row[I["obstacle_collision_samples"]] += c < mp.robot_radius
        else:
            row[I["off_grid_samples"]] += 1
    if source is not None:
        row[I["fallback_samples"]] += int(source) != 0
    if status is not None:
        row[I["unusable_solves"]] += int(status) not in (0, 1)   # SMPC_CONVERGENCE, SMPC_NO_CONVERGENCE
    row[I["last_x"]], row[I["last_y"]], row[I["last_yaw"]] = x, y, yaw
    row[I["samples"]] += 1
    if goal is not None:
        gx, gy = x - goal[0], y - goal[1]
        gd = math.sqrt(gx * gx + gy * gy)
        row[I["goal_dist"]] = gd
        if gd <= mp.goal_tolerance:
            row[I["time_to_goal"]] = row[I["samples"]] * dt
    return row


def update(acc, mp, dt, pose, twist, people, count, goal=None, od_distances=None, od_origin=None, od_resolution=None,
           status=None, source=None):
    """One sample of B robots (the arguments of BatchSolver.episode_metrics): returns the new acc [B,24]."""
    acc = np.asarray(acc, np.float64)
    out = np.empty_like(acc)
    shared = od_distances is not None and np.ndim(od_distances) == 2
    for b in range(acc.shape[0]):
        grid = origin = None
        if od_distances is not None:
            grid = od_distances if shared else od_distances[b]
            origin = np.reshape(od_origin, (-1, 2))[0 if shared else b]
        out[b] = update_row(acc[b], mp, dt, pose[b], twist[b], people[b], count[b], None if goal is None else goal[b], grid,
                            origin, od_resolution, None if status is None else status[b], None if source is None else source[b])
    return out


def margins(mp, pose, people, count, goal=None, dist_grid=None, origin=None, resolution=None):
    """How far one robot's sample is from every decision of the rules: dict(theta: min over the pairs of min(|theta|,
    pi - |theta|); pair: smallest pair distance; edge: distance of the position to the nearest cell edge of the grid;
    threshold: smallest |value - threshold| over dmin against the four radii, the clearance against robot_radius and the
    goal distance against goal_tolerance). Entries that do not apply are +inf."""
    x, y, yaw = (float(v) for v in pose)
    m = {"theta": np.inf, "pair": np.inf, "edge": np.inf, "threshold": np.inf}
    count = int(count)
    ds = []
    for i in range(count):
        ds.append(math.hypot(x - people[i][0], y - people[i][1]))
    if count:
        dmin = min(ds)
        m["pair"] = dmin
        for r in (mp.intimate_radius, mp.personal_radius, mp.social_radius, mp.robot_radius + mp.person_radius):
            m["threshold"] = min(m["threshold"], abs(dmin - r))
    if dist_grid is not None:
        res = float(np.float32(resolution))
        for val in ((x - origin[0]) / res, (y - origin[1]) / res):
            m["edge"] = min(m["edge"], abs(val - round(val)) * res)
        cx, cy = cell_of(x, y, origin, resolution)
        h, w = dist_grid.shape
        if 0 <= cx < w and 0 <= cy < h:
            m["threshold"] = min(m["threshold"], abs(float(dist_grid[cy, cx]) - mp.robot_radius))
    if goal is not None:
        m["threshold"] = min(m["threshold"], abs(math.hypot(x - goal[0], y - goal[1]) - mp.goal_tolerance))
    return m


def theta_margin(pose, twist, people, count):
    """min over a robot's pairs of min(|theta|, pi - |theta|) (+inf without persons), both directions of every pair."""
    x, y, yaw = (float(v) for v in pose)
    rvel = (twist[0] * math.cos(yaw), twist[0] * math.sin(yaw))
    out = np.inf
    for i in range(int(count)):
        ppos, pvel = (people[i][0], people[i][1]), (people[i][2], people[i][3])
        for th in (social_force((x, y), rvel, ppos, pvel)[1], social_force(ppos, pvel, (x, y), rvel)[1]):
            out = min(out, abs(th), math.pi - abs(th))
    return out


def compare(got, want, what=""):
    """Asserts got == want at the tolerances of the column classes above; prints the largest deviation of each class
    first."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst = {}
    for c in LENGTH_COLS:
        g, w = got[:, I[c]], want[:, I[c]]
        fin = np.isfinite(w)
        assert np.array_equal(g[~fin], w[~fin]), (what, c)
        rel = np.abs(g[fin] - w[fin]) / np.maximum(np.abs(w[fin]), np.finfo(float).tiny)
        rel = np.where(g[fin] == w[fin], 0.0, rel)
        worst[c] = float(rel.max()) if rel.size else 0.0
    g, w = got[:, I["social_work"]], want[:, I["social_work"]]
    worst["social_work"] = float((np.abs(g - w) / np.maximum(1.0, np.abs(w))).max())
    print(f"metrics {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for c in EXACT_COLS:
        assert np.array_equal(got[:, I[c]], want[:, I[c]]), (what, c, got[:, I[c]], want[:, I[c]])
    for c in LENGTH_COLS:
        assert worst[c] <= LENGTH_RTOL, (what, c, worst[c])
    assert worst["social_work"] <= WORK_TOL, (what, worst["social_work"])
