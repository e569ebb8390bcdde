"""The seeded inputs of the crowd-step tests, shared by tests/test_crowd.py (which shows, with the checker alone, that
they stay clear of every decision the rules take) and tests/test_gpu_crowd.py (which runs them on the device)."""
import math

import numpy as np

import crowd_ref as R

SHAPES = [(1, 1), (3, 64), (65, 33), (130, 8)]
SEEDS = {(1, 1): 21, (3, 64): 22, (65, 33): 23, (130, 8): 24}
DT, CELLS, RES, KMAX = 0.05, 20, 0.25, 3
# the least distance of the generated inputs from each decision (tests/test_crowd.py asserts them)
CONDITIONS = {"theta": 1e-3, "pair": 1e-3, "goal": 1e-9, "edge": 1e-9, "speed": 1e-3}
# K, cyclic, robot_visible, desired_speeds given, grid: every flag on and off, K = 1 and 3, the grid absent / shared / per robot
CONFIGS = [dict(K=3, cyclic=True, robot_visible=True, speeds=True, grid="per"),
           dict(K=1, cyclic=False, robot_visible=False, speeds=False, grid=None),
           dict(K=3, cyclic=False, robot_visible=True, speeds=False, grid="shared"),
           dict(K=1, cyclic=True, robot_visible=False, speeds=True, grid="per")]
PARAMS = dict(goal_radius=0.25, person_radius=0.35, desired_speed=0.6)


def _pair_ok(a, b):
    """both ordered pairs of two (x, y, vx, vy) states stay 2 x CONDITIONS away from theta = 0, |theta| = pi and each other"""
    if math.hypot(a[0] - b[0], a[1] - b[1]) < 2 * CONDITIONS["pair"]:
        return False
    for me, ot in ((a, b), (b, a)):
        th = abs(R.pair_theta(ot[0] - me[0], ot[1] - me[1], me[2] - ot[2], me[3] - ot[3])[0])
        if min(th, abs(th - math.pi)) < 2 * CONDITIONS["theta"]:
            return False
    return True


def generate(B, Np, seed):
    g = np.random.default_rng(seed)
    count = g.integers(0, Np + 1, B).astype(np.int32)
    count[0] = Np
    if B >= 2:
        count[B - 1] = 0
    pose = np.concatenate([g.uniform(-2.0, 2.0, (B, 2)), g.uniform(-math.pi, math.pi, (B, 1))], axis=1)
    twist = np.stack([g.uniform(0.05, 0.6, B), g.uniform(-1.0, 1.0, B)], axis=1)
    twist[np.arange(B) % 4 == 1, 0] = 0.0                       # every fourth robot stands
    grids = g.integers(0, CELLS * CELLS, (B, CELLS, CELLS)).astype(np.uint32)
    origin = np.array([-2.5, -2.5]) + g.uniform(-0.1, 0.1, (B, 2))   # 5 m x 5 m: the persons beyond +-2.5 m are off it
    grids[0, 11, 7] = CELLS * CELLS                             # an out-of-range entry, under person 0 of robot 0 (below)

    def person():
        sp, hd = g.uniform(0.2, 0.8), g.uniform(-math.pi, math.pi)
        return np.array([g.uniform(-3.0, 3.0), g.uniform(-3.0, 3.0), sp * math.cos(hd), sp * math.sin(hd), g.uniform(-1.0, 1.0)])

    people = np.stack([np.stack([person() for _ in range(Np)]) for _ in range(B)])
    people[0, 0, 0:2] = origin[0] + np.array([7.3, 11.6]) * float(np.float32(RES))
    for b in range(B):
        rob = (pose[b, 0], pose[b, 1], twist[b, 0] * math.cos(pose[b, 2]), twist[b, 0] * math.sin(pose[b, 2]))
        for i in range(count[b]):
            fixed = b == 0 and i == 0
            while not (all(_pair_ok(people[b, i], people[b, j]) for j in range(i)) and _pair_ok(people[b, i], rob)):
                assert not fixed
                people[b, i] = person()
    waypoints = g.uniform(-4.0, 4.0, (B, Np, KMAX, 2))
    n_wp = g.integers(0, KMAX + 1, (B, Np)).astype(np.int32)
    cursor = (g.integers(0, KMAX + 1, (B, Np)) % (n_wp + 1)).astype(np.int32)   # 0 .. n_wp (n_wp: no goal left)
    near = g.uniform(0.255, 0.30, (B, Np))                      # every third person is about to arrive at its waypoint
    for b in range(B):
        for i in range(0, Np, 3):
            v = people[b, i, 2:4]
            waypoints[b, i, :, :] = people[b, i, 0:2] + near[b, i] * v / math.hypot(*v)
    speeds = g.uniform(0.3, 0.9, (B, Np))
    return dict(B=B, Np=Np, count=count, pose=pose, twist=twist, people=people, cursor=cursor, waypoints=waypoints,
                n_waypoints=n_wp, speeds=speeds, grids=grids, origin=origin)


def arguments(d, cfg, rows=slice(None), people=None, cursor=None):
    """(positional arguments dt .. n_waypoints, keyword arguments) of R.step_batch for one configuration; the library's
    BatchSolver.crowd_step takes the same values (see call() in tests/test_gpu_crowd.py)."""
    K = cfg["K"]
    n_wp = np.minimum(d["n_waypoints"], K)
    cur = np.minimum(d["cursor"], n_wp) if cursor is None else cursor
    pos = (DT, d["people"][rows] if people is None else people, cur[rows] if cursor is None else cur, d["pose"][rows],
           d["twist"][rows], d["count"][rows], np.ascontiguousarray(d["waypoints"][rows, :, :K]), n_wp[rows])
    kw = dict(cyclic=cfg["cyclic"], robot_visible=cfg["robot_visible"], desired_speeds=d["speeds"][rows] if cfg["speeds"] else None,
              **PARAMS)
    if cfg["grid"] == "per":
        kw.update(od_indexes=d["grids"][rows], od_origin=d["origin"][rows], od_resolution=RES)
    elif cfg["grid"] == "shared":
        kw.update(od_indexes=d["grids"][0], od_origin=d["origin"][0], od_resolution=RES)
    return pos, kw


def robot_arguments(pos, kw, b):
    """arguments() of robot b alone, for R.step / R.margins"""
    one = dict(kw)
    if kw["desired_speeds"] is not None:
        one["desired_speeds"] = kw["desired_speeds"][b]
    if kw.get("od_indexes") is not None and np.ndim(kw["od_indexes"]) == 3:
        one["od_indexes"], one["od_origin"] = kw["od_indexes"][b], kw["od_origin"][b]
    return (pos[0],) + tuple(a[b] for a in pos[1:]), one


_cache = {}


def case(shape):
    if shape not in _cache:
        _cache[shape] = generate(*shape, SEEDS[shape])
    return _cache[shape]


def reference(shape, ci, events=None):
    """(people, cursor) after one step of configuration CONFIGS[ci], by the checker: computed once per session."""
    key = (shape, ci)
    if key not in _cache:
        pos, kw = arguments(case(shape), CONFIGS[ci])
        ev = {}
        _cache[key] = R.step_batch(*pos, events=ev, **kw) + (ev,)
    return _cache[key]


# ---- reactivity: a person walks at 0.6 m/s towards a standing robot from 3 m, OFFSET off the robot's axis, its waypoint
# 3 m behind the robot; 120 steps
OFFSET, REACT_STEPS = 0.1, 120


def reactivity_inputs():
    people = np.array([[[3.0, OFFSET, -0.6, 0.0, 0.0]]])
    return dict(people=people, cursor=np.zeros((1, 1), np.int32), pose=np.zeros((1, 3)), twist=np.zeros((1, 2)),
                count=np.ones(1, np.int32), waypoints=np.array([[[[-3.0, OFFSET]]]]), n_waypoints=np.ones((1, 1), np.int32))


def closest_approach(stepper, visible):
    """min over REACT_STEPS steps of the person's distance to the robot; stepper(people, cursor, d, visible) -> (people, cursor)"""
    d = reactivity_inputs()
    people, cursor, least = d["people"], d["cursor"], math.inf
    for _ in range(REACT_STEPS):
        people, cursor = stepper(people, cursor, d, visible)
        least = min(least, math.hypot(people[0, 0, 0], people[0, 0, 1]))
    return least
