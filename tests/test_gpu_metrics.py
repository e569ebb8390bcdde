"""smpc_episode_metrics_batch on the device against the CPU checker (tests/metrics_ref.py): seeded random walks of B
robots among up to Np persons each, twelve samples, per-robot 20 x 20 distance grids, some robots off the grid, some
reaching their goal mid-way. Shapes: one robot per wave (Np = 64 and, rounded up to 64 lanes, Np = 33), several robots
per wave (Np = 8: eight of them; Np = 1: sixty-four), a partly filled last wave, the widest crowd, B = 1.

The generator's inputs are checked here, on the CPU, to stay clear of every decision the rules take (CONDITIONS), so a
comparison flipped on the device cannot hide behind a tie; the seeds below were chosen so that every robot of every
shape passes. The ties themselves are the binary-exact cases of tests/test_metrics.py, repeated on the device in
test_boundary_cases."""
import ctypes as C
import math

import numpy as np
import pytest

import metrics_ref as R
from nav2_social_mpc_controller_amd.params import MetricsParams, OptimizerParams

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 64), (65, 33), (130, 8)]
SEEDS = {(1, 1): 11, (3, 64): 12, (65, 33): 13, (130, 8): 14}
STEPS, DT, CELLS, RES = 12, 0.05, 20, 0.25
MP = MetricsParams(goal_tolerance=0.05)   # below the walk's shortest step: a robot is at its goal in one sample only
I = R.I
# the least distance of the generated inputs from each decision (asserted by check_conditions)
CONDITIONS = {"theta": 1e-3, "pair": 1e-3, "edge": 1e-9, "threshold": 1e-9}


def generate(B, Np, seed):
    """dict of per-sample inputs (lists of STEPS arrays) and fixed ones."""
    g = np.random.default_rng(seed)
    count = g.integers(0, Np + 1, B).astype(np.int32)
    if B >= 2:   # (a batch of one robot cannot have both)
        count[0], count[B - 1] = Np, 0
    else:
        count[0] = Np
    grids = g.uniform(0.0, 2.0, (B, CELLS, CELLS)).astype(np.float32)      # robot_radius 0.3: some cells collide
    origin = np.array([-2.5, -2.5]) + g.uniform(-0.1, 0.1, (B, 2))         # 5 m x 5 m around the start area
    pos = g.uniform(-2.0, 2.0, (B, 2))
    off = np.arange(B) % 5 == 2                                            # these start beyond the grid's edge
    pos[off, 0] += 4.0
    course = g.uniform(-math.pi, math.pi, B)                               # the walk drifts along it: no sample comes back

    def person():
        return np.concatenate([g.uniform(-3.0, 3.0, 2), g.uniform(-0.8, 0.8, 2), g.uniform(-1, 1, 1)])

    poses, twists, peoples, statuses, sources = [], [], [], [], []
    for k in range(STEPS):
        v = g.uniform(0.0, 0.6, B)
        heading = course + g.uniform(-math.pi / 3, math.pi / 3, B)
        step = g.uniform(0.15, 0.3, B)                                     # >= 0.075 m along the course per sample
        pos = pos + step[:, None] * np.stack([np.cos(heading), np.sin(heading)], axis=1)
        yaw = g.uniform(-math.pi, math.pi, B)                              # large turns: the wrap is exercised
        here = pos.copy()
        if k == 1:   # an excursion beyond the grid and back for every fourth robot (the lone robot of B = 1 among them)
            here[np.arange(B) % 4 == 0, 0] += 6.0
        poses.append(np.concatenate([here, yaw[:, None]], axis=1))
        twists.append(np.stack([v, g.uniform(-1, 1, B)], axis=1))
        # the crowd of every sample is drawn afresh (a sample is one world state; nothing in the rules links two crowds);
        # a person whose pair with the robot sits within twice CONDITIONS of the sign change of theta, or on the robot, is
        # drawn again
        pp = np.stack([np.stack([person() for _ in range(Np)]) for _ in range(B)])
        for b in range(B):
            for i in range(count[b]):
                while (R.theta_margin(poses[k][b], twists[k][b], pp[b, i:i + 1], 1) < 2 * CONDITIONS["theta"]
                       or math.hypot(*(pp[b, i, 0:2] - here[b])) < 2 * CONDITIONS["pair"]):
                    pp[b, i] = person()
        peoples.append(pp)
        statuses.append(g.choice(np.array([0, 1, 2, -1], np.int32), B))
        sources.append(g.choice(np.array([0, 0, 1, 2, 3], np.int32), B))
    # goals: every third robot stands on its goal at sample 2 + (b mod 7) (distance exactly 0), the others never get near
    goal = np.full((B, 2), 50.0)
    for b in range(0, B, 3):
        goal[b] = poses[2 + b % 7][b, 0:2]
    return dict(B=B, Np=Np, count=count, grids=grids, origin=origin, goal=goal, pose=poses, twist=twists, people=peoples,
                status=statuses, source=sources)


def check_conditions(d):
    """Every robot, every sample: clear of each decision by CONDITIONS (a robot frozen at its goal is checked all the same)."""
    for k in range(STEPS):
        for b in range(d["B"]):
            m = R.margins(MP, d["pose"][k][b], d["people"][k][b], d["count"][b], d["goal"][b], d["grids"][b], d["origin"][b], RES)
            m["theta"] = R.theta_margin(d["pose"][k][b], d["twist"][k][b], d["people"][k][b], d["count"][b])
            for name, least in CONDITIONS.items():
                assert m[name] >= least, (d["B"], d["Np"], k, b, name, m[name])


def reference(d, grid=True, goal=True, ctl=True):
    """acc after every sample, by the checker: list of STEPS arrays [B,24]."""
    acc, out = np.zeros((d["B"], R.NCOLS)), []
    for k in range(STEPS):
        acc = R.update(acc, MP, DT, d["pose"][k], d["twist"][k], d["people"][k], d["count"], d["goal"] if goal else None,
                       d["grids"] if grid else None, d["origin"] if grid else None, RES if grid else None,
                       d["status"][k] if ctl else None, d["source"][k] if ctl else None)
        out.append(acc)
    return out


_cache = {}


def case(shape):
    """(inputs, checker rows after every sample) of a shape: generated, checked and evaluated once per session."""
    if shape not in _cache:
        d = generate(*shape, SEEDS[shape])
        check_conditions(d)
        _cache[shape] = (d, reference(d))
    return _cache[shape]


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme())
    yield s
    s.close()


def sample(s, d, k, acc, grid=True, goal=True, ctl=True, rows=slice(None), grids=None, origin=None):
    return s.episode_metrics(MP, DT, acc, d["pose"][k][rows], d["twist"][k][rows], d["people"][k][rows], d["count"][rows],
                             goal=d["goal"][rows] if goal else None,
                             od_distances=(d["grids"][rows] if grids is None else grids) if grid else None,
                             od_origin=(d["origin"][rows] if origin is None else origin) if grid else None,
                             od_resolution=RES if grid else None,
                             status=d["status"][k][rows] if ctl else None, source=d["source"][k][rows] if ctl else None)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}_Np{s[1]}")
def test_one_and_twelve_samples_match_the_checker(solver, shape):
    d, want = case(shape)
    B = d["B"]
    if B >= 2:
        assert (d["count"] == 0).any() and (d["count"] == d["Np"]).any()
    acc = np.zeros((B, R.NCOLS))
    frozen_since = {}
    for k in range(STEPS):
        new = sample(solver, d, k, acc)
        for b, row in frozen_since.items():   # frozen at the goal: bit-identical from then on
            assert new[b].tobytes() == row, (k, b)
        for b in np.where(new[:, I["time_to_goal"]] >= 0)[0]:
            frozen_since.setdefault(int(b), new[b].tobytes())
        acc = new
        if k in (0, STEPS - 1):
            R.compare(acc, want[k], f"B={B} Np={d['Np']} after {k + 1} samples")
    # the walk did what the test is about: arrivals mid-way, robots on and off the grid, every zone counter moving
    ttg = want[-1][:, I["time_to_goal"]]
    assert ((ttg > DT) & (ttg < STEPS * DT)).any()
    assert (want[-1][:, I["off_grid_samples"]] > 0).any() and (want[-1][:, I["min_clearance"]] < np.inf).any()
    if B >= 65:
        assert (ttg < 0).any()
        for c in ("intimate_samples", "personal_samples", "social_samples", "person_collision_samples",
                  "obstacle_collision_samples", "fallback_samples", "unusable_solves"):
            assert (want[-1][:, I[c]] > 0).any(), c


def test_boundary_cases(solver):
    """The ties of tests/test_metrics.py on the device: binary-exact inputs that sit on a threshold."""
    mp = MetricsParams(intimate_radius=0.5, personal_radius=1.25, social_radius=3.5, robot_radius=0.25, person_radius=0.25,
                       goal_tolerance=0.25)
    # robot 0: a person exactly 0.5 m away; robot 1: the same, 1/128 m closer; robot 2: exactly on the goal tolerance, in a
    # cell whose clearance equals robot_radius; robot 3: x exactly on the grid's far edge
    pose = np.array([[1.0, 1.0, 0.0], [1.0078125, 1.0, 0.0], [0.75, 0.0, 0.0], [1.0, 0.25, 0.0]])
    twist = np.array([[0.5, 0.0]] * 4)
    people = np.zeros((4, 2, 5))
    people[:, 0] = [1.5, 1.0, 0.0, 0.25, 0.0]
    people[:, 1] = [8.0, 8.0, 0.0, 0.0, 0.0]
    count = np.array([2, 2, 0, 0], np.int32)
    goal = np.array([[9.0, 9.0], [9.0, 9.0], [1.0, 0.0], [9.0, 9.0]])
    grid = np.full((3, 4), 0.25, np.float32)
    origin, res = np.array([-1.0, 0.0]), 0.5
    got = solver.episode_metrics(mp, DT, np.zeros((4, R.NCOLS)), pose, twist, people, count, goal=goal, od_distances=grid,
                                 od_origin=origin, od_resolution=res)
    want = R.update(np.zeros((4, R.NCOLS)), mp, DT, pose, twist, people, count, goal, grid, origin, res)
    R.compare(got, want, "boundary cases")
    assert got[:, I["intimate_samples"]].tolist() == [0, 1, 0, 0] and got[:, I["person_collision_samples"]].tolist() == [0, 1, 0, 0]
    assert got[0, I["min_person_dist"]] == 0.5 and got[:, I["personal_samples"]].tolist() == [1, 1, 0, 0]
    assert got[2, I["time_to_goal"]] == DT and got[2, I["goal_dist"]] == 0.25       # <= : on the tolerance counts
    assert got[2, I["min_clearance"]] == 0.25 and got[2, I["obstacle_collision_samples"]] == 0   # < : it does not
    assert got[:, I["off_grid_samples"]].tolist() == [1, 1, 0, 1]                   # x = 1.0 is the first cell beyond
    # heading change through pi
    acc = solver.episode_metrics(mp, DT, np.zeros((1, R.NCOLS)), [[0.0, 0.0, 3.1]], [[0.0, 0.0]], people[:1], [0])
    acc = solver.episode_metrics(mp, DT, acc, [[0.0, 0.0, -3.1]], [[0.0, 0.0]], people[:1], [0])
    assert acc[0, I["heading_change"]] == (-3.1 - 3.1) + 2.0 * math.pi and acc[0, I["path_length"]] == 0.0


def test_optional_inputs(solver):
    d, _ = case((65, 33))
    B = d["B"]
    want = reference(d, grid=False, goal=False, ctl=False)
    acc = np.zeros((B, R.NCOLS))
    for k in range(3):
        acc = sample(solver, d, k, acc, grid=False, goal=False, ctl=False)
    R.compare(acc, want[2], "no grid, goal, status, source")
    assert (acc[:, I["min_clearance"]] == np.inf).all() and (acc[:, I["time_to_goal"]] == -1.0).all()
    for c in ("obstacle_collision_samples", "off_grid_samples", "goal_dist", "fallback_samples", "unusable_solves"):
        assert (acc[:, I[c]] == 0.0).all(), c
    # one input at a time
    for kw in (dict(goal=False, ctl=False), dict(grid=False, ctl=False), dict(grid=False, goal=False)):
        got = sample(solver, d, 0, np.zeros((B, R.NCOLS)), **{**dict(grid=True, goal=True, ctl=True), **kw})
        R.compare(got, reference(d, **{**dict(grid=True, goal=True, ctl=True), **kw})[0], str(kw))
    # a shared grid against per-robot copies of it
    one, origin = d["grids"][7], d["origin"][7]
    a = sample(solver, d, 0, np.zeros((B, R.NCOLS)), grids=one, origin=origin)
    b = sample(solver, d, 0, np.zeros((B, R.NCOLS)), grids=np.repeat(one[None], B, axis=0), origin=np.repeat(origin[None], B, axis=0))
    assert a.tobytes() == b.tobytes()
    assert (a[:, I["off_grid_samples"]] > 0).any() and (a[:, I["min_clearance"]] < np.inf).any()


def test_rows_do_not_depend_on_the_batch_or_the_memory_space(solver):
    import torch

    d, _ = case((130, 8))
    B, Np = d["B"], d["Np"]
    acc = np.zeros((B, R.NCOLS))
    for k in range(3):
        acc = sample(solver, d, k, acc)
    full = sample(solver, d, 3, acc)
    for b in range(B):
        alone = sample(solver, d, 3, acc[b:b + 1], rows=slice(b, b + 1))
        assert alone.tobytes() == full[b:b + 1].tobytes(), b
    # device pointers
    dev = "cuda:0"
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(
        pose=d["pose"][3], twist=d["twist"][3], people=d["people"][3], count=d["count"], goal=d["goal"], grids=d["grids"],
        origin=d["origin"], status=d["status"][3], source=d["source"][3], acc=acc).items()}
    mb = solver.metrics_c(MP, B, Np, DT, 1)
    mb.robot_pose, mb.robot_twist, mb.people, mb.count = t["pose"].data_ptr(), t["twist"].data_ptr(), t["people"].data_ptr(), t["count"].data_ptr()
    mb.goal, mb.od_distances, mb.od_origin = t["goal"].data_ptr(), t["grids"].data_ptr(), t["origin"].data_ptr()
    mb.od_shared, mb.od_width, mb.od_height, mb.od_resolution = 0, CELLS, CELLS, RES
    mb.status, mb.source = t["status"].data_ptr(), t["source"].data_ptr()
    solver.episode_metrics_device(mb, t["acc"].data_ptr())
    torch.cuda.synchronize()
    solver.set_stream(0)
    assert t["acc"].cpu().numpy().tobytes() == full.tobytes()


def test_refusals_leave_acc_untouched(solver):
    d, _ = case((3, 64))
    B, Np = d["B"], d["Np"]
    lib, h = solver.lib, solver._h
    arrays = dict(pose=d["pose"][0], twist=d["twist"][0], people=d["people"][0], count=d["count"].copy(), goal=d["goal"],
                  grids=d["grids"], origin=d["origin"])
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    sentinel = np.arange(B * R.NCOLS, dtype=np.float64).reshape(B, R.NCOLS) + 0.5

    def call(acc_null=False, **change):
        mb = solver.metrics_c(MP, B, Np, DT, 0)
        mb.robot_pose, mb.robot_twist = arrays["pose"].ctypes.data, arrays["twist"].ctypes.data
        mb.people, mb.count, mb.goal = arrays["people"].ctypes.data, arrays["count"].ctypes.data, arrays["goal"].ctypes.data
        mb.od_distances, mb.od_origin = arrays["grids"].ctypes.data, arrays["origin"].ctypes.data
        mb.od_shared, mb.od_width, mb.od_height, mb.od_resolution = 0, CELLS, CELLS, RES
        keep = []
        for k, v in change.items():
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = v.ctypes.data
            setattr(mb, k, v)
        acc = sentinel.copy()
        rc = lib.smpc_episode_metrics_batch(h, C.byref(mb), None if acc_null else acc.ctypes.data)
        assert acc.tobytes() == sentinel.tobytes(), change
        return rc

    INVALID, UNSUPPORTED = -1, -2
    wide = np.zeros((B, 65, 5))
    assert call(Np=65, people=wide) == UNSUPPORTED
    bad = [dict(B=0), dict(B=-1), dict(Np=0), dict(dt=0.0), dict(dt=-0.05), dict(dt=float("nan")),
           dict(goal_tolerance=-1e-9), dict(robot_radius=-0.1), dict(person_radius=-0.1), dict(intimate_radius=-0.1),
           dict(personal_radius=-0.1), dict(social_radius=-0.1),
           dict(robot_pose=None), dict(robot_twist=None), dict(people=None), dict(count=None),
           dict(od_origin=None), dict(od_width=0), dict(od_height=0), dict(od_height=-3), dict(od_resolution=0.0),
           dict(od_resolution=-0.25)]
    for change in bad:
        assert call(**change) == INVALID, change
    assert call(acc_null=True) == INVALID
    for where, value in ((0, -1), (B - 1, Np + 1)):
        c = arrays["count"].copy()
        c[where] = value
        assert call(count=c) == INVALID, (where, value)
