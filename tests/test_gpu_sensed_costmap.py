"""smpc_sensed_costmap_batch on the GPU against tests/sensed_costmap_ref.py, bit for bit in all three outputs: the hand-made
calls of tests/sensed_costmap_cases.py, random calls on make_world floors (24 x 20 windows whose 16-byte pieces straddle
rows, windows of odd sizes, windows of more rows than one band), one call that fills the LDS (64 robots, 200 x 200, 360
beams, r = 14) and the limits (256 x 256, d2_max = 1024, 4096 beams); host against device pointers, an unaligned window
array, a robot's rows under a permuted and a shorter batch, two runs, worlds per robot, NULL beam arrays and the refusals."""
import re

import numpy as np
import pytest

import sensed_costmap_cases as K
import sensed_costmap_ref as R
from nav2_social_mpc_controller_amd import _abi_sensed_costmap as SA
from nav2_social_mpc_controller_amd.params import OptimizerParams

pytestmark = pytest.mark.gpu

HAND = K.hand_cases()
RANDOM = {
    "reach10": dict(seed=1, reach=10, off_fraction=0.3),                                  # make_world(96, 80), B = 8, Np = 3, 24 x 20, 64 beams, r = 3
    "reach30": dict(seed=1, reach=30, off_fraction=0.3, base=1),
    "odd_size": dict(seed=2, reach=30, size=(37, 70), r=5, base=1, off_fraction=0.3),   # a byte at a time
    "two_bands_narrow": dict(seed=3, reach=30, size=(21, 150), r=3, world_size=(96, 200), off_fraction=0.3),
    "tiny_window": dict(seed=4, reach=10, size=(8, 3), r=3, base=1),                    # size_x a multiple of 8, the window no multiple of 16
    "full_lds": dict(world_size=(400, 400), B=64, Np=8, size=(200, 200), n_beams=360, reach=50, r=14, seed=3, discs=30, base=1,
                     agent_d2=36),
    "limits": dict(world_size=(300, 300), B=2, Np=8, size=(256, 256), n_beams=4096, reach=127, r=32, seed=5, discs=20, agent_d2=36),
}
INFORMATIVE = ("reach10", "reach30")
_cache = {}


def arguments(name):
    """(arguments, the yardstick's outputs, its statistics) of a case, computed once."""
    if name not in _cache:
        kw = HAND[name][0] if name in HAND else K.random_case(**RANDOM[name])
        stats = {}
        want = R.sensed_costmap(**kw, stats=stats)
        for a in want:
            a.setflags(write=False)
        _cache[name] = (kw, want, stats)
    return _cache[name]


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


def host_call(solver, kw, rows=None, beams=True):
    rows = slice(None) if rows is None else rows
    world, origin = kw["world"], kw["origin"]
    if np.ndim(world) == 3:
        world, origin = world[rows], np.asarray(origin).reshape(-1, 2)[rows]
    return solver.sensed_costmap(world, origin, kw["res"], kw["robot_pose"][rows], kw["people"][rows], kw["count"][rows], kw["cell"][rows],
                                 kw["size_x"], kw["size_y"], kw["beam_cells"], kw["agent_d2"], kw["table"], kw["base"], kw["outside_cost"],
                                 kw["min_cost"], kw["unknown"], beams=beams)


def device_call(solver, kw, offset=0, beams=True):
    """The call on device pointers; the window array starts `offset` bytes into its allocation."""
    import torch
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point
    dev = "cuda:0"
    B, Np, nb = kw["people"].shape[0], kw["people"].shape[1], len(kw["beam_cells"])
    world = np.asarray(kw["world"], np.uint8)
    shared = world.ndim == 2
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(world=world, world_origin=np.asarray(kw["origin"], np.float64).reshape(-1, 2), robot_pose=kw["robot_pose"], people=kw["people"],
              count=kw["count"].astype(np.int32), cell=kw["cell"].astype(np.int32), beam_cells=kw["beam_cells"].astype(np.int32),
              inflation_cost=np.asarray(kw["table"], np.uint8)).items()}
    si = point(BatchSolver.sensed_costmap_c(B, Np, kw["size_x"], kw["size_y"], world.shape[-1], world.shape[-2], shared, kw["res"], 1, nb,
                                            kw["agent_d2"], len(kw["table"]) - 1, kw["base"], kw["outside_cost"], kw["min_cost"], kw["unknown"]), t)
    n = B * kw["size_x"] * kw["size_y"]
    raw = torch.full((n + offset,), 0xEE, dtype=torch.uint8, device=dev)
    cm = raw[offset:]
    kind = torch.full((B, nb), 0xEE, dtype=torch.uint8, device=dev)
    hit = torch.full((B, nb, 2), -77, dtype=torch.int32, device=dev)
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    solver.sensed_costmap_device(si, cm.data_ptr(), kind.data_ptr() if beams else 0, hit.data_ptr() if beams else 0)
    torch.cuda.synchronize()
    solver.set_stream(0)
    return cm.cpu().numpy().reshape(B, kw["size_y"], kw["size_x"]), kind.cpu().numpy(), hit.cpu().numpy()


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def where(got, want):
    return [np.argwhere(g != w)[:4].tolist() for g, w in zip(got, want)]


# ---- against the yardstick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND) + list(RANDOM))
def test_all_three_outputs_are_the_yardsticks_from_host_and_device_pointers_twice(solver, name):
    kw, want, _ = arguments(name)
    got = host_call(solver, kw)
    assert same(got, want), where(got, want)
    if name in HAND:
        for (b, k), (kind, cell) in HAND[name][1].items():
            assert (int(got[1][b, k]), tuple(int(v) for v in got[2][b, k])) == (kind, cell)
    dev = device_call(solver, kw)
    assert same(dev, want), where(dev, want)
    assert same(device_call(solver, kw), dev) and same(host_call(solver, kw), got)           # two runs, bit for bit


@pytest.mark.parametrize("name", INFORMATIVE)
def test_the_random_cases_are_informative_by_the_yardstick_alone(name):
    kw, (_, kind, _), stats = arguments(name)
    counts = np.bincount(kind.ravel(), minlength=6)
    assert (counts[[R.NONE, R.WORLD, R.AGENT, R.CORNER_PAIR]] > 0).all() and counts[R.INVALID] == 0 and counts[R.NO_ROBOT] == 0
    assert stats["dropped"] >= 1                                                              # a hit outside its window
    assert (stats["marks"] >= 3).sum() * 4 >= len(stats["marks"])                             # a quarter of the robots with three marks or more


@pytest.mark.parametrize("name", ["reach10", "reach30", "count_clamp", "no_robot", "full_lds", "limits"])
def test_a_robots_rows_do_not_depend_on_the_batch(solver, name):
    kw, want, _ = arguments(name)
    B = kw["people"].shape[0]
    perm = np.random.default_rng(B).permutation(B)
    got = host_call(solver, kw, perm)
    assert same(got, [w[perm] for w in want])
    for rows in ([B - 1], list(range(0, B, 2))):
        got = host_call(solver, kw, rows)
        assert same(got, [w[rows] for w in want])


def test_worlds_per_robot(solver):
    kw = dict(arguments("reach30")[0])
    B = kw["people"].shape[0]
    g = np.random.default_rng(17)
    worlds = np.repeat(kw["world"][None], B, axis=0).copy()
    worlds[g.random(worlds.shape) < 0.01] = 254                                               # every robot its own clutter
    origins = np.repeat(np.asarray(kw["origin"]).reshape(1, 2), B, axis=0)
    origins[1::2] += 0.05 * g.integers(-3, 4, (len(origins[1::2]), 2))                        # ... and every other one its own origin
    kw.update(world=worlds, origin=origins)
    want = R.sensed_costmap(**kw)
    assert len({w.tobytes() for w in worlds}) == B and not same(want, arguments("reach30")[1])
    assert same(host_call(solver, kw), want) and same(device_call(solver, kw), want)
    one = host_call(solver, kw, [3])
    assert same(one, [w[[3]] for w in want])


def test_an_unaligned_window_array_and_null_beam_arrays(solver):
    for name in ("reach30", "full_lds"):
        kw, want, _ = arguments(name)
        for offset in (8, 3):                                                                 # the 16-byte path needs 16-byte windows
            assert same(device_call(solver, kw, offset=offset), want)
    kw, want, _ = arguments("reach10")
    cm, kind, hit = device_call(solver, kw, beams=False)
    assert np.array_equal(cm, want[0]) and (kind == 0xEE).all() and (hit == -77).all()
    cm, kind, hit = host_call(solver, kw, beams=False)
    assert np.array_equal(cm, want[0]) and kind is None and hit is None


def test_a_pedestrian_in_range_puts_lethal_cells_where_the_world_has_none(solver):
    from nav2_social_mpc_controller_amd.params import SensorParams
    sp, res = SensorParams(), 0.05
    world = np.zeros((120, 120), np.uint8)
    table, _ = sp.inflation_table(res)
    pose = np.array([[3.0, 3.0, 0.0]])
    people = np.array([[[4.5, 3.0, 0.0, 0.0, 0.0]]])                                          # 1.5 m ahead, within the 2.5 m of the scan
    cell = np.array([[20, 20]], np.int32)                                                     # an 80 x 80 window around the robot
    args = (world, [0.0, 0.0], res, pose, people, [1], cell, 80, 80, sp.beam_cells(res), sp.agent_d2(res), table)
    cm, kind, hit = solver.sensed_costmap(*args)
    assert (kind == R.AGENT).sum() >= 10 and set(kind.ravel()) == {R.NONE, R.AGENT}
    lethal = np.argwhere(cm[0] == 254) + [20, 20]                                             # (y, x) world cells
    assert len(lethal) >= 5 and (np.hypot(lethal[:, 1] - 90, lethal[:, 0] - 60) <= 6.0).all()   # on the person's disc of 6 cells
    assert (lethal[:, 1] <= 90).all()                                                         # its near side only
    empty, kind0, _ = solver.sensed_costmap(*args[:5], [0], *args[6:])
    assert not empty.any() and (kind0 == R.NONE).all()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_poisoned_outputs_alone(solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError, _ptr
    world, origin = np.zeros((5, 7), np.uint8), np.zeros((1, 2))
    pose, people, count = np.array([[3.5, 2.5, 0.0]]), np.full((1, 2, 5), 2.5), np.full(1, 2, np.int32)
    cell, beams, table = np.zeros((1, 2), np.int32), np.array([[2, 0], [0, 2]], np.int32), np.array([254, 100], np.uint8)
    cm, kind, hit = np.full((1, 5, 7), 0xEE, np.uint8), np.full((1, 2), 0xEE, np.uint8), np.full((1, 2, 2), -77, np.int32)

    def sensed_in(**kw):
        st = SA.SmpcSensedCostmapIn(B=1, Np=2, on_device=0, size_x=7, size_y=5, world_x=7, world_y=5, world_shared=1, n_beams=2, agent_d2=0,
                                    d2_max=1, occlusion_min_cost=254, base=0, outside_cost=255, resolution=1.0, world=_ptr(world),
                                    world_origin=_ptr(origin), robot_pose=_ptr(pose), people=_ptr(people), count=_ptr(count), cell=_ptr(cell),
                                    beam_cells=_ptr(beams), inflation_cost=_ptr(table))
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    INVALID, UNSUPPORTED = "(-1)", "(-2)"
    nan, inf = float("nan"), float("inf")
    cases = [(dict(B=-1), INVALID), (dict(Np=0), INVALID), (dict(size_x=0), INVALID), (dict(size_y=-2), INVALID), (dict(world_x=0), INVALID),
             (dict(world_y=-1), INVALID), (dict(resolution=0.0), INVALID), (dict(resolution=-1.0), INVALID), (dict(resolution=nan), INVALID),
             (dict(resolution=inf), INVALID), (dict(n_beams=0), INVALID), (dict(agent_d2=-1), INVALID), (dict(d2_max=-1), INVALID),
             (dict(base=2), INVALID), (dict(world=None), INVALID), (dict(world_origin=None), INVALID), (dict(robot_pose=None), INVALID),
             (dict(people=None), INVALID), (dict(count=None), INVALID), (dict(cell=None), INVALID), (dict(beam_cells=None), INVALID),
             (dict(inflation_cost=None), INVALID), (dict(size_x=257), UNSUPPORTED), (dict(size_y=257), UNSUPPORTED),
             (dict(d2_max=1025), UNSUPPORTED), (dict(n_beams=4097), UNSUPPORTED), (dict(world_x=2 ** 16, world_y=2 ** 15), UNSUPPORTED)]
    for kw, code in cases:
        with pytest.raises(SmpcError, match=re.escape(code)):
            solver._call("smpc_sensed_costmap_batch", sensed_in(**kw), _ptr(cm), _ptr(kind), _ptr(hit))
    with pytest.raises(SmpcError, match=re.escape(INVALID)):
        solver._call("smpc_sensed_costmap_batch", sensed_in(), None, _ptr(kind), _ptr(hit))
    assert solver.lib.smpc_sensed_costmap_batch(None, sensed_in(), _ptr(cm), _ptr(kind), _ptr(hit)) == -1          # NULL handle
    assert solver.lib.smpc_sensed_costmap_batch(solver._h, None, _ptr(cm), _ptr(kind), _ptr(hit)) == -1            # NULL struct
    # an empty batch is no refusal and writes nothing, whatever else is in the struct
    solver._call("smpc_sensed_costmap_batch", sensed_in(B=0), _ptr(cm), _ptr(kind), _ptr(hit))
    assert (cm == 0xEE).all() and (kind == 0xEE).all() and (hit == -77).all()
    # the accepted call runs: both agents stand in cell (2, 2), one cell left of the robot's (3, 2); nothing stops the beams
    solver._call("smpc_sensed_costmap_batch", sensed_in(), _ptr(cm), _ptr(kind), _ptr(hit))
    assert kind.tolist() == [[R.NONE, R.NONE]] and hit.tolist() == [[[2, 0], [0, 2]]] and not cm.any()
    solver._call("smpc_sensed_costmap_batch", sensed_in(agent_d2=2), _ptr(cm), _ptr(kind), _ptr(hit))
    assert kind.tolist() == [[R.NONE, R.AGENT]] and hit.tolist() == [[[2, 0], [0, 1]]] and cm[0, 3, 3] == 254 and cm[0, 2, 3] == 100
