"""smpc_obstacle_memory_batch on the GPU against tests/obstacle_memory_ref.py, bit for bit in all five outputs (window, beam
kinds, beam cells, mark bitmap, its window cell), tick by tick with the state fed forward from the device's own output: the
hand-made and seeded sequences of tests/obstacle_memory_cases.py, three ticks at 8 robots x 200 x 200 x 360 beams with
r = 14 (two bands, the 16-byte store path), one call at each limit (256 x 256, 4096 beams, d2_max = 1024); the memoryless
call as the special case the header names; host against device pointers, two runs, a permuted and a shorter batch, an
unaligned window array, NULL beam arrays, garbage in the padding bits, a robot without a cell, and the refusals."""
import re

import numpy as np
import pytest

import obstacle_memory_cases as OC
import obstacle_memory_ref as M
import sensed_costmap_cases as K
import sensed_costmap_ref as R
from nav2_social_mpc_controller_amd import _abi_obstacle_memory as OA
from nav2_social_mpc_controller_amd import _abi_sensed_costmap as SA
from nav2_social_mpc_controller_amd.params import OptimizerParams

pytestmark = pytest.mark.gpu

HAND = OC.hand_sequences()
SEEDED = OC.seeded_sequences()
_cache = {}


def reference(name):
    """The yardstick's ticks of a sequence, computed once: [(kw, mark_d2, footprint_d2, state before, outputs)]."""
    if name not in _cache:
        seq = HAND[name] if name in HAND else SEEDED[name] if name in SEEDED else BIG[name]()
        _cache[name] = [(kw, seq["ticks"][t][1], seq["ticks"][t][2], before, got) for t, kw, before, got, _ in OC.run(seq, OC.ref_call)]
        for _, _, _, before, got in _cache[name]:
            for a in list(before) + list(got[:3]) + list(got[3]):
                a.setflags(write=False)
    return _cache[name]


def wide_sequence():
    """3 ticks, 8 robots, 200 x 200 windows, 360 beams out to 60 cells, marks out to 50, r = 14: two bands, 16-byte stores."""
    return OC.seeded_sequence(seed=21, size=(200, 200), reach=60, ticks=3, B=8, Np=8, r=14, base=1, footprint_d2=23, mark_fraction=50 / 60,
                              world_size=(400, 400), n_beams=360, discs=30, agent_d2=36)


def limits_sequence():
    """One call at each limit: 256 x 256 windows, 4096 beams out to 127 cells, d2_max = 1024, on a populated memory."""
    seq = OC.seeded_sequence(seed=22, size=(256, 256), reach=127, ticks=1, B=2, Np=8, r=32, footprint_d2=23, mark_fraction=0.8, near_fraction=0.0,
                             world_size=(300, 300), n_beams=4096, discs=20, agent_d2=36)
    g = np.random.default_rng(22)
    marks = [{(int(x), int(y)) for x, y in g.integers(0, 256, (300, 2))} for _ in range(2)]
    seq["initial"] = (marks, seq["ticks"][0][0]["cell"] + np.array([[3, -2], [-37, 64]], np.int32))
    return seq


BIG = {"wide": wide_sequence, "limits": limits_sequence}


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


def host_call(solver, state, kw, mark_d2, footprint_d2, rows=None, beams=True):
    rows = slice(None) if rows is None else rows
    world, origin = kw["world"], kw["origin"]
    out = solver.obstacle_memory(state[0][rows], state[1][rows], world, origin, kw["res"], kw["robot_pose"][rows], kw["people"][rows],
                                 kw["count"][rows], kw["cell"][rows], kw["size_x"], kw["size_y"], kw["beam_cells"], kw["agent_d2"], kw["table"],
                                 mark_d2, footprint_d2, kw["base"], kw["outside_cost"], kw["min_cost"], kw["unknown"], beams=beams)
    return out[0], out[1], out[2], (out[3], out[4])


def device_call(solver, state, kw, mark_d2, footprint_d2, offset=0, beams=True):
    """The call on device pointers; the window array starts `offset` bytes into its allocation."""
    import torch
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point
    dev = "cuda:0"
    B, Np, nb = kw["people"].shape[0], kw["people"].shape[1], len(kw["beam_cells"])
    world = np.asarray(kw["world"], np.uint8)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(world=world, world_origin=np.asarray(kw["origin"], np.float64).reshape(-1, 2), robot_pose=kw["robot_pose"], people=kw["people"],
              count=kw["count"].astype(np.int32), cell=kw["cell"].astype(np.int32), beam_cells=kw["beam_cells"].astype(np.int32),
              inflation_cost=np.asarray(kw["table"], np.uint8)).items()}
    si = point(BatchSolver.sensed_costmap_c(B, Np, kw["size_x"], kw["size_y"], world.shape[-1], world.shape[-2], world.ndim == 2, kw["res"], 1, nb,
                                            kw["agent_d2"], len(kw["table"]) - 1, kw["base"], kw["outside_cost"], kw["min_cost"], kw["unknown"]), t)
    mi = BatchSolver.obstacle_memory_c(si, mark_d2, footprint_d2)
    n = B * kw["size_x"] * kw["size_y"]
    raw = torch.full((n + offset,), 0xEE, dtype=torch.uint8, device=dev)
    cm = raw[offset:]
    kind = torch.full((B, nb), 0xEE, dtype=torch.uint8, device=dev)
    hit = torch.full((B, nb, 2), -77, dtype=torch.int32, device=dev)
    memory = torch.from_numpy(np.ascontiguousarray(state[0]).view(np.int32).copy()).to(dev)
    memory_cell = torch.from_numpy(np.ascontiguousarray(state[1], np.int32).copy()).to(dev)
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    solver.obstacle_memory_device(mi, memory.data_ptr(), memory_cell.data_ptr(), cm.data_ptr(), kind.data_ptr() if beams else 0,
                                  hit.data_ptr() if beams else 0)
    torch.cuda.synchronize()
    solver.set_stream(0)
    return (cm.cpu().numpy().reshape(B, kw["size_y"], kw["size_x"]), kind.cpu().numpy(), hit.cpu().numpy(),
            (memory.cpu().numpy().view(np.uint32), memory_cell.cpu().numpy()))


def flat(out):
    return list(out[:3]) + list(out[3])


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(flat(got), flat(want)))


def where(got, want):
    return [np.argwhere(g != w)[:4].tolist() if g.shape == w.shape else (g.shape, w.shape) for g, w in zip(flat(got), flat(want))]


# ---- against the yardstick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND) + sorted(SEEDED) + sorted(BIG))
def test_all_five_outputs_are_the_yardsticks_tick_by_tick_from_the_devices_own_state(solver, name):
    ticks = reference(name)
    state = ticks[0][3]
    for t, (kw, mark_d2, footprint_d2, before, want) in enumerate(ticks):
        assert all(np.array_equal(a, b) for a, b in zip(state, before)), (name, t)           # the device's state is the yardstick's
        got = device_call(solver, state, kw, mark_d2, footprint_d2)
        assert same(got, want), (name, t, where(got, want))
        state = got[3]
    # the last tick again: from host pointers, and twice from the same state
    host = host_call(solver, before, kw, mark_d2, footprint_d2)
    assert same(host, want), (name, where(host, want))
    assert same(device_call(solver, before, kw, mark_d2, footprint_d2), got) and same(host_call(solver, before, kw, mark_d2, footprint_d2), host)


def test_zero_memory_and_a_wide_marking_range_is_the_memoryless_call(solver):
    for name in ("seed2_24x20_reach30", "seed3_40x33_reach10", "wide"):
        kw = reference(name)[-1][0]
        B = kw["people"].shape[0]
        plain = solver.sensed_costmap(kw["world"], kw["origin"], kw["res"], kw["robot_pose"], kw["people"], kw["count"], kw["cell"], kw["size_x"],
                                      kw["size_y"], kw["beam_cells"], kw["agent_d2"], kw["table"], kw["base"], kw["outside_cost"], kw["min_cost"],
                                      kw["unknown"])
        zero = M.zero_state(B, kw["size_x"], kw["size_y"])
        wild = (zero[0], np.tile(np.array([[-2 ** 31, 2 ** 31 - 1]], np.int32), (B, 1)))       # no valid memory_cell is needed
        for state in (zero, wild):
            for call in (host_call, device_call):
                got = call(solver, state, kw, OC.BIG, -1)
                assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got[:3], plain)), name
                assert np.array_equal(got[3][1], kw["cell"])
        assert (plain[1] != R.NONE).any()


@pytest.mark.parametrize("name", ["seed2_24x20_reach30", "seed4_40x33_reach30", "roll", "wide"])
def test_a_robots_rows_do_not_depend_on_the_batch(solver, name):
    kw, mark_d2, footprint_d2, before, want = reference(name)[-1]
    B = kw["people"].shape[0]
    take = lambda out, rows: (out[0][rows], out[1][rows], out[2][rows], (out[3][0][rows], out[3][1][rows]))
    perm = np.random.default_rng(B).permutation(B)
    for rows in (perm, [B - 1], list(range(0, B, 2))):
        got = host_call(solver, before, kw, mark_d2, footprint_d2, rows)
        assert same(got, take(want, rows)), where(got, take(want, rows))


def test_an_unaligned_window_array_and_null_beam_arrays(solver):
    for name in ("seed2_24x20_reach30", "wide"):
        kw, mark_d2, footprint_d2, before, want = reference(name)[-1]
        for offset in (8, 3):                                                                 # the 16-byte path needs 16-byte windows
            assert same(device_call(solver, before, kw, mark_d2, footprint_d2, offset=offset), want)
    kw, mark_d2, footprint_d2, before, want = reference("seed1_24x20_reach10")[-1]
    cm, kind, hit, state = device_call(solver, before, kw, mark_d2, footprint_d2, beams=False)
    assert np.array_equal(cm, want[0]) and (kind == 0xEE).all() and (hit == -77).all() and same((cm, want[1], want[2], state), want)
    cm, kind, hit, state = host_call(solver, before, kw, mark_d2, footprint_d2, beams=False)
    assert np.array_equal(cm, want[0]) and kind is None and hit is None and same((cm, want[1], want[2], state), want)


def test_garbage_in_the_input_padding_changes_nothing_and_the_output_padding_is_zero(solver):
    for name in ("seed3_40x33_reach10", "width_1", "width_31", "width_33", "seed1_24x20_reach10"):
        kw, mark_d2, footprint_d2, before, want = reference(name)[-1]
        sx = kw["size_x"]
        pad = ~np.array([(1 << min(32, max(0, sx - 32 * w))) - 1 for w in range(M.words(sx))], np.uint64).astype(np.uint32)
        assert pad[-1] != 0                                                                   # these widths have padding bits
        dirty = (before[0] | pad[None, None, :], before[1])
        for call in (host_call, device_call):
            got = call(solver, dirty, kw, mark_d2, footprint_d2)
            assert same(got, want) and not (got[3][0] & pad[None, None, :]).any()


def test_a_robot_with_a_nan_pose_rolls_its_memory_and_casts_nothing(solver):
    ticks = reference("seed4_40x33_reach30")
    kw, mark_d2, footprint_d2, before, _ = ticks[-1]
    kw = dict(kw, robot_pose=kw["robot_pose"].copy(), base=1)
    lost = np.argsort([len(M.bits_to_cells(m, kw["size_x"])) for m in before[0]])[-2:].tolist()   # the two robots that remember most
    kw["robot_pose"][lost, 0] = np.nan
    want = M.step(before, mark_d2=mark_d2, footprint_d2=footprint_d2, **kw)
    got = device_call(solver, before, kw, mark_d2, footprint_d2)
    assert same(got, want)
    for b in lost:
        sx, sy = kw["size_x"], kw["size_y"]
        s = before[1][b].astype(int) - kw["cell"][b].astype(int)
        moved = {(x + s[0], y + s[1]) for x, y in M.bits_to_cells(before[0][b], sx) if 0 <= x + s[0] < sx and 0 <= y + s[1] < sy}
        assert M.bits_to_cells(got[3][0][b], sx) == moved and len(moved) >= 1 and (got[1][b] == R.NO_ROBOT).all()
        assert np.array_equal(got[0][b], np.maximum(R.inflate(moved, sx, sy, kw["table"]), R.world_cut(kw["world"], kw["cell"][b], sx, sy, 255)))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_every_buffer_alone(solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError, _ptr
    world, origin = np.zeros((5, 7), np.uint8), np.zeros((1, 2))
    world[2, 5] = 254
    pose, people, count = np.array([[3.5, 2.5, 0.0]]), np.full((1, 2, 5), 2.5), np.full(1, 2, np.int32)
    cell, beams, table = np.zeros((1, 2), np.int32), np.array([[2, 0], [0, 2]], np.int32), np.array([254, 100], np.uint8)
    cm, kind, hit = np.full((1, 5, 7), 0xEE, np.uint8), np.full((1, 2), 0xEE, np.uint8), np.full((1, 2, 2), -77, np.int32)
    memory, memory_cell = np.full((1, 5, 1), 0x55, np.uint32), np.full((1, 2), 1, np.int32)

    def memory_in(mark_d2=100, footprint_d2=-1, **kw):
        st = SA.SmpcSensedCostmapIn(B=1, Np=2, on_device=0, size_x=7, size_y=5, world_x=7, world_y=5, world_shared=1, n_beams=2, agent_d2=0,
                                    d2_max=1, occlusion_min_cost=254, base=0, outside_cost=255, resolution=1.0, world=_ptr(world),
                                    world_origin=_ptr(origin), robot_pose=_ptr(pose), people=_ptr(people), count=_ptr(count), cell=_ptr(cell),
                                    beam_cells=_ptr(beams), inflation_cost=_ptr(table))
        for k, v in kw.items():
            setattr(st, k, v)
        return OA.SmpcObstacleMemoryIn(scan=st, mark_d2=mark_d2, footprint_d2=footprint_d2)

    out = lambda: (_ptr(memory), _ptr(memory_cell), _ptr(cm), _ptr(kind), _ptr(hit))
    untouched = lambda: ((cm == 0xEE).all() and (kind == 0xEE).all() and (hit == -77).all() and (memory == 0x55).all()
                         and (memory_cell == 1).all())
    INVALID, UNSUPPORTED = "(-1)", "(-2)"
    nan, inf = float("nan"), float("inf")
    cases = [(dict(B=-1), INVALID), (dict(Np=0), INVALID), (dict(size_x=0), INVALID), (dict(size_y=-2), INVALID), (dict(world_x=0), INVALID),
             (dict(world_y=-1), INVALID), (dict(resolution=0.0), INVALID), (dict(resolution=-1.0), INVALID), (dict(resolution=nan), INVALID),
             (dict(resolution=inf), INVALID), (dict(n_beams=0), INVALID), (dict(agent_d2=-1), INVALID), (dict(d2_max=-1), INVALID),
             (dict(base=2), INVALID), (dict(world=None), INVALID), (dict(world_origin=None), INVALID), (dict(robot_pose=None), INVALID),
             (dict(people=None), INVALID), (dict(count=None), INVALID), (dict(cell=None), INVALID), (dict(beam_cells=None), INVALID),
             (dict(inflation_cost=None), INVALID), (dict(size_x=257), UNSUPPORTED), (dict(size_y=257), UNSUPPORTED),
             (dict(d2_max=1025), UNSUPPORTED), (dict(n_beams=4097), UNSUPPORTED), (dict(world_x=2 ** 16, world_y=2 ** 15), UNSUPPORTED),
             (dict(mark_d2=-1), INVALID), (dict(footprint_d2=-2), INVALID), (dict(mark_d2=-2 ** 31), INVALID), (dict(footprint_d2=-2 ** 31), INVALID)]
    for kw, code in cases:
        with pytest.raises(SmpcError, match=re.escape(code)):
            solver._call("smpc_obstacle_memory_batch", memory_in(**kw), *out())
        assert untouched(), kw
    for hole in range(3):                                                                     # NULL memory, memory_cell, costmap
        args = list(out())
        args[hole] = None
        with pytest.raises(SmpcError, match=re.escape(INVALID)):
            solver._call("smpc_obstacle_memory_batch", memory_in(), *args)
        assert untouched(), hole
    assert solver.lib.smpc_obstacle_memory_batch(None, memory_in(), *out()) == -1             # NULL handle
    assert solver.lib.smpc_obstacle_memory_batch(solver._h, None, *out()) == -1               # NULL struct
    assert untouched()
    # an empty batch is no refusal and writes nothing, whatever else is in the struct
    solver._call("smpc_obstacle_memory_batch", memory_in(B=0), *out())
    assert untouched()
    # the accepted call runs: the memory 0x55 per row (cells 0, 2, 4, 6; bits beyond column 6 ignored) rolls by (1, 1), the beam
    # along x passes (3, 2) and (4, 2) and hits the wall at (5, 2), the beam along y passes (3, 2), (3, 3), (3, 4)
    solver._call("smpc_obstacle_memory_batch", memory_in(), *out())
    assert kind.tolist() == [[R.WORLD, R.NONE]] and hit.tolist() == [[[2, 0], [0, 2]]] and memory_cell.tolist() == [[0, 0]]
    rows = [0, 0b0101010, 0b0100010, 0b0100010, 0b0100010]                                    # cells 1, 3, 5 of rows 1 .. 4, less the passed ones
    assert memory[0, :, 0].tolist() == rows
    assert np.array_equal(cm[0] == 254, np.array([[(r >> x) & 1 for x in range(7)] for r in rows], bool))
