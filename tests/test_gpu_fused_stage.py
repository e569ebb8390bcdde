"""Staging at the scene fetch (`-m gpu`): a solve of the headline shape on reference-layout people runs
smpc_solve_fixed_kernel alone, and every slot stages the people block of the scene it fetches (csrc/smpc_sweep.hpp
load_scene(), csrc/smpc_stage.hpp). All nine result arrays must be, bit for bit, those of

  (b) the same handle given the records of stage_people_device: the fixed-shape kernel, reading a staged block;
  (c) smpc_set_fixed_shapes(h, 0): the run-time-shape kernel behind the staging kernel.

The fixed-shape kernel is picked above the one-scene-per-wave threshold only, which is read from the library
(smpc_solve_shape_is_fixed), so the batches are: one scene past the threshold (most slots of the grid never get a scene),
and as many as the grid has slots plus 104, so that 104 slots fetch a second scene after a first one has used the
record buffer and the CU's cache. The scenes: some without people, agents invalid at some steps, a scene with a standing
person within 2 m and a tag, a scene with nobody within 2 m and no tag at any step."""
import numpy as np
import pytest

from nav2_social_mpc_controller_amd._abi import SmpcSceneBatch
from nav2_social_mpc_controller_amd.params import OptimizerParams
from nav2_social_mpc_controller_amd.scenes import make_scenes

pytestmark = pytest.mark.gpu

README = OptimizerParams.readme()
T, N = 28, 8
KEYS = ("params", "cmds", "path", "status", "reason", "iterations", "evaluations", "initial_cost", "final_cost")
NO_TARGET = 1e300
SMPC_NOT_SOLVED = -1


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(README)
    yield s
    s.close()


@pytest.fixture(scope="module")
def sizes(solver):
    """(one past the threshold, slots of the grid + 104): the threshold is the largest batch that still runs one scene per
    wave, and a lone launch above it takes that many waves of two slots."""
    if not solver.solve_shape_is_fixed(1 << 20, T, N):
        pytest.skip("no fixed-shape solve kernel for this shape on this device")
    lo, hi = 1, 1 << 20  # smallest B that runs the fixed-shape kernel
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if solver.solve_shape_is_fixed(mid, T, N) else (mid + 1, hi)
    return lo, 2 * (lo - 1) + 104


@pytest.fixture(scope="module")
def pool(solver):
    """1024 different scenes the batches are drawn from, with the cases the staging rules branch on."""
    sc = make_scenes(README, 1024, N, T=T, seed=2811, map_cells=80, standing_fraction=0.25)
    sc.has_people[::41] = 0
    sc.people[3::7, 5:19, 3, 2] = -1.0     # agent 2 invalid at steps 5..18
    sc.people[5::11, :, 3, 6:] = -1.0      # agents 6, 7 never valid
    sc.people[9, 1:, 3, :] = -1.0          # a scene with people and no valid agent at any step
    p0 = sc.pose0
    # scene 1 (heading 0): a standing person 1 m ahead, who gives no tag, and one walking alongside 1.5 m to the right, who
    # is the nearest moving agent and gives one at every step
    p0[1, 2] = 0.0
    sc.people[1, :, 0, 0], sc.people[1, :, 1, 0], sc.people[1, :, 4, 0] = p0[1, 0] + 1.0, p0[1, 1], 0.0
    sc.people[1, :, 0, 1] = p0[1, 0] + 0.01 * np.arange(T + 1)
    sc.people[1, :, 1, 1], sc.people[1, :, 2, 1], sc.people[1, :, 4, 1] = p0[1, 1] - 1.5, 0.0, 0.2
    ang = np.linspace(0.0, 2 * np.pi, N, endpoint=False)
    sc.people[1, :, 0, 2:], sc.people[1, :, 1, 2:] = p0[1, 0] + 3.0 * np.cos(ang[2:]), p0[1, 1] + 3.0 * np.sin(ang[2:])
    sc.people[1, :, 4, 2:] = 0.0           # the others stand 3 m away
    # scene 2: everybody at least 2.5 m away: no tag at any step
    sc.people[2, :, 0, :] = p0[2, 0] + 2.5 * np.cos(ang) + 0.02 * np.cos(ang) * np.arange(T + 1)[:, None]
    sc.people[2, :, 1, :] = p0[2, 1] + 2.5 * np.sin(ang) + 0.02 * np.sin(ang) * np.arange(T + 1)[:, None]
    sc.people[2, :, 2, :], sc.people[2, :, 4, :] = ang, 0.4
    sc.has_people[1:3] = 1
    _, aux = solver.stage_people(sc.select(np.arange(16)))
    assert (aux[1, :, 1] != NO_TARGET).all() and (aux[2, :, 1] == NO_TARGET).all()
    return sc


def batch(pool, B, shift=0):
    return pool.select((np.arange(B) + shift) % pool.B)


def run(s, sb, B, order=None):
    """One solve on device pointers into outputs of a known fill; the nine arrays as numpy."""
    import torch
    rb, rt = s.alloc_results(B, T)
    for v in rt.values():
        v.fill_(-3)
    if order is not None:
        sb = SmpcSceneBatch.from_buffer_copy(sb)
        sb.order = order.data_ptr()
    s.solve_device(sb, rb)
    torch.cuda.synchronize()
    return {k: rt[k].cpu().numpy() for k in KEYS}


def same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)


def reference(s, sb, B, order=None):
    """(c): the run-time-shape kernel behind the staging kernel."""
    s.set_fixed_shapes(False)
    assert not s.solve_shape_is_fixed(B, T, N)
    try:
        return run(s, sb, B, order)
    finally:
        s.set_fixed_shapes(True)


@pytest.fixture(scope="module")
def cases(solver, pool, sizes):
    """Per batch size: the device batch and its reference (c), computed once."""
    out = {}
    for name, B in zip(("small", "big"), sizes):
        sb, keep = batch(pool, B).to_device()
        out[name] = (B, sb, keep, reference(solver, sb, B))
    return out


@pytest.mark.parametrize("which", ["small", "big"])
def test_fused_staged_and_plain_solves_are_bit_equal(solver, cases, which):
    B, sb, _keep, plain = cases[which]
    assert solver.solve_shape_is_fixed(B, T, N) and solver.solve_slot_width(B, T, N) == 32
    fused = run(solver, sb, B)
    sb_staged = SmpcSceneBatch.from_buffer_copy(sb)
    _keep2 = solver.stage_people_device(sb_staged)
    staged = run(solver, sb_staged, B)
    same(fused, plain, "fused against the run-time-shape kernel")
    same(fused, staged, "fused against the fixed-shape kernel on a staged block")
    assert (fused["status"] >= 0).all() and (fused["evaluations"] > 1).any()
    assert len(np.unique(fused["evaluations"])) > 4  # the batch is not one scene many times over


def test_a_second_batch_on_the_handle_is_its_own(solver, pool, cases):
    """Two different batches back to back: the second one's records replace the first one's, scene by scene, as the
    slots fetch them. Records left over from the first launch would show as the first batch's results."""
    B, sb1, _keep, ref1 = cases["big"]
    sb2, _keep2 = batch(pool, B, shift=517).to_device()
    ref2 = reference(solver, sb2, B)
    assert not np.array_equal(ref1["cmds"], ref2["cmds"])
    first = run(solver, sb1, B)
    second = run(solver, sb2, B)
    same(first, ref1, "first batch")
    same(second, ref2, "second batch")


def test_a_device_order_changes_nothing(solver, cases):
    import torch
    B, sb, _keep, plain = cases["big"]
    order = torch.from_numpy(np.random.default_rng(7).permutation(B).astype(np.int32)).to("cuda:0")
    same(run(solver, sb, B, order), plain, "permuted order")


def test_scenes_a_device_order_leaves_out_stay_unsolved(solver, cases):
    import torch
    B, sb, _keep, _ = cases["big"]
    o = np.random.default_rng(8).permutation(B).astype(np.int32)
    left_out = o[[3, 500, B - 1]].copy()
    o[3], o[500], o[B - 1] = B + 1000, -5, B       # entries outside the batch: skipped
    order = torch.from_numpy(o).to("cuda:0")
    fused = run(solver, sb, B, order)
    same(fused, reference(solver, sb, B, order), "order with entries left out")
    assert (fused["status"][left_out] == SMPC_NOT_SOLVED).all()
    assert (np.delete(fused["status"], left_out) >= 0).all()
    assert (fused["cmds"][left_out] == -3).all()  # untouched: still the fill
