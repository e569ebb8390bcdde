"""smpc_track_people_batch on the GPU against tests/tracker_ref.py, bit for bit in the state (tracks, track_meta, next_id)
and all outputs (people, count, out_track), tick by tick with the state fed forward from the device's own output: the
hand-made and seeded sequences of tests/tracker_cases.py and the (64, 64, 64) limit with all 64 detections inside every
gate (the longest association); host against device pointers, two runs, a permuted and a shorter batch, out_track NULL,
unaligned detections, and the refusals."""
import re

import numpy as np
import pytest

import tracker_cases as TC
from nav2_social_mpc_controller_amd import _abi_tracker as TA
from nav2_social_mpc_controller_amd.params import OptimizerParams, TrackerParams

pytestmark = pytest.mark.gpu

HAND = TC.hand_sequences()
SEEDED = TC.seeded_sequences()
BIG = {"dense_limit": TC.dense_limit_sequence}
_cache = {}


def sequence(name):
    return HAND[name] if name in HAND else SEEDED[name] if name in SEEDED else BIG[name]()


def reference(name):
    """The yardstick's ticks of a sequence, computed once: (p, [(tick, state before, new state, outputs)])."""
    if name not in _cache:
        seq = sequence(name)
        ticks = [(tick, before, new, outs) for _, tick, before, new, outs in TC.run(seq, TC.ref_call)]
        for tick, before, new, outs in ticks:
            for a in list(before) + list(new) + list(outs) + [tick["det"], tick["count"], tick["pose"]]:
                a.setflags(write=False)
        _cache[name] = (seq["p"], ticks)
    return _cache[name]


def tracker_params(p):
    """The yardstick's scalars as the library's caller states them; gain(dt) forms beta / dt as the yardstick does."""
    tp = TrackerParams(alpha=float(p["alpha"]), beta=float(p["beta"]), gate=float(p["gate"]), confirm_hits=p["confirm_hits"],
                       max_missed=p["max_missed"], slots=p["Nt"])
    assert tp.gain(float(p["dt"])) == float(p["gain"])
    return tp


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


def host_call(solver, state, tick, p, rows=None, with_out_track=True):
    rows = slice(None) if rows is None else rows
    people, count, source, tracks, meta, next_id = solver.track_people(
        tracker_params(p), float(p["dt"]), state[0][rows], state[1][rows], state[2][rows], tick["det"][rows], tick["count"][rows],
        tick["pose"][rows], Np=p["Np"], with_out_track=with_out_track)
    return (tracks, meta, next_id), (people, count, source)


def device_call(solver, state, tick, p, offset=0, with_out_track=True):
    """The call on device pointers; the detections start `offset` bytes into their allocation."""
    import torch
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point
    dev = "cuda:0"
    det = np.ascontiguousarray(tick["det"], np.float64)
    B, Nd, Nt, Np = det.shape[0], det.shape[1], p["Nt"], p["Np"]
    raw = torch.zeros(det.nbytes + offset, dtype=torch.uint8, device=dev)
    raw[offset:] = torch.from_numpy(det.view(np.uint8).reshape(-1).copy()).to(dev)
    t = {"det_count": torch.from_numpy(np.ascontiguousarray(tick["count"], np.int32).copy()).to(dev),
         "robot_pose": torch.from_numpy(np.ascontiguousarray(tick["pose"], np.float64).copy()).to(dev)}
    ti = point(BatchSolver.tracker_c(tracker_params(p), B, Nd, Np, float(p["dt"]), 1), t)
    ti.detections = raw.data_ptr() + offset
    tracks = torch.from_numpy(np.array(state[0], np.float64)).to(dev)
    meta = torch.from_numpy(np.array(state[1], np.int32)).to(dev)
    next_id = torch.from_numpy(np.array(state[2], np.int32)).to(dev)
    people = torch.full((B, Np, 5), float("nan"), dtype=torch.float64, device=dev)
    count = torch.full((B,), -9, dtype=torch.int32, device=dev)
    source = torch.full((B, Np, 2), -1, dtype=torch.int32, device=dev)
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    solver.track_people_device(ti, tracks.data_ptr(), meta.data_ptr(), next_id.data_ptr(), people.data_ptr(), count.data_ptr(),
                               source.data_ptr() if with_out_track else 0)
    torch.cuda.synchronize()
    solver.set_stream(0)
    return (tracks.cpu().numpy(), meta.cpu().numpy(), next_id.cpu().numpy()), (people.cpu().numpy(), count.cpu().numpy(), source.cpu().numpy())


def where(got, want):
    """The arrays (0 - 2: the state, 3 - 5: the outputs) that differ."""
    return [k for k, (g, w) in enumerate(zip(list(got[0]) + list(got[1]), list(want[0]) + list(want[1])))
            if np.asarray(g).tobytes() != np.asarray(w).tobytes()]


# ---- against the yardstick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND) + sorted(SEEDED) + sorted(BIG))
def test_state_and_outputs_are_the_yardsticks_tick_by_tick_from_the_devices_own_state(solver, name):
    p, ticks = reference(name)
    state = ticks[0][1]
    for t, (tick, before, new, outs) in enumerate(ticks):
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(state, before)), (name, t)   # the device's state is the yardstick's
        got = device_call(solver, state, tick, p)
        assert TC.same(got, (new, outs)), (name, t, where(got, (new, outs)))
        if tick["want"] is not None:
            TC.check_want(got[0], got[1], tick["want"])
        state = got[0]
    # the last tick again: from host pointers, and twice from the same state
    host = host_call(solver, before, tick, p)
    assert TC.same(host, (new, outs)), (name, where(host, (new, outs)))
    assert TC.same(device_call(solver, before, tick, p), got) and TC.same(host_call(solver, before, tick, p), host)


@pytest.mark.parametrize("name", ["3x8x2_B67", "16x8x8_B67", "64x64x64_B5"])
def test_a_robots_rows_do_not_depend_on_the_batch(solver, name):
    p, ticks = reference(name)
    tick, before, new, outs = ticks[-1]
    B = len(tick["count"])
    take = lambda pair, rows: (tuple(a[rows] for a in pair[0]), tuple(a[rows] for a in pair[1]))
    perm = np.random.default_rng(B).permutation(B)
    for rows in (perm, [B - 1], list(range(0, B, 2))):
        got = host_call(solver, before, tick, p, rows)
        assert TC.same(got, take((new, outs), rows)), where(got, take((new, outs), rows))


def test_out_track_null_and_unaligned_detections(solver):
    for name in ("16x8x8_B67", "crossing_greedy"):
        p, ticks = reference(name)
        tick, before, new, outs = ticks[-1]
        for offset in (8, 24):                                                                   # doubles, but no 16- or 32-byte boundary
            assert TC.same(device_call(solver, before, tick, p, offset=offset), (new, outs))
        state, (people, count, source) = device_call(solver, before, tick, p, with_out_track=False)
        assert (source == -1).all() and TC.same((state, (people, count, outs[2])), (new, outs))
        state, (people, count, source) = host_call(solver, before, tick, p, with_out_track=False)
        assert source is None and TC.same((state, (people, count, outs[2])), (new, outs))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_every_buffer_alone(solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError, _ptr
    det, det_count, pose = np.array([[[1.0, 1.0, 0.0, 0.0, 0.0], [2.0, 2.0, 0.0, 0.0, 0.0]]]), np.array([2], np.int32), np.zeros((1, 3))
    tracks, meta, next_id = np.full((1, 3, 4), 0.5), np.full((1, 3, 4), 9, np.int32), np.full(1, 5, np.int32)
    people, count, source = np.full((1, 2, 5), 7.5), np.full(1, -9, np.int32), np.full((1, 2, 2), -1, np.int32)

    def tracker_in(**kw):
        ti = TA.SmpcTrackerIn(B=1, Nd=2, Nt=3, Np=2, on_device=0, confirm_hits=1, max_missed=2, dt=0.1, alpha=0.5, gain=2.0, gate=0.6,
                              detections=_ptr(det), det_count=_ptr(det_count), robot_pose=_ptr(pose))
        for k, v in kw.items():
            setattr(ti, k, v)
        return ti

    out = lambda: (_ptr(tracks), _ptr(meta), _ptr(next_id), _ptr(people), _ptr(count), _ptr(source))
    untouched = lambda: ((tracks == 0.5).all() and (meta == 9).all() and (next_id == 5).all() and (people == 7.5).all()
                         and (count == -9).all() and (source == -1).all())
    INVALID, UNSUPPORTED = "(-1)", "(-2)"
    nan, inf = float("nan"), float("inf")
    cases = [(dict(B=-1), INVALID), (dict(Nd=0), INVALID), (dict(Nt=0), INVALID), (dict(Np=0), INVALID), (dict(Nd=-3), INVALID),
             (dict(confirm_hits=0), INVALID), (dict(max_missed=-1), INVALID), (dict(dt=0.0), INVALID), (dict(dt=-0.1), INVALID),
             (dict(dt=nan), INVALID), (dict(dt=inf), INVALID), (dict(alpha=-0.5), INVALID), (dict(alpha=nan), INVALID), (dict(alpha=inf), INVALID),
             (dict(gain=-1.0), INVALID), (dict(gain=nan), INVALID), (dict(gain=inf), INVALID), (dict(gate=0.0), INVALID), (dict(gate=-1.0), INVALID),
             (dict(gate=nan), INVALID), (dict(gate=inf), INVALID), (dict(detections=None), INVALID), (dict(det_count=None), INVALID),
             (dict(robot_pose=None), INVALID), (dict(Nd=65), UNSUPPORTED), (dict(Nt=65), UNSUPPORTED), (dict(Np=65), UNSUPPORTED)]
    for kw, code in cases:
        with pytest.raises(SmpcError, match=re.escape(code)):
            solver._call("smpc_track_people_batch", tracker_in(**kw), *out())
        assert untouched(), kw
    for hole in range(5):                                                                        # NULL tracks, track_meta, next_id, people, count
        args = list(out())
        args[hole] = None
        with pytest.raises(SmpcError, match=re.escape(INVALID)):
            solver._call("smpc_track_people_batch", tracker_in(), *args)
        assert untouched(), hole
    assert solver.lib.smpc_track_people_batch(None, tracker_in(), *out()) == -1                  # NULL handle
    assert solver.lib.smpc_track_people_batch(solver._h, None, *out()) == -1                     # NULL struct
    assert untouched()
    solver._call("smpc_track_people_batch", tracker_in(B=0), *out())                             # an empty batch is no refusal and writes nothing
    assert untouched()
    # the accepted call runs: the garbage state (state 9) is freed, both detections are born, confirmed at once
    solver._call("smpc_track_people_batch", tracker_in(), *out())
    assert meta.tolist() == [[[2, 1, 0, 5], [2, 1, 0, 6], [0, 0, 0, 0]]] and next_id.tolist() == [7] and count.tolist() == [2]
    assert tracks.tolist() == [[[1.0, 1.0, 0.0, 0.0], [2.0, 2.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]] and source.tolist() == [[[0, 5], [1, 6]]]
    assert people.tolist() == [[[1.0, 1.0, 0.0, 0.0, 0.0], [2.0, 2.0, 0.0, 0.0, 0.0]]] and solver.last_kernel_ms() > 0.0
