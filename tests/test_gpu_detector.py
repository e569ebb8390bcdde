"""smpc_detect_people_batch on the GPU against tests/detector_ref.py, bit for bit in the state (draw_state) and all outputs
(detections, det_count, det_source, outcome), tick by tick with the state fed forward from the device's own output: the
hand-made cases and seeded sequences of tests/detector_cases.py; host against device pointers, two runs, a permuted and a
shorter batch, det_source / outcome NULL, rows beyond det_count untouched, and the refusals."""
import re

import numpy as np
import pytest

import detector_cases as DC
from nav2_social_mpc_controller_amd import _abi_detector as DA
from nav2_social_mpc_controller_amd.params import DetectorParams, OptimizerParams

pytestmark = pytest.mark.gpu

HAND = DC.hand_cases()
SEEDED = DC.seeded_cases()


def case_of(name):
    return HAND[name] if name in HAND else SEEDED[name]


def reference(name):
    return case_of(name)["p"], DC.reference(name, case_of(name))


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


def detector_in(p, B, Np, on_device):
    """The yardstick's scalars in the call's struct; where the case was made from DetectorParams' own arguments, through
    BatchSolver.detector_c, which must form the same thresholds and scales."""
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    di = BatchSolver.detector_c(DetectorParams(**p["given"]), B, Np, p["Nd"], on_device)
    assert (di.noise_scale, di.noise_growth, di.clutter_scale, di.body_radius) == tuple(float(p[k]) for k in ("noise_scale", "noise_growth", "clutter_scale", "body_radius"))
    assert (di.seed_lo, di.seed_hi, di.Kc) == (p["seed_lo"], p["seed_hi"], p["Kc"])
    thresholds = (di.miss_threshold, di.clutter_threshold)
    di.miss_threshold, di.clutter_threshold = p["miss_threshold"], p["clutter_threshold"]    # a hand-made case may set them directly
    if thresholds != (p["miss_threshold"], p["clutter_threshold"]):
        assert p["miss_threshold"] in (0, DC.ALL, thresholds[0]) and p["clutter_threshold"] in (0, DC.ALL, thresholds[1])
    return di


def host_call(solver, state, tick, p, rows=None, with_source=True, with_outcome=True):
    from nav2_social_mpc_controller_amd.solver import _ptr, point
    rows = slice(None) if rows is None else rows
    people = np.ascontiguousarray(tick["people"][rows], np.float64)
    count, pose = np.ascontiguousarray(tick["count"][rows], np.int32), np.ascontiguousarray(tick["pose"][rows], np.float64)
    B, Np, Nd = people.shape[0], people.shape[1], p["Nd"]
    di = point(detector_in(p, B, Np, 0), {"people": people, "count": count, "robot_pose": pose})
    new = np.array(state[rows], np.uint32, order="C")
    det, det_count = np.full((B, Nd, 5), np.nan), np.full(B, -9, np.int32)
    source, outcome = np.full((B, Nd), -99, np.int32), np.full((B, Np), 255, np.uint8)
    solver._call("smpc_detect_people_batch", di, _ptr(new), _ptr(det), _ptr(det_count), _ptr(source) if with_source else None,
                 _ptr(outcome) if with_outcome else None)
    return new, (det, det_count, source, outcome)


def device_call(solver, state, tick, p, with_source=True, with_outcome=True):
    import torch
    from nav2_social_mpc_controller_amd.solver import point
    dev = "cuda:0"
    people = np.ascontiguousarray(tick["people"], np.float64)
    B, Np, Nd = people.shape[0], people.shape[1], p["Nd"]
    t = {"people": torch.from_numpy(people.copy()).to(dev), "count": torch.from_numpy(np.ascontiguousarray(tick["count"], np.int32).copy()).to(dev),
         "robot_pose": torch.from_numpy(np.ascontiguousarray(tick["pose"], np.float64).copy()).to(dev)}
    di = point(detector_in(p, B, Np, 1), t)
    draw_state = torch.from_numpy(np.array(state, np.uint32).view(np.int32)).to(dev)
    det = torch.full((B, Nd, 5), float("nan"), dtype=torch.float64, device=dev)
    det_count = torch.full((B,), -9, dtype=torch.int32, device=dev)
    source = torch.full((B, Nd), -99, dtype=torch.int32, device=dev)
    outcome = torch.full((B, Np), 255, dtype=torch.uint8, device=dev)
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    solver.detect_people_device(di, draw_state.data_ptr(), det.data_ptr(), det_count.data_ptr(), source.data_ptr() if with_source else 0,
                                outcome.data_ptr() if with_outcome else 0)
    torch.cuda.synchronize()
    solver.set_stream(0)
    return draw_state.cpu().numpy().view(np.uint32), (det.cpu().numpy(), det_count.cpu().numpy(), source.cpu().numpy(), outcome.cpu().numpy())


def where(got, want):
    """The arrays (0: the state, 1 - 4: the outputs) that differ."""
    return [k for k, (g, w) in enumerate(zip([got[0]] + list(got[1]), [want[0]] + list(want[1]))) if np.asarray(g).tobytes() != np.asarray(w).tobytes()]


# ---- against the yardstick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND) + sorted(SEEDED))
def test_state_and_outputs_are_the_yardsticks_tick_by_tick_from_the_devices_own_state(solver, name):
    """The yardstick leaves NaN / -99 / 255 where the rule writes nothing, as the sentinel-filled device buffers do: bit
    equality of whole arrays is also "rows beyond det_count and outcomes beyond the count untouched"."""
    p, ticks = reference(name)
    state = ticks[0][1]
    for t, (tick, before, new, outs, _) in enumerate(ticks):
        assert np.asarray(state).tobytes() == before.tobytes(), (name, t)                      # the device's state is the yardstick's
        got = device_call(solver, state, tick, p)
        assert DC.same(got, (new, outs)), (name, t, where(got, (new, outs)))
        if tick["want"] is not None:
            DC.check_want(got[0], got[1], tick["want"])
        state = got[0]
    # the last tick again: from host pointers, and twice from the same state
    host = host_call(solver, before, tick, p)
    assert DC.same(host, (new, outs)), (name, where(host, (new, outs)))
    assert DC.same(device_call(solver, before, tick, p), got) and DC.same(host_call(solver, before, tick, p), host)


@pytest.mark.parametrize("name", ["3x4x2_B67", "8x8x4_B67", "64x64x64_B5"])
def test_a_robots_rows_do_not_depend_on_the_batch(solver, name):
    """A permuted batch with permuted draw_state gives permuted results; so do one robot alone and every other robot."""
    p, ticks = reference(name)
    tick, before, new, outs, _ = ticks[-1]
    B = len(tick["count"])
    take = lambda pair, rows: (pair[0][rows], tuple(a[rows] for a in pair[1]))
    perm = np.random.default_rng(B).permutation(B)
    for rows in (perm, [B - 1], list(range(0, B, 2))):
        got = host_call(solver, before, tick, p, rows)
        assert DC.same(got, take((new, outs), rows)), where(got, take((new, outs), rows))


def test_det_source_and_outcome_null(solver):
    for name in ("8x8x4_B67", "nan_person", "nan_pose"):
        p, ticks = reference(name)
        tick, before, new, outs, _ = ticks[-1]
        for call in (device_call, host_call):
            for with_source, with_outcome in ((False, True), (True, False), (False, False)):
                state, (det, det_count, source, outcome) = call(solver, before, tick, p, with_source=with_source, with_outcome=with_outcome)
                assert with_source or (source == -99).all()
                assert with_outcome or (outcome == 255).all()
                got = (state, (det, det_count, source if with_source else outs[2], outcome if with_outcome else outs[3]))
                assert DC.same(got, (new, outs)), (name, with_source, with_outcome)


def test_the_solvers_host_method_returns_the_new_state_beside_the_outputs(solver):
    p, ticks = reference("8x8x4_B5")
    tick, before, new, outs, _ = ticks[3]
    keep = before.copy()
    det, det_count, source, outcome, state = solver.detect_people(DetectorParams(**p["given"]), before, tick["people"], tick["count"], tick["pose"], Nd=p["Nd"])
    assert DC.same((state, (det, det_count, source, outcome)), (new, outs)) and before.tobytes() == keep.tobytes()
    det, det_count, source, outcome, state = solver.detect_people(DetectorParams(**p["given"]), before, tick["people"], tick["count"], tick["pose"],
                                                                  Nd=p["Nd"], with_source=False, with_outcome=False)
    assert source is None and outcome is None and DC.same((state, (det, det_count, None, None)), (new, outs))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_every_buffer_alone(solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError, _ptr
    people = np.array([[[1.0, 0.0, 0.5, 0.0, 0.0], [2.0, 0.0, 0.0, 0.5, 1.0]]])
    count, pose = np.array([2], np.int32), np.zeros((1, 3))
    state, det, det_count = np.array([[5, 9]], np.uint32), np.full((1, 3, 5), 7.5), np.full(1, -9, np.int32)
    source, outcome = np.full((1, 3), -99, np.int32), np.full((1, 2), 255, np.uint8)

    def detector_in(**kw):
        di = DA.SmpcDetectorIn(B=1, Np=2, Nd=3, Kc=1, on_device=0, seed_lo=1, seed_hi=2, miss_threshold=0, clutter_threshold=0, body_radius=0.25,
                               noise_scale=0.0, noise_growth=0.0, clutter_scale=1.0, people=_ptr(people), count=_ptr(count), robot_pose=_ptr(pose))
        for k, v in kw.items():
            setattr(di, k, v)
        return di

    out = lambda: (_ptr(state), _ptr(det), _ptr(det_count), _ptr(source), _ptr(outcome))
    untouched = lambda: (state.tolist() == [[5, 9]] and (det == 7.5).all() and (det_count == -9).all() and (source == -99).all()
                         and (outcome == 255).all())
    INVALID, UNSUPPORTED = "(-1)", "(-2)"
    nan, inf = float("nan"), float("inf")
    cases = [(dict(B=-1), INVALID), (dict(Np=0), INVALID), (dict(Nd=0), INVALID), (dict(Np=-2), INVALID), (dict(Kc=-1), INVALID),
             (dict(people=None), INVALID), (dict(count=None), INVALID), (dict(robot_pose=None), INVALID),
             (dict(Np=65), UNSUPPORTED), (dict(Nd=65), UNSUPPORTED), (dict(Kc=65), UNSUPPORTED)]
    cases += [({k: v}, INVALID) for k in ("body_radius", "noise_scale", "noise_growth", "clutter_scale") for v in (-0.5, nan, inf, -inf)]
    for kw, code in cases:
        with pytest.raises(SmpcError, match=re.escape(code)):
            solver._call("smpc_detect_people_batch", detector_in(**kw), *out())
        assert untouched(), kw
    for hole in range(3):                                                                        # NULL draw_state, detections, det_count
        args = list(out())
        args[hole] = None
        with pytest.raises(SmpcError, match=re.escape(INVALID)):
            solver._call("smpc_detect_people_batch", detector_in(), *args)
        assert untouched(), hole
    assert solver.lib.smpc_detect_people_batch(None, detector_in(), *out()) == -1                # NULL handle
    assert solver.lib.smpc_detect_people_batch(solver._h, None, *out()) == -1                    # NULL struct
    assert untouched()
    solver._call("smpc_detect_people_batch", detector_in(B=0), *out())                           # an empty batch is no refusal and writes nothing
    assert untouched()
    # the accepted call runs: the rear person is hidden, the front one is copied bit for bit, the counter advances
    solver._call("smpc_detect_people_batch", detector_in(), *out())
    assert state.tolist() == [[5, 10]] and det_count.tolist() == [1] and outcome.tolist() == [[0, 1]] and source.tolist() == [[0, -99, -99]]
    assert det.tolist() == [[[1.0, 0.0, 0.5, 0.0, 0.0], [7.5] * 5, [7.5] * 5]] and solver.last_kernel_ms() > 0.0
