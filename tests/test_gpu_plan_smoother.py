"""smpc_smooth_plan_batch on the GPU against tests/plan_smoother_ref.py: plan, status, info and change bit for bit on the
hand-made and seeded cases of tests/plan_smoother_cases.py (plans of 3 to 1024 rows at both slot counts of the kernel, one
robot and thirteen, one map for all and a map each on a 96 x 64 world with discs), from host pointers and from device pointers
over sentinel prefill; the rows that must not change against their sentinel pattern; a permuted batch; info, change and range
as NULL; every refusal with sentinel-filled buffers, B == 0 and the accepted call after them."""
import numpy as np
import pytest

import plan_smoother_cases as MC
import plan_smoother_ref as R
from nav2_social_mpc_controller_amd import _abi_plan_smoother as MA
from nav2_social_mpc_controller_amd.params import OptimizerParams

pytestmark = pytest.mark.gpu

HAND = MC.hand_cases()
SEEDED = MC.seeded_cases()
INFO_FILL, STATUS_FILL, CHANGE_FILL = -99, -7, -3.5


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def seeded_ref():
    return {name: R.run(c) for name, c in SEEDED.items()}


def smoother_in(c, B, on_device):
    """The case's scalars as the call's struct (no array pointers yet)."""
    H, W = c["world"].shape[-2:]
    return MA.SmpcPlanSmootherIn(B=B, L=c["plan"].shape[1], on_device=on_device, world_x=W, world_y=H, world_shared=int(c["world"].ndim == 2),
                                 max_its=c["max_its"], refinement_num=c["refinement_num"], lethal_min_cost=c["lethal_min_cost"],
                                 allow_unknown=int(c["allow_unknown"]), resolution=float(c["res"]), w_data=float(c["w_data"]),
                                 w_smooth=float(c["w_smooth"]), tolerance=float(c["tolerance"]))


def rows_of(c, rows):
    """The case with the robots `rows` alone, in that order (a shared map stays shared)."""
    shared = c["world"].ndim == 2
    return dict(c, world=c["world"] if shared else c["world"][rows], origin=c["origin"] if shared else c["origin"][rows], plan=c["plan"][rows],
                plan_len=c["plan_len"][rows], range=None if c["range"] is None else c["range"][rows])


def host_call(solver, c, without=()):
    B = c["plan"].shape[0]
    got = solver.smooth_plan(smoother_in(c, B, 0), c["world"], c["origin"], c["plan"], c["plan_len"], None if "range" in without else c["range"],
                             with_info="info" not in without, with_change="change" not in without)
    return dict(zip(R.OUTPUTS, got))


def device_call(solver, c, without=()):
    """The call on device pointers; status over -7, info over -99, change over -3.5. The arrays named in `without` are NULL."""
    import torch
    from nav2_social_mpc_controller_amd.solver import point
    dev = "cuda:0"
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).copy()).to(dev)
    B = c["plan"].shape[0]
    t = {"world": up(c["world"], np.uint8), "world_origin": up(c["origin"], np.float64), "plan_len": up(c["plan_len"], np.int32)}
    if c["range"] is not None and "range" not in without:
        t["range"] = up(c["range"], np.int32)
    si = point(smoother_in(c, B, 1), t)
    out = {"plan": up(c["plan"], np.float64), "status": torch.full((B,), STATUS_FILL, dtype=torch.int32, device=dev),
           "info": torch.full((B, 4), INFO_FILL, dtype=torch.int32, device=dev), "change": torch.full((B,), CHANGE_FILL, dtype=torch.float64, device=dev)}
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    solver.smooth_plan_device(si, out["plan"].data_ptr(), out["status"].data_ptr(), 0 if "info" in without else out["info"].data_ptr(),
                              0 if "change" in without else out["change"].data_ptr())
    torch.cuda.synchronize()
    solver.set_stream(0)
    del t
    return {k: v.cpu().numpy() for k, v in out.items()}


def differing(got, want):
    """What a failing comparison prints: per output the robots whose entries differ, and the first such robot's status and info."""
    out = []
    for k in R.OUTPUTS:
        if got[k] is not None and got[k].tobytes() != want[k].tobytes():
            bad = [b for b in range(len(want[k])) if got[k][b].tobytes() != want[k][b].tobytes()]
            out.append((k, bad[:8], got["status"][bad[0]], want["status"][bad[0]], None if got["info"] is None else got["info"][bad[0]].tolist(), want["info"][bad[0]].tolist()))
    return out


# ---- against the yardstick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_cases(solver, name):
    c = HAND[name]
    want = R.run(c)
    for got in (host_call(solver, c), device_call(solver, c)):
        assert R.same(got, want), differing(got, want)
        MC.check_want(c, got)


@pytest.mark.parametrize("name", list(SEEDED))
def test_seeded_cases_from_host_and_device_pointers(solver, seeded_ref, name):
    c, want = SEEDED[name], seeded_ref[name]
    for got in (host_call(solver, c), device_call(solver, c)):
        assert R.same(got, want), differing(got, want)
    # the rows that never change, against the case's own pattern (not only against the yardstick's copy of it)
    B, L = c["plan"].shape[:2]
    for b in range(B):
        n = int(c["plan_len"][b])
        lo, hi = (1, n - 2) if c["range"] is None else (max(int(c["range"][b, 0]), 1), min(int(c["range"][b, 1]), n - 2))
        keep = [i for i in range(L) if not lo <= i <= hi]
        assert got["plan"][b, keep].tobytes() == c["plan"][b, keep].tobytes()
        assert (got["plan"][b, n:] <= -1000.0).all()


def test_the_staircase(solver):
    for c in (MC.zigzag_case(), MC.zigzag_case(blocked=MC.ZIGZAG_BLOCKED)):
        want = R.run(c)
        got = device_call(solver, c)
        assert R.same(got, want), differing(got, want)
        assert got["info"][0, 0] > 150 and got["status"][0] == R.CONVERGED


@pytest.mark.parametrize("name", [MC.seeded_name(13, 448, False, 4), MC.seeded_name(13, 1024, True, 5)])
def test_a_permuted_batch_gives_permuted_results(solver, seeded_ref, name):
    c, want = SEEDED[name], seeded_ref[name]
    perm = np.random.default_rng(11).permutation(13)
    got = device_call(solver, rows_of(c, perm))
    assert all(got[k].tobytes() == want[k][perm].tobytes() for k in R.OUTPUTS), differing(got, {k: want[k][perm] for k in R.OUTPUTS})
    few = np.array([12, 3, 7])
    got = host_call(solver, rows_of(c, few))
    assert all(got[k].tobytes() == want[k][few].tobytes() for k in R.OUTPUTS)


def test_optional_arrays_as_null(solver, seeded_ref):
    name = MC.seeded_name(13, 448, True, 3)
    c, want = SEEDED[name], seeded_ref[name]
    got = device_call(solver, c, without=("info", "change"))
    assert got["plan"].tobytes() == want["plan"].tobytes() and got["status"].tobytes() == want["status"].tobytes()
    assert (got["info"] == INFO_FILL).all() and (got["change"] == CHANGE_FILL).all()
    got = host_call(solver, c, without=("info", "change"))
    assert got["info"] is None and got["change"] is None and got["plan"].tobytes() == want["plan"].tobytes()
    free = R.run(dict(c, range=None))
    for got in (device_call(solver, c, without=("range",)), host_call(solver, c, without=("range",))):
        assert R.same(got, free), differing(got, free)
    assert not R.same(free, want)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_alone(solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError, point, _ptr
    c = SEEDED[MC.seeded_name(13, 448, True, 3)]
    B, L = c["plan"].shape[:2]
    arrays = {"world": c["world"], "world_origin": np.ascontiguousarray(c["origin"]), "plan_len": c["plan_len"], "range": c["range"]}

    def attempt(code, outputs=None, **changed):
        si = point(smoother_in(c, B, 0), arrays)
        nulls = [k for k, v in changed.items() if v is None and k in arrays]
        for k, v in changed.items():
            setattr(si, k, v)
        plan, status = c["plan"].copy(), np.full(B, STATUS_FILL, np.int32)
        info, change = np.full((B, 4), INFO_FILL, np.int32), np.full(B, CHANGE_FILL)
        out = dict(dict(plan=plan, status=status, info=info, change=change), **(outputs or {}))
        with pytest.raises(SmpcError) as e:
            solver._call("smpc_smooth_plan_batch", si, _ptr(out["plan"]), _ptr(out["status"]), _ptr(out["info"]), _ptr(out["change"]))
        assert f"failed ({code})" in str(e.value), (changed, nulls, str(e.value))
        assert plan.tobytes() == c["plan"].tobytes() and (status == STATUS_FILL).all() and (info == INFO_FILL).all() and (change == CHANGE_FILL).all()

    INVALID, UNSUPPORTED = -1, -2          # SMPC_ERR_INVALID_ARG, SMPC_ERR_UNSUPPORTED (include/smpc.h)
    for changed in (dict(world=None), dict(world_origin=None), dict(plan_len=None), dict(B=-1), dict(L=1), dict(world_x=0), dict(world_y=0),
                    dict(resolution=0.0), dict(resolution=-0.05), dict(resolution=np.nan), dict(resolution=np.inf),
                    dict(w_data=0.0), dict(w_data=-0.2), dict(w_data=np.nan), dict(w_data=np.inf), dict(w_smooth=-0.1), dict(w_smooth=np.nan),
                    dict(w_smooth=np.inf), dict(w_data=1.0, w_smooth=0.25), dict(w_data=0.2, w_smooth=0.45), dict(tolerance=np.nan),
                    dict(tolerance=-1e-12), dict(max_its=0), dict(refinement_num=-1)):
        attempt(INVALID, **changed)
    attempt(INVALID, outputs=dict(plan=None))
    attempt(INVALID, outputs=dict(status=None))
    for changed in (dict(L=1025), dict(max_its=100001), dict(refinement_num=9), dict(world_x=65536, world_y=32768)):
        attempt(UNSUPPORTED, **changed)
    # B == 0 succeeds and writes nothing; the accepted call after all of them is the yardstick's
    si = point(smoother_in(c, 0, 0), arrays)
    plan, status = c["plan"].copy(), np.full(B, STATUS_FILL, np.int32)
    solver._call("smpc_smooth_plan_batch", si, _ptr(plan), _ptr(status), None, None)
    assert plan.tobytes() == c["plan"].tobytes() and (status == STATUS_FILL).all()
    got, want = host_call(solver, c), R.run(c)
    assert R.same(got, want), differing(got, want)
    # the largest accepted weights and tolerance
    edge = dict(c, w_data=1.0, w_smooth=0.2499, tolerance=np.inf, max_its=3)
    got, want = host_call(solver, edge), R.run(edge)
    assert R.same(got, want) and (want["info"][:, 0][want["status"] == 0] == 3).all()
