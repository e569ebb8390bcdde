"""smpc_repair_plan_batch on the GPU against tests/plan_repair_ref.py: plan, plan_len, status, info and field byte for byte on
the hand-made and seeded cases of tests/plan_repair_cases.py (regions of 3 x 3 to 127 x 127 cells, plans of 9 to 400 rows),
from device pointers over NaN and sentinel prefill, from host pointers, and twice; a permuted, a one-robot and an
every-other-robot batch; info, field and plan_start as NULL; plan, workspace and field rows at 8-byte but not 16-byte addresses;
every refusal with sentinel-filled buffers, B == 0 and the accepted call after them."""
import numpy as np
import pytest

import plan_repair_cases as MC
import plan_repair_ref as R
from nav2_social_mpc_controller_amd import _abi_plan_repair as MA
from nav2_social_mpc_controller_amd.params import OptimizerParams

pytestmark = pytest.mark.gpu

HAND = MC.hand_cases()
SEEDED = MC.seeded_cases()
OUTPUTS = ("plan", "plan_len", "status", "info", "field")
FIELD_FILL, INFO_FILL = 0xABCD1234, -99


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def seeded_ref():
    return {name: reference(c) for name, c in SEEDED.items()}


def reference(c, info=None, field=None):
    B, S = len(c["pose"]), 2 * c["R"] + 1
    return R.run(c, info=np.full((B, 4), INFO_FILL, np.int32) if info is None else info,
                 field=np.full((B, S, S), FIELD_FILL, np.uint32) if field is None else field)


def repair_in(c, B, on_device):
    """The case's scalars as the call's struct (no array pointers yet)."""
    H, W = c["costmap"].shape[-2:]
    ri = MA.SmpcPlanRepairIn(B=B, L=c["plan"].shape[1], on_device=on_device, size_x=W, size_y=H, costmap_shared=int(c["costmap"].ndim == 2),
                             radius=c["R"], stride=c["stride"], resolution=float(c["res"]), clearance_d2=float(c["clearance_d2"]))
    cost = c["cost"]
    ri.cost.neutral_cost, ri.cost.cost_weight, ri.cost.lethal_min_cost, ri.cost.allow_unknown = cost.neutral_cost, cost.cost_weight, cost.lethal_min_cost, int(cost.allow_unknown)
    return ri


def rows_of(c, rows):
    """The case with the robots `rows` alone (a shared costmap stays shared)."""
    if rows is None:
        return c
    shared = c["costmap"].ndim == 2
    return dict(c, costmap=c["costmap"] if shared else c["costmap"][rows], origin=c["origin"] if shared else c["origin"][rows], pose=c["pose"][rows],
                plan=c["plan"][rows], plan_len=c["plan_len"][rows], plan_start=None if c["plan_start"] is None else c["plan_start"][rows])


def host_call(solver, c, rows=None, without=()):
    c = rows_of(c, rows)
    B, S = len(c["pose"]), 2 * c["R"] + 1
    start = None if "plan_start" in without else c["plan_start"]
    got = solver.repair_plan(repair_in(c, B, 0), c["costmap"], c["origin"], c["pose"], c["plan"], c["plan_len"], plan_start=start,
                             with_info="info" not in without, field=None if "field" in without else np.full((B, S, S), FIELD_FILL, np.uint32))
    return dict(zip(OUTPUTS, got))


def device_call(solver, c, without=(), skew=False):
    """The call on device pointers; info over -99, field over a sentinel, status over -7, the workspace NaN. The arrays named in
    `without` are passed as NULL. skew: plan, workspace and field start 8 (4) bytes into 16-byte aligned allocations."""
    import torch
    from nav2_social_mpc_controller_amd.solver import point
    dev = "cuda:0"
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).copy()).to(dev)
    B, L = c["plan"].shape[:2]
    S = 2 * c["R"] + 1
    pad = 1 if skew else 0
    plan = torch.zeros(pad + B * L * 2, dtype=torch.float64, device=dev)
    plan[pad:] = up(c["plan"], np.float64).reshape(-1)
    ws = torch.full((pad + B * L * 2,), float("nan"), dtype=torch.float64, device=dev)
    field = torch.from_numpy(np.full(2 * pad + B * S * S, FIELD_FILL, np.uint32).view(np.int32)).to(dev)
    t = {"costmap": up(c["costmap"], np.uint8), "costmap_origin": up(c["origin"], np.float64), "robot_pose": up(c["pose"], np.float64)}
    if c["plan_start"] is not None and "plan_start" not in without:
        t["plan_start"] = up(c["plan_start"], np.int32)
    if skew:
        assert plan[pad:].data_ptr() % 16 == 8 and ws[pad:].data_ptr() % 16 == 8 and field[2 * pad:].data_ptr() % 16 == 8
    ri = point(repair_in(c, B, 1), t)
    out = {"plan": plan[pad:], "plan_len": up(c["plan_len"], np.int32), "status": torch.full((B,), -7, dtype=torch.int32, device=dev),
           "info": torch.full((B, 4), INFO_FILL, dtype=torch.int32, device=dev), "field": field[2 * pad:]}
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    solver.repair_plan_device(ri, out["plan"].data_ptr(), out["plan_len"].data_ptr(), ws[pad:].data_ptr(), out["status"].data_ptr(),
                              0 if "info" in without else out["info"].data_ptr(), 0 if "field" in without else out["field"].data_ptr())
    torch.cuda.synchronize()
    solver.set_stream(0)
    del t
    got = {k: None if k in without else v.cpu().numpy() for k, v in out.items()}
    got["plan"] = got["plan"].reshape(B, L, 2)
    if got["field"] is not None:
        got["field"] = got["field"].view(np.uint32).reshape(B, S, S)
    assert pad == 0 or (plan[0].item() == 0.0 and np.isnan(ws[0].item()) and field[:2].cpu().numpy().view(np.uint32).tolist() == [FIELD_FILL] * 2)
    return got


def equal(a, b, keys=OUTPUTS):
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and a[k].tobytes() == b[k].tobytes()) for k in keys)


def differing(got, want):
    """What a failing comparison prints: per output the robots whose rows differ, and the first such robot's status and info."""
    out = []
    for k in OUTPUTS:
        if got[k] is not None and got[k].tobytes() != want[k].tobytes():
            bad = [b for b in range(len(want[k])) if got[k][b].tobytes() != want[k][b].tobytes()]
            out.append((k, bad[:8], int(got["status"][bad[0]]), int(want["status"][bad[0]]), want["info"][bad[0]].tolist()))
    return out


# ---- against the yardstick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_the_kernels_are_the_yardstick_on_the_hand_made_cases(solver, name):
    c = HAND[name]
    got, want = device_call(solver, c), reference(c)
    assert R.same(got, want), differing(got, want)
    MC.check_want(c, got)
    host = host_call(solver, c)
    assert equal(host, got), differing(host, got)
    assert equal(device_call(solver, c), got) and equal(host_call(solver, c), host)


@pytest.mark.parametrize("name", list(SEEDED))
def test_the_kernels_are_the_yardstick_on_the_seeded_cases(solver, seeded_ref, name):
    c, want = SEEDED[name], seeded_ref[name]
    got = device_call(solver, c)
    assert R.same(got, want), differing(got, want)           # rows, info and field the rule does not write: the prefill
    host = host_call(solver, c)
    assert equal(host, got), differing(host, got)
    assert equal(device_call(solver, c), got) and equal(host_call(solver, c), host)    # and twice


# ---- independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [MC.seeded_name(*MC.SHAPES[1]), MC.seeded_name(*MC.SHAPES[2])])
def test_a_permuted_a_one_robot_and_an_every_other_robot_batch_give_each_robot_the_same_rows(solver, seeded_ref, name):
    c, full = SEEDED[name], seeded_ref[name]
    B = len(c["pose"])
    perm = np.random.default_rng(5).permutation(B)
    repaired = int(np.flatnonzero(full["status"] == R.REPAIRED)[0])
    for rows in (perm, slice(repaired, repaired + 1), slice(3, 4), slice(0, B, 2), slice(1, B, 2)):
        part = host_call(solver, c, rows=rows)
        assert all(part[k].tobytes() == full[k][rows].tobytes() for k in OUTPUTS), rows
    dev = device_call(solver, rows_of(c, perm))
    assert all(dev[k].tobytes() == full[k][perm].tobytes() for k in OUTPUTS)


# ---- optional arrays, alignment -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [MC.seeded_name(*MC.SHAPES[0]), MC.seeded_name(*MC.SHAPES[2])])
def test_info_field_and_plan_start_as_null(solver, seeded_ref, name):
    c, full = SEEDED[name], seeded_ref[name]
    for without in (("info",), ("field",), ("info", "field")):
        got = device_call(solver, c, without=without)
        assert all(got[k] is None for k in without) and equal(got, full, [k for k in OUTPUTS if k not in without]), without
        host = host_call(solver, c, without=without)
        assert all(host[k] is None for k in without) and equal(host, got), without
    unstarted = dict(c, plan_start=None)                       # NULL plan_start: 0 for every robot
    want = reference(unstarted)
    assert (want["info"][:, 0] != full["info"][:, 0]).any()
    got = device_call(solver, c, without=("plan_start",))
    assert R.same(got, want), differing(got, want)
    assert equal(host_call(solver, c, without=("plan_start",)), got)


@pytest.mark.parametrize("name", [MC.seeded_name(*MC.SHAPES[1]), MC.seeded_name(*MC.SHAPES[3])])
def test_rows_at_8_byte_but_not_16_byte_addresses(solver, seeded_ref, name):
    got = device_call(solver, SEEDED[name], skew=True)
    assert R.same(got, seeded_ref[name]), differing(got, seeded_ref[name])


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_every_buffer_alone_and_an_empty_batch_succeeds(solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError
    c = HAND["wall"]
    B, L, S = 1, c["plan"].shape[1], 2 * c["R"] + 1
    costmap, origin, pose = np.ascontiguousarray(c["costmap"]), np.ascontiguousarray(c["origin"]), np.ascontiguousarray(c["pose"])
    ARGS = ("plan", "plan_len", "workspace", "status", "info", "field")
    fresh = lambda: {"plan": c["plan"].copy(), "plan_len": c["plan_len"].copy(), "workspace": np.full((B, L, 2), 777.0), "status": np.full(B, -7, np.int32),
                     "info": np.full((B, 4), -7, np.int32), "field": np.full((B, S, S), 7, np.uint32)}
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(change=None, outs=None, args=None):
        """One host-pointer call after `change(ri)`; outs: replacements of the arrays (None: NULL); returns (code or None, the
        arrays, the arrays before)."""
        ri = repair_in(c, B, 0)
        ri.costmap, ri.costmap_origin, ri.robot_pose = costmap.ctypes.data, origin.ctypes.data, pose.ctypes.data
        out = fresh()
        if outs:
            out.update(outs)
        if change:
            change(ri)
        before = {k: None if v is None else v.copy() for k, v in out.items()}
        try:
            solver._call("smpc_repair_plan_batch", *(args if args is not None else (ri,)), *(ptr(out[k]) for k in ARGS))
            code = None
        except SmpcError as e:
            code = int(str(e).split("(")[1].split(")")[0])
        return code, out, before

    def accepted():
        ok, out, _ = call()
        assert ok is None and out["status"].tolist() == [R.REPAIRED] and out["info"].tolist() == [[0, 3, 4, 6]] and out["plan_len"].tolist() == [13]
        assert (out["workspace"] == 777.0).all()                         # a host-pointer call brings its own
        MC.check_want(c, out)
        assert solver.last_kernel_ms() > 0.0

    accepted()
    INVALID, UNSUPPORTED = -1, -2                                    # SMPC_ERR_INVALID_ARG, SMPC_ERR_UNSUPPORTED of include/smpc.h

    def field(**kw):
        def change(ri):
            for k, v in kw.items():
                if k in ("neutral_cost", "cost_weight"):
                    setattr(ri.cost, k, v)
                else:
                    setattr(ri, k, v)
        return change

    nan, inf = float("nan"), float("inf")
    refusals = [
        (field(costmap=None), INVALID), (field(costmap_origin=None), INVALID), (field(robot_pose=None), INVALID), (field(B=-1), INVALID),
        (field(L=1), INVALID), (field(L=0), INVALID), (field(size_x=0), INVALID), (field(size_y=0), INVALID), (field(size_x=-3), INVALID),
        (field(radius=0), INVALID), (field(radius=-1), INVALID), (field(stride=0), INVALID), (field(stride=-2), INVALID),
        (field(resolution=0.0), INVALID), (field(resolution=-0.05), INVALID), (field(resolution=nan), INVALID), (field(resolution=inf), INVALID),
        (field(clearance_d2=-0.1), INVALID), (field(clearance_d2=nan), INVALID), (field(clearance_d2=inf), INVALID),
        (field(neutral_cost=0), INVALID), (field(cost_weight=-1), INVALID), (field(neutral_cost=50, cost_weight=257), INVALID),
        (field(radius=64), UNSUPPORTED), (field(radius=63, neutral_cost=50, cost_weight=150), UNSUPPORTED),
    ]
    for i, (change, want) in enumerate(refusals):
        code, out, before = call(change)
        assert code == want, (i, code, want)
        assert all(out[k].tobytes() == before[k].tobytes() for k in ARGS), i
    for outs in ({"plan": None}, {"plan_len": None}, {"workspace": None}, {"status": None}):    # NULL required arrays, a NULL input struct
        code, out, before = call(outs=outs)
        assert code == INVALID and all(out[k] is None or out[k].tobytes() == before[k].tobytes() for k in ARGS), outs
    assert call(args=(None,))[0] == INVALID
    code, out, before = call(field(B=0))                                # an empty batch succeeds, launches nothing and writes nothing
    assert code is None and all(out[k].tobytes() == before[k].tobytes() for k in ARGS)
    assert call(field(B=0, robot_pose=None))[0] == INVALID              # ... but is checked like any other
    # the largest region under the heaviest costs that fit (its field rows are 127 x 127)
    code, out, _ = call(field(radius=63, neutral_cost=50, cost_weight=148), outs={"field": np.full((B, 127, 127), 7, np.uint32)})
    assert code is None and out["status"].tolist() == [R.REPAIRED] and out["info"].tolist() == [[0, 3, 4, 6]]
    accepted()                                                          # the accepted call after them
