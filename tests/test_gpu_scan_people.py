"""smpc_scan_people_batch on the GPU against tests/scan_people_ref.py, all four outputs bit for bit: the hand-made and seeded
cases of tests/scan_people_cases.py (n_beams 1 / 2 / 63 / 64 / 65 / 130 / 360 / 4096, Nd 1 .. 64) on device pointers over NaN
and sentinel prefill, from host pointers, and twice; a permuted, a one-robot and an every-other-robot batch; det_segment and
seg_stats as NULL; beam_cell and detections at 8-byte but not 16-byte offsets; the call fed from smpc_sensed_costmap_batch's own
beam_kind / beam_cell; every refusal with sentinel-filled buffers, B == 0 and the accepted call after them."""
import numpy as np
import pytest

import scan_people_cases as MC
import scan_people_ref as R
import sensed_costmap_cases
from nav2_social_mpc_controller_amd import _abi_scan_people as MA
from nav2_social_mpc_controller_amd.params import OptimizerParams

pytestmark = pytest.mark.gpu

HAND = MC.hand_cases()
SEEDED = MC.seeded_cases()
OUTPUTS = ("detections", "det_count", "det_segment", "seg_stats")


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def seeded_ref():
    return {name: R.run(c["p"], c["Nd"], c["pose"], c["kind"], c["cell"]) for name, c in SEEDED.items()}


def scan_in(p, B, n_beams, Nd, on_device):
    """The yardstick's scalars as the call's struct (no array pointers yet)."""
    si = MA.SmpcScanPeopleIn(B=B, n_beams=n_beams, Nd=Nd, on_device=on_device, subtract_map=p["subtract_map"], min_points=p["min_points"],
                             link_d2=p["link_d2"], width_d2_min=p["width_d2_min"], width_d2_max=p["width_d2_max"], range_d2=p["range_d2"],
                             resolution=float(p["res"]), body_offset=float(p["body_offset"]))
    si.world_origin[0], si.world_origin[1] = float(p["origin"][0]), float(p["origin"][1])
    return si


def host_call(solver, c, rows=None, **kw):
    rows = slice(None) if rows is None else rows
    kind = c["kind"][rows]
    got = solver.scan_people(scan_in(c["p"], kind.shape[0], kind.shape[1], c["Nd"], 0), c["pose"][rows], kind, c["cell"][rows], **kw)
    return dict(zip(OUTPUTS, got))


def device_call(solver, c, without=(), skew=False):
    """The call on device pointers over NaN / -99 / -1 prefill; the outputs named in `without` are passed as NULL (and come back
    None). skew: beam_cell and detections start 8 bytes into their allocations, so at 8-byte but not 16-byte addresses."""
    import torch
    from nav2_social_mpc_controller_amd.solver import point
    dev = "cuda:0"
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).copy()).to(dev)
    B, n = c["kind"].shape
    Nd = c["Nd"]
    pad = 2 if skew else 0
    cells = torch.zeros(pad + B * n * 2, dtype=torch.int32, device=dev)
    cells[pad:] = up(c["cell"], np.int32).reshape(-1)
    det = torch.full((pad // 2 + B * Nd * 5,), float("nan"), dtype=torch.float64, device=dev)
    t = {"robot_pose": up(c["pose"], np.float64), "beam_kind": up(c["kind"], np.uint8), "beam_cell": cells[pad:]}   # alive until the call has run
    if skew:
        assert t["beam_cell"].data_ptr() % 16 == 8 and det[1:].data_ptr() % 16 == 8
    si = point(scan_in(c["p"], B, n, Nd, 1), t)
    out = {"detections": det[pad // 2:], "det_count": torch.full((B,), -1, dtype=torch.int32, device=dev),
           "det_segment": torch.full((B, Nd, 4), -99, dtype=torch.int32, device=dev), "seg_stats": torch.full((B, 4), -1, dtype=torch.int32, device=dev)}
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    solver.scan_people_device(si, *(0 if k in without else out[k].data_ptr() for k in OUTPUTS))
    torch.cuda.synchronize()
    solver.set_stream(0)
    del t
    got = {k: None if k in without else v.cpu().numpy() for k, v in out.items()}
    got["detections"] = got["detections"].reshape(B, Nd, 5)
    assert pad == 0 or np.isnan(det[0].item())
    return got


def equal(a, b, keys=OUTPUTS):
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and a[k].tobytes() == b[k].tobytes()) for k in keys)


def differing(got, want):
    """What a failing comparison prints: per output the robots whose rows differ, and the first such robot's rows."""
    out = []
    for k in OUTPUTS:
        if got[k] is not None and got[k].tobytes() != want[k].tobytes():
            bad = [b for b in range(len(want[k])) if got[k][b].tobytes() != want[k][b].tobytes()]
            out.append((k, bad[:8], got[k][bad[0]].tolist(), want[k][bad[0]].tolist()))
    return out


# ---- against the yardstick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_the_kernel_is_the_yardstick_on_the_hand_made_cases(solver, name):
    c = HAND[name]
    got = device_call(solver, c)
    want = R.run(c["p"], c["Nd"], c["pose"], c["kind"], c["cell"])
    assert R.same(got, want), differing(got, want)
    MC.check_want(c, got)
    host = host_call(solver, c)
    assert equal(host, got), differing(host, got)
    assert equal(device_call(solver, c), got) and equal(host_call(solver, c), host)


@pytest.mark.parametrize("name", list(SEEDED))
def test_the_kernel_is_the_yardstick_on_the_seeded_cases(solver, seeded_ref, name):
    c, want = SEEDED[name], seeded_ref[name]
    got = device_call(solver, c)
    assert R.same(got, want), differing(got, want)                      # rows beyond det_count: the NaN and -99 prefill
    host = host_call(solver, c)
    assert equal(host, got), differing(host, got)
    assert equal(device_call(solver, c), got) and equal(host_call(solver, c), host)    # and twice
    fill = dict(detections=np.full((len(c["pose"]), c["Nd"], 5), 7.5), det_segment=np.full((len(c["pose"]), c["Nd"], 4), 1234, np.int32))
    assert R.same(host_call(solver, c, **fill), R.run(c["p"], c["Nd"], c["pose"], c["kind"], c["cell"], **fill))


# ---- independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [MC.seeded_name(67, 65, 8), MC.seeded_name(33, 360, 16)])
def test_a_permuted_a_one_robot_and_an_every_other_robot_batch_give_each_robot_the_same_rows(solver, seeded_ref, name):
    c, full = SEEDED[name], seeded_ref[name]
    B = len(c["pose"])
    perm = np.random.default_rng(5).permutation(B)
    for rows in (perm, slice(1, 2), slice(3, 4), slice(0, B, 2), slice(1, B, 2)):
        part = host_call(solver, c, rows=rows)
        assert all(part[k].tobytes() == full[k][rows].tobytes() for k in OUTPUTS), rows
    dev = device_call(solver, dict(c, pose=c["pose"][perm], kind=c["kind"][perm], cell=c["cell"][perm]))
    assert all(dev[k].tobytes() == full[k][perm].tobytes() for k in OUTPUTS)


# ---- optional outputs, alignment -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [MC.seeded_name(33, 360, 16), MC.seeded_name(5, 4096, 64), MC.seeded_name(9, 130, 1)])
def test_each_optional_output_as_null_leaves_the_others_unchanged(solver, seeded_ref, name):
    c, full = SEEDED[name], seeded_ref[name]
    for without in (("det_segment",), ("seg_stats",), ("det_segment", "seg_stats")):     # without seg_stats the walk may end early
        got = device_call(solver, c, without=without)
        assert all(got[k] is None for k in without) and R.same(got, full), (without, differing(got, full))
    host = host_call(solver, c, with_segment=False, with_stats=False)
    assert host["det_segment"] is None and host["seg_stats"] is None and R.same(host, full)
    assert R.same(host_call(solver, c, with_stats=False), full) and R.same(host_call(solver, c, with_segment=False), full)


@pytest.mark.parametrize("name", [MC.seeded_name(67, 63, 4), MC.seeded_name(33, 360, 16)])
def test_arrays_at_8_byte_but_not_16_byte_addresses(solver, seeded_ref, name):
    got = device_call(solver, SEEDED[name], skew=True)
    assert R.same(got, seeded_ref[name]), differing(got, seeded_ref[name])


# ---- fed from the real scan ------------------------------------------------------------------------------------------------------
def test_the_call_clusters_the_beams_the_scan_itself_wrote(solver):
    kw = sensed_costmap_cases.random_case(world_size=(96, 96), B=24, Np=3, size=(40, 40), n_beams=360, reach=30, r=3, seed=11, discs=8, agent_d2=16)
    _, kind, cell = solver.sensed_costmap(kw["world"], kw["origin"], kw["res"], kw["robot_pose"], kw["people"], kw["count"], kw["cell"], kw["size_x"],
                                          kw["size_y"], kw["beam_cells"], kw["agent_d2"], kw["table"], kw["base"], kw["outside_cost"], kw["min_cost"],
                                          kw["unknown"])
    assert kind.shape == (24, 360) and set(np.unique(kind)) >= {0, 1, 2}
    for subtract in (1, 0):
        p = R.params(link_d2=9, min_points=3, width_d2_min=4, width_d2_max=144, range_d2=900, subtract_map=subtract, body_offset=0.2, res=kw["res"],
                     origin=tuple(kw["origin"]))
        c = dict(p=p, Nd=16, pose=kw["robot_pose"], kind=kind, cell=cell)
        got, want = device_call(solver, c), R.run(p, 16, kw["robot_pose"], kind, cell)
        assert R.same(got, want), differing(got, want)
        assert want["seg_stats"][:, 3].sum() >= 8 and (want["seg_stats"][:, 1] > 0).any(), want["seg_stats"]   # people are found, slivers are not


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_every_buffer_alone_and_an_empty_batch_succeeds(solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError
    c = HAND["one_arc"]
    B, n = c["kind"].shape
    Nd = c["Nd"]
    pose, kind, cell = np.ascontiguousarray(c["pose"]), np.ascontiguousarray(c["kind"]), np.ascontiguousarray(c["cell"])
    fresh = lambda: {"detections": np.full((B, Nd, 5), 777.0), "det_count": np.full(B, -7, np.int32), "det_segment": np.full((B, Nd, 4), -7, np.int32),
                     "seg_stats": np.full((B, 4), -7, np.int32)}
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(change=None, outs=None, args=None):
        """One host-pointer call after `change(si)`; outs: the output arrays (None: NULL); returns (code or None, the arrays)."""
        si = scan_in(c["p"], B, n, Nd, 0)
        si.robot_pose, si.beam_kind, si.beam_cell = pose.ctypes.data, kind.ctypes.data, cell.ctypes.data
        out = fresh()
        if outs:
            out.update(outs)
        if change:
            change(si)
        before = {k: None if v is None else v.copy() for k, v in out.items()}
        try:
            solver._call("smpc_scan_people_batch", *(args if args is not None else (si,)), *(ptr(out[k]) for k in OUTPUTS))
            code = None
        except SmpcError as e:
            code = int(str(e).split("(")[1].split(")")[0])
        return code, out, before

    def accepted():
        ok, out, _ = call()
        assert ok is None and out["det_count"].tolist() == [1] and out["det_segment"][0, 0].tolist() == [3, 3, 24, 3]
        assert out["seg_stats"].tolist() == [[1, 0, 0, 1]] and (out["detections"][0, 1:] == 777.0).all() and (out["det_segment"][0, 1:] == -7).all()
        assert solver.last_kernel_ms() > 0.0

    accepted()
    INVALID, UNSUPPORTED = -1, -2                                    # SMPC_ERR_INVALID_ARG, SMPC_ERR_UNSUPPORTED of include/smpc.h

    def field(**kw):
        def change(si):
            for k, v in kw.items():
                if k == "origin":
                    si.world_origin[v[0]] = v[1]
                else:
                    setattr(si, k, v)
        return change

    nan, inf = float("nan"), float("inf")
    refusals = [
        (field(robot_pose=None), INVALID), (field(beam_kind=None), INVALID), (field(beam_cell=None), INVALID), (field(B=-1), INVALID),
        (field(n_beams=0), INVALID), (field(n_beams=-5), INVALID), (field(Nd=0), INVALID), (field(Nd=-1), INVALID), (field(min_points=0), INVALID),
        (field(min_points=-2), INVALID), (field(link_d2=-1), INVALID), (field(width_d2_min=-1), INVALID), (field(width_d2_max=-1), INVALID),
        (field(range_d2=-1), INVALID), (field(width_d2_min=5, width_d2_max=4), INVALID), (field(subtract_map=2), INVALID),
        (field(subtract_map=-1), INVALID), (field(resolution=0.0), INVALID), (field(resolution=-0.05), INVALID), (field(resolution=nan), INVALID),
        (field(resolution=inf), INVALID), (field(origin=(0, nan)), INVALID), (field(origin=(1, inf)), INVALID), (field(origin=(1, -inf)), INVALID),
        (field(body_offset=-0.1), INVALID), (field(body_offset=nan), INVALID), (field(body_offset=inf), INVALID),
        (field(n_beams=4097), UNSUPPORTED), (field(Nd=65), UNSUPPORTED),
    ]
    for i, (change, want) in enumerate(refusals):
        code, out, before = call(change)
        assert code == want, (i, code, want)
        assert all(out[k].tobytes() == before[k].tobytes() for k in OUTPUTS), i
    for outs in ({"detections": None}, {"det_count": None}):          # NULL required outputs, a NULL input struct
        code, out, before = call(outs=outs)
        assert code == INVALID and all(out[k] is None or out[k].tobytes() == before[k].tobytes() for k in OUTPUTS), outs
    assert call(args=(None,))[0] == INVALID
    code, out, before = call(field(B=0))                                # an empty batch succeeds, launches nothing and writes nothing
    assert code is None and all(out[k].tobytes() == before[k].tobytes() for k in OUTPUTS)
    assert call(field(B=0, robot_pose=None))[0] == INVALID              # ... but is checked like any other
    accepted()                                                          # the accepted call after them
