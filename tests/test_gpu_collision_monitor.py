"""smpc_collision_monitor_batch on the GPU against tests/collision_monitor_ref.py: cmd_out, action, zone_points and ratio bit
for bit given the device's own heading_cs and step_cs, those held against numpy's by the bound tests/test_math.py holds
sincos_tab to: the hand-made and seeded cases of tests/collision_monitor_cases.py (n_beams 1 / 63 / 64 / 65 / 360 / 512 / 513 /
4096, Z 1 / 8, a circle, a 3-gon and a 16-gon, M 0 / 1 / 12 / 32, min_points 1 / 4 / more than n_beams); host against device
pointers, two runs, a permuted and a shorter batch, every optional output as NULL, every refusal with sentinel-filled
buffers, B == 0, and the call fed from smpc_sensed_costmap_batch's own beam_kind / beam_cell."""
import ctypes as C

import numpy as np
import pytest

import collision_monitor_cases as MC
import collision_monitor_ref as R
import sensed_costmap_cases
from nav2_social_mpc_controller_amd import _abi_collision_monitor as MA
from nav2_social_mpc_controller_amd.params import OptimizerParams

pytestmark = pytest.mark.gpu

HAND = MC.hand_cases()
SEEDED = MC.seeded_cases()
OUTPUTS = ("cmd_out", "action", "zone_points", "ratio", "heading_cs", "step_cs")


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


def monitor_in(p, B, n_beams, on_device):
    """The yardstick's scalars and zones as the call's struct (no array pointers yet)."""
    zones = (MA.SmpcMonitorZone * len(p["zones"]))()
    for zc, z in zip(zones, p["zones"]):
        zc.shape, zc.action, zc.n_vertices, zc.min_points = z["shape"], z["action"], z["n"], z["min_points"]
        zc.radius, zc.slowdown_ratio, zc.linear_limit, zc.angular_limit = (float(z[k]) for k in ("radius", "slowdown_ratio", "linear_limit", "angular_limit"))
        for i, (vx, vy) in enumerate(z["vertices"]):
            zc.vertices[i][0], zc.vertices[i][1] = float(vx), float(vy)
    mi = MA.SmpcCollisionMonitorIn(B=B, n_beams=n_beams, Z=len(zones), M=p["M"], on_device=on_device, sim_dt=float(p["sim_dt"]),
                                   resolution=float(p["res"]))
    mi.world_origin[0], mi.world_origin[1] = float(p["origin"][0]), float(p["origin"][1])
    mi._zones = zones
    mi.zones = C.addressof(zones)
    return mi


def host_call(solver, c, rows=None, **with_flags):
    rows = slice(None) if rows is None else rows
    kind = c["kind"][rows]
    return solver.collision_monitor(monitor_in(c["p"], kind.shape[0], kind.shape[1], 0), c["pose"][rows], c["cmd"][rows], kind, c["cell"][rows], **with_flags)


def device_call(solver, c, without=()):
    """The call on device pointers; the outputs named in `without` are passed as NULL (and come back None)."""
    import torch
    from nav2_social_mpc_controller_amd.solver import point
    dev = "cuda:0"
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).copy()).to(dev)
    B, n = c["kind"].shape
    Z = len(c["p"]["zones"])
    t = {"robot_pose": up(c["pose"], np.float64), "cmd": up(c["cmd"], np.float64), "beam_kind": up(c["kind"], np.uint8),
         "beam_cell": up(c["cell"], np.int32)}                                  # alive until the call has run
    mi = point(monitor_in(c["p"], B, n, 1), t)
    out = {"cmd_out": torch.full((B, 2), float("nan"), dtype=torch.float64, device=dev), "action": torch.full((B, 4), -1, dtype=torch.int32, device=dev),
           "zone_points": torch.full((B, Z), -1, dtype=torch.int32, device=dev), "ratio": torch.full((B,), float("nan"), dtype=torch.float64, device=dev),
           "heading_cs": torch.full((B, 2), float("nan"), dtype=torch.float64, device=dev),
           "step_cs": torch.full((B, 2), float("nan"), dtype=torch.float64, device=dev)}
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    solver.collision_monitor_device(mi, *(0 if k in without else out[k].data_ptr() for k in OUTPUTS))
    torch.cuda.synchronize()
    solver.set_stream(0)
    del t
    return {k: None if k in without else v.cpu().numpy() for k, v in out.items()}


def equal(a, b, keys=OUTPUTS):
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and a[k].tobytes() == b[k].tobytes()) for k in keys)


def held_to_the_yardstick(c, got):
    p, M = c["p"], c["p"]["M"]
    want = R.run(p, c["pose"], c["cmd"], c["kind"], c["cell"], got["heading_cs"], got["step_cs"])
    assert R.same(got, want), [k for k in ("cmd_out", "action", "zone_points", "ratio") if got[k].tobytes() != want[k].tobytes()]
    assert R.angles_close(got["heading_cs"], got["step_cs"], c["pose"], c["cmd"], p["sim_dt"], M)
    fin = want["finite"]
    assert np.isfinite(got["heading_cs"][fin]).all() and np.isnan(got["heading_cs"][~fin]).all()          # rows of bad inputs: not written
    assert np.isnan(got["step_cs"][~fin]).all() and (np.isfinite(got["step_cs"][fin]).all() if M > 0 else np.isnan(got["step_cs"]).all())
    return want


# ---- against the yardstick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND) + sorted(SEEDED))
def test_the_kernel_is_the_yardstick_given_its_own_cosines_and_sines(solver, name):
    c = HAND[name] if name in HAND else SEEDED[name]
    got = device_call(solver, c)
    held_to_the_yardstick(c, got)
    if name in HAND:
        MC.check_want(c, got)
    # from host pointers, and twice each
    host = host_call(solver, c)
    assert equal(host, got), [k for k in OUTPUTS if host[k].tobytes() != got[k].tobytes()]
    assert equal(device_call(solver, c), got) and equal(host_call(solver, c), host)


def test_the_seeded_cases_cover_the_shapes_the_kernel_branches_on():
    beams = {c["kind"].shape[1] for c in SEEDED.values()}
    assert beams >= {1, 63, 64, 65, 360, 513, 4096} and max(c["kind"].shape[0] for c in SEEDED.values()) <= 64
    assert {len(c["p"]["zones"]) for c in SEEDED.values()} == {1, 8} and {c["p"]["M"] for c in SEEDED.values()} == {0, 1, 12, 32}
    assert {z["n"] for c in SEEDED.values() for z in c["p"]["zones"]} >= {0, 3, 16}
    mins = {(z["min_points"] > c["kind"].shape[1], z["min_points"]) for c in SEEDED.values() for z in c["p"]["zones"]}
    assert {m for _, m in mins} >= {1, 4} and any(over for over, _ in mins)


# ---- independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [MC.MAIN, "B8_n513_Z8_M12"])
def test_a_permuted_and_a_shorter_batch_give_each_robot_the_same_rows(solver, name):
    c = SEEDED[name]
    B = len(c["pose"])
    full = host_call(solver, c)
    perm = np.random.default_rng(5).permutation(B)
    shuffled = host_call(solver, c, rows=perm)
    assert all(shuffled[k].tobytes() == full[k][perm].tobytes() for k in OUTPUTS)
    for rows in (slice(0, 1), slice(3, B - 2), slice(B - 5, B)):
        part = host_call(solver, c, rows=rows)
        assert all(part[k].tobytes() == full[k][rows].tobytes() for k in OUTPUTS), rows
    dev = device_call(solver, dict(c, pose=c["pose"][perm], cmd=c["cmd"][perm], kind=c["kind"][perm], cell=c["cell"][perm]))
    assert equal(dev, shuffled)


# ---- optional outputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [MC.MAIN, "B4_n4096_Z8_M32"])
def test_each_optional_output_as_null_leaves_the_others_unchanged(solver, name):
    c = SEEDED[name]
    full = device_call(solver, c)
    host = host_call(solver, c)
    for k in ("zone_points", "ratio", "heading_cs", "step_cs"):
        got = device_call(solver, c, without=(k,))
        assert got[k] is None and equal(got, full, [o for o in OUTPUTS if o != k]), k
        flag = {"zone_points": "with_zone_points", "ratio": "with_ratio", "heading_cs": "with_heading", "step_cs": "with_step"}[k]
        got = host_call(solver, c, **{flag: False})
        assert got[k] is None and equal(got, host, [o for o in OUTPUTS if o != k]), k
    none = device_call(solver, c, without=("zone_points", "ratio", "heading_cs", "step_cs"))
    assert equal(none, full, ["cmd_out", "action"])


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_every_buffer_alone_and_an_empty_batch_succeeds(solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError
    c = HAND["least_ratio_decides"]
    B, n = c["kind"].shape
    Z = len(c["p"]["zones"])
    pose, cmd = np.ascontiguousarray(c["pose"]), np.ascontiguousarray(c["cmd"])
    kind, cell = np.ascontiguousarray(c["kind"]), np.ascontiguousarray(c["cell"])
    fresh = lambda: {"cmd_out": np.full((B, 2), 777.0), "action": np.full((B, 4), -7, np.int32), "zone_points": np.full((B, Z), -7, np.int32),
                     "ratio": np.full(B, 777.0), "heading_cs": np.full((B, 2), 777.0), "step_cs": np.full((B, 2), 777.0)}
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(change=None, outs=None, args=None):
        """One host-pointer call after `change(mi)`; outs: the output arrays (None: NULL); returns (code or None, the arrays)."""
        mi = monitor_in(c["p"], B, n, 0)
        mi.robot_pose, mi.cmd, mi.beam_kind, mi.beam_cell = pose.ctypes.data, cmd.ctypes.data, kind.ctypes.data, cell.ctypes.data
        out = fresh()
        if outs:
            out.update(outs)
        if change:
            change(mi)
        before = {k: None if v is None else v.copy() for k, v in out.items()}
        try:
            solver._call("smpc_collision_monitor_batch", *(args if args is not None else (mi,)), *(ptr(out[k]) for k in OUTPUTS))
            code = None
        except SmpcError as e:
            code = int(str(e).split("(")[1].split(")")[0])
        return code, out, before

    ok, out, _ = call()
    assert ok is None and out["action"][0, 1] == 0 and (out["cmd_out"] != 777.0).all()
    kms = solver.last_kernel_ms()
    assert kms > 0.0
    INVALID, UNSUPPORTED = -1, -2                                    # SMPC_ERR_INVALID_ARG, SMPC_ERR_UNSUPPORTED of include/smpc.h

    def zone(i, **kw):
        def change(mi):
            for k, v in kw.items():
                if k == "vertex":
                    mi._zones[i].vertices[v[0]][v[1]] = v[2]
                else:
                    setattr(mi._zones[i], k, v)
        return change

    def field(**kw):
        def change(mi):
            for k, v in kw.items():
                setattr(mi, k, v)
        return change

    def polygon(mi):
        z = mi._zones[0]
        z.shape, z.n_vertices = 1, 3
        for i, (x, y) in enumerate([(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]):
            z.vertices[i][0], z.vertices[i][1] = x, y

    def then(*changes):
        def change(mi):
            for f in changes:
                f(mi)
        return change

    nan, inf = float("nan"), float("inf")
    refusals = [
        (field(zones=None), INVALID), (field(robot_pose=None), INVALID), (field(cmd=None), INVALID), (field(beam_kind=None), INVALID),
        (field(beam_cell=None), INVALID), (field(B=-1), INVALID), (field(Z=0), INVALID), (field(Z=-3), INVALID), (field(n_beams=0), INVALID),
        (field(M=-1), INVALID), (field(M=0), INVALID),                                          # zone 2 is an APPROACH zone
        (field(resolution=0.0), INVALID), (field(resolution=-0.05), INVALID), (field(resolution=nan), INVALID), (field(resolution=inf), INVALID),
        (field(sim_dt=0.0), INVALID), (field(sim_dt=-0.1), INVALID), (field(sim_dt=nan), INVALID), (field(sim_dt=inf), INVALID),
        (zone(0, shape=2), INVALID), (zone(0, shape=-1), INVALID), (zone(1, action=4), INVALID), (zone(1, action=-1), INVALID),
        (then(polygon, zone(0, n_vertices=2)), INVALID), (then(polygon, zone(0, n_vertices=17)), INVALID),
        (then(polygon, zone(0, vertex=(1, 0, nan))), INVALID), (then(polygon, zone(0, vertex=(2, 1, inf))), INVALID),
        (zone(2, min_points=0), INVALID), (zone(0, radius=-0.1), INVALID), (zone(0, radius=nan), INVALID), (zone(0, radius=inf), INVALID),
        (zone(1, linear_limit=-0.1), INVALID), (zone(1, angular_limit=-1.0), INVALID), (zone(1, linear_limit=nan), INVALID),
        (zone(0, slowdown_ratio=1.5), INVALID), (zone(0, slowdown_ratio=-0.1), INVALID), (zone(0, slowdown_ratio=nan), INVALID),
        (field(Z=9), UNSUPPORTED), (field(M=33), UNSUPPORTED), (field(n_beams=4097), UNSUPPORTED),
    ]
    for i, (change, want) in enumerate(refusals):
        code, out, before = call(change)
        assert code == want, (i, code, want)
        assert all(out[k].tobytes() == before[k].tobytes() for k in OUTPUTS), i
    assert call(polygon)[0] is None                                                                # the polygon itself is fine
    # NULL required outputs, cmd_out == cmd, a NULL input struct
    for outs in ({"cmd_out": None}, {"action": None}, {"cmd_out": cmd}):
        code, out, before = call(outs=outs)
        assert code == INVALID and all(out[k] is None or out[k].tobytes() == before[k].tobytes() for k in OUTPUTS), outs
    assert call(args=(None,))[0] == INVALID and cmd.tobytes() == np.ascontiguousarray(c["cmd"]).tobytes()
    # an empty batch succeeds, launches nothing and writes nothing
    code, out, before = call(field(B=0))
    assert code is None and all(out[k].tobytes() == before[k].tobytes() for k in OUTPUTS)
    code, out, before = call(field(B=0, robot_pose=None))                                          # ... but is checked like any other
    assert code == INVALID


# ---- fed from the real scan ------------------------------------------------------------------------------------------------------
def test_the_monitor_judges_the_beams_the_scan_itself_wrote(solver):
    kw = sensed_costmap_cases.random_case(world_size=(96, 80), B=16, Np=3, size=(24, 20), n_beams=72, reach=14, r=3, seed=3, discs=10)
    _, kind, cell = solver.sensed_costmap(kw["world"], kw["origin"], kw["res"], kw["robot_pose"], kw["people"], kw["count"], kw["cell"], kw["size_x"],
                                          kw["size_y"], kw["beam_cells"], kw["agent_d2"], kw["table"], kw["base"], kw["outside_cost"], kw["min_cost"],
                                          kw["unknown"])
    assert kind.shape == (16, 72) and set(np.unique(kind)) >= {0, 1, 2} and (np.abs(cell) <= 14).all()
    g = np.random.default_rng(3)
    pose = kw["robot_pose"].copy()
    pose[:, 2] = g.uniform(-np.pi, np.pi, 16)
    cmd = np.stack([g.uniform(0.2, 0.8, 16), g.uniform(-1.0, 1.0, 16)], axis=1)
    zones = [R.circle(R.STOP, 0.2, 2), R.polygon(R.SLOWDOWN, [(-0.2, -0.3), (0.7, -0.3), (0.7, 0.3), (-0.2, 0.3)], 3, slowdown_ratio=0.5),
             R.polygon(R.APPROACH, MC.regular(8, 0.26, np.pi / 8), 2)]
    c = dict(p=R.params(zones, M=12, sim_dt=0.1, res=kw["res"], origin=tuple(kw["origin"])), pose=pose, cmd=cmd, kind=kind, cell=cell)
    got = device_call(solver, c)
    want = held_to_the_yardstick(c, got)
    assert (want["action"][:, 3] > 0).sum() >= 12 and len(set(want["action"][:, 1])) >= 3, want["action"]     # the scan's hits decide in several ways
