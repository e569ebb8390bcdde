"""Host pointers against device pointers (`-m gpu`): every batch entry point with a device mode is called with the same
inputs through host arrays (staged by the library through its arena and pinned mirror) and through torch tensors on the
GPU, and every output, the arrays updated in place included, must come back byte for byte the same.

Each case runs on a fresh handle. Its first host-pointer call finds an empty arena, so every array takes the overflow
hipMalloc and its own copy; the second finds the arena grown and gathers what fits into the 8 MiB mirror. The device
calls run twice, into outputs filled with two different bytes: what a kernel leaves unwritten keeps the fill, differs
between the two, and is left out of the comparison (the host call hands back whatever its staging memory held there)."""
import ctypes as C

import numpy as np
import pytest

from nav2_social_mpc_controller_amd import _abi
from nav2_social_mpc_controller_amd.params import OptimizerParams, TrajectorizerParams, scene_param_rows
from nav2_social_mpc_controller_amd.scenes import make_scenes

pytestmark = pytest.mark.gpu

README = OptimizerParams.readme()
DEV = "cuda:0"
FIELD = {f: i for i, f in enumerate(_abi.SCENE_PARAM_FIELDS)}


class Arrays:
    """The arrays of one call: host numpy copies (on_device 0) or torch tensors holding the same bytes (on_device 1)."""

    def __init__(self, on_device):
        self.on_device = int(on_device)
        self.arrays = {}

    def __call__(self, name, a):
        a = np.ascontiguousarray(a).copy()
        if self.on_device:
            import torch
            a = torch.from_numpy(a).to(DEV)
            self.arrays[name] = a
            return a.data_ptr()
        self.arrays[name] = a
        return a.ctypes.data

    def empty(self, name, shape, dtype, fill):
        return self(name, np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, fill, np.uint8).view(dtype).reshape(shape))

    def result(self):
        import torch
        torch.cuda.synchronize()
        return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in self.arrays.items()}


def check(lib, rc, what):
    assert rc == 0, f"{what} failed ({rc}): {lib.smpc_last_error().decode()}"


def both_modes(call):
    """call(solver, arrays, fill) makes the call(s) of one case. Returns the device-pointer result."""
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(README)
    runs = {}
    for mode, fill in (("host overflow", 0x5A), ("host arena", 0x5A), ("device", 0x00), ("device refilled", 0xA5)):
        a = Arrays(mode.startswith("device"))
        call(s, a, fill)
        runs[mode] = a.result()
        assert s.last_kernel_ms() > 0, mode
    dev = runs["device"]
    for k, x in dev.items():
        x = x.reshape(-1).view(np.uint8)
        written = x == runs["device refilled"][k].reshape(-1).view(np.uint8)
        assert written.any(), k
        for mode in ("host overflow", "host arena"):
            assert np.array_equal(runs[mode][k].reshape(-1).view(np.uint8)[written], x[written]), (mode, k)
    s.close()
    return dev


# -- scenes: solve, eval, stage_people ---------------------------------------------------------------------------------
def scene_batch(a, sc):
    sb = _abi.SmpcSceneBatch()
    sb.B, sb.T, sb.N, sb.on_device, sb.dt = sc.B, sc.T, sc.N, a.on_device, sc.dt
    for k in ("pose0", "init_params", "path_pts", "goal_yaw", "people", "has_people", "costmap", "costmap_origin", "T_scene",
              "scene_params"):
        if getattr(sc, k) is not None:
            setattr(sb, k, a(k, getattr(sc, k)))
    sb.costmap_shared = 1 if sc.costmap_shared else 0
    sb.size_x, sb.size_y, sb.resolution = sc.size_x, sc.size_y, sc.resolution
    return sb


def stage(s, a, sb, fill):
    rec = a.empty("records", (sb.B, sb.N, sb.T, 4), np.float64, fill)
    aux = a.empty("aux", (sb.B, sb.T, 2), np.float64, fill)
    check(s.lib, s.lib.smpc_stage_people_batch(s._h, C.byref(sb), C.c_void_p(rec), C.c_void_p(aux)), "smpc_stage_people_batch")
    return rec, aux


def scenes(B=48, N=8, varied=False):
    sc = make_scenes(README, B, N, map_cells=80, seed=31, standing_fraction=0.25)
    if varied:  # horizons and weights of their own
        rng = np.random.default_rng(32)
        sc = sc.with_horizons(rng.integers(5, sc.T + 1, size=B))
        rows = scene_param_rows([README], np.zeros(B, np.int64))
        rows[1::2, FIELD["distance_w"]] *= 1.5
        rows[2::3, FIELD["v_max"]] = 0.4
        sc = sc.with_scene_params(rows)
    return sc


@pytest.mark.parametrize("variant", ["plain", "varied", "order", "staged"])
def test_solve(variant):
    sc = scenes(varied=variant == "varied")
    B, T = sc.B, sc.T
    P = README.dims(T, True)[3]
    order = np.random.default_rng(33).permutation(B).astype(np.int32)

    def call(s, a, fill):
        sb = scene_batch(a, sc)
        if variant == "order":
            sb.order = a("order", order)
        if variant == "staged":
            sb.people_records, sb.people_aux = stage(s, a, sb, fill)
        rb = _abi.SmpcResultBatch()
        for k, shape, dt in (("params", (B, P), np.float64), ("cmds", (B, T + 1, 2), np.float64), ("path", (B, T + 1, 3), np.float64),
                             ("status", B, np.int32), ("reason", B, np.int32), ("iterations", B, np.int32),
                             ("evaluations", B, np.int32), ("initial_cost", B, np.float64), ("final_cost", B, np.float64)):
            setattr(rb, k, a.empty(k, shape, dt, fill))
        check(s.lib, s.lib.smpc_solve_batch(s._h, C.byref(sb), C.byref(rb)), "smpc_solve_batch")

    got = both_modes(call)
    assert (got["status"] >= 0).all() and (got["iterations"] > 0).any()


@pytest.mark.parametrize("row_order", [0, 1])
def test_eval(row_order):
    sc = scenes(varied=row_order == 1)
    B = sc.B
    _, _, _, P, M, _ = README.dims(sc.T, True)
    x = sc.init_params + np.random.default_rng(34).normal(scale=0.05, size=sc.init_params.shape)

    def call(s, a, fill):
        sb = scene_batch(a, sc)
        eo = _abi.SmpcEvalOut()
        for k, shape in (("residuals", (B, M)), ("jacobian", (B, M, P)), ("cost", B), ("gradient", (B, P))):
            setattr(eo, k, a.empty(k, shape, np.float64, fill))
        eo.row_order = row_order
        check(s.lib, s.lib.smpc_eval_batch(s._h, C.byref(sb), C.c_void_p(a("x", x)), C.byref(eo)), "smpc_eval_batch")

    got = both_modes(call)
    assert np.isfinite(got["cost"]).all()


def test_stage_people():
    sc = scenes()
    got = both_modes(lambda s, a, fill: stage(s, a, scene_batch(a, sc), fill))
    assert np.abs(got["records"]).max() > 0


# -- the plugin's other stages -------------------------------------------------------------------------------------------
def arcs(rng, B, L):
    th = rng.uniform(-np.pi, np.pi, (B, 1)) + rng.uniform(-0.5, 0.5, (B, 1)) * 0.06 * np.arange(L)
    step = rng.uniform(0.04, 0.1, (B, 1))
    return rng.uniform(-5, 5, (B, 1, 2)) + np.cumsum(np.stack([step * np.cos(th), step * np.sin(th)], -1), axis=1)


def poses_near(rng, plan, plan_len):
    B = plan.shape[0]
    j = rng.integers(0, np.maximum(plan_len // 2, 1))
    return np.concatenate([plan[np.arange(B), j] + rng.uniform(-0.3, 0.3, (B, 2)), rng.uniform(-3, 3, (B, 1))], 1)


def test_project_people():
    rng = np.random.default_rng(40)
    B, N, T, g = 64, 5, 28, 120
    init = np.zeros((B, N, 6))
    r, phi = rng.uniform(0.8, 3.0, (B, N)), rng.uniform(-np.pi, np.pi, (B, N))
    init[:, :, 0], init[:, :, 1], init[:, :, 2] = r * np.cos(phi), r * np.sin(phi), rng.uniform(-np.pi, np.pi, (B, N))
    init[:, :, 4] = rng.uniform(0.0, 1.2, (B, N))
    init[::4, 3:, 3] = -1.0  # no such agent
    path = np.zeros((B, T + 1, 6))
    path[:, :, 0:2] = np.cumsum(rng.uniform(-0.03, 0.03, (B, T + 1, 2)), axis=1)
    path[:, :, 2] = rng.uniform(-np.pi, np.pi, (B, 1))
    path[:, :, 3] = 0.05 * np.arange(T + 1)
    path[:, :, 4] = 0.6
    idx = rng.integers(0, g * g, size=(1, g, g)).astype(np.uint32)

    def call(s, a, fill):
        pb = _abi.SmpcProjectionBatch()
        pb.B, pb.T, pb.N, pb.on_device, pb.max_time, pb.time_step = B, T, N, a.on_device, 1.5, 0.05
        pb.init_people, pb.robot_path = a("init_people", init), a("robot_path", path)
        pb.od_indexes, pb.od_shared, pb.od_width, pb.od_height, pb.od_resolution = a("od_indexes", idx), 1, g, g, 0.1
        pb.od_origin = a("od_origin", np.array([[-6.0, -6.0]]))
        out = a.empty("people_proj", (B, T + 1, 6, N), np.float64, fill)
        err = a.empty("error", B, np.int32, fill)
        check(s.lib, s.lib.smpc_project_people_batch(s._h, C.byref(pb), C.c_void_p(out), C.c_void_p(err)), "smpc_project_people_batch")

    both_modes(call)


@pytest.mark.parametrize("B,H,W", [(16, 61, 37), (64, 200, 200)])  # the second stages 23 MB: far beyond the mirror
def test_obstacle_distance(B, H, W):
    rng = np.random.default_rng(41)
    cm = np.where(rng.uniform(size=(B, H, W)) < 0.01, 254, rng.integers(0, 200, (B, H, W))).astype(np.uint8)
    cm[0] = 0  # no obstacle at all

    def call(s, a, fill):
        ob = s.obstacle_distance_c(B, W, H, False, 0.05, a.on_device)
        ob.costmap = a("costmap", cm)
        oo = _abi.SmpcObstacleDistanceOut()
        oo.indexes = a.empty("indexes", (B, H, W), np.uint32, fill)
        oo.distances = a.empty("distances", (B, H, W), np.float32, fill)
        oo.n_obstacles = a.empty("n_obstacles", B, np.int32, fill)
        check(s.lib, s.lib.smpc_obstacle_distance_batch(s._h, C.byref(ob), C.byref(oo)), "smpc_obstacle_distance_batch")

    got = both_modes(call)
    assert got["n_obstacles"][0] == 0 and (got["n_obstacles"][1:] > 0).all()


@pytest.mark.parametrize("fov", [False, True])
def test_people_to_status(fov):
    rng = np.random.default_rng(42)
    B, Np, N = 200, 10, 3
    pose = np.stack([rng.uniform(3, 7, B), rng.uniform(3, 7, B), rng.uniform(-np.pi, np.pi, B)], 1)
    people = rng.normal(size=(B, Np, 5))
    people[:, :, 0:2] += pose[:, None, 0:2]
    count = rng.integers(0, Np + 1, size=B).astype(np.int32)

    def call(s, a, fill):
        pb = _abi.SmpcPeopleBatch()
        pb.B, pb.Np, pb.N, pb.on_device = B, Np, N, a.on_device
        pb.people, pb.count = a("people", people), a("count", count)
        if fov:
            pb.robot_pose, pb.fov_angle, pb.costmap_origin = a("robot_pose", pose), 1.0, a("costmap_origin", np.zeros((1, 2)))
            pb.costmap_shared, pb.size_x, pb.size_y, pb.resolution = 1, 200, 200, 0.05
        out = a.empty("init_people", (B, N, 6), np.float64, fill)
        has = a.empty("has_people", B, np.uint8, fill)
        check(s.lib, s.lib.smpc_people_to_status_batch(s._h, C.byref(pb), C.c_void_p(out), C.c_void_p(has)), "smpc_people_to_status_batch")

    both_modes(call)


def memory(rng, B, T, lengths):
    m = {"prev_path": rng.normal(size=(B, T + 1, 3)), "prev_cmds": rng.normal(size=(B, T + 1, 2)),
         "valid": (rng.uniform(size=B) < 0.6).astype(np.int32)}
    if lengths:
        m["length"] = np.repeat(rng.integers(1, T + 2, size=(B, 1)), 2, axis=1).astype(np.int32)
    return m


def memory_batch(a, m):
    mb = _abi.SmpcMemoryBatch()
    for k, v in m.items():
        setattr(mb, k, a(k, v))
    return mb


@pytest.mark.parametrize("B,ragged", [(300, True), (16384, False)])  # the second stages 21 MB: beyond the mirror
def test_format(B, ragged):
    rng = np.random.default_rng(43)
    max_poses = 30
    T, rows = max_poses - 1, max_poses + 1
    P = README.dims(T, True)[3]
    path = np.concatenate([np.cumsum(rng.uniform(-0.03, 0.03, (B, rows, 2)), axis=1), rng.uniform(-np.pi, np.pi, (B, rows, 1))], 2)
    cmds, speed = rng.normal(size=(B, rows, 2)), rng.normal(size=(B, 2))
    n_poses = rng.integers(0, rows + 1, size=B).astype(np.int32)
    mem = memory(rng, B, T, ragged)

    def call(s, a, fill):
        fb = _abi.SmpcFormatBatch()
        fb.B, fb.T, fb.path_rows, fb.on_device = B, T, rows, a.on_device
        fb.time_step, fb.current_path_w, fb.current_cmds_w = 0.05, 0.7, 0.4
        fb.path, fb.cmds, fb.speed = a("path", path), a("cmds", cmds), a("speed", speed)
        fb.memory = memory_batch(a, mem)
        if ragged:
            fb.n_poses, fb.max_poses = a("n_poses", n_poses), max_poses
        fo = _abi.SmpcFormatOut()
        for k, shape, dt in (("robot_status", (B, T + 1, 6), np.float64), ("pose0", (B, 3), np.float64), ("init_params", (B, P), np.float64),
                             ("path_pts", (B, T + 1, 2), np.float64), ("goal_yaw", B, np.float64), ("T_scene", B, np.int32)):
            setattr(fo, k, a.empty(k, shape, dt, fill))
        check(s.lib, s.lib.smpc_format_to_optimize_batch(s._h, C.byref(fb), C.byref(fo)), "smpc_format_to_optimize_batch")

    got = both_modes(call)
    assert not np.array_equal(got["prev_path"], mem["prev_path"])


def test_memory_store():
    rng = np.random.default_rng(44)
    B, T = 257, 28
    status = rng.integers(0, 3, size=B).astype(np.int32)
    path, cmds = rng.normal(size=(B, T + 1, 3)), rng.normal(size=(B, T + 1, 2))
    T_scene = rng.integers(1, T + 1, size=B).astype(np.int32)
    mem = memory(rng, B, T, True)

    def call(s, a, fill):
        mb = memory_batch(a, mem)
        check(s.lib, s.lib.smpc_memory_store_batch(s._h, B, T, a.on_device, a("status", status), a("path", path), a("cmds", cmds),
                                                   C.byref(mb), a("T_scene", T_scene)), "smpc_memory_store_batch")

    got = both_modes(call)
    assert (got["valid"] == np.where(status == 2, mem["valid"], 1)).all()


def test_trajectorize():
    rng = np.random.default_rng(45)
    B, L = 200, 160
    tp = TrajectorizerParams()
    plan = arcs(rng, B, L)
    plan_len = rng.integers(3, L + 1, size=B).astype(np.int32)
    pose = poses_near(rng, plan, plan_len)
    S1 = tp.max_steps + 1

    def call(s, a, fill):
        tb = s.trajectorize_c(tp, B, L, a.on_device)
        tb.plan, tb.plan_len, tb.robot_pose = a("plan", plan), a("plan_len", plan_len), a("robot_pose", pose)
        to = _abi.SmpcTrajectorizeOut()
        for k, shape, dt in (("path", (B, S1, 3), np.float64), ("cmds", (B, S1, 2), np.float64), ("cmds_vy", (B, S1), np.float64),
                             ("n_poses", B, np.int32), ("error", B, np.int32)):
            setattr(to, k, a.empty(k, shape, dt, fill))
        check(s.lib, s.lib.smpc_trajectorize_path_batch(s._h, C.byref(tb), C.byref(to)), "smpc_trajectorize_path_batch")

    both_modes(call)


def test_transform_global_plan():
    rng = np.random.default_rng(46)
    B, L = 150, 400
    plan = arcs(rng, B, L)
    plan_len = rng.integers(2, L + 1, size=B).astype(np.int32)
    pose = poses_near(rng, plan, plan_len)
    pose[5::11, :2] += 25.0  # far off the plan: empty window
    start = np.minimum(rng.integers(0, 4, size=B), plan_len - 1).astype(np.int32)
    to_local = np.stack([rng.uniform(-2, 2, B), rng.uniform(-2, 2, B), rng.uniform(-3, 3, B)], 1)

    def call(s, a, fill):
        wb = _abi.SmpcPlanWindowBatch()
        wb.B, wb.L, wb.on_device, wb.max_robot_pose_search_dist, wb.dist_threshold = B, L, a.on_device, 1.5, 4.0
        wb.plan, wb.plan_len, wb.plan_start = a("plan", plan), a("plan_len", plan_len), a("plan_start", start)
        wb.robot_pose, wb.to_local = a("robot_pose", pose), a("to_local", to_local)
        window = a.empty("window", (B, L, 2), np.float64, fill)
        wlen, err = a.empty("window_len", B, np.int32, fill), a.empty("error", B, np.int32, fill)
        check(s.lib, s.lib.smpc_transform_global_plan_batch(s._h, C.byref(wb), C.c_void_p(window), C.c_void_p(wlen), C.c_void_p(err)),
              "smpc_transform_global_plan_batch")

    got = both_modes(call)
    assert (got["plan_start"] > start).any() and (got["window_len"] == 0).any()


def test_select_command():
    rng = np.random.default_rng(47)
    B, T, rows = 300, 28, 31
    traj_cmds, cmds = rng.normal(size=(B, rows, 2)), rng.normal(size=(B, T + 1, 2))
    status = rng.integers(0, 3, size=B).astype(np.int32)
    n = rng.choice([0, 5, T + 1, rows], size=B).astype(np.int32)
    werr = rng.choice([0, 0, 0, 1, 2], size=B).astype(np.int32)

    def call(s, a, fill):
        out, src = a.empty("cmd_vel", (B, 2), np.float64, fill), a.empty("source", B, np.int32, fill)
        check(s.lib, s.lib.smpc_select_command_batch(s._h, B, T, rows, a.on_device, a("traj_n_poses", n), a("traj_cmds", traj_cmds),
                                                     a("status", status), a("cmds", cmds), out, src, a("window_error", werr)),
              "smpc_select_command_batch")

    got = both_modes(call)
    assert set(got["source"].tolist()) == {0, 1, 2, 3}
