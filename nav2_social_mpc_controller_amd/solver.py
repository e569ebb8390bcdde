"""Python host side above the C ABI (include/smpc.h): loads csrc/libsmpc_hip.so and mirrors the part of the
reference's `Optimizer` interface that sits on the hot path (optimizer.hpp:152,167-170):

    Optimizer.initialize(OptimizerParams)   -> BatchSolver(params)
    Optimizer.optimize(...) for B scenes     -> BatchSolver.solve(scenes) / solve_device(...)

There is NO CPU fallback: a missing library or a missing HIP device raises.
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import (SmpcCrowdBatch, SmpcCrowdGroups, SmpcEvalOut, SmpcFormatBatch, SmpcFormatOut, SmpcMemoryBatch, SmpcMetricsBatch, SmpcObstacleDistanceIn,
                   SmpcObstacleDistanceOut, SmpcParams, SmpcPeopleBatch, SmpcPlanWindowBatch, SmpcProjectionBatch, SmpcResultBatch, SmpcSceneBatch, SmpcTraceOut,
                   SmpcTrajectorizeBatch, SmpcTrajectorizeOut)
from .params import CrowdGroupParams, CrowdParams, MetricsParams, OptimizerParams, TrajectorizerParams
from .scenes import SceneBatch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMPC_LIB_PATH", os.path.join(_HERE, "csrc", "libsmpc_hip.so"))  # env override: A/B builds
_lib = None
# columns of a trace row (smpc_trace_out, include/smpc.h): one row per LM iteration
TRACE_COLS = ["iter", "cost", "cost_change", "gradient_max_norm", "step_norm", "rho", "radius", "ls_evals", "accepted"]
assert len(TRACE_COLS) == _abi.SMPC_TRACE_COLS
# columns of a metrics row (enum smpc_metric_col, include/smpc.h): one row per robot, accumulated over an episode
METRIC_COLS = ["samples", "path_length", "heading_change", "sum_speed", "people_samples", "min_person_dist",
               "sum_min_person_dist", "intimate_samples", "personal_samples", "social_samples", "person_collision_samples",
               "social_work", "min_clearance", "obstacle_collision_samples", "off_grid_samples", "time_to_goal", "goal_dist",
               "fallback_samples", "unusable_solves", "last_x", "last_y", "last_yaw", "reserved0", "reserved1"]
assert len(METRIC_COLS) == _abi.SMPC_METRIC_COLS


class SmpcError(RuntimeError):
    pass


def load_library():
    """dlopen libsmpc_hip.so (built by __graft_entry__.build() / csrc/build.sh). Fails loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SmpcError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). There is no CPU fallback for the solver.")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 and no longer finds a GPU when it is imported
    # after this library has initialised /opt/rocm's copy, so when torch is installed it goes first (it is only the
    # allocator / stream plumbing of the device-resident paths; the host-array paths never touch it).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.smpc_abi_version.restype = C.c_int
    lib.smpc_last_error.restype = C.c_char_p
    lib.smpc_params_default.argtypes = [C.POINTER(SmpcParams)]
    lib.smpc_params_default.restype = None
    lib.smpc_dims.restype = C.c_int
    lib.smpc_dims.argtypes = [C.POINTER(SmpcParams), C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 6
    lib.smpc_create.restype = C.c_void_p
    lib.smpc_create.argtypes = [C.POINTER(SmpcParams), C.c_int]
    lib.smpc_destroy.argtypes = [C.c_void_p]
    lib.smpc_destroy.restype = None
    lib.smpc_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.smpc_set_stream.restype = C.c_int
    lib.smpc_set_solve_share.argtypes = [C.c_void_p, C.c_int32]
    lib.smpc_set_solve_share.restype = C.c_int
    lib.smpc_solve_slot_width.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.smpc_solve_slot_width.restype = C.c_int
    lib.smpc_solve_batch.argtypes = [C.c_void_p, C.POINTER(SmpcSceneBatch), C.POINTER(SmpcResultBatch)]
    lib.smpc_solve_batch.restype = C.c_int
    lib.smpc_solve_trace_batch.argtypes = [C.c_void_p, C.POINTER(SmpcSceneBatch), C.POINTER(SmpcResultBatch), C.POINTER(SmpcTraceOut)]
    lib.smpc_solve_trace_batch.restype = C.c_int
    lib.smpc_eval_batch.argtypes = [C.c_void_p, C.POINTER(SmpcSceneBatch), C.c_void_p, C.POINTER(SmpcEvalOut)]
    lib.smpc_eval_batch.restype = C.c_int
    lib.smpc_project_people_batch.argtypes = [C.c_void_p, C.POINTER(SmpcProjectionBatch), C.c_void_p, C.c_void_p]
    lib.smpc_project_people_batch.restype = C.c_int
    lib.smpc_obstacle_distance_batch.argtypes = [C.c_void_p, C.POINTER(SmpcObstacleDistanceIn), C.POINTER(SmpcObstacleDistanceOut)]
    lib.smpc_obstacle_distance_batch.restype = C.c_int
    lib.smpc_people_to_status_batch.argtypes = [C.c_void_p, C.POINTER(SmpcPeopleBatch), C.c_void_p, C.c_void_p]
    lib.smpc_people_to_status_batch.restype = C.c_int
    lib.smpc_format_to_optimize_batch.argtypes = [C.c_void_p, C.POINTER(SmpcFormatBatch), C.POINTER(SmpcFormatOut)]
    lib.smpc_format_to_optimize_batch.restype = C.c_int
    lib.smpc_memory_store_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(SmpcMemoryBatch), C.c_void_p]
    lib.smpc_memory_store_batch.restype = C.c_int
    lib.smpc_trajectorize_path_batch.argtypes = [C.c_void_p, C.POINTER(SmpcTrajectorizeBatch), C.POINTER(SmpcTrajectorizeOut)]
    lib.smpc_trajectorize_path_batch.restype = C.c_int
    lib.smpc_transform_global_plan_batch.argtypes = [C.c_void_p, C.POINTER(SmpcPlanWindowBatch), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.smpc_transform_global_plan_batch.restype = C.c_int
    lib.smpc_select_command_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7
    lib.smpc_select_command_batch.restype = C.c_int
    lib.smpc_episode_metrics_batch.argtypes = [C.c_void_p, C.POINTER(SmpcMetricsBatch), C.c_void_p]
    lib.smpc_episode_metrics_batch.restype = C.c_int
    lib.smpc_crowd_step_batch.argtypes = [C.c_void_p, C.POINTER(SmpcCrowdBatch), C.c_void_p, C.c_void_p]
    lib.smpc_crowd_step_batch.restype = C.c_int
    lib.smpc_crowd_step_groups_batch.argtypes = [C.c_void_p, C.POINTER(SmpcCrowdBatch), C.POINTER(SmpcCrowdGroups), C.c_void_p, C.c_void_p]
    lib.smpc_crowd_step_groups_batch.restype = C.c_int
    lib.smpc_stage_people_batch.argtypes = [C.c_void_p, C.POINTER(SmpcSceneBatch), C.c_void_p, C.c_void_p]
    lib.smpc_stage_people_batch.restype = C.c_int
    lib.smpc_fp64_peak_probe.argtypes = [C.c_void_p, C.c_int32]
    lib.smpc_fp64_peak_probe.restype = C.c_double
    lib.smpc_math_probe.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4
    lib.smpc_math_probe.restype = C.c_int
    lib.smpc_last_kernel_ms.argtypes = [C.c_void_p]
    lib.smpc_last_kernel_ms.restype = C.c_double
    if lib.smpc_abi_version() != _abi.SMPC_ABI_VERSION:
        raise SmpcError("libsmpc_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _check(lib, rc, what):
    if rc != 0:
        raise SmpcError(f"{what} failed ({rc}): {lib.smpc_last_error().decode()}")


def summarize_metrics(acc: np.ndarray, dt: float) -> dict:
    """Per-robot values derived from metrics rows acc [B,24] (columns METRIC_COLS) of an episode with control period dt:
    success (goal reached), time_to_goal (NaN without success), duration (samples * dt), path_length, mean_speed,
    min_person_dist, mean_min_person_dist (over the samples with people; NaN without any), social_work_per_metre (NaN for a
    robot that did not move), intimate_share / personal_share / social_share (of the samples with people; 0 without any),
    min_clearance, person_collision / obstacle_collision (any sample), fallback_share and unusable_share (of all
    samples). A row without samples gives NaN shares and means."""
    acc = np.asarray(acc, np.float64)
    assert acc.ndim == 2 and acc.shape[1] == _abi.SMPC_METRIC_COLS
    c = {name: acc[:, i] for i, name in enumerate(METRIC_COLS)}
    n, npl = c["samples"], c["people_samples"]
    with np.errstate(divide="ignore", invalid="ignore"):
        per_sample = lambda v: np.where(n > 0, v / n, np.nan)
        per_people = lambda v, empty: np.where(npl > 0, v / npl, np.where(n > 0, empty, np.nan))
        success = (n > 0) & (c["time_to_goal"] >= 0)  # (a zero-filled row is an empty one, not an arrival at t = 0)
        return {
            "success": success,
            "time_to_goal": np.where(success, c["time_to_goal"], np.nan),
            "duration": n * float(dt),
            "path_length": c["path_length"].copy(),
            "mean_speed": per_sample(c["sum_speed"]),
            "min_person_dist": c["min_person_dist"].copy(),
            "mean_min_person_dist": per_people(c["sum_min_person_dist"], np.nan),
            "social_work_per_metre": np.where(c["path_length"] > 0, c["social_work"] / c["path_length"], np.nan),
            "intimate_share": per_people(c["intimate_samples"], 0.0),
            "personal_share": per_people(c["personal_samples"], 0.0),
            "social_share": per_people(c["social_samples"], 0.0),
            "min_clearance": c["min_clearance"].copy(),
            "person_collision": c["person_collision_samples"] > 0,
            "obstacle_collision": c["obstacle_collision_samples"] > 0,
            "fallback_share": per_sample(c["fallback_samples"]),
            "unusable_share": per_sample(c["unusable_solves"]),
        }


class BatchSolver:
    """One solver bound to one HIP device; mirrors Optimizer::initialize + Optimizer::optimize for B scenes."""

    def __init__(self, params: OptimizerParams, device: int = 0):
        self.lib = load_library()
        self.params = params
        self._cparams = params.to_c()
        self._h = self.lib.smpc_create(C.byref(self._cparams), int(device))
        if not self._h:
            raise SmpcError(f"smpc_create failed: {self.lib.smpc_last_error().decode()}")
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self.lib.smpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int):
        _check(self.lib, self.lib.smpc_set_stream(self._h, C.c_void_p(stream_ptr)), "smpc_set_stream")

    def set_solve_share(self, n: int):
        """smpc_set_solve_share: this handle's solve launches leave room for n - 1 concurrent ones (other streams)."""
        _check(self.lib, self.lib.smpc_set_solve_share(self._h, int(n)), "smpc_set_solve_share")

    def solve_slot_width(self, B: int, T: int, N: int) -> int:
        """smpc_solve_slot_width: 32 (two scenes per wave) or 64 (one) for a solve launch of this shape."""
        w = self.lib.smpc_solve_slot_width(self._h, int(B), int(T), int(N))
        if w < 0:
            _check(self.lib, w, "smpc_solve_slot_width")
        return w

    def math_probe(self, fn: int, a: np.ndarray, b: np.ndarray = None):
        """smpc_math_probe: the sweep's elementary functions evaluated on the device (see include/smpc.h)."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        n = a.size // 8 if fn == 7 else a.size
        bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        o0 = np.empty(n)
        o1 = np.empty(n)
        _check(self.lib, self.lib.smpc_math_probe(self._h, int(fn), n, a.ctypes.data, None if bb is None else bb.ctypes.data,
                                                  o0.ctypes.data, o1.ctypes.data), "smpc_math_probe")
        return o0, o1

    def fp64_peak_tflops(self, iters: int = 20000) -> float:
        """Measured FP64 vector peak of this device (smpc_fp64_peak_probe)."""
        return float(self.lib.smpc_fp64_peak_probe(self._h, int(iters)))

    def last_kernel_ms(self) -> float:
        return float(self.lib.smpc_last_kernel_ms(self._h))

    # -- host-memory path (stages through HBM inside the library) ---------------------------------
    def _solve_call(self, scenes: SceneBatch, order):
        """What solve() and solve_trace() hand to the library: (result dict of host arrays, SmpcSceneBatch, SmpcResultBatch,
        the arrays the structs point into)."""
        CH, bl, nb, P, M, _ = self.params.dims(scenes.T, True)
        scenes.validate(P)
        B, T = scenes.B, scenes.T
        out = {
            "params": np.zeros((B, P)), "cmds": np.zeros((B, T + 1, 2)), "path": np.zeros((B, T + 1, 3)),
            "status": np.zeros(B, np.int32), "reason": np.zeros(B, np.int32), "iterations": np.zeros(B, np.int32),
            "evaluations": np.zeros(B, np.int32), "initial_cost": np.zeros(B), "final_cost": np.zeros(B),
        }
        rb = SmpcResultBatch()
        for k, v in out.items():
            setattr(rb, k, v.ctypes.data)
        sb = scenes.to_c()
        if order is not None:
            order = np.ascontiguousarray(order, np.int32)
            assert order.shape == (B,)
            sb.order = order.ctypes.data
        return out, sb, rb, order

    def solve(self, scenes: SceneBatch, order: np.ndarray = None):
        """Solve B scenes (host arrays in, host arrays out). order: optional queue order of the persistent kernel, a
        permutation of 0..B-1 (smpc_scene_batch.order: longest scenes first shortens a lone launch; results do not
        depend on it)."""
        out, sb, rb, _keep = self._solve_call(scenes, order)
        _check(self.lib, self.lib.smpc_solve_batch(self._h, C.byref(sb), C.byref(rb)), "smpc_solve_batch")
        return out

    def solve_trace(self, scenes: SceneBatch, order: np.ndarray = None, max_rows: int = None):
        """solve() that also returns the per-iteration record of every scene (optimizer.debug_optimizer; smpc_solve_trace_batch):
        "trace" [B, max_rows, 9], columns TRACE_COLS, row i = LM iteration i, NaN where a scene has no row; "trace_rows" [B],
        the rows each solve produced (more than max_rows: the rest were dropped). max_rows defaults to max_iterations + 1,
        which holds every row. The other entries are those of solve(), bit for bit."""
        max_rows = self.params.max_iterations + 1 if max_rows is None else int(max_rows)
        if max_rows < 0:
            raise SmpcError(f"max_rows must be >= 0, got {max_rows}")
        out, sb, rb, _keep = self._solve_call(scenes, order)
        out["trace"] = np.full((scenes.B, max_rows, _abi.SMPC_TRACE_COLS), np.nan)
        out["trace_rows"] = np.zeros(scenes.B, np.int32)
        to = SmpcTraceOut(out["trace"].ctypes.data if out["trace"].size else None, max_rows, out["trace_rows"].ctypes.data)
        _check(self.lib, self.lib.smpc_solve_trace_batch(self._h, C.byref(sb), C.byref(rb), C.byref(to)), "smpc_solve_trace_batch")
        return out

    @staticmethod
    def longest_first(evaluations):
        """Queue order for the next solve of the same (or the next control period's) scenes from the sweep counts of the
        last one: a torch int32 tensor on the device of `evaluations`, scenes with the most sweeps first."""
        import torch

        return torch.argsort(evaluations, descending=True, stable=True).to(torch.int32)

    def row_permutation(self, T: int, has_people: bool = True):
        """perm with reference_rows = critic_major_rows[perm] (smpc_eval_batch_out.row_order 1 -> 0) for one scene."""
        CH, bl, nb, P, M, _ = self.params.dims(T, has_people)
        rps = 8 if has_people else 5
        nfeas = M - rps * T
        perm = np.empty(M, np.int64)
        for t in range(T):
            base = rps * t + min(max(t - 1, 0), nfeas)
            for c in range(rps):
                perm[base + c] = c * T + t
            if 1 <= t <= nfeas:
                perm[base + rps] = rps * T + (t - 1)
        return perm

    def evaluate(self, scenes: SceneBatch, x: np.ndarray, row_order: int = 0):
        CH, bl, nb, P, M, _ = self.params.dims(scenes.T, True)
        scenes.validate(P)
        B = scenes.B
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (B, P)
        out = {"residuals": np.zeros((B, M)), "jacobian": np.zeros((B, M, P)), "cost": np.zeros(B),
               "gradient": np.zeros((B, P))}
        eo = SmpcEvalOut()
        for k, v in out.items():
            setattr(eo, k, v.ctypes.data)
        eo.row_order = int(row_order)
        sb = scenes.to_c()
        _check(self.lib, self.lib.smpc_eval_batch(self._h, C.byref(sb), x.ctypes.data, C.byref(eo)), "smpc_eval_batch")
        return out

    # -- people projection: Optimizer::project_people for B scenes -------------
    def project_people(self, init_people: np.ndarray, robot_path: np.ndarray, od_indexes: np.ndarray,
                       od_origin: np.ndarray, od_resolution: float, max_time: float, time_step: float):
        """init_people [B,N,6], robot_path [B,T+1,6], od_indexes [B or 1,h,w] uint32, od_origin [B or 1,2].
        Returns (people_proj [B,T+1,6,N], error [B])."""
        init_people = np.ascontiguousarray(init_people, np.float64)
        robot_path = np.ascontiguousarray(robot_path, np.float64)
        od_indexes = np.ascontiguousarray(od_indexes, np.uint32)
        od_origin = np.ascontiguousarray(od_origin, np.float64)
        B, N, _ = init_people.shape
        T = robot_path.shape[1] - 1
        pb = SmpcProjectionBatch()
        pb.B, pb.T, pb.N, pb.on_device = B, T, N, 0
        pb.max_time, pb.time_step = float(max_time), float(time_step)
        pb.init_people, pb.robot_path = init_people.ctypes.data, robot_path.ctypes.data
        pb.od_indexes = od_indexes.ctypes.data if od_indexes.size else None
        pb.od_shared = 1 if od_indexes.shape[0] == 1 else 0
        pb.od_height, pb.od_width = (int(od_indexes.shape[1]), int(od_indexes.shape[2])) if od_indexes.ndim == 3 else (0, 0)
        pb.od_resolution = float(od_resolution)
        pb.od_origin = od_origin.ctypes.data
        out = np.zeros((B, T + 1, 6, N))
        err = np.zeros(B, np.int32)
        _check(self.lib, self.lib.smpc_project_people_batch(self._h, C.byref(pb), out.ctypes.data, err.ctypes.data),
               "smpc_project_people_batch")
        return out, err

    # -- the ObstacleDistance grid of the projection, from the costmaps (smpc_obstacle_distance_batch) -----------
    @staticmethod
    def obstacle_distance_c(B: int, size_x: int, size_y: int, costmap_shared: bool, resolution: float, on_device: int,
                            obstacle_min_cost: int = 254, unknown_is_obstacle: bool = False) -> SmpcObstacleDistanceIn:
        ob = SmpcObstacleDistanceIn()
        ob.B, ob.size_x, ob.size_y, ob.on_device = int(B), int(size_x), int(size_y), int(on_device)
        ob.costmap_shared = 1 if costmap_shared else 0
        if not 1 <= int(obstacle_min_cost) <= 255:
            raise SmpcError(f"obstacle_min_cost must be 1..255, got {obstacle_min_cost}")
        ob.obstacle_min_cost, ob.unknown_is_obstacle = int(obstacle_min_cost), 1 if unknown_is_obstacle else 0
        ob.resolution = float(resolution)
        return ob

    def obstacle_distance(self, costmap: np.ndarray, resolution: float, obstacle_min_cost: int = 254,
                          unknown_is_obstacle: bool = False, distances: bool = True):
        """costmap [B,H,W] uint8 (one grid per scene) or [H,W] (one shared grid). Returns dict(indexes [..,H,W] uint32,
        distances [..,H,W] float32 or None, n_obstacles [B or 1] int32): the exact nearest-obstacle transform of
        include/smpc.h, shaped like `costmap`."""
        costmap = np.ascontiguousarray(costmap, np.uint8)
        shared = costmap.ndim == 2
        cm = costmap[None] if shared else costmap
        G, H, W = cm.shape
        ob = self.obstacle_distance_c(G, W, H, shared, resolution, 0, obstacle_min_cost, unknown_is_obstacle)
        ob.costmap = cm.ctypes.data if cm.size else None
        out = {"indexes": np.zeros(cm.shape, np.uint32), "distances": np.zeros(cm.shape, np.float32) if distances else None,
               "n_obstacles": np.zeros(G, np.int32)}
        oo = SmpcObstacleDistanceOut()
        oo.indexes, oo.n_obstacles = out["indexes"].ctypes.data, out["n_obstacles"].ctypes.data
        oo.distances = out["distances"].ctypes.data if distances else None
        _check(self.lib, self.lib.smpc_obstacle_distance_batch(self._h, C.byref(ob), C.byref(oo)), "smpc_obstacle_distance_batch")
        if shared:
            out["indexes"] = out["indexes"][0]
            out["distances"] = None if out["distances"] is None else out["distances"][0]
        return out

    def obstacle_distance_device(self, ob: SmpcObstacleDistanceIn, indexes_ptr: int, distances_ptr: int = 0,
                                 n_obstacles_ptr: int = 0):
        """Device pointers in and out (ob.on_device == 1), asynchronous on the handle's stream."""
        assert ob.on_device == 1
        oo = SmpcObstacleDistanceOut()
        oo.indexes, oo.distances, oo.n_obstacles = indexes_ptr or None, distances_ptr or None, n_obstacles_ptr or None
        _check(self.lib, self.lib.smpc_obstacle_distance_batch(self._h, C.byref(ob), C.byref(oo)), "smpc_obstacle_distance_batch")

    # -- initial-guess generator: PathTrajectorizer::trajectorize for B plans ------------------
    @staticmethod
    def trajectorize_c(tp: TrajectorizerParams, B: int, L: int, on_device: int) -> SmpcTrajectorizeBatch:
        tb = SmpcTrajectorizeBatch()
        tb.B, tb.L, tb.max_steps, tb.on_device = B, L, tp.max_steps, on_device
        tb.omnidirectional = 1 if tp.omnidirectional else 0
        tb.desired_linear_vel, tb.lookahead_dist = tp.desired_linear_vel, tp.lookahead_dist
        tb.max_angular_vel, tb.time_step = tp.max_angular_vel, tp.time_step
        return tb

    def trajectorize(self, tp: TrajectorizerParams, plan: np.ndarray, plan_len: np.ndarray, robot_pose: np.ndarray):
        """plan [B,L,2], plan_len [B], robot_pose [B,3] (x, y, yaw). Returns dict(path [B,S+1,3], cmds [B,S+1,2],
        cmds_vy [B,S+1], n_poses [B], error [B]) with S = tp.max_steps."""
        plan = np.ascontiguousarray(plan, np.float64)
        plan_len = np.ascontiguousarray(plan_len, np.int32)
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        B, L, _ = plan.shape
        tb = self.trajectorize_c(tp, B, L, 0)
        tb.plan, tb.plan_len, tb.robot_pose = plan.ctypes.data, plan_len.ctypes.data, robot_pose.ctypes.data
        S1 = tp.max_steps + 1
        out = {"path": np.zeros((B, S1, 3)), "cmds": np.zeros((B, S1, 2)), "cmds_vy": np.zeros((B, S1)),
               "n_poses": np.zeros(B, np.int32), "error": np.zeros(B, np.int32)}
        to = SmpcTrajectorizeOut()
        for k, v in out.items():
            setattr(to, k, v.ctypes.data)
        _check(self.lib, self.lib.smpc_trajectorize_path_batch(self._h, C.byref(tb), C.byref(to)), "smpc_trajectorize_path_batch")
        return out

    def transform_global_plan(self, plan: np.ndarray, plan_len: np.ndarray, plan_start: np.ndarray, robot_pose: np.ndarray,
                              max_robot_pose_search_dist: float, dist_threshold: float, to_local: np.ndarray = None):
        """PathHandler::transformGlobalPlan for B robots (smpc_transform_global_plan_batch): plan [B,L,2], plan_len [B],
        plan_start [B] (updated in place: the pruning), robot_pose [B,3] in the plan frame, to_local [B,3] or None.
        Returns dict(window [B,L,2], window_len [B], error [B])."""
        plan = np.ascontiguousarray(plan, np.float64)
        plan_len = np.ascontiguousarray(plan_len, np.int32)
        assert plan_start.dtype == np.int32 and plan_start.flags.c_contiguous
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        B, L, _ = plan.shape
        wb = SmpcPlanWindowBatch()
        wb.B, wb.L, wb.on_device = B, L, 0
        wb.max_robot_pose_search_dist, wb.dist_threshold = float(max_robot_pose_search_dist), float(dist_threshold)
        wb.plan, wb.plan_len, wb.plan_start, wb.robot_pose = plan.ctypes.data, plan_len.ctypes.data, plan_start.ctypes.data, robot_pose.ctypes.data
        if to_local is not None:
            to_local = np.ascontiguousarray(to_local, np.float64)
            wb.to_local = to_local.ctypes.data
        out = {"window": np.zeros((B, L, 2)), "window_len": np.zeros(B, np.int32), "error": np.zeros(B, np.int32)}
        _check(self.lib, self.lib.smpc_transform_global_plan_batch(self._h, C.byref(wb), out["window"].ctypes.data,
                                                                   out["window_len"].ctypes.data, out["error"].ctypes.data),
               "smpc_transform_global_plan_batch")
        return out

    def transform_global_plan_device(self, wb: "SmpcPlanWindowBatch", window_ptr: int, window_len_ptr: int, error_ptr: int = 0):
        assert wb.on_device == 1
        _check(self.lib, self.lib.smpc_transform_global_plan_batch(self._h, C.byref(wb), C.c_void_p(window_ptr),
                                                                   C.c_void_p(window_len_ptr), C.c_void_p(error_ptr)),
               "smpc_transform_global_plan_batch")

    def trajectorize_device(self, tb: SmpcTrajectorizeBatch, to: SmpcTrajectorizeOut):
        assert tb.on_device == 1
        _check(self.lib, self.lib.smpc_trajectorize_path_batch(self._h, C.byref(tb), C.byref(to)), "smpc_trajectorize_path_batch")

    def people_to_status(self, people: np.ndarray, count: np.ndarray, N: int = 3, robot_pose: np.ndarray = None,
                         fov_angle: float = np.pi / 4, costmap_origin: np.ndarray = None, size_x: int = 0, size_y: int = 0,
                         resolution: float = 0.0):
        """Optimizer::people_to_status for B scenes: people [B,Np,5] (px, py, vx, vy, vz), count [B] ->
        (init_people [B,N,6], has_people [B] uint8). With robot_pose [B,3] the field-of-view filter of
        computeVelocityCommands runs first (costmap_origin [B or 1,2], size_x/size_y cells, resolution)."""
        people = np.ascontiguousarray(people, np.float64)
        count = np.ascontiguousarray(count, np.int32)
        B, Np, _ = people.shape
        pb = SmpcPeopleBatch()
        pb.B, pb.Np, pb.N, pb.on_device = B, Np, N, 0
        pb.people, pb.count = people.ctypes.data, count.ctypes.data
        if robot_pose is not None:
            robot_pose = np.ascontiguousarray(robot_pose, np.float64)
            costmap_origin = np.ascontiguousarray(costmap_origin, np.float64).reshape(-1, 2)
            pb.robot_pose, pb.fov_angle = robot_pose.ctypes.data, float(fov_angle)
            pb.costmap_origin, pb.costmap_shared = costmap_origin.ctypes.data, 1 if costmap_origin.shape[0] == 1 else 0
            pb.size_x, pb.size_y, pb.resolution = int(size_x), int(size_y), float(resolution)
        out, has = np.zeros((B, N, 6)), np.zeros(B, np.uint8)
        _check(self.lib, self.lib.smpc_people_to_status_batch(self._h, C.byref(pb), out.ctypes.data, has.ctypes.data),
               "smpc_people_to_status_batch")
        return out, has

    def select_command(self, traj_n_poses, traj_cmds: np.ndarray, status: np.ndarray, cmds: np.ndarray, window_error=None):
        """The command computeVelocityCommands returns for B robots (fallbacks included): traj_cmds [B,rows,2],
        status [B], cmds [B,T+1,2], traj_n_poses [B] or None, window_error [B] (smpc_window_error of this cycle) or None.
        Returns (cmd_vel [B,2], source [B])."""
        traj_cmds = np.ascontiguousarray(traj_cmds, np.float64)
        status = np.ascontiguousarray(status, np.int32)
        cmds = np.ascontiguousarray(cmds, np.float64)
        B, rows, _ = traj_cmds.shape
        T = cmds.shape[1] - 1
        n = None if traj_n_poses is None else np.ascontiguousarray(traj_n_poses, np.int32)
        out, src = np.zeros((B, 2)), np.zeros(B, np.int32)
        we = None if window_error is None else np.ascontiguousarray(window_error, np.int32)
        _check(self.lib, self.lib.smpc_select_command_batch(self._h, B, T, rows, 0, None if n is None else n.ctypes.data,
                                                            traj_cmds.ctypes.data, status.ctypes.data, cmds.ctypes.data,
                                                            out.ctypes.data, src.ctypes.data,
                                                            None if we is None else we.ctypes.data), "smpc_select_command_batch")
        return out, src

    # -- per-robot navigation metrics of a closed-loop episode (smpc_episode_metrics_batch) ------------------------
    @staticmethod
    def metrics_c(mp: MetricsParams, B: int, Np: int, dt: float, on_device: int) -> SmpcMetricsBatch:
        mb = SmpcMetricsBatch()
        mb.B, mb.Np, mb.on_device, mb.dt = int(B), int(Np), int(on_device), float(dt)
        mb.goal_tolerance, mb.robot_radius, mb.person_radius = mp.goal_tolerance, mp.robot_radius, mp.person_radius
        mb.intimate_radius, mb.personal_radius, mb.social_radius = mp.intimate_radius, mp.personal_radius, mp.social_radius
        return mb

    def episode_metrics(self, mp: MetricsParams, dt: float, acc: np.ndarray, robot_pose: np.ndarray, robot_twist: np.ndarray,
                        people: np.ndarray, count: np.ndarray, goal: np.ndarray = None, od_distances: np.ndarray = None,
                        od_origin: np.ndarray = None, od_resolution: float = None, status: np.ndarray = None,
                        source: np.ndarray = None) -> np.ndarray:
        """One sample folded into the metrics rows (host arrays): acc [B,24] (zeros: empty rows), robot_pose [B,3],
        robot_twist [B,2], people [B,Np,5], count [B]; optional goal [B,2], od_distances [h,w] (one shared grid, od_origin
        [2]) or [B,h,w] (od_origin [B,2]) float32 with od_resolution, status [B] and source [B] of the tick. Returns the
        updated copy of acc (columns METRIC_COLS)."""
        acc = np.array(acc, dtype=np.float64, order="C")
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        robot_twist = np.ascontiguousarray(robot_twist, np.float64)
        people = np.ascontiguousarray(people, np.float64)
        count = np.ascontiguousarray(count, np.int32)
        B, Np, _ = people.shape
        assert acc.shape == (B, _abi.SMPC_METRIC_COLS) and robot_pose.shape == (B, 3) and robot_twist.shape == (B, 2)
        assert count.shape == (B,) and people.shape[2] == 5
        mb = self.metrics_c(mp, B, Np, dt, 0)
        mb.robot_pose, mb.robot_twist = robot_pose.ctypes.data, robot_twist.ctypes.data
        mb.people, mb.count = people.ctypes.data, count.ctypes.data
        keep = []
        if goal is not None:
            goal = np.ascontiguousarray(goal, np.float64)
            assert goal.shape == (B, 2)
            mb.goal = goal.ctypes.data
        if od_distances is not None:
            od_distances = np.ascontiguousarray(od_distances, np.float32)
            shared = od_distances.ndim == 2
            od_origin = np.ascontiguousarray(od_origin, np.float64).reshape(-1, 2)
            assert od_distances.ndim == 2 or od_distances.shape[0] == B
            assert od_origin.shape == ((1, 2) if shared else (B, 2))
            mb.od_distances, mb.od_origin = od_distances.ctypes.data, od_origin.ctypes.data
            mb.od_shared, mb.od_height, mb.od_width = 1 if shared else 0, int(od_distances.shape[-2]), int(od_distances.shape[-1])
            mb.od_resolution = float(od_resolution)
        for name, arr in (("status", status), ("source", source)):
            if arr is not None:
                arr = np.ascontiguousarray(arr, np.int32)
                assert arr.shape == (B,)
                keep.append(arr)
                setattr(mb, name, arr.ctypes.data)
        _check(self.lib, self.lib.smpc_episode_metrics_batch(self._h, C.byref(mb), acc.ctypes.data), "smpc_episode_metrics_batch")
        return acc

    def episode_metrics_device(self, mb: SmpcMetricsBatch, acc_ptr: int):
        """Device pointers in mb (on_device == 1) and for acc; asynchronous on the handle's stream."""
        assert mb.on_device == 1
        _check(self.lib, self.lib.smpc_episode_metrics_batch(self._h, C.byref(mb), C.c_void_p(acc_ptr)), "smpc_episode_metrics_batch")

    # -- the reactive crowd of a closed-loop episode (smpc_crowd_step_batch) -----------------------------------------
    @staticmethod
    def crowd_c(cp: CrowdParams, B: int, Np: int, K: int, dt: float, on_device: int) -> SmpcCrowdBatch:
        cb = SmpcCrowdBatch()
        cb.B, cb.Np, cb.K, cb.on_device, cb.dt = int(B), int(Np), int(K), int(on_device), float(dt)
        cb.cyclic, cb.robot_visible = 1 if cp.cyclic else 0, 1 if cp.robot_visible else 0
        cb.goal_radius, cb.person_radius, cb.desired_speed = cp.goal_radius, cp.person_radius, cp.desired_speed
        return cb

    @staticmethod
    def crowd_groups_c(gp: CrowdGroupParams, group_id_ptr: int) -> SmpcCrowdGroups:
        gb = SmpcCrowdGroups()
        gb.group_id = group_id_ptr
        gb.factor_gaze, gb.factor_coherence, gb.factor_repulsion = gp.factor_gaze, gp.factor_coherence, gp.factor_repulsion
        return gb

    def crowd_step(self, cp: CrowdParams, dt: float, people: np.ndarray, cursor: np.ndarray, robot_pose: np.ndarray,
                   robot_twist: np.ndarray, count: np.ndarray, waypoints: np.ndarray, n_waypoints: np.ndarray,
                   desired_speeds: np.ndarray = None, od_indexes: np.ndarray = None, od_origin: np.ndarray = None,
                   od_resolution: float = None, groups: np.ndarray = None, group_params: CrowdGroupParams = None):
        """One control period of the crowd (host arrays): people [B,Np,5], cursor [B,Np], robot_pose [B,3] at the start of
        the period, robot_twist [B,2], count [B], waypoints [B,Np,K,2], n_waypoints [B,Np]; optional desired_speeds [B,Np],
        od_indexes [h,w] (one shared grid, od_origin [2]) or [B,h,w] (od_origin [B,2]) uint32 with od_resolution.
        groups [B,Np] int32 group ids (< 0: none) with group_params (default CrowdGroupParams()): the step with group forces
        (smpc_crowd_step_groups_batch); None: the plain step. Returns the updated copies (people, cursor)."""
        people = np.array(people, dtype=np.float64, order="C")
        cursor = np.array(cursor, dtype=np.int32, order="C")
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        robot_twist = np.ascontiguousarray(robot_twist, np.float64)
        count = np.ascontiguousarray(count, np.int32)
        waypoints = np.ascontiguousarray(waypoints, np.float64)
        n_waypoints = np.ascontiguousarray(n_waypoints, np.int32)
        B, Np, _ = people.shape
        K = waypoints.shape[2]
        assert people.shape[2] == 5 and cursor.shape == (B, Np) and robot_pose.shape == (B, 3) and robot_twist.shape == (B, 2)
        assert count.shape == (B,) and waypoints.shape == (B, Np, K, 2) and n_waypoints.shape == (B, Np)
        cb = self.crowd_c(cp, B, Np, K, dt, 0)
        cb.robot_pose, cb.robot_twist, cb.count = robot_pose.ctypes.data, robot_twist.ctypes.data, count.ctypes.data
        cb.waypoints, cb.n_waypoints = waypoints.ctypes.data, n_waypoints.ctypes.data
        if desired_speeds is not None:
            desired_speeds = np.ascontiguousarray(desired_speeds, np.float64)
            assert desired_speeds.shape == (B, Np)
            cb.desired_speeds = desired_speeds.ctypes.data
        if od_indexes is not None:
            od_indexes = np.ascontiguousarray(od_indexes, np.uint32)
            shared = od_indexes.ndim == 2
            od_origin = np.ascontiguousarray(od_origin, np.float64).reshape(-1, 2)
            assert od_indexes.ndim == 2 or od_indexes.shape[0] == B
            assert od_origin.shape == ((1, 2) if shared else (B, 2))
            cb.od_indexes, cb.od_origin = od_indexes.ctypes.data, od_origin.ctypes.data
            cb.od_shared, cb.od_height, cb.od_width = 1 if shared else 0, int(od_indexes.shape[-2]), int(od_indexes.shape[-1])
            cb.od_resolution = float(od_resolution)
        if groups is not None:
            groups = np.ascontiguousarray(groups, np.int32)
            assert groups.shape == (B, Np)
            gb = self.crowd_groups_c(group_params if group_params is not None else CrowdGroupParams(), groups.ctypes.data)
            _check(self.lib, self.lib.smpc_crowd_step_groups_batch(self._h, C.byref(cb), C.byref(gb), people.ctypes.data,
                                                                   cursor.ctypes.data), "smpc_crowd_step_groups_batch")
            return people, cursor
        _check(self.lib, self.lib.smpc_crowd_step_batch(self._h, C.byref(cb), people.ctypes.data, cursor.ctypes.data),
               "smpc_crowd_step_batch")
        return people, cursor

    def crowd_step_device(self, cb: SmpcCrowdBatch, people_ptr: int, cursor_ptr: int, groups: SmpcCrowdGroups = None):
        """Device pointers in cb (on_device == 1), in groups (crowd_groups_c; None: the plain step) and for people and
        cursor; asynchronous on the handle's stream."""
        assert cb.on_device == 1
        if groups is not None:
            _check(self.lib, self.lib.smpc_crowd_step_groups_batch(self._h, C.byref(cb), C.byref(groups), C.c_void_p(people_ptr),
                                                                   C.c_void_p(cursor_ptr)), "smpc_crowd_step_groups_batch")
            return
        _check(self.lib, self.lib.smpc_crowd_step_batch(self._h, C.byref(cb), C.c_void_p(people_ptr), C.c_void_p(cursor_ptr)),
               "smpc_crowd_step_batch")

    def select_command_device(self, B, T, rows, traj_n_ptr, traj_cmds_ptr, status_ptr, cmds_ptr, cmd_vel_ptr, source_ptr,
                              window_error_ptr=0):
        _check(self.lib, self.lib.smpc_select_command_batch(self._h, B, T, rows, 1, C.c_void_p(traj_n_ptr), C.c_void_p(traj_cmds_ptr),
                                                            C.c_void_p(status_ptr), C.c_void_p(cmds_ptr), C.c_void_p(cmd_vel_ptr),
                                                            C.c_void_p(source_ptr), C.c_void_p(window_error_ptr)),
               "smpc_select_command_batch")

    # -- warm start / input formatting: format_to_optimize + TrajectoryMemory for B scenes -----
    def format_to_optimize(self, path: np.ndarray, cmds: np.ndarray, speed: np.ndarray, memory: dict,
                           current_path_w: float = None, current_cmds_w: float = None, n_poses=None, max_poses: int = 0,
                           T: int = None):
        """path [B,rows,3] (x, y, yaw), cmds [B,rows,2], speed [B,2]; memory = new_memory(B, T) (updated in place when a
        record is empty). T: horizon (stride) of the outputs, default rows - 1. n_poses [B] + max_poses: horizons per
        scene (smpc_format_batch.n_poses; the memory then needs its `length` array: new_memory(..., lengths=True)).
        Returns dict(robot_status [B,T+1,6], pose0, init_params, path_pts, goal_yaw, T_scene)."""
        path = np.ascontiguousarray(path, np.float64)
        cmds = np.ascontiguousarray(cmds, np.float64)
        speed = np.ascontiguousarray(speed, np.float64)
        B, rows, _ = path.shape
        T = rows - 1 if T is None else int(T)
        Tp = T + 1
        assert cmds.shape == (B, rows, 2) and speed.shape == (B, 2) and rows >= Tp
        assert memory["prev_path"].shape == (B, Tp, 3) and memory["prev_cmds"].shape == (B, Tp, 2)
        CH, bl, nb, P, M, _ = self.params.dims(T, True)
        fb = SmpcFormatBatch()
        fb.B, fb.T, fb.path_rows, fb.on_device = B, T, rows, 0
        if n_poses is not None:
            n_poses = np.ascontiguousarray(n_poses, np.int32)
            assert n_poses.shape == (B,) and "length" in memory
            fb.n_poses, fb.max_poses = n_poses.ctypes.data, int(max_poses)
        if "length" in memory:
            fb.memory.length = memory["length"].ctypes.data
        fb.time_step = float(self.params.dt)
        fb.current_path_w = float(self.params.current_path_weight if current_path_w is None else current_path_w)
        fb.current_cmds_w = float(self.params.current_cmds_weight if current_cmds_w is None else current_cmds_w)
        fb.path, fb.cmds, fb.speed = path.ctypes.data, cmds.ctypes.data, speed.ctypes.data
        fb.memory.prev_path = memory["prev_path"].ctypes.data
        fb.memory.prev_cmds = memory["prev_cmds"].ctypes.data
        fb.memory.valid = memory["valid"].ctypes.data
        out = {"robot_status": np.zeros((B, Tp, 6)), "pose0": np.zeros((B, 3)), "init_params": np.zeros((B, P)),
               "path_pts": np.zeros((B, Tp, 2)), "goal_yaw": np.zeros(B), "T_scene": np.zeros(B, np.int32)}
        fo = SmpcFormatOut()
        for k, v in out.items():
            setattr(fo, k, v.ctypes.data)
        _check(self.lib, self.lib.smpc_format_to_optimize_batch(self._h, C.byref(fb), C.byref(fo)),
               "smpc_format_to_optimize_batch")
        return out

    @staticmethod
    def new_memory(B: int, T: int, lengths: bool = False):
        """An empty TrajectoryMemory record per scene (host arrays). lengths: with the per-record sizes that scenes with
        horizons of their own need (smpc_memory_batch.length)."""
        m = {"prev_path": np.zeros((B, T + 1, 3)), "prev_cmds": np.zeros((B, T + 1, 2)), "valid": np.zeros(B, np.int32)}
        if lengths:
            m["length"] = np.zeros((B, 2), np.int32)
        return m

    def memory_store(self, status: np.ndarray, path: np.ndarray, cmds: np.ndarray, memory: dict, T_scene=None):
        """The store at the end of Optimizer::optimize: usable solves (status != FAILURE) overwrite their record (the
        first T_scene[b] + 1 rows when the scenes have horizons of their own)."""
        status = np.ascontiguousarray(status, np.int32)
        path = np.ascontiguousarray(path, np.float64)
        cmds = np.ascontiguousarray(cmds, np.float64)
        B, Tp, _ = path.shape
        mb = SmpcMemoryBatch()
        mb.prev_path, mb.prev_cmds, mb.valid = (memory["prev_path"].ctypes.data, memory["prev_cmds"].ctypes.data,
                                                memory["valid"].ctypes.data)
        if "length" in memory:
            mb.length = memory["length"].ctypes.data
        ts = None if T_scene is None else np.ascontiguousarray(T_scene, np.int32)
        _check(self.lib, self.lib.smpc_memory_store_batch(self._h, B, Tp - 1, 0, status.ctypes.data, path.ctypes.data,
                                                          cmds.ctypes.data, C.byref(mb), None if ts is None else ts.ctypes.data),
               "smpc_memory_store_batch")

    def format_device(self, fb: SmpcFormatBatch, fo: SmpcFormatOut):
        assert fb.on_device == 1
        _check(self.lib, self.lib.smpc_format_to_optimize_batch(self._h, C.byref(fb), C.byref(fo)),
               "smpc_format_to_optimize_batch")

    def memory_store_device(self, B: int, T: int, status_ptr: int, path_ptr: int, cmds_ptr: int, mb: SmpcMemoryBatch,
                            T_scene_ptr: int = 0):
        _check(self.lib, self.lib.smpc_memory_store_batch(self._h, B, T, 1, C.c_void_p(status_ptr), C.c_void_p(path_ptr),
                                                          C.c_void_p(cmds_ptr), C.byref(mb), C.c_void_p(T_scene_ptr)),
               "smpc_memory_store_batch")

    def people_to_status_device(self, pb: SmpcPeopleBatch, out_ptr: int, has_people_ptr: int):
        assert pb.on_device == 1
        _check(self.lib, self.lib.smpc_people_to_status_batch(self._h, C.byref(pb), C.c_void_p(out_ptr), C.c_void_p(has_people_ptr)),
               "smpc_people_to_status_batch")

    def project_people_device(self, pb: SmpcProjectionBatch, out_ptr: int, err_ptr: int):
        assert pb.on_device == 1
        _check(self.lib, self.lib.smpc_project_people_batch(self._h, C.byref(pb), C.c_void_p(out_ptr), C.c_void_p(err_ptr)),
               "smpc_project_people_batch")

    # -- device-resident path (inputs already in HBM; asynchronous on the handle's stream) -------
    def alloc_results(self, B: int, T: int, device="cuda:0"):
        import torch

        CH, bl, nb, P, M, _ = self.params.dims(T, True)
        t = {
            "params": torch.empty((B, P), dtype=torch.float64, device=device),
            "cmds": torch.empty((B, T + 1, 2), dtype=torch.float64, device=device),
            "path": torch.empty((B, T + 1, 3), dtype=torch.float64, device=device),
            "status": torch.empty(B, dtype=torch.int32, device=device),
            "reason": torch.empty(B, dtype=torch.int32, device=device),
            "iterations": torch.empty(B, dtype=torch.int32, device=device),
            "evaluations": torch.empty(B, dtype=torch.int32, device=device),
            "initial_cost": torch.empty(B, dtype=torch.float64, device=device),
            "final_cost": torch.empty(B, dtype=torch.float64, device=device),
        }
        rb = SmpcResultBatch()
        for k, v in t.items():
            setattr(rb, k, v.data_ptr())
        return rb, t

    def stage_people(self, scenes: SceneBatch):
        """smpc_stage_people_batch on host arrays: (records [B,N,T,4], aux [B,T,2])."""
        B, T, N = scenes.B, scenes.T, scenes.N
        rec = np.zeros((B, N, T, 4))
        aux = np.zeros((B, T, 2))
        sb = scenes.to_c()
        _check(self.lib, self.lib.smpc_stage_people_batch(self._h, C.byref(sb), rec.ctypes.data, aux.ctypes.data),
               "smpc_stage_people_batch")
        return rec, aux

    def stage_people_device(self, sb: SmpcSceneBatch, device="cuda:0"):
        """Stage the device-resident people block of `sb` once and attach the result to it: later solve_device /
        eval_device calls with this batch read the staged records instead of running the staging pass again.
        Returns the tensors that own the memory (keep them alive as long as `sb` is used)."""
        import torch

        assert sb.on_device == 1
        rec = torch.zeros((sb.B, sb.N, sb.T, 4), dtype=torch.float64, device=device)
        aux = torch.zeros((sb.B, sb.T, 2), dtype=torch.float64, device=device)
        _check(self.lib, self.lib.smpc_stage_people_batch(self._h, C.byref(sb), C.c_void_p(rec.data_ptr()),
                                                          C.c_void_p(aux.data_ptr())), "smpc_stage_people_batch")
        sb.people_records, sb.people_aux = rec.data_ptr(), aux.data_ptr()
        return rec, aux

    def solve_device(self, sb: SmpcSceneBatch, rb: SmpcResultBatch):
        assert sb.on_device == 1
        _check(self.lib, self.lib.smpc_solve_batch(self._h, C.byref(sb), C.byref(rb)), "smpc_solve_batch")

    def alloc_trace(self, B: int, max_rows: int = None, device="cuda:0"):
        """(SmpcTraceOut, tensors) for solve_trace_device: "trace" [B, max_rows, 9] filled with NaN, "trace_rows" [B]."""
        import torch

        max_rows = self.params.max_iterations + 1 if max_rows is None else int(max_rows)
        t = {"trace": torch.full((B, max_rows, _abi.SMPC_TRACE_COLS), float("nan"), dtype=torch.float64, device=device),
             "trace_rows": torch.zeros(B, dtype=torch.int32, device=device)}
        return SmpcTraceOut(t["trace"].data_ptr() if t["trace"].numel() else None, max_rows, t["trace_rows"].data_ptr()), t

    def solve_trace_device(self, sb: SmpcSceneBatch, rb: SmpcResultBatch, to: SmpcTraceOut):
        """solve_device that also records the per-iteration rows (alloc_trace); asynchronous on the handle's stream."""
        assert sb.on_device == 1
        _check(self.lib, self.lib.smpc_solve_trace_batch(self._h, C.byref(sb), C.byref(rb), C.byref(to)), "smpc_solve_trace_batch")

    def alloc_eval(self, B: int, T: int, device="cuda:0", row_order: int = 0):
        import torch

        CH, bl, nb, P, M, _ = self.params.dims(T, True)
        t = {
            "residuals": torch.empty((B, M), dtype=torch.float64, device=device),
            "jacobian": torch.empty((B, M, P), dtype=torch.float64, device=device),
            "cost": torch.empty(B, dtype=torch.float64, device=device),
            "gradient": torch.empty((B, P), dtype=torch.float64, device=device),
        }
        eo = SmpcEvalOut()
        for k, v in t.items():
            setattr(eo, k, v.data_ptr())
        eo.row_order = int(row_order)
        return eo, t

    def eval_device(self, sb: SmpcSceneBatch, x_ptr: int, eo: SmpcEvalOut):
        assert sb.on_device == 1
        _check(self.lib, self.lib.smpc_eval_batch(self._h, C.byref(sb), C.c_void_p(x_ptr), C.byref(eo)), "smpc_eval_batch")
