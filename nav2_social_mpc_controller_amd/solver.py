"""Python host side above the C ABI (include/smpc.h): loads csrc/libsmpc_hip.so and mirrors the part of the
reference's `Optimizer` interface that sits on the hot path (optimizer.hpp:152,167-170):

    Optimizer.initialize(OptimizerParams)   -> BatchSolver(params)
    Optimizer.optimize(...) for B scenes     -> BatchSolver.solve(scenes) / solve_device(...)

There is NO CPU fallback: a missing library or a missing HIP device raises.
"""
import ctypes as C
import os

import numpy as np

from . import (_abi, _abi_collision_monitor, _abi_crowd_pool, _abi_detector, _abi_global_plan, _abi_local_costmap, _abi_nearest, _abi_obstacle_memory, _abi_plan_repair,
               _abi_plan_smoother, _abi_plant, _abi_scan_people, _abi_sensed_costmap, _abi_tracker, _abi_visibility)
from ._abi import (SmpcCrowdBatch, SmpcCrowdGroups, SmpcEvalOut, SmpcFormatBatch, SmpcFormatOut, SmpcMemoryBatch, SmpcMetricsBatch, SmpcObstacleDistanceIn,
                   SmpcObstacleDistanceOut, SmpcPeopleBatch, SmpcPlanWindowBatch, SmpcProjectionBatch, SmpcResultBatch, SmpcSceneBatch, SmpcTraceOut,
                   SmpcTrajectorizeBatch, SmpcTrajectorizeOut)
from ._abi_detector import SmpcDetectorIn
from ._abi_collision_monitor import SmpcCollisionMonitorIn, SmpcMonitorZone
from ._abi_crowd_pool import SmpcCrowdPoolIn
from ._abi_global_plan import SmpcExtractPlanIn, SmpcGoalFieldIn
from ._abi_local_costmap import SmpcLocalCostmapIn
from ._abi_nearest import SmpcNearestIn
from ._abi_obstacle_memory import SmpcObstacleMemoryIn
from ._abi_plan_repair import SmpcPlanRepairIn
from ._abi_plan_smoother import SmpcPlanSmootherIn
from ._abi_plant import SmpcPlantIn
from ._abi_scan_people import SmpcScanPeopleIn
from ._abi_sensed_costmap import SmpcSensedCostmapIn
from ._abi_tracker import SmpcTrackerIn
from ._abi_visibility import SmpcVisibilityIn
from .params import (CrowdGroupParams, CrowdParams, DetectorParams, GlobalPlanParams, MetricsParams, MonitorParams, OptimizerParams, PlanRepairParams, PlanSmootherParams, PlantParams,
                     PoolCrowdParams,
                     ScanDetectorParams, TrackerParams, TrajectorizerParams, VisibilityParams)
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
    for name, (restype, argtypes) in {**_abi.FUNCTIONS, **_abi.FIXED_SHAPE_FUNCTIONS, **_abi_local_costmap.FUNCTIONS,
                                       **_abi_global_plan.FUNCTIONS, **_abi_visibility.FUNCTIONS, **_abi_nearest.FUNCTIONS,
                                       **_abi_crowd_pool.FUNCTIONS, **_abi_sensed_costmap.FUNCTIONS,
                                       **_abi_obstacle_memory.FUNCTIONS, **_abi_tracker.FUNCTIONS,
                                       **_abi_detector.FUNCTIONS, **_abi_plant.FUNCTIONS,
                                       **_abi_collision_monitor.FUNCTIONS, **_abi_scan_people.FUNCTIONS,
                                       **_abi_plan_repair.FUNCTIONS, **_abi_plan_smoother.FUNCTIONS}.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.smpc_abi_version() != _abi.SMPC_ABI_VERSION:
        raise SmpcError("libsmpc_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _ptr(a):
    """Address of a numpy array or a torch tensor; None (a NULL field) and plain addresses pass through."""
    if a is None or isinstance(a, int):
        return a or None
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def point(struct, arrays: dict):
    """Point the fields of `struct` named by the keys of `arrays` at its numpy arrays or torch tensors."""
    for k, v in arrays.items():
        setattr(struct, k, _ptr(v))
    return struct


def _alloc(spec: dict, device=None) -> dict:
    """The buffers `spec` declares, name -> (shape, dtype name, fill): host arrays (fill None: zeros) without `device`,
    else torch tensors on it (fill None: uninitialised)."""
    if device is None:
        return {k: np.full(shape, 0 if fill is None else fill, dtype) for k, (shape, dtype, fill) in spec.items()}
    import torch

    return {k: torch.empty(shape, dtype=getattr(torch, dtype), device=device) if fill is None else
            torch.full(shape, fill, dtype=getattr(torch, dtype), device=device) for k, (shape, dtype, fill) in spec.items()}


_OD_DTYPE = {"od_indexes": np.uint32, "od_distances": np.float32}


def set_od_grid(st, field: str, grid, origin, resolution: float, dims: tuple = None, B: int = None):
    """Fill the ObstacleDistance-grid fields of `st` (SmpcProjectionBatch, SmpcMetricsBatch, SmpcCrowdBatch): `field`
    ("od_indexes" or "od_distances"), od_origin, od_shared, od_height, od_width and od_resolution.
    dims = (shared, h, w): grid and origin are addresses or device tensors of a grid of that shape.
    dims = None: host arrays of a batch of B scenes, grid [h,w] + origin [2] one grid shared by all of them, grid [B,h,w] +
    origin [B,2] one per scene. Returns the arrays `st` then points into (they must outlive the call)."""
    if dims is None:
        grid = np.ascontiguousarray(grid, _OD_DTYPE[field])
        origin = np.ascontiguousarray(origin, np.float64).reshape(-1, 2)
        shared = grid.ndim == 2
        assert shared or grid.shape[0] == B
        assert origin.shape == ((1, 2) if shared else (B, 2))
        dims = (shared, grid.shape[-2], grid.shape[-1])
    setattr(st, field, _ptr(grid) if dims[1] * dims[2] else None)
    st.od_origin = _ptr(origin)
    st.od_shared, st.od_height, st.od_width, st.od_resolution = int(dims[0]), int(dims[1]), int(dims[2]), float(resolution)
    return grid, origin


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
    """One solver bound to one HIP device; mirrors Optimizer::initialize + Optimizer::optimize for B scenes.
    Every entry point has a host method (numpy arrays in and out: it converts, allocates and sets on_device = 0) and a
    `*_device` method (structs and addresses of device memory, asynchronous on the handle's stream); both end in the same
    `_call` of the library function."""

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

    def _call(self, name: str, *args) -> int:
        """lib.<name>(handle, *args), as _abi.FUNCTIONS declares it (a struct goes by reference, an int or None is an
        address); a negative result code raises with the library's message. Returns the result (0, or a count)."""
        rc = getattr(self.lib, name)(self._h, *args)
        if rc < 0:
            raise SmpcError(f"{name} failed ({rc}): {self.lib.smpc_last_error().decode()}")
        return rc

    def set_stream(self, stream_ptr: int):
        self._call("smpc_set_stream", stream_ptr)

    def set_solve_share(self, n: int):
        """smpc_set_solve_share: this handle's solve launches leave room for n - 1 concurrent ones (other streams)."""
        self._call("smpc_set_solve_share", int(n))

    def solve_slot_width(self, B: int, T: int, N: int) -> int:
        """smpc_solve_slot_width: 32 (two scenes per wave) or 64 (one) for a solve launch of this shape."""
        return self._call("smpc_solve_slot_width", int(B), int(T), int(N))

    def set_fixed_shapes(self, enable: bool):
        """smpc_set_fixed_shapes: whether launches of a listed shape run that shape's compile-time-shape kernels (default
        on; the results are the same bit for bit either way)."""
        self._call("smpc_set_fixed_shapes", 1 if enable else 0)

    def solve_shape_is_fixed(self, B: int, T: int, N: int) -> bool:
        """smpc_solve_shape_is_fixed: does a plain solve launch of this shape run a fixed-shape kernel?"""
        return self._call("smpc_solve_shape_is_fixed", int(B), int(T), int(N)) == 1

    def eval_shape_is_fixed(self, T: int, N: int) -> bool:
        """smpc_eval_shape_is_fixed: does a plain K1 launch (evaluate / eval_device) of this shape run a fixed-shape kernel?"""
        return self._call("smpc_eval_shape_is_fixed", int(T), int(N)) == 1

    def math_probe(self, fn: int, a: np.ndarray, b: np.ndarray = None):
        """smpc_math_probe: the sweep's elementary functions evaluated on the device (see include/smpc.h)."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        n = a.size // 8 if fn == 7 else a.size
        bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        o0 = np.empty(n)
        o1 = np.empty(n)
        self._call("smpc_math_probe", int(fn), n, _ptr(a), _ptr(bb), _ptr(o0), _ptr(o1))
        return o0, o1

    def fp64_peak_tflops(self, iters: int = 20000) -> float:
        """Measured FP64 vector peak of this device (smpc_fp64_peak_probe)."""
        return float(self.lib.smpc_fp64_peak_probe(self._h, int(iters)))

    def last_kernel_ms(self) -> float:
        return float(self.lib.smpc_last_kernel_ms(self._h))

    # -- what the entry points write, declared once: name -> (shape, dtype, fill) for _alloc -------------------------
    def _result_spec(self, B: int, T: int) -> dict:
        """The arrays of SmpcResultBatch."""
        P = self.params.dims(T, True)[3]
        return {"params": ((B, P), "float64", None), "cmds": ((B, T + 1, 2), "float64", None),
                "path": ((B, T + 1, 3), "float64", None), "status": ((B,), "int32", None), "reason": ((B,), "int32", None),
                "iterations": ((B,), "int32", None), "evaluations": ((B,), "int32", None),
                "initial_cost": ((B,), "float64", None), "final_cost": ((B,), "float64", None)}

    def _eval_spec(self, B: int, T: int) -> dict:
        """The arrays of SmpcEvalOut."""
        CH, bl, nb, P, M, _ = self.params.dims(T, True)
        return {"residuals": ((B, M), "float64", None), "jacobian": ((B, M, P), "float64", None),
                "cost": ((B,), "float64", None), "gradient": ((B, P), "float64", None)}

    def _trace_out(self, B: int, max_rows, device=None):
        """(SmpcTraceOut, its buffers): "trace" [B, max_rows, 9] filled with NaN, "trace_rows" [B]; max_rows defaults to
        max_iterations + 1, which holds every row."""
        max_rows = self.params.max_iterations + 1 if max_rows is None else int(max_rows)
        if max_rows < 0:
            raise SmpcError(f"max_rows must be >= 0, got {max_rows}")
        t = _alloc({"trace": ((B, max_rows, _abi.SMPC_TRACE_COLS), "float64", float("nan")),
                    "trace_rows": ((B,), "int32", 0)}, device)
        return SmpcTraceOut(_ptr(t["trace"]) if B * max_rows else None, max_rows, _ptr(t["trace_rows"])), t

    # -- host-memory path (stages through HBM inside the library) ---------------------------------
    def _solve_call(self, scenes: SceneBatch, order):
        """What solve() and solve_trace() hand to the library: (result dict of host arrays, SmpcSceneBatch, SmpcResultBatch,
        the arrays the structs point into)."""
        scenes.validate(self.params.dims(scenes.T, True)[3])
        out = _alloc(self._result_spec(scenes.B, scenes.T))
        rb = point(SmpcResultBatch(), out)
        sb = scenes.to_c()
        if order is not None:
            order = np.ascontiguousarray(order, np.int32)
            assert order.shape == (scenes.B,)
            sb.order = order.ctypes.data
        return out, sb, rb, order

    def solve(self, scenes: SceneBatch, order: np.ndarray = None):
        """Solve B scenes (host arrays in, host arrays out). order: optional queue order of the persistent kernel, a
        permutation of 0..B-1 (smpc_scene_batch.order: longest scenes first shortens a lone launch; results do not
        depend on it)."""
        out, sb, rb, _keep = self._solve_call(scenes, order)
        self._call("smpc_solve_batch", sb, rb)
        return out

    def solve_device(self, sb: SmpcSceneBatch, rb: SmpcResultBatch):
        assert sb.on_device == 1
        self._call("smpc_solve_batch", sb, rb)

    def alloc_results(self, B: int, T: int, device="cuda:0"):
        t = _alloc(self._result_spec(B, T), device)
        return point(SmpcResultBatch(), t), t

    def solve_trace(self, scenes: SceneBatch, order: np.ndarray = None, max_rows: int = None):
        """solve() that also returns the per-iteration record of every scene (optimizer.debug_optimizer; smpc_solve_trace_batch):
        "trace" [B, max_rows, 9], columns TRACE_COLS, row i = LM iteration i, NaN where a scene has no row; "trace_rows" [B],
        the rows each solve produced (more than max_rows: the rest were dropped). max_rows defaults to max_iterations + 1,
        which holds every row. The other entries are those of solve(), bit for bit."""
        to, trace = self._trace_out(scenes.B, max_rows)
        out, sb, rb, _keep = self._solve_call(scenes, order)
        out.update(trace)
        self._call("smpc_solve_trace_batch", sb, rb, to)
        return out

    def alloc_trace(self, B: int, max_rows: int = None, device="cuda:0"):
        """(SmpcTraceOut, tensors) for solve_trace_device: "trace" [B, max_rows, 9] filled with NaN, "trace_rows" [B]."""
        return self._trace_out(B, max_rows, device)

    def solve_trace_device(self, sb: SmpcSceneBatch, rb: SmpcResultBatch, to: SmpcTraceOut):
        """solve_device that also records the per-iteration rows (alloc_trace); asynchronous on the handle's stream."""
        assert sb.on_device == 1
        self._call("smpc_solve_trace_batch", sb, rb, to)

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
        P = self.params.dims(scenes.T, True)[3]
        scenes.validate(P)
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (scenes.B, P)
        out = _alloc(self._eval_spec(scenes.B, scenes.T))
        eo = point(SmpcEvalOut(row_order=int(row_order)), out)
        self._call("smpc_eval_batch", scenes.to_c(), _ptr(x), eo)
        return out

    def alloc_eval(self, B: int, T: int, device="cuda:0", row_order: int = 0):
        t = _alloc(self._eval_spec(B, T), device)
        return point(SmpcEvalOut(row_order=int(row_order)), t), t

    def eval_device(self, sb: SmpcSceneBatch, x_ptr: int, eo: SmpcEvalOut):
        assert sb.on_device == 1
        self._call("smpc_eval_batch", sb, x_ptr, eo)

    def stage_people(self, scenes: SceneBatch):
        """smpc_stage_people_batch on host arrays: (records [B,N,T,4], aux [B,T,2])."""
        B, T, N = scenes.B, scenes.T, scenes.N
        rec = np.zeros((B, N, T, 4))
        aux = np.zeros((B, T, 2))
        self._call("smpc_stage_people_batch", scenes.to_c(), _ptr(rec), _ptr(aux))
        return rec, aux

    def stage_people_device(self, sb: SmpcSceneBatch, device="cuda:0"):
        """Stage the device-resident people block of `sb` once and attach the result to it: later solve_device /
        eval_device calls with this batch read the staged records instead of running the staging pass again.
        Returns the tensors that own the memory (keep them alive as long as `sb` is used)."""
        import torch

        assert sb.on_device == 1
        rec = torch.zeros((sb.B, sb.N, sb.T, 4), dtype=torch.float64, device=device)
        aux = torch.zeros((sb.B, sb.T, 2), dtype=torch.float64, device=device)
        self._call("smpc_stage_people_batch", sb, rec.data_ptr(), aux.data_ptr())
        sb.people_records, sb.people_aux = rec.data_ptr(), aux.data_ptr()
        return rec, aux

    # -- people projection: Optimizer::project_people for B scenes -------------
    def project_people(self, init_people: np.ndarray, robot_path: np.ndarray, od_indexes: np.ndarray,
                       od_origin: np.ndarray, od_resolution: float, max_time: float, time_step: float):
        """init_people [B,N,6], robot_path [B,T+1,6], od_indexes [B or 1,h,w] uint32, od_origin [B or 1,2].
        Returns (people_proj [B,T+1,6,N], error [B])."""
        init_people = np.ascontiguousarray(init_people, np.float64)
        robot_path = np.ascontiguousarray(robot_path, np.float64)
        B, N, _ = init_people.shape
        T = robot_path.shape[1] - 1
        pb = SmpcProjectionBatch(B=B, T=T, N=N, on_device=0, max_time=float(max_time), time_step=float(time_step))
        pb.init_people, pb.robot_path = init_people.ctypes.data, robot_path.ctypes.data
        od_indexes = np.asarray(od_indexes)
        if od_indexes.ndim == 3 and od_indexes.shape[0] == 1:  # [1,h,w]: the one grid of all scenes
            od_indexes = od_indexes[0]
        _keep = set_od_grid(pb, "od_indexes", od_indexes, od_origin, od_resolution, B=B)
        out = np.zeros((B, T + 1, 6, N))
        err = np.zeros(B, np.int32)
        self._call("smpc_project_people_batch", pb, _ptr(out), _ptr(err))
        return out, err

    def project_people_device(self, pb: SmpcProjectionBatch, out_ptr: int, err_ptr: int):
        assert pb.on_device == 1
        self._call("smpc_project_people_batch", pb, out_ptr, err_ptr)

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
        self._call("smpc_obstacle_distance_batch", ob, point(SmpcObstacleDistanceOut(), out))
        if shared:
            out["indexes"] = out["indexes"][0]
            out["distances"] = None if out["distances"] is None else out["distances"][0]
        return out

    def obstacle_distance_device(self, ob: SmpcObstacleDistanceIn, indexes_ptr: int, distances_ptr: int = 0,
                                 n_obstacles_ptr: int = 0):
        """Device pointers in and out (ob.on_device == 1), asynchronous on the handle's stream."""
        assert ob.on_device == 1
        oo = SmpcObstacleDistanceOut(indexes_ptr or None, distances_ptr or None, n_obstacles_ptr or None)
        self._call("smpc_obstacle_distance_batch", ob, oo)

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
        tb = point(self.trajectorize_c(tp, B, L, 0), {"plan": plan, "plan_len": plan_len, "robot_pose": robot_pose})
        S1 = tp.max_steps + 1
        out = {"path": np.zeros((B, S1, 3)), "cmds": np.zeros((B, S1, 2)), "cmds_vy": np.zeros((B, S1)),
               "n_poses": np.zeros(B, np.int32), "error": np.zeros(B, np.int32)}
        self._call("smpc_trajectorize_path_batch", tb, point(SmpcTrajectorizeOut(), out))
        return out

    def trajectorize_device(self, tb: SmpcTrajectorizeBatch, to: SmpcTrajectorizeOut):
        assert tb.on_device == 1
        self._call("smpc_trajectorize_path_batch", tb, to)

    def transform_global_plan(self, plan: np.ndarray, plan_len: np.ndarray, plan_start: np.ndarray, robot_pose: np.ndarray,
                              max_robot_pose_search_dist: float, dist_threshold: float, to_local: np.ndarray = None):
        """PathHandler::transformGlobalPlan for B robots (smpc_transform_global_plan_batch): plan [B,L,2], plan_len [B],
        plan_start [B] (updated in place: the pruning), robot_pose [B,3] in the plan frame, to_local [B,3] or None.
        Returns dict(window [B,L,2], window_len [B], error [B])."""
        plan = np.ascontiguousarray(plan, np.float64)
        plan_len = np.ascontiguousarray(plan_len, np.int32)
        assert plan_start.dtype == np.int32 and plan_start.flags.c_contiguous
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        to_local = None if to_local is None else np.ascontiguousarray(to_local, np.float64)
        B, L, _ = plan.shape
        wb = SmpcPlanWindowBatch(B=B, L=L, on_device=0, max_robot_pose_search_dist=float(max_robot_pose_search_dist),
                                 dist_threshold=float(dist_threshold))
        point(wb, {"plan": plan, "plan_len": plan_len, "plan_start": plan_start, "robot_pose": robot_pose, "to_local": to_local})
        out = {"window": np.zeros((B, L, 2)), "window_len": np.zeros(B, np.int32), "error": np.zeros(B, np.int32)}
        self._call("smpc_transform_global_plan_batch", wb, _ptr(out["window"]), _ptr(out["window_len"]), _ptr(out["error"]))
        return out

    def transform_global_plan_device(self, wb: "SmpcPlanWindowBatch", window_ptr: int, window_len_ptr: int, error_ptr: int = 0):
        assert wb.on_device == 1
        self._call("smpc_transform_global_plan_batch", wb, window_ptr, window_len_ptr, error_ptr)

    def people_to_status(self, people: np.ndarray, count: np.ndarray, N: int = 3, robot_pose: np.ndarray = None,
                         fov_angle: float = np.pi / 4, costmap_origin: np.ndarray = None, size_x: int = 0, size_y: int = 0,
                         resolution: float = 0.0):
        """Optimizer::people_to_status for B scenes: people [B,Np,5] (px, py, vx, vy, vz), count [B] ->
        (init_people [B,N,6], has_people [B] uint8). With robot_pose [B,3] the field-of-view filter of
        computeVelocityCommands runs first (costmap_origin [B or 1,2], size_x/size_y cells, resolution)."""
        people = np.ascontiguousarray(people, np.float64)
        count = np.ascontiguousarray(count, np.int32)
        B, Np, _ = people.shape
        pb = SmpcPeopleBatch(B=B, Np=Np, N=N, on_device=0, people=people.ctypes.data, count=count.ctypes.data)
        if robot_pose is not None:
            robot_pose = np.ascontiguousarray(robot_pose, np.float64)
            costmap_origin = np.ascontiguousarray(costmap_origin, np.float64).reshape(-1, 2)
            pb.robot_pose, pb.fov_angle = robot_pose.ctypes.data, float(fov_angle)
            pb.costmap_origin, pb.costmap_shared = costmap_origin.ctypes.data, 1 if costmap_origin.shape[0] == 1 else 0
            pb.size_x, pb.size_y, pb.resolution = int(size_x), int(size_y), float(resolution)
        out, has = np.zeros((B, N, 6)), np.zeros(B, np.uint8)
        self._call("smpc_people_to_status_batch", pb, _ptr(out), _ptr(has))
        return out, has

    def people_to_status_device(self, pb: SmpcPeopleBatch, out_ptr: int, has_people_ptr: int):
        assert pb.on_device == 1
        self._call("smpc_people_to_status_batch", pb, out_ptr, has_people_ptr)

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
        self._call("smpc_select_command_batch", B, T, rows, 0, _ptr(n), _ptr(traj_cmds), _ptr(status), _ptr(cmds), _ptr(out),
                   _ptr(src), _ptr(we))
        return out, src

    def select_command_device(self, B, T, rows, traj_n_ptr, traj_cmds_ptr, status_ptr, cmds_ptr, cmd_vel_ptr, source_ptr,
                              window_error_ptr=0):
        self._call("smpc_select_command_batch", B, T, rows, 1, traj_n_ptr, traj_cmds_ptr, status_ptr, cmds_ptr, cmd_vel_ptr,
                   source_ptr, window_error_ptr)

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
        people = np.ascontiguousarray(people, np.float64)
        B, Np, _ = people.shape
        f64, i32 = np.float64, np.int32
        ins = {name: None if a is None else np.ascontiguousarray(a, dtype) for name, a, dtype in (
            ("robot_pose", robot_pose, f64), ("robot_twist", robot_twist, f64), ("people", people, f64), ("count", count, i32),
            ("goal", goal, f64), ("status", status, i32), ("source", source, i32))}
        assert acc.shape == (B, _abi.SMPC_METRIC_COLS) and ins["robot_pose"].shape == (B, 3) and ins["robot_twist"].shape == (B, 2)
        assert ins["count"].shape == (B,) and people.shape[2] == 5
        assert goal is None or ins["goal"].shape == (B, 2)
        assert all(ins[k] is None or ins[k].shape == (B,) for k in ("status", "source"))
        mb = point(self.metrics_c(mp, B, Np, dt, 0), ins)
        if od_distances is not None:
            _keep = set_od_grid(mb, "od_distances", od_distances, od_origin, od_resolution, B=B)
        self._call("smpc_episode_metrics_batch", mb, _ptr(acc))
        return acc

    def episode_metrics_device(self, mb: SmpcMetricsBatch, acc_ptr: int):
        """Device pointers in mb (on_device == 1) and for acc; asynchronous on the handle's stream."""
        assert mb.on_device == 1
        self._call("smpc_episode_metrics_batch", mb, acc_ptr)

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
        return SmpcCrowdGroups(group_id_ptr, gp.factor_gaze, gp.factor_coherence, gp.factor_repulsion)

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
        f64, i32 = np.float64, np.int32
        ins = {name: None if a is None else np.ascontiguousarray(a, dtype) for name, a, dtype in (
            ("robot_pose", robot_pose, f64), ("robot_twist", robot_twist, f64), ("count", count, i32),
            ("waypoints", waypoints, f64), ("n_waypoints", n_waypoints, i32), ("desired_speeds", desired_speeds, f64))}
        B, Np, _ = people.shape
        K = ins["waypoints"].shape[2]
        assert people.shape[2] == 5 and cursor.shape == (B, Np) and ins["robot_pose"].shape == (B, 3) and ins["robot_twist"].shape == (B, 2)
        assert ins["count"].shape == (B,) and ins["waypoints"].shape == (B, Np, K, 2) and ins["n_waypoints"].shape == (B, Np)
        assert desired_speeds is None or ins["desired_speeds"].shape == (B, Np)
        cb = point(self.crowd_c(cp, B, Np, K, dt, 0), ins)
        if od_indexes is not None:
            _keep = set_od_grid(cb, "od_indexes", od_indexes, od_origin, od_resolution, B=B)
        gb = None
        if groups is not None:
            groups = np.ascontiguousarray(groups, np.int32)
            assert groups.shape == (B, Np)
            gb = self.crowd_groups_c(group_params if group_params is not None else CrowdGroupParams(), groups.ctypes.data)
        self._crowd_call(cb, _ptr(people), _ptr(cursor), gb)
        return people, cursor

    def _crowd_call(self, cb, people_ptr, cursor_ptr, groups):
        if groups is not None:
            self._call("smpc_crowd_step_groups_batch", cb, groups, people_ptr, cursor_ptr)
        else:
            self._call("smpc_crowd_step_batch", cb, people_ptr, cursor_ptr)

    def crowd_step_device(self, cb: SmpcCrowdBatch, people_ptr: int, cursor_ptr: int, groups: SmpcCrowdGroups = None):
        """Device pointers in cb (on_device == 1), in groups (crowd_groups_c; None: the plain step) and for people and
        cursor; asynchronous on the handle's stream."""
        assert cb.on_device == 1
        self._crowd_call(cb, people_ptr, cursor_ptr, groups)

    # -- rolling local costmaps of a closed-loop episode (smpc_local_costmap_batch, include/smpc_local_costmap.h) ------
    @staticmethod
    def local_costmap_c(B: int, size_x: int, size_y: int, world_x: int, world_y: int, world_shared: bool, resolution: float,
                        on_device: int, outside_cost: int = 255, force: bool = False) -> SmpcLocalCostmapIn:
        if not 0 <= int(outside_cost) <= 255:
            raise SmpcError(f"outside_cost must be 0..255, got {outside_cost}")
        lc = SmpcLocalCostmapIn()
        lc.B, lc.on_device, lc.size_x, lc.size_y = int(B), int(on_device), int(size_x), int(size_y)
        lc.world_x, lc.world_y, lc.world_shared = int(world_x), int(world_y), 1 if world_shared else 0
        lc.outside_cost, lc.force, lc.resolution = int(outside_cost), 1 if force else 0, float(resolution)
        return lc

    def local_costmap(self, world: np.ndarray, world_origin: np.ndarray, resolution: float, pose: np.ndarray, cell: np.ndarray,
                      costmap: np.ndarray, costmap_origin: np.ndarray, outside_cost: int = 255, force: bool = False,
                      moved: bool = True):
        """One roll of B robots' local costmaps (host arrays): world [Hy,Hx] uint8 with world_origin [2] (one map shared by
        all) or [B,Hy,Hx] with [B,2], pose [B,3], cell [B,2] int32 (the world cell of every window's cell (0,0)), costmap
        [B,size_y,size_x] uint8 and costmap_origin [B,2] as the last roll left them (a robot whose window does not move
        keeps them bit for bit). force: the stored cells are taken as (0,0) and every window is written. Returns the
        updated copies (cell, costmap, costmap_origin, moved [B] int32: 0 kept, 1 moved, 2 pose not finite; None with
        moved=False, which passes a NULL array)."""
        world = np.ascontiguousarray(world, np.uint8)
        shared = world.ndim == 2
        world_origin = np.ascontiguousarray(world_origin, np.float64).reshape(-1, 2)
        pose = np.ascontiguousarray(pose, np.float64)
        cell = np.array(cell, dtype=np.int32, order="C")
        costmap = np.array(costmap, dtype=np.uint8, order="C")
        costmap_origin = np.array(costmap_origin, dtype=np.float64, order="C")
        B, size_y, size_x = costmap.shape
        assert pose.shape == (B, 3) and cell.shape == (B, 2) and costmap_origin.shape == (B, 2)
        assert shared or world.shape[0] == B
        assert world_origin.shape == ((1, 2) if shared else (B, 2))
        lc = point(self.local_costmap_c(B, size_x, size_y, world.shape[-1], world.shape[-2], shared, resolution, 0, outside_cost, force),
                   {"world": world, "world_origin": world_origin, "pose": pose})
        mv = np.zeros(B, np.int32) if moved else None
        self._call("smpc_local_costmap_batch", lc, _ptr(cell), _ptr(costmap), _ptr(costmap_origin), _ptr(mv))
        return cell, costmap, costmap_origin, mv

    def local_costmap_device(self, lc: SmpcLocalCostmapIn, cell_ptr: int, costmap_ptr: int, origin_ptr: int, moved_ptr: int = 0):
        """Device pointers in lc (on_device == 1) and for cell, costmap, costmap_origin and moved (0: none); asynchronous on
        the handle's stream."""
        assert lc.on_device == 1
        self._call("smpc_local_costmap_batch", lc, cell_ptr, costmap_ptr, origin_ptr, moved_ptr or None)

    # -- global plans on a world map (smpc_goal_field_batch / smpc_extract_plan_batch, include/smpc_global_plan.h) ------
    @staticmethod
    def _plan_world_c(st, gp: GlobalPlanParams, world_x: int, world_y: int, world_shared: bool, resolution: float, on_device: int):
        """The members SmpcGoalFieldIn and SmpcExtractPlanIn share."""
        st.on_device, st.world_x, st.world_y, st.world_shared = int(on_device), int(world_x), int(world_y), 1 if world_shared else 0
        st.resolution = float(resolution)
        st.cost.neutral_cost, st.cost.cost_weight = int(gp.neutral_cost), int(gp.cost_weight)
        st.cost.lethal_min_cost, st.cost.allow_unknown = int(gp.lethal_min_cost), 1 if gp.allow_unknown else 0
        return st

    @staticmethod
    def goal_field_c(gp: GlobalPlanParams, G: int, world_x: int, world_y: int, world_shared: bool, resolution: float,
                     on_device: int) -> SmpcGoalFieldIn:
        return BatchSolver._plan_world_c(SmpcGoalFieldIn(G=int(G)), gp, world_x, world_y, world_shared, resolution, on_device)

    @staticmethod
    def extract_plan_c(gp: GlobalPlanParams, B: int, G: int, world_x: int, world_y: int, world_shared: bool, resolution: float,
                       on_device: int) -> SmpcExtractPlanIn:
        st = SmpcExtractPlanIn(B=int(B), G=int(G), L=int(gp.max_poses), stride=int(gp.stride))
        return BatchSolver._plan_world_c(st, gp, world_x, world_y, world_shared, resolution, on_device)

    @staticmethod
    def _plan_world_arrays(world, world_origin, G: int):
        world = np.ascontiguousarray(world, np.uint8)
        shared = world.ndim == 2
        world_origin = np.ascontiguousarray(world_origin, np.float64).reshape(-1, 2)
        assert shared or world.shape[0] == G
        assert world_origin.shape == ((1, 2) if shared else (G, 2))
        return world, world_origin, shared

    def goal_field(self, gp: GlobalPlanParams, world: np.ndarray, world_origin: np.ndarray, resolution: float, goal: np.ndarray):
        """The goal fields of G goal points (host arrays): world [Hy,Hx] uint8 with world_origin [2] (one map shared by all
        goals) or [G,Hy,Hx] with [G,2], goal [G,2]. Returns (field [G,Hy,Hx] uint32: the exact cost-to-go of every cell,
        0xFFFFFFFF where there is none; status [G] int32: 0 ok, 1 the goal has no cell, 2 its cell is impassable)."""
        goal = np.ascontiguousarray(goal, np.float64).reshape(-1, 2)
        G = goal.shape[0]
        world, world_origin, shared = self._plan_world_arrays(world, world_origin, G)
        gf = point(self.goal_field_c(gp, G, world.shape[-1], world.shape[-2], shared, resolution, 0),
                   {"world": world, "world_origin": world_origin, "goal": goal})
        field, status = np.zeros((G,) + world.shape[-2:], np.uint32), np.zeros(G, np.int32)
        self._call("smpc_goal_field_batch", gf, _ptr(field), _ptr(status))
        return field, status

    def goal_field_device(self, gf: SmpcGoalFieldIn, field_ptr: int, status_ptr: int = 0):
        """Device pointers in gf (on_device == 1) and for field and status (0: none). The kernel runs on the handle's
        stream; the call waits for it (one word is read back): not for a captured tick."""
        assert gf.on_device == 1
        self._call("smpc_goal_field_batch", gf, field_ptr, status_ptr or None)

    def extract_plan(self, gp: GlobalPlanParams, world: np.ndarray, world_origin: np.ndarray, resolution: float, field: np.ndarray,
                     goal: np.ndarray, robot_goal: np.ndarray, pose: np.ndarray, plan: np.ndarray = None):
        """The plans of B robots down their goals' fields (host arrays): field [G,Hy,Hx] uint32 (goal_field), goal [G,2],
        robot_goal [B] int32, pose [B,3]; world as for goal_field. plan [B,gp.max_poses,2]: the rows before the call (default
        NaN): the call writes the first plan_len rows of each robot and leaves the others. Returns (plan, plan_len [B]
        int32, error [B] int32: enum smpc_plan_error, _abi_global_plan.PLAN_ERRORS)."""
        goal = np.ascontiguousarray(goal, np.float64).reshape(-1, 2)
        field = np.ascontiguousarray(field, np.uint32)
        robot_goal = np.ascontiguousarray(robot_goal, np.int32)
        pose = np.ascontiguousarray(pose, np.float64)
        B, G = pose.shape[0], goal.shape[0]
        world, world_origin, shared = self._plan_world_arrays(world, world_origin, G)
        assert field.shape == (G,) + world.shape[-2:] and robot_goal.shape == (B,) and pose.shape == (B, 3)
        plan = np.full((B, gp.max_poses, 2), np.nan) if plan is None else np.array(plan, dtype=np.float64, order="C")
        assert plan.shape == (B, gp.max_poses, 2)
        ep = point(self.extract_plan_c(gp, B, G, world.shape[-1], world.shape[-2], shared, resolution, 0),
                   {"world": world, "world_origin": world_origin, "field": field, "goal": goal, "robot_goal": robot_goal, "pose": pose})
        plan_len, error = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._call("smpc_extract_plan_batch", ep, _ptr(plan), _ptr(plan_len), _ptr(error))
        return plan, plan_len, error

    def extract_plan_device(self, ep: SmpcExtractPlanIn, plan_ptr: int, plan_len_ptr: int, error_ptr: int = 0):
        """Device pointers in ep (on_device == 1) and for plan, plan_len and error (0: none); asynchronous on the handle's
        stream."""
        assert ep.on_device == 1
        self._call("smpc_extract_plan_batch", ep, plan_ptr, plan_len_ptr, error_ptr or None)

    # -- line-of-sight filter of the people (smpc_visible_people_batch, include/smpc_visibility.h) -----------------------
    @staticmethod
    def visibility_c(vp: VisibilityParams, B: int, Np: int, world_x: int, world_y: int, world_shared: bool, resolution: float,
                     on_device: int) -> SmpcVisibilityIn:
        return SmpcVisibilityIn(B=int(B), Np=int(Np), on_device=int(on_device), world_x=int(world_x), world_y=int(world_y),
                                world_shared=1 if world_shared else 0, occlusion_min_cost=int(vp.occlusion_min_cost),
                                unknown_occludes=1 if vp.unknown_occludes else 0, resolution=float(resolution),
                                max_range=float(vp.max_range))

    def visible_people(self, vp: VisibilityParams, world: np.ndarray, world_origin: np.ndarray, resolution: float,
                       robot_pose: np.ndarray, people: np.ndarray, count: np.ndarray, visible: np.ndarray = None,
                       seen: np.ndarray = None):
        """The persons each of B robots has in line of sight (host arrays): world [Hy,Hx] uint8 with world_origin [2] (one map
        shared by all robots) or [B,Hy,Hx] with [B,2], robot_pose [B,3], people [B,Np,5], count [B] int32. visible [B,Np,5] /
        seen [B,Np] uint8: the arrays before the call (default NaN / 0xEE): the call writes the first visible_count rows
        and the first count flags of each robot and leaves the others. Returns (visible, visible_count [B] int32, seen:
        _abi_visibility.SEEN_CODES)."""
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        people = np.ascontiguousarray(people, np.float64)
        count = np.ascontiguousarray(count, np.int32)
        B, Np = people.shape[0], people.shape[1]
        world, world_origin, shared = self._plan_world_arrays(world, world_origin, B)
        assert people.shape == (B, Np, 5) and robot_pose.shape == (B, 3) and count.shape == (B,)
        visible = np.full((B, Np, 5), np.nan) if visible is None else np.array(visible, dtype=np.float64, order="C")
        seen = np.full((B, Np), 0xEE, np.uint8) if seen is None else np.array(seen, dtype=np.uint8, order="C")
        assert visible.shape == (B, Np, 5) and seen.shape == (B, Np)
        vi = point(self.visibility_c(vp, B, Np, world.shape[-1], world.shape[-2], shared, resolution, 0),
                   {"world": world, "world_origin": world_origin, "robot_pose": robot_pose, "people": people, "count": count})
        visible_count = np.zeros(B, np.int32)
        self._call("smpc_visible_people_batch", vi, _ptr(visible), _ptr(visible_count), _ptr(seen))
        return visible, visible_count, seen

    def visible_people_device(self, vi: SmpcVisibilityIn, visible_ptr: int, visible_count_ptr: int, seen_ptr: int = 0):
        """Device pointers in vi (on_device == 1) and for visible, visible_count and seen (0: none); asynchronous on the
        handle's stream."""
        assert vi.on_device == 1
        self._call("smpc_visible_people_batch", vi, visible_ptr, visible_count_ptr, seen_ptr or None)

    # -- people tracks (smpc_track_people_batch, include/smpc_tracker.h) ----------------------------------------------------
    @staticmethod
    def tracker_c(tp: TrackerParams, B: int, Nd: int, Np: int, dt: float, on_device: int) -> SmpcTrackerIn:
        return SmpcTrackerIn(B=int(B), Nd=int(Nd), Nt=int(tp.slots), Np=int(Np), on_device=int(on_device),
                             confirm_hits=int(tp.confirm_hits), max_missed=int(tp.max_missed), dt=float(dt), alpha=float(tp.alpha),
                             gain=tp.gain(dt), gate=float(tp.gate))

    def track_people(self, tp: TrackerParams, dt: float, tracks: np.ndarray, track_meta: np.ndarray, next_id: np.ndarray,
                     detections: np.ndarray, det_count: np.ndarray, robot_pose: np.ndarray, Np: int = None, people: np.ndarray = None,
                     out_track: np.ndarray = None, with_out_track: bool = True):
        """One tick of the people tracker on host arrays: tracks [B,Nt,4] float64, track_meta [B,Nt,4] int32 and next_id [B]
        int32 are the state the last call returned (zeros to start with; they are not modified), Nt = tp.slots; detections
        [B,Nd,5] (only x and y are read), det_count [B] int32, robot_pose [B,3]. people [B,Np,5] / out_track [B,Np,2] int32:
        the arrays before the call (default NaN / -1): the call writes the first count rows of each robot and leaves the
        others. Returns (people, count [B] int32, out_track or None with with_out_track=False, new tracks, new track_meta,
        new next_id)."""
        detections = np.ascontiguousarray(detections, np.float64)
        det_count = np.ascontiguousarray(det_count, np.int32)
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        B, Nd, Nt = detections.shape[0], detections.shape[1], int(tp.slots)
        Np = Nt if Np is None else int(Np)
        tracks = np.array(tracks, np.float64, order="C")
        track_meta = np.array(track_meta, np.int32, order="C")
        next_id = np.array(next_id, np.int32, order="C")
        assert detections.shape == (B, Nd, 5) and det_count.shape == (B,) and robot_pose.shape == (B, 3)
        assert tracks.shape == (B, Nt, 4) and track_meta.shape == (B, Nt, 4) and next_id.shape == (B,)
        people = np.full((B, Np, 5), np.nan) if people is None else np.array(people, dtype=np.float64, order="C")
        if with_out_track:
            out_track = np.full((B, Np, 2), -1, np.int32) if out_track is None else np.array(out_track, dtype=np.int32, order="C")
            assert out_track.shape == (B, Np, 2)
        else:
            out_track = None
        assert people.shape == (B, Np, 5)
        ti = point(self.tracker_c(tp, B, Nd, Np, dt, 0), {"detections": detections, "det_count": det_count, "robot_pose": robot_pose})
        count = np.zeros(B, np.int32)
        self._call("smpc_track_people_batch", ti, _ptr(tracks), _ptr(track_meta), _ptr(next_id), _ptr(people), _ptr(count), _ptr(out_track))
        return people, count, out_track, tracks, track_meta, next_id

    def track_people_device(self, ti: SmpcTrackerIn, tracks_ptr: int, track_meta_ptr: int, next_id_ptr: int, people_ptr: int,
                            count_ptr: int, out_track_ptr: int = 0):
        """Device pointers in ti (on_device == 1) and for the state (tracks, track_meta, next_id: read and written), people,
        count and out_track (0: none); asynchronous on the handle's stream."""
        assert ti.on_device == 1
        self._call("smpc_track_people_batch", ti, tracks_ptr, track_meta_ptr, next_id_ptr, people_ptr, count_ptr, out_track_ptr or None)

    # -- people detections (smpc_detect_people_batch, include/smpc_detector.h) ----------------------------------------------
    @staticmethod
    def detector_c(dp: DetectorParams, B: int, Np: int, Nd: int, on_device: int) -> SmpcDetectorIn:
        miss, clutter = dp.thresholds()
        noise_scale, noise_growth, clutter_scale = dp.scales()
        seed_lo, seed_hi = dp.key()
        return SmpcDetectorIn(B=int(B), Np=int(Np), Nd=int(Nd), Kc=int(dp.clutter_candidates), on_device=int(on_device), seed_lo=seed_lo,
                              seed_hi=seed_hi, miss_threshold=miss, clutter_threshold=clutter, body_radius=float(dp.body_radius),
                              noise_scale=noise_scale, noise_growth=noise_growth, clutter_scale=clutter_scale)

    def detect_people(self, dp: DetectorParams, draw_state: np.ndarray, people: np.ndarray, count: np.ndarray, robot_pose: np.ndarray,
                      Nd: int = None, detections: np.ndarray = None, det_source: np.ndarray = None, outcome: np.ndarray = None,
                      with_source: bool = True, with_outcome: bool = True):
        """One tick of the detector model on host arrays: draw_state [B,2] uint32 (stream id, tick counter) is the state the
        last call returned (it is not modified); people [B,Np,5], count [B] int32, robot_pose [B,3]. detections [B,Nd,5] /
        det_source [B,Nd] int32 / outcome [B,Np] uint8: the arrays before the call (default NaN / -99 / 255): the call writes
        the first det_count rows of each robot, and the outcome of the first clamp(count, 0, Np) persons, and leaves the others.
        Returns (detections, det_count [B] int32, det_source or None with with_source=False, outcome or None with
        with_outcome=False, new draw_state)."""
        people = np.ascontiguousarray(people, np.float64)
        count = np.ascontiguousarray(count, np.int32)
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        draw_state = np.array(draw_state, np.uint32, order="C")
        B, Np = people.shape[0], people.shape[1]
        Nd = Np if Nd is None else int(Nd)
        assert people.shape == (B, Np, 5) and count.shape == (B,) and robot_pose.shape == (B, 3) and draw_state.shape == (B, 2)
        detections = np.full((B, Nd, 5), np.nan) if detections is None else np.array(detections, dtype=np.float64, order="C")
        assert detections.shape == (B, Nd, 5)
        if with_source:
            det_source = np.full((B, Nd), -99, np.int32) if det_source is None else np.array(det_source, dtype=np.int32, order="C")
            assert det_source.shape == (B, Nd)
        else:
            det_source = None
        if with_outcome:
            outcome = np.full((B, Np), 255, np.uint8) if outcome is None else np.array(outcome, dtype=np.uint8, order="C")
            assert outcome.shape == (B, Np)
        else:
            outcome = None
        di = point(self.detector_c(dp, B, Np, Nd, 0), {"people": people, "count": count, "robot_pose": robot_pose})
        det_count = np.zeros(B, np.int32)
        self._call("smpc_detect_people_batch", di, _ptr(draw_state), _ptr(detections), _ptr(det_count), _ptr(det_source), _ptr(outcome))
        return detections, det_count, det_source, outcome, draw_state

    def detect_people_device(self, di: SmpcDetectorIn, draw_state_ptr: int, detections_ptr: int, det_count_ptr: int, det_source_ptr: int = 0,
                             outcome_ptr: int = 0):
        """Device pointers in di (on_device == 1) and for the state (draw_state: read and written), detections, det_count,
        det_source and outcome (0: none); asynchronous on the handle's stream."""
        assert di.on_device == 1
        self._call("smpc_detect_people_batch", di, draw_state_ptr, detections_ptr, det_count_ptr, det_source_ptr or None, outcome_ptr or None)

    # -- people detections from the scan (smpc_scan_people_batch, include/smpc_scan_people.h) -------------------------------
    @staticmethod
    def scan_people_c(sp: ScanDetectorParams, B: int, n_beams: int, Nd: int, on_device: int, resolution: float, world_origin,
                      sensor, sensor_memory=None) -> SmpcScanPeopleIn:
        """The call's struct without its array pointers: sp's lengths as squared cell distances of `resolution`, the cells
        counted from world_origin. sensor: the SensorParams whose scan is read (sp.max_range None: its marking range, also
        with sensor_memory, whose beams reach further but mark no further)."""
        wmin, wmax = sp.width_d2(resolution)
        si = SmpcScanPeopleIn(B=int(B), n_beams=int(n_beams), Nd=int(Nd), on_device=int(on_device), subtract_map=int(bool(sp.subtract_map)),
                              min_points=int(sp.min_points), link_d2=sp.link_d2(resolution), width_d2_min=wmin, width_d2_max=wmax,
                              range_d2=sp.range_d2(resolution, sensor), resolution=float(resolution), body_offset=float(sp.body_offset))
        si.world_origin[0], si.world_origin[1] = float(world_origin[0]), float(world_origin[1])
        return si

    def scan_people(self, si: SmpcScanPeopleIn, robot_pose: np.ndarray, beam_kind: np.ndarray, beam_cell: np.ndarray,
                    detections: np.ndarray = None, det_segment: np.ndarray = None, with_segment: bool = True, with_stats: bool = True):
        """One call of the scan-based people detector on host arrays. si: scan_people_c(..., on_device=0) (its array pointers are
        set here). robot_pose [B,3], beam_kind [B,n_beams] uint8, beam_cell [B,n_beams,2] int32. detections [B,Nd,5] /
        det_segment [B,Nd,4] int32: the arrays before the call (default NaN / -99): the call writes the first det_count rows of
        each robot and leaves the others. Returns (detections, det_count [B] int32, det_segment or None with with_segment=False,
        seg_stats [B,4] int32 or None with with_stats=False)."""
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        beam_kind = np.ascontiguousarray(beam_kind, np.uint8)
        beam_cell = np.ascontiguousarray(beam_cell, np.int32)
        B, n, Nd = robot_pose.shape[0], si.n_beams, si.Nd
        assert si.on_device == 0 and si.B == B
        assert robot_pose.shape == (B, 3) and beam_kind.shape == (B, n) and beam_cell.shape == (B, n, 2)
        detections = np.full((B, Nd, 5), np.nan) if detections is None else np.array(detections, dtype=np.float64, order="C")
        assert detections.shape == (B, Nd, 5)
        if with_segment:
            det_segment = np.full((B, Nd, 4), -99, np.int32) if det_segment is None else np.array(det_segment, dtype=np.int32, order="C")
            assert det_segment.shape == (B, Nd, 4)
        else:
            det_segment = None
        det_count = np.full(B, -1, np.int32)
        seg_stats = np.full((B, 4), -1, np.int32) if with_stats else None
        point(si, {"robot_pose": robot_pose, "beam_kind": beam_kind, "beam_cell": beam_cell})
        self._call("smpc_scan_people_batch", si, _ptr(detections), _ptr(det_count), _ptr(det_segment), _ptr(seg_stats))
        return detections, det_count, det_segment, seg_stats

    def scan_people_device(self, si: SmpcScanPeopleIn, detections_ptr: int, det_count_ptr: int, det_segment_ptr: int = 0, seg_stats_ptr: int = 0):
        """Device pointers in si (on_device == 1) and for detections, det_count, det_segment and seg_stats (0: none);
        asynchronous on the handle's stream."""
        assert si.on_device == 1
        self._call("smpc_scan_people_batch", si, detections_ptr, det_count_ptr, det_segment_ptr or None, seg_stats_ptr or None)

    # -- plan repair (smpc_repair_plan_batch, include/smpc_plan_repair.h) -----------------------------------------------------
    @staticmethod
    def repair_plan_c(rp: PlanRepairParams, B: int, L: int, size_x: int, size_y: int, costmap_shared: bool, resolution: float,
                      on_device: int) -> SmpcPlanRepairIn:
        """The call's struct without its array pointers: rp's radius in cells of `resolution`, its clearance squared."""
        ri = SmpcPlanRepairIn(B=int(B), L=int(L), on_device=int(on_device), size_x=int(size_x), size_y=int(size_y),
                              costmap_shared=1 if costmap_shared else 0, radius=rp.radius_cells(resolution), stride=int(rp.stride),
                              resolution=float(resolution), clearance_d2=rp.clearance_d2)
        ri.cost.neutral_cost, ri.cost.cost_weight = int(rp.neutral_cost), int(rp.cost_weight)
        ri.cost.lethal_min_cost, ri.cost.allow_unknown = int(rp.lethal_min_cost), 1 if rp.allow_unknown else 0
        return ri

    def repair_plan(self, ri: SmpcPlanRepairIn, costmap: np.ndarray, costmap_origin: np.ndarray, robot_pose: np.ndarray, plan: np.ndarray,
                    plan_len: np.ndarray, plan_start: np.ndarray = None, with_info: bool = True, with_field: bool = False, field: np.ndarray = None):
        """One call of the plan repair on host arrays. ri: repair_plan_c(..., on_device=0) (its array pointers are set here).
        costmap [size_y,size_x] uint8 with costmap_origin [2] (ri.costmap_shared) or [B,size_y,size_x] with [B,2]; robot_pose
        [B,3]; plan [B,L,2] and plan_len [B] int32: the plans before the call, which are not modified; plan_start [B] int32 or
        None. field [B,S,S] uint32: the rows before the call (default 0). Returns (plan, plan_len, status [B] int32, info
        [B,4] int32 or None, field or None): copies of the plans with the repaired robots' rows replaced."""
        costmap = np.ascontiguousarray(costmap, np.uint8)
        costmap_origin = np.ascontiguousarray(costmap_origin, np.float64).reshape(-1, 2)
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        B, L, S = robot_pose.shape[0], ri.L, 2 * ri.radius + 1
        assert ri.on_device == 0 and ri.B == B and robot_pose.shape == (B, 3)
        assert costmap.shape == ((ri.size_y, ri.size_x) if ri.costmap_shared else (B, ri.size_y, ri.size_x))
        assert costmap_origin.shape == ((1, 2) if ri.costmap_shared else (B, 2))
        plan = np.array(plan, dtype=np.float64, order="C")
        plan_len = np.array(plan_len, dtype=np.int32, order="C")
        assert plan.shape == (B, L, 2) and plan_len.shape == (B,)
        if plan_start is not None:
            plan_start = np.ascontiguousarray(plan_start, np.int32)
            assert plan_start.shape == (B,)
        workspace = np.zeros((B, L, 2))
        status = np.full(B, -1, np.int32)
        info = np.full((B, 4), -99, np.int32) if with_info else None
        if with_field or field is not None:
            field = np.zeros((B, S, S), np.uint32) if field is None else np.array(field, dtype=np.uint32, order="C")
            assert field.shape == (B, S, S)
        point(ri, {"costmap": costmap, "costmap_origin": costmap_origin, "robot_pose": robot_pose, "plan_start": plan_start})
        self._call("smpc_repair_plan_batch", ri, _ptr(plan), _ptr(plan_len), _ptr(workspace), _ptr(status), _ptr(info), _ptr(field))
        return plan, plan_len, status, info, field

    def repair_plan_device(self, ri: SmpcPlanRepairIn, plan_ptr: int, plan_len_ptr: int, workspace_ptr: int, status_ptr: int, info_ptr: int = 0,
                           field_ptr: int = 0):
        """Device pointers in ri (on_device == 1) and for plan, plan_len (both edited in place), workspace, status, info and field
        (0: none); asynchronous on the handle's stream."""
        assert ri.on_device == 1
        self._call("smpc_repair_plan_batch", ri, plan_ptr, plan_len_ptr, workspace_ptr, status_ptr, info_ptr or None, field_ptr or None)

    # -- plan smoothing (smpc_smooth_plan_batch, include/smpc_plan_smoother.h) -------------------------------------------------
    @staticmethod
    def smooth_plan_c(sp: PlanSmootherParams, B: int, L: int, world_x: int, world_y: int, world_shared: bool, resolution: float,
                      on_device: int, lethal_min_cost: int = 253, allow_unknown: bool = False) -> SmpcPlanSmootherIn:
        """The call's struct without its array pointers. lethal_min_cost / allow_unknown: what sp's None stand for (the
        planner's values)."""
        lethal = sp.lethal_min_cost if sp.lethal_min_cost is not None else lethal_min_cost
        unknown = sp.allow_unknown if sp.allow_unknown is not None else allow_unknown
        return SmpcPlanSmootherIn(B=int(B), L=int(L), on_device=int(on_device), world_x=int(world_x), world_y=int(world_y),
                                  world_shared=1 if world_shared else 0, max_its=int(sp.max_its), refinement_num=int(sp.refinement_num),
                                  lethal_min_cost=int(lethal), allow_unknown=1 if unknown else 0, resolution=float(resolution),
                                  w_data=float(sp.w_data), w_smooth=float(sp.w_smooth), tolerance=float(sp.tolerance))

    def smooth_plan(self, si: SmpcPlanSmootherIn, world: np.ndarray, world_origin: np.ndarray, plan: np.ndarray, plan_len: np.ndarray,
                    range_: np.ndarray = None, with_info: bool = True, with_change: bool = True):
        """One call of the plan smoothing on host arrays. si: smooth_plan_c(..., on_device=0) (its array pointers are set here).
        world [world_y,world_x] uint8 with world_origin [2] (si.world_shared) or [B,world_y,world_x] with [B,2]; plan [B,L,2]
        and plan_len [B] int32: the plans before the call, which are not modified; range_ [B,2] int32 or None. Returns
        (plan: a copy with the movable rows smoothed, status [B] int32: _abi_plan_smoother.SMOOTH_STATUS, info [B,4] int32 or
        None: sweeps, rounds, rejected, n; change [B] or None)."""
        world = np.ascontiguousarray(world, np.uint8)
        world_origin = np.ascontiguousarray(world_origin, np.float64).reshape(-1, 2)
        plan = np.array(plan, dtype=np.float64, order="C")
        plan_len = np.ascontiguousarray(plan_len, np.int32)
        B, L = si.B, si.L
        assert si.on_device == 0 and plan.shape == (B, L, 2) and plan_len.shape == (B,)
        assert world.shape == ((si.world_y, si.world_x) if si.world_shared else (B, si.world_y, si.world_x))
        assert world_origin.shape == ((1, 2) if si.world_shared else (B, 2))
        if range_ is not None:
            range_ = np.ascontiguousarray(range_, np.int32)
            assert range_.shape == (B, 2)
        status = np.full(B, -1, np.int32)
        info = np.full((B, 4), -99, np.int32) if with_info else None
        change = np.full(B, np.nan) if with_change else None
        point(si, {"world": world, "world_origin": world_origin, "plan_len": plan_len, "range": range_})
        self._call("smpc_smooth_plan_batch", si, _ptr(plan), _ptr(status), _ptr(info), _ptr(change))
        return plan, status, info, change

    def smooth_plan_device(self, si: SmpcPlanSmootherIn, plan_ptr: int, status_ptr: int, info_ptr: int = 0, change_ptr: int = 0):
        """Device pointers in si (on_device == 1) and for plan (smoothed in place), status, info and change (0: none);
        asynchronous on the handle's stream."""
        assert si.on_device == 1
        self._call("smpc_smooth_plan_batch", si, plan_ptr, status_ptr, info_ptr or None, change_ptr or None)

    # -- robot plant (smpc_robot_plant_batch, include/smpc_plant.h) ----------------------------------------------------------
    @staticmethod
    def plant_c(pp: PlantParams, prm: OptimizerParams, B: int, Np: int, on_device: int, world_x: int = 0, world_y: int = 0,
                resolution: float = 1.0, world_origin=(0.0, 0.0)) -> SmpcPlantIn:
        """The call's struct without its pointers: the velocity bounds are prm's (v_min, v_max, w_max), the period prm.dt; the
        walls are world_x x world_y cells of `resolution` at world_origin (point `world` at the map, or leave it NULL)."""
        dv_up, dv_down, dw = pp.deltas(prm.dt)
        pi = SmpcPlantIn(B=int(B), Np=int(Np), S=int(pp.substeps), L=int(pp.latency_ticks), on_device=int(on_device), Hx=int(world_x),
                         Hy=int(world_y), footprint_d2=pp.footprint_d2(resolution), wall_min_cost=int(pp.wall_min_cost),
                         unknown_is_wall=int(bool(pp.unknown_is_wall)), outside_is_wall=int(bool(pp.outside_is_wall)),
                         dt=float(prm.dt), v_min=float(prm.v_min), v_max=float(prm.v_max), w_max=float(prm.w_max), dv_up=dv_up,
                         dv_down=dv_down, dw=dw, contact_dist=pp.contact_dist(), resolution=float(resolution))
        pi.world_origin[0], pi.world_origin[1] = float(world_origin[0]), float(world_origin[1])
        return pi

    def robot_plant(self, pi: SmpcPlantIn, pose: np.ndarray, twist: np.ndarray, cmd_queue: np.ndarray, plant_tick: np.ndarray,
                    cmd: np.ndarray, agents: np.ndarray, count: np.ndarray, world: np.ndarray = None, contact: np.ndarray = None,
                    heading_cs: np.ndarray = None, with_heading: bool = True):
        """One period of the plant on host arrays. pi: plant_c(..., on_device=0) (its pointers are set here; world [Hy,Hx] uint8
        or None). pose [B,3], twist [B,2], cmd_queue [B,8,2] (None with L == 0) and plant_tick [B] uint32 are the state the
        last call returned (zeros to start with; they are not modified); cmd [B,2], agents [B,Np,5], count [B] int32.
        contact [B,2] int32 / heading_cs [B,2]: the arrays before the call (default -1 / NaN). Returns (new pose, new twist,
        new cmd_queue or None, new plant_tick, contact, heading_cs or None with with_heading=False)."""
        cmd = np.ascontiguousarray(cmd, np.float64)
        agents = np.ascontiguousarray(agents, np.float64)
        count = np.ascontiguousarray(count, np.int32)
        B, Np = agents.shape[0], agents.shape[1]
        pose = np.array(pose, np.float64, order="C")
        twist = np.array(twist, np.float64, order="C")
        plant_tick = np.array(plant_tick, np.uint32, order="C")
        cmd_queue = None if cmd_queue is None else np.array(cmd_queue, np.float64, order="C")
        assert pi.on_device == 0 and pi.B == B and pi.Np == Np
        assert cmd.shape == (B, 2) and agents.shape == (B, Np, 5) and count.shape == (B,)
        assert pose.shape == (B, 3) and twist.shape == (B, 2) and plant_tick.shape == (B,)
        assert cmd_queue is None or cmd_queue.shape == (B, 8, 2)
        contact = np.full((B, 2), -1, np.int32) if contact is None else np.array(contact, dtype=np.int32, order="C")
        if with_heading:
            heading_cs = np.full((B, 2), np.nan) if heading_cs is None else np.array(heading_cs, dtype=np.float64, order="C")
            assert heading_cs.shape == (B, 2)
        else:
            heading_cs = None
        if world is not None:
            world = np.ascontiguousarray(world, np.uint8)
            assert world.shape == (pi.Hy, pi.Hx)
        point(pi, {"world": world, "cmd": cmd, "agents": agents, "count": count})
        self._call("smpc_robot_plant_batch", pi, _ptr(pose), _ptr(twist), _ptr(cmd_queue), _ptr(plant_tick), _ptr(contact), _ptr(heading_cs))
        return pose, twist, cmd_queue, plant_tick, contact, heading_cs

    def robot_plant_device(self, pi: SmpcPlantIn, pose_ptr: int, twist_ptr: int, cmd_queue_ptr: int, plant_tick_ptr: int, contact_ptr: int,
                           heading_cs_ptr: int = 0):
        """Device pointers in pi (on_device == 1) and for the state (pose, twist, cmd_queue, plant_tick: read and written),
        contact and heading_cs (0: none); asynchronous on the handle's stream."""
        assert pi.on_device == 1
        self._call("smpc_robot_plant_batch", pi, pose_ptr, twist_ptr, cmd_queue_ptr or None, plant_tick_ptr, contact_ptr, heading_cs_ptr or None)

    # -- collision monitor (smpc_collision_monitor_batch, include/smpc_collision_monitor.h) ------------------------------------
    @staticmethod
    def collision_monitor_c(mp: MonitorParams, B: int, n_beams: int, on_device: int, resolution: float,
                            world_origin=(0.0, 0.0)) -> SmpcCollisionMonitorIn:
        """The call's struct without its array pointers: the zones (a host array the struct keeps alive as `_zones`: the
        library reads it during every call, whatever on_device), M and sim_dt from mp, the cells of `resolution` at
        world_origin that the beams' offsets count in."""
        from .params import MONITOR_ACTIONS, MONITOR_SHAPES
        zones = (SmpcMonitorZone * len(mp.zones))()
        for zc, z in zip(zones, mp.zones):
            zc.shape, zc.action, zc.min_points = MONITOR_SHAPES[z.shape], MONITOR_ACTIONS[z.action], int(z.min_points)
            zc.radius = float(z.radius) if z.radius is not None else 0.0
            zc.slowdown_ratio, zc.linear_limit, zc.angular_limit = float(z.slowdown_ratio), float(z.linear_limit), float(z.angular_limit)
            zc.n_vertices = 0 if z.vertices is None else len(z.vertices)
            for i, (vx, vy) in enumerate(z.vertices or ()):
                zc.vertices[i][0], zc.vertices[i][1] = vx, vy
        mi = SmpcCollisionMonitorIn(B=int(B), n_beams=int(n_beams), Z=len(mp.zones), M=mp.steps(), on_device=int(on_device),
                                    sim_dt=float(mp.simulation_time_step), resolution=float(resolution))
        mi.world_origin[0], mi.world_origin[1] = float(world_origin[0]), float(world_origin[1])
        mi._zones = zones
        mi.zones = C.addressof(zones)
        return mi

    def collision_monitor(self, mi: SmpcCollisionMonitorIn, robot_pose: np.ndarray, cmd: np.ndarray, beam_kind: np.ndarray,
                          beam_cell: np.ndarray, with_zone_points: bool = True, with_ratio: bool = True, with_heading: bool = True,
                          with_step: bool = True, fill: dict = None) -> dict:
        """One call of the monitor on host arrays. mi: collision_monitor_c(..., on_device=0) (its array pointers are set here).
        robot_pose [B,3], cmd [B,2], beam_kind [B,n_beams] uint8, beam_cell [B,n_beams,2] int32. Returns {"cmd_out" [B,2],
        "action" [B,4] int32, "zone_points" [B,Z] int32, "ratio" [B], "heading_cs" [B,2], "step_cs" [B,2]}; an output
        switched off by its with_* flag is passed as NULL and comes back None. What the call does not write keeps the
        arrays' fill: NaN and -1, or the arrays `fill` gives by name."""
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        cmd = np.ascontiguousarray(cmd, np.float64)
        beam_kind = np.ascontiguousarray(beam_kind, np.uint8)
        beam_cell = np.ascontiguousarray(beam_cell, np.int32)
        B, n, Z = robot_pose.shape[0], mi.n_beams, mi.Z
        assert mi.on_device == 0 and mi.B == B
        assert robot_pose.shape == (B, 3) and cmd.shape == (B, 2) and beam_kind.shape == (B, n) and beam_cell.shape == (B, n, 2)
        spec = {"cmd_out": ((B, 2), np.float64, np.nan, True), "action": ((B, 4), np.int32, -1, True),
                "zone_points": ((B, Z), np.int32, -1, with_zone_points), "ratio": ((B,), np.float64, np.nan, with_ratio),
                "heading_cs": ((B, 2), np.float64, np.nan, with_heading), "step_cs": ((B, 2), np.float64, np.nan, with_step)}
        out = {}
        for k, (shape, dtype, value, on) in spec.items():
            if not on:
                out[k] = None
            elif fill is not None and k in fill:
                out[k] = np.array(fill[k], dtype=dtype, order="C")
                assert out[k].shape == shape
            else:
                out[k] = np.full(shape, value, dtype)
        point(mi, {"robot_pose": robot_pose, "cmd": cmd, "beam_kind": beam_kind, "beam_cell": beam_cell})
        self._call("smpc_collision_monitor_batch", mi, *(_ptr(out[k]) for k in spec))
        return out

    def collision_monitor_device(self, mi: SmpcCollisionMonitorIn, cmd_out_ptr: int, action_ptr: int, zone_points_ptr: int = 0,
                                 ratio_ptr: int = 0, heading_cs_ptr: int = 0, step_cs_ptr: int = 0):
        """Device pointers in mi (on_device == 1; its zones stay the host array collision_monitor_c made) and for the outputs
        (0: none); asynchronous on the handle's stream."""
        assert mi.on_device == 1
        self._call("smpc_collision_monitor_batch", mi, cmd_out_ptr, action_ptr, zone_points_ptr or None, ratio_ptr or None,
                   heading_cs_ptr or None, step_cs_ptr or None)

    # -- sensed local costmaps (smpc_sensed_costmap_batch, include/smpc_sensed_costmap.h) ----------------------------------
    @staticmethod
    def sensed_costmap_c(B: int, Np: int, size_x: int, size_y: int, world_x: int, world_y: int, world_shared: bool, resolution: float,
                         on_device: int, n_beams: int, agent_d2: int, d2_max: int, base: int = 0, outside_cost: int = 255,
                         occlusion_min_cost: int = 254, unknown_occludes: bool = False) -> SmpcSensedCostmapIn:
        if not 0 <= int(outside_cost) <= 255:
            raise SmpcError(f"outside_cost must be 0..255, got {outside_cost}")
        return SmpcSensedCostmapIn(B=int(B), Np=int(Np), on_device=int(on_device), size_x=int(size_x), size_y=int(size_y),
                                   world_x=int(world_x), world_y=int(world_y), world_shared=1 if world_shared else 0,
                                   n_beams=int(n_beams), agent_d2=int(agent_d2), d2_max=int(d2_max),
                                   occlusion_min_cost=int(occlusion_min_cost), unknown_occludes=1 if unknown_occludes else 0,
                                   base=int(base), outside_cost=int(outside_cost), resolution=float(resolution))

    def sensed_costmap(self, world: np.ndarray, world_origin: np.ndarray, resolution: float, robot_pose: np.ndarray,
                       people: np.ndarray, count: np.ndarray, cell: np.ndarray, size_x: int, size_y: int, beam_cells: np.ndarray,
                       agent_d2: int, inflation_cost: np.ndarray, base: int = 0, outside_cost: int = 255,
                       occlusion_min_cost: int = 254, unknown_occludes: bool = False, beams: bool = True):
        """The sensed windows of B robots (host arrays): world [Hy,Hx] uint8 with world_origin [2] (one map shared by all
        robots) or [B,Hy,Hx] with [B,2], robot_pose [B,3], people [B,Np,5], count [B] int32, cell [B,2] int32 (the world cell of
        every window's cell (0,0)), beam_cells [n_beams,2] int32 (e.g. SensorParams.beam_cells), inflation_cost [d2_max + 1]
        uint8 (e.g. SensorParams.inflation_table). Returns (costmap [B,size_y,size_x] uint8, beam_kind [B,n_beams] uint8:
        _abi_sensed_costmap.BEAM_KINDS, beam_cell [B,n_beams,2] int32); the last two None with beams=False, which passes NULL
        arrays."""
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        people = np.ascontiguousarray(people, np.float64)
        count = np.ascontiguousarray(count, np.int32)
        cell = np.ascontiguousarray(cell, np.int32)
        beam_cells = np.ascontiguousarray(beam_cells, np.int32)
        inflation_cost = np.ascontiguousarray(inflation_cost, np.uint8)
        B, Np, K = people.shape[0], people.shape[1], beam_cells.shape[0]
        world, world_origin, shared = self._plan_world_arrays(world, world_origin, B)
        assert people.shape == (B, Np, 5) and robot_pose.shape == (B, 3) and count.shape == (B,) and cell.shape == (B, 2)
        assert beam_cells.shape == (K, 2) and inflation_cost.ndim == 1 and inflation_cost.size >= 1
        si = point(self.sensed_costmap_c(B, Np, size_x, size_y, world.shape[-1], world.shape[-2], shared, resolution, 0, K, agent_d2,
                                         inflation_cost.size - 1, base, outside_cost, occlusion_min_cost, unknown_occludes),
                   {"world": world, "world_origin": world_origin, "robot_pose": robot_pose, "people": people, "count": count,
                    "cell": cell, "beam_cells": beam_cells, "inflation_cost": inflation_cost})
        costmap = np.zeros((B, int(size_y), int(size_x)), np.uint8)
        kind = np.zeros((B, K), np.uint8) if beams else None
        hit = np.zeros((B, K, 2), np.int32) if beams else None
        self._call("smpc_sensed_costmap_batch", si, _ptr(costmap), _ptr(kind), _ptr(hit))
        return costmap, kind, hit

    def sensed_costmap_device(self, si: SmpcSensedCostmapIn, costmap_ptr: int, beam_kind_ptr: int = 0, beam_cell_ptr: int = 0):
        """Device pointers in si (on_device == 1) and for costmap, beam_kind and beam_cell (0: none); asynchronous on the
        handle's stream."""
        assert si.on_device == 1
        self._call("smpc_sensed_costmap_batch", si, costmap_ptr, beam_kind_ptr or None, beam_cell_ptr or None)

    # -- sensed local costmaps with memory (smpc_obstacle_memory_batch, include/smpc_obstacle_memory.h) ---------------------
    @staticmethod
    def obstacle_memory_c(scan: SmpcSensedCostmapIn, mark_d2: int, footprint_d2: int = -1) -> SmpcObstacleMemoryIn:
        """The input struct around a copy of `scan` (sensed_costmap_c's, pointers and all)."""
        mi = SmpcObstacleMemoryIn(mark_d2=int(mark_d2), footprint_d2=int(footprint_d2))
        C.memmove(C.byref(mi.scan), C.byref(scan), C.sizeof(SmpcSensedCostmapIn))
        return mi

    def obstacle_memory(self, memory: np.ndarray, memory_cell: np.ndarray, world: np.ndarray, world_origin: np.ndarray, resolution: float,
                        robot_pose: np.ndarray, people: np.ndarray, count: np.ndarray, cell: np.ndarray, size_x: int, size_y: int,
                        beam_cells: np.ndarray, agent_d2: int, inflation_cost: np.ndarray, mark_d2: int, footprint_d2: int = -1,
                        base: int = 0, outside_cost: int = 255, occlusion_min_cost: int = 254, unknown_occludes: bool = False,
                        beams: bool = True):
        """One call of the sensed windows with memory on host arrays: memory [B,size_y,(size_x + 31) // 32] uint32 and
        memory_cell [B,2] int32 are the state the last call returned (zeros to start with; they are not modified), every
        other argument as sensed_costmap's, with beam_cells out to the clearing range. Returns (costmap, beam_kind,
        beam_cell, new memory, new memory_cell); the two beam arrays None with beams=False."""
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        people = np.ascontiguousarray(people, np.float64)
        count = np.ascontiguousarray(count, np.int32)
        cell = np.ascontiguousarray(cell, np.int32)
        beam_cells = np.ascontiguousarray(beam_cells, np.int32)
        inflation_cost = np.ascontiguousarray(inflation_cost, np.uint8)
        B, Np, K = people.shape[0], people.shape[1], beam_cells.shape[0]
        memory = np.array(memory, np.uint32, order="C")
        memory_cell = np.array(memory_cell, np.int32, order="C")
        world, world_origin, shared = self._plan_world_arrays(world, world_origin, B)
        assert people.shape == (B, Np, 5) and robot_pose.shape == (B, 3) and count.shape == (B,) and cell.shape == (B, 2)
        assert beam_cells.shape == (K, 2) and inflation_cost.ndim == 1 and inflation_cost.size >= 1
        assert memory.shape == (B, int(size_y), (int(size_x) + 31) // 32) and memory_cell.shape == (B, 2)
        arrays = {"world": world, "world_origin": world_origin, "robot_pose": robot_pose, "people": people, "count": count,
                  "cell": cell, "beam_cells": beam_cells, "inflation_cost": inflation_cost}
        si = point(self.sensed_costmap_c(B, Np, size_x, size_y, world.shape[-1], world.shape[-2], shared, resolution, 0, K, agent_d2,
                                         inflation_cost.size - 1, base, outside_cost, occlusion_min_cost, unknown_occludes), arrays)
        mi = self.obstacle_memory_c(si, mark_d2, footprint_d2)
        costmap = np.zeros((B, int(size_y), int(size_x)), np.uint8)
        kind = np.zeros((B, K), np.uint8) if beams else None
        hit = np.zeros((B, K, 2), np.int32) if beams else None
        self._call("smpc_obstacle_memory_batch", mi, _ptr(memory), _ptr(memory_cell), _ptr(costmap), _ptr(kind), _ptr(hit))
        del arrays
        return costmap, kind, hit, memory, memory_cell

    def obstacle_memory_device(self, mi: SmpcObstacleMemoryIn, memory_ptr: int, memory_cell_ptr: int, costmap_ptr: int,
                               beam_kind_ptr: int = 0, beam_cell_ptr: int = 0):
        """Device pointers in mi.scan (on_device == 1) and for memory, memory_cell (both read and written), costmap,
        beam_kind and beam_cell (0: none); asynchronous on the handle's stream."""
        assert mi.scan.on_device == 1
        self._call("smpc_obstacle_memory_batch", mi, memory_ptr, memory_cell_ptr, costmap_ptr, beam_kind_ptr or None, beam_cell_ptr or None)

    # -- nearest-agent gather of a shared world (smpc_nearest_people_batch, include/smpc_nearest.h) -----------------------
    @staticmethod
    def nearest_c(B: int, Np: int, A: int, grid_x: int, grid_y: int, grid_origin, bin_size: float, max_range: float,
                  on_device: int) -> SmpcNearestIn:
        ni = SmpcNearestIn(B=int(B), Np=int(Np), A=int(A), on_device=int(on_device), grid_x=int(grid_x), grid_y=int(grid_y),
                           bin_size=float(bin_size), max_range=float(max_range))
        ni.grid_origin[0], ni.grid_origin[1] = float(grid_origin[0]), float(grid_origin[1])
        return ni

    def nearest_workspace_bytes(self, A: int, grid_x: int, grid_y: int) -> int:
        """Bytes of device memory smpc_nearest_people_batch needs as `workspace` for A agents on grid_x x grid_y bins (0 for a
        shape the call refuses)."""
        return int(self.lib.smpc_nearest_workspace_bytes(int(A), int(grid_x), int(grid_y)))

    def nearest_people(self, agents: np.ndarray, robot_pose: np.ndarray, Np: int, grid_x: int, grid_y: int, grid_origin,
                       bin_size: float, max_range: float, self_row: np.ndarray = None, people: np.ndarray = None,
                       source: np.ndarray = None):
        """Each of B robots' at most Np nearest agents within max_range out of one table (host arrays): agents [A,5],
        robot_pose [B,3], self_row [B] int32 (the row of `agents` that is the robot itself, < 0: none) or None; the bins
        (grid_x x grid_y of bin_size from grid_origin [2], e.g. params.SharedWorldParams.grid) do not show in the result.
        people [B,Np,5] / source [B,Np] int32: the arrays before the call (default NaN / -1): the call writes the first
        count rows of each robot, nearest first, and leaves the others. Returns (people, count [B] int32, source: the rows
        of `agents`)."""
        agents = np.ascontiguousarray(agents, np.float64).reshape(-1, 5)
        robot_pose = np.ascontiguousarray(robot_pose, np.float64)
        B, A, Np = robot_pose.shape[0], agents.shape[0], int(Np)
        assert robot_pose.shape == (B, 3)
        if self_row is not None:
            self_row = np.ascontiguousarray(self_row, np.int32)
            assert self_row.shape == (B,)
        people = np.full((B, Np, 5), np.nan) if people is None else np.array(people, dtype=np.float64, order="C")
        source = np.full((B, Np), -1, np.int32) if source is None else np.array(source, dtype=np.int32, order="C")
        assert people.shape == (B, Np, 5) and source.shape == (B, Np)
        ni = point(self.nearest_c(B, Np, A, grid_x, grid_y, grid_origin, bin_size, max_range, 0),
                   {"agents": agents if A > 0 else None, "robot_pose": robot_pose, "self": self_row})
        count = np.zeros(B, np.int32)
        self._call("smpc_nearest_people_batch", ni, _ptr(people), _ptr(count), _ptr(source))
        return people, count, source

    def nearest_people_device(self, ni: SmpcNearestIn, people_ptr: int, count_ptr: int, source_ptr: int = 0):
        """Device pointers in ni (on_device == 1, workspace included) and for people, count and source (0: none);
        asynchronous on the handle's stream."""
        assert ni.on_device == 1
        self._call("smpc_nearest_people_batch", ni, people_ptr, count_ptr, source_ptr or None)

    # -- the reactive crowd of a shared world (smpc_crowd_pool_step_batch, include/smpc_crowd_pool.h) ----------------------
    @staticmethod
    def crowd_pool_c(cp: PoolCrowdParams, M: int, A: int, K: int, dt: float, grid_x: int, grid_y: int, grid_origin,
                     bin_size: float, on_device: int, bins_ready: int = 0) -> SmpcCrowdPoolIn:
        ci = SmpcCrowdPoolIn(M=int(M), A=int(A), K=int(K), on_device=int(on_device), cyclic=1 if cp.cyclic else 0,
                             bins_ready=int(bins_ready), grid_x=int(grid_x), grid_y=int(grid_y), bin_size=float(bin_size),
                             interaction_range=float(cp.interaction_range), dt=float(dt), goal_radius=cp.goal_radius,
                             person_radius=cp.person_radius, desired_speed=cp.desired_speed)
        ci.grid_origin[0], ci.grid_origin[1] = float(grid_origin[0]), float(grid_origin[1])
        return ci

    def crowd_pool_step(self, cp: PoolCrowdParams, dt: float, agents: np.ndarray, M: int, cursor: np.ndarray,
                        waypoints: np.ndarray, n_waypoints: np.ndarray, grid_x: int, grid_y: int, grid_origin, bin_size: float,
                        desired_speeds: np.ndarray = None, od_indexes: np.ndarray = None, od_origin: np.ndarray = None,
                        od_resolution: float = None, next: np.ndarray = None):
        """One control period of a shared world's pedestrians (host arrays): agents [A,5], of which rows 0 .. M-1 move and
        the others are partners that stand in for themselves (the robots); cursor [M], waypoints [M,K,2], n_waypoints [M];
        the bins (grid_x x grid_y of bin_size from grid_origin [2], e.g. params.SharedWorldParams.grid(world, reach)) do
        not show in the result; optional desired_speeds [M] and one ObstacleDistance grid od_indexes [h,w] uint32 with
        od_origin [2] and od_resolution. next [M,5]: the array before the call (default NaN). `agents` is left alone.
        Returns (next [M,5], the updated copy of cursor)."""
        agents = np.ascontiguousarray(agents, np.float64).reshape(-1, 5)
        A, M = agents.shape[0], int(M)
        rows = max(M, 0)
        cursor = np.array(cursor, dtype=np.int32, order="C")
        waypoints = np.ascontiguousarray(waypoints, np.float64)
        n_waypoints = np.ascontiguousarray(n_waypoints, np.int32)
        K = int(waypoints.shape[1])
        assert cursor.shape == (rows,) and waypoints.shape == (rows, K, 2) and n_waypoints.shape == (rows,)
        if desired_speeds is not None:
            desired_speeds = np.ascontiguousarray(desired_speeds, np.float64)
            assert desired_speeds.shape == (rows,)
        next = np.full((rows, 5), np.nan) if next is None else np.array(next, dtype=np.float64, order="C")
        assert next.shape == (rows, 5)
        ci = point(self.crowd_pool_c(cp, M, A, K, dt, grid_x, grid_y, grid_origin, bin_size, 0),
                   {"agents": agents if A > 0 else None, "waypoints": waypoints if rows > 0 else None,
                    "n_waypoints": n_waypoints if rows > 0 else None, "desired_speeds": desired_speeds})
        if od_indexes is not None:
            grid = np.ascontiguousarray(od_indexes, np.uint32)
            origin = np.ascontiguousarray(od_origin, np.float64).reshape(2)
            assert grid.ndim == 2
            point(ci, {"od_indexes": grid if grid.size else None, "od_origin": origin})
            ci.od_height, ci.od_width, ci.od_resolution = int(grid.shape[0]), int(grid.shape[1]), float(od_resolution)
        self._call("smpc_crowd_pool_step_batch", ci, _ptr(next) if rows > 0 else None, _ptr(cursor) if rows > 0 else None)
        return next, cursor

    def crowd_pool_step_device(self, ci: SmpcCrowdPoolIn, next_ptr: int, cursor_ptr: int):
        """Device pointers in ci (on_device == 1, workspace included; bins_ready as the caller vouches) and for next and
        cursor; asynchronous on the handle's stream."""
        assert ci.on_device == 1
        self._call("smpc_crowd_pool_step_batch", ci, next_ptr or None, cursor_ptr or None)

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
        P = self.params.dims(T, True)[3]
        fb = SmpcFormatBatch(B=B, T=T, path_rows=rows, on_device=0, time_step=float(self.params.dt))
        if n_poses is not None:
            n_poses = np.ascontiguousarray(n_poses, np.int32)
            assert n_poses.shape == (B,) and "length" in memory
            fb.n_poses, fb.max_poses = n_poses.ctypes.data, int(max_poses)
        fb.current_path_w = float(self.params.current_path_weight if current_path_w is None else current_path_w)
        fb.current_cmds_w = float(self.params.current_cmds_weight if current_cmds_w is None else current_cmds_w)
        point(fb, {"path": path, "cmds": cmds, "speed": speed})
        point(fb.memory, memory)
        out = {"robot_status": np.zeros((B, Tp, 6)), "pose0": np.zeros((B, 3)), "init_params": np.zeros((B, P)),
               "path_pts": np.zeros((B, Tp, 2)), "goal_yaw": np.zeros(B), "T_scene": np.zeros(B, np.int32)}
        self._call("smpc_format_to_optimize_batch", fb, point(SmpcFormatOut(), out))
        return out

    def format_device(self, fb: SmpcFormatBatch, fo: SmpcFormatOut):
        assert fb.on_device == 1
        self._call("smpc_format_to_optimize_batch", fb, fo)

    @staticmethod
    def new_memory(B: int, T: int, lengths: bool = False):
        """An empty TrajectoryMemory record per scene (host arrays, named like the fields of SmpcMemoryBatch). lengths:
        with the per-record sizes that scenes with horizons of their own need (smpc_memory_batch.length)."""
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
        ts = None if T_scene is None else np.ascontiguousarray(T_scene, np.int32)
        self._call("smpc_memory_store_batch", B, Tp - 1, 0, _ptr(status), _ptr(path), _ptr(cmds),
                   point(SmpcMemoryBatch(), memory), _ptr(ts))

    def memory_store_device(self, B: int, T: int, status_ptr: int, path_ptr: int, cmds_ptr: int, mb: SmpcMemoryBatch,
                            T_scene_ptr: int = 0):
        self._call("smpc_memory_store_batch", B, T, 1, status_ptr, path_ptr, cmds_ptr, mb, T_scene_ptr)
