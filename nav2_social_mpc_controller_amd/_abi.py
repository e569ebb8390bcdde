"""ctypes mirror of include/smpc.h (the C ABI of the HIP solver).

Only declarations live here: the constants, every struct (`c_name`: its C type) and FUNCTIONS, the signature of every
exported function; the shared library itself is loaded by `solver.py`. All of it must stay in lock-step with
include/smpc.h: tests/test_abi.py compiles a probe against the header and compares every sizeof, every field's offsetof
and the constants, and refuses a header struct or function without a mirror here.
"""
import ctypes as C

SMPC_ABI_VERSION = 6
SMPC_MAX_BLOCKS = 10
SMPC_MAX_AGENTS = 64

# enum smpc_linear_solver (mirrors OptimizerParams::solver_types, reference optimizer.hpp:71-77)
LINEAR_SOLVER = {
    "DENSE_SCHUR": 0,
    "SPARSE_SCHUR": 1,
    "DENSE_NORMAL_CHOLESKY": 2,
    "DENSE_QR": 3,
    "SPARSE_NORMAL_CHOLESKY": 4,
}

CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2
REASONS = ["none", "gradient_tol", "parameter_tol", "function_tol", "min_radius", "max_iterations",
           "invalid_steps", "eval_failed"]

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)


class SmpcParams(C.Structure):
    c_name = "smpc_params"
    _fields_ = [
        ("distance_w", C.c_double),
        ("socialwork_w", C.c_double),
        ("velocity_w", C.c_double),
        ("angle_w", C.c_double),
        ("agent_angle_w", C.c_double),
        ("proxemics_w", C.c_double),
        ("velocity_feasibility_w", C.c_double),
        ("obstacle_w", C.c_double),
        ("goal_align_w", C.c_double),
        ("control_horizon", C.c_int),
        ("parameter_block_length", C.c_int),
        ("max_iterations", C.c_int),
        ("linear_solver_type", C.c_int),
        ("fn_tol", C.c_double),
        ("gradient_tol", C.c_double),
        ("param_tol", C.c_double),
        ("desired_linear_vel", C.c_double),
        ("v_min", C.c_double),
        ("v_max", C.c_double),
        ("w_min", C.c_double),
        ("w_max", C.c_double),
        ("fixed_iterations", C.c_int),
        ("tol_needs_successful_step", C.c_int),
    ]


# smpc_scene_params: per-scene values of the SmpcParams fields with the same names (smpc_scene_batch.scene_params)
SCENE_PARAM_FIELDS = ("distance_w", "socialwork_w", "velocity_w", "angle_w", "agent_angle_w", "proxemics_w",
                      "velocity_feasibility_w", "obstacle_w", "goal_align_w", "desired_linear_vel",
                      "v_min", "v_max", "w_min", "w_max")


class SmpcSceneParams(C.Structure):
    c_name = "smpc_scene_params"
    _fields_ = [(f, C.c_double) for f in SCENE_PARAM_FIELDS]


class SmpcSceneBatch(C.Structure):
    c_name = "smpc_scene_batch"
    _fields_ = [
        ("B", C.c_int32),
        ("T", C.c_int32),
        ("N", C.c_int32),
        ("on_device", C.c_int32),
        ("dt", C.c_double),
        ("pose0", C.c_void_p),
        ("init_params", C.c_void_p),
        ("path_pts", C.c_void_p),
        ("goal_yaw", C.c_void_p),
        ("people", C.c_void_p),
        ("has_people", C.c_void_p),
        ("costmap", C.c_void_p),
        ("costmap_shared", C.c_int32),
        ("size_x", C.c_int32),
        ("size_y", C.c_int32),
        ("costmap_origin", C.c_void_p),
        ("resolution", C.c_double),
        ("people_records", C.c_void_p),
        ("people_aux", C.c_void_p),
        ("order", C.c_void_p),
        ("T_scene", C.c_void_p),
        ("scene_params", C.c_void_p),
    ]


class SmpcProjectionBatch(C.Structure):
    c_name = "smpc_projection_batch"
    _fields_ = [
        ("B", C.c_int32),
        ("T", C.c_int32),
        ("N", C.c_int32),
        ("on_device", C.c_int32),
        ("max_time", C.c_float),
        ("time_step", C.c_float),
        ("init_people", C.c_void_p),
        ("robot_path", C.c_void_p),
        ("od_indexes", C.c_void_p),
        ("od_shared", C.c_int32),
        ("od_width", C.c_int32),
        ("od_height", C.c_int32),
        ("od_resolution", C.c_float),
        ("od_origin", C.c_void_p),
    ]


class SmpcPeopleBatch(C.Structure):
    c_name = "smpc_people_batch"
    _fields_ = [
        ("B", C.c_int32),
        ("Np", C.c_int32),
        ("N", C.c_int32),
        ("on_device", C.c_int32),
        ("people", C.c_void_p),
        ("count", C.c_void_p),
        ("robot_pose", C.c_void_p),
        ("fov_angle", C.c_double),
        ("costmap_origin", C.c_void_p),
        ("costmap_shared", C.c_int32),
        ("size_x", C.c_int32),
        ("size_y", C.c_int32),
        ("resolution", C.c_double),
    ]


class SmpcObstacleDistanceIn(C.Structure):
    c_name = "smpc_obstacle_distance_in"
    _fields_ = [
        ("B", C.c_int32),
        ("size_x", C.c_int32),
        ("size_y", C.c_int32),
        ("on_device", C.c_int32),
        ("costmap", C.c_void_p),
        ("costmap_shared", C.c_int32),
        ("obstacle_min_cost", C.c_uint8),
        ("unknown_is_obstacle", C.c_uint8),
        ("reserved", C.c_uint8 * 2),
        ("resolution", C.c_double),
    ]


class SmpcObstacleDistanceOut(C.Structure):
    c_name = "smpc_obstacle_distance_out"
    _fields_ = [
        ("indexes", C.c_void_p),
        ("distances", C.c_void_p),
        ("n_obstacles", C.c_void_p),
    ]


class SmpcMemoryBatch(C.Structure):
    c_name = "smpc_memory_batch"
    _fields_ = [
        ("prev_path", C.c_void_p),
        ("prev_cmds", C.c_void_p),
        ("valid", C.c_void_p),
        ("length", C.c_void_p),
    ]


class SmpcFormatBatch(C.Structure):
    c_name = "smpc_format_batch"
    _fields_ = [
        ("B", C.c_int32),
        ("T", C.c_int32),
        ("path_rows", C.c_int32),
        ("on_device", C.c_int32),
        ("time_step", C.c_float),
        ("current_path_w", C.c_float),
        ("current_cmds_w", C.c_float),
        ("path", C.c_void_p),
        ("cmds", C.c_void_p),
        ("speed", C.c_void_p),
        ("memory", SmpcMemoryBatch),
        ("n_poses", C.c_void_p),
        ("max_poses", C.c_int32),
    ]


class SmpcFormatOut(C.Structure):
    c_name = "smpc_format_out"
    _fields_ = [
        ("robot_status", C.c_void_p),
        ("pose0", C.c_void_p),
        ("init_params", C.c_void_p),
        ("path_pts", C.c_void_p),
        ("goal_yaw", C.c_void_p),
        ("T_scene", C.c_void_p),
    ]


class SmpcTrajectorizeBatch(C.Structure):
    c_name = "smpc_trajectorize_batch"
    _fields_ = [
        ("B", C.c_int32),
        ("L", C.c_int32),
        ("max_steps", C.c_int32),
        ("on_device", C.c_int32),
        ("omnidirectional", C.c_int32),
        ("desired_linear_vel", C.c_double),
        ("lookahead_dist", C.c_double),
        ("max_angular_vel", C.c_double),
        ("time_step", C.c_double),
        ("plan", C.c_void_p),
        ("plan_len", C.c_void_p),
        ("robot_pose", C.c_void_p),
    ]


class SmpcPlanWindowBatch(C.Structure):
    c_name = "smpc_plan_window_batch"
    _fields_ = [
        ("B", C.c_int32),
        ("L", C.c_int32),
        ("on_device", C.c_int32),
        ("reserved", C.c_int32),
        ("max_robot_pose_search_dist", C.c_double),
        ("dist_threshold", C.c_double),
        ("plan", C.c_void_p),
        ("plan_len", C.c_void_p),
        ("plan_start", C.c_void_p),
        ("robot_pose", C.c_void_p),
        ("to_local", C.c_void_p),
    ]


class SmpcTrajectorizeOut(C.Structure):
    c_name = "smpc_trajectorize_out"
    _fields_ = [
        ("path", C.c_void_p),
        ("cmds", C.c_void_p),
        ("cmds_vy", C.c_void_p),
        ("n_poses", C.c_void_p),
        ("error", C.c_void_p),
    ]


class SmpcResultBatch(C.Structure):
    c_name = "smpc_result_batch"
    _fields_ = [
        ("params", C.c_void_p),
        ("cmds", C.c_void_p),
        ("path", C.c_void_p),
        ("status", C.c_void_p),
        ("reason", C.c_void_p),
        ("iterations", C.c_void_p),
        ("evaluations", C.c_void_p),
        ("initial_cost", C.c_void_p),
        ("final_cost", C.c_void_p),
    ]


SMPC_TRACE_COLS = 9


class SmpcTraceOut(C.Structure):
    c_name = "smpc_trace_out"
    _fields_ = [
        ("rows", C.c_void_p),
        ("max_rows", C.c_int32),
        ("n_rows", C.c_void_p),
    ]


SMPC_METRIC_COLS = 24


class SmpcMetricsBatch(C.Structure):
    c_name = "smpc_metrics_batch"
    _fields_ = [
        ("B", C.c_int32),
        ("Np", C.c_int32),
        ("on_device", C.c_int32),
        ("reserved", C.c_int32),
        ("dt", C.c_double),
        ("robot_pose", C.c_void_p),
        ("robot_twist", C.c_void_p),
        ("people", C.c_void_p),
        ("count", C.c_void_p),
        ("goal", C.c_void_p),
        ("goal_tolerance", C.c_double),
        ("robot_radius", C.c_double),
        ("person_radius", C.c_double),
        ("intimate_radius", C.c_double),
        ("personal_radius", C.c_double),
        ("social_radius", C.c_double),
        ("od_distances", C.c_void_p),
        ("od_shared", C.c_int32),
        ("od_width", C.c_int32),
        ("od_height", C.c_int32),
        ("od_resolution", C.c_float),
        ("od_origin", C.c_void_p),
        ("status", C.c_void_p),
        ("source", C.c_void_p),
    ]


SMPC_MAX_WAYPOINTS = 8


class SmpcCrowdBatch(C.Structure):
    c_name = "smpc_crowd_batch"
    _fields_ = [
        ("B", C.c_int32),
        ("Np", C.c_int32),
        ("K", C.c_int32),
        ("on_device", C.c_int32),
        ("cyclic", C.c_int32),
        ("robot_visible", C.c_int32),
        ("dt", C.c_double),
        ("goal_radius", C.c_double),
        ("person_radius", C.c_double),
        ("desired_speed", C.c_double),
        ("robot_pose", C.c_void_p),
        ("robot_twist", C.c_void_p),
        ("count", C.c_void_p),
        ("waypoints", C.c_void_p),
        ("n_waypoints", C.c_void_p),
        ("desired_speeds", C.c_void_p),
        ("od_indexes", C.c_void_p),
        ("od_shared", C.c_int32),
        ("od_width", C.c_int32),
        ("od_height", C.c_int32),
        ("od_resolution", C.c_float),
        ("od_origin", C.c_void_p),
    ]


class SmpcCrowdGroups(C.Structure):
    c_name = "smpc_crowd_groups"
    _fields_ = [
        ("group_id", C.c_void_p),
        ("factor_gaze", C.c_double),
        ("factor_coherence", C.c_double),
        ("factor_repulsion", C.c_double),
    ]


class SmpcEvalOut(C.Structure):
    c_name = "smpc_eval_batch_out"
    _fields_ = [
        ("residuals", C.c_void_p),
        ("jacobian", C.c_void_p),
        ("cost", C.c_void_p),
        ("gradient", C.c_void_p),
        ("row_order", C.c_int32),
    ]


def _p(struct):
    return C.POINTER(struct)


_h, _vp, _i32 = C.c_void_p, C.c_void_p, C.c_int32  # the handle, a buffer, an int32_t argument

# Every function include/smpc.h declares: name -> (restype, argtypes). solver.load_library() binds the library from
# this table; tests/test_abi.py holds it against the header and the built library.
FUNCTIONS = {
    "smpc_params_default": (None, [_p(SmpcParams)]),
    "smpc_dims": (C.c_int, [_p(SmpcParams), C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 6),
    "smpc_create": (_h, [_p(SmpcParams), C.c_int]),
    "smpc_destroy": (None, [_h]),
    "smpc_set_stream": (C.c_int, [_h, _vp]),
    "smpc_set_solve_share": (C.c_int, [_h, _i32]),
    "smpc_solve_slot_width": (C.c_int, [_h, _i32, _i32, _i32]),
    "smpc_solve_batch": (C.c_int, [_h, _p(SmpcSceneBatch), _p(SmpcResultBatch)]),
    "smpc_solve_trace_batch": (C.c_int, [_h, _p(SmpcSceneBatch), _p(SmpcResultBatch), _p(SmpcTraceOut)]),
    "smpc_eval_batch": (C.c_int, [_h, _p(SmpcSceneBatch), _vp, _p(SmpcEvalOut)]),
    "smpc_project_people_batch": (C.c_int, [_h, _p(SmpcProjectionBatch), _vp, _vp]),
    "smpc_people_to_status_batch": (C.c_int, [_h, _p(SmpcPeopleBatch), _vp, _vp]),
    "smpc_obstacle_distance_batch": (C.c_int, [_h, _p(SmpcObstacleDistanceIn), _p(SmpcObstacleDistanceOut)]),
    "smpc_format_to_optimize_batch": (C.c_int, [_h, _p(SmpcFormatBatch), _p(SmpcFormatOut)]),
    "smpc_memory_store_batch": (C.c_int, [_h, _i32, _i32, _i32, _vp, _vp, _vp, _p(SmpcMemoryBatch), _vp]),
    "smpc_trajectorize_path_batch": (C.c_int, [_h, _p(SmpcTrajectorizeBatch), _p(SmpcTrajectorizeOut)]),
    "smpc_transform_global_plan_batch": (C.c_int, [_h, _p(SmpcPlanWindowBatch), _vp, _vp, _vp]),
    "smpc_select_command_batch": (C.c_int, [_h, _i32, _i32, _i32, _i32] + [_vp] * 7),
    "smpc_episode_metrics_batch": (C.c_int, [_h, _p(SmpcMetricsBatch), _vp]),
    "smpc_crowd_step_batch": (C.c_int, [_h, _p(SmpcCrowdBatch), _vp, _vp]),
    "smpc_crowd_step_groups_batch": (C.c_int, [_h, _p(SmpcCrowdBatch), _p(SmpcCrowdGroups), _vp, _vp]),
    "smpc_math_probe": (C.c_int, [_h, _i32, _i32] + [_vp] * 4),
    "smpc_fp64_peak_probe": (C.c_double, [_h, _i32]),
    "smpc_stage_people_batch": (C.c_int, [_h, _p(SmpcSceneBatch), _vp, _vp]),
    "smpc_last_kernel_ms": (C.c_double, [_h]),
    "smpc_last_error": (C.c_char_p, []),
    "smpc_abi_version": (C.c_int, []),
}
EXPORTED_SYMBOLS = list(FUNCTIONS)

# The functions include/smpc_fixed_shapes.h declares, bound by solver.load_library() like the table above.
FIXED_SHAPE_FUNCTIONS = {
    "smpc_set_fixed_shapes": (C.c_int, [_h, _i32]),
    "smpc_solve_shape_is_fixed": (C.c_int, [_h, _i32, _i32, _i32]),
    "smpc_eval_shape_is_fixed": (C.c_int, [_h, _i32, _i32]),
}
