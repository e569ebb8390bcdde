"""ctypes mirror of include/smpc_plan_smoother.h (plan smoothing: the global plans' grid paths relaxed before the controller
reads them, where the planner runs), beside `_abi.py` as that header stands beside include/smpc.h: the struct (`c_name`: its C
type), the limits, the status values and FUNCTIONS, bound by solver.load_library() like `_abi`'s tables.
tests/test_plan_smoother.py compiles a probe against the header and compares sizeof and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp

SMPC_SMOOTH_MAX_POSES = 1024
SMPC_SMOOTH_MAX_ITS = 100000
SMPC_SMOOTH_MAX_REFINEMENTS = 8

# enum smpc_smooth_status
SMOOTH_STATUS = ["CONVERGED", "REACHED_MAX_ITS", "TOO_SHORT", "BAD_PLAN"]
SMPC_SMOOTH_CONVERGED, SMPC_SMOOTH_REACHED_MAX_ITS, SMPC_SMOOTH_TOO_SHORT, SMPC_SMOOTH_BAD_PLAN = range(4)


class SmpcPlanSmootherIn(C.Structure):
    c_name = "smpc_plan_smoother_in"
    _fields_ = [
        ("B", C.c_int32),
        ("L", C.c_int32),
        ("on_device", C.c_int32),
        ("world_x", C.c_int32),
        ("world_y", C.c_int32),
        ("world_shared", C.c_int32),
        ("max_its", C.c_int32),
        ("refinement_num", C.c_int32),
        ("lethal_min_cost", C.c_int32),
        ("allow_unknown", C.c_int32),
        ("resolution", C.c_double),
        ("w_data", C.c_double),
        ("w_smooth", C.c_double),
        ("tolerance", C.c_double),
        ("world", C.c_void_p),
        ("world_origin", C.c_void_p),
        ("plan_len", C.c_void_p),
        ("range", C.c_void_p),
    ]


STRUCTS = [SmpcPlanSmootherIn]

FUNCTIONS = {
    "smpc_smooth_plan_batch": (C.c_int, [_h, _p(SmpcPlanSmootherIn), _vp, _vp, _vp, _vp]),
}
