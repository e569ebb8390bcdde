"""ctypes mirror of include/smpc_global_plan.h (goal fields and plan extraction on a world map), beside `_abi.py` as that
header stands beside include/smpc.h: the structs (`c_name`: their C types) and FUNCTIONS, bound by solver.load_library()
like `_abi`'s tables. tests/test_global_plan.py compiles a probe against the header and compares sizeof and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp

SMPC_FIELD_UNREACHABLE = 0xFFFFFFFF
# enum smpc_plan_error
PLAN_ERRORS = ["OK", "START_OUTSIDE", "START_BLOCKED", "UNREACHABLE", "TRUNCATED", "BAD_GOAL_INDEX", "INCONSISTENT_FIELD"]


class SmpcPlanCostParams(C.Structure):
    c_name = "smpc_plan_cost_params"
    _fields_ = [
        ("neutral_cost", C.c_int32),
        ("cost_weight", C.c_int32),
        ("lethal_min_cost", C.c_uint8),
        ("allow_unknown", C.c_uint8),
        ("reserved", C.c_uint8 * 6),
    ]


class SmpcGoalFieldIn(C.Structure):
    c_name = "smpc_goal_field_in"
    _fields_ = [
        ("G", C.c_int32),
        ("on_device", C.c_int32),
        ("world_x", C.c_int32),
        ("world_y", C.c_int32),
        ("world_shared", C.c_int32),
        ("reserved", C.c_int32),
        ("resolution", C.c_double),
        ("cost", SmpcPlanCostParams),
        ("world", C.c_void_p),
        ("world_origin", C.c_void_p),
        ("goal", C.c_void_p),
    ]


class SmpcExtractPlanIn(C.Structure):
    c_name = "smpc_extract_plan_in"
    _fields_ = [
        ("B", C.c_int32),
        ("G", C.c_int32),
        ("L", C.c_int32),
        ("stride", C.c_int32),
        ("on_device", C.c_int32),
        ("world_x", C.c_int32),
        ("world_y", C.c_int32),
        ("world_shared", C.c_int32),
        ("resolution", C.c_double),
        ("cost", SmpcPlanCostParams),
        ("world", C.c_void_p),
        ("world_origin", C.c_void_p),
        ("field", C.c_void_p),
        ("goal", C.c_void_p),
        ("robot_goal", C.c_void_p),
        ("pose", C.c_void_p),
    ]


STRUCTS = [SmpcPlanCostParams, SmpcGoalFieldIn, SmpcExtractPlanIn]

FUNCTIONS = {
    "smpc_goal_field_batch": (C.c_int, [_h, _p(SmpcGoalFieldIn), _vp, _vp]),
    "smpc_extract_plan_batch": (C.c_int, [_h, _p(SmpcExtractPlanIn), _vp, _vp, _vp]),
}
