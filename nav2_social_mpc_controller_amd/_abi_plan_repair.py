"""ctypes mirror of include/smpc_plan_repair.h (plan repair: detours around the impassable cells a robot's own window shows
on its plan, behind the tick's sensing stage), beside `_abi.py` as that header stands beside include/smpc.h: the struct
(`c_name`: its C type), the status values and FUNCTIONS, bound by solver.load_library() like `_abi`'s tables.
tests/test_plan_repair.py compiles a probe against the header and compares sizeof and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp
from ._abi_global_plan import SmpcPlanCostParams

SMPC_REPAIR_MAX_RADIUS = 63
SMPC_FIELD_UNREACHABLE = 0xFFFFFFFF

# enum smpc_repair_status
REPAIR_STATUS = ["CLEAR", "REPAIRED", "NO_PLAN", "NO_CELL", "NO_REJOIN", "UNREACHABLE", "TOO_LONG", "INCONSISTENT_FIELD"]
(SMPC_REPAIR_CLEAR, SMPC_REPAIR_REPAIRED, SMPC_REPAIR_NO_PLAN, SMPC_REPAIR_NO_CELL, SMPC_REPAIR_NO_REJOIN, SMPC_REPAIR_UNREACHABLE,
 SMPC_REPAIR_TOO_LONG, SMPC_REPAIR_INCONSISTENT_FIELD) = range(8)


class SmpcPlanRepairIn(C.Structure):
    c_name = "smpc_plan_repair_in"
    _fields_ = [
        ("B", C.c_int32),
        ("L", C.c_int32),
        ("on_device", C.c_int32),
        ("size_x", C.c_int32),
        ("size_y", C.c_int32),
        ("costmap_shared", C.c_int32),
        ("radius", C.c_int32),
        ("stride", C.c_int32),
        ("resolution", C.c_double),
        ("clearance_d2", C.c_double),
        ("cost", SmpcPlanCostParams),
        ("costmap", C.c_void_p),
        ("costmap_origin", C.c_void_p),
        ("robot_pose", C.c_void_p),
        ("plan_start", C.c_void_p),
    ]


STRUCTS = [SmpcPlanRepairIn]

FUNCTIONS = {
    "smpc_repair_plan_batch": (C.c_int, [_h, _p(SmpcPlanRepairIn), _vp, _vp, _vp, _vp, _vp, _vp]),
}
