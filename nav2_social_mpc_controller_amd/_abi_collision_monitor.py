"""ctypes mirror of include/smpc_collision_monitor.h (the collision monitor: scan-based stop, slowdown, limit and approach
zones between the selected command and the base), beside `_abi.py` as that header stands beside include/smpc.h: the structs
(`c_name`: their C types) and FUNCTIONS, bound by solver.load_library() like `_abi`'s tables.
tests/test_collision_monitor.py compiles a probe against the header and compares sizeof and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp

SMPC_MONITOR_MAX_ZONES = 8
SMPC_MONITOR_MAX_VERTICES = 16
SMPC_MONITOR_MAX_STEPS = 32

SMPC_MONITOR_CIRCLE = 0
SMPC_MONITOR_POLYGON = 1

SMPC_MONITOR_STOP = 0
SMPC_MONITOR_SLOWDOWN = 1
SMPC_MONITOR_LIMIT = 2
SMPC_MONITOR_APPROACH = 3

SMPC_MONITOR_BY_STOP = 1
SMPC_MONITOR_BY_SLOWDOWN = 2
SMPC_MONITOR_BY_LIMIT = 4
SMPC_MONITOR_BY_APPROACH = 8
SMPC_MONITOR_BAD_INPUT = 16
SMPC_MONITOR_NO_CELL = 32


class SmpcMonitorZone(C.Structure):
    c_name = "smpc_monitor_zone"
    _fields_ = [
        ("shape", C.c_int32),
        ("action", C.c_int32),
        ("n_vertices", C.c_int32),
        ("min_points", C.c_int32),
        ("radius", C.c_double),
        ("slowdown_ratio", C.c_double),
        ("linear_limit", C.c_double),
        ("angular_limit", C.c_double),
        ("vertices", (C.c_double * 2) * SMPC_MONITOR_MAX_VERTICES),
    ]


class SmpcCollisionMonitorIn(C.Structure):
    c_name = "smpc_collision_monitor_in"
    _fields_ = [
        ("B", C.c_int32),
        ("n_beams", C.c_int32),
        ("Z", C.c_int32),
        ("M", C.c_int32),
        ("on_device", C.c_int32),
        ("reserved", C.c_int32),
        ("sim_dt", C.c_double),
        ("resolution", C.c_double),
        ("world_origin", C.c_double * 2),
        ("zones", C.c_void_p),
        ("robot_pose", C.c_void_p),
        ("cmd", C.c_void_p),
        ("beam_kind", C.c_void_p),
        ("beam_cell", C.c_void_p),
    ]


STRUCTS = [SmpcMonitorZone, SmpcCollisionMonitorIn]

FUNCTIONS = {
    "smpc_collision_monitor_batch": (C.c_int, [_h, _p(SmpcCollisionMonitorIn), _vp, _vp, _vp, _vp, _vp, _vp]),
}
