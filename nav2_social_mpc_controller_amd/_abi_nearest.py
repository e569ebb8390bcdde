"""ctypes mirror of include/smpc_nearest.h (the nearest-agent gather of a shared world), beside `_abi.py` as that header
stands beside include/smpc.h: the struct (`c_name`: its C type) and FUNCTIONS, bound by solver.load_library() like `_abi`'s
tables. tests/test_nearest.py compiles a probe against the header and compares sizeof and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp

SMPC_NEAREST_BIN_MARGIN = 1.0 + 2.0 ** -20
SMPC_NEAREST_MAX_BINS = 65536
SMPC_NEAREST_MAX_ROWS = 2 ** 24


class SmpcNearestIn(C.Structure):
    c_name = "smpc_nearest_in"
    _fields_ = [
        ("B", C.c_int32),
        ("Np", C.c_int32),
        ("A", C.c_int32),
        ("on_device", C.c_int32),
        ("grid_x", C.c_int32),
        ("grid_y", C.c_int32),
        ("grid_origin", C.c_double * 2),
        ("bin_size", C.c_double),
        ("max_range", C.c_double),
        ("agents", C.c_void_p),
        ("robot_pose", C.c_void_p),
        ("self", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
    ]


STRUCTS = [SmpcNearestIn]

FUNCTIONS = {
    "smpc_nearest_workspace_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int32]),
    "smpc_nearest_people_batch": (C.c_int, [_h, _p(SmpcNearestIn), _vp, _vp, _vp]),
}
