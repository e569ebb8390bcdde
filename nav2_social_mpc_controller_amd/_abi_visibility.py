"""ctypes mirror of include/smpc_visibility.h (the line-of-sight filter of the people a robot perceives), beside `_abi.py` as
that header stands beside include/smpc.h: the struct (`c_name`: its C type) and FUNCTIONS, bound by solver.load_library()
like `_abi`'s tables. tests/test_visibility.py compiles a probe against the header and compares sizeof and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp

# enum smpc_seen_code
SEEN_CODES = ["HIDDEN", "SEEN", "OUT_OF_RANGE", "NOT_FINITE"]


class SmpcVisibilityIn(C.Structure):
    c_name = "smpc_visibility_in"
    _fields_ = [
        ("B", C.c_int32),
        ("Np", C.c_int32),
        ("on_device", C.c_int32),
        ("world_x", C.c_int32),
        ("world_y", C.c_int32),
        ("world_shared", C.c_int32),
        ("occlusion_min_cost", C.c_uint8),
        ("unknown_occludes", C.c_uint8),
        ("reserved", C.c_uint8 * 2),
        ("resolution", C.c_double),
        ("max_range", C.c_double),
        ("world", C.c_void_p),
        ("world_origin", C.c_void_p),
        ("robot_pose", C.c_void_p),
        ("people", C.c_void_p),
        ("count", C.c_void_p),
    ]


STRUCTS = [SmpcVisibilityIn]

FUNCTIONS = {
    "smpc_visible_people_batch": (C.c_int, [_h, _p(SmpcVisibilityIn), _vp, _vp, _vp]),
}
