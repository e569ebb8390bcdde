"""ctypes mirror of include/smpc_local_costmap.h (the rolling local costmaps), beside `_abi.py` as that header stands
beside include/smpc.h: the struct (`c_name`: its C type) and FUNCTIONS, bound by solver.load_library() like `_abi`'s
tables. tests/test_local_costmap.py compiles a probe against the header and compares sizeof and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp


class SmpcLocalCostmapIn(C.Structure):
    c_name = "smpc_local_costmap_in"
    _fields_ = [
        ("B", C.c_int32),
        ("on_device", C.c_int32),
        ("size_x", C.c_int32),
        ("size_y", C.c_int32),
        ("world_x", C.c_int32),
        ("world_y", C.c_int32),
        ("world_shared", C.c_int32),
        ("outside_cost", C.c_uint8),
        ("force", C.c_uint8),
        ("reserved", C.c_uint8 * 2),
        ("resolution", C.c_double),
        ("world", C.c_void_p),
        ("world_origin", C.c_void_p),
        ("pose", C.c_void_p),
    ]


FUNCTIONS = {
    "smpc_local_costmap_batch": (C.c_int, [_h, _p(SmpcLocalCostmapIn), _vp, _vp, _vp, _vp]),
}
