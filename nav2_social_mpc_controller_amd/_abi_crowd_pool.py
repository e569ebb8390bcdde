"""ctypes mirror of include/smpc_crowd_pool.h (the reactive Social-Force step of a shared world's pedestrians), beside
`_abi.py` as that header stands beside include/smpc.h: the struct (`c_name`: its C type) and FUNCTIONS, bound by
solver.load_library() like `_abi`'s tables. tests/test_crowd_pool.py compiles a probe against the header and compares
sizeof and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp

SMPC_CROWD_POOL_FRACTION_BITS = 36
SMPC_CROWD_POOL_TERM_CLAMP = 8.0


class SmpcCrowdPoolIn(C.Structure):
    c_name = "smpc_crowd_pool_in"
    _fields_ = [
        ("M", C.c_int32),
        ("A", C.c_int32),
        ("K", C.c_int32),
        ("on_device", C.c_int32),
        ("cyclic", C.c_int32),
        ("bins_ready", C.c_int32),
        ("grid_x", C.c_int32),
        ("grid_y", C.c_int32),
        ("grid_origin", C.c_double * 2),
        ("bin_size", C.c_double),
        ("interaction_range", C.c_double),
        ("dt", C.c_double),
        ("goal_radius", C.c_double),
        ("person_radius", C.c_double),
        ("desired_speed", C.c_double),
        ("agents", C.c_void_p),
        ("waypoints", C.c_void_p),
        ("n_waypoints", C.c_void_p),
        ("desired_speeds", C.c_void_p),
        ("od_indexes", C.c_void_p),
        ("od_origin", C.c_void_p),
        ("od_width", C.c_int32),
        ("od_height", C.c_int32),
        ("od_resolution", C.c_float),
        ("reserved0", C.c_int32),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
    ]


STRUCTS = [SmpcCrowdPoolIn]

FUNCTIONS = {
    "smpc_crowd_pool_step_batch": (C.c_int, [_h, _p(SmpcCrowdPoolIn), _vp, _vp]),
}
