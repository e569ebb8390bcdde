"""ctypes mirror of include/smpc_sensed_costmap.h (sensed local costmaps: a scan marks walls and agents, then inflation),
beside `_abi.py` as that header stands beside include/smpc.h: the struct (`c_name`: its C type), the limits and FUNCTIONS,
bound by solver.load_library() like `_abi`'s tables. tests/test_sensed_costmap.py compiles a probe against the header and
compares sizeof, every offsetof, the limits and the enum."""
import ctypes as C

from ._abi import _h, _p, _vp

# enum smpc_beam_kind
BEAM_KINDS = ["NONE", "WORLD", "AGENT", "CORNER_PAIR", "INVALID", "NO_ROBOT"]
# SMPC_SENSED_*
LIMITS = {"MAX_REACH": 127, "MAX_SIZE": 256, "MAX_D2": 1024, "MAX_BEAMS": 4096}


class SmpcSensedCostmapIn(C.Structure):
    c_name = "smpc_sensed_costmap_in"
    _fields_ = [
        ("B", C.c_int32),
        ("Np", C.c_int32),
        ("on_device", C.c_int32),
        ("size_x", C.c_int32),
        ("size_y", C.c_int32),
        ("world_x", C.c_int32),
        ("world_y", C.c_int32),
        ("world_shared", C.c_int32),
        ("n_beams", C.c_int32),
        ("agent_d2", C.c_int32),
        ("d2_max", C.c_int32),
        ("occlusion_min_cost", C.c_uint8),
        ("unknown_occludes", C.c_uint8),
        ("base", C.c_uint8),
        ("outside_cost", C.c_uint8),
        ("resolution", C.c_double),
        ("world", C.c_void_p),
        ("world_origin", C.c_void_p),
        ("robot_pose", C.c_void_p),
        ("people", C.c_void_p),
        ("count", C.c_void_p),
        ("cell", C.c_void_p),
        ("beam_cells", C.c_void_p),
        ("inflation_cost", C.c_void_p),
    ]


STRUCTS = [SmpcSensedCostmapIn]

FUNCTIONS = {
    "smpc_sensed_costmap_batch": (C.c_int, [_h, _p(SmpcSensedCostmapIn), _vp, _vp, _vp]),
}
