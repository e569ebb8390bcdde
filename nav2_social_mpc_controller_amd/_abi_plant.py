"""ctypes mirror of include/smpc_plant.h (the robot plant: commands executed under limits, stopped by contact), beside
`_abi.py` as that header stands beside include/smpc.h: the struct (`c_name`: its C type) and FUNCTIONS, bound by
solver.load_library() like `_abi`'s tables. tests/test_plant.py compiles a probe against the header and compares sizeof
and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp

SMPC_PLANT_MAX_SUBSTEPS = 16
SMPC_PLANT_MAX_LATENCY = 8
SMPC_PLANT_MAX_FOOTPRINT_D2 = 225

SMPC_PLANT_BLOCKED_BY_WALL = 1
SMPC_PLANT_BLOCKED_BY_AGENT = 2
SMPC_PLANT_WALL_CONTACT = 4
SMPC_PLANT_AGENT_CONTACT = 8
SMPC_PLANT_BAD_COMMAND = 16
SMPC_PLANT_BAD_STATE = 32


class SmpcPlantIn(C.Structure):
    c_name = "smpc_plant_in"
    _fields_ = [
        ("B", C.c_int32),
        ("Np", C.c_int32),
        ("S", C.c_int32),
        ("L", C.c_int32),
        ("on_device", C.c_int32),
        ("Hx", C.c_int32),
        ("Hy", C.c_int32),
        ("footprint_d2", C.c_int32),
        ("wall_min_cost", C.c_int32),
        ("unknown_is_wall", C.c_int32),
        ("outside_is_wall", C.c_int32),
        ("reserved", C.c_int32),
        ("dt", C.c_double),
        ("v_min", C.c_double),
        ("v_max", C.c_double),
        ("w_max", C.c_double),
        ("dv_up", C.c_double),
        ("dv_down", C.c_double),
        ("dw", C.c_double),
        ("contact_dist", C.c_double),
        ("resolution", C.c_double),
        ("world_origin", C.c_double * 2),
        ("world", C.c_void_p),
        ("cmd", C.c_void_p),
        ("agents", C.c_void_p),
        ("count", C.c_void_p),
    ]


STRUCTS = [SmpcPlantIn]

FUNCTIONS = {
    "smpc_robot_plant_batch": (C.c_int, [_h, _p(SmpcPlantIn), _vp, _vp, _vp, _vp, _vp, _vp]),
}
