"""ctypes mirror of include/smpc_obstacle_memory.h (sensed local costmaps with memory: marks persist until a beam clears
them), beside `_abi_sensed_costmap.py` as that header stands beside include/smpc_sensed_costmap.h: the struct (`c_name`:
its C type, with the memoryless call's struct as its first member) and FUNCTIONS, bound by solver.load_library() like
`_abi`'s tables. tests/test_obstacle_memory.py compiles a probe against the header and compares sizeof and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp
from ._abi_sensed_costmap import SmpcSensedCostmapIn


class SmpcObstacleMemoryIn(C.Structure):
    c_name = "smpc_obstacle_memory_in"
    _fields_ = [
        ("scan", SmpcSensedCostmapIn),
        ("mark_d2", C.c_int32),
        ("footprint_d2", C.c_int32),
    ]


STRUCTS = [SmpcObstacleMemoryIn]

FUNCTIONS = {
    "smpc_obstacle_memory_batch": (C.c_int, [_h, _p(SmpcObstacleMemoryIn), _vp, _vp, _vp, _vp, _vp]),
}
