"""ctypes mirror of include/smpc_scan_people.h (people detections from the scan: the tick's beam hits clustered into
person-sized segments, between the sensed costmap and the tracker), beside `_abi.py` as that header stands beside
include/smpc.h: the struct (`c_name`: its C type) and FUNCTIONS, bound by solver.load_library() like `_abi`'s tables.
tests/test_scan_people.py compiles a probe against the header and compares sizeof and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp

SMPC_SCAN_PEOPLE_MAX_BEAMS = 4096     # SMPC_SENSED_MAX_BEAMS
SMPC_SCAN_PEOPLE_MAX_ROWS = 64        # SMPC_MAX_AGENTS


class SmpcScanPeopleIn(C.Structure):
    c_name = "smpc_scan_people_in"
    _fields_ = [
        ("B", C.c_int32),
        ("n_beams", C.c_int32),
        ("Nd", C.c_int32),
        ("on_device", C.c_int32),
        ("subtract_map", C.c_int32),
        ("min_points", C.c_int32),
        ("link_d2", C.c_int32),
        ("width_d2_min", C.c_int32),
        ("width_d2_max", C.c_int32),
        ("range_d2", C.c_int32),
        ("resolution", C.c_double),
        ("world_origin", C.c_double * 2),
        ("body_offset", C.c_double),
        ("robot_pose", C.c_void_p),
        ("beam_kind", C.c_void_p),
        ("beam_cell", C.c_void_p),
    ]


STRUCTS = [SmpcScanPeopleIn]

FUNCTIONS = {
    "smpc_scan_people_batch": (C.c_int, [_h, _p(SmpcScanPeopleIn), _vp, _vp, _vp, _vp]),
}
