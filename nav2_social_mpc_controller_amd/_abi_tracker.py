"""ctypes mirror of include/smpc_tracker.h (people tracks: a per-robot tracker between detection and people_to_status),
beside `_abi.py` as that header stands beside include/smpc.h: the struct (`c_name`: its C type) and FUNCTIONS, bound by
solver.load_library() like `_abi`'s tables. tests/test_tracker.py compiles a probe against the header and compares sizeof
and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp

SMPC_TRACK_FREE = 0
SMPC_TRACK_TENTATIVE = 1
SMPC_TRACK_CONFIRMED = 2


class SmpcTrackerIn(C.Structure):
    c_name = "smpc_tracker_in"
    _fields_ = [
        ("B", C.c_int32),
        ("Nd", C.c_int32),
        ("Nt", C.c_int32),
        ("Np", C.c_int32),
        ("on_device", C.c_int32),
        ("confirm_hits", C.c_int32),
        ("max_missed", C.c_int32),
        ("reserved", C.c_int32),
        ("dt", C.c_double),
        ("alpha", C.c_double),
        ("gain", C.c_double),
        ("gate", C.c_double),
        ("detections", C.c_void_p),
        ("det_count", C.c_void_p),
        ("robot_pose", C.c_void_p),
    ]


STRUCTS = [SmpcTrackerIn]

FUNCTIONS = {
    "smpc_track_people_batch": (C.c_int, [_h, _p(SmpcTrackerIn), _vp, _vp, _vp, _vp, _vp, _vp]),
}
