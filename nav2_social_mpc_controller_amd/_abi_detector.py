"""ctypes mirror of include/smpc_detector.h (people detections: a detector model between the line-of-sight filter and the
tracker), beside `_abi.py` as that header stands beside include/smpc.h: the struct (`c_name`: its C type) and FUNCTIONS,
bound by solver.load_library() like `_abi`'s tables. tests/test_detector.py compiles a probe against the header and
compares sizeof and every offsetof."""
import ctypes as C

from ._abi import _h, _p, _vp

SMPC_DETECT_DETECTED = 0
SMPC_DETECT_BODY_OCCLUDED = 1
SMPC_DETECT_MISSED = 2
SMPC_DETECT_NOT_FINITE = 3


class SmpcDetectorIn(C.Structure):
    c_name = "smpc_detector_in"
    _fields_ = [
        ("B", C.c_int32),
        ("Np", C.c_int32),
        ("Nd", C.c_int32),
        ("Kc", C.c_int32),
        ("on_device", C.c_int32),
        ("reserved", C.c_int32),
        ("seed_lo", C.c_uint32),
        ("seed_hi", C.c_uint32),
        ("miss_threshold", C.c_uint32),
        ("clutter_threshold", C.c_uint32),
        ("body_radius", C.c_double),
        ("noise_scale", C.c_double),
        ("noise_growth", C.c_double),
        ("clutter_scale", C.c_double),
        ("people", C.c_void_p),
        ("count", C.c_void_p),
        ("robot_pose", C.c_void_p),
    ]


STRUCTS = [SmpcDetectorIn]

FUNCTIONS = {
    "smpc_detect_people_batch": (C.c_int, [_h, _p(SmpcDetectorIn), _vp, _vp, _vp, _vp, _vp]),
}
