"""The C-ABI library loads, exports every symbol include/smpc.h declares, and its struct layouts match the
ctypes mirror: every struct, every field, every constant. No compute calls (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from nav2_social_mpc_controller_amd import _abi
from nav2_social_mpc_controller_amd import solver as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc.h")


def _declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_header_and_python_symbol_lists_agree():
    assert _declared_functions() == sorted(_abi.EXPORTED_SYMBOLS)


def test_library_exports_every_declared_symbol():
    assert os.path.exists(S.LIB_PATH), "run __graft_entry__.build() first"
    out = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in _declared_functions():
        assert name in exported, f"{name} declared in include/smpc.h but not exported by libsmpc_hip.so"


def test_library_loads_and_reports_abi_version():
    lib = S.load_library()
    assert lib.smpc_abi_version() == _abi.SMPC_ABI_VERSION


def _structs():
    return [v for v in vars(_abi).values() if isinstance(v, type) and issubclass(v, C.Structure)]


def _header_struct_typedefs():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S))


def test_function_table_is_the_symbol_list_and_what_the_library_is_bound_with():
    assert _abi.EXPORTED_SYMBOLS == list(_abi.FUNCTIONS) and len(_abi.FUNCTIONS) == 27
    lib = S.load_library()
    for name, (restype, argtypes) in _abi.FUNCTIONS.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


CONSTANTS = ("SMPC_ABI_VERSION", "SMPC_MAX_BLOCKS", "SMPC_TRACE_COLS", "SMPC_METRIC_COLS", "SMPC_MAX_WAYPOINTS", "SMPC_MAX_AGENTS")


def test_every_struct_field_and_constant_matches_the_c_header(tmp_path):
    """Every struct of _abi against include/smpc.h: one C program prints sizeof and the offsetof of every field (and the
    header's constants and metric-column enumerators), and every value must be ctypes'. Every struct the header typedefs has
    a mirror (smpc_handle is opaque), under the C name the mirror states."""
    structs = _structs()
    assert sorted(st.c_name for st in structs) == _header_struct_typedefs() and len(structs) == 19
    probes = [(st, None) for st in structs] + [(st, f[0]) for st in structs for f in st._fields_]
    enumerators = ["SMPC_M_" + n.upper() for n in S.METRIC_COLS[:22]]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' if f is None else f'printf("%zu\\n", offsetof({st.c_name}, {f}));\n'
                   for st, f in probes)
    body += "".join(f'printf("%d\\n", (int){name});\n' for name in CONSTANTS + tuple(enumerators))
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc.h"\nint main(void){\n' + body + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert len(probes) == 19 + 217 and len(values) == len(probes) + len(CONSTANTS) + 22
    print(f"{len(probes)} sizeof/offsetof probes of {len(structs)} structs, {len(values) - len(probes)} constants")
    for (st, f), v in zip(probes, values):
        assert v == (C.sizeof(st) if f is None else getattr(st, f).offset), (st.c_name, f)
    consts = values[len(probes):]
    assert consts[:len(CONSTANTS)] == [getattr(_abi, name) for name in CONSTANTS] == [6, 10, 9, 24, 8, 64]
    # enum smpc_metric_col: a column's enumerator is its index in solver.METRIC_COLS (the last two columns are reserved)
    assert consts[len(CONSTANTS):] == list(range(22))
    # the literal sizes of the structs that were added beside unchanged ones, and the order inside them
    size = {st.c_name: C.sizeof(st) for st in structs}
    assert size["smpc_crowd_batch"] == 136 and size["smpc_crowd_groups"] == 32 and size["smpc_scene_params"] == 14 * 8
    assert [getattr(_abi.SmpcCrowdGroups, f).offset for f, _ in _abi.SmpcCrowdGroups._fields_] == [0, 8, 16, 24]
    assert [f for f, _ in _abi.SmpcCrowdGroups._fields_] == ["group_id", "factor_gaze", "factor_coherence", "factor_repulsion"]
    assert _abi.SmpcSceneBatch._fields_[-1][0] == "scene_params"  # appended: every earlier offset is unchanged
    assert [f for f, _ in _abi.SmpcSceneParams._fields_] == list(_abi.SCENE_PARAM_FIELDS)


def test_params_default_matches_reference_code_defaults():
    lib = S.load_library()
    p = _abi.SmpcParams()
    lib.smpc_params_default(C.byref(p))
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    q = OptimizerParams().to_c()
    for name, _ in _abi.SmpcParams._fields_:
        assert getattr(p, name) == getattr(q, name), name


def test_dims_follow_the_reference_rules():
    lib = S.load_library()
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    cases = [(OptimizerParams.readme(), 28, (18, 6, 3, 6, 226, 3)),          # H18/bl6, T=28: P=6, M=226
             (OptimizerParams.params_yaml(), 38, (20, 4, 5, 10, 308, 5)),    # params.yaml: P=10, M=308
             (OptimizerParams.params_yaml().replace(control_horizon=18), 38, (18, 4, 5, 10, 307, 4)),
             (OptimizerParams.readme().replace(time_step=0.1), 13, (13, 6, 3, 6, 105, 2))]  # bl does not divide CH
    for prm, T, want in cases:
        vals = [C.c_int() for _ in range(6)]
        cp = prm.to_c()
        rc = lib.smpc_dims(C.byref(cp), T, 1, *[C.byref(v) for v in vals])
        assert rc == 0
        assert tuple(v.value for v in vals) == want
        assert prm.dims(T, True) == want


def test_invalid_solver_type_is_rejected_like_the_reference():
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    with pytest.raises(RuntimeError, match="linear_solver_type"):
        OptimizerParams(linear_solver_type="NOT_A_SOLVER")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU failure mode")
def test_create_fails_loudly_without_a_gpu():
    """No CPU fallback behind the ABI: creating a solver on a box without a HIP device must raise."""
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    with pytest.raises(S.SmpcError, match="no HIP device|hip"):
        S.BatchSolver(OptimizerParams.readme())


def test_block_limit_matches_the_header():
    """smpc_dims reports nb for any shape; the header's SMPC_MAX_BLOCKS is what the library instantiates (nb 1..10)."""
    lib = S.load_library()
    src = open(HEADER).read()
    assert int(re.search(r"#define SMPC_MAX_BLOCKS (\d+)", src).group(1)) == 10
    p = _abi.SmpcParams()
    lib.smpc_params_default(C.byref(p))
    nb = C.c_int()
    p.control_horizon, p.parameter_block_length = 33, 3
    assert lib.smpc_dims(C.byref(p), 40, 1, None, None, C.byref(nb), None, None, None) == 0 and nb.value == 11
    hip_src = open(os.path.join(ROOT, "nav2_social_mpc_controller_amd", "csrc", "smpc_sweep_host.hpp")).read()
    assert "case 10: return pick_w<10>" in hip_src and "case 11" not in hip_src


def test_absurd_iteration_caps_are_refused_before_anything_is_launched():
    """A persistent wave runs until its scenes stop: smpc_create refuses max_iterations outside 0 .. 100000 (the check
    comes before the device query, so it is visible on a box without a GPU too)."""
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    src = open(HEADER).read()
    cap = int(re.search(r"#define SMPC_MAX_LM_ITERATIONS (\d+)", src).group(1))
    assert cap == 100000
    for bad in (-1, cap + 1, 2 ** 31 - 1):
        with pytest.raises(S.SmpcError, match="max_iterations"):
            S.BatchSolver(OptimizerParams.readme().replace(max_iterations=bad))
