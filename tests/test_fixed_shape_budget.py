"""The fixed-shape kernels of the headline configuration (csrc/smpc_launch.hpp, SMPC_FIXED_SHAPES), checked at compile
time (CPU only, ~20 s): their register budget, the kernel names other tests pin, and the rule that picks a shape.

Like test_kernel_budget.py this compiles the NB = 3 instantiations with the flags of `csrc/build.sh` and reads the
compiler's kernel-resource-usage remarks. The picker rule is the constexpr function `plan_sweep()` of smpc_plan.hpp
dispatches through (`smpc::fixed_shape_index`), called from a small host program: `smpc_solve_shape_is_fixed` itself
needs a handle, and a handle needs a device. The functions of include/smpc_fixed_shapes.h stand outside the table
tests/test_abi.py holds against include/smpc.h, so their declaration, export and binding are checked here."""
import os
import re
import subprocess

import pytest

from nav2_social_mpc_controller_amd.params import OptimizerParams
from test_kernel_budget import CSRC, HIPCC, MAX_VGPRS, parse_resource_remarks

SHAPE = "NS_10FixedShapeILi28ELi8ELi18ELi6EEE"   # smpc::FixedShape<28, 8, 18, 6>: T, N, CH, bl of the headline workload
FIXED = {
    "solve_fixed<28,8,18,6>": f"_ZN4smpc23smpc_solve_fixed_kernelI{SHAPE}EEvNS_7KParamsE",
    "K1_fixed<28,8,18,6>": f"_ZN4smpc22smpc_eval_fixed_kernelI{SHAPE}EEvNS_7KParamsE",
}
# what test_kernel_budget.py, test_scene_params.py and test_trace_host.py look up by name: the run-time-shape kernels
PINNED = [
    "_ZN4smpc17smpc_solve_kernelILi3ELi32ELb0ELb0ELb0EEEvNS_7KParamsE",
    "_ZN4smpc16smpc_eval_kernelILi3ELi32ELb0ELb0EEEvNS_7KParamsE",
    "_ZN4smpc17smpc_solve_kernelILi3ELi32ELb1ELb0ELb0EEEvNS_7KParamsE",
    "_ZN4smpc17smpc_solve_kernelILi3ELi32ELb1ELb1ELb0EEEvNS_7KParamsE",
    "_ZN4smpc16smpc_eval_kernelILi3ELi32ELb1ELb1EEEvNS_7KParamsE",
    "_ZN4smpc16smpc_eval_kernelILi3ELi64ELb1ELb1EEEvNS_7KParamsE",
    "_ZN4smpc17smpc_solve_kernelILi3ELi32ELb1ELb1ELb1EEEvNS_7KParamsE",
    "_ZN4smpc17smpc_solve_kernelILi3ELi64ELb1ELb1ELb1EEEvNS_7KParamsE",
]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    obj = str(tmp_path_factory.mktemp("fixed_budget") / "smpc_nb3.o")
    r = subprocess.run(["bash", os.path.join(CSRC, "build.sh"), "-DSMPC_ONLY_NB=3", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage"],
                       env={**os.environ, "SMPC_OUT": obj}, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return parse_resource_remarks(r.stderr)


@pytest.mark.parametrize("name", sorted(FIXED))
def test_fixed_shape_kernel_fits_three_waves_without_spills(usage, name):
    r = usage.get(FIXED[name])
    assert r is not None, f"{name}: no resource remark (instantiation missing?)"
    print(name, {f: r[f] for f in ("VGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")})
    assert r["VGPRs"] <= MAX_VGPRS, f"{name}: {r['VGPRs']} VGPRs > {MAX_VGPRS} (fewer than three waves per SIMD)"
    assert r["VGPRs Spill"] == 0, f"{name}: {r['VGPRs Spill']} spilled VGPRs"
    assert r["SGPRs Spill"] == 0, f"{name}: {r['SGPRs Spill']} spilled SGPRs"
    assert r["ScratchSize [bytes/lane]"] == 0, f"{name}: {r['ScratchSize [bytes/lane]']} B/lane private segment"
    assert r["Occupancy [waves/SIMD]"] >= 3, f"{name}: occupancy {r['Occupancy [waves/SIMD]']}"


def test_the_kernels_other_tests_pin_by_name_are_still_compiled(usage):
    missing = [n for n in PINNED if n not in usage]
    assert not missing, missing


def test_fixed_solve_kernel_needs_no_more_scalar_registers_than_the_run_time_shape_kernel(usage):
    """The point of the constants: T, N, CH, bl and the LDS offsets take no scalar registers."""
    fixed, plain = usage[FIXED["solve_fixed<28,8,18,6>"]], usage[PINNED[0]]
    assert fixed["TotalSGPRs"] <= plain["TotalSGPRs"], (fixed["TotalSGPRs"], plain["TotalSGPRs"])


PROBE = r"""
#include <cstdio>
#include "smpc_launch.hpp"
int main() {
  using S = smpc::FixedShape<28, 8, 18, 6>;
  std::printf("%d %d %d %d\n", S::kNB, S::kW, S::kNfeas, S::kNbounded);
  const int q[][4] = {{28, 8, 18, 6}, {28, 7, 18, 6}, {28, 9, 18, 6}, {27, 8, 18, 6}, {29, 8, 18, 6},
                      {28, 8, 17, 6}, {28, 8, 18, 5}, {28, 0, 18, 6}, {38, 8, 20, 4}};
  for (const auto& s : q) std::printf("%d\n", smpc::fixed_shape_index(s[0], s[1], s[2], s[3]));
  return 0;
}
"""


def test_picker_rule_lists_the_headline_shape_and_none_of_its_neighbours(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} not available")
    src, exe = tmp_path / "probe.hip", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split()
    CH, bl, nb, P, M, nbounded = OptimizerParams.readme().dims(28, True)
    assert (CH, bl) == (18, 6), "the listed shape is the headline configuration's"
    nfeas = M - 8 * 28
    assert [int(v) for v in out[:4]] == [nb, 32, nfeas, nbounded]   # what the kernels fold in = what smpc_dims reports
    assert [int(v) for v in out[4:]] == [0, -1, -1, -1, -1, -1, -1, -1, -1]


def test_host_picker_dispatches_through_the_rule():
    def function(path, start):
        text = open(os.path.join(CSRC, path)).read()
        text = text[text.index(start):]
        return text[:text.index("\n}\n")]

    # the rule is asked where the launch is planned, its index is mapped to the kernels where the launch is issued
    body = function("smpc_plan.hpp", "inline SweepPlan plan_sweep(") + function("smpc_sweep_host.hpp", "KernelFn pick_fixed(")
    assert "smpc::fixed_shape_index(k.T, k.N, k.CH, k.bl)" in body and "SMPC_FIXED_SHAPES(SMPC_X)" in body
    assert "k.T ==" not in body and "k.N ==" not in body   # no second copy of the comparison


def test_fixed_shape_functions_are_declared_exported_and_bound():
    from nav2_social_mpc_controller_amd import _abi
    from nav2_social_mpc_controller_amd import solver as S

    root = os.path.dirname(os.path.dirname(CSRC))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "smpc_fixed_shapes.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_abi.FIXED_SHAPE_FUNCTIONS) and len(declared) == 3
    assert not set(declared) & set(_abi.FUNCTIONS)
    assert os.path.exists(S.LIB_PATH), "run __graft_entry__.build() first"
    out = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = S.load_library()
    for name, (restype, argtypes) in _abi.FIXED_SHAPE_FUNCTIONS.items():
        assert name in exported, name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # the header compiles as C beside smpc.h
    subprocess.check_call(["gcc", "-fsyntax-only", "-x", "c", "-I", os.path.join(root, "include"),
                           os.path.join(root, "include", "smpc_fixed_shapes.h")])
