"""The per-iteration trace of a solve (`smpc_solve_trace_batch`, optimizer.debug_optimizer), host side: the C ABI addition,
the register budget of the trace kernel and the text the C++ host mirror prints (CPU only; the device behaviour is in
tests/test_gpu_trace.py, the row rules themselves in tests/test_trace_oracle_rules.py)."""
import ctypes as C
import os
import re
import subprocess

from nav2_social_mpc_controller_amd import _abi
from test_kernel_budget import MAX_VGPRS, usage  # noqa: F401  (usage: the NB = 3 build's resource remarks)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nav2_social_mpc_controller_amd", "host")


def test_trace_entry_point_is_exported_and_the_version_stays():
    from nav2_social_mpc_controller_amd import solver as S
    lib = S.load_library()
    assert "smpc_solve_trace_batch" in _abi.EXPORTED_SYMBOLS
    assert lib.smpc_solve_trace_batch.restype is C.c_int  # bound by load_library(): the symbol resolves
    out = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    assert re.search(r"\bsmpc_solve_trace_batch$", out, flags=re.M)
    # an addition: no existing struct changed, the version did not move
    assert _abi.SMPC_ABI_VERSION == 6 and lib.smpc_abi_version() == 6
    assert S.TRACE_COLS == ["iter", "cost", "cost_change", "gradient_max_norm", "step_norm", "rho", "radius", "ls_evals", "accepted"]


# ---- register budget of the trace kernel (compile time, like tests/test_scene_params.py) --------------------------
TRACE_SOLVE = "_ZN4smpc17smpc_solve_kernelILi3ELi32ELb1ELb1ELb1EEEvNS_7KParamsE"
SP_SOLVE = "_ZN4smpc17smpc_solve_kernelILi3ELi32ELb1ELb1ELb0EEEvNS_7KParamsE"  # the same template without kTrace


def test_trace_kernel_costs_no_register_spill_or_private_segment(usage):
    """The values of a row are in LDS (sv[]) or in registers that are live anyway where a row is written: the trace kernel
    <3,32> stays within what smpc_solve_kernel<3,32,true,true> had before it existed (168 VGPRs, 12 spilled VGPRs, a 20 B
    private segment, 3 waves per SIMD, no spilled SGPR), and within what that kernel has in the same build."""
    r, sp = usage.get(TRACE_SOLVE), usage[SP_SOLVE]
    assert r is not None, "no resource remark for the trace kernel (instantiation missing?)"
    assert r["VGPRs"] <= MAX_VGPRS and r["Occupancy [waves/SIMD]"] >= 3, r
    assert r["SGPRs Spill"] == 0, r
    assert r["VGPRs Spill"] <= 12 and r["ScratchSize [bytes/lane]"] <= 20, r
    assert r["VGPRs Spill"] <= sp["VGPRs Spill"] and r["ScratchSize [bytes/lane]"] <= sp["ScratchSize [bytes/lane]"], (r, sp)


def test_one_scene_per_wave_trace_kernel_is_compiled(usage):
    assert "_ZN4smpc17smpc_solve_kernelILi3ELi64ELb1ELb1ELb1EEEvNS_7KParamsE" in usage


# ---- what debug_optimizer prints (host/optimizer.cpp: format_trace, format_trace_summary) --------------------------
FORMAT_PROG = r"""
#include <iostream>
#include "optimizer.hpp"
int main() {
  const double rows[3 * SMPC_TRACE_COLS] = {
    0, 12.5, 0, 3.25, 0, 0, 1e4, 0, 1,
    1, 10.0, 2.5, 1.5, 0.125, 0.75, 12000, 2, 1,
    2, 10.0, -1e-3, 1.5, 0.0625, -0.5, 6000, 1, 0};
  nav2_social_mpc_controller::format_trace(std::cout, rows, 3);
  nav2_social_mpc_controller::format_trace_summary(std::cout, SMPC_NO_CONVERGENCE, SMPC_REASON_MAX_ITERATIONS, 2, 12.5, 10.0);
  nav2_social_mpc_controller::format_trace(std::cout, rows, 0);
  nav2_social_mpc_controller::format_trace_summary(std::cout, SMPC_FAILURE, SMPC_REASON_SHORT_PATH, 0, 0.0, 0.0);
  return 0;
}
"""
FORMAT_TEXT = """\
iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius  ls_iter  ok
   0  1.250000e+01    0.00e+00    3.25e+00   0.00e+00   0.00e+00  1.00e+04        0   1
   1  1.000000e+01    2.50e+00    1.50e+00   1.25e-01   7.50e-01  1.20e+04        2   1
   2  1.000000e+01   -1.00e-03    1.50e+00   6.25e-02  -5.00e-01  6.00e+03        1   0
NO_CONVERGENCE (max_iterations) after 2 iterations, cost 1.250000e+01 -> 1.000000e+01
iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius  ls_iter  ok
FAILURE (short_path) after 0 iterations, cost 0.000000e+00 -> 0.000000e+00
"""


def test_host_formatter_prints_the_rows_in_ceres_layout(tmp_path):
    assert os.path.exists(os.path.join(HOST, "libsmpc_host.so")), "run __graft_entry__.build() first"
    prog = tmp_path / "format_trace.cpp"
    prog.write_text(FORMAT_PROG)
    exe = tmp_path / "format_trace"
    csrc = os.path.join(ROOT, "nav2_social_mpc_controller_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-I", HOST, str(prog), "-o", str(exe), "-L", HOST, "-lsmpc_host", "-L", csrc,
                           "-lsmpc_hip", f"-Wl,-rpath,{HOST}", f"-Wl,-rpath,{csrc}"])
    assert subprocess.check_output([str(exe)], text=True) == FORMAT_TEXT
