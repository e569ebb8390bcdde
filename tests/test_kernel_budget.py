"""Register budget of the headline kernels, checked at compile time (CPU only, ~15 s).

`__launch_bounds__` holds the solve kernel and K1 at the 168 VGPRs three waves per SIMD allow, but an edit that needs
more does not fail the build: the allocator spills instead (private-segment stores and reloads inside the sweep, and a
kernel that allocates scratch at every launch). This test compiles the NB = 3 instantiations with the flags of
`csrc/build.sh` and reads the compiler's kernel-resource-usage remarks."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nav2_social_mpc_controller_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"   # what build.sh invokes

# the two-scenes-per-wave, fixed-horizon instantiations bench.py's workload runs: solve (timed) and K1 (roofline)
KERNELS = {
    "solve<3,32,false>": "_ZN4smpc17smpc_solve_kernelILi3ELi32ELb0ELb0ELb0EEEvNS_7KParamsE",
    "K1<3,32,false>": "_ZN4smpc16smpc_eval_kernelILi3ELi32ELb0ELb0EEEvNS_7KParamsE",
}
MAX_VGPRS = 168   # 512 / 3, in the allocation granule: three waves per SIMD


def parse_resource_remarks(text):
    """{function name: {field: int}} from `-Rpass-analysis=kernel-resource-usage` output."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*?): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    obj = str(tmp_path_factory.mktemp("budget") / "smpc_nb3.o")
    r = subprocess.run(["bash", os.path.join(CSRC, "build.sh"), "-DSMPC_ONLY_NB=3", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage"],
                       env={**os.environ, "SMPC_OUT": obj}, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return parse_resource_remarks(r.stderr)


def test_parser_reads_a_remark_block():
    text = ("x.hpp:1:1: remark: Function Name: k [-Rpass-analysis=kernel-resource-usage]\n"
            "x.hpp:1:1: remark:     VGPRs: 161 [-Rpass-analysis=kernel-resource-usage]\n"
            "x.hpp:1:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]\n"
            "x.hpp:1:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]\n")
    assert parse_resource_remarks(text) == {"k": {"VGPRs": 161, "ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0}}


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_headline_kernel_fits_three_waves_without_spills(usage, name):
    r = usage.get(KERNELS[name])
    assert r is not None, f"{name}: no resource remark (instantiation missing?)"
    assert r["VGPRs"] <= MAX_VGPRS, f"{name}: {r['VGPRs']} VGPRs > {MAX_VGPRS} (fewer than three waves per SIMD)"
    assert r["VGPRs Spill"] == 0, f"{name}: {r['VGPRs Spill']} spilled VGPRs"
    assert r["SGPRs Spill"] == 0, f"{name}: {r['SGPRs Spill']} spilled SGPRs"
    assert r["ScratchSize [bytes/lane]"] == 0, f"{name}: {r['ScratchSize [bytes/lane]']} B/lane private segment"
    assert r["Occupancy [waves/SIMD]"] >= 3, f"{name}: occupancy {r['Occupancy [waves/SIMD]']}"
