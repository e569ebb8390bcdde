"""Plan smoothing on the CPU: the yardstick itself (tests/plan_smoother_ref.py, a sequential walk through the rule of
include/smpc_plan_smoother.h) on hand-made cases with the expected rows written out and on the 91-pose staircase the rule was
tried on; the `__host__ __device__` rule of csrc/smpc_plan_smoother_rule.hpp compiled into a host-only program and composed as
the kernel composes it (pose i in lane i mod 64 and slot i div 64, the slots swept upwards in place with the rotated copies
handed on, the verdict cache, the ballot in place of the maximum) against the yardstick bit for bit; the same program under the
address and undefined-behaviour sanitizers; the ctypes mirror against the header; PlanSmootherParams, GlobalPlanParams' new last
field and the planner's refusals; and the kernels' resource remarks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import plan_smoother_cases as MC
import plan_smoother_ref as R
from nav2_social_mpc_controller_amd import _abi_plan_smoother as MA
from nav2_social_mpc_controller_amd import solver as S
from nav2_social_mpc_controller_amd.params import GlobalPlanParams, PlanSmootherParams
from test_kernel_budget import CSRC, HIPCC, parse_resource_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc_plan_smoother.h")
KERNELS = {7: "_ZN4smpc23smpc_smooth_plan_kernelILi7EEEvNS_18PlanSmootherParamsE", 16: "_ZN4smpc23smpc_smooth_plan_kernelILi16EEEvNS_18PlanSmootherParamsE"}

HAND = MC.hand_cases()
SEEDED = MC.seeded_cases()


@pytest.fixture(scope="module")
def seeded_ref():
    return {name: R.run(c) for name, c in SEEDED.items()}


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_cases_end_where_the_header_says(name):
    got = R.run(HAND[name])
    MC.check_want(HAND[name], got)
    assert got["plan"].dtype == np.float64 and got["change"].dtype == np.float64 and got["status"].dtype == np.int32 and got["info"].dtype == np.int32


def test_the_hand_made_cases_cover_the_list():
    seen = {s for c in HAND.values() for s in c["want"]["status"]}
    assert seen == {R.CONVERGED, R.MAX_ITS, R.TOO_SHORT, R.BAD_PLAN}
    assert [HAND[k]["plan_len"][0] for k in ("n0", "n1", "n2", "n3_corner_one_sweep")] == [0, 1, 2, 3]
    assert np.isnan(HAND["nan_beyond_n"]["plan"][0, 3:]).all() and HAND["collinear_tolerance_zero"]["tolerance"] == 0.0
    assert [HAND[f"refinement_{r}"]["want"]["info"][0][1] for r in (0, 1, 2)] == [1, 2, 3]
    assert HAND["range_first_above_last"]["range"][0, 0] > HAND["range_first_above_last"]["range"][0, 1]
    assert HAND["a_map_each"]["world"].ndim == 3 and HAND["accepted_with_allow_unknown"]["allow_unknown"]
    assert all(HAND[k]["want"]["info"][0][2] == 1 for k in ("rejected_by_a_lethal_cell", "rejected_by_the_maps_edge", "rejected_by_unknown"))


def test_the_staircase_loses_nine_tenths_of_its_turning():
    c = MC.zigzag_case()
    got = R.run(c)
    raw, smooth = R.turning(c["plan"][0, :91]), R.turning(got["plan"][0, :91])
    print("turning", raw, smooth, got["info"][0].tolist(), got["change"][0])
    assert 32.0 < raw < 32.5                                   # 30 cells east, 20 diagonal, 40 alternating: 41 turns of 45 degrees
    assert smooth < raw / 10.0
    assert got["status"][0] == R.CONVERGED and got["info"][0].tolist()[1:] == [3, 0, 91] and got["change"][0] <= 1e-10
    assert np.array_equal(got["plan"][0, [0, 90]], c["plan"][0, [0, 90]]) and (got["plan"][0, 91:] == MC.SENTINEL).all()
    # the data term keeps every row near where it started: within the staircase's own amplitude of a cell or two
    assert np.abs(got["plan"][0, :91] - c["plan"][0, :91]).max() < 3 * c["res"]


def test_the_staircase_beside_blocked_cells_ends_on_passable_cells():
    c = MC.zigzag_case(blocked=MC.ZIGZAG_BLOCKED)
    free = R.run(MC.zigzag_case())
    got = R.run(c)
    assert got["status"][0] == R.CONVERGED and got["info"][0][2] > 0            # candidates were rejected
    cells = np.floor((got["plan"][0, :91] - c["origin"]) / c["res"]).astype(int)
    assert (c["world"][cells[:, 1], cells[:, 0]] < 253).all()
    # without the blocked cells some row ends in one of them: they do lie where the corner is cut
    free_cells = {tuple(v) for v in np.floor(free["plan"][0, :91] / c["res"]).astype(int).tolist()}
    assert free_cells & set(MC.ZIGZAG_BLOCKED)
    assert R.turning(got["plan"][0, :91]) < R.turning(c["plan"][0, :91]) / 10.0


def test_the_seeded_cases_exercise_the_rule(seeded_ref):
    """By the yardstick alone, before anything is compared with it."""
    seen, rejected, short, ranged = set(), 0, 0, 0
    lengths = {L: set() for L in MC.LS}
    for name, c in SEEDED.items():
        got = seeded_ref[name]
        B, L = c["plan"].shape[:2]
        assert L in MC.LS and c["world"].shape[-2:] == (MC.WORLD_Y, MC.WORLD_X) and B in (1, 13)
        lengths[L] |= set(c["plan_len"].tolist())
        seen |= set(got["status"].tolist())
        rejected += int((got["info"][:, 2] > 0).sum())
        ranged += c["range"] is not None
        for b in range(B):
            n = int(c["plan_len"][b])
            keep = [0, n - 1] + list(range(n, L))
            assert got["plan"][b, keep].tobytes() == c["plan"][b, keep].tobytes()
            moved = (got["plan"][b] != c["plan"][b]).any(axis=1)
            assert moved.any() == (got["status"][b] <= R.MAX_ITS and n > 2) or got["info"][b, 2] > 0
            if c["range"] is not None and moved.any():
                lo, hi = np.flatnonzero(moved)[[0, -1]]
                assert lo >= max(c["range"][b, 0], 1) and hi <= min(c["range"][b, 1], n - 2)
    assert lengths[448] >= {n for n in MC.NS if n <= 448} and lengths[1024] >= set(MC.NS)
    assert {R.CONVERGED, R.MAX_ITS} <= seen and rejected >= 10 and ranged == 4, (seen, rejected, ranged)
    assert sum(c["world"].ndim == 3 for c in SEEDED.values()) == 2


# ---- the compiled rule ------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include "smpc_plan_smoother_rule.hpp"

static double num(const std::string& s) { return std::strtod(s.c_str(), nullptr); }   // hex floats, nan, inf
static std::string hex(double v) { char b[40]; uint64_t u; std::memcpy(&u, &v, 8); std::snprintf(b, sizeof b, "%016llx", (unsigned long long)u); return b; }
static double rd() { std::string w; std::cin >> w; return num(w); }
static long long ri() { long long v; std::cin >> v; return v; }

// The scalars, the maps, then one robot per record, composed as the kernel composes the rule: pose i in lane i % 64 of slot
// i / 64; a sweep goes through the slots upwards and overwrites them in place, the copy of a slot rotated by one lane taken
// before that and handed to the next slot; the map is read only when a candidate has left the cell of the row's last verdict;
// "change <= tolerance" is "no lane above tolerance"; the maximum is reduced after the last sweep.
constexpr int kLanes = 64;
using namespace smpc;

int main() {
  const int B = (int)ri(), L = (int)ri(), W = (int)ri(), H = (int)ri(), shared = (int)ri(), has_range = (int)ri();
  const int32_t max_its = (int32_t)ri(), refinement_num = (int32_t)ri();
  const uint32_t lethal = (uint32_t)ri(), unknown = (uint32_t)ri();
  const double res = rd(), w_data = rd(), w_smooth = rd(), tolerance = rd();
  if (B < 0 || L < 2 || L > kSmoothMaxPoses || W < 1 || H < 1 || max_its < 1 || max_its > kSmoothMaxIts || refinement_num < 0 || refinement_num > kSmoothMaxRefinements) std::abort();
  const int S = L <= 448 ? 7 : 16;
  const int nmap = shared ? 1 : B;
  std::vector<uint8_t> maps((size_t)nmap * W * H);
  for (auto& v : maps) v = (uint8_t)ri();
  std::vector<double> origins((size_t)nmap * 2);
  for (auto& v : origins) v = rd();
  std::vector<double> rows((size_t)L * 2);
  std::vector<double> yx((size_t)S * kLanes), yy(yx), px(yx), py(yx);
  std::vector<uint32_t> verdict((size_t)S * kLanes);
  for (int b = 0; b < B; ++b) {
    const int32_t plan_len = (int32_t)ri(), r0 = (int32_t)ri(), r1 = (int32_t)ri();
    for (auto& v : rows) v = rd();
    const uint8_t* world = maps.data() + (size_t)(shared ? 0 : b) * W * H;
    const SmMap map = {origins[2 * (size_t)(shared ? 0 : b)], origins[2 * (size_t)(shared ? 0 : b) + 1], res, W, H, lethal, unknown};
    const int32_t n = sm_rows(plan_len, L);
    bool finite = true;
    for (int k = 0; k < S; ++k)
      for (int l = 0; l < kLanes; ++l) {
        const int i = kLanes * k + l;
        const size_t at = (size_t)k * kLanes + l;
        yx[at] = yy[at] = 0.0;
        if (i < n) { yx[at] = rows[2 * (size_t)i]; yy[at] = rows[2 * (size_t)i + 1]; finite = finite && sm_finite(yx[at]) && sm_finite(yy[at]); }
        px[at] = yx[at]; py[at] = yy[at];
        verdict[at] = kSmNoVerdict;
      }
    int32_t first = 0, last = 0;
    const bool any_movable = sm_movable(n, has_range != 0, r0, r1, &first, &last);
    SmProgress prog = sm_start();
    uint64_t rejected = 0;
    double moved[kLanes];
    for (double& m : moved) m = 0.0;
    if (!finite) prog.status = kSmoothBadPlan;
    else if (!any_movable) prog.status = kSmoothTooShort;
    else {
      const int64_t bound = sm_sweep_bound(max_its, refinement_num);
      for (int64_t t = 0; t < bound; ++t) {
        for (double& m : moved) m = 0.0;
        double below_x[kLanes] = {0}, below_y[kLanes] = {0}, above_x[kLanes], above_y[kLanes];
        for (int l = 0; l < kLanes; ++l) { above_x[l] = yx[(l + 1) & 63]; above_y[l] = yy[(l + 1) & 63]; }
        for (int k = 0; k < S; ++k) {
          if (kLanes * k >= n) continue;
          double up_x[kLanes], up_y[kLanes], next_x[kLanes] = {0}, next_y[kLanes] = {0}, ox[kLanes], oy[kLanes];
          for (int l = 0; l < kLanes; ++l) {
            const size_t at = (size_t)k * kLanes;
            ox[l] = yx[at + l]; oy[l] = yy[at + l];
            up_x[l] = yx[at + ((l + 63) & 63)]; up_y[l] = yy[at + ((l + 63) & 63)];
            if (k + 1 < S) { next_x[l] = yx[at + kLanes + ((l + 1) & 63)]; next_y[l] = yy[at + kLanes + ((l + 1) & 63)]; }
          }
          for (int l = 0; l < kLanes; ++l) {
            const size_t at = (size_t)k * kLanes + l;
            const int i = kLanes * k + l;
            const double mx = l == 0 ? below_x[l] : up_x[l], my = l == 0 ? below_y[l] : up_y[l];
            const double qx = l == 63 ? next_x[l] : above_x[l], qy = l == 63 ? next_y[l] : above_y[l];
            const bool mine = i >= first && i <= last;
            const double cx = sm_candidate(px[at], ox[l], mx, qx, w_data, w_smooth);
            const double cy = sm_candidate(py[at], oy[l], my, qy, w_data, w_smooth);
            int32_t idx = 0;
            const bool in_map = mine && sm_cell(map, cx, cy, &idx);
            if (in_map && !sm_verdict_is_of(verdict[at], idx)) {
              if (idx < 0 || idx >= W * H) std::abort();
              verdict[at] = sm_verdict(idx, sm_passable(map, world[idx]));
            }
            const bool accepted = in_map && sm_verdict_passable(verdict[at]);
            if (mine && !accepted) ++rejected;
            if (accepted) {
              yx[at] = cx; yy[at] = cy;
              const double hx = sm_moved(cx, ox[l]), hy = sm_moved(cy, oy[l]);
              const double h = hx > hy ? hx : hy;
              moved[l] = h > moved[l] ? h : moved[l];
            }
          }
          std::memcpy(below_x, up_x, sizeof up_x); std::memcpy(below_y, up_y, sizeof up_y);
          std::memcpy(above_x, next_x, sizeof next_x); std::memcpy(above_y, next_y, sizeof next_y);
        }
        bool within = true;
        for (double m : moved) within = within && (m <= tolerance);
        const int then = sm_after_sweep(prog, within, max_its, refinement_num);
        if (then == kSmStop) break;
        if (then == kSmNextRound) { px = yx; py = yy; }
      }
      for (int i = first; i <= last; ++i) { rows[2 * (size_t)i] = yx[i]; rows[2 * (size_t)i + 1] = yy[i]; }   // slot-major: index i
      for (int m = 32; m >= 1; m >>= 1) {
        double other[kLanes];
        for (int l = 0; l < kLanes; ++l) other[l] = moved[l ^ m];
        for (int l = 0; l < kLanes; ++l) moved[l] = other[l] > moved[l] ? other[l] : moved[l];
      }
    }
    std::printf("%d %d %d %d %d %s", prog.status, prog.sweeps, prog.rounds, sm_saturate(rejected), n, hex(moved[0]).c_str());
    for (double v : rows) std::printf(" %s", hex(v).c_str());
    std::printf("\n");
  }
  return 0;
}
"""


def probe_input(c):
    hx = lambda v: float(v).hex() if np.isfinite(v) else repr(float(v))
    B, L = c["plan"].shape[:2]
    H, W = c["world"].shape[-2:]
    lines = [" ".join(map(str, [B, L, W, H, int(c["world"].ndim == 2), int(c["range"] is not None), c["max_its"], c["refinement_num"],
                                c["lethal_min_cost"], int(c["allow_unknown"]), hx(c["res"]), hx(c["w_data"]), hx(c["w_smooth"]), hx(c["tolerance"])]))]
    lines.append(" ".join(map(str, c["world"].ravel().tolist())))
    lines.append(" ".join(hx(v) for v in np.asarray(c["origin"], np.float64).ravel()))
    for b in range(B):
        r = (0, 0) if c["range"] is None else c["range"][b]
        lines.append(f"{int(c['plan_len'][b])} {int(r[0])} {int(r[1])}")
        lines.append(" ".join(hx(v) for v in c["plan"][b].ravel()))
    return "\n".join(lines) + "\n"


def probe_output(c, text):
    """The program's lines as plan_smoother_ref.run's outputs."""
    B, L = c["plan"].shape[:2]
    out = text.splitlines()
    assert len(out) == B
    got = dict(plan=np.zeros((B, L, 2)), status=np.zeros(B, np.int32), info=np.zeros((B, 4), np.int32), change=np.zeros(B))
    for b in range(B):
        w = out[b].split()
        got["status"][b], got["info"][b] = int(w[0]), [int(v) for v in w[1:5]]
        got["change"][b] = np.array([int(w[5], 16)], np.uint64).view(np.float64)[0]
        got["plan"][b] = np.array([int(v, 16) for v in w[6:]], np.uint64).view(np.float64).reshape(L, 2)
    return got


def build_probe(tmp, name, extra=()):
    src, exe = tmp / "probe.hip", tmp / name
    src.write_text(PROBE)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", *extra, "-I", CSRC, str(src), "-o", str(exe)])   # -O3 as build.sh
    return exe


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    exe = build_probe(tmp_path_factory.mktemp("plan_smoother_rule"), "probe")
    return lambda c: probe_output(c, subprocess.run([str(exe)], input=probe_input(c), capture_output=True, text=True, check=True).stdout)


@pytest.mark.parametrize("name", sorted(HAND))
def test_compiled_rule_is_the_yardstick_on_the_hand_made_cases(rule, name):
    got = rule(HAND[name])
    assert R.same(got, R.run(HAND[name]))
    MC.check_want(HAND[name], got)


@pytest.mark.parametrize("name", list(SEEDED))
def test_compiled_rule_is_the_yardstick_on_the_seeded_cases(rule, seeded_ref, name):
    got, want = rule(SEEDED[name]), seeded_ref[name]
    for k in R.OUTPUTS:
        assert got[k].tobytes() == want[k].tobytes(), (k, got["status"].tolist(), want["status"].tolist(), got["info"].tolist(), want["info"].tolist())


def test_compiled_rule_is_the_yardstick_on_the_staircase(rule):
    for c in (MC.zigzag_case(), MC.zigzag_case(blocked=MC.ZIGZAG_BLOCKED)):
        assert R.same(rule(c), R.run(c))


def test_the_program_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path, seeded_ref):
    """The stand-alone program (its own main, nothing loaded into Python), built once more with the sanitizers: it exits 0 and
    prints what the plain build prints."""
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    exe = build_probe(tmp_path, "probe_san", ("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"))
    for name in (MC.seeded_name(13, 448, False, 4), MC.seeded_name(13, 1024, True, 5)):
        r = subprocess.run([str(exe)], input=probe_input(SEEDED[name]), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        assert R.same(probe_output(SEEDED[name], r.stdout), seeded_ref[name])
    for name in ("n0", "nan_in_a_row", "rejected_by_the_maps_edge", "range_one_row", "a_map_each"):
        r = subprocess.run([str(exe)], input=probe_input(HAND[name]), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        assert R.same(probe_output(HAND[name], r.stdout), R.run(HAND[name]))


def test_the_rule_header_rounds_every_operation_on_its_own_and_the_kernel_uses_it():
    text = open(os.path.join(CSRC, "smpc_plan_smoother_rule.hpp")).read()
    assert "#pragma clang fp contract(off)" in text and "fma(" not in text and "hip_runtime" not in text
    assert re.findall(r'#include\s+([<"][^>"]+[>"])', text) == ["<stdint.h>", '"smpc_global_plan_rule.hpp"']
    assert "gp_cell_axis(" in text and "gp_passable(" in text and "floor(" not in text
    kernel = open(os.path.join(CSRC, "smpc_plan_smoother.hpp")).read()
    code = kernel.split("#pragma once")[1]
    assert '#include "smpc_plan_smoother_rule.hpp"' in kernel and "atomic" not in code and "__shared__" not in code
    assert "sm_candidate(" in code and "sm_cell(" in code and "sm_after_sweep(" in code and "sm_sweep_bound(" in code and "__ballot(" in code
    hip = open(os.path.join(CSRC, "smpc_hip.hip")).read()
    assert '#include "smpc_plan_smoother.hpp"' in hip and "smpc::smpc_smooth_plan_kernel<smpc::kSmSlotsShort>" in hip and "smpc::smpc_smooth_plan_kernel<smpc::kSmSlotsLong>" in hip
    entry = hip[hip.index("int smpc_smooth_plan_batch("):]
    entry = entry[:entry.index("\n}\n")]
    assert "hipMalloc" not in entry and "Synchronize" not in entry and "hipMemcpy" not in entry     # capturable with device pointers
    header = open(HEADER).read()
    assert "as recalled" in header


# ---- the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mirror_matches_the_header_and_the_library_exports_the_function(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src))) == sorted(MA.FUNCTIONS) == ["smpc_smooth_plan_batch"]
    assert re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S) == [st.c_name for st in MA.STRUCTS]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' + "".join(f'printf("%zu\\n", offsetof({st.c_name}, {f[0]}));\n' for f in st._fields_)
                   for st in MA.STRUCTS)
    names = ["SMPC_SMOOTH_" + n for n in MA.SMOOTH_STATUS]
    limits = ["SMPC_SMOOTH_MAX_POSES", "SMPC_SMOOTH_MAX_ITS", "SMPC_SMOOTH_MAX_REFINEMENTS"]
    body += "".join(f'printf("%d\\n", (int){n});\n' for n in limits + names)
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc_plan_smoother.h"\nint main(void){\n' + body + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [v for st in MA.STRUCTS for v in [C.sizeof(st)] + [getattr(st, f[0]).offset for f in st._fields_]]
    assert values == want + [getattr(MA, n) for n in limits + names]
    assert values[-7:] == [1024, 100000, 8, 0, 1, 2, 3]
    assert R.STATUS == MA.SMOOTH_STATUS and (R.CONVERGED, R.MAX_ITS, R.TOO_SHORT, R.BAD_PLAN) == (0, 1, 2, 3)
    assert (PlanSmootherParams.MAX_POSES, PlanSmootherParams.MAX_ITS, PlanSmootherParams.MAX_REFINEMENTS) == (1024, 100000, 8)
    for st in MA.STRUCTS:
        fields = re.findall(r"\b(\w+)\s*(?:\[\w+\]\s*)*(?:,|;)", re.search(r"typedef struct %s \{(.*?)\}" % st.c_name, src, flags=re.S).group(1))
        assert fields == [f[0] for f in st._fields_], st.c_name
    assert C.sizeof(MA.SmpcPlanSmootherIn) == 10 * 4 + 4 * 8 + 4 * 8
    exported = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    lib = S.load_library()
    for name, (restype, argtypes) in MA.FUNCTIONS.items():
        assert f" {name}\n" in exported
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes


def test_the_main_abi_is_as_it_was():
    from nav2_social_mpc_controller_amd import _abi
    assert _abi.SMPC_ABI_VERSION == 6 and len(_abi.FUNCTIONS) == 27 and not set(MA.FUNCTIONS) & set(_abi.FUNCTIONS)
    assert "SMPC_ABI_VERSION 6" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "smpc.h")).read())


# ---- the parameters -------------------------------------------------------------------------------------------------------
def test_plan_smoother_params():
    sp = PlanSmootherParams()
    assert (sp.w_data, sp.w_smooth, sp.tolerance, sp.max_its, sp.refinement_num, sp.lethal_min_cost, sp.allow_unknown) == (0.2, 0.3, 1e-10, 1000, 2, None, None)
    assert sp.supported(400) and sp.supported(1024) and not sp.supported(1025)
    assert PlanSmootherParams(max_its=100000).supported(400) and not PlanSmootherParams(max_its=100001).supported(400)
    assert PlanSmootherParams(refinement_num=8).supported(400) and not PlanSmootherParams(refinement_num=9).supported(400)
    PlanSmootherParams(w_data=1.0, w_smooth=0.2499), PlanSmootherParams(tolerance=0.0), PlanSmootherParams(tolerance=np.inf), PlanSmootherParams(w_smooth=0.0)
    for bad in (dict(w_data=0.0), dict(w_data=-0.1), dict(w_data=np.nan), dict(w_data=np.inf), dict(w_smooth=-0.1), dict(w_smooth=np.nan),
                dict(w_smooth=np.inf), dict(w_data=1.0, w_smooth=0.25), dict(w_data=0.2, w_smooth=0.45), dict(tolerance=-1e-12), dict(tolerance=np.nan),
                dict(max_its=0), dict(max_its=1.5), dict(refinement_num=-1), dict(refinement_num=0.5), dict(lethal_min_cost=256), dict(lethal_min_cost=-1)):
        with pytest.raises(ValueError):
            PlanSmootherParams(**bad)


def test_global_plan_params_gain_a_last_field():
    assert GlobalPlanParams(7, 3, 200, True, 33, 4).smoother is None and GlobalPlanParams().smoother is None
    assert list(GlobalPlanParams.__dataclass_fields__)[-1] == "smoother"
    sp = PlanSmootherParams()
    assert GlobalPlanParams(7, 3, 200, True, 33, 4, sp).smoother is sp and GlobalPlanParams(smoother=sp).max_poses == 400
    with pytest.raises(ValueError):
        GlobalPlanParams(smoother=dict(w_data=0.2))


def test_the_struct_the_call_takes():
    si = S.BatchSolver.smooth_plan_c(PlanSmootherParams(), 7, 400, 200, 180, True, 0.05, 1, 200, True)
    assert (si.B, si.L, si.on_device, si.world_x, si.world_y, si.world_shared, si.max_its, si.refinement_num) == (7, 400, 1, 200, 180, 1, 1000, 2)
    assert (si.lethal_min_cost, si.allow_unknown, si.resolution, si.w_data, si.w_smooth, si.tolerance) == (200, 1, 0.05, 0.2, 0.3, 1e-10)
    assert not si.world and not si.world_origin and not si.plan_len and not si.range
    own = S.BatchSolver.smooth_plan_c(PlanSmootherParams(lethal_min_cost=100, allow_unknown=False), 1, 2, 3, 4, False, 0.1, 0, 200, True)
    assert (own.lethal_min_cost, own.allow_unknown, own.world_shared, own.on_device) == (100, 0, 0, 0)


def test_the_planner_refuses_what_the_library_would():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, TickRecord
    from nav2_social_mpc_controller_amd.episode_stages import Planner
    world, traj, goal = object(), object(), np.zeros((1, 2))
    Planner.check(GlobalPlanParams(smoother=PlanSmootherParams()), None, None, world, traj, goal)
    Planner.check(GlobalPlanParams(max_poses=1024, smoother=PlanSmootherParams(max_its=100000, refinement_num=8)), None, None, world, traj, goal)
    Planner.check(GlobalPlanParams(max_poses=2000), None, None, world, traj, goal)                  # no smoother: the planner's own limits
    for bad in (GlobalPlanParams(max_poses=1025, smoother=PlanSmootherParams()), GlobalPlanParams(smoother=PlanSmootherParams(max_its=100001)),
                GlobalPlanParams(smoother=PlanSmootherParams(refinement_num=9))):
        with pytest.raises(ValueError, match="planner.smoother"):
            Planner.check(bad, None, None, world, traj, goal)
    gp = GlobalPlanParams()
    gp.smoother = dict(w_data=0.2)                                                                # set behind the constructor's back
    with pytest.raises(ValueError, match="must be a PlanSmootherParams"):
        Planner.check(gp, None, None, world, traj, goal)
    # the smoother rides on an existing keyword: no new keyword, stage or record field
    assert "smoother" not in BatchEpisode.FORWARDED + BatchEpisode.PER_ROBOT + BatchEpisode.PER_GRID and Planner not in BatchEpisode.STAGES
    assert not [f for f in TickRecord.__dataclass_fields__ if "smooth" in f]


# ---- the kernels' resources -------------------------------------------------------------------------------------------------
def test_the_kernels_have_no_spills_and_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    r = subprocess.run(["bash", os.path.join(CSRC, "build.sh"), "-DSMPC_ONLY_NB=3", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage"],
                       env={**os.environ, "SMPC_OUT": str(tmp_path / "smpc_nb3.o")}, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = parse_resource_remarks(r.stderr)
    for slots, kernel in KERNELS.items():
        use = remarks.get(kernel)
        assert use is not None, f"no resource remark for {kernel}"
        print(kernel, use)
        assert use["VGPRs Spill"] == 0 and use["SGPRs Spill"] == 0 and use["ScratchSize [bytes/lane]"] == 0, use   # no private segment
        assert use["LDS Size [bytes/block]"] == 0
    # the kernel of the planner's plans (L <= 448): four wavefronts a SIMD; a slot's state alone is nine registers
    assert 9 * 7 <= remarks[KERNELS[7]]["VGPRs"] <= 128
    assert 9 * 16 <= remarks[KERNELS[16]]["VGPRs"] + remarks[KERNELS[16]]["AGPRs"] <= 512
