"""Plan repair on the CPU: the yardstick itself (tests/plan_repair_ref.py, a sequential walk through the rules of
include/smpc_plan_repair.h) on hand-made cases with the expected rows written out, what the seeded cases exercise, the
`__host__ __device__` rule of csrc/smpc_plan_repair_rule.hpp compiled into a host-only program and composed as the kernels
compose it (passes of 64 lanes with a butterfly for the closest pose, ballots for the stretch in view, the region relaxed in
place in four colours under the cap, the walk, the splice through the workspace) against the yardstick bit for bit, the same
program under the address and undefined-behaviour sanitizers, the ctypes mirror against the header, PlanRepairParams, the
episode's declaration and refusals, the kernels' resource remarks, and what the rule does behind a real scan, on the
yardsticks of the scan and of this stage alone."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import global_plan_ref as G
import plan_repair_cases as MC
import plan_repair_ref as R
import sensed_costmap_ref
from nav2_social_mpc_controller_amd import _abi_plan_repair as MA
from nav2_social_mpc_controller_amd import solver as S
from nav2_social_mpc_controller_amd.params import PlanRepairParams, SensorParams
from test_kernel_budget import CSRC, HIPCC, parse_resource_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc_plan_repair.h")
JUDGE = "_ZN4smpc24smpc_repair_judge_kernelENS_16PlanRepairParamsE"
FIELD = "_ZN4smpc24smpc_repair_field_kernelENS_16PlanRepairParamsE"

HAND = MC.hand_cases()
SEEDED = MC.seeded_cases()


@pytest.fixture(scope="module")
def seeded_ref():
    out = {}
    for name, c in SEEDED.items():
        details = []
        out[name] = (R.run(c, details=details), details)
    return out


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_cases_end_where_the_contract_says(name):
    c = HAND[name]
    details = []
    got = R.run(c, details=details)
    MC.check_want(c, got)
    assert got["plan"].dtype == np.float64 and got["field"].dtype == np.uint32 and all(got[k].dtype == np.int32 for k in ("plan_len", "status", "info"))
    for r in details:
        if r["F"] is not None:
            fa = int(r["F"][c["R"], c["R"]])
            assert R.check_fixed_point(r["field"], r["w"], r["t"], fa) >= 1


def test_the_hand_made_cases_cover_the_list():
    assert max(c["costmap"].shape[-1] for c in HAND.values()) <= 15 and max(c["costmap"].shape[-2] for c in HAND.values()) <= 15
    seen = {s for c in HAND.values() for s in c["want"]["status"]}
    assert seen == set(range(8)) - {R.INCONSISTENT_FIELD}
    assert HAND["m_zero"]["want"]["info"][0][3] == 0 and HAND["m_below_stride"]["want"]["info"][0][3] < HAND["m_below_stride"]["stride"]
    assert HAND["shared"]["costmap"].ndim == 2 and HAND["allow_unknown"]["cost"].allow_unknown
    assert len(HAND["fits_exactly"]["want"]["rows"][0]) == HAND["fits_exactly"]["plan"].shape[1] == HAND["too_long"]["plan"].shape[1] + 1


def test_the_seeded_cases_exercise_the_rule(seeded_ref):
    """By the yardstick alone, before anything is compared with it."""
    assert [MC.seeded_name(*s) for s in MC.SHAPES] == list(SEEDED)
    seen, bends, own_cell = set(), 0, 0
    for (B, L, window, radius, stride), (name, c) in zip(MC.SHAPES, SEEDED.items()):
        got, details = seeded_ref[name]
        assert c["plan"].shape == (B, L, 2) and c["costmap"].shape == (B, window[1], window[0]) and c["R"] == radius and c["stride"] == stride
        seen |= set(got["status"].tolist())
        assert (got["status"] == R.REPAIRED).sum() * 4 >= B, (name, np.bincount(got["status"], minlength=8))
        for b, r in enumerate(details):
            if r["F"] is not None:
                assert R.check_fixed_point(r["field"], r["w"], r["t"], int(r["F"][radius, radius])) >= 1
            if r["cells"]:
                steps = [(q[0] - p[0], q[1] - p[1]) for p, q in zip(r["cells"], r["cells"][1:])]
                bends += any(u != v for u, v in zip(steps, steps[1:]))
                a = r["cells"][0]
                own_cell += not G.passable(c["costmap"][b], c["cost"])[a[1], a[0]]
            if got["status"][b] != R.REPAIRED:
                assert got["plan_len"][b] == c["plan_len"][b] and G.same_bits(got["plan"][b], c["plan"][b])
    assert seen == set(range(8)) - {R.INCONSISTENT_FIELD}, seen
    assert bends >= 10 and own_cell >= 1, (bends, own_cell)


# ---- the compiled rule ------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include "smpc_plan_repair_rule.hpp"

static double num(const std::string& s) { return std::strtod(s.c_str(), nullptr); }   // hex floats, nan, inf
static std::string hex(double v) { char b[40]; uint64_t u; std::memcpy(&u, &v, 8); std::snprintf(b, sizeof b, "%016llx", (unsigned long long)u); return b; }
static double rd() { std::string w; std::cin >> w; return num(w); }
static long long ri() { long long v; std::cin >> v; return v; }

// The scalars, the windows, then one robot per record, composed as the kernels compose the rule. Judging: 64 "lanes", lane l
// takes poses s + l, s + l + 64, .. and keeps its best key, a butterfly over the lanes makes them agree; the stretch in view
// in passes of 64 poses from i0, the first pose out of view ends it, the blocked poses below it give i1 and i2; the rejoin
// is the first hit of a pass behind i2. Field: the haloed arrays, relaxed in place colour by colour, the colour of the
// robot's cell last, under the cap read at the start of the sweep, until a sweep changes nothing; the walk; the splice
// through the workspace.
constexpr int kLanes = 64;
using namespace smpc;

int main() {
  const int B = (int)ri(), L = (int)ri(), W = (int)ri(), H = (int)ri(), shared = (int)ri(), R = (int)ri(), stride = (int)ri(), has_start = (int)ri();
  const double res = rd(), clearance = rd();
  GpCost cost;
  cost.neutral = (int32_t)ri(); cost.weight = (int32_t)ri(); cost.lethal_min = (uint32_t)ri(); cost.allow_unknown = (uint32_t)ri();
  if (B < 0 || L < 2 || R < 1 || R > kRepairMaxRadius || stride < 1 || W < 1 || H < 1) std::abort();
  const int nmap = shared ? 1 : B;
  std::vector<uint8_t> maps((size_t)nmap * W * H);
  for (auto& v : maps) v = (uint8_t)ri();
  std::vector<double> origins((size_t)nmap * 2);
  for (auto& v : origins) v = rd();
  const int S = 2 * R + 1, pitch = S + 2, ia = (R + 1) * pitch + R + 1;
  std::vector<uint32_t> f((size_t)pitch * pitch);
  std::vector<uint16_t> w((size_t)pitch * pitch);
  std::vector<double> rows((size_t)L * 2), ws((size_t)L * 2);
  for (int b = 0; b < B; ++b) {
    const double x = rd(), y = rd();
    int32_t n = (int32_t)ri();
    const int32_t s = (int32_t)ri();
    for (auto& v : rows) v = rd();
    const uint8_t* costmap = maps.data() + (size_t)(shared ? 0 : b) * W * H;
    const PrWindow win = {origins[2 * (size_t)(shared ? 0 : b)], origins[2 * (size_t)(shared ? 0 : b) + 1], res, W, H};
    auto classify = [&](double px, double py, int32_t ax, int32_t ay) {
      int32_t cx = 0, cy = 0;
      if (!pr_region_cell(win, px, py, ax, ay, R, &cx, &cy)) return kPoseOutOfView;
      return pr_pose_class(cost, costmap[(size_t)cy * W + cx], cx == ax && cy == ay);
    };
    int32_t st = kRepairPending, i0 = -1, i1 = -1, j = -1, m = -1, ax = 0, ay = 0;
    bool wrote_field = false;
    if (n < 2 || n > L || (has_start && (s < 0 || s >= n))) st = kRepairNoPlan;
    else if (!(gp_cell_axis(x, win.ox, win.res, win.sx, &ax) && gp_cell_axis(y, win.oy, win.res, win.sy, &ay))) st = kRepairNoCell;
    else {
      bool bv[kLanes]; double bd[kLanes]; int32_t bi[kLanes];
      for (int l = 0; l < kLanes; ++l) {
        bv[l] = false; bd[l] = 0.0; bi[l] = 0;
        for (long long i = (long long)s + l; i < n; i += kLanes) {
          const double d = pr_d2(rows[2 * (size_t)i], rows[2 * (size_t)i + 1], x, y);
          if (pr_closer(pr_finite(d), d, (int32_t)i, bv[l], bd[l], bi[l])) { bv[l] = true; bd[l] = d; bi[l] = (int32_t)i; }
        }
      }
      for (int mask = 32; mask >= 1; mask >>= 1) {
        bool nv[kLanes]; double nd[kLanes]; int32_t ni[kLanes];
        for (int l = 0; l < kLanes; ++l) {
          const int o = l ^ mask;
          const bool take = pr_closer(bv[o], bd[o], bi[o], bv[l], bd[l], bi[l]);
          nv[l] = take ? true : bv[l]; nd[l] = take ? bd[o] : bd[l]; ni[l] = take ? bi[o] : bi[l];
        }
        std::memcpy(bv, nv, sizeof bv); std::memcpy(bd, nd, sizeof bd); std::memcpy(bi, ni, sizeof bi);
      }
      for (int l = 1; l < kLanes; ++l) if (bv[l] != bv[0] || bi[l] != bi[0]) std::abort();   // the lanes agree
      if (!bv[0]) st = kRepairNoPlan;
      else {
        i0 = bi[0];
        int32_t i2 = -1;
        long long e = n;
        for (long long base = i0; base < n; base += kLanes) {
          int lim = kLanes, first = -1, last = -1;
          for (int l = 0; l < kLanes; ++l) {
            const long long i = base + l;
            const int cls = i < n ? classify(rows[2 * (size_t)i], rows[2 * (size_t)i + 1], ax, ay) : kPoseOutOfView;
            if (i < n && cls == kPoseOutOfView && lim == kLanes) lim = l;
            if (cls == kPoseBlocked && l < lim) { if (first < 0) first = l; last = l; }
          }
          if (first >= 0) { if (i1 < 0) i1 = (int32_t)(base + first); i2 = (int32_t)(base + last); }
          if (lim < kLanes) { e = base + lim; break; }
        }
        if (i1 < 0) st = kRepairClear;
        else {
          const double qx = rows[2 * (size_t)i2], qy = rows[2 * (size_t)i2 + 1];
          for (long long i = (long long)i2 + 1; i < e && j < 0; ++i) {
            const double px = rows[2 * (size_t)i], py = rows[2 * (size_t)i + 1];
            if (classify(px, py, ax, ay) == kPosePassable && pr_d2(px, py, qx, qy) >= clearance) j = (int32_t)i;
          }
          if (j < 0) st = kRepairNoRejoin;
        }
      }
    }
    if (st == kRepairPending) {
      int32_t tx = 0, ty = 0;
      if (!gp_cell_axis(rows[2 * (size_t)j], win.ox, win.res, win.sx, &tx) || !gp_cell_axis(rows[2 * (size_t)j + 1], win.oy, win.res, win.sy, &ty)) std::abort();
      const int x0 = ax - R - 1, y0 = ay - R - 1;
      for (int hy = 0; hy < pitch; ++hy)
        for (int hx = 0; hx < pitch; ++hx) {
          const int wx = x0 + hx, wy = y0 + hy;
          uint32_t wt = 0u;
          if (hx >= 1 && hx <= S && hy >= 1 && hy <= S && wx >= 0 && wx < W && wy >= 0 && wy < H) wt = pr_weight(cost, costmap[(size_t)wy * W + wx], wx == ax && wy == ay);
          w[(size_t)hy * pitch + hx] = (uint16_t)wt;
          f[(size_t)hy * pitch + hx] = (wx == tx && wy == ty) ? 0u : kFieldUnreachable;
        }
      const int last_colour = (R & 1) * 3;
      bool failed = false;
      for (uint32_t sweep = 1;; ++sweep) {
        const uint32_t cap = f[ia];
        bool changed = false;
        for (int ph = 1; ph <= 4; ++ph) {
          const int colour = (last_colour + ph) & 3, cx = colour & 1, cy = colour >> 1;
          const int nx = (S + 1 - cx) >> 1, ny = (S + 1 - cy) >> 1;
          std::vector<uint32_t> next((size_t)nx * ny);    // a phase's lanes all read before any of them writes: the same result
          for (int qy = 0; qy < ny; ++qy)
            for (int qx = 0; qx < nx; ++qx) next[(size_t)qy * nx + qx] = pr_relax(f.data(), w.data(), (2 * qy + cy + 1) * pitch + 2 * qx + cx + 1, pitch, cap);
          for (int qy = 0; qy < ny; ++qy)
            for (int qx = 0; qx < nx; ++qx) {
              uint32_t& cell = f[(size_t)(2 * qy + cy + 1) * pitch + 2 * qx + cx + 1];
              if (cell != next[(size_t)qy * nx + qx]) { cell = next[(size_t)qy * nx + qx]; changed = true; }
            }
        }
        if (!changed) break;
        if (sweep >= (uint32_t)(S * S)) { failed = true; break; }
      }
      const uint32_t fa = f[ia];
      wrote_field = true;
      std::printf("F");
      for (int ry = 0; ry < S; ++ry)
        for (int rx = 0; rx < S; ++rx) std::printf(" %u", pr_field_out(f[(size_t)(ry + 1) * pitch + rx + 1], fa));
      std::printf("\n");
      if (failed) st = kRepairInconsistent;
      else if (fa == kFieldUnreachable) st = kRepairUnreachable;
      else {
        int idx = ia, rx = R, ry = R;
        int32_t steps = 0, K = 0, until = stride;
        uint32_t fc = fa;
        bool bad = false;
        while (fc != 0u) {
          int k = -1;
          for (int l = 0; l < 8 && k < 0; ++l) if (pr_walk_probe(f.data(), w.data(), idx, pitch, l)) k = l;
          if (k < 0 || steps >= S * S) { bad = true; break; }
          idx += pr_offset(k, pitch); rx += gp_dx(k); ry += gp_dy(k);
          fc = f[idx];
          ++steps;
          if (--until == 0) {
            until = stride;
            if (fc != 0u) {
              if (K < L) { ws[2 * (size_t)K] = gp_centre(win.ox, ax - R + rx, win.res); ws[2 * (size_t)K + 1] = gp_centre(win.oy, ay - R + ry, win.res); }
              ++K;
            }
          }
        }
        if (bad) st = kRepairInconsistent;
        else {
          m = steps;
          const int64_t len = pr_new_length(i0, K, n, j);
          if (len > L) st = kRepairTooLong;
          else {
            st = kRepairRepaired;
            const size_t tail = 2 * (size_t)(n - j), moved = 2 * (size_t)K + tail;
            for (size_t r = 0; r < tail; ++r) ws[2 * (size_t)K + r] = rows[2 * (size_t)j + r];
            for (size_t r = 0; r < moved; ++r) rows[2 * ((size_t)i0 + 1) + r] = ws[r];
            rows[2 * (size_t)i0] = x; rows[2 * (size_t)i0 + 1] = y;
            n = (int32_t)len;
          }
        }
      }
    }
    if (!wrote_field) std::printf("-\n");
    std::printf("%d %d %d %d %d %d", st, i0, i1, j, m, n);
    for (double v : rows) std::printf(" %s", hex(v).c_str());
    std::printf("\n");
  }
  return 0;
}
"""


def probe_input(c):
    hx = lambda v: float(v).hex() if np.isfinite(v) else repr(float(v))
    B, L = c["plan"].shape[:2]
    H, W = c["costmap"].shape[-2:]
    cost = c["cost"]
    lines = [" ".join(map(str, [B, L, W, H, int(c["costmap"].ndim == 2), c["R"], c["stride"], int(c["plan_start"] is not None), hx(c["res"]),
                                hx(c["clearance_d2"]), cost.neutral_cost, cost.cost_weight, cost.lethal_min_cost, int(cost.allow_unknown)]))]
    lines.append(" ".join(map(str, c["costmap"].ravel().tolist())))
    lines.append(" ".join(hx(v) for v in np.asarray(c["origin"], np.float64).ravel()))
    for b in range(B):
        s = 0 if c["plan_start"] is None else int(c["plan_start"][b])
        lines.append(" ".join([hx(c["pose"][b, 0]), hx(c["pose"][b, 1]), str(int(c["plan_len"][b])), str(s)]))
        lines.append(" ".join(hx(v) for v in c["plan"][b].ravel()))
    return "\n".join(lines) + "\n"


def probe_output(c, text):
    """The program's lines as plan_repair_ref.run's outputs over its prefill."""
    B, L = c["plan"].shape[:2]
    S_ = 2 * c["R"] + 1
    out = text.splitlines()
    assert len(out) == 2 * B
    got = dict(plan=np.zeros((B, L, 2)), plan_len=np.zeros(B, np.int32), status=np.zeros(B, np.int32), info=np.zeros((B, 4), np.int32),
               field=np.zeros((B, S_, S_), np.uint32))
    for b in range(B):
        if out[2 * b] != "-":
            got["field"][b] = np.array(out[2 * b].split()[1:], np.uint64).astype(np.uint32).reshape(S_, S_)
        w = out[2 * b + 1].split()
        got["status"][b], got["info"][b], got["plan_len"][b] = int(w[0]), [int(v) for v in w[1:5]], int(w[5])
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
    exe = build_probe(tmp_path_factory.mktemp("plan_repair_rule"), "probe")
    return lambda c: probe_output(c, subprocess.run([str(exe)], input=probe_input(c), capture_output=True, text=True, check=True).stdout)


@pytest.mark.parametrize("name", sorted(HAND))
def test_compiled_rule_is_the_yardstick_on_the_hand_made_cases(rule, name):
    got = rule(HAND[name])
    assert R.same(got, R.run(HAND[name]))
    MC.check_want(HAND[name], got)


@pytest.mark.parametrize("name", list(SEEDED))
def test_compiled_rule_is_the_yardstick_on_the_seeded_cases(rule, seeded_ref, name):
    got, want = rule(SEEDED[name]), seeded_ref[name][0]
    for k in ("status", "info", "plan_len", "plan", "field"):
        assert G.same_bits(got[k], want[k]), (k, np.argwhere(got["status"] != want["status"]).ravel().tolist())


def test_the_program_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path, seeded_ref):
    """The stand-alone program (its own main, nothing loaded into Python), built once more with the sanitizers: it exits 0 and
    prints what the plain build prints."""
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    exe = build_probe(tmp_path, "probe_san", ("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"))
    for name in (MC.seeded_name(*MC.SHAPES[0]), MC.seeded_name(*MC.SHAPES[2])):
        r = subprocess.run([str(exe)], input=probe_input(SEEDED[name]), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        assert R.same(probe_output(SEEDED[name], r.stdout), seeded_ref[name][0])
    for name in ("corner", "no_plan", "too_long", "m_zero"):
        r = subprocess.run([str(exe)], input=probe_input(HAND[name]), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        assert R.same(probe_output(HAND[name], r.stdout), R.run(HAND[name]))


def test_the_rule_header_rounds_every_operation_on_its_own_and_reuses_the_global_plans_rule():
    text = open(os.path.join(CSRC, "smpc_plan_repair_rule.hpp")).read()
    assert "#pragma clang fp contract(off)" in text and "fma(" not in text and "hip_runtime" not in text
    assert re.findall(r'#include\s+([<"][^>"]+[>"])', text) == ["<stdint.h>", '"smpc_global_plan_rule.hpp"']
    assert "gp_cell_axis(" in text and "gp_step_cost(" in text and "gp_weight(" in text and "floor(" not in text
    kernel = open(os.path.join(CSRC, "smpc_plan_repair.hpp")).read()
    code = kernel.split("#pragma once")[1]
    assert '#include "smpc_plan_repair_rule.hpp"' in kernel and "atomic" not in code and "__ballot(" in code and "__shfl_xor(" in code
    hip = open(os.path.join(CSRC, "smpc_hip.hip")).read()
    assert '#include "smpc_plan_repair.hpp"' in hip and "smpc::smpc_repair_judge_kernel" in hip and "smpc::smpc_repair_field_kernel" in hip
    entry = hip[hip.index("int smpc_repair_plan_batch("):]
    entry = entry[:entry.index("\n}\n")]
    assert "hipMalloc" not in entry and "Synchronize" not in entry and "hipMemcpy" not in entry     # capturable with device pointers


# ---- the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mirror_matches_the_header_and_the_library_exports_the_function(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src))) == sorted(MA.FUNCTIONS) == ["smpc_repair_plan_batch"]
    assert re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S) == [st.c_name for st in MA.STRUCTS]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' + "".join(f'printf("%zu\\n", offsetof({st.c_name}, {f[0]}));\n' for f in st._fields_)
                   for st in MA.STRUCTS)
    names = ["SMPC_REPAIR_" + n for n in MA.REPAIR_STATUS]
    body += 'printf("%d\\n", (int)SMPC_REPAIR_MAX_RADIUS);\nprintf("%u\\n", (unsigned)SMPC_FIELD_UNREACHABLE);\n' + "".join(f'printf("%d\\n", (int){n});\n' for n in names)
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc_plan_repair.h"\nint main(void){\n' + body + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [v for st in MA.STRUCTS for v in [C.sizeof(st)] + [getattr(st, f[0]).offset for f in st._fields_]]
    assert values == want + [MA.SMPC_REPAIR_MAX_RADIUS, MA.SMPC_FIELD_UNREACHABLE] + [getattr(MA, n) for n in names]
    assert values[-10:] == [63, 0xFFFFFFFF] + list(range(8))
    assert [R.STATUS[v] for v in (R.CLEAR, R.REPAIRED, R.NO_PLAN, R.NO_CELL, R.NO_REJOIN, R.UNREACHABLE_CELL, R.TOO_LONG, R.INCONSISTENT_FIELD)] == MA.REPAIR_STATUS
    for st in MA.STRUCTS:
        fields = re.findall(r"\b(\w+)\s*(?:\[\w+\]\s*)*(?:,|;)", re.search(r"typedef struct %s \{(.*?)\}" % st.c_name, src, flags=re.S).group(1))
        assert fields == [f[0] for f in st._fields_], st.c_name
    assert C.sizeof(MA.SmpcPlanRepairIn) == 8 * 4 + 2 * 8 + 16 + 4 * 8
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
def test_plan_repair_params():
    rp = PlanRepairParams()
    assert (rp.radius, rp.rejoin_clearance, rp.stride, rp.neutral_cost, rp.cost_weight, rp.lethal_min_cost, rp.allow_unknown) == (3.0, 0.5, 2, 50, 1, 253, False)
    assert rp.radius_cells(0.05) == 60 and rp.radius_cells(0.1) == 30 and rp.radius_cells(4.0) == 1 and rp.clearance_d2 == 0.25
    assert PlanRepairParams(radius=3.15).radius_cells(0.05) == 63 and PlanRepairParams(radius=3.2).radius_cells(0.05) == 64
    assert rp.supported() and rp.supported(0.05) and PlanRepairParams(radius=3.15).supported(0.05)
    assert not PlanRepairParams(radius=3.2).supported(0.05) and not rp.supported(0.04)
    heavy = PlanRepairParams(radius=3.15, neutral_cost=50, cost_weight=150)          # 127 * 127 * 7 * 38300 >= 2^32 - 1
    assert not heavy.supported() and not heavy.supported(0.05) and heavy.supported(0.06) and heavy.supported(0.5)
    assert 127 * 127 * 7 * (50 + 255 * 148) < 2 ** 32 - 1 <= 127 * 127 * 7 * (50 + 255 * 150)
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=np.nan), dict(radius=np.inf), dict(rejoin_clearance=-0.1), dict(rejoin_clearance=np.nan),
                dict(stride=0), dict(stride=1.5), dict(neutral_cost=0), dict(cost_weight=-1), dict(neutral_cost=50, cost_weight=257),
                dict(lethal_min_cost=256), dict(lethal_min_cost=-1)):
        with pytest.raises(ValueError):
            PlanRepairParams(**bad)


def test_the_struct_the_call_takes():
    ri = S.BatchSolver.repair_plan_c(PlanRepairParams(allow_unknown=True), 7, 400, 200, 180, False, 0.05, 1)
    assert (ri.B, ri.L, ri.on_device, ri.size_x, ri.size_y, ri.costmap_shared, ri.radius, ri.stride) == (7, 400, 1, 200, 180, 0, 60, 2)
    assert (ri.resolution, ri.clearance_d2) == (0.05, 0.25)
    assert (ri.cost.neutral_cost, ri.cost.cost_weight, ri.cost.lethal_min_cost, ri.cost.allow_unknown) == (50, 1, 253, 1)
    assert not ri.costmap and not ri.costmap_origin and not ri.robot_pose and not ri.plan_start


# ---- the kernels' resources -------------------------------------------------------------------------------------------------
def test_the_kernels_have_no_spills_and_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    r = subprocess.run(["bash", os.path.join(CSRC, "build.sh"), "-DSMPC_ONLY_NB=3", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage"],
                       env={**os.environ, "SMPC_OUT": str(tmp_path / "smpc_nb3.o")}, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = parse_resource_remarks(r.stderr)
    for kernel in (JUDGE, FIELD):
        use = remarks.get(kernel)
        assert use is not None, f"no resource remark for {kernel}"
        print(kernel, use)
        assert use["VGPRs Spill"] == 0 and use["SGPRs Spill"] == 0 and use["ScratchSize [bytes/lane]"] == 0, use   # no private segment
    assert remarks[JUDGE]["LDS Size [bytes/block]"] == 0 and remarks[JUDGE]["VGPRs"] <= 64
    # 16 wavefronts of a workgroup on four SIMDs: 128 registers each; the static LDS is the two stamps and the walk's words
    assert remarks[FIELD]["VGPRs"] <= 128 and remarks[FIELD]["LDS Size [bytes/block]"] <= 64
    assert (2 * 63 + 3) ** 2 * 6 + 64 <= 160 * 1024


# ---- behaviour, on the yardsticks of the scan and of this stage alone ----------------------------------------------------------
RES, ORIGIN = 0.05, (0.0, 0.0)
SENSOR = SensorParams()
FLOOR = np.zeros((160, 160), np.uint8)                   # 8 m x 8 m, open


def sensed_window(robot_xy, persons):
    """The floor with what one scan from robot_xy marks of the persons: the cells the beams stopped at, lethal (the scan's
    yardstick, tests/sensed_costmap_ref.py; no inflation: the plan repair asks only which cells are impassable)."""
    people = np.zeros((max(len(persons), 1), 5))
    people[:len(persons), :2] = persons
    occupied = sensed_costmap_ref.occupied_cells(people, len(persons), ORIGIN, RES, SENSOR.agent_d2(RES))
    a = sensed_costmap_ref.point_cell(robot_xy[0], robot_xy[1], ORIGIN, RES)
    window = FLOOR.copy()
    hits = 0
    for off in SENSOR.beam_cells(RES):
        kind, o, _ = sensed_costmap_ref.cast(FLOOR, occupied, a, off)
        if kind in (2, 3):                               # AGENT, CORNER_PAIR
            window[a[1] + o[1], a[0] + o[0]] = 254
            hits += 1
    return window, hits


def test_a_straight_plan_through_a_standing_person_is_led_around():
    rp = PlanRepairParams()
    robot, person = (2.025, 4.025), (3.525, 4.025)                       # 1.5 m ahead
    window, hits = sensed_window(robot, [person])
    assert hits >= 5
    L = 400
    line = np.stack([np.arange(1.525, 7.5, 0.05), np.full(120, 4.025)], axis=1)
    plan = np.full((1, L, 2), np.nan)
    plan[0, :len(line)] = line
    case = dict(costmap=window, origin=np.array(ORIGIN), res=RES, pose=np.array([[robot[0], robot[1], 0.0]]), plan=plan,
                plan_len=np.array([len(line)], np.int32), plan_start=None, R=rp.radius_cells(RES), stride=rp.stride, clearance_d2=rp.clearance_d2,
                cost=G.Cost(rp.neutral_cost, rp.cost_weight, rp.lethal_min_cost, rp.allow_unknown))
    got = R.run(case)
    assert got["status"][0] == R.REPAIRED, R.STATUS[got["status"][0]]
    i0, i1, j, m = got["info"][0]
    n = got["plan_len"][0]
    new = got["plan"][0, :n]
    assert i0 == 10 and line[i1, 0] < person[0] < line[j, 0] and m >= j - i0
    # no pose of the new plan in view is blocked
    passable = G.passable(window, case["cost"])
    a = G.cell_of(robot, ORIGIN, RES, 160, 160)
    for p in new[i0:]:
        c = G.cell_of(p, ORIGIN, RES, 160, 160)
        if c is None or max(abs(c[0] - a[0]), abs(c[1] - a[1])) > case["R"]:
            break
        assert passable[c[1], c[0]], p
    # consecutive detour poses: stride cells apart at the most, a cell's diagonal each, plus the rounding: a centre's
    # coordinate is a rounded product plus a rounded sum, within one unit in the last place of the floor's 8 m of the exact
    # centre, so a difference of two is within two, a gap within 2 * sqrt(2) of them; hypot adds a relative 2^-52 or so
    ulp = np.spacing(8.0)
    K = n - i0 - 1 - (len(line) - j)
    detour = new[i0 + 1:i0 + 1 + K]
    assert K == (m - 1) // rp.stride
    gaps = np.hypot(*np.diff(detour, axis=0).T)
    assert gaps.max() <= rp.stride * np.sqrt(2.0) * RES * (1 + 2 ** -50) + 4 * ulp
    assert np.hypot(*(detour[0] - new[i0])) <= (rp.stride * np.sqrt(2.0) + np.sqrt(0.5)) * RES * (1 + 2 ** -50) + 4 * ulp   # from anywhere in its cell
    # a second call on the result is CLEAR
    again = R.run({**case, "plan": got["plan"], "plan_len": got["plan_len"]})
    assert again["status"][0] == R.CLEAR and G.same_bits(again["plan"], got["plan"])


# ---- the episode ------------------------------------------------------------------------------------------------------------
def test_the_episode_declares_the_argument_and_refuses_what_it_must():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode, TickRecord, shard_kwargs
    assert "repair" in BatchEpisode.FORWARDED and "repair" not in BatchEpisode.PER_ROBOT
    assert inspect.signature(BatchEpisode.__init__).parameters["repair"].default is None
    fields = TickRecord.__dataclass_fields__
    assert all(fields[name].default is None for name in ("repair_plan_before", "repair_plan_len_before", "repair_plan_after", "repair_plan_len_after",
                                                         "repair_status", "repair_info"))
    from nav2_social_mpc_controller_amd.episode_stages import Repair
    assert Repair.TIMING == "repair" and BatchEpisode.STAGES.count(Repair) == 1
    rp = PlanRepairParams()
    assert shard_kwargs({"repair": rp}, np.arange(2), 4)["repair"] is rp and "shard_kwargs" in inspect.getsource(ShardedEpisode.__init__)
    BatchEpisode.check_repair(rp, True, 0.05)
    with pytest.raises(ValueError, match=re.escape("repair needs plan= or planner=: there is no plan to repair")):
        BatchEpisode.check_repair(rp, False, 0.05)
    for bad in (dict(radius=3.0), None, PlanRepairParams(radius=4.0), PlanRepairParams(radius=3.15, cost_weight=150)):
        with pytest.raises(ValueError):
            BatchEpisode.check_repair(bad, True, 0.05)
