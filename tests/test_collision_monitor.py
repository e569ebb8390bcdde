"""The collision monitor on the CPU: the yardstick itself (tests/collision_monitor_ref.py: every point, every zone, every step)
on hand-made cases with the expected result written out, what the seeded cases exercise, the `__host__ __device__` rule of
csrc/smpc_collision_monitor_rule.hpp compiled into a host-only program and composed as the kernel composes it (points in
passes of 64 lanes and chunks of eight, counts as sums of per-pass popcounts, the two reach filters and both early exits) against
the yardstick bit for bit given the program's own cosines and sines, those held against numpy's, the same program under the
address and undefined-behaviour sanitizers, the ctypes mirror against include/smpc_collision_monitor.h, MonitorParams, the
episode's declarations and refusals, the kernel's resource remarks, and what the monitor does to a robot that drives at a
wall, on the yardsticks of the scan, the plant and the monitor alone."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import collision_monitor_cases as MC
import collision_monitor_ref as R
import plant_ref
import sensed_costmap_ref
from nav2_social_mpc_controller_amd import _abi_collision_monitor as MA
from nav2_social_mpc_controller_amd import solver as S
from nav2_social_mpc_controller_amd.params import MonitorParams, MonitorZone, SensorParams
from test_kernel_budget import CSRC, HIPCC, parse_resource_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc_collision_monitor.h")
KERNELS = ["_ZN4smpc29smpc_collision_monitor_kernelILb1EEEvNS_13MonitorParamsE", "_ZN4smpc29smpc_collision_monitor_kernelILb0EEEvNS_13MonitorParamsE"]

HAND = MC.hand_cases()
SEEDED = MC.seeded_cases()


def ref_with_numpy_angles(c):
    cs, cs1 = R.numpy_angles(c["pose"], c["cmd"], c["p"]["sim_dt"])
    return R.run(c["p"], c["pose"], c["cmd"], c["kind"], c["cell"], cs, cs1)


@pytest.fixture(scope="module")
def seeded_ref():
    return {name: ref_with_numpy_angles(c) for name, c in SEEDED.items()}


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_cases_end_where_the_contract_says(name):
    c = HAND[name]
    assert c["p"]["res"] == 0.125 and c["p"]["origin"] == (0.0, 0.0)
    got = ref_with_numpy_angles(c)
    MC.check_want(c, got)
    assert got["cmd_out"].dtype == np.float64 and got["action"].dtype == np.int32 and got["zone_points"].dtype == np.int32


def test_the_wall_ahead_stops_the_straight_run_and_not_the_arc():
    got = ref_with_numpy_angles(HAND["wall_ahead"])
    assert list(got["zone_step"][:, 0]) == [7, -1, -1] and list(got["zone_counts"][0, 0]) == [0] * 7 + [4, 4]
    assert got["zone_counts"][1].max() == 0 and got["zone_counts"][2].max() == 0


def test_the_main_seeded_case_exercises_the_rule(seeded_ref):
    """By the yardstick alone, before anything is compared with it: 64 robots x 360 beams x 8 zones, 12 steps."""
    c, got = SEEDED[MC.MAIN], seeded_ref[MC.MAIN]
    zones, M = c["p"]["zones"], c["p"]["M"]
    assert c["kind"].shape == (64, 360) and len(zones) == 8 and M == 12
    assert {z["shape"] for z in zones} == {R.CIRCLE, R.POLYGON} and {z["n"] for z in zones} >= {0, 3, 16}
    action = got["action"]
    assert set(np.unique(action[:, 0])) >= {0, 1, 2, 4, 8, 16, 32}, np.unique(action[:, 0])      # every action decides, BAD_INPUT, NO_CELL
    assert (action[:, 1] == -1).sum() >= 8 and (got["ratio"] == 1.0).sum() >= 8
    steps = got["zone_step"][:, 1]                                                                # the main shape: the 16-gon APPROACH zone
    assert zones[1]["action"] == R.APPROACH and zones[1]["n"] == 16
    assert set(steps.tolist()) >= set(range(-1, M + 1)), sorted(set(steps.tolist()))
    approach = [zi for zi, z in enumerate(zones) if z["action"] == R.APPROACH]
    assert len(approach) == 3 and any((action[:, 1] == zi).any() and (action[action[:, 1] == zi, 2] > 0).any() for zi in approach)
    exactly = missed = 0
    for zi, z in enumerate(zones):
        top = got["zone_counts"][got["finite"], zi].max(axis=1)
        at_step = np.array([got["zone_counts"][b, zi, s] if s >= 0 else -1 for b, s in enumerate(got["zone_step"][:, zi])])
        exactly += int((at_step == z["min_points"]).sum())
        missed += int((top == z["min_points"] - 1).sum()) if z["min_points"] > 1 else 0
    assert exactly >= 1 and missed >= 1, (exactly, missed)
    assert 0.0 < got["ratio"][got["ratio"] > 0].min() < 0.2 and ((got["ratio"] > 0) & (got["ratio"] < 1)).sum() >= 10
    assert (action[got["finite"], 3] > 0).sum() >= 55 and action[9, 3] == 0 and action[5, 0] == 32


def test_every_seeded_case_is_what_its_name_says(seeded_ref):
    for name, c in SEEDED.items():
        B, n, got = int(name.split("_")[0][1:]), int(name.split("_")[1][1:]), seeded_ref[name]
        assert c["kind"].shape == (B, n) and c["cell"].shape == (B, n, 2) and c["pose"].shape == (B, 3), name
        assert c["p"]["M"] == int(re.search(r"_M(\d+)", name).group(1)) and len(c["p"]["zones"]) == int(re.search(r"_Z(\d+)", name).group(1)), name
        if "never" in name or name == "B16_n360_Z8_M0":                # the last zone asks for more points than there are beams
            assert all(z["min_points"] > n for z in c["p"]["zones"][-1:]) and (got["zone_step"][:, -1] == -1).all(), name
        if "never" not in name:
            assert (got["ratio"] < 1.0).any() and (got["ratio"] == 1.0).any(), name
    assert {int(n.split("_")[1][1:]) for n in SEEDED} == {1, 63, 64, 65, 360, 512, 513, 4096}
    assert {int(re.search(r"_M(\d+)", n).group(1)) for n in SEEDED} == {0, 1, 12, 32}


# ---- the compiled rule ------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <string>
#include <vector>
#include "smpc_collision_monitor_rule.hpp"

static double num(const std::string& s) { return std::strtod(s.c_str(), nullptr); }   // hex floats, nan, inf
static std::string hex(double v) { char b[40]; uint64_t u; std::memcpy(&u, &v, 8); std::snprintf(b, sizeof b, "%016llx", (unsigned long long)u); return b; }
static double rd() { std::string w; std::cin >> w; return num(w); }
static long long ri() { long long v; std::cin >> v; return v; }

// The scalars and the zones, then one robot per record, composed as the kernel composes the rule: 64 "lanes" take the beams
// in chunks of eight slots, a slot without a point holds a NaN, a count is the sum of the slots' "ballots", the pass of step
// 0 counts the points within the zone's reach, a zone with too few of them is not simulated, a polygon walks its edges only
// for the slots that hold a point within the disc around it, and the approach loop ends at the first triggering step and
// before a step that could not decide.
constexpr int kSlots = 8, kLanes = 64;
struct Chunk { double px[kSlots][kLanes], py[kSlots][kLanes]; int slots; };

int main() {
  const int Z = (int)ri(), M = (int)ri(), n_beams = (int)ri(), B = (int)ri();
  const double sim_dt = rd(), res = rd(), ox = rd(), oy = rd();
  if (Z < 1 || Z > smpc::kMonitorMaxZones || M < 0 || M > smpc::kMonitorMaxSteps || n_beams < 1 || n_beams > 4096) std::abort();
  std::vector<smpc::MonitorZone> zones((size_t)Z);
  for (auto& z : zones) {
    std::memset(&z, 0, sizeof z);
    z.shape = (int32_t)ri(); z.action = (int32_t)ri(); z.n = (int32_t)ri(); z.min_points = (int32_t)ri();
    const double radius = rd();
    z.slowdown_ratio = rd(); z.linear_limit = rd(); z.angular_limit = rd();
    if (z.n < 0 || z.n > smpc::kMonitorMaxVertices) std::abort();
    for (int i = 0; i < z.n; ++i) { z.vx[i] = rd(); z.vy[i] = rd(); }
    z.radius2 = smpc::cm_radius2(radius);
    z.bound = smpc::cm_bound(z.shape, radius, z.n, z.vx, z.vy);
  }
  smpc::MathTab tab;
  smpc::fill_math_table(&tab);
  const smpc::MathTab* mt = &tab;
  std::vector<long long> kind((size_t)n_beams);
  std::vector<int32_t> cell((size_t)n_beams * 2);
  const int per_chunk = kSlots * kLanes, chunks = (n_beams + per_chunk - 1) / per_chunk;
  std::vector<Chunk> chunk((size_t)chunks);
  for (int b = 0; b < B; ++b) {
    const double x = rd(), y = rd(), th = rd(), v = rd(), w = rd();
    for (auto& k : kind) k = ri();
    for (auto& c : cell) c = (int32_t)ri();
    if (!(smpc::cm_finite(x) && smpc::cm_finite(y) && smpc::cm_finite(th) && smpc::cm_finite(v) && smpc::cm_finite(w))) {
      std::printf("%s %s %d -1 -1 0 %s - - - -", hex(0.0).c_str(), hex(0.0).c_str(), smpc::kMonitorBadInput, hex(0.0).c_str());
      for (int z = 0; z < Z; ++z) std::printf(" 0");
      std::printf("\n");
      continue;
    }
    double c, s, c1 = 1.0, s1 = 0.0;
    smpc::cm_heading(mt, th, &c, &s);
    if (M > 0) smpc::cm_heading(mt, smpc::cm_step_angle(w, sim_dt), &c1, &s1);
    int32_t ax = 0, ay = 0;
    const bool has_cell = smpc::cm_robot_cell(x, y, ox, oy, res, &ax, &ay);
    int points = 0;
    for (int q = 0; q < chunks; ++q) {
      Chunk& ch = chunk[(size_t)q];
      const int first = q * per_chunk, left = n_beams - first;
      ch.slots = left >= per_chunk ? kSlots : (left + 63) / 64;
      for (int j = 0; j < kSlots; ++j)
        for (int lane = 0; lane < kLanes; ++lane) {
          ch.px[j][lane] = ch.py[j][lane] = std::numeric_limits<double>::quiet_NaN();
          const int k = first + 64 * j + lane;
          if (j < ch.slots && has_cell && k < n_beams && smpc::cm_is_hit((uint32_t)(uint8_t)kind[(size_t)k])) {
            const double rx = smpc::cm_rel(ox, ax, cell[2 * (size_t)k], res, x), ry = smpc::cm_rel(oy, ay, cell[2 * (size_t)k + 1], res, y);
            smpc::cm_to_frame(c, s, rx, ry, &ch.px[j][lane], &ch.py[j][lane]);
            ++points;
          }
        }
    }
    auto count = [&](const smpc::MonitorZone& z, bool moved, double X, double Y, double C, double S, double near2, double reach2, bool first,
                     int* reach) {
      int cnt = 0;
      for (const Chunk& ch : chunk)
        for (int j = 0; j < ch.slots; ++j) {
          double qx[kLanes], qy[kLanes];
          int ballot = 0, within = 0, near = 0;
          for (int lane = 0; lane < kLanes; ++lane) {
            qx[lane] = ch.px[j][lane]; qy[lane] = ch.py[j][lane];
            if (moved) smpc::cm_step_point(ch.px[j][lane], ch.py[j][lane], X, Y, C, S, &qx[lane], &qy[lane]);
            near += smpc::cm_within_reach(qx[lane], qy[lane], near2);
            within += first && smpc::cm_within_reach(ch.px[j][lane], ch.py[j][lane], reach2);
          }
          if (first) *reach += within;
          if (z.shape != smpc::kMonitorCircle && near == 0) continue;   // a polygon walks its edges only for a slot with a point in its disc
          for (int lane = 0; lane < kLanes; ++lane) {
            bool in = false;
            if (z.shape == smpc::kMonitorCircle) {
              in = smpc::cm_in_circle(qx[lane], qy[lane], z.radius2);
            } else {   // edges outside, points inside in the kernel: the same parity
              double vjx = z.vx[z.n - 1], vjy = z.vy[z.n - 1];
              for (int i = 0; i < z.n; ++i) { in ^= smpc::cm_edge_counts(z.vx[i], z.vy[i], vjx, vjy, qx[lane], qy[lane]); vjx = z.vx[i]; vjy = z.vy[i]; }
              if (in != smpc::cm_in_polygon(&z, qx[lane], qy[lane])) std::abort();
            }
            ballot += in;
          }
          cnt += ballot;
        }
      return cnt;
    };
    double best = 1.0;
    int decide = -1, dstep = -1, by = 0;
    std::vector<int> zone_points((size_t)Z);
    for (int zi = 0; zi < Z; ++zi) {
      const smpc::MonitorZone& z = zones[(size_t)zi];
      const double reach2 = smpc::cm_reach2(z.bound, v, z.action == smpc::kMonitorApproach ? M : 0, sim_dt);
      const double near2 = smpc::cm_reach2(z.bound, v, 0, sim_dt);
      double X = 0.0, Y = 0.0, C = 1.0, S = 0.0, ratio = 1.0, f = 0.0;
      int step = -1, reach = 0;
      for (int m = 0;;) {
        const int cnt = count(z, m > 0, X, Y, C, S, near2, reach2, m == 0, &reach);
        if (m == 0) zone_points[(size_t)zi] = cnt;
        if (cnt >= z.min_points) {
          step = m;
          ratio = z.action == smpc::kMonitorStop ? 0.0 : z.action == smpc::kMonitorSlowdown ? z.slowdown_ratio
                : z.action == smpc::kMonitorLimit ? smpc::cm_limit_ratio(v, w, z.linear_limit, z.angular_limit) : f;
          break;
        }
        if (z.action != smpc::kMonitorApproach || reach < z.min_points || m == M) break;
        ++m;
        f = smpc::cm_step_ratio(m, M);
        if (!(f < best)) break;
        smpc::cm_advance(v, sim_dt, c1, s1, &X, &Y, &C, &S);
      }
      if (ratio < best) { best = ratio; decide = zi; dstep = step; by = 1 << z.action; }
    }
    std::printf("%s %s %d %d %d %d %s %s %s", hex(smpc::cm_scale(v, best)).c_str(), hex(smpc::cm_scale(w, best)).c_str(),
                by | (has_cell ? 0 : smpc::kMonitorNoCell), decide, dstep, points, hex(best).c_str(), hex(c).c_str(), hex(s).c_str());
    if (M > 0) std::printf(" %s %s", hex(c1).c_str(), hex(s1).c_str()); else std::printf(" - -");
    for (int z = 0; z < Z; ++z) std::printf(" %d", zone_points[(size_t)z]);
    std::printf("\n");
  }
  return 0;
}
"""


def probe_input(c):
    hx = lambda v: float(v).hex() if np.isfinite(v) else repr(float(v))
    p = c["p"]
    B, n = c["kind"].shape
    lines = [" ".join(map(str, [len(p["zones"]), p["M"], n, B, hx(p["sim_dt"]), hx(p["res"]), hx(p["origin"][0]), hx(p["origin"][1])]))]
    for z in p["zones"]:
        lines.append(" ".join(map(str, [z["shape"], z["action"], z["n"], z["min_points"], hx(z["radius"]), hx(z["slowdown_ratio"]), hx(z["linear_limit"]),
                                        hx(z["angular_limit"])] + [hx(v) for v in z["vertices"].ravel()])))
    for b in range(B):
        lines.append(" ".join([hx(v) for v in list(c["pose"][b]) + list(c["cmd"][b])]))
        lines.append(" ".join(map(str, c["kind"][b].tolist())))
        lines.append(" ".join(map(str, c["cell"][b].ravel().tolist())))
    return "\n".join(lines) + "\n"


def probe_output(c, text):
    """The program's lines as collision_monitor_ref.run's keys plus heading_cs / step_cs (NaN rows where it printed none)."""
    B, Z = len(c["pose"]), len(c["p"]["zones"])
    out = text.splitlines()
    assert len(out) == B
    f64 = lambda words: np.array([int(w, 16) for w in words], np.uint64).view(np.float64)
    got = dict(cmd_out=np.zeros((B, 2)), action=np.zeros((B, 4), np.int32), zone_points=np.zeros((B, Z), np.int32), ratio=np.zeros(B),
               heading_cs=np.full((B, 2), np.nan), step_cs=np.full((B, 2), np.nan))
    for b, line in enumerate(out):
        w = line.split()
        assert len(w) == 11 + Z
        got["cmd_out"][b], got["action"][b], got["ratio"][b] = f64(w[0:2]), [int(v) for v in w[2:6]], f64(w[6:7])[0]
        if w[7] != "-":
            got["heading_cs"][b] = f64(w[7:9])
        if w[9] != "-":
            got["step_cs"][b] = f64(w[9:11])
        got["zone_points"][b] = [int(v) for v in w[11:]]
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
    exe = build_probe(tmp_path_factory.mktemp("monitor_rule"), "probe")
    return lambda c: probe_output(c, subprocess.run([str(exe)], input=probe_input(c), capture_output=True, text=True, check=True).stdout)


def held_to_the_yardstick(c, got):
    """`got` (a call's outputs with its heading_cs and step_cs) against the yardstick fed those four numbers."""
    p, M = c["p"], c["p"]["M"]
    want = R.run(p, c["pose"], c["cmd"], c["kind"], c["cell"], got["heading_cs"], got["step_cs"])
    assert R.same(got, want)
    assert R.angles_close(got["heading_cs"], got["step_cs"], c["pose"], c["cmd"], p["sim_dt"], M)
    fin = want["finite"]
    assert np.isfinite(got["heading_cs"][fin]).all() and np.isnan(got["heading_cs"][~fin]).all()
    assert np.isnan(got["step_cs"][~fin]).all() and (np.isfinite(got["step_cs"][fin]).all() if M > 0 else np.isnan(got["step_cs"]).all())
    return want


@pytest.mark.parametrize("name", sorted(HAND))
def test_compiled_rule_is_the_yardstick_on_the_hand_made_cases(rule, name):
    got = rule(HAND[name])
    held_to_the_yardstick(HAND[name], got)
    MC.check_want(HAND[name], got)


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_compiled_rule_is_the_yardstick_on_the_seeded_cases(rule, name):
    held_to_the_yardstick(SEEDED[name], rule(SEEDED[name]))


def test_the_program_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The stand-alone program (its own main, nothing loaded into Python), built once more with the sanitizers, on the main
    seeded case: it exits 0 and prints what the plain build prints."""
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    exe = build_probe(tmp_path, "probe_san", ("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"))
    c = SEEDED[MC.MAIN]
    r = subprocess.run([str(exe)], input=probe_input(c), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    held_to_the_yardstick(c, probe_output(c, r.stdout))


def test_the_rule_header_rounds_every_operation_on_its_own():
    text = open(os.path.join(CSRC, "smpc_collision_monitor_rule.hpp")).read()
    assert text.count("#pragma clang fp contract(off)") >= 14 and "fma(" not in text and "hip_runtime" not in text
    assert re.findall(r'#include\s+([<"][^>"]+[>"])', text) == ["<stdint.h>", '"smpc_math.hpp"']
    kernel = open(os.path.join(CSRC, "smpc_collision_monitor.hpp")).read()
    code = kernel.split("#pragma once")[1]
    assert '#include "smpc_collision_monitor_rule.hpp"' in kernel and "SMPC_CHAIN_PRIORITY();" in kernel
    assert "atomic" not in code and "__shared__" not in code and "__ballot(" in code and "__popcll(" in code
    assert " / " not in re.search(r"cm_edge_counts\(.*?\n}", text, flags=re.S).group(0)        # the polygon test has no division


# ---- the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mirror_matches_the_header_and_the_library_exports_the_function(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src))) == sorted(MA.FUNCTIONS) == ["smpc_collision_monitor_batch"]
    assert re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S) == [st.c_name for st in MA.STRUCTS]
    consts = ["SMPC_MONITOR_MAX_ZONES", "SMPC_MONITOR_MAX_VERTICES", "SMPC_MONITOR_MAX_STEPS", "SMPC_MONITOR_CIRCLE", "SMPC_MONITOR_POLYGON",
              "SMPC_MONITOR_STOP", "SMPC_MONITOR_SLOWDOWN", "SMPC_MONITOR_LIMIT", "SMPC_MONITOR_APPROACH", "SMPC_MONITOR_BY_STOP",
              "SMPC_MONITOR_BY_SLOWDOWN", "SMPC_MONITOR_BY_LIMIT", "SMPC_MONITOR_BY_APPROACH", "SMPC_MONITOR_BAD_INPUT", "SMPC_MONITOR_NO_CELL"]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' + "".join(f'printf("%zu\\n", offsetof({st.c_name}, {f[0]}));\n' for f in st._fields_)
                   for st in MA.STRUCTS)
    body += "".join(f'printf("%d\\n", (int){name});\n' for name in consts)
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc_collision_monitor.h"\nint main(void){\n' + body + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [v for st in MA.STRUCTS for v in [C.sizeof(st)] + [getattr(st, f[0]).offset for f in st._fields_]]
    assert values == want + [getattr(MA, name) for name in consts] and values[-15:] == [8, 16, 32, 0, 1, 0, 1, 2, 3, 1, 2, 4, 8, 16, 32]
    for st in MA.STRUCTS:
        fields = re.findall(r"\b(\w+)\s*(?:\[\w+\]\s*)*(?:,|;)", re.search(r"typedef struct %s \{(.*?)\}" % st.c_name, src, flags=re.S).group(1))
        assert fields == [f[0] for f in st._fields_], st.c_name
    assert C.sizeof(MA.SmpcMonitorZone) == 16 + 4 * 8 + 16 * 2 * 8 and C.sizeof(MA.SmpcCollisionMonitorIn) == 24 + 4 * 8 + 5 * 8
    assert (R.STOP, R.SLOWDOWN, R.LIMIT, R.APPROACH, R.FLAG_BAD_INPUT, R.FLAG_NO_CELL) == (0, 1, 2, 3, MA.SMPC_MONITOR_BAD_INPUT, MA.SMPC_MONITOR_NO_CELL)
    assert (R.KIND_NONE, R.KIND_WORLD, R.KIND_AGENT, R.KIND_CORNER_PAIR, R.KIND_INVALID, R.KIND_NO_ROBOT) == (0, 1, 2, 3, 4, 5)
    assert "SMPC_SENSED_MAX_BEAMS 4096" in open(os.path.join(ROOT, "include", "smpc_sensed_costmap.h")).read()
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
def test_monitor_params():
    z = MonitorZone(action="stop", radius=0.3)
    assert (z.shape, z.min_points, z.slowdown_ratio, z.linear_limit, z.angular_limit) == ("circle", 4, 0.5, 0.5, 0.5)
    sq = MonitorZone(action="approach", vertices=[(0, 0), (1, 0), (1, 1)], min_points=1)
    assert sq.shape == "polygon" and sq.vertices == ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0))
    for bad in (dict(action="halt", radius=0.3), dict(action="stop"), dict(action="stop", radius=0.3, vertices=[(0, 0), (1, 0), (1, 1)]),
                dict(radius=-0.1), dict(radius=np.inf), dict(radius=np.nan), dict(vertices=[(0, 0), (1, 0)]), dict(vertices=[(0, 0)] * 17),
                dict(vertices=[(0, 0), (1, np.nan), (1, 1)]), dict(vertices=[0.0, 1.0, 2.0]), dict(radius=0.3, min_points=0),
                dict(radius=0.3, min_points=1.5), dict(radius=0.3, slowdown_ratio=1.1), dict(radius=0.3, slowdown_ratio=-0.1),
                dict(radius=0.3, slowdown_ratio=np.nan), dict(radius=0.3, linear_limit=-1.0), dict(radius=0.3, angular_limit=np.nan)):
        with pytest.raises(ValueError):
            MonitorZone(**bad)
    mp = MonitorParams(zones=[z, sq])
    assert (mp.time_before_collision, mp.simulation_time_step, mp.steps()) == (1.2, 0.1, 12) and mp.supported() and mp.zones == (z, sq)
    assert MonitorParams(zones=[z], time_before_collision=0.0).steps() == 0
    assert MonitorParams(zones=[sq], time_before_collision=3.2, simulation_time_step=0.1).supported()
    assert not MonitorParams(zones=[sq], time_before_collision=3.3, simulation_time_step=0.1).supported()
    assert not MonitorParams(zones=[z] * 9).supported() and MonitorParams(zones=[z] * 8).supported()
    for bad in (dict(zones=[]), dict(zones=[z, "zone"]), dict(zones=[z], time_before_collision=-1.0), dict(zones=[z], time_before_collision=np.nan),
                dict(zones=[z], simulation_time_step=0.0), dict(zones=[z], simulation_time_step=np.inf), dict(zones=[sq], time_before_collision=0.0)):
        with pytest.raises(ValueError):
            MonitorParams(**bad)
    for bad in (0.0, -0.2, np.nan, np.inf):
        with pytest.raises(ValueError):
            MonitorParams.nav2_like(bad)


def test_the_preset_and_the_struct_the_call_takes():
    mp = MonitorParams.nav2_like(0.24)
    stop, slow, appr = mp.zones
    assert (stop.action, stop.shape, slow.action, slow.shape, appr.action, appr.shape) == ("stop", "circle", "slowdown", "polygon", "approach", "polygon")
    assert stop.radius == pytest.approx(0.3) and stop.radius > 0.24 and slow.slowdown_ratio == 0.5 and mp.steps() == 12 and mp.supported()
    sv, av = np.array(slow.vertices), np.array(appr.vertices)
    assert sv[:, 0].max() == pytest.approx(1.2) and sv[:, 0].max() > stop.radius and np.abs(sv[:, 1]).max() == pytest.approx(0.48)   # larger, ahead
    assert len(av) == 8 and np.allclose(np.hypot(av[:, 0], av[:, 1]), 0.24 / np.cos(np.pi / 8))                                     # around the disc
    mid = (av + np.roll(av, -1, axis=0)) / 2
    assert np.allclose(np.hypot(mid[:, 0], mid[:, 1]), 0.24)
    mi = S.BatchSolver.collision_monitor_c(mp, 7, 360, 1, 0.05, (-1.0, -0.5))
    assert (mi.B, mi.n_beams, mi.Z, mi.M, mi.on_device, mi.reserved, mi.sim_dt, mi.resolution) == (7, 360, 3, 12, 1, 0, 0.1, 0.05)
    assert tuple(mi.world_origin) == (-1.0, -0.5) and mi.zones == C.addressof(mi._zones) and not mi.robot_pose and not mi.cmd and not mi.beam_kind
    zc = mi._zones
    assert [(q.shape, q.action, q.n_vertices, q.min_points) for q in zc] == [(0, 0, 0, 4), (1, 1, 4, 4), (1, 3, 8, 4)]
    assert zc[0].radius == stop.radius and zc[1].slowdown_ratio == 0.5 and [tuple(v) for v in zc[2].vertices][:8] == list(appr.vertices)
    assert all(tuple(v) == (0.0, 0.0) for v in list(zc[2].vertices)[8:])


def test_the_episode_declares_the_argument_and_refuses_what_the_library_would():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode, TickRecord, shard_kwargs
    assert "monitor" in BatchEpisode.FORWARDED and "monitor" not in BatchEpisode.PER_ROBOT
    assert inspect.signature(BatchEpisode.__init__).parameters["monitor"].default is None
    fields = TickRecord.__dataclass_fields__
    assert all(fields[name].default is None for name in ("cmd_safe", "monitor_action", "monitor_points", "monitor_ratio", "monitor_heading_cs", "monitor_step_cs"))
    from nav2_social_mpc_controller_amd.episode_stages import Core, Crowd, Monitor, Plant
    at = BatchEpisode.STAGES.index                                                              # the launch order: Core ends with the command selection
    assert at(Core) < at(Monitor) < at(Crowd) < at(Plant) and Monitor.TIMING == "monitor"
    mp = MonitorParams.nav2_like()
    assert shard_kwargs({"monitor": mp}, np.arange(2), 4)["monitor"] is mp and "shard_kwargs" in inspect.getsource(ShardedEpisode.__init__)
    BatchEpisode.check_monitor(mp, SensorParams())
    with pytest.raises(ValueError, match=re.escape("monitor needs sensor=SensorParams(...): it reads the scan")):
        BatchEpisode.check_monitor(mp, None)
    zone = MonitorZone(action="approach", radius=0.3)
    for bad in (dict(zones=[zone]), None, MonitorParams(zones=[zone] * 9), MonitorParams(zones=[zone], time_before_collision=4.0)):
        with pytest.raises(ValueError):
            BatchEpisode.check_monitor(bad, SensorParams())


# ---- the kernel's resources ------------------------------------------------------------------------------------------------
def test_the_kernels_have_no_spills_no_scratch_and_no_lds(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    r = subprocess.run(["bash", os.path.join(CSRC, "build.sh"), "-DSMPC_ONLY_NB=3", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage"],
                       env={**os.environ, "SMPC_OUT": str(tmp_path / "smpc_nb3.o")}, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = parse_resource_remarks(r.stderr)
    for kernel in KERNELS:
        use = remarks.get(kernel)
        assert use is not None, f"no resource remark for {kernel}"
        print(kernel, use)
        assert use["VGPRs Spill"] == 0 and use["SGPRs Spill"] == 0 and use["ScratchSize [bytes/lane]"] == 0, use   # no private segment
        assert use["LDS Size [bytes/block]"] == 0, use
    resident = remarks[KERNELS[0]]                                            # the kernel of n_beams <= 512: four waves per SIMD
    assert resident["VGPRs"] <= 128 and resident["Occupancy [waves/SIMD]"] >= 4, resident


# ---- behaviour, on the yardsticks alone -------------------------------------------------------------------------------------
def drive_at_the_wall(zones=None, M=0, ticks=48):
    """A robot on a floor of 64 x 24 cells of 0.125 m with a wall across at column 28 drives at it from cell (8, 12) under the
    constant command (0.5, 0), in periods of 0.125 s: every tick the scan's yardstick casts 72 beams of 20 cells, the
    monitor's yardstick (with `zones`) judges the command, the plant's yardstick (a disc of 2 cells, no rate limits)
    executes it. Returns per tick (plant flags, executed v, ratio)."""
    res, origin = 0.125, (0.0, 0.0)
    world = np.zeros((24, 64), np.uint8)
    world[:, 28] = 254
    beams = np.unique(np.round(20 * np.stack([np.cos(np.arange(72) * np.pi / 36), np.sin(np.arange(72) * np.pi / 36)], axis=1)).astype(np.int32), axis=0)
    pp = plant_ref.params(S=4, L=0, dt=0.125, v_min=-0.6, v_max=0.6, w_max=1.4, world=world, origin=origin, res=res, footprint_d2=4, outside_is_wall=False)
    mp = None if zones is None else R.params(zones, M=M, sim_dt=0.125, res=res, origin=origin)
    state = plant_ref.zero_state(1)
    state[0][0] = (8.5 * res, 12.5 * res, 0.0)
    cmd = np.array([[0.5, 0.0]])
    out = []
    for _ in range(ticks):
        pose = state[0].copy()
        ratio = 1.0
        safe = cmd
        if mp is not None:
            a = sensed_costmap_ref.point_cell(pose[0, 0], pose[0, 1], origin, res)
            cast = [sensed_costmap_ref.cast(world, set(), a, off) for off in beams]
            kind = np.array([[k for k, _, _ in cast]], np.uint8)
            cell = np.array([[o for _, o, _ in cast]], np.int32)
            cs, cs1 = R.numpy_angles(pose, cmd, 0.125)
            got = R.run(mp, pose, cmd, kind, cell, cs, cs1)
            safe, ratio = got["cmd_out"], float(got["ratio"][0])
        state, contact, _ = plant_ref.step(state, {"cmd": safe, "agents": np.zeros((1, 1, 5)), "count": np.zeros(1, np.int32)}, pp,
                                           plant_ref.numpy_heading(pose))
        out.append((int(contact[0, 0]), float(state[1][0, 0]), ratio))
    return out, state


def test_a_stop_circle_keeps_the_robot_off_the_wall_the_plant_alone_lets_it_touch():
    bare, bare_state = drive_at_the_wall()
    assert any(f & plant_ref.FLAG_WALL for f, _, _ in bare) and bare[0][1] == 0.5       # without the monitor the bumper is what stops it
    assert bare_state[0][0, 0] > 25.0 * 0.125
    guarded, state = drive_at_the_wall([R.circle(R.STOP, 0.5, min_points=1)])           # 0.5 m: twice the footprint of 2 cells
    assert not any(f & (plant_ref.FLAG_WALL | plant_ref.FLAG_WALL_CONTACT) for f, _, _ in guarded)
    assert guarded[0][1] == 0.5 and guarded[-1][1] == 0.0 and guarded[-1][2] == 0.0 and state[1][0, 0] == 0.0
    assert state[0][0, 0] == 25.0 * 0.125      # it stands where the wall's nearest centre, at 28.5 cells, came within 0.5 m: 3.5 cells short


def test_an_approach_footprint_slows_the_robot_down_monotonically():
    run, _ = drive_at_the_wall([R.polygon(R.APPROACH, MC.SQUARE, min_points=1)], M=8)
    ratios, speeds = [r for _, _, r in run], [v for _, v, _ in run]
    first = next(i for i, r in enumerate(ratios) if r < 1.0)
    assert first > 4 and ratios[first] == 0.875 and all(r == 1.0 for r in ratios[:first])
    assert all(b <= a for a, b in zip(speeds[first:], speeds[first + 1:])) and speeds[-1] < 0.1 < speeds[first - 1] == 0.5
