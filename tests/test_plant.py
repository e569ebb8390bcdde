"""The robot plant on the CPU: the yardstick itself (tests/plant_ref.py: every substep's two clearances from scratch) on
hand-made sequences with the expected result written out, what the seeded sequences exercise, the `__host__ __device__`
rule of csrc/smpc_plant_rule.hpp compiled into a host-only program and composed as the kernel composes it (footprint
offsets in passes of 64 lanes, one wall clearance per distinct cell, the walk ended at the first blocked substep) against
the yardstick bit for bit given the program's own cosine and sine, those held against numpy's, the ctypes mirror against
include/smpc_plant.h, PlantParams, the episode's declarations and refusals, and the kernel's resource remarks."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import plant_cases as PC
import plant_ref as R
from nav2_social_mpc_controller_amd import _abi_plant as PA
from nav2_social_mpc_controller_amd import solver as S
from nav2_social_mpc_controller_amd.params import OptimizerParams, PlantParams, SensorParams
from test_kernel_budget import CSRC, HIPCC, parse_resource_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc_plant.h")
KERNEL = "_ZN4smpc23smpc_robot_plant_kernelENS_11PlantParamsE"

HAND = PC.hand_sequences()
SEEDED = PC.seeded_sequences()
MAIN = "B64_Np4_S4_L0_fd6"


@pytest.fixture(scope="module")
def seeded_ref():
    """name -> the yardstick's ticks of a seeded sequence with numpy's headings: [(tick, state before, new state, contact,
    counters)]."""
    out = {}
    for name, seq in SEEDED.items():
        ticks = []
        for t, tick, before, new, contact, cs in PC.run(seq, PC.ref_call):
            ticks.append((tick, before, new, contact, R.step(before, tick, seq["p"], cs)[2]))
        out[name] = ticks
    return out


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_sequences_end_where_the_contract_says(name):
    seq = HAND[name]
    n = 0
    for t, tick, before, new, contact, cs in PC.run(seq, PC.ref_call):
        assert tick["want"] is not None
        PC.check_want(seq, before, new, contact, tick["want"])
        assert new[0].dtype == np.float64 and new[1].dtype == np.float64 and new[3].dtype == np.uint32 and contact.dtype == np.int32
        th = new[0][:, 2]
        assert np.abs(th[np.isfinite(th)]).max(initial=0.0) <= 1e3                         # all cases keep |theta| <= 1e3
        n += 1
    assert n == len(seq["ticks"])


def test_the_main_seeded_sequence_exercises_the_plant(seeded_ref):
    """By the yardstick alone, before anything is compared with it: 64 robots x 40 ticks on the 64 x 48 world with 4 agents."""
    seq, ticks = SEEDED[MAIN], seeded_ref[MAIN]
    assert seq["p"]["world"].shape == (48, 64) and len(ticks) == 40 and ticks[0][0]["agents"].shape == (64, 4, 5)
    total, flags, n = dict.fromkeys(R.COUNTERS, 0), 0, 0
    for _, _, _, contact, counters in ticks:
        for k in R.COUNTERS:
            total[k] += int(counters[k].sum())
        flags |= int(np.bitwise_or.reduce(contact[:, 0]))
        n += len(contact)
    assert n == 64 * 40 and flags == 63, (flags, total)                # every flag bit ...
    assert all(total[k] >= 1 for k in R.COUNTERS), total               # ... and every counter fires
    assert total["full"] >= 0.05 * n, total
    assert total["blocked"] >= 0.20 * n, total
    assert total["partial"] >= 0.01 * n, total
    assert total["slide"] >= 1, total                                  # in wall contact, all S substeps, at the full target speed


def test_every_seeded_shape_blocks_and_advances_somewhere(seeded_ref):
    for name, ticks in seeded_ref.items():
        full = sum(int(c["full"].sum()) for *_, c in ticks)
        assert full >= 1, name
        if name != "B1_Np1_S1_L0_fd0":
            assert sum(int(c["blocked"].sum()) for *_, c in ticks) >= 1, name
        for tick, before, new, contact, _ in ticks:                   # all cases keep |theta| <= 1e3
            th = new[0][:, 2]
            assert np.abs(th[np.isfinite(th)]).max(initial=0.0) <= 1e3


# ---- the compiled rule ------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include "smpc_plant_rule.hpp"

static double num(const std::string& s) { return std::strtod(s.c_str(), nullptr); }   // hex floats, nan, inf
static std::string hex(double v) { char b[40]; uint64_t u; std::memcpy(&u, &v, 8); std::snprintf(b, sizeof b, "%016llx", (unsigned long long)u); return b; }
static double rd() { std::string w; std::cin >> w; return num(w); }

// The world, the scalars, then one robot per line, composed as the kernel composes the rule: 64 "lanes" take the offsets of
// the footprint's square in passes, a wall clearance is computed once per distinct cell, the walk ends at the first blocked
// substep.
int main() {
  long long Hx, Hy, has_world;
  std::cin >> Hx >> Hy >> has_world;
  std::vector<uint8_t> world((size_t)(Hx * Hy));
  for (auto& c : world) { long long v; std::cin >> v; c = (uint8_t)v; }
  long long S, L, fd2, min_cost, unknown, outside, Np, B;
  std::cin >> S >> L >> fd2 >> min_cost >> unknown >> outside >> Np >> B;
  const double dt = rd(), v_min = rd(), v_max = rd(), w_max = rd(), dv_up = rd(), dv_down = rd(), dw = rd(), contact_dist = rd(), res = rd(),
               ox = rd(), oy = rd();
  if (S < 1 || S > smpc::kPlantMaxSubsteps || L < 0 || L > smpc::kPlantMaxLatency || fd2 > smpc::kPlantMaxFootprintD2 || Np < 1 || Np > 64) std::abort();
  smpc::MathTab tab;
  smpc::fill_math_table(&tab);
  const bool on = has_world && fd2 >= 0;
  smpc::PlantWalls walls;
  walls.world = on ? world.data() : nullptr; walls.Hx = (int32_t)Hx; walls.Hy = (int32_t)Hy; walls.footprint_d2 = on ? (int32_t)fd2 : -1;
  walls.r = on ? smpc::pl_isqrt((int32_t)fd2) : 0; walls.min_cost = (int32_t)min_cost; walls.unknown = (int32_t)unknown; walls.outside = (int32_t)outside;
  const double contact2 = smpc::pl_contact2(contact_dist);
  const int n_off = (2 * walls.r + 1) * (2 * walls.r + 1);
  for (long long b = 0; b < B; ++b) {
    unsigned long long tick0; long long count;
    std::cin >> tick0 >> count;
    const double x = rd(), y = rd(), th = rd(), v = rd(), wz = rd(), cv = rd(), cw = rd();
    double queue[16];
    for (double& q : queue) q = rd();
    std::vector<double> px(Np), py(Np);
    for (long long j = 0; j < Np; ++j) { px[j] = rd(); py[j] = rd(); }
    const uint32_t tick = (uint32_t)tick0;
    double tv = cv, tw = cw;
    if (L > 0) { double* slot = queue + 2 * (tick % (uint32_t)L); tv = slot[0]; tw = slot[1]; slot[0] = cv; slot[1] = cw; }
    std::string q16;
    for (double q : queue) q16 += hex(q) + ",";
    const uint32_t tick1 = tick + 1u;
    if (!(smpc::pl_finite(x) && smpc::pl_finite(y) && smpc::pl_finite(th) && smpc::pl_finite(v) && smpc::pl_finite(wz))) {
      std::printf("%s %s %s %s %s %s %u %d %d - -\n", hex(x).c_str(), hex(y).c_str(), hex(th).c_str(), hex(0.0).c_str(), hex(0.0).c_str(), q16.c_str(),
                  tick1, smpc::kPlantBadState, 0);
      continue;
    }
    int flags = 0;
    if (!(smpc::pl_finite(tv) && smpc::pl_finite(tw))) { tv = 0.0; tw = 0.0; flags |= smpc::kPlantBadCommand; }
    const double v1 = smpc::pl_limit_v(v, tv, v_min, v_max, dv_up, dv_down), w1 = smpc::pl_limit_w(wz, tw, w_max, dw);
    double c, sn;
    smpc::pl_heading((const smpc::MathTab*)&tab, th, &c, &sn);
    const double Lx = smpc::pl_length(v1, c, dt), Ly = smpc::pl_length(v1, sn, dt);
    const long long n = count < 0 ? 0 : (count > Np ? Np : count);
    auto agent2 = [&](double qx, double qy) {
      uint64_t k = smpc::kPlantNoAgent;
      for (long long lane = 0; lane < 64; ++lane) {
        if (!(lane < n && smpc::pl_finite(px[lane]) && smpc::pl_finite(py[lane]))) continue;
        const uint64_t kl = smpc::pl_agent_key(px[lane], py[lane], qx, qy, contact2);
        k = kl < k ? kl : k;
      }
      return k;
    };
    long long scans = 0;
    auto wall2 = [&](int32_t cx, int32_t cy) {
      ++scans;
      uint32_t k = smpc::kPlantNoWall;
      for (int lane = 0; lane < 64; ++lane)
        for (int t = lane; t < n_off; t += 64) { const uint32_t kt = smpc::pl_offset_key(walls, cx, cy, t); k = kt < k ? kt : k; }
      return k;
    };
    const bool walls_on = smpc::pl_walls_on(walls);
    int32_t cx = 0, cy = 0;
    bool cell_ok = walls_on && smpc::pl_cell(x, y, ox, oy, res, &cx, &cy);
    uint32_t wk = cell_ok ? wall2(cx, cy) : smpc::kPlantNoWall;
    uint64_t ak = agent2(x, y);
    if (wk != smpc::kPlantNoWall) flags |= smpc::kPlantWallContact;
    if (ak != smpc::kPlantNoAgent) flags |= smpc::kPlantAgentContact;
    int K = 0;
    double qx = x, qy = y;
    for (int k = 1; k <= (int)S; ++k) {
      const double nx = smpc::pl_point(x, Lx, k, (int)S), ny = smpc::pl_point(y, Ly, k, (int)S);
      int32_t ncx = 0, ncy = 0;
      const bool nok = walls_on && smpc::pl_cell(nx, ny, ox, oy, res, &ncx, &ncy);
      uint32_t nwk = smpc::kPlantNoWall;
      if (nok) nwk = (cell_ok && ncx == cx && ncy == cy) ? wk : wall2(ncx, ncy);
      const uint64_t nak = agent2(nx, ny);
      const int blocked = (nwk < wk ? smpc::kPlantBlockedByWall : 0) | (nak < ak ? smpc::kPlantBlockedByAgent : 0);
      if (blocked != 0) { flags |= blocked; break; }
      K = k; qx = nx; qy = ny; cx = ncx; cy = ncy; cell_ok = nok; wk = nwk; ak = nak;
    }
    std::printf("%s %s %s %s %s %s %u %d %d %s %s\n", hex(qx).c_str(), hex(qy).c_str(), hex(smpc::pl_turn(th, w1, dt)).c_str(),
                hex(K == (int)S ? v1 : 0.0).c_str(), hex(w1).c_str(), q16.c_str(), tick1, flags, K, hex(c).c_str(), hex(sn).c_str());
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    tmp = tmp_path_factory.mktemp("plant_rule")
    src, exe = tmp / "probe.hip", tmp / "probe"
    src.write_text(PROBE)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])   # -O3 as build.sh

    def call(state, tick, p):
        """(new state, contact, cs) by the compiled rule; cs rows of robots whose state is not finite are NaN."""
        pose, twist, queue, ticks = state
        agents, B = np.asarray(tick["agents"], np.float64), len(tick["count"])
        Np = agents.shape[1]
        hx = lambda v: float(v).hex() if np.isfinite(v) else repr(float(v))
        world = p["world"]
        Hy, Hx = (0, 0) if world is None else world.shape
        lines = [" ".join(map(str, [Hx, Hy, int(world is not None)] + ([] if world is None else world.ravel().tolist()))),
                 " ".join(map(str, [p["S"], p["L"], p["footprint_d2"], p["wall_min_cost"], int(p["unknown_is_wall"]), int(p["outside_is_wall"]), Np, B]
                              + [hx(p[k]) for k in ("dt", "v_min", "v_max", "w_max", "dv_up", "dv_down", "dw", "contact_dist", "res")]
                              + [hx(p["origin"][0]), hx(p["origin"][1])]))]
        for b in range(B):
            lines.append(" ".join(map(str, [int(ticks[b]), int(tick["count"][b])] + [hx(v) for v in list(pose[b]) + list(twist[b]) + list(tick["cmd"][b])
                                                                                      + list(queue[b].ravel()) + list(agents[b, :, :2].ravel())])))
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == B
        f64 = lambda words: np.array([int(w, 16) for w in words], np.uint64).view(np.float64)
        new = (np.zeros((B, 3)), np.zeros((B, 2)), np.zeros((B, 8, 2)), np.zeros(B, np.uint32))
        contact, cs = np.zeros((B, 2), np.int32), np.full((B, 2), np.nan)
        for b, line in enumerate(out):
            w = line.split()
            new[0][b], new[1][b], new[2][b] = f64(w[0:3]), f64(w[3:5]), f64(w[5].split(",")[:-1]).reshape(8, 2)
            new[3][b], contact[b] = int(w[6]), (int(w[7]), int(w[8]))
            if w[9] != "-":
                cs[b] = f64(w[9:11])
        return new, contact, cs

    return call


def held_to_the_yardstick(seq, call):
    """Runs `call` over a sequence from its own state; every tick against the yardstick fed the call's cosine and sine."""
    n = 0
    for t, tick, before, new, contact, cs in PC.run(seq, call):
        want = PC.ref_call(before, tick, seq["p"], cs)
        assert PC.same((new, contact), want[:2]), t
        assert R.heading_close(cs, before), t
        finite = np.isfinite(before[0]).all(axis=1) & np.isfinite(before[1]).all(axis=1)
        assert np.isfinite(cs[finite]).all() and np.isnan(cs[~finite]).all()
        PC.check_want(seq, before, new, contact, tick["want"])
        n += 1
    return n


@pytest.mark.parametrize("name", sorted(HAND))
def test_compiled_rule_is_the_yardstick_on_the_hand_made_sequences(rule, name):
    assert held_to_the_yardstick(HAND[name], rule) == len(HAND[name]["ticks"])


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_compiled_rule_is_the_yardstick_on_the_seeded_sequences(rule, name):
    assert held_to_the_yardstick(SEEDED[name], rule) == len(SEEDED[name]["ticks"])


def test_the_rule_header_rounds_every_operation_on_its_own():
    text = open(os.path.join(CSRC, "smpc_plant_rule.hpp")).read()
    assert text.count("#pragma clang fp contract(off)") >= 8 and "fma(" not in text and "hip_runtime" not in text
    assert re.findall(r'#include\s+([<"][^>"]+[>"])', text) == ["<stdint.h>", '"smpc_math.hpp"']
    kernel = open(os.path.join(CSRC, "smpc_plant.hpp")).read()
    assert '#include "smpc_plant_rule.hpp"' in kernel and "SMPC_CHAIN_PRIORITY();" in kernel and "atomic" not in kernel.split("#pragma once")[1]


# ---- the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mirror_matches_the_header_and_the_library_exports_the_function(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src))) == sorted(PA.FUNCTIONS) == ["smpc_robot_plant_batch"]
    assert re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S) == [st.c_name for st in PA.STRUCTS]
    consts = ["SMPC_PLANT_MAX_SUBSTEPS", "SMPC_PLANT_MAX_LATENCY", "SMPC_PLANT_MAX_FOOTPRINT_D2", "SMPC_PLANT_BLOCKED_BY_WALL",
              "SMPC_PLANT_BLOCKED_BY_AGENT", "SMPC_PLANT_WALL_CONTACT", "SMPC_PLANT_AGENT_CONTACT", "SMPC_PLANT_BAD_COMMAND", "SMPC_PLANT_BAD_STATE"]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' + "".join(f'printf("%zu\\n", offsetof({st.c_name}, {f[0]}));\n' for f in st._fields_)
                   for st in PA.STRUCTS)
    body += "".join(f'printf("%d\\n", (int){name});\n' for name in consts)
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc_plant.h"\nint main(void){\n' + body + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [v for st in PA.STRUCTS for v in [C.sizeof(st)] + [getattr(st, f[0]).offset for f in st._fields_]]
    assert values == want + [getattr(PA, name) for name in consts] and values[-9:] == [16, 8, 225, 1, 2, 4, 8, 16, 32]
    fields = re.findall(r"\b(\w+)\s*(?:\[\d+\]\s*)?(?:,|;)", re.search(r"typedef struct smpc_plant_in \{(.*?)\}", src, flags=re.S).group(1))
    assert fields == [f[0] for f in PA.SmpcPlantIn._fields_] and C.sizeof(PA.SmpcPlantIn) == 48 + 11 * 8 + 4 * 8
    assert (R.FLAG_WALL, R.FLAG_AGENT, R.FLAG_WALL_CONTACT, R.FLAG_AGENT_CONTACT, R.FLAG_BAD_COMMAND, R.FLAG_BAD_STATE) == tuple(values[-6:])
    exported = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    lib = S.load_library()
    for name, (restype, argtypes) in PA.FUNCTIONS.items():
        assert f" {name}\n" in exported
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes


def test_the_main_abi_is_as_it_was():
    from nav2_social_mpc_controller_amd import _abi
    assert _abi.SMPC_ABI_VERSION == 6 and len(_abi.FUNCTIONS) == 27 and not set(PA.FUNCTIONS) & set(_abi.FUNCTIONS)
    assert "SMPC_ABI_VERSION 6" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "smpc.h")).read())


# ---- the parameters -------------------------------------------------------------------------------------------------------
def test_plant_params():
    pp = PlantParams()
    assert (pp.max_accel, pp.max_decel, pp.max_ang_accel, pp.latency_ticks, pp.substeps) == (2.5, 2.5, 3.2, 0, 8)
    assert (pp.robot_radius, pp.agent_radius, pp.wall_min_cost, pp.unknown_is_wall, pp.outside_is_wall) == (0.24, 0.3, 254, False, True)
    # footprint_d2 rounds as SensorParams.agent_d2 does: floor((radius / resolution)^2 + 1e-9)
    for radius, res in ((0.24, 0.05), (0.3, 0.1), (0.25, 0.05), (0.0, 0.05), (0.75, 0.05), (0.7499, 0.05)):
        assert PlantParams(robot_radius=radius).footprint_d2(res) == SensorParams(agent_radius=radius).agent_d2(res)
    assert PlantParams(robot_radius=0.3).footprint_d2(0.1) == 9 and PlantParams(robot_radius=0.75).footprint_d2(0.05) == 225
    assert PlantParams(robot_radius=None).footprint_d2(0.05) == -1
    assert pp.supported() and pp.supported(0.05) and PlantParams(robot_radius=0.75).supported(0.05) and not PlantParams(robot_radius=0.76).supported(0.05)
    assert pp.contact_dist() == float(np.float64(0.24) + np.float64(0.3)) and PlantParams(agent_radius=None).contact_dist() == 0.0
    assert PlantParams(max_accel=0.5, max_decel=1.0, max_ang_accel=2.0).deltas(0.125) == (0.0625, 0.125, 0.25)
    assert pp.deltas(0.1) == (float(np.float64(2.5) * np.float64(0.1)),) * 2 + (float(np.float64(3.2) * np.float64(0.1)),)
    ideal = PlantParams.ideal()
    assert ideal.deltas(0.1) == (np.inf,) * 3 and ideal.deltas(0.0) == (np.inf,) * 3 and ideal.latency_ticks == 0
    assert ideal.footprint_d2(0.05) == -1 and ideal.contact_dist() == 0.0 and ideal.substeps == 1
    for bad in (dict(max_accel=-0.1), dict(max_accel=np.nan), dict(max_decel=-1.0), dict(max_ang_accel=np.nan), dict(latency_ticks=-1),
                dict(latency_ticks=9), dict(latency_ticks=1.5), dict(substeps=0), dict(substeps=17), dict(robot_radius=-0.1),
                dict(robot_radius=np.inf), dict(agent_radius=np.nan), dict(wall_min_cost=256), dict(wall_min_cost=-1)):
        with pytest.raises(ValueError):
            PlantParams(**bad)
    for dt in (-0.1, np.nan, np.inf):
        with pytest.raises(ValueError):
            pp.deltas(dt)
    prm = OptimizerParams.readme()
    pi = S.BatchSolver.plant_c(PlantParams(max_accel=0.5, max_decel=1.0, max_ang_accel=2.0, latency_ticks=3, substeps=5, robot_radius=0.3,
                                           agent_radius=0.2, wall_min_cost=200, unknown_is_wall=True, outside_is_wall=False),
                               prm, 7, 6, 1, 64, 48, 0.1, (-1.0, -0.5))
    assert (pi.B, pi.Np, pi.S, pi.L, pi.on_device, pi.Hx, pi.Hy, pi.footprint_d2, pi.wall_min_cost, pi.unknown_is_wall, pi.outside_is_wall,
            pi.reserved) == (7, 6, 5, 3, 1, 64, 48, 9, 200, 1, 0, 0)
    dt = float(prm.dt)
    assert (pi.dt, pi.v_min, pi.v_max, pi.w_max) == (dt, float(prm.v_min), float(prm.v_max), float(prm.w_max))
    assert (pi.dv_up, pi.dv_down, pi.dw) == (0.5 * dt, 1.0 * dt, 2.0 * dt) and pi.contact_dist == 0.5 and pi.resolution == 0.1
    assert tuple(pi.world_origin) == (-1.0, -0.5) and not pi.world and not pi.cmd and not pi.agents and not pi.count


def test_the_episode_declares_the_argument_and_refuses_what_the_library_would():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode, TickRecord, shard_kwargs
    assert "plant" in BatchEpisode.FORWARDED and "plant" not in BatchEpisode.PER_ROBOT
    assert inspect.signature(BatchEpisode.__init__).parameters["plant"].default is None
    fields = TickRecord.__dataclass_fields__
    names = ("plant_agents", "plant_agent_count", "plant_queue_before", "plant_tick_before", "plant_queue_after", "plant_tick_after",
             "plant_contact", "heading_cs", "speed_after")
    assert all(fields[name].default is None for name in names)
    from nav2_social_mpc_controller_amd.episode_stages import Core, Crowd, Metrics, Plant, PoolCrowd
    at = BatchEpisode.STAGES.index                                                              # the launch order: Core ends with the command selection
    assert at(Core) < at(Crowd) < at(PoolCrowd) < at(Plant) < at(Metrics) and Plant.TIMING == "plant"
    assert Plant.STATE == ("plant_queue", "plant_tick")                                         # saved and restored around the warm-up tick
    pp = PlantParams()
    assert shard_kwargs({"plant": pp}, np.arange(2), 4)["plant"] is pp and "shard_kwargs" in inspect.getsource(ShardedEpisode.__init__)
    BatchEpisode.check_plant(pp)
    BatchEpisode.check_plant(pp, 0.05)
    BatchEpisode.check_plant(PlantParams.ideal(), 0.05)
    for bad, res in ((dict(max_accel=1.0), 0.05), (None, None), (PlantParams(robot_radius=0.8), 0.05), (PlantParams(robot_radius=1.6), 0.1)):
        with pytest.raises(ValueError):
            BatchEpisode.check_plant(bad, res)


# ---- the kernel's resources ------------------------------------------------------------------------------------------------
def test_the_kernel_has_no_spills_no_scratch_no_lds_and_full_occupancy(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    r = subprocess.run(["bash", os.path.join(CSRC, "build.sh"), "-DSMPC_ONLY_NB=3", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage"],
                       env={**os.environ, "SMPC_OUT": str(tmp_path / "smpc_nb3.o")}, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    use = parse_resource_remarks(r.stderr).get(KERNEL)
    assert use is not None, "no resource remark for smpc_robot_plant_kernel"
    assert use["VGPRs Spill"] == 0 and use["SGPRs Spill"] == 0 and use["ScratchSize [bytes/lane]"] == 0, use   # no private segment
    assert use["LDS Size [bytes/block]"] == 0 and use["Occupancy [waves/SIMD]"] == 8, use
