"""Sensed local costmaps with memory on the CPU: the yardstick itself (tests/obstacle_memory_ref.py: the sequential walk
with its passed cells, the roll, marks, footprint) on hand-made sequences with the bitmaps written out, the `__host__
__device__` rule of csrc/smpc_obstacle_memory_rule.hpp (closed-form columns that report passed cells, the roll of words)
compiled into a host-only program and composed as the kernel composes it against the yardstick, the ctypes mirror against
include/smpc_obstacle_memory.h, ObstacleMemoryParams, the episode's declarations, the kernel's resource remarks, and that
the seeded sequences exercise what the feature adds."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import obstacle_memory_cases as OC
import obstacle_memory_ref as M
import sensed_costmap_cases as K
import sensed_costmap_ref as R
from nav2_social_mpc_controller_amd import _abi_obstacle_memory as OA
from nav2_social_mpc_controller_amd import _abi_sensed_costmap as SA
from nav2_social_mpc_controller_amd import solver as S
from nav2_social_mpc_controller_amd.params import ObstacleMemoryParams, SensorParams
from test_kernel_budget import CSRC, HIPCC, parse_resource_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc_obstacle_memory.h")
KERNEL = "_ZN4smpc27smpc_obstacle_memory_kernelENS_20ObstacleMemoryParamsE"
LDS_BUDGET = 54613                                 # three workgroups per CU in 160 KB

HAND = OC.hand_sequences()
SEEDED = OC.seeded_sequences()


@pytest.fixture(scope="module")
def seeded_ref():
    """name -> the yardstick's ticks of a seeded sequence: [(kw, mark_d2, footprint_d2, before, got)]."""
    return {name: [(kw, seq["ticks"][t][1], seq["ticks"][t][2], before, got) for t, kw, before, got, _ in OC.run(seq, OC.ref_call)]
            for name, seq in SEEDED.items()}


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_sequences_leave_the_marks_the_contract_gives(name):
    for t, kw, before, got, want in OC.run(HAND[name], OC.ref_call):
        costmap, _, _, (memory, memory_cell), _ = got
        B, sx, sy = kw["people"].shape[0], kw["size_x"], kw["size_y"]
        assert want is not None and len(want) == B
        assert np.array_equal(memory_cell, kw["cell"]) and memory.dtype == np.uint32 and memory.shape == (B, sy, M.words(sx))
        for b in range(B):
            assert M.bits_to_cells(memory[b], sx) == want[b], (name, t, b)
            assert np.array_equal(costmap[b], R.inflate(want[b], sx, sy, kw["table"])), (name, t, b)    # base 0 throughout
            assert {(x, y) for y, x in np.argwhere(costmap[b] == 254)} == want[b]


def test_the_walk_is_the_memoryless_walk_on_every_beam_of_every_seeded_case(seeded_ref):
    beams = 0
    for ticks in seeded_ref.values():
        for kw, _, _, _, got in ticks:
            for b in range(kw["people"].shape[0]):
                a = R.point_cell(*kw["robot_pose"][b, :2], kw["origin"], kw["res"])
                occupied = R.occupied_cells(kw["people"][b], kw["count"][b], kw["origin"], kw["res"], kw["agent_d2"])
                for k, off in enumerate(kw["beam_cells"]):
                    kind, cell, hits = R.cast(kw["world"], occupied, a, off)
                    assert (kind, cell, hits) == M.walk(kw["world"], occupied, a, off)[:3]
                    assert (got[1][b, k], tuple(got[2][b, k])) == (kind, cell)
                    beams += 1
    assert beams >= 4 * 6 * 8 * 48


def test_zero_memory_and_a_wide_marking_range_is_the_memoryless_call(seeded_ref):
    for ticks in seeded_ref.values():
        kw = ticks[3][0]
        got = M.step(M.zero_state(kw["people"].shape[0], kw["size_x"], kw["size_y"]), mark_d2=OC.BIG, footprint_d2=-1, **kw)
        want = R.sensed_costmap(**kw)
        assert all(np.array_equal(g, w) for g, w in zip(got[:3], want))
        # nor does an all-zero memory need a valid memory_cell
        wild = (M.zero_state(8, kw["size_x"], kw["size_y"])[0], np.full((8, 2), -2 ** 31, np.int32))
        assert all(np.array_equal(g, w) for g, w in zip(M.step(wild, mark_d2=OC.BIG, footprint_d2=-1, **kw)[:3], want))


def test_the_seeded_sequences_exercise_what_the_memory_adds(seeded_ref):
    """By the yardstick alone: every counter is at least 1 in some robot-tick, and at least 5 % of the robot-ticks keep a
    mark that no beam hit this tick."""
    some = {name: 0 for name in M.COUNTERS}
    robot_ticks = 0
    for ticks in seeded_ref.values():
        for _, _, _, _, got in ticks:
            for name in M.COUNTERS:
                some[name] += int((got[4][name] >= 1).sum())
            robot_ticks += len(got[4]["kept"])
    assert robot_ticks == 4 * 6 * 8 and all(v >= 1 for v in some.values()), some
    assert some["kept"] >= 0.05 * robot_ticks


# ---- the __host__ __device__ rule, compiled for the host -----------------------------------------------------------------
# One robot per query, whitespace-separated: Hx Hy min unknown size_x size_y cell_x cell_y agent_d2 d2_max base outside K Np
# count mark_d2 footprint_d2 memory_cell_x memory_cell_y res ox oy rx ry (the doubles as hex floats), the world, the table and
# the memory (little-endian words) as hex strings, K beam offsets, Np agent points. Composed as the kernel composes it: the
# roll of words into padded row masks, the occupancy bitmap of the reach square, om_cast with a pass functor that clears
# and a mark within om_in_mark_range, om_in_footprint over the window, then the memoryless rule's inflation. Answer: the
# kinds, the beam cells, the window, the new memory, and per beam the passed offsets.
PROBE = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "smpc_obstacle_memory_rule.hpp"
static double num(const std::string& s) { return std::strtod(s.c_str(), nullptr); }
static std::vector<unsigned char> bytes(const std::string& s) {
  std::vector<unsigned char> v(s.size() / 2);
  for (size_t i = 0; i < v.size(); ++i) v[i] = (unsigned char)std::stoi(s.substr(2 * i, 2), nullptr, 16);
  return v;
}
static long long isqrt(long long v) {
  long long r = (long long)std::sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}
int main() {
  long long Hx, Hy, mn, unk, sx, sy, cellx, celly, agent_d2, d2_max, base, outside, K, Np, count, mark_d2, foot_d2, mcx, mcy;
  while (std::cin >> Hx >> Hy >> mn >> unk >> sx >> sy >> cellx >> celly >> agent_d2 >> d2_max >> base >> outside >> K >> Np >> count >>
         mark_d2 >> foot_d2 >> mcx >> mcy) {
    std::string t[5], ws, ts, ms;
    for (auto& s : t) std::cin >> s;
    std::cin >> ws >> ts >> ms;
    const double res = num(t[0]), ox = num(t[1]), oy = num(t[2]), rx = num(t[3]), ry = num(t[4]);
    const std::vector<unsigned char> world = bytes(ws), table = bytes(ts), mem_bytes = bytes(ms);
    std::vector<long long> beams(2 * K);
    for (auto& v : beams) std::cin >> v;
    std::vector<std::string> pts(2 * Np);
    for (auto& s : pts) std::cin >> s;
    const int32_t W = (int32_t)((sx + 31) / 32);
    std::vector<uint32_t> memory((size_t)(sy * W));
    for (size_t i = 0; i < memory.size(); ++i)
      memory[i] = (uint32_t)mem_bytes[4 * i] | ((uint32_t)mem_bytes[4 * i + 1] << 8) | ((uint32_t)mem_bytes[4 * i + 2] << 16) | ((uint32_t)mem_bytes[4 * i + 3] << 24);
    const smpc::VisOcc vo{(uint32_t)mn, (uint32_t)unk};
    int32_t ax = 0, ay = 0;
    const bool robot_ok = smpc::vis_robot_cell(rx, ry, ox, oy, res, &ax, &ay);
    // the roll
    std::vector<uint32_t> marks(256 * 10, 0u);
    const int32_t shx = smpc::om_shift((int32_t)mcx, (int32_t)cellx), shy = smpc::om_shift((int32_t)mcy, (int32_t)celly);
    for (int32_t y = 0; y < sy; ++y)
      for (int32_t w = 0; w < W; ++w) {
        int32_t src_y = 0;
        smpc::OmRoll ro;
        if (!smpc::om_roll_row(shy, (int32_t)sy, y, &src_y) || !smpc::om_roll_source(shx, (int32_t)sx, w, &ro)) continue;
        if (src_y < 0 || src_y >= sy || ro.sh > 31u) std::abort();
        const uint32_t* src = &memory[(size_t)src_y * W];
        const int32_t lo = ro.hi - 1;
        const uint32_t hi_word = (ro.hi >= 0 && ro.hi < W) ? src[ro.hi] & smpc::om_word_mask((int32_t)sx, ro.hi) : 0u;
        const uint32_t lo_word = (lo >= 0 && lo < W) ? src[lo] & smpc::om_word_mask((int32_t)sx, lo) : 0u;
        marks[y * 10 + 1 + w] = smpc::om_roll_join(hi_word, lo_word, ro.sh) & smpc::om_word_mask((int32_t)sx, w);
      }
    std::vector<unsigned char> occupied(255 * 255, 0);
    const long long cnt = count < 0 ? 0 : (count > Np ? Np : count);
    if (robot_ok)
      for (long long j = 0; j < cnt; ++j) {
        int32_t qx = 0, qy = 0;
        if (!smpc::sc_agent_cell(num(pts[2 * j]), num(pts[2 * j + 1]), ox, oy, res, &qx, &qy)) continue;
        for (long long cy = -127; cy <= 127; ++cy)
          for (long long cx = -127; cx <= 127; ++cx) {
            const long long ddx = (long long)ax + cx - qx, ddy = (long long)ay + cy - qy;
            if (ddx * ddx + ddy * ddy <= agent_d2) occupied[(cy + 127) * 255 + (cx + 127)] = 1;
          }
      }
    const auto stops = [&](int32_t cx, int32_t cy) -> uint32_t {
      if (cx == 0 && cy == 0) std::abort();                                  // never asked for
      if (cx < -127 || cx > 127 || cy < -127 || cy > 127) std::abort();      // nor outside the reach square
      const long long wx = (long long)ax + cx, wy = (long long)ay + cy;
      if (wx >= 0 && wx < Hx && wy >= 0 && wy < Hy && smpc::vis_occludes(vo, world[wy * Hx + wx])) return smpc::kBeamWorld;
      return occupied[(cy + 127) * 255 + (cx + 127)] ? smpc::kBeamAgent : 0u;
    };
    const int32_t rel_x = smpc::om_window_rel(ax, (int32_t)cellx), rel_y = smpc::om_window_rel(ay, (int32_t)celly);
    std::string passed;
    const auto pass = [&](int32_t cx, int32_t cy) {
      passed += std::to_string(cx) + ":" + std::to_string(cy) + ";";
      int32_t wx = 0, wy = 0, vx = 0, vy = 0;
      const bool in = smpc::om_window_cell(rel_x, rel_y, cx, cy, (int32_t)sx, (int32_t)sy, &wx, &wy);
      if (in != smpc::sc_window_cell(ax, ay, cx, cy, (int32_t)cellx, (int32_t)celly, (int32_t)sx, (int32_t)sy, &vx, &vy)) std::abort();
      if (!in) return;
      if (wx != vx || wy != vy) std::abort();
      marks[wy * 10 + 1 + (wx >> 5)] &= ~(1u << (wx & 31));
    };
    const auto mark = [&](int32_t cx, int32_t cy) {
      int32_t wx = 0, wy = 0;
      if (!smpc::om_in_mark_range(cx, cy, (int32_t)mark_d2)) return;
      if (smpc::om_window_cell(rel_x, rel_y, cx, cy, (int32_t)sx, (int32_t)sy, &wx, &wy)) marks[wy * 10 + 1 + (wx >> 5)] |= 1u << (wx & 31);
    };
    std::string kinds, cells;
    for (long long k = 0; k < K; ++k) {
      const int32_t ex = (int32_t)beams[2 * k], ey = (int32_t)beams[2 * k + 1];
      uint32_t kind = smpc::kBeamNoRobot;
      int32_t hx = ex, hy = ey;
      if (robot_ok) {
        kind = smpc::kBeamInvalid;
        if (smpc::sc_beam_valid(ex, ey)) {
          const smpc::ScHit h = smpc::om_cast(ex, ey, stops, pass);
          const smpc::ScHit h0 = smpc::sc_cast(ex, ey, stops);
          if (h.kind != h0.kind || h.ox != h0.ox || h.oy != h0.oy || (h.kind == smpc::kBeamCornerPair && (h.px != h0.px || h.py != h0.py))) std::abort();
          kind = h.kind; hx = h.ox; hy = h.oy;
          if (kind != smpc::kBeamNone) mark(h.ox, h.oy);
          if (kind == smpc::kBeamCornerPair) mark(h.px, h.py);
        }
      }
      kinds += std::to_string(kind) + ",";
      cells += std::to_string(hx) + "," + std::to_string(hy) + ",";
      passed += "|";
    }
    if (robot_ok && foot_d2 >= 0)
      for (long long y = 0; y < sy; ++y)
        for (long long x = 0; x < sx; ++x)
          if (smpc::om_in_footprint(cellx + x - ax, celly + y - ay, (int32_t)foot_d2)) marks[y * 10 + 1 + (x >> 5)] &= ~(1u << (x & 31));
    const long long r = isqrt(d2_max);
    std::vector<unsigned char> gap(sx * sy);
    for (long long y = 0; y < sy; ++y)
      for (long long x = 0; x < sx; ++x) {
        const uint32_t* line = &marks[y * 10 + (x >> 5)];
        const uint32_t sh = (uint32_t)(x & 31), w2 = line[2];
        const uint64_t w01 = ((uint64_t)line[1] << 32) | line[0];
        const uint64_t v = sh ? (w01 >> sh) | ((uint64_t)w2 << (64u - sh)) : w01;
        gap[y * sx + x] = (unsigned char)smpc::sc_row_gap(v, w2 >> sh, (uint32_t)r);
      }
    std::string out, mem;
    char hex[3];
    for (long long y = 0; y < sy; ++y)
      for (long long x = 0; x < sx; ++x) {
        uint32_t best = smpc::kSensedNoMark;
        for (long long yy = (y - r < 0 ? 0 : y - r); yy <= (y + r > sy - 1 ? sy - 1 : y + r); ++yy)
          best = smpc::sc_least_d2(best, gap[yy * sx + x], (uint32_t)((yy - y) * (yy - y)));
        uint32_t c = smpc::sc_cost(best, table.data(), (uint32_t)d2_max);
        if (base) {
          const long long wx = cellx + x, wy = celly + y;
          const uint32_t w = (wx >= 0 && wx < Hx && wy >= 0 && wy < Hy) ? world[wy * Hx + wx] : (uint32_t)outside;
          c = c > w ? c : w;
        }
        std::snprintf(hex, sizeof hex, "%02x", c);
        out += hex;
      }
    for (long long y = 0; y < sy; ++y)
      for (int32_t w = 0; w < W; ++w) {
        const uint32_t v = marks[y * 10 + 1 + w] & smpc::om_word_mask((int32_t)sx, w);
        for (int c = 0; c < 4; ++c) { std::snprintf(hex, sizeof hex, "%02x", (v >> (8 * c)) & 255u); mem += hex; }
      }
    std::printf("%s %s %s %s %s\n", kinds.c_str(), cells.c_str(), out.c_str(), mem.c_str(), passed.c_str());
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    tmp = tmp_path_factory.mktemp("obstacle_memory_rule")
    src, exe = tmp / "probe.hip", tmp / "probe"
    src.write_text(PROBE)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])   # -O3 as build.sh

    def ask(state, kw, mark_d2, footprint_d2):
        """The compiled rule's (costmap, beam_kind, beam_cell, new state, passed: per robot and beam a set of offsets)."""
        memory, memory_cell = state
        world, origin = np.asarray(kw["world"], np.uint8), np.asarray(kw["origin"], np.float64).reshape(-1, 2)
        B, Np, beams = kw["people"].shape[0], kw["people"].shape[1], np.asarray(kw["beam_cells"], np.int64)
        hx = lambda v: float(v).hex() if np.isfinite(v) else repr(float(v))
        lines = []
        for b in range(B):
            w, o = (world, origin[0]) if world.ndim == 2 else (world[b], origin[b])
            lines.append(" ".join(map(str, [w.shape[1], w.shape[0], kw["min_cost"], int(kw["unknown"]), kw["size_x"], kw["size_y"],
                                            kw["cell"][b, 0], kw["cell"][b, 1], kw["agent_d2"], len(kw["table"]) - 1, kw["base"],
                                            kw["outside_cost"], len(beams), Np, kw["count"][b], mark_d2, footprint_d2,
                                            memory_cell[b, 0], memory_cell[b, 1]]
                                      + [hx(v) for v in (kw["res"], o[0], o[1], kw["robot_pose"][b, 0], kw["robot_pose"][b, 1])]
                                      + [w.tobytes().hex(), np.asarray(kw["table"], np.uint8).tobytes().hex(),
                                         np.ascontiguousarray(memory[b], "<u4").tobytes().hex()]
                                      + beams.ravel().tolist() + [hx(v) for v in kw["people"][b, :, :2].ravel()])))
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == B
        sx, sy = kw["size_x"], kw["size_y"]
        cm, new = np.zeros((B, sy, sx), np.uint8), np.zeros((B, sy, M.words(sx)), np.uint32)
        kind, hit = np.zeros((B, len(beams)), np.uint8), np.zeros((B, len(beams), 2), np.int32)
        passed = []
        for b, line in enumerate(out):
            kinds, cells, window, mem, trail = line.split()
            kind[b] = [int(v) for v in kinds.split(",")[:-1]]
            hit[b] = np.array([int(v) for v in cells.split(",")[:-1]]).reshape(-1, 2)
            cm[b] = np.frombuffer(bytes.fromhex(window), np.uint8).reshape(sy, sx)
            new[b] = np.frombuffer(bytes.fromhex(mem), "<u4").reshape(sy, M.words(sx))
            passed.append([{tuple(int(v) for v in c.split(":")) for c in beam.split(";") if c} for beam in trail.split("|")[:-1]])
        return cm, kind, hit, (new, np.asarray(kw["cell"], np.int32).copy()), passed

    return ask


def same(got, want):
    """costmap, beam_kind, beam_cell, memory and memory_cell, value and dtype."""
    pairs = list(zip(got[:3], want[:3])) + list(zip(got[3], want[3]))
    return all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in pairs)


def test_compiled_rule_is_the_yardstick_on_the_hand_made_sequences(rule):
    for name, seq in HAND.items():
        for t, kw, before, got, _ in OC.run(seq, rule):
            assert same(got, OC.ref_call(before, kw, seq["ticks"][t][1], seq["ticks"][t][2])), (name, t)


def test_compiled_rule_is_the_yardstick_on_the_seeded_sequences(rule, seeded_ref):
    for name, ticks in seeded_ref.items():
        for t, (kw, mark_d2, footprint_d2, before, want) in enumerate(ticks):
            assert same(rule(before, kw, mark_d2, footprint_d2), want), (name, t)


@pytest.mark.parametrize("seed,reach,size,r,base", [(11, 10, (37, 70), 5, 1), (12, 60, (90, 41), 9, 0), (13, 127, (256, 33), 32, 0)])
def test_compiled_rule_is_the_yardstick_on_random_sequences(rule, seed, reach, size, r, base):
    g = np.random.default_rng(seed)
    kw = K.random_case(seed=seed, reach=reach, size=size, r=r, base=base, off_fraction=0.3, world_size=(96, 80) if reach < 60 else (300, 200),
                       n_beams=64 if reach < 60 else 180)
    B = kw["people"].shape[0]
    # a random memory with garbage in the padding, shifted by a few cells, then a second tick from the result
    state = (g.integers(0, 2 ** 32, (B, size[1], M.words(size[0])), dtype=np.uint64).astype(np.uint32) & g.integers(0, 2 ** 32, (B, size[1], M.words(size[0])), dtype=np.uint64).astype(np.uint32),
             (kw["cell"] + g.integers(-40, 41, (B, 2))).astype(np.int32))
    for t in range(2):
        want = M.step(state, mark_d2=(reach * 3 // 4) ** 2, footprint_d2=6, **kw)
        assert same(rule(state, kw, (reach * 3 // 4) ** 2, 6), want), t
        assert max(int(want[4][name].sum()) for name in ("kept", "cleared", "rolled_out")) >= 1
        state = want[3]
        kw = dict(kw, cell=(kw["cell"] + g.integers(-3, 4, (B, 2))).astype(np.int32))


def test_compiled_rule_passes_the_cells_of_the_walk_on_every_beam_of_a_square(rule):
    """Every end offset within 12 cells, over a random clutter of walls and one agent: the closed-form columns pass the cells
    the sequential walk passes, in all eight octants, corners included (compared as sets, beam by beam)."""
    g = np.random.default_rng(7)
    world = (g.random((31, 31)) < 0.12).astype(np.uint8) * 254
    beams = [(x, y) for x in range(-12, 13) for y in range(-12, 13)]
    kw, _ = K.case(robots=[(15, 15)], agents=[[(19, 12)]], agent_d2=2, beams=beams, size=(31, 31), world_size=(31, 31))
    kw["world"] = world
    state = (np.full((1, 31, 1), 0xFFFFFFFF, np.uint32), np.array([[1, -2]], np.int32))
    want = M.step(state, mark_d2=100, footprint_d2=2, **kw)
    got = rule(state, kw, 100, 2)
    assert same(got, want)
    occupied = R.occupied_cells(kw["people"][0], kw["count"][0], kw["origin"], kw["res"], 2)
    kinds = np.zeros(4, int)
    for k, off in enumerate(beams):
        kind, _, hits, passed = M.walk(world, occupied, (15, 15), off)
        assert got[4][0][k] == set(passed) and not set(passed) & set(hits), off
        kinds[kind] += 1
    assert kinds.min() >= 5                                                               # none, world, agent and pairs all occur


@pytest.mark.parametrize("width", [33, 64])
def test_compiled_roll_for_every_shift(rule, width):
    """One-row windows, robots without a cell, one per shift in -40 .. 40 on each axis' turn; garbage in the input padding."""
    g = np.random.default_rng(width)
    shifts = [(s, 0) for s in range(-40, 41)] + [(0, s) for s in (-1, 1)] + [(width, 0), (-width, 0), (2 ** 31 - 1, 0), (-2 ** 31, 0)]
    B = len(shifts)
    kw, _ = K.case(robots=[(OC.NAN, 0.0)] * B, size=(width, 1), world_size=(width, 2), cell=[(0, 0)] * B)
    row = g.integers(0, 2 ** 32, (1, 1, M.words(width)), dtype=np.uint64).astype(np.uint32)
    memory_cell = np.array([(min(max(s, -2 ** 31), 2 ** 31 - 1), t) for s, t in shifts], np.int64)
    kw["cell"] = np.zeros((B, 2), np.int32)
    for b, (s, t) in enumerate(shifts):                                                  # s = memory_cell - cell, at the ends of int32 too
        if s == 2 ** 31 - 1:
            memory_cell[b, 0], kw["cell"][b, 0] = 2 ** 30, -2 ** 30 + 1
        if s == -2 ** 31:
            memory_cell[b, 0], kw["cell"][b, 0] = -2 ** 31, 2 ** 31 - 1                   # s = -2^32 + 1
    state = (np.repeat(row, B, axis=0), memory_cell.astype(np.int32))
    want = M.step(state, mark_d2=0, footprint_d2=-1, **kw)
    got = rule(state, kw, 0, -1)
    assert same(got, want)
    cells = M.bits_to_cells(row[0], width)
    for b, (s, t) in enumerate(shifts[:81]):
        assert M.bits_to_cells(got[3][0][b], width) == {(x + s, 0) for x, _ in cells if 0 <= x + s < width}
    assert all(not got[3][0][b].any() for b in range(81, B)) and len(cells) >= 8


# ---- the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mirror_matches_the_header_and_the_library_exports_the_function(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src))) == sorted(OA.FUNCTIONS) == ["smpc_obstacle_memory_batch"]
    assert re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S) == [st.c_name for st in OA.STRUCTS]
    inner = [f"scan.{f[0]}" for f in SA.SmpcSensedCostmapIn._fields_]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' + "".join(f'printf("%zu\\n", offsetof({st.c_name}, {f[0]}));\n' for f in st._fields_)
                   for st in OA.STRUCTS)
    body += "".join(f'printf("%zu\\n", offsetof(smpc_obstacle_memory_in, {name}));\n' for name in inner)
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc_obstacle_memory.h"\nint main(void){\n' + body + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [v for st in OA.STRUCTS for v in [C.sizeof(st)] + [getattr(st, f[0]).offset for f in st._fields_]]
    want += [OA.SmpcObstacleMemoryIn.scan.offset + getattr(SA.SmpcSensedCostmapIn, f[0]).offset for f in SA.SmpcSensedCostmapIn._fields_]
    assert values == want
    assert [C.sizeof(st) for st in OA.STRUCTS] == [128] and [f[0] for f in OA.SmpcObstacleMemoryIn._fields_] == ["scan", "mark_d2", "footprint_d2"]
    exported = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    lib = S.load_library()
    for name, (restype, argtypes) in OA.FUNCTIONS.items():
        assert f" {name}\n" in exported
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes


def test_the_main_abi_and_the_memoryless_header_are_as_they_were():
    from nav2_social_mpc_controller_amd import _abi
    assert _abi.SMPC_ABI_VERSION == 6 and len(_abi.FUNCTIONS) == 27 and not set(OA.FUNCTIONS) & (set(_abi.FUNCTIONS) | set(SA.FUNCTIONS))
    assert list(SA.FUNCTIONS) == ["smpc_sensed_costmap_batch"] and C.sizeof(SA.SmpcSensedCostmapIn) == 120


# ---- the parameters -------------------------------------------------------------------------------------------------------
def test_obstacle_memory_params():
    mp, sp = ObstacleMemoryParams(), SensorParams()
    assert (mp.raytrace_range, mp.footprint_radius) == (3.0, 0.24)
    beams = mp.beam_cells(sp, 0.05)
    assert beams.dtype == np.int32 and beams.shape == (360, 2) and beams[0].tolist() == [60, 0] and beams[90].tolist() == [0, 60]
    k = np.arange(360)
    assert np.array_equal(beams, np.stack([np.rint(60 * np.cos(2 * np.pi * k / 360)), np.rint(60 * np.sin(2 * np.pi * k / 360))], 1).astype(np.int32))
    # the same directions as the sensor's own beams, farther out
    assert np.array_equal(ObstacleMemoryParams(raytrace_range=2.5).beam_cells(sp, 0.05), sp.beam_cells(0.05))
    assert mp.mark_d2(sp, 0.05) == 2500 and mp.mark_d2(SensorParams(max_range=0.3), 0.05) == 36 == SensorParams(agent_radius=0.3).agent_d2(0.05)
    assert mp.footprint_d2(0.05) == 23 and ObstacleMemoryParams(footprint_radius=0.0).footprint_d2(0.05) == 0   # 4.8 cells: 23.04
    assert ObstacleMemoryParams(footprint_radius=None).footprint_d2(0.05) == -1
    assert ObstacleMemoryParams(footprint_radius=0.12).footprint_d2(0.05) == SensorParams(agent_radius=0.12).agent_d2(0.05) == 5
    assert mp.supported(sp, 0.05) and ObstacleMemoryParams(raytrace_range=127.0).supported(SensorParams(max_range=100.0), 1.0)
    assert not ObstacleMemoryParams(raytrace_range=127.5).supported(SensorParams(max_range=100.0), 1.0)
    for bad in (dict(raytrace_range=0.0), dict(raytrace_range=np.nan), dict(raytrace_range=np.inf), dict(footprint_radius=-0.1),
                dict(footprint_radius=np.nan)):
        with pytest.raises(ValueError):
            ObstacleMemoryParams(**bad)
    for call in (lambda m: m.beam_cells(sp, 0.05), lambda m: m.mark_d2(sp, 0.05), lambda m: m.check(sp)):
        with pytest.raises(ValueError):
            call(ObstacleMemoryParams(raytrace_range=2.4))                               # clears less far than the sensor marks
    ObstacleMemoryParams(raytrace_range=2.5).check(sp)
    scan = S.BatchSolver.sensed_costmap_c(5, 3, 24, 20, 96, 80, True, 0.05, 1, 64, 36, 196, 1, 77, 200, True)
    scan.world = 0x1234
    mi = S.BatchSolver.obstacle_memory_c(scan, 2500, 23)
    assert (mi.mark_d2, mi.footprint_d2, mi.scan.B, mi.scan.size_x, mi.scan.d2_max, mi.scan.outside_cost, mi.scan.world) == (2500, 23, 5, 24, 196, 77, 0x1234)
    assert S.BatchSolver.obstacle_memory_c(scan, 1).footprint_d2 == -1


def test_the_episode_declares_the_argument():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, TickRecord
    assert "sensor_memory" in BatchEpisode.FORWARDED and inspect.signature(BatchEpisode.__init__).parameters["sensor_memory"].default is None
    fields = TickRecord.__dataclass_fields__
    assert all(fields[name].default is None for name in ("obstacle_memory_before", "obstacle_memory_cell_before", "obstacle_memory_after"))


# ---- the kernel's resources ------------------------------------------------------------------------------------------------
def test_the_kernel_has_no_spills_no_scratch_and_lds_for_three_workgroups(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    r = subprocess.run(["bash", os.path.join(CSRC, "build.sh"), "-DSMPC_ONLY_NB=3", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage"],
                       env={**os.environ, "SMPC_OUT": str(tmp_path / "smpc_nb3.o")}, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    use = parse_resource_remarks(r.stderr).get(KERNEL)
    assert use is not None, "no resource remark for smpc_obstacle_memory_kernel"
    assert use["VGPRs Spill"] == 0 and use["SGPRs Spill"] == 0 and use["ScratchSize [bytes/lane]"] == 0, use
    assert use["LDS Size [bytes/block]"] <= LDS_BUDGET and use["Occupancy [waves/SIMD]"] >= 3, use
