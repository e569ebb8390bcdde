"""Sensed local costmaps on the CPU: the yardstick itself (tests/sensed_costmap_ref.py, the sequential walk and brute-force
inflation) on hand-made calls, the `__host__ __device__` rule of csrc/smpc_sensed_costmap_rule.hpp (closed-form columns, row
gaps from bit masks) compiled into a host-only program against the yardstick on random calls, the ctypes mirror against
include/smpc_sensed_costmap.h, SensorParams' tables, the episode's declarations, and the kernel's resource remarks."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import sensed_costmap_cases as K
import sensed_costmap_ref as R
from nav2_social_mpc_controller_amd import _abi_sensed_costmap as SA
from nav2_social_mpc_controller_amd import solver as S
from nav2_social_mpc_controller_amd.params import SensorParams
from test_kernel_budget import CSRC, HIPCC, parse_resource_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc_sensed_costmap.h")
KERNEL = "_ZN4smpc26smpc_sensed_costmap_kernelENS_19SensedCostmapParamsE"


# ---- the yardstick on hand-made calls -------------------------------------------------------------------------------------
HAND = K.hand_cases()


@pytest.fixture(scope="module")
def hand():
    return {name: R.sensed_costmap(**kw) for name, (kw, _) in HAND.items()}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_beams_have_the_kinds_and_cells_the_contract_gives(hand, name):
    _, kind, hit = hand[name]
    want = HAND[name][1]
    assert want
    for (b, k), (want_kind, want_cell) in want.items():
        assert (int(kind[b, k]), tuple(int(v) for v in hit[b, k])) == (want_kind, want_cell), (name, b, k)


def disc(table, centre, size=(21, 21)):
    """The inflation of one mark, from the table, cell by cell."""
    out = np.zeros((size[1], size[0]), np.uint8)
    for y in range(size[1]):
        for x in range(size[0]):
            d2 = (x - centre[0]) ** 2 + (y - centre[1]) ** 2
            out[y, x] = table[d2] if d2 < len(table) else 0
    return out


def test_hand_made_windows():
    cm = lambda name: R.sensed_costmap(**HAND[name][0])[0]
    assert np.array_equal(cm("axis")[0], disc(K.TABLE, (13, 10))) and cm("axis")[0, 10, 13] == 254 and cm("axis")[0, 12, 13] == 100
    assert np.array_equal(cm("corner_both")[0], np.maximum(disc(K.TABLE, (11, 10)), disc(K.TABLE, (10, 11))))      # both cells of the pair
    assert not cm("corner_one").any() and not cm("corner_other").any() and not cm("robot_cell_never_stops").any()
    assert np.array_equal(cm("corner_slope")[0], np.maximum.reduce([disc(K.TABLE, c) for c in ((12, 10), (11, 11), (9, 11), (10, 12))]))
    assert np.array_equal(cm("agent_before_wall")[0], disc(K.TABLE, (12, 10)))          # the disc's near cell; the wall behind is not seen
    assert np.array_equal(cm("wall_before_agent")[0], disc(K.TABLE, (12, 10)))
    assert np.array_equal(cm("agent_off_world")[0], disc(K.TABLE, (7, 8)))              # world cell (-1, 10) in the window at (-8, 2)
    assert not cm("hit_outside_window").any()                                            # the hit is dropped
    assert np.array_equal(cm("robot_outside_window_and_world")[0], disc(K.TABLE, (2, 2), (8, 5)))
    # no robot: nothing is cast, the window is still written: the world cut under base 1
    kw = HAND["no_robot"][0]
    got, cut = cm("no_robot"), R.world_cut(kw["world"], (5, 5), 9, 9, 255)
    assert all(np.array_equal(got[b], cut) for b in range(3)) and cut[5, 8] == 254 and (cut == 254).sum() == 1
    assert np.array_equal(got[3], np.maximum(cut, disc(K.TABLE, (8, 5), (9, 9))))
    # the window hangs over the world's edge: base 0 free, base 1 the cut with outside_cost beyond the edge
    kw = HAND["edge_base1"][0]
    free, based = cm("edge_base0")[0], cm("edge_base1")[0]
    cut = R.world_cut(kw["world"], (-3, -2), 12, 9, 77)
    assert np.array_equal(free, disc(K.TABLE, (4, 3), (12, 9))) and np.array_equal(based, np.maximum(free, cut))
    assert cut[0, 0] == 77 and cut[8, 11] == 77 and cut[2, 3] == 0 and cut[3, 4] == 254 and cut[5, 3] == 100 and cut[2, 7] == 255
    assert (cut == 77).sum() == 12 * 9 - 7 * 6
    # a table that is not monotone: the nearest mark decides, not the largest cost
    odd = cm("odd_table")[0]
    marks = [(13, 10), (10, 6), (7, 11)]                                                  # the agent's disc cell nearest the beam's walk
    assert R.sensed_costmap(**HAND["odd_table"][0])[2][0, 2].tolist() == [-3, 1]
    want = np.zeros((21, 21), np.uint8)
    for y in range(21):
        for x in range(21):
            d2 = min((x - mx) ** 2 + (y - my) ** 2 for mx, my in marks)
            want[y, x] = K.ODD_TABLE[d2] if d2 <= 8 else 0
    assert np.array_equal(odd, want) and odd[10, 14] == 10 and odd[11, 14] == 200 and odd[11, 15] == 7 and odd[12, 15] == 33 and odd[10, 15] == 90
    assert odd[11, 12] == 200 and odd[12, 11] == 33                                       # d2 = 2 to (13, 10); d2 = 8 to (13, 10), 17 to (7, 11)
    # cells at the 2^30 bound and a window cell at the end of int32: no overflow, nothing marked off the window
    far = cm("far_cells")
    assert np.array_equal(far[0], disc(K.TABLE, (2, 1), (6, 6))) and not far[1].any()


# ---- the __host__ __device__ rule, compiled for the host -----------------------------------------------------------------
# One robot per query, whitespace-separated: Hx Hy min unknown size_x size_y cell_x cell_y agent_d2 d2_max base outside K Np
# count res ox oy rx ry (the doubles as hex floats), the world and the table as hex strings, K beam offsets, Np agent
# points. Composed as the kernel composes it: occupancy bitmap of the reach square, sc_cast, sc_window_cell into padded row
# masks, sc_row_gap, sc_least_d2 over the rows within r, sc_cost. Answer: the kinds, the beam cells, the window as hex.
PROBE = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "smpc_sensed_costmap_rule.hpp"
static double num(const std::string& s) { return std::strtod(s.c_str(), nullptr); }
static std::vector<unsigned char> bytes(const std::string& s) {
  std::vector<unsigned char> v(s.size() / 2);
  for (size_t i = 0; i < v.size(); ++i) v[i] = (unsigned char)std::stoi(s.substr(2 * i, 2), nullptr, 16);
  return v;
}
int main() {
  long long Hx, Hy, mn, unk, sx, sy, cellx, celly, agent_d2, d2_max, base, outside, K, Np, count;
  while (std::cin >> Hx >> Hy >> mn >> unk >> sx >> sy >> cellx >> celly >> agent_d2 >> d2_max >> base >> outside >> K >> Np >> count) {
    std::string t[5], ws, ts;
    for (auto& s : t) std::cin >> s;
    std::cin >> ws >> ts;
    const double res = num(t[0]), ox = num(t[1]), oy = num(t[2]), rx = num(t[3]), ry = num(t[4]);
    const std::vector<unsigned char> world = bytes(ws), table = bytes(ts);
    std::vector<long long> beams(2 * K);
    for (auto& v : beams) std::cin >> v;
    std::vector<std::string> pts(2 * Np);
    for (auto& s : pts) std::cin >> s;
    const smpc::VisOcc vo{(uint32_t)mn, (uint32_t)unk};
    int32_t ax = 0, ay = 0;
    const bool robot_ok = smpc::vis_robot_cell(rx, ry, ox, oy, res, &ax, &ay);
    std::vector<unsigned char> occupied(255 * 255, 0);
    const long long cnt = count < 0 ? 0 : (count > Np ? Np : count);
    long long ra = (long long)std::sqrt((double)agent_d2);
    while (ra * ra > agent_d2) --ra;
    while ((ra + 1) * (ra + 1) <= agent_d2) ++ra;
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
    std::vector<uint32_t> marks(256 * 10, 0u);
    const auto mark = [&](int32_t cx, int32_t cy) {
      int32_t wx = 0, wy = 0;
      if (smpc::sc_window_cell(ax, ay, cx, cy, (int32_t)cellx, (int32_t)celly, (int32_t)sx, (int32_t)sy, &wx, &wy))
        marks[wy * 10 + 1 + (wx >> 5)] |= 1u << (wx & 31);
    };
    std::string kinds, cells;
    for (long long k = 0; k < K; ++k) {
      const int32_t ex = (int32_t)beams[2 * k], ey = (int32_t)beams[2 * k + 1];
      uint32_t kind = smpc::kBeamNoRobot;
      int32_t hx = ex, hy = ey;
      if (robot_ok) {
        kind = smpc::kBeamInvalid;
        if (smpc::sc_beam_valid(ex, ey)) {
          const smpc::ScHit h = smpc::sc_cast(ex, ey, stops);
          kind = h.kind; hx = h.ox; hy = h.oy;
          if (kind != smpc::kBeamNone) mark(h.ox, h.oy);
          if (kind == smpc::kBeamCornerPair) mark(h.px, h.py);
        }
      }
      kinds += std::to_string(kind) + ",";
      cells += std::to_string(hx) + "," + std::to_string(hy) + ",";
    }
    long long r = (long long)std::sqrt((double)d2_max);
    while (r * r > d2_max) --r;
    while ((r + 1) * (r + 1) <= d2_max) ++r;
    std::vector<unsigned char> gap(sx * sy);
    for (long long y = 0; y < sy; ++y)
      for (long long x = 0; x < sx; ++x) {
        const uint32_t* line = &marks[y * 10 + (x >> 5)];
        const uint32_t sh = (uint32_t)(x & 31), w2 = line[2];
        const uint64_t w01 = ((uint64_t)line[1] << 32) | line[0];
        const uint64_t v = sh ? (w01 >> sh) | ((uint64_t)w2 << (64u - sh)) : w01;
        gap[y * sx + x] = (unsigned char)smpc::sc_row_gap(v, w2 >> sh, (uint32_t)r);
      }
    std::string out;
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
    std::printf("%s %s %s\n", kinds.c_str(), cells.c_str(), out.c_str());
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    tmp = tmp_path_factory.mktemp("sensed_rule")
    src, exe = tmp / "probe.hip", tmp / "probe"
    src.write_text(PROBE)
    # -O3 as build.sh compiles the library
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])

    def ask(kw):
        """The compiled rule's (costmap, beam_kind, beam_cell) of one call, robot by robot."""
        world, origin = np.asarray(kw["world"], np.uint8), np.asarray(kw["origin"], np.float64).reshape(-1, 2)
        B, Np, beams = kw["people"].shape[0], kw["people"].shape[1], np.asarray(kw["beam_cells"], np.int64)
        hx = lambda v: float(v).hex() if np.isfinite(v) else repr(float(v))
        lines = []
        for b in range(B):
            w, o = (world, origin[0]) if world.ndim == 2 else (world[b], origin[b])
            lines.append(" ".join(map(str, [w.shape[1], w.shape[0], kw["min_cost"], int(kw["unknown"]), kw["size_x"], kw["size_y"],
                                            kw["cell"][b, 0], kw["cell"][b, 1], kw["agent_d2"], len(kw["table"]) - 1, kw["base"],
                                            kw["outside_cost"], len(beams), Np, kw["count"][b]]
                                      + [hx(v) for v in (kw["res"], o[0], o[1], kw["robot_pose"][b, 0], kw["robot_pose"][b, 1])]
                                      + [w.tobytes().hex(), np.asarray(kw["table"], np.uint8).tobytes().hex()]
                                      + beams.ravel().tolist() + [hx(v) for v in kw["people"][b, :, :2].ravel()])))
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == B
        cm = np.zeros((B, kw["size_y"], kw["size_x"]), np.uint8)
        kind, hit = np.zeros((B, len(beams)), np.uint8), np.zeros((B, len(beams), 2), np.int32)
        for b, line in enumerate(out):
            kinds, cells, window = line.split()
            kind[b] = [int(v) for v in kinds.split(",")[:-1]]
            hit[b] = np.array([int(v) for v in cells.split(",")[:-1]]).reshape(-1, 2)
            cm[b] = np.frombuffer(bytes.fromhex(window), np.uint8).reshape(kw["size_y"], kw["size_x"])
        return cm, kind, hit

    return ask


def same(got, want):
    return all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))


def test_compiled_rule_is_the_yardstick_on_the_hand_made_calls(rule, hand):
    for name, (kw, _) in HAND.items():
        assert same(rule(kw), hand[name]), name


@pytest.mark.parametrize("seed,reach,size,r,base", [(1, 10, (24, 20), 3, 0), (2, 30, (24, 20), 3, 1), (3, 10, (37, 70), 5, 1),
                                                    (4, 60, (90, 41), 9, 0), (5, 127, (256, 33), 32, 0)])
def test_compiled_rule_is_the_yardstick_on_random_calls(rule, seed, reach, size, r, base):
    kw = K.random_case(seed=seed, reach=reach, size=size, r=r, base=base, off_fraction=0.3, world_size=(96, 80) if reach < 60 else (300, 200),
                       n_beams=64 if reach < 60 else 180)
    stats = {}
    want = R.sensed_costmap(**kw, stats=stats)
    assert same(rule(kw), want)
    assert {R.NONE, R.WORLD, R.AGENT} <= set(want[1].ravel()) and (stats["marks"] >= 3).sum() >= 2


def test_compiled_rule_on_every_beam_of_a_square_around_a_cluttered_robot(rule):
    """Every end offset within 12 cells, over a random clutter of walls and one agent: the closed-form columns give the walk's
    first hit, pairs included, in all eight octants."""
    g = np.random.default_rng(7)
    world = (g.random((31, 31)) < 0.12).astype(np.uint8) * 254
    beams = [(x, y) for x in range(-12, 13) for y in range(-12, 13)]
    kw, _ = K.case(robots=[(15, 15)], agents=[[(19, 12)]], agent_d2=2, beams=beams, size=(31, 31), world_size=(31, 31))
    kw["world"] = world
    want = R.sensed_costmap(**kw)
    assert same(rule(kw), want)
    assert np.bincount(want[1].ravel(), minlength=4)[:4].min() >= 5                     # none, world, agent and pairs all occur


def test_row_gap_from_bit_masks_is_the_nearest_mark_of_the_row(rule):
    """One-row windows of every width class with random marks: the gaps behind the costs, through a table that names d2."""
    g = np.random.default_rng(9)
    table = (np.arange(33 * 33 + 1) % 251 + 1).astype(np.uint8)                          # r = 33 > 32 is not asked for: d2_max = 1024 below
    table = table[:1025]
    for width, density in ((1, 1.0), (31, 0.1), (32, 0.05), (33, 0.05), (64, 0.02), (65, 0.02), (200, 0.01), (255, 0.004), (256, 0.004), (256, 0.0)):
        marks = np.flatnonzero(g.random(width) < density)
        walls = [(int(x), 1) for x in marks]
        # one robot in row 0 looking straight up at each marked cell of row 1: every mark is a hit of its own beam
        for robot_x in ([int(marks[0])] if len(marks) else [0]):
            beams = [(int(x) - robot_x, 1) for x in marks if abs(int(x) - robot_x) <= 127] or [(0, 0)]
            kw, _ = K.case(walls=walls, robots=[(robot_x, 0)], beams=beams, size=(width, 1), cell=(0, 1), world_size=(width, 2), table=table)
            want = R.sensed_costmap(**kw)
            assert same(rule(kw), want), width


# ---- the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mirror_matches_the_header_and_the_library_exports_the_function(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src))) == sorted(SA.FUNCTIONS) == ["smpc_sensed_costmap_batch"]
    assert re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S) == [st.c_name for st in SA.STRUCTS]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' + "".join(f'printf("%zu\\n", offsetof({st.c_name}, {f[0]}));\n' for f in st._fields_)
                   for st in SA.STRUCTS)
    body += "".join(f'printf("%d\\n", (int)SMPC_BEAM_{name});\n' for name in SA.BEAM_KINDS)
    body += "".join(f'printf("%d\\n", (int)SMPC_SENSED_{name});\n' for name in SA.LIMITS)
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc_sensed_costmap.h"\nint main(void){\n' + body + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [v for st in SA.STRUCTS for v in [C.sizeof(st)] + [getattr(st, f[0]).offset for f in st._fields_]]
    assert values == want + list(range(len(SA.BEAM_KINDS))) + list(SA.LIMITS.values())
    assert [C.sizeof(st) for st in SA.STRUCTS] == [120]
    assert [R.NONE, R.WORLD, R.AGENT, R.CORNER_PAIR, R.INVALID, R.NO_ROBOT] == list(range(6)) and R.MAX_REACH == SA.LIMITS["MAX_REACH"]
    exported = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    lib = S.load_library()
    for name, (restype, argtypes) in SA.FUNCTIONS.items():
        assert f" {name}\n" in exported
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes


def test_the_main_abi_is_as_it_was():
    from nav2_social_mpc_controller_amd import _abi
    assert _abi.SMPC_ABI_VERSION == 6 and len(_abi.FUNCTIONS) == 27 and not set(SA.FUNCTIONS) & set(_abi.FUNCTIONS)


# ---- the parameters -------------------------------------------------------------------------------------------------------
def test_sensor_params_defaults_and_tables():
    sp = SensorParams()
    assert (sp.n_beams, sp.max_range, sp.agent_radius, sp.inflation_radius, sp.cost_scaling_factor, sp.inscribed_radius,
            sp.occlusion_min_cost, sp.unknown_occludes, sp.base) == (360, 2.5, 0.3, 0.7, 3.0, 0.0, 254, False, "free")
    table, d2_max = sp.inflation_table(0.05)
    assert d2_max == 14 * 14 and table.dtype == np.uint8 and table.shape == (197,)       # 0.7 m at 0.05 m: r = 14, not 13
    assert table[0] == 254 and (np.diff(table.astype(int)) <= 0).all()                   # non-increasing
    assert table[1] == int(252 * np.exp(-3.0 * 0.05)) and table[196] == int(252 * np.exp(-3.0 * 0.7)) and table[196] > 0
    for res, r in ((0.05, 14), (0.1, 7), (0.025, 28), (0.7, 1), (1.0, 0)):
        assert SensorParams().inflation_table(res)[1] == r * r
    t, _ = SensorParams(inscribed_radius=0.11).inflation_table(0.05)
    assert t[0] == 254 and t[1] == 253 and t[4] == 253 and t[5] == int(252 * np.exp(-3.0 * (np.sqrt(5.0) * 0.05 - 0.11)))
    assert sp.agent_d2(0.05) == 36 and SensorParams(agent_radius=0.0).agent_d2(0.05) == 0 and SensorParams(agent_radius=0.12).agent_d2(0.05) == 5
    beams = sp.beam_cells(0.05)
    assert beams.dtype == np.int32 and beams.shape == (360, 2) and beams[0].tolist() == [50, 0] and beams[90].tolist() == [0, 50]
    assert beams[180].tolist() == [-50, 0] and beams[45].tolist() == [35, 35] and np.abs(beams).max() == 50
    k = np.arange(360)
    assert np.array_equal(beams, np.stack([np.rint(50 * np.cos(2 * np.pi * k / 360)), np.rint(50 * np.sin(2 * np.pi * k / 360))], 1).astype(np.int32))
    assert sp.supported(0.05) and SensorParams(max_range=127.0).supported(1.0) and not SensorParams(max_range=127.5).supported(1.0)
    assert SensorParams(inflation_radius=32.0).supported(1.0) and not SensorParams(inflation_radius=33.0).supported(1.0)
    for bad in (dict(n_beams=0), dict(n_beams=4097), dict(max_range=0.0), dict(max_range=np.nan), dict(agent_radius=-0.1),
                dict(inflation_radius=np.inf), dict(cost_scaling_factor=0.0), dict(occlusion_min_cost=256), dict(base="static")):
        with pytest.raises(ValueError):
            SensorParams(**bad)
    st = S.BatchSolver.sensed_costmap_c(5, 3, 24, 20, 96, 80, True, 0.05, 1, 64, 36, 196, 1, 77, 200, True)
    assert (st.B, st.Np, st.on_device, st.size_x, st.size_y, st.world_x, st.world_y, st.world_shared) == (5, 3, 1, 24, 20, 96, 80, 1)
    assert (st.n_beams, st.agent_d2, st.d2_max, st.base, st.outside_cost, st.occlusion_min_cost, st.unknown_occludes, st.resolution) == \
        (64, 36, 196, 1, 77, 200, 1, 0.05)


def test_the_episode_declares_the_argument():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, TickRecord
    assert "sensor" in BatchEpisode.FORWARDED and inspect.signature(BatchEpisode.__init__).parameters["sensor"].default is None
    fields = TickRecord.__dataclass_fields__
    assert all(fields[name].default is None for name in ("sensed_costmap", "beam_kind", "beam_cell"))


# ---- the kernel's resources ------------------------------------------------------------------------------------------------
def test_the_kernel_has_no_spills_and_no_private_segment(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    r = subprocess.run(["bash", os.path.join(CSRC, "build.sh"), "-DSMPC_ONLY_NB=3", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage"],
                       env={**os.environ, "SMPC_OUT": str(tmp_path / "smpc_nb3.o")}, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    use = parse_resource_remarks(r.stderr).get(KERNEL)
    assert use is not None, "no resource remark for smpc_sensed_costmap_kernel"
    assert use["VGPRs Spill"] == 0 and use["SGPRs Spill"] == 0 and use["ScratchSize [bytes/lane]"] == 0, use
    assert use["LDS Size [bytes/block]"] <= 64 * 1024 and use["Occupancy [waves/SIMD]"] >= 2
