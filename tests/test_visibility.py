"""The line-of-sight filter on the CPU: the yardstick itself (tests/visibility_ref.py, the sequential walk) against a
brute-force statement of the geometric definition and on hand-made rays, the `__host__ __device__` rule of
csrc/smpc_visibility_rule.hpp (the closed form per column) compiled into a host-only program against the reference, the
ctypes mirror against include/smpc_visibility.h, and VisibilityParams with its range bound."""
import ctypes as C
import itertools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import visibility_ref as V
from nav2_social_mpc_controller_amd import _abi_visibility as VA
from nav2_social_mpc_controller_amd import solver as S
from nav2_social_mpc_controller_amd.params import VisibilityParams
from test_kernel_budget import CSRC, HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc_visibility.h")
OCTANTS = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
CORNER_SLOPES = [(3, 1), (5, 3), (9, 3)]


# ---- the geometric definition, slowly ------------------------------------------------------------------------------------
def meets_interior(ex, ey, cx, cy):
    """Does the segment from the centre of cell (0,0) to the centre of cell (ex,ey) meet the open interior of cell (cx,cy)?
    In half cells: centres are odd points, cell c is the open square (2c, 2c + 2)^2; exact rational clipping."""
    lo, hi = Fraction(0), Fraction(1)          # the t of [0, 1] with the point strictly inside, as an open interval within
    for p, d, c in ((1, 2 * ex, 2 * cx), (1, 2 * ey, 2 * cy)):
        if d == 0:
            if not c < p < c + 2:
                return False
            continue
        t0, t1 = sorted((Fraction(c - p, d), Fraction(c + 2 - p, d)))
        lo, hi = max(lo, t0), min(hi, t1)
    # {t in [0,1]: every axis strictly inside}: the open interval (max t0, min t1) cut to [0, 1]
    return lo < hi


def geometry(ex, ey):
    """(cells met in their open interior, pairs of cells that touch the segment only at a lattice corner it passes through),
    relative to a = (0, 0), b = (ex, ey)."""
    xs, ys = range(min(0, ex), max(0, ex) + 1), range(min(0, ey), max(0, ey) + 1)
    met = {(cx, cy) for cx in xs for cy in ys if meets_interior(ex, ey, cx, cy)}
    pairs = []
    for u in range(min(0, ex), max(0, ex) + 2):
        for v in range(min(0, ey), max(0, ey) + 2):
            px, py = 2 * u - 1, 2 * v - 1      # the corner (2u, 2v) relative to a's centre (1, 1)
            on_line = px * (2 * ey) - py * (2 * ex) == 0
            inside = min(0, 2 * ex) <= px <= max(0, 2 * ex) and min(0, 2 * ey) <= py <= max(0, 2 * ey)
            if on_line and inside:
                touch = [c for c in ((u - 1, v - 1), (u, v - 1), (u - 1, v), (u, v)) if c not in met]
                assert len(touch) == 2, (ex, ey, u, v)   # a segment through a corner enters two opposite cells
                pairs.append(tuple(touch))
    return met, pairs


def brute_hidden(world, a, b, min_cost, unknown, cache={}):
    ex, ey = b[0] - a[0], b[1] - a[1]
    if (ex, ey) not in cache:
        cache[(ex, ey)] = geometry(ex, ey)
    met, pairs = cache[(ex, ey)]
    occ = lambda c: (c != (0, 0) and c != (ex, ey) and V.occludes(world, a[0] + c[0], a[1] + c[1], min_cost, unknown))
    return any(occ(c) for c in met) or any(occ(p) and occ(q) for p, q in pairs)


@pytest.mark.parametrize("Hx,Hy,seed,min_cost,unknown", [(9, 7, 1, 254, False), (7, 9, 2, 254, True), (9, 7, 3, 100, False),
                                                         (5, 4, 4, 254, False), (1, 6, 5, 254, False), (1, 1, 6, 0, True)])
def test_reference_walk_is_the_geometric_definition_for_every_ordered_pair_of_cells(Hx, Hy, seed, min_cost, unknown):
    g = np.random.default_rng(seed)
    world = g.choice(np.array([0, 0, 0, 0, 99, 100, 253, 254, 254, 255], np.uint8), (Hy, Hx))
    cells = list(itertools.product(range(Hx), range(Hy)))
    n_hidden = 0
    for a in cells:
        for b in cells:
            want = brute_hidden(world, a, b, min_cost, unknown)
            assert V.hidden(world, a, b, min_cost, unknown) == want, (a, b)
            assert V.hidden(world, b, a, min_cost, unknown) == want, (a, b)      # symmetry
            n_hidden += want
    if Hx * Hy >= 20:
        assert 0.1 * len(cells) ** 2 < n_hidden < 0.9 * len(cells) ** 2


def test_the_cells_and_corner_pairs_of_the_walk_are_those_of_the_geometry():
    for ex in range(-9, 10):
        for ey in range(-7, 8):
            met, pairs = geometry(ex, ey)
            cells, walked_pairs = V.walk_cells((2, -3), (2 + ex, -3 + ey))
            rel = lambda c: (c[0] - 2, c[1] + 3)
            assert len(set(cells)) == len(cells) and {rel(c) for c in cells} == met - {(0, 0), (ex, ey)}, (ex, ey)
            assert {frozenset(map(rel, p)) for p in walked_pairs} == {frozenset(p) for p in pairs}, (ex, ey)


# ---- hand-made rays -------------------------------------------------------------------------------------------------------
def blank(n=25):
    return np.zeros((n, n), np.uint8)


def test_axis_aligned_rays_and_exact_diagonals():
    a = (12, 12)
    for sx, sy in OCTANTS:
        for length in (1, 2, 7):
            for ex, ey in ((length, 0), (0, length), (length, length)):
                b = (a[0] + sx * ex, a[1] + sy * ey)
                w = blank()
                assert not V.hidden(w, a, b)
                w[a[1], a[0]] = w[b[1], b[0]] = 254                              # a and b themselves never occlude
                assert not V.hidden(w, a, b)
                steps = max(ex, ey)
                for k in range(1, steps):                                        # every cell strictly between hides
                    w2 = blank()
                    w2[a[1] + sy * (k if ey else 0), a[0] + sx * (k if ex else 0)] = 254
                    assert V.hidden(w2, a, b) and V.hidden(w2, b, a)
                if ex and ey:                                                    # a diagonal passes `length` corners
                    for k in range(length):
                        one, other = (a[0] + sx * (k + 1), a[1] + sy * k), (a[0] + sx * k, a[1] + sy * (k + 1))
                        for cells, want in (([one], False), ([other], False), ([one, other], True)):
                            w2 = blank()
                            for c in cells:
                                w2[c[1], c[0]] = 254
                            assert V.hidden(w2, a, b) == want and V.hidden(w2, b, a) == want, (a, b, cells)
                else:                                                            # walls along both sides of an axis ray
                    w2 = blank()
                    for k in range(-1, steps + 2):
                        for side in (-1, 1):
                            w2[a[1] + (sy * k if ey else side), a[0] + (sx * k if ex else side)] = 254
                    assert not V.hidden(w2, a, b) and not V.hidden(w2, b, a)


def corner_cases():
    """(a, b, one corner cell, the other) for the corner slopes in all eight octants: the segment of slope (p, q), p > q odd,
    passes the lattice corner in its middle (and (9, 3) two more)."""
    a = (12, 12)
    for p, q in CORNER_SLOPES:
        for swap in (False, True):
            for sx, sy in OCTANTS:
                ex, ey = (q, p) if swap else (p, q)
                b = (a[0] + sx * ex, a[1] + sy * ey)
                _, pairs = geometry(sx * ex, sy * ey)
                assert len(pairs) == (3 if (p, q) == (9, 3) else 1)
                for c0, c1 in pairs:
                    yield a, b, (a[0] + c0[0], a[1] + c0[1]), (a[0] + c1[0], a[1] + c1[1])


def test_corner_slopes_in_all_eight_octants_one_the_other_and_both_corner_cells():
    n = 0
    for a, b, one, other in corner_cases():
        for cells, want in (([one], False), ([other], False), ([one, other], True)):
            w = blank()
            for c in cells:
                w[c[1], c[0]] = 254
            assert V.hidden(w, a, b) == want and V.hidden(w, b, a) == want, (a, b, cells)
        n += 1
    assert n == (1 + 1 + 3) * 8


def test_unknown_cells_cells_outside_the_world_and_a_equal_b():
    w = blank(5)
    w[2, 2] = 255
    assert not V.hidden(w, (0, 2), (4, 2)) and V.hidden(w, (0, 2), (4, 2), unknown=True)
    assert not V.hidden(w, (0, 2), (4, 2), min_cost=255) and V.hidden(w, (0, 2), (4, 2), min_cost=255, unknown=True)
    w[2, 2] = 253
    assert not V.hidden(w, (0, 2), (4, 2)) and V.hidden(w, (0, 2), (4, 2), min_cost=253)
    w[2, 2] = 254
    assert V.hidden(w, (0, 2), (4, 2)) and V.hidden(w, (-3, 2), (9, 2)) and V.hidden(w, (2, -6), (2, 30))
    assert not V.hidden(w, (-3, 7), (9, 7)) and not V.hidden(w, (-5, -5), (-1, -9))     # wholly outside: transparent
    assert not V.hidden(w, (2, 2), (2, 2)) and not V.occludes(w, 5, 2) and not V.occludes(w, 2, -1)
    full = np.full((5, 5), 254, np.uint8)
    assert not V.hidden(full, (1, 1), (1, 1)) and not V.hidden(full, (1, 1), (2, 1))
    assert V.hidden(full, (1, 1), (2, 2)) and V.hidden(full, (1, 1), (3, 1))             # the corner pair; the cell between
    # classify: the codes in the contract's order
    o, res = np.array([0.0, 0.0]), 1.0
    assert V.classify(w, o, res, (0.5, 2.5), (4.5, 2.5)) == V.HIDDEN and V.classify(w, o, res, (0.5, 2.5), (0.7, 2.9)) == V.SEEN
    assert V.classify(w, o, res, (0.5, 2.5), (4.5, 2.5), max_range=3.0) == V.OUT_OF_RANGE
    assert V.classify(w, o, res, (np.nan, 2.5), (4.5, 2.5)) == V.NOT_FINITE and V.classify(w, o, res, (0.5, 2.5), (4.5, np.inf)) == V.NOT_FINITE
    assert V.classify(w, o, res, (2.0 ** 30 + 1.5, 0.5), (2.0 ** 30 + 1.5, 0.5)) == V.NOT_FINITE          # |q| > 2^30
    assert V.classify(w, o, res, (2.0 ** 30 + 0.5, 0.5), (2.0 ** 30 + 1.5, 0.5)) == V.SEEN                # |q| = 2^30
    assert V.classify(w, o, res, (0.5, 0.5), (1e300, 0.5)) == V.OUT_OF_RANGE


def test_the_range_gate_on_a_3_4_5_triangle():
    w, o = blank(12), np.array([0.0, 0.0])
    assert V.in_range(1.0, 2.0, 4.0, 6.0, 5.0) and not V.in_range(1.0, 2.0, 4.0, 6.0, np.nextafter(5.0, 0.0))
    assert V.classify(w, o, 1.0, (1.0, 2.0), (4.0, 6.0), max_range=5.0) == V.SEEN
    assert V.classify(w, o, 1.0, (1.0, 2.0), (4.0, 6.0), max_range=np.nextafter(5.0, 0.0)) == V.OUT_OF_RANGE
    assert V.classify(w, o, 1.0, (4.0, 6.0), (1.0, 2.0), max_range=np.nextafter(5.0, 0.0)) == V.OUT_OF_RANGE


def test_compaction_keeps_order_bits_and_the_rows_beyond_the_counts():
    w = blank(8)
    w[3, 3] = 254
    people = np.zeros((2, 4, 5))
    people[0, :, :2] = [[6.5, 3.5], [1.5, 5.5], [np.nan, 1.0], [2.5, 3.5]]
    people[1, :, :2] = [[0.5, 0.5], [0.5, 7.5], [50.0, 0.5], [0.6, 0.6]]
    people[:, :, 2:] = np.arange(24).reshape(2, 4, 3) + 0.25
    people[0, 1, 4] = -0.0
    pose = np.array([[0.5, 3.5, 0.0], [0.5, 0.5, 0.0]])
    vis, n, seen = V.visible_people(w, [0.0, 0.0], 1.0, pose, people, [4, 9], max_range=20.0)
    assert list(n) == [2, 3] and seen.tolist() == [[V.HIDDEN, V.SEEN, V.NOT_FINITE, V.SEEN], [V.SEEN, V.SEEN, V.OUT_OF_RANGE, V.SEEN]]
    assert V.same_bits(vis[0, :2], people[0, [1, 3]]) and V.same_bits(vis[1, :3], people[1, [0, 1, 3]])
    assert np.isnan(vis[0, 2:]).all() and np.isnan(vis[1, 3:]).all()
    vis, n, seen = V.visible_people(w, [0.0, 0.0], 1.0, pose, people, [-3, 1], max_range=20.0)
    assert list(n) == [0, 1] and (seen[0] == 0xEE).all() and seen[1].tolist() == [V.SEEN, 0xEE, 0xEE, 0xEE] and np.isnan(vis[0]).all()


# ---- the __host__ __device__ rule, compiled for the host -----------------------------------------------------------------
# queries, one per line: "w Hx Hy min unknown <Hx*Hy costs as hex pairs>" sets the world; "h ax ay bx by" -> hidden 0/1;
# "k rx ry px py ox oy res range" -> the seen code, composed as the kernel composes it; "o cost min unknown" -> occludes 0/1
PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "smpc_visibility_rule.hpp"
int main() {
  static char line[1 << 20];
  std::vector<unsigned char> world;
  int Hx = 0, Hy = 0;
  smpc::VisOcc vo{254u, 0u};
  const auto occ = [&](int32_t x, int32_t y) {
    if ((uint32_t)x >= (uint32_t)Hx || (uint32_t)y >= (uint32_t)Hy) return false;
    return smpc::vis_occludes(vo, world[(size_t)y * Hx + x]);
  };
  while (std::fgets(line, sizeof line, stdin)) {
    double rx, ry, px, py, ox, oy, res, range;
    int a, b, c, d, n = 0;
    unsigned u, v;
    if (std::sscanf(line, "w %d %d %u %u %n", &a, &b, &u, &v, &n) == 4) {
      Hx = a; Hy = b; vo.min_cost = u; vo.unknown = v;
      world.assign((size_t)Hx * Hy, 0);
      for (size_t i = 0; i < world.size(); ++i) { unsigned x; std::sscanf(line + n + 2 * i, "%2x", &x); world[i] = (unsigned char)x; }
      std::printf("ok\n");
    } else if (std::sscanf(line, "h %d %d %d %d", &a, &b, &c, &d) == 4) {
      std::printf("%d\n", smpc::vis_hidden(smpc::vis_ray(a, b, c, d), occ) ? 1 : 0);
    } else if (std::sscanf(line, "k %la %la %la %la %la %la %la %la", &rx, &ry, &px, &py, &ox, &oy, &res, &range) == 8) {
      int32_t ax = 0, ay = 0;
      unsigned code;
      if (!smpc::vis_robot_cell(rx, ry, ox, oy, res, &ax, &ay) || !(smpc::vis_finite(px) && smpc::vis_finite(py))) code = smpc::kSeenNotFinite;
      else if (!smpc::vis_in_range(rx, ry, px, py, range)) code = smpc::kSeenOutOfRange;
      else code = smpc::vis_hidden(smpc::vis_ray(ax, ay, (int32_t)smpc::vis_cell_axis(px, ox, res), (int32_t)smpc::vis_cell_axis(py, oy, res)), occ)
                      ? smpc::kSeenHidden : smpc::kSeenSeen;
      std::printf("%u\n", code);
    } else if (std::sscanf(line, "o %d %u %u", &a, &u, &v) == 3) {
      const smpc::VisOcc q{u, v};
      std::printf("%d\n", smpc::vis_occludes(q, (uint32_t)a) ? 1 : 0);
    } else {
      return 1;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    tmp = tmp_path_factory.mktemp("visibility_rule")
    src, exe = tmp / "probe.hip", tmp / "probe"
    src.write_text(PROBE)
    # -O3 as build.sh compiles the library: a fused multiply-add, if the compiler made one, would show here
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])

    def ask(lines):
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [l.split()[0] for l in out]

    return ask


def world_line(world, min_cost=254, unknown=False):
    return f"w {world.shape[1]} {world.shape[0]} {min_cost} {int(unknown)} " + world.tobytes().hex()


def hx(v):
    return float(v).hex()


def test_compiled_column_rule_is_the_reference_walk(rule):
    g = np.random.default_rng(61)
    # every ordered pair of cells of a 9 x 7 map, and of cells around it
    world = g.choice(np.array([0, 0, 0, 100, 254, 254, 255], np.uint8), (7, 9))
    cells = list(itertools.product(range(-1, 10), range(-1, 8)))
    for min_cost, unknown in ((254, False), (254, True), (100, False)):
        pairs = [(a, b) for a in cells for b in cells]
        got = rule([world_line(world, min_cost, unknown)] + [f"h {a[0]} {a[1]} {b[0]} {b[1]}" for a, b in pairs])[1:]
        want = [V.hidden(world, a, b, min_cost, unknown) for a, b in pairs]
        assert [v == "1" for v in got] == want
    # long random rays over a larger random map, a third of the cells occluding near the diagonal to keep some rays open
    world = (g.random((120, 150)) < 0.004).astype(np.uint8) * 254
    a, b = g.integers(-20, 170, (3000, 2)), g.integers(-20, 170, (3000, 2))
    b[:200] = a[:200] + g.integers(-1, 2, (200, 2)) * g.integers(1, 140, (200, 1))          # axis-aligned and exact diagonals
    got = rule([world_line(world)] + [f"h {p[0]} {p[1]} {q[0]} {q[1]}" for p, q in zip(a, b)])[1:]
    want = [V.hidden(world, p, q) for p, q in zip(a, b)]
    assert [v == "1" for v in got] == want and 0.2 < np.mean(want) < 0.8
    # the corner slopes, one, the other and both
    lines, want = [], []
    for ca, cb, one, other in corner_cases():
        for cells_, hid in (([one], False), ([other], False), ([one, other], True)):
            w = blank()
            for c in cells_:
                w[c[1], c[0]] = 254
            lines += [world_line(w), f"h {ca[0]} {ca[1]} {cb[0]} {cb[1]}", f"h {cb[0]} {cb[1]} {ca[0]} {ca[1]}"]
            want += ["ok", str(int(hid)), str(int(hid))]
    assert rule(lines) == want
    # the longest supported ray: 32769 cells along both axes, around cells of magnitude 2^30
    far = 2 ** 30
    empty = np.zeros((1, 1), np.uint8)
    assert rule([world_line(empty), f"h {far} {-far} {far + 32769} {-far - 32769}", f"h {far} {far} {far - 32769} {far + 32768}"])[1:] == ["0", "0"]
    got = rule([f"o {c} {m} {u}" for c in range(256) for m in (0, 1, 254, 255) for u in (0, 1)])
    assert got == [str(int(c >= m and (c != 255 or bool(u)))) for c in range(256) for m in (0, 1, 254, 255) for u in (0, 1)]


def test_compiled_classification_agrees_with_the_reference_on_edges_ulps_and_non_finite_points(rule):
    g = np.random.default_rng(62)
    origin, res, rng = np.array([-3.2, 1.15]), 0.05, 3.0
    world = (g.random((192, 256)) < 0.01).astype(np.uint8) * 254
    world[g.integers(0, 192, 200), g.integers(0, 256, 200)] = 255
    edges = origin + g.integers(-3, 260, (500, 2)) * res                       # on cell edges (up to rounding) ...
    beside = np.concatenate([np.nextafter(edges, np.inf), np.nextafter(edges, -np.inf)])   # ... and one ulp to either side
    special = np.array([[1e12, 2.0], [-1e12, 2.0], [0.0, 1e12], [0.0, -1e12], [np.nan, 2.0], [0.0, np.nan], [np.inf, 2.0], [0.0, -np.inf],
                        [np.nan, np.inf], [1e300, -1e300], [-1e300, 1e300], origin, [-0.0, 1.15]])
    pts = np.concatenate([edges, beside, g.uniform(-4.0, 12.0, (1500, 2)), special])
    robots = pts[g.permutation(len(pts))]
    robots[::3] = pts[::3] + g.uniform(-2.5, 2.5, (len(pts[::3]), 2))          # most pairs within range of each other
    lines = [world_line(world)] + [f"k {hx(r[0])} {hx(r[1])} {hx(p[0])} {hx(p[1])} {hx(origin[0])} {hx(origin[1])} {hx(res)} {hx(rng)}"
                                   for r, p in zip(robots, pts)]
    got = [int(v) for v in rule(lines)[1:]]
    want = [V.classify(world, origin, res, r, p, rng) for r, p in zip(robots, pts)]
    assert got == want
    assert all(want.count(code) > 30 for code in (V.HIDDEN, V.SEEN, V.OUT_OF_RANGE)) and want.count(V.NOT_FINITE) >= 10
    # the range gate: the 3-4-5 triangle and one ulp below, and the robot's 2^30 bound
    o = [hx(0.0), hx(0.0), hx(1.0)]
    far = 2.0 ** 30
    lines = [world_line(np.zeros((1, 1), np.uint8)),
             " ".join(["k", hx(1.0), hx(2.0), hx(4.0), hx(6.0)] + o + [hx(5.0)]),
             " ".join(["k", hx(1.0), hx(2.0), hx(4.0), hx(6.0)] + o + [hx(np.nextafter(5.0, 0.0))]),
             " ".join(["k", hx(far + 0.5), hx(0.5), hx(far + 1.5), hx(0.5)] + o + [hx(5.0)]),
             " ".join(["k", hx(far + 1.5), hx(0.5), hx(far + 1.5), hx(0.5)] + o + [hx(5.0)]),
             " ".join(["k", hx(-far - 0.5), hx(0.5), hx(-far - 0.5), hx(0.5)] + o + [hx(5.0)]),
             " ".join(["k", hx(0.5), hx(-far), hx(0.5), hx(-far)] + o + [hx(5.0)])]
    assert [int(v) for v in rule(lines)[1:]] == [V.SEEN, V.OUT_OF_RANGE, V.SEEN, V.NOT_FINITE, V.NOT_FINITE, V.SEEN]


# ---- the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mirror_matches_the_header_and_the_library_exports_the_function(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src))) == sorted(VA.FUNCTIONS) == ["smpc_visible_people_batch"]
    assert re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S) == [st.c_name for st in VA.STRUCTS]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' + "".join(f'printf("%zu\\n", offsetof({st.c_name}, {f[0]}));\n' for f in st._fields_)
                   for st in VA.STRUCTS)
    body += "".join(f'printf("%d\\n", (int)SMPC_SEEN_{name});\n' for name in VA.SEEN_CODES)
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc_visibility.h"\nint main(void){\n' + body + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [v for st in VA.STRUCTS for v in [C.sizeof(st)] + [getattr(st, f[0]).offset for f in st._fields_]]
    assert values == want + list(range(len(VA.SEEN_CODES)))
    assert [C.sizeof(st) for st in VA.STRUCTS] == [88]
    assert [V.HIDDEN, V.SEEN, V.OUT_OF_RANGE, V.NOT_FINITE] == list(range(4))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    lib = S.load_library()
    for name, (restype, argtypes) in VA.FUNCTIONS.items():
        assert f" {name}\n" in exported
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes


def test_the_main_abi_is_as_it_was():
    from nav2_social_mpc_controller_amd import _abi
    assert _abi.SMPC_ABI_VERSION == 6 and len(_abi.FUNCTIONS) == 27 and not set(VA.FUNCTIONS) & set(_abi.FUNCTIONS)


# ---- the parameters -------------------------------------------------------------------------------------------------------
def test_visibility_params_defaults_checks_and_the_range_bound_at_32768_cells():
    vp = VisibilityParams()
    assert (vp.max_range, vp.occlusion_min_cost, vp.unknown_occludes) == (10.0, 254, False)
    for bad in (dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=np.inf), dict(max_range=np.nan), dict(occlusion_min_cost=256),
                dict(occlusion_min_cost=-1)):
        with pytest.raises(ValueError):
            VisibilityParams(**bad)
    assert vp.supported(0.05) and VisibilityParams(max_range=32768.0).supported(1.0)
    assert not VisibilityParams(max_range=np.nextafter(32768.0, np.inf)).supported(1.0)
    assert VisibilityParams(max_range=1638.4).supported(0.05) == bool(np.float64(1638.4) / np.float64(0.05) <= 32768.0)
    assert VisibilityParams(max_range=8192.0).supported(0.25) and not VisibilityParams(max_range=8192.5).supported(0.25)
    st = S.BatchSolver.visibility_c(VisibilityParams(7.5, 200, True), 5, 3, 11, 13, False, 0.25, 1)
    assert (st.B, st.Np, st.on_device, st.world_x, st.world_y, st.world_shared) == (5, 3, 1, 11, 13, 0)
    assert (st.occlusion_min_cost, st.unknown_occludes, st.resolution, st.max_range) == (200, 1, 0.25, 7.5)


def test_the_episode_declares_the_argument_and_refuses_it_without_a_world():
    import inspect

    from nav2_social_mpc_controller_amd.episode import BatchEpisode, TickRecord
    assert "visibility" in BatchEpisode.FORWARDED and inspect.signature(BatchEpisode.__init__).parameters["visibility"].default is None
    assert {"person_seen", "seen_count", "seen_persons"} <= set(TickRecord.__dataclass_fields__)
