"""The nearest-agent gather of a shared world on the CPU: the yardstick itself (tests/nearest_ref.py) against a plain-Python
sorted() statement and on hand-made cases, the `__host__ __device__` rule of csrc/smpc_nearest_rule.hpp compiled into a
host-only program against numpy, the 3 x 3 property of the bins under attack, the ctypes mirror against
include/smpc_nearest.h, SharedWorldParams.grid, scenes.shared_pool and the episode's arguments."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import nearest_ref as R
from nav2_social_mpc_controller_amd import _abi_nearest as NA
from nav2_social_mpc_controller_amd import solver as S
from nav2_social_mpc_controller_amd.params import SharedWorldParams
from nav2_social_mpc_controller_amd.scenes import World, make_world, shared_pool
from test_kernel_budget import CSRC, HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc_nearest.h")
UP, DOWN = np.inf, -np.inf


def table(xy, seed=0):
    """Agent rows x, y with recognisable velocity columns."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    rows = np.zeros((len(xy), 5))
    rows[:, 0:2] = xy
    rows[:, 2:5] = np.arange(3 * len(xy)).reshape(-1, 3) + 0.25 + seed
    return rows


def plain(agents, pose, Np, max_range, self_row=None):
    """Rule 2, 4 and 5 in plain Python floats: [(rows of agents, nearest first)] per robot."""
    out = []
    for b, (rx, ry) in enumerate(np.asarray(pose)[:, :2].tolist()):
        keys = []
        for c, (ax, ay) in enumerate(np.asarray(agents)[:, :2].tolist()):
            if self_row is not None and c == self_row[b]:
                continue
            if not all(np.isfinite(v) for v in (rx, ry, ax, ay)):
                continue
            ddx, ddy = ax - rx, ay - ry
            d2 = ddx * ddx + ddy * ddy
            if d2 <= max_range * max_range:
                keys.append((d2, c))
        out.append([c for _, c in sorted(keys)][:Np])
    return out


def check(agents, pose, Np, max_range, self_row=None):
    people, count, source = R.nearest_people(agents, pose, Np, max_range, self_row)
    want = plain(agents, pose, Np, max_range, self_row)
    for b, rows in enumerate(want):
        assert count[b] == len(rows) and source[b, :len(rows)].tolist() == rows, (b, rows, source[b])
        assert R.same_bits(people[b, :len(rows)], np.asarray(agents)[rows].reshape(-1, 5))
        assert np.isnan(people[b, len(rows):]).all() and (source[b, len(rows):] == -1).all()
    return people, count, source


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,B,Np,seed", [(0, 3, 4, 1), (1, 1, 1, 2), (40, 7, 8, 3), (150, 9, 64, 4), (90, 5, 3, 5)])
def test_reference_is_a_sorted_statement_on_random_tables(A, B, Np, seed):
    g = np.random.default_rng(seed)
    agents = table(np.round(g.uniform(-6.0, 6.0, (A, 2)), 1), seed)      # one decimal: equal distances happen
    pose = np.concatenate([np.round(g.uniform(-6.0, 6.0, (B, 2)), 1), g.uniform(-3.0, 3.0, (B, 1))], axis=1)
    self_row = g.integers(-2, max(A, 1), B)
    check(agents, pose, Np, 4.0, self_row)
    check(agents, pose, Np, 4.0)


def test_ties_go_to_the_lower_row_also_across_the_cut():
    four = table([[0.0, 1.0], [1.0, 0.0], [0.0, -1.0], [-1.0, 0.0]])
    pose = np.zeros((1, 3))
    for Np in (1, 2, 3, 4, 5):
        _, count, source = check(four, pose, Np, 2.0)
        assert source[0, :count[0]].tolist() == [0, 1, 2, 3][:Np]
    dup = table([[2.0, 2.0]] * 5 + [[0.5, 0.0]] + [[2.0, 2.0]] * 2)
    dup[:, 4] = np.arange(8)                                              # same point, different rows: told apart by vz
    people, count, source = check(dup, pose, 4, 5.0)
    assert source[0].tolist() == [5, 0, 1, 2] and people[0, :, 4].tolist() == [5.0, 0.0, 1.0, 2.0]
    # a tie that straddles the cut: rows 1, 3, 4 at one distance, Np takes two of them
    cut = table([[3.0, 0.0], [0.0, 2.0], [0.1, 0.0], [2.0, 0.0], [0.0, -2.0]])
    _, count, source = check(cut, pose, 3, 5.0)
    assert source[0].tolist() == [2, 1, 3]


def test_the_range_gate_on_a_3_4_5_triangle():
    pose = np.array([[1.0, 2.0, 0.0]])
    agents = table([[4.0, 6.0]])
    assert R.nearest_people(agents, pose, 2, 5.0)[1].tolist() == [1]
    assert R.nearest_people(agents, pose, 2, np.nextafter(5.0, 0.0))[1].tolist() == [0]
    agents = table([[4.0, np.nextafter(6.0, UP)]])
    assert R.nearest_people(agents, pose, 2, 5.0)[1].tolist() == [0]
    check(agents, pose, 2, 5.0)


def test_self_in_three_forms():
    # robots 0 and 1 on one spot, rows 2 and 3 of the table; row 0 is a pedestrian right under them
    agents = table([[1.0, 1.0], [2.0, 1.0], [1.0, 1.0], [1.0, 1.0]])
    pose = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.5]])
    _, count, source = check(agents, pose, 4, 3.0)                        # no self: everybody, d2 = 0 first by row
    assert source.tolist() == [[0, 2, 3, 1], [0, 2, 3, 1]]
    _, count, source = check(agents, pose, 4, 3.0, np.array([-1, -7]))     # < 0: nobody is skipped
    assert source.tolist() == [[0, 2, 3, 1], [0, 2, 3, 1]]
    _, count, source = check(agents, pose, 4, 3.0, np.array([2, 3]))       # each skips itself and sees the other at d2 = 0
    assert source.tolist() == [[0, 3, 1, -1], [0, 2, 1, -1]] and count.tolist() == [3, 3]


def test_non_finite_agents_and_robots():
    agents = table([[np.nan, 0.0], [0.0, np.inf], [1e300, 0.0], [0.5, 0.0], [-np.inf, np.nan], [0.0, -1e300]])
    pose = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1e300, 0.0, 0.0]])
    people, count, source = check(agents, pose, 3, 10.0)
    assert count.tolist() == [1, 0, 0, 1] and source[0, 0] == 3 and source[3, 0] == 2
    assert np.isnan(people[1]).all() and np.isnan(people[2]).all()


# ---- the __host__ __device__ rule, compiled for the host -----------------------------------------------------------------
# queries, one per line: "b p origin bin_size n" -> the bin; "g rx ry ax ay range" -> "<qualifies 0/1> <bits of d2, hex>";
# "k d2a ca d2b cb" -> key (d2a, ca) < key (d2b, cb), 0/1
PROBE = r"""
#include <cinttypes>
#include <cstdio>
#include "smpc_nearest_rule.hpp"
int main() {
  static char line[4096];
  while (std::fgets(line, sizeof line, stdin)) {
    double a, b, c, d, e;
    int n;
    unsigned u, v;
    if (std::sscanf(line, "b %la %la %la %d", &a, &b, &c, &n) == 4) {
      std::printf("%d\n", (int)smpc::nn_bin_axis(a, b, c, n));
    } else if (std::sscanf(line, "g %la %la %la %la %la", &a, &b, &c, &d, &e) == 5) {
      const double d2 = smpc::nn_d2(a, b, c, d);
      const bool ok = smpc::nn_finite(a) && smpc::nn_finite(b) && smpc::nn_finite(c) && smpc::nn_finite(d) && smpc::nn_in_range(d2, e);
      std::printf("%d %016" PRIx64 "\n", ok ? 1 : 0, smpc::nn_key(d2, 0u).d);
    } else if (std::sscanf(line, "k %la %u %la %u", &a, &u, &b, &v) == 4) {
      const smpc::NnKey x = smpc::nn_key(a, u), y = smpc::nn_key(b, v);
      std::printf("%d\n", smpc::nn_key_less(x.d, x.c, y.d, y.c) ? 1 : 0);
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
    tmp = tmp_path_factory.mktemp("nearest_rule")
    src, exe = tmp / "probe.hip", tmp / "probe"
    src.write_text(PROBE)
    # -O3 as build.sh compiles the library: a fused multiply-add, if the compiler made one, would show here
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])

    def ask(lines):
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out

    return ask


def hx(v):
    return float(v).hex()


def test_compiled_bin_function_is_numpys_on_edges_ulps_far_points_and_non_finite_ones(rule):
    g = np.random.default_rng(71)
    lines, want = [], []
    for origin, size, n in ((-3.2, 0.7, 40), (1.15, 10.0 * R.MARGIN, 7), (0.1, 1.0 / 3.0, 65536), (-1e3, 5.0, 1)):
        k = np.concatenate([g.integers(-3, n + 3, 300), [0, 1, n - 1, n]])
        edges = origin + k * size                                            # on bin edges (up to rounding) ...
        pts = np.concatenate([edges, np.nextafter(edges, UP), np.nextafter(edges, DOWN),  # ... and one ulp to either side
                              origin + g.uniform(-2.0, n + 2.0, 400) * size,
                              [1e12, -1e12, 1e300, -1e300, np.nan, np.inf, -np.inf, origin, -0.0, 0.0]])
        lines += [f"b {hx(p)} {hx(origin)} {hx(size)} {n}" for p in pts]
        bins = R.bin_axis(pts, origin, size, n)
        assert bins.min() == 0 and bins.max() == n - 1
        assert (np.diff(R.bin_axis(np.sort(pts[np.isfinite(pts)]), origin, size, n)) >= 0).all()   # monotone in p
        want += bins.tolist()
    assert len(lines) > 4000 and [int(v) for v in rule(lines)] == want


def test_compiled_gate_and_key_order_are_numpys(rule):
    g = np.random.default_rng(72)
    n = 1500
    r = np.round(g.uniform(-5.0, 5.0, (n, 2)), 1)
    a = np.round(r + g.uniform(-3.0, 3.0, (n, 2)), 1)
    special = [np.nan, np.inf, -np.inf, 1e300, -1e300, 1e12]
    a[:40, 0] = g.choice(special, 40)
    r[40:80, 1] = g.choice(special, 40)
    rng = 2.5
    extra = [(1.0, 2.0, 4.0, 6.0, 5.0), (1.0, 2.0, 4.0, 6.0, np.nextafter(5.0, 0.0)), (1.0, 2.0, 4.0, np.nextafter(6.0, UP), 5.0),
             (0.0, 0.0, 0.0, 0.0, 1e-300), (1e300, 0.0, 1e300, 0.0, 1.0)]
    cases = [(r[i, 0], r[i, 1], a[i, 0], a[i, 1], rng) for i in range(n)] + extra
    got = [l.split() for l in rule(["g " + " ".join(hx(v) for v in c) for c in cases])]
    passed = 0
    for (rx, ry, ax, ay, m), (ok, bits) in zip(cases, got):
        w_ok, w_d2 = R.qualifying(table([[ax, ay]]), np.array([[rx, ry, 0.0]]), m)
        assert int(ok) == int(w_ok[0, 0]) and int(bits, 16) == int(np.float64(w_d2[0, 0]).view(np.uint64)), (rx, ry, ax, ay, m)
        passed += int(ok)
    assert 300 < passed < 1300
    assert [l[0] for l in got[-5:]] == ["1", "0", "0", "1", "1"]
    # the key order: the bits of a d2 >= +0 order as the doubles do, then the row
    d = np.concatenate([[0.0, 5e-324, 1e-300, 1.0, np.nextafter(1.0, UP), 25.0, 1e300], np.round(g.uniform(0.0, 3.0, 40), 1)])
    i, j = g.integers(0, len(d), 600), g.integers(0, len(d), 600)
    ci, cj = g.integers(0, 2 ** 24, 600), g.integers(0, 2 ** 24, 600)
    cj[:100] = ci[:100]
    j[:200] = i[:200]
    got = rule([f"k {hx(d[x])} {u} {hx(d[y])} {v}" for x, u, y, v in zip(i, ci, j, cj)])
    assert [int(v) for v in got] == [int((d[x], u) < (d[y], v)) for x, u, y, v in zip(i, ci, j, cj)]


# ---- the 3 x 3 property, under attack ---------------------------------------------------------------------------------------
def gate(rx, ry, ax, ay, max_range):
    with np.errstate(over="ignore"):
        ddx, ddy = ax - rx, ay - ry
        xx, yy = ddx * ddx, ddy * ddy
        return (xx + yy) <= np.float64(max_range) * np.float64(max_range)


def test_every_pair_that_passes_the_gate_sits_within_one_bin_per_axis(rule):
    g = np.random.default_rng(73)
    total = beside = 0
    lines, want = [], []
    for max_range in (10.0, 5.0, 0.3, 1.0 / 3.0, 2.0 ** -3, 123.456):
        size = float(np.float64(max_range) * np.float64(R.MARGIN))             # exactly the least bin_size the call takes
        for origin in (0.0, 0.1, -3.3, 1e-3, 7.7 / 3.0, -1e4 / 7.0):           # most are not representable sums with k * size
            n = 65536
            k = np.concatenate([[0, 1, 2, 3, 100, 4097, 65533, 65534, 65535, 65536], g.integers(0, 65536, 30)]).astype(np.float64)
            edge = origin + k * size
            ulps = [edge]
            for _ in range(3):
                ulps = [np.nextafter(ulps[0], DOWN)] + ulps + [np.nextafter(ulps[-1], UP)]
            at = np.concatenate(ulps + [edge + g.uniform(-1.0, 1.0, len(edge)) * size])   # robots on, beside and near the edges
            for sign in (-1.0, 1.0):
                for f in (1.0, 0.6, 0.8, 0.5 ** 0.5, 0.999999):                 # along the axis, 3-4-5 corners, the diagonal
                    reach = sign * f * max_range
                    far = at + reach
                    other = np.sqrt(max(1.0 - f * f, 0.0)) * max_range
                    for ax in (far, np.nextafter(far, UP), np.nextafter(far, DOWN), np.nextafter(np.nextafter(far, UP), UP)):
                        for oy in (other, np.nextafter(other, UP), np.nextafter(other, DOWN)):
                            ok = gate(at, 0.0, ax, oy, max_range)
                            br, ba = R.bin_axis(at, origin, size, n), R.bin_axis(ax, origin, size, n)
                            assert (np.abs(br - ba)[ok] <= 1).all(), (max_range, origin, sign, f)
                            total += int(ok.sum())
                            beside += int((np.abs(br - ba)[ok] == 1).sum())
                            if f == 1.0 and oy == other and len(lines) < 6000:   # the compiled function on the same points
                                lines += [f"b {hx(p)} {hx(origin)} {hx(size)} {n}" for p in np.concatenate([at[:40], ax[:40]])]
                                want += np.concatenate([br[:40], ba[:40]]).tolist()
    assert total > 100000 and beside > 20000          # the attack lands: many pairs in range, many of them one bin apart
    assert [int(v) for v in rule(lines)] == want
    # random pairs on a small grid, far outside it and on its last bins, with a larger bin too
    for size, n, origin in ((5.0 * R.MARGIN, 7, -3.0), (7.5, 3, 2.0), (5.0 * R.MARGIN, 1, 0.0), (5.0 * R.MARGIN, 65536, -11.0)):
        rx = np.concatenate([g.uniform(-30.0, 70.0, 20000), g.uniform(-1.0, 1.0, 2000) * 1e12,
                             origin + size * (n - g.uniform(0.0, 3.0, 2000))])
        ax = rx + g.uniform(-5.5, 5.5, len(rx))
        ok = gate(rx, 0.0, ax, 0.0, 5.0)
        assert ok.sum() > 15000 and (np.abs(R.bin_axis(rx, origin, size, n) - R.bin_axis(ax, origin, size, n))[ok] <= 1).all()


def test_a_bin_below_the_margin_would_break_the_property():
    """The attack is one: with bin_size == max_range (what the margin forbids) a pair in range sits two bins apart."""
    max_range, origin, n = 0.3, 0.1, 65536
    edge = origin + np.arange(0, 4000, dtype=np.float64) * max_range
    rx = np.nextafter(edge, DOWN)
    ax = rx + max_range
    ok = gate(rx, 0.0, ax, 0.0, max_range)
    apart = np.abs(R.bin_axis(rx, origin, max_range, n) - R.bin_axis(ax, origin, max_range, n))
    assert ok.any() and apart[ok].max() == 2


# ---- the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mirror_matches_the_header_and_the_library_exports_the_functions(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src))) == sorted(NA.FUNCTIONS) == ["smpc_nearest_people_batch",
                                                                                                "smpc_nearest_workspace_bytes"]
    assert re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S) == [st.c_name for st in NA.STRUCTS]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' + "".join(f'printf("%zu\\n", offsetof({st.c_name}, {f[0]}));\n' for f in st._fields_)
                   for st in NA.STRUCTS)
    body += 'printf("%a\\n%d\\n%d\\n", (double)SMPC_NEAREST_BIN_MARGIN, (int)SMPC_NEAREST_MAX_BINS, (int)SMPC_NEAREST_MAX_ROWS);\n'
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc_nearest.h"\nint main(void){\n' + body + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = subprocess.check_output([str(exe)], text=True).split()
    want = [v for st in NA.STRUCTS for v in [C.sizeof(st)] + [getattr(st, f[0]).offset for f in st._fields_]]
    assert [int(v) for v in values[:-3]] == want and C.sizeof(NA.SmpcNearestIn) == 96
    assert float.fromhex(values[-3]) == NA.SMPC_NEAREST_BIN_MARGIN == R.MARGIN == 1.0 + 2.0 ** -20
    assert [int(v) for v in values[-2:]] == [NA.SMPC_NEAREST_MAX_BINS, NA.SMPC_NEAREST_MAX_ROWS] == [65536, 2 ** 24]
    exported = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    lib = S.load_library()
    for name, (restype, argtypes) in NA.FUNCTIONS.items():
        assert f" {name}\n" in exported
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes


def test_the_main_abi_is_as_it_was():
    from nav2_social_mpc_controller_amd import _abi
    assert _abi.SMPC_ABI_VERSION == 6 and len(_abi.FUNCTIONS) == 27 and not set(NA.FUNCTIONS) & set(_abi.FUNCTIONS)
    assert re.search(r"#define\s+SMPC_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "smpc.h")).read())


# ---- the parameters, the pool and the episode's arguments -----------------------------------------------------------------
def test_shared_world_params_defaults_checks_and_grid():
    sp = SharedWorldParams()
    assert (sp.max_range, sp.max_people, sp.robots_as_people) == (10.0, None, True)
    for bad in (dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=np.inf), dict(max_range=np.nan), dict(max_people=0),
                dict(max_people=65)):
        with pytest.raises(ValueError):
            SharedWorldParams(**bad)
    flat = lambda cx, cy, res, origin=(0.0, 0.0): World(np.zeros((cy, cx), np.uint8), np.asarray(origin, np.float64), res)
    gx, gy, origin, size = sp.grid(flat(256, 192, 0.05, (-1.5, 2.0)))        # 12.8 m x 9.6 m: the range decides
    assert (gx, gy, size) == (2, 1, 10.0 * (1.0 + 2.0 ** -20)) and origin.tolist() == [-1.5, 2.0]
    gx, gy, origin, size = SharedWorldParams(max_range=2.0).grid(flat(400, 120, 0.05))   # 20 m x 6 m
    assert size == 2.0 * (1.0 + 2.0 ** -20) and (gx, gy) == (10, 3) and gx * size >= 20.0 > (gx - 1) * size
    gx, gy, origin, size = SharedWorldParams(max_range=1.0).grid(flat(4000, 1000, 0.25))  # 1000 m x 250 m: the 65536-bin cap decides
    assert size == 1000.0 / 256.0 and (gx, gy) == (256, 64) and gx * gy <= 65536
    gx, gy, origin, size = SharedWorldParams(max_range=0.01).grid(flat(3001, 3001, 1.0))
    assert (gx, gy) == (256, 256) and size == 3001.0 / 256.0 and size >= 0.01 * (1.0 + 2.0 ** -20)
    st = S.BatchSolver.nearest_c(5, 3, 11, 4, 2, [0.5, -2.0], 7.75, 7.5, 1)
    assert (st.B, st.Np, st.A, st.on_device, st.grid_x, st.grid_y) == (5, 3, 11, 1, 4, 2)
    assert (list(st.grid_origin), st.bin_size, st.max_range) == ([0.5, -2.0], 7.75, 7.5)


def test_shared_pool_is_seeded_and_lands_on_free_cells():
    world = make_world(200, 160, 0.05, origin=(-2.0, 1.0))
    pool = shared_pool(world, 300)
    assert pool.shape == (300, 5) and pool.dtype == np.float64 and np.isfinite(pool).all()
    ci = np.floor((pool[:, 0] - world.origin[0]) / world.resolution).astype(int)
    cj = np.floor((pool[:, 1] - world.origin[1]) / world.resolution).astype(int)
    assert (world.map[cj, ci] == 0).all()
    speed = np.hypot(pool[:, 2], pool[:, 3])
    standing = speed == 0.0
    assert 0.1 < standing.mean() < 0.3 and (speed[~standing] >= 0.2 - 1e-12).all() and (speed[~standing] < 1.2 + 1e-12).all()
    assert (pool[:, 4] == 0.0).all()
    assert R.same_bits(pool, shared_pool(world, 300)) and R.same_bits(pool[:100], shared_pool(world, 100))
    assert not R.same_bits(pool, shared_pool(world, 300, seed=5))
    assert (np.hypot(*shared_pool(world, 50, standing_fraction=1.0)[:, 2:4].T) == 0.0).all()
    assert shared_pool(world, 0).shape == (0, 5)


def test_the_episode_declares_the_arguments_and_sharded_episodes_refuse_them():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode, TickRecord
    sig = inspect.signature(BatchEpisode.__init__).parameters
    for name in ("shared", "pool"):
        assert name in BatchEpisode.FORWARDED and sig[name].default is None
    assert {"agents", "person_source", "agents_after"} <= set(TickRecord.__dataclass_fields__)
    for kw in (dict(shared=SharedWorldParams()), dict(pool=np.zeros((3, 5)))):
        with pytest.raises(ValueError, match="independent"):
            ShardedEpisode(None, None, None, None, None, None, **kw)
