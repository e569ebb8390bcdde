"""Global plans on the CPU: the yardstick itself (tests/global_plan_ref.py) against a brute-force Bellman-Ford and on
hand-made worlds, the `__host__ __device__` rule of csrc/smpc_global_plan_rule.hpp compiled into a host-only program against
numpy and the reference, the ctypes mirror against include/smpc_global_plan.h, scenes.world_goals, and the bound that keeps
32-bit potentials from overflowing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import global_plan_ref as R
from nav2_social_mpc_controller_amd import _abi_global_plan as GA
from nav2_social_mpc_controller_amd import solver as S
from nav2_social_mpc_controller_amd.params import GlobalPlanParams
from nav2_social_mpc_controller_amd.scenes import make_world, world_goals
from test_kernel_budget import CSRC, HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc_global_plan.h")
U = R.UNREACHABLE


# ---- the reference against brute force -----------------------------------------------------------------------------------
def bellman_ford(world, goal_cell, cost):
    """field [Hy,Hx] by relaxing every cell from every neighbour until nothing changes: the contract's definition, slowly."""
    w = R.weights(world, cost)
    Hy, Hx = world.shape
    f = np.full((Hy, Hx), U, np.uint64)
    f[goal_cell[1], goal_cell[0]] = 0
    for _ in range(Hx * Hy + 1):
        changed = False
        for y in range(Hy):
            for x in range(Hx):
                if w[y, x] == 0:
                    continue
                for dx, dy in R.NEIGHBOURS:
                    nx, ny = x + dx, y + dy
                    if not (0 <= nx < Hx and 0 <= ny < Hy) or w[ny, nx] == 0 or f[ny, nx] == U:
                        continue
                    if dx and dy and (w[y, nx] == 0 or w[ny, x] == 0):
                        continue
                    cand = int(f[ny, nx]) + (5 if dx == 0 or dy == 0 else 7) * int(w[ny, nx])
                    if cand < f[y, x]:
                        f[y, x], changed = cand, True
        if not changed:
            return f.astype(np.uint32)
    raise AssertionError("Bellman-Ford did not settle")


@pytest.mark.parametrize("Hx,Hy,seed", [(12, 9, 1), (9, 12, 2), (7, 5, 3), (1, 9, 4), (12, 1, 5), (1, 1, 6)])
def test_reference_field_is_the_bellman_ford_fixed_point(Hx, Hy, seed):
    g = np.random.default_rng(seed)
    for cost in (R.Cost(), R.Cost(1, 0), R.Cost(7, 3, 200, True)):
        world = g.choice(np.array([0, 0, 0, 30, 120, 252, 253, 254, 255], np.uint8), (Hy, Hx))
        free = np.argwhere(R.passable(world, cost))
        if len(free) == 0:
            world[0, 0] = 0
            free = np.array([[0, 0]])
        gy, gx = free[g.integers(len(free))]
        origin, res = np.array([-0.3, 1.7]), 0.25
        field, status = R.goal_field(world, origin, res, R.centre_of((gx, gy), origin, res), cost)
        assert status == 0 and field.dtype == np.uint32
        assert np.array_equal(field, bellman_ford(world, (gx, gy), cost))
        assert (field[~R.passable(world, cost)] == U).all() and field[gy, gx] == 0


# ---- hand-made cases -----------------------------------------------------------------------------------------------------
ORIGIN, RES = np.array([0.0, 0.0]), 1.0


def centre(x, y):
    return np.array([x + 0.5, y + 0.5])


def test_a_diagonal_gap_between_two_lethal_cells_is_not_passed():
    world = np.zeros((3, 3), np.uint8)
    world[0, 1] = world[1, 0] = 254          # (1,0) and (0,1) lethal: the corner cell (0,0) touches the rest only diagonally
    field, status = R.goal_field(world, ORIGIN, RES, centre(2, 2))
    assert status == 0 and field[0, 0] == U and field[1, 1] == 7 * 50 and field[2, 2] == 0
    world[0, 1] = 0                          # one of the two opens: still no diagonal, but an axis way round
    field, _ = R.goal_field(world, ORIGIN, RES, centre(2, 2))
    assert field[0, 0] == 5 * 50 + field[0, 1] and field[0, 1] == 5 * 50 + field[1, 1]
    # one lethal edge-sharing cell is enough to forbid the diagonal
    world = np.zeros((2, 2), np.uint8)
    world[0, 1] = 254
    field, _ = R.goal_field(world, ORIGIN, RES, centre(1, 1))
    assert field[0, 0] == 10 * 50            # two axis steps, not one diagonal of 7 * 50


def test_the_walk_takes_the_first_neighbour_in_the_contract_order():
    # uniform floor, goal two columns right and one row up: (1,0) then (1,1), and (1,1) then (1,0), cost the same;
    # neighbour 0 = (1,0) comes first
    world = np.zeros((3, 4), np.uint8)
    field, _ = R.goal_field(world, ORIGIN, RES, centre(3, 1))
    cells, err = R.walk(world, field, (1, 0))
    assert err == 0 and cells == [(1, 0), (2, 0), (3, 1)]
    # goal straight up-left: the diagonal (-1,1) is neighbour 5, nothing before it satisfies the equality
    field, _ = R.goal_field(world, ORIGIN, RES, centre(0, 2))
    assert R.walk(world, field, (2, 0))[0] == [(2, 0), (1, 1), (0, 2)]
    # (0,1) is neighbour 1 and comes before (-1,0), neighbour 2
    field, _ = R.goal_field(world, ORIGIN, RES, centre(0, 2))
    assert R.walk(world, field, (1, 1))[0] == [(1, 1), (0, 2)]
    # from (2,1) both (-1,0) then (-1,1) and (-1,1) then (-1,0) cost 5 * 50 + 7 * 50: neighbour 2 = (-1,0) is earlier than 5
    assert field[1, 2] == 5 * 50 + 7 * 50 and field[1, 1] == 7 * 50 and field[2, 1] == 5 * 50
    assert R.walk(world, field, (2, 1))[0] == [(2, 1), (1, 1), (0, 2)]
    fits = [k for k, nx, ny, c in R.steps_from(R.weights(world, R.Cost()), 2, 1) if int(field[ny, nx]) + c == int(field[1, 2])]
    assert fits == [2, 5]


def test_unknown_cells_with_and_without_allow_unknown():
    world = np.array([[0, 255, 0]], np.uint8)
    field, status = R.goal_field(world, ORIGIN, RES, centre(2, 0))
    assert status == 0 and list(field[0]) == [U, U, 0]
    cost = R.Cost(allow_unknown=True)
    field, status = R.goal_field(world, ORIGIN, RES, centre(2, 0), cost)
    assert list(field[0]) == [5 * 50 + 5 * (50 + 255), 5 * 50, 0]
    assert R.goal_field(world, ORIGIN, RES, centre(1, 0))[1] == 2 and R.goal_field(world, ORIGIN, RES, centre(1, 0), cost)[1] == 0
    assert R.goal_field(world, ORIGIN, RES, [3.0, 0.5])[1] == 1 and R.goal_field(world, ORIGIN, RES, [np.nan, 0.5])[1] == 1
    # 253 and 254 stay impassable with allow_unknown
    assert not R.passable(np.array([[253, 254]], np.uint8), cost).any() and R.passable(np.array([[252, 255]], np.uint8), cost).all()


def test_a_walled_in_pocket_is_unreachable_and_so_is_a_start_in_it():
    world = np.zeros((7, 7), np.uint8)
    world[2:5, 2:5] = 254
    world[3, 3] = 0                                           # the pocket
    field, status = R.goal_field(world, ORIGIN, RES, centre(0, 0))
    assert status == 0 and field[3, 3] == U and (field[world == 0].ravel() != U).sum() == (world == 0).sum() - 1
    pose = np.array([[3.5, 3.5, 0.0], [6.5, 6.5, 0.0], [2.5, 2.5, 0.0], [-1.0, 0.0, 0.0], [1.5, 1.5, 0.0]])
    plan, n, err = R.extract_plan(world, ORIGIN, RES, field[None], [centre(0, 0)], [0, 0, 0, 0, 3], pose, 16)
    assert list(err) == [R.UNREACHABLE_START, R.OK, R.START_BLOCKED, R.START_OUTSIDE, R.BAD_GOAL_INDEX]
    assert list(n) == [0, n[1], 0, 0, 0] and n[1] > 2 and np.isnan(plan[[0, 2, 3, 4]]).all() and np.isnan(plan[1, n[1]:]).all()
    # from inside the pocket the pocket is a world of its own
    inner, _ = R.goal_field(world, ORIGIN, RES, centre(3, 3))
    assert inner[3, 3] == 0 and (inner.ravel() == U).sum() == 48


def test_plan_rows_stride_and_truncation():
    world = np.zeros((1, 12), np.uint8)
    goal = np.array([11.25, 0.75])
    field, _ = R.goal_field(world, ORIGIN, RES, goal)
    pose = np.array([[0.25, 0.5, 0.0]])
    plan, n, err = R.extract_plan(world, ORIGIN, RES, field[None], [goal], [0], pose, 16)      # 11 steps: pose, c1..c10, goal
    assert n[0] == 12 and err[0] == 0 and np.array_equal(plan[0, 0], [0.25, 0.5]) and np.array_equal(plan[0, 11], goal)
    assert np.array_equal(plan[0, 1:11, 0], np.arange(1, 11) + 0.5)
    plan, n, err = R.extract_plan(world, ORIGIN, RES, field[None], [goal], [0], pose, 16, stride=5)   # j * 5 < 11: c5, c10
    assert n[0] == 4 and np.array_equal(plan[0, :4, 0], [0.25, 5.5, 10.5, 11.25])
    plan, n, err = R.extract_plan(world, ORIGIN, RES, field[None], [goal], [0], pose, 16, stride=11)  # 11 < 11 fails: no centre
    assert n[0] == 2 and err[0] == 0
    for L, want in ((12, R.OK), (11, R.TRUNCATED), (2, R.TRUNCATED)):
        plan, n, err = R.extract_plan(world, ORIGIN, RES, field[None], [goal], [0], pose, L)
        assert err[0] == want and n[0] == L and np.array_equal(plan[0, :L - 1, 0], np.r_[0.25, np.arange(1, L - 1) + 0.5])
    same = np.array([[11.5, 0.5, 0.0]])                                                             # start cell = goal cell
    plan, n, err = R.extract_plan(world, ORIGIN, RES, field[None], [goal], [0], same, 2)
    assert n[0] == 2 and err[0] == 0 and np.array_equal(plan[0], [[11.5, 0.5], goal])
    raised = field.copy()
    raised[0, 5] += 1                                                                               # no neighbour of c4 fits any more
    assert R.extract_plan(world, ORIGIN, RES, raised[None], [goal], [0], pose, 16)[2][0] == R.INCONSISTENT_FIELD


# ---- the __host__ __device__ rule, compiled for the host -----------------------------------------------------------------
# queries, one per line: "c px py ox oy res sx sy" -> "has cx cy", "m ix iy ox oy res" -> centre x y (hex floats),
# "w v neutral weight lethal unknown" -> weight, "s k wn wa wb" -> "dx dy cost"
PROBE = r"""
#include <cstdio>
#include "smpc_global_plan_rule.hpp"
int main() {
  char line[512];
  while (std::fgets(line, sizeof line, stdin)) {
    double a, b, c, d, e;
    int i, j, k, l, m;
    if (std::sscanf(line, "c %la %la %la %la %la %d %d", &a, &b, &c, &d, &e, &i, &j) == 7) {
      int cx = -1, cy = -1;
      const bool hx = smpc::gp_cell_axis(a, c, e, i, &cx), hy = smpc::gp_cell_axis(b, d, e, j, &cy);
      std::printf("%d %d %d\n", hx && hy ? 1 : 0, hx ? cx : -1, hy ? cy : -1);
    } else if (std::sscanf(line, "m %d %d %la %la %la", &i, &j, &a, &b, &c) == 5) {
      std::printf("%a %a\n", smpc::gp_centre(a, i, c), smpc::gp_centre(b, j, c));
    } else if (std::sscanf(line, "w %d %d %d %d %d", &i, &j, &k, &l, &m) == 5) {
      const smpc::GpCost cost{j, k, (uint32_t)l, (uint32_t)m};
      std::printf("%u\n", smpc::gp_weight(cost, (uint32_t)i));
    } else if (std::sscanf(line, "s %d %d %d %d", &i, &j, &k, &l) == 4) {
      std::printf("%d %d %u\n", smpc::gp_dx(i), smpc::gp_dy(i), smpc::gp_step_cost(i, (uint32_t)j, (uint32_t)k, (uint32_t)l));
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
    tmp = tmp_path_factory.mktemp("global_plan_rule")
    src, exe = tmp / "probe.hip", tmp / "probe"
    src.write_text(PROBE)
    # -O3 as build.sh compiles the library: a fused multiply-add, if the compiler made one, would show here
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])

    def ask(lines):
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [l.split() for l in out]

    return ask


def hx(v):
    return float(v).hex()


def test_compiled_cells_and_centres_agree_with_numpy_bit_for_bit(rule):
    g = np.random.default_rng(41)
    origin, res, sx, sy = np.array([-3.2, 1.15]), 0.05, 256, 192
    edges = origin + g.integers(-3, 260, (400, 2)) * res                       # on cell edges (up to rounding) ...
    beside = np.concatenate([np.nextafter(edges, np.inf), np.nextafter(edges, -np.inf)])   # ... and one ulp to either side
    special = np.array([[1e12, 2.0], [-1e12, 2.0], [0.0, 1e12], [0.0, -1e12], [np.nan, 2.0], [0.0, np.nan], [np.inf, 2.0], [0.0, -np.inf],
                        [np.nan, np.inf], [1e300, -1e300], origin, origin + np.array([sx, sy]) * res, [-0.0, 1.15]])
    pts = np.concatenate([edges, beside, g.uniform(-4.0, 12.0, (1500, 2)), special])
    got = rule([f"c {hx(p[0])} {hx(p[1])} {hx(origin[0])} {hx(origin[1])} {hx(res)} {sx} {sy}" for p in pts])
    want = [R.cell_of(p, origin, res, sx, sy) for p in pts]
    with np.errstate(invalid="ignore"):
        q = np.floor((pts - origin) / res)
    for p, row, w, qq in zip(pts, got, want, q):
        has, cx, cy = (int(v) for v in row)
        assert (has == 1) == (w is not None), p
        if w is not None:
            assert (cx, cy) == w, p
        # per axis the compiled rule is numpy's floor of numpy's quotient
        assert cx == (int(qq[0]) if 0 <= qq[0] < sx else -1) and cy == (int(qq[1]) if 0 <= qq[1] < sy else -1), p
    assert sum(w is None for w in want) > 100 and sum(w is not None for w in want) > 1500
    assert all(w is None for w in want[-len(special):-3]) and want[-3] == (0, 0) and want[-2] is None
    cells = np.concatenate([g.integers(0, 2 ** 31 - 1, (300, 2)), [[0, 0], [255, 191], [2 ** 31 - 1, 2 ** 31 - 1]]]).astype(np.int32)
    for o, r in ((origin, res), (np.array([1e6 + 0.1, -7e5 - 0.3]), 0.1), (np.array([0.0, 0.0]), 1.0 / 3.0)):
        got = rule([f"m {c[0]} {c[1]} {hx(o[0])} {hx(o[1])} {hx(r)}" for c in cells])
        have = np.array([[float.fromhex(v) for v in row] for row in got])
        assert R.same_bits(have, np.array([R.centre_of(c, o, r) for c in cells]))


def test_compiled_weights_neighbours_and_step_costs_are_the_references(rule):
    for cost in (R.Cost(), R.Cost(1, 0), R.Cost(7, 3, 200, True), R.Cost(280, 256, 255, False), R.Cost(50, 1, 0, True)):
        got = rule([f"w {v} {cost.neutral_cost} {cost.cost_weight} {cost.lethal_min_cost} {int(cost.allow_unknown)}" for v in range(256)])
        assert [int(r[0]) for r in got] == list(R.weights(np.arange(256, dtype=np.uint8)[None], cost)[0])
    lines, want = [], []
    for k, (dx, dy) in enumerate(R.NEIGHBOURS):
        for wn, wa, wb in ((50, 60, 70), (0, 60, 70), (50, 0, 70), (50, 60, 0), (65535, 1, 1), (50, 0, 0)):
            lines.append(f"s {k} {wn} {wa} {wb}")
            ok = wn != 0 and (k < 4 or (wa != 0 and wb != 0))
            want.append([dx, dy, (5 if k < 4 else 7) * wn if ok else 0])
    assert [[int(v) for v in r] for r in rule(lines)] == want


# ---- the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mirror_matches_the_header_and_the_library_exports_the_functions(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src))) == sorted(GA.FUNCTIONS)
    assert re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S) == [st.c_name for st in GA.STRUCTS]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' + "".join(f'printf("%zu\\n", offsetof({st.c_name}, {f[0]}));\n' for f in st._fields_)
                   for st in GA.STRUCTS)
    body += "".join(f'printf("%d\\n", (int)SMPC_PLAN_{name});\n' for name in GA.PLAN_ERRORS) + 'printf("%u\\n", SMPC_FIELD_UNREACHABLE);\n'
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc_global_plan.h"\nint main(void){\n' + body + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [v for st in GA.STRUCTS for v in [C.sizeof(st)] + [getattr(st, f[0]).offset for f in st._fields_]]
    assert values == want + list(range(len(GA.PLAN_ERRORS))) + [GA.SMPC_FIELD_UNREACHABLE]
    assert [C.sizeof(st) for st in GA.STRUCTS] == [16, 72, 104]
    assert [R.OK, R.START_OUTSIDE, R.START_BLOCKED, R.UNREACHABLE_START, R.TRUNCATED, R.BAD_GOAL_INDEX, R.INCONSISTENT_FIELD] == list(range(7))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    lib = S.load_library()
    for name, (restype, argtypes) in GA.FUNCTIONS.items():
        assert f" {name}\n" in exported
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes


def test_the_main_abi_is_as_it_was():
    from nav2_social_mpc_controller_amd import _abi
    assert _abi.SMPC_ABI_VERSION == 6 and len(_abi.FUNCTIONS) == 27 and not set(GA.FUNCTIONS) & set(_abi.FUNCTIONS)


# ---- the generator -------------------------------------------------------------------------------------------------------
def test_world_goals_are_seeded_free_far_from_the_start_and_inside_the_margin():
    w = make_world(256, 192, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15))
    g = np.random.default_rng(51)
    start = w.origin + g.uniform(1.0, 8.0, (64, 2))
    goal = world_goals(w, start)
    assert goal.shape == (64, 2) and goal.dtype == np.float64 and R.same_bits(goal, world_goals(w, start))
    assert not np.array_equal(goal, world_goals(w, start, seed=7))
    assert R.same_bits(world_goals(w, start[:10]), goal[:10])                       # a robot's goal is keyed by its index alone
    ci = np.floor((goal - w.origin) / w.resolution).astype(int)
    assert (w.map[ci[:, 1], ci[:, 0]] == 0).all()
    assert (np.hypot(*(goal - start).T) >= 3.0).all()
    rel = goal - w.origin
    assert (rel >= 1.0).all() and (rel[:, 0] <= 256 * 0.05 - 1.0).all() and (rel[:, 1] <= 192 * 0.05 - 1.0).all()
    assert len(np.unique(goal, axis=0)) == 64
    # the first qualifying candidate: with a larger min_dist a robot keeps its goal or moves on to a later one
    far = world_goals(w, start, min_dist=5.0)
    assert (np.hypot(*(far - start).T) >= 5.0).all() and (far == goal).all(axis=1).any() and not (far == goal).all()
    # no candidate qualifies: the centre of the free cell nearest the floor's centre
    none = world_goals(w, start, min_dist=1e3)
    assert (none == none[0]).all()
    cj, ci = np.floor((none[0] - w.origin) / w.resolution).astype(int)[::-1]
    assert w.map[cj, ci] == 0 and R.same_bits(none[0], w.origin + (np.array([ci, cj]) + 0.5) * w.resolution)
    free = np.argwhere(w.map == 0)
    d2 = (free[:, 1] + 0.5 - 128) ** 2 + (free[:, 0] + 0.5 - 96) ** 2
    assert (ci + 0.5 - 128) ** 2 + (cj + 0.5 - 96) ** 2 == d2.min()


def test_global_plan_params_defaults_and_checks():
    gp = GlobalPlanParams()
    assert (gp.neutral_cost, gp.cost_weight, gp.lethal_min_cost, gp.allow_unknown, gp.max_poses, gp.stride) == (50, 1, 253, False, 400, 1)
    for bad in (dict(neutral_cost=0), dict(cost_weight=-1), dict(neutral_cost=1, cost_weight=257), dict(max_poses=1), dict(stride=0),
                dict(lethal_min_cost=256)):
        with pytest.raises(ValueError):
            GlobalPlanParams(**bad)
    st = S.BatchSolver.extract_plan_c(GlobalPlanParams(7, 3, 200, True, 33, 4), 5, 2, 11, 13, False, 0.25, 1)
    assert (st.B, st.G, st.L, st.stride, st.on_device, st.world_x, st.world_y, st.world_shared, st.resolution) == (5, 2, 33, 4, 1, 11, 13, 0, 0.25)
    assert (st.cost.neutral_cost, st.cost.cost_weight, st.cost.lethal_min_cost, st.cost.allow_unknown) == (7, 3, 200, 1)


# ---- the bound that keeps 32-bit potentials exact --------------------------------------------------------------------------
def overflow_refused(cells_x, cells_y, neutral_cost=50, cost_weight=1):
    """smpc_goal_field_batch's SMPC_ERR_UNSUPPORTED as the package computes it (tests/test_gpu_global_plan.py holds the
    library against the same function)."""
    return not GlobalPlanParams(neutral_cost=neutral_cost, cost_weight=cost_weight).world_supported(cells_x, cells_y)


def test_the_overflow_bound_accepts_1024_x_1024_at_the_defaults_and_refuses_just_over_it():
    assert 1024 * 1024 * 7 * 305 == 2238709760 and not overflow_refused(1024, 1024)
    # the largest accepted cell count at the defaults, and the first refused one
    most = (2 ** 32 - 2) // (7 * 305)
    assert most == 2011694 and not overflow_refused(most, 1) and overflow_refused(most + 1, 1)
    assert not overflow_refused(1418, 1418) and overflow_refused(1419, 1419)
    # the longest conceivable path visits every cell once by diagonal steps into the dearest cells: still below the marker
    assert most * 7 * 305 < R.UNREACHABLE
    assert overflow_refused(64, 48, 65535, 0) is False and overflow_refused(9363, 1, 65535, 0) is True
    assert overflow_refused(2 ** 16, 2 ** 15, 1, 0) and not overflow_refused(2 ** 16, 2 ** 13, 1, 0)      # 2^31 cells
