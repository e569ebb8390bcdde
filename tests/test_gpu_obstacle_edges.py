"""The obstacle critic's costmap gather on the device (`-m gpu`), on the inputs of tests/obstacle_edge_cases.py: the three
paths of csrc/smpc_bicubic.hpp (four unaligned dwords without clamps when a whole wave is interior; clamped dwords with
per-tap shifts otherwise; byte by byte on maps narrower than four cells) at map borders, on the smallest and on non-square
maps, far off the map, and in waves whose scenes or steps disagree about the path. tests/test_obstacle_edges.py holds the
checkers and the table to account without a device.

  K1 against the oracle    every case in both row orders at init_params and at a perturbed point, by
                           test_gpu_instantiations.check_k1's bounds; the obstacle rows also on their own, so that a failure
                           names the scene, the step and the cell bands of the step. README-shape cases run with the
                           fixed-shape kernels on and off.
  pad against crop         the obstacle rows of a case against those of its edge-replicated twin (every lane interior: the
                           unclamped path), within JAC_RTOL: the device paths against each other, without the oracle.
  path independence        rows do not depend on the path a wave takes, bit for bit: an interior batch against the same batch
                           with one scene moved off its map, a scene alone against the scene inside its batch.
  solve                    the smooth-map cases at W = 32 and W = 64 by parity_checks.check_solve, check_population over
                           the pool, and initial_cost against the K1 cost at the projected start point. Checked on the CPU
                           first (test_obstacle_edges.test_solve_inputs_...): README weights, the table's seeds: 224 scenes,
                           all well conditioned, 0.97 firm, 0.93 moved by more than 1e-3 when the map is zeroed.
  trace, arguments         solve_trace on a border-crossing case; sizes of 0 are refused, 1 x 1 is served; a NaN start pose
                           fails its scene alone."""
import numpy as np
import pytest

import obstacle_edge_cases as E
from parity_checks import add_counts, check_population, check_solve
from test_gpu_instantiations import EVAL_KEYS, JAC_RTOL, RESULT_KEYS, check_k1, same
from test_obstacle_edges import solve_inputs

pytestmark = pytest.mark.gpu
ALL = list(E.CASES)
PADDED = [n for n in ALL if E.pad_cells(*E.make_case(n)) is not None]
WORST = {}      # path -> worst relative K1 discrepancy of an obstacle row seen in this run (printed, not asserted)


@pytest.fixture(scope="module")
def Solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    return BatchSolver


def rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(a))


def path_of(prm, sc, x):
    """The path the case is there for (a wave decides for itself: `clamped` batches may hold interior waves)."""
    if sc.size_x < 4:
        return "bytes"
    cc = np.floor(E.cell_coordinates(prm, sc, x)).astype(np.int64)
    return "interior" if E.interior(cc[..., 0], cc[..., 1], sc.size_x, sc.size_y).all() else "clamped"


def obstacle_block(prm, sc, ev, row_order):
    """(residuals [B, T], Jacobian [B, T, P]) of the obstacle critic out of a K1 / oracle result"""
    r = np.empty((sc.B, sc.T))
    J = np.empty((sc.B, sc.T, ev["jacobian"].shape[2]))
    for b in range(sc.B):
        rows = E.obstacle_rows(prm, sc.T, bool(sc.has_people[b]) and sc.N > 0)[row_order]
        r[b], J[b] = ev["residuals"][b, rows], ev["jacobian"][b, rows]
    return r, J


def check_obstacle_rows(oracle, s, prm, sc, x, what):
    """the obstacle rows, taken out of the critic-major result, against the oracle's; returns the worst discrepancy"""
    want = obstacle_block(prm, sc, oracle.evaluate(prm, sc, x), 0)
    got = obstacle_block(prm, sc, s.evaluate(sc, x, row_order=1), 1)
    err = np.maximum(rel(want[0], got[0]), rel(want[1], got[1]).max(axis=2))    # [B, T]
    if not err.max() < JAC_RTOL:
        b, i = np.unravel_index(np.argmax(err), err.shape)
        q, r = np.floor(E.cell_coordinates(prm, sc, x)[b, i]).astype(np.int64)
        raise AssertionError(f"obstacle critic {what}: scene {b} step {i}: relative error {err[b, i]:.3e}; row {r} in bands "
                             f"{sorted(E.bands(r, sc.size_y))}, column {q} in bands {sorted(E.bands(q, sc.size_x))}; "
                             f"{int((err >= JAC_RTOL).sum())} rows beyond {JAC_RTOL}")
    return float(err.max())


@pytest.mark.parametrize("name", ALL)
def test_k1_matches_oracle(Solver, oracle, name):
    prm, sc = E.make_case(name)
    s = Solver(prm)
    fixed = s.eval_shape_is_fixed(sc.T, sc.N)
    assert fixed == (E.CASES[name].shape == "readme")
    worst = 0.0
    for on in ((True, False) if fixed else (True,)):
        s.set_fixed_shapes(on)
        assert s.eval_shape_is_fixed(sc.T, sc.N) == (fixed and on)
        for x in (sc.init_params, E.perturbed(sc)):
            e = check_obstacle_rows(oracle, s, prm, sc, x, (name, "fixed shapes" if on else "run-time shapes"))
            check_k1(s, [(prm, np.arange(sc.B))], sc, x)
            path = path_of(prm, sc, x)
            WORST[path] = max(WORST.get(path, 0.0), e)
            worst = max(worst, e)
    print(f"\n[obstacle K1] {name} {sc.size_x} x {sc.size_y} @ {sc.resolution} {path_of(prm, sc, sc.init_params)}: "
          f"worst rel {worst:.2e}")


def test_k1_worst_per_path():
    if not WORST:
        pytest.skip("needs test_k1_matches_oracle in the same run")
    assert set(WORST) == {"bytes", "clamped", "interior"}
    print("\n[obstacle K1] worst relative discrepancy of an obstacle row per path: " +
          " ".join(f"{k}={v:.2e}" for k, v in sorted(WORST.items())))


@pytest.mark.parametrize("name", PADDED)
def test_k1_pad_against_crop(Solver, name):
    prm, sc = E.make_case(name)
    big = E.padded(sc, E.pad_cells(prm, sc))
    s = Solver(prm)
    worst = 0.0
    for x in (sc.init_params, E.perturbed(sc)):
        assert path_of(prm, big, x) == "interior"
        for row_order in (0, 1):
            a = obstacle_block(prm, sc, s.evaluate(sc, x, row_order=row_order), row_order)
            b = obstacle_block(prm, sc, s.evaluate(big, x, row_order=row_order), row_order)
            err = np.maximum(rel(a[0], b[0]), rel(a[1], b[1]).max(axis=2))
            assert err.max() < JAC_RTOL, (name, row_order, float(err.max()), np.unravel_index(np.argmax(err), err.shape))
            worst = max(worst, float(err.max()))
    print(f"\n[obstacle pad/crop] {name}: worst rel {worst:.2e}")


@pytest.mark.parametrize("name", ["edge_in_64x40_xmin", "edge_in_64x40_ymin", "edge_in_64x40_ymax", "edge_in_40x64_ymax"])
def test_rows_do_not_depend_on_the_path(Solver, name):
    """smpc_bicubic.hpp: "the taps and the arithmetic on them are the same, so the result does not depend on which path a
    wave takes". An interior batch (the README shape, with an even and an odd batch, T = 31 and a one-slot shape) against the same batch with
    scene 5 moved 100 cells off its map, which sends its wave down the clamped path: every other scene's rows, cost and
    gradient are the same bits. Likewise a scene evaluated alone (its wave's other slot idle) against the scene inside the
    batch, and the solve of the untouched scenes."""
    prm, sc = E.make_case(name)
    moved = sc.select(np.arange(sc.B))
    moved.costmap_origin = moved.costmap_origin.copy()
    moved.costmap_origin[5] += 100.0 * sc.resolution
    rest = np.setdiff1d(np.arange(sc.B), [5])
    s = Solver(prm)
    fixed = s.eval_shape_is_fixed(sc.T, sc.N)
    for on in ((True, False) if fixed else (True,)):
        s.set_fixed_shapes(on)
        for x in (sc.init_params, E.perturbed(sc)):
            if x is sc.init_params:   # what the table places; the perturbed point lies where it lies
                assert path_of(prm, sc, x) == "interior" and path_of(prm, moved, x) == "clamped"
            for row_order in (0, 1):
                whole = s.evaluate(sc, x, row_order=row_order)
                same(whole, s.evaluate(moved, x, row_order=row_order), EVAL_KEYS, where=rest, what=(name, on, row_order))
                for b in (4, sc.B - 1):
                    alone = s.evaluate(sc.select([b]), x[[b]], row_order=row_order)
                    same(alone, {k: v[[b]] for k, v in whole.items()}, EVAL_KEYS, what=(name, on, row_order, "alone", b))
        same(s.solve(sc), s.solve(moved), RESULT_KEYS, where=rest, what=(name, on, "solve"))


POPULATION = {}


def projected_start(prm, sc):
    CH, bl, nb, P, M, nbnd = prm.dims(sc.T)
    return np.clip(sc.init_params, [prm.v_min, prm.w_min] * nbnd + [-np.inf, -np.inf] * (nb - nbnd),
                   [prm.v_max, prm.w_max] * nbnd + [np.inf, np.inf] * (nb - nbnd))


@pytest.mark.parametrize("W", [32, 64])
@pytest.mark.parametrize("name", E.SOLVE_CASES)
def test_solve_matches_oracle(Solver, name, W, monkeypatch):
    prm, sc = E.make_case(name)
    monkeypatch.setenv("SMPC_SOLVE_WIDTH", str(W))
    s = Solver(prm)
    assert s.solve_slot_width(sc.B, sc.T, sc.N) == W
    r = s.solve(sc)
    counts, worst = check_solve(prm, sc, r)
    POPULATION[(name, W)] = counts
    # the solve kernel's own sweep, tied to the rows held above: its initial cost is K1's at the projected start point
    ev = s.evaluate(sc, projected_start(prm, sc))
    assert np.allclose(ev["cost"], r["initial_cost"], rtol=1e-12)
    print(f"\n[obstacle solve] {name} W={W}: worst firm |dcmd| {worst:.2e}; set aside {counts['scenes'] - counts['firm']}/{counts['scenes']}")


def test_solve_population(oracle):
    if set(POPULATION) != {(n, W) for n in E.SOLVE_CASES for W in (32, 64)}:
        pytest.skip("needs test_solve_matches_oracle of every case in the same run")
    total = None
    for n in POPULATION.values():
        total = add_counts(total, n)
    print(f"\n[obstacle solve] {total['scenes']} scenes: {total['stable']} well conditioned, {total['firm']} firm, "
          f"{total['moved']} moved, {total['clean']} of {total['noise_free']} clean")
    check_population(total)
    # the obstacle term is live in these solves: an assertion on the inputs, by the oracle alone
    live = np.concatenate([v[3] for v in solve_inputs(oracle).values()])
    assert live.mean() >= 0.5


def test_trace_variant_on_a_border_crossing_case(Solver):
    prm, sc = E.make_case("solve_crossing")
    s = Solver(prm)
    same(s.solve(sc), s.solve_trace(sc), RESULT_KEYS, what="solve_trace")


def test_map_sizes_of_zero_are_refused_and_one_by_one_is_served(Solver, oracle):
    from nav2_social_mpc_controller_amd.solver import SmpcError
    prm, sc = E.make_case("narrow_1x1")
    assert (sc.size_x, sc.size_y) == (1, 1)
    s = Solver(prm)
    for shape in ((0, 1), (1, 0), (0, 0)):
        bad = sc.select(np.arange(sc.B))
        bad.costmap = np.zeros((sc.costmap.shape[0],) + shape, np.uint8)
        with pytest.raises(SmpcError):
            s.solve(bad)
        with pytest.raises(SmpcError):
            s.evaluate(bad, bad.init_params)
    check_k1(s, [(prm, np.arange(sc.B))], sc, sc.init_params)
    counts, _ = check_solve(prm, sc, s.solve(sc))
    assert counts["firm"] >= 1      # check_solve compared something


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", ["solve_narrow_3x9", "solve_crossing"])
def test_a_nan_start_pose_fails_its_scene_alone(Solver, name, monkeypatch):
    """test_gpu_parity.test_non_finite_inputs_terminate_and_fail_cleanly's rule on the byte path (a narrow map) and on the
    clamped dword path (a wide one), two scenes per wave: the scene ends as FAILURE, its wave partner and everybody else
    get the bits they get without it."""
    prm, sc = E.make_case(name)
    monkeypatch.setenv("SMPC_SOLVE_WIDTH", "32")
    s = Solver(prm)
    assert s.solve_slot_width(sc.B, sc.T, sc.N) == 32
    clean = s.solve(sc)
    bad = sc.select(np.arange(sc.B))
    bad.pose0[6, 2] = np.nan          # start heading
    bad.pose0[11, 0] = np.nan         # start position: the cell coordinate itself
    out = s.solve(bad)
    hit = np.array([6, 11])
    assert np.all(out["status"][hit] == 2), out["status"][hit]
    rest = np.setdiff1d(np.arange(sc.B), hit)
    same(out, clean, RESULT_KEYS, where=rest, what=name)
