"""The LM solver's rare exits and branches on the device (`-m gpu`): the cases of tests/lm_exit_cases.py, which
tests/test_lm_exits.py shows to reach GRADIENT_TOL (behind a step and before iteration 1), PARAMETER_TOL, MIN_RADIUS,
INVALID_STEPS, the failing line search and both orders of the tolerance tests on the CPU oracle, at N = 4 and N = 8:

  "w32"      two scenes per wave (SMPC_SOLVE_WIDTH=32); N = 8 is the fixed-shape headline kernel, and is launched again
             with the run-time-shape kernel, bit for bit
  "default"  the width the library picks for batches this small: one scene per wave, helper lanes at N = 8

The parity cases go through parity_checks.check_solve unchanged (and `reason`, which it does not compare); the exact
cases compare every scene; pinned_box_fixed, whose oracle path is not determined by its inputs, is held to invariants.
Then the exits inside mixed launches: scenes that leave at iteration 0, or fail after five invalid steps, beside scenes
that run on in the same wave, and in slots that take their next scene from the queue.

No tolerance of its own: 1e-5 on commands (check_solve), 1e-10 on costs, 10 x the oracle's spread on trace columns,
ulps on the radius. Measured worst values: DESIGN.md section 4, "LM exits"."""
import numpy as np
import pytest

import lm_exit_cases as L
from conftest import yaw_err
from parity_checks import add_counts, check_population, check_solve
from test_gpu_instantiations import RESULT_KEYS, same
from test_gpu_trace import INT_COLS, REAL_COLS, TRACE_KEYS, check_rows, on_device, oracle_rows, rel
from test_trace_oracle_rules import COL, TOLERANCE, check_radius_recurrence
from nav2_social_mpc_controller_amd.params import scene_param_rows

pytestmark = pytest.mark.gpu

MODES = ("w32", "default")
ROW_SCENES = 32   # the first scenes of a parity case whose rows are compared: the oracle's traces come one scene at a time
PARITY_RUNS = [(n, alt) for n in L.PARITY for alt in ((False, True) if L.CASES[n].alt else (False,))]
ZERO_PRM, PIN_PRM = L.README.replace(**L.ZERO), L.README.replace(**L.PIN)

_device, _parity, _rows = {}, {}, {}


@pytest.fixture(scope="module")
def Solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    return BatchSolver


def solver_at(Solver, monkeypatch, prm, mode, B, N):
    if mode == "w32":
        monkeypatch.setenv("SMPC_SOLVE_WIDTH", "32")
    else:
        monkeypatch.delenv("SMPC_SOLVE_WIDTH", raising=False)
    s = Solver(prm)
    assert s.solve_slot_width(B, L.T, N) == (32 if mode == "w32" else 64)
    return s


def device_of(Solver, monkeypatch, name, N, mode, alt=False):
    """solve_trace() of one case (once per session): the traced solve, checked here to return the untraced solve's
    results bit for bit, and at "w32" with N = 8 the fixed-shape kernel's results to be the run-time-shape kernel's."""
    key = (name, N, mode, alt)
    if key not in _device:
        prm, sc = L.params_of(name, alt), L.scenes_of(name, N)
        s = solver_at(Solver, monkeypatch, prm, mode, sc.B, N)
        plain, res = s.solve(sc), s.solve_trace(sc)
        same(plain, res, RESULT_KEYS, what=(key, "traced"))
        if mode == "w32":
            assert s.solve_shape_is_fixed(sc.B, L.T, N) == (N == 8)
        if mode == "w32" and N == 8:
            s.set_fixed_shapes(False)
            assert not s.solve_shape_is_fixed(sc.B, L.T, N)
            same(plain, s.solve(sc), RESULT_KEYS, what=(key, "run-time shape"))
            same(res, s.solve_trace(sc), RESULT_KEYS + TRACE_KEYS, what=(key, "run-time shape, traced"))
        _device[key] = res
    return _device[key]


def parity_of(Solver, monkeypatch, name, N, mode, alt):
    """(device result, check_solve's counts, worst firm command error) of one parity launch, once per session"""
    key = (name, N, mode, alt)
    if key not in _parity:
        rg = device_of(Solver, monkeypatch, name, N, mode, alt)
        counts, worst = check_solve(L.params_of(name, alt), L.scenes_of(name, N), rg)
        _parity[key] = (rg, counts, worst)
    return _parity[key]


# ---------------------------------------------------------------------------------------------------------------------
# a. the parity cases


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", L.SIZES)
@pytest.mark.parametrize("name,alt", PARITY_RUNS)
def test_parity_cases_match_the_oracle(Solver, oracle, name, alt, N, mode, monkeypatch):
    c = L.CASES[name]
    rg, counts, worst = parity_of(Solver, monkeypatch, name, N, mode, alt)
    rz, firm = L.oracle_of(name, N, alt)
    assert counts["firm"] == firm.sum()  # the scenes check_solve compared
    assert np.array_equal(rg["reason"][firm], rz["reason"][firm]), np.where(firm & (rg["reason"] != rz["reason"]))[0]
    named = firm & (rg["reason"] == c.named)
    cost = np.max(np.abs(rg["final_cost"][firm] - rz["final_cost"][firm]) / rz["final_cost"][firm])
    print(f"\n[lm exits] {name} alt={alt} N={N} {mode}: {firm.sum()}/{c.B} firm, {named.sum()} by {c.named}, worst firm |dcmd| "
          f"{worst:.2e}, rel |dcost| {cost:.2e}, moved {counts['moved']}")
    assert firm.mean() >= L.FIRM_SHARE and named.sum() >= L.NAMED_SCENES
    assert np.allclose(rg["initial_cost"], rz["initial_cost"], rtol=1e-10)
    check_rows(rg, c.prm.max_iterations)


def test_set_aside_scenes_are_few_over_the_parity_cases(Solver, oracle, monkeypatch):
    """check_population() over every launch of test_parity_cases_match_the_oracle (1024 scenes): one launch of 64 is too
    small for its shares to mean anything."""
    total = None
    for name, alt in PARITY_RUNS:
        for N in L.SIZES:
            for mode in MODES:
                total = add_counts(total, parity_of(Solver, monkeypatch, name, N, mode, alt)[1])
    print(f"\n[lm exits population] {total['scenes']} scenes: {total['stable']} well conditioned, {total['firm']} firm, "
          f"{total['moved']} moved, {total['clean']} of {total['noise_free']} clean")
    check_population(total)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", L.SIZES)
def test_the_successful_step_flag_decides_on_the_device(Solver, oracle, N, mode, monkeypatch):
    """What tests/test_lm_exits.py shows for the oracle: with the flag no compared scene ends by a tolerance before it has
    accepted a step, without it many stop in their first iteration, and the flag changes the iteration count of a large
    share of the scenes firm under both."""
    name = "successful_step_rule"
    r0, r1 = (parity_of(Solver, monkeypatch, name, N, mode, alt)[0] for alt in (False, True))
    f0, f1 = L.oracle_of(name, N)[1], L.oracle_of(name, N, alt=True)[1]
    for b in np.where(f1)[0]:
        tr = r1["trace"][b, :r1["trace_rows"][b]]
        if r1["reason"][b] in TOLERANCE:
            assert tr[1:-1, COL["accepted"]].any() and r1["iterations"][b] >= 2, b
    both = f0 & f1
    changed = both & (r0["iterations"] != r1["iterations"])
    first = f0 & (r0["iterations"] == 1)
    print(f"\n[lm exits] {name} N={N} {mode}: {both.sum()} compared, the flag changes the iteration count of {changed.sum()}, "
          f"{first.sum()} stop in iteration 1 without it")
    assert changed.sum() >= L.FLAG_CHANGES[N] and first.sum() >= L.FIRST_ITERATION_STOPS[N]
    assert not (f1 & (r1["iterations"] < 2)).any()


# ---------------------------------------------------------------------------------------------------------------------
# b. the exact cases: every scene, and (c) their rows


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", L.SIZES)
@pytest.mark.parametrize("name", L.EXACT)
def test_exact_cases_equal_the_oracle(Solver, oracle, name, N, mode, monkeypatch):
    c = L.CASES[name]
    res = device_of(Solver, monkeypatch, name, N, mode)
    rz, firm = L.oracle_of(name, N)
    assert firm.all()
    for k in ("status", "reason", "iterations", "params", "cmds"):
        assert np.array_equal(res[k], rz[k]), k
    assert (res["reason"] == c.named).all()
    start = L.projected_start(name, N)
    assert np.array_equal(res["params"], start)  # FAILURE scenes too: the projected start point is handed back
    assert (res["status"] == (L.FAILURE if name == "invalid_steps" else L.CONVERGENCE)).all()
    assert (res["evaluations"] == 1).all()       # the device's count: 1 + the sum of ls_evals (check_rows)
    dcost = np.abs(res["initial_cost"] - rz["initial_cost"]) / np.maximum(rz["initial_cost"], 1e-300)
    print(f"\n[lm exits] {name} N={N} {mode}: {c.B}/{c.B} compared, reason {c.named}, worst rel |dcost| {dcost.max():.2e}")
    assert np.allclose(res["initial_cost"], rz["initial_cost"], rtol=1e-10, atol=0.0)
    assert np.allclose(res["final_cost"], rz["final_cost"], rtol=1e-10, atol=0.0)
    assert np.array_equal(res["final_cost"], res["initial_cost"])
    # the path: the re-roll of the projected start point (the oracle's, whose params are that point)
    assert np.max(np.abs(res["path"][:, :, :2] - rz["path"][:, :, :2])) <= 1e-12
    assert np.max(yaw_err(res["path"][:, :, 2], rz["path"][:, :, 2])) <= 1e-12
    check_rows(res, c.prm.max_iterations)  # invalid_steps: the INVALID_STEPS branch, trace_rows == iterations
    want_rows = 5 if name == "invalid_steps" else 1
    assert (res["trace_rows"] == want_rows).all()
    for b in range(c.B):
        got, want = res["trace"][b, :want_rows], L.oracle_trace(name, N, b)
        if name == "invalid_steps":
            # Bit for bit, the radius among them (1e4 / 2 / 4 / 8 / 16). The row of an invalid step carries
            # gradient_max_norm (include/smpc.h; the kernel writes gmax, the oracle's Trace() its gradient_max_norm_); with
            # every weight zero that is 0, so this case cannot tell a row that carries the gradient norm from one that
            # writes 0 there. The column's rule stays as smpc.h states it.
            assert np.array_equal(got, want), b
            assert np.array_equal(got[:, COL["radius"]], L.INVALID_RADII), b
        else:
            assert np.array_equal(got[:, INT_COLS], want[:, INT_COLS]), b
            assert np.max(rel(got, want)) <= 1e-10, b  # the cost: within the bound on costs; every other entry is exact
            assert np.array_equal(np.delete(got, COL["cost"], axis=1), np.delete(want, COL["cost"], axis=1)), b


# ---------------------------------------------------------------------------------------------------------------------
# c. the rows of the parity cases


def rows_of(oracle, name, N, alt):
    key = (name, N, alt)
    if key not in _rows:
        sc = L.scenes_of(name, N)
        _rows[key] = oracle_rows(oracle, L.params_of(name, alt), sc.select(np.arange(ROW_SCENES)))
    return _rows[key]


@pytest.mark.parametrize("N", L.SIZES)
@pytest.mark.parametrize("name,alt", PARITY_RUNS)
def test_rows_match_the_oracles(Solver, oracle, name, alt, N, monkeypatch):
    """The rule of test_gpu_trace.test_rows_match_the_oracles on the first ROW_SCENES scenes of each parity case: on the firm
    scenes whose rows are determined by their inputs the iteration counts agree, the integer columns are equal in every
    row, and the real-valued ones lie within 10 x the move of the oracle's own rows under a 1e-15 perturbation.

    At least three quarters of the scenes are compared: a parity case has four fifths of its scenes firm, and a few of
    those change their LM path under the perturbation."""
    rz, rows, usable, spread = rows_of(oracle, name, N, alt)
    compared = usable & L.oracle_of(name, N, alt)[1][:ROW_SCENES]
    assert compared.mean() >= 0.75, (name, N, int(compared.sum()))
    for mode in MODES:
        res = device_of(Solver, monkeypatch, name, N, mode, alt)
        assert np.array_equal(res["iterations"][:ROW_SCENES][compared], rz["iterations"][compared])
        worst = np.zeros(9)
        for b in np.where(compared)[0]:
            want, got = rows[b], res["trace"][b, :res["trace_rows"][b]]
            assert got.shape == want.shape, (b, got.shape, want.shape)
            assert np.array_equal(got[:, INT_COLS], want[:, INT_COLS]), b
            worst = np.maximum(worst, rel(got, want).max(axis=0))
        print(f"\n[lm exits rows] {name} alt={alt} N={N} {mode}: {compared.sum()}/{ROW_SCENES} compared; " +
              " ".join(f"{c}: oracle {spread[COL[c]]:.1e} device {worst[COL[c]]:.1e}" for c in COL if COL[c] in REAL_COLS))
        for j in REAL_COLS:
            assert worst[j] <= 10.0 * spread[j], (name, N, mode, list(COL)[j], worst[j], spread[j])


# ---------------------------------------------------------------------------------------------------------------------
# d. the failing line search and the minimum radius, by invariants


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", L.SIZES)
def test_pinned_box_fixed_invariants(Solver, oracle, N, mode, monkeypatch):
    """Every candidate is the start point itself: no step can be accepted, every line search fails behind several samples,
    and the radius falls until MIN_RADIUS or the iteration cap ends the solve. The oracle's iteration counts are not
    compared: every decision of these scenes is marginal (tests/lm_exit_cases.py)."""
    name = "pinned_box_fixed"
    c = L.CASES[name]
    res = device_of(Solver, monkeypatch, name, N, mode)
    rz, _ = L.oracle_of(name, N)
    assert np.array_equal(res["params"], np.tile(L.PIN_POINT, (c.B, 1)))
    assert np.array_equal(res["final_cost"].view(np.uint64), res["initial_cost"].view(np.uint64))
    assert np.allclose(res["initial_cost"], rz["initial_cost"], rtol=1e-10, atol=0.0)
    assert set(zip(res["status"].tolist(), res["reason"].tolist())) <= {(L.CONVERGENCE, L.MIN_RADIUS), (L.NO_CONVERGENCE, L.MAX_ITERATIONS)}
    assert (res["reason"] == L.MIN_RADIUS).any() and (rz["reason"] == L.MIN_RADIUS).any()
    check_rows(res, c.prm.max_iterations)  # evaluations == 1 + sum(ls_evals) and the radius recurrence at 8 ulp among its rules
    for b in range(c.B):
        tr = res["trace"][b, :res["trace_rows"][b]]
        assert not tr[1:, COL["accepted"]].any(), b
        check_radius_recurrence(tr, int(res["reason"][b]), max_ulp=8)
        assert res["evaluations"][b] == 1 + int(tr[:, COL["ls_evals"]].sum()), b
        assert tr[:, COL["ls_evals"]].max() >= 5, b  # the failing line search ran
        if res["reason"][b] == L.MIN_RADIUS:
            assert tr[-1, COL["radius"]] <= 1e-32 < tr[-2, COL["radius"]], b
        else:
            assert res["iterations"][b] == c.prm.max_iterations and tr[-1, COL["radius"]] > 1e-32, b
    print(f"\n[lm exits] {name} N={N} {mode}: by MIN_RADIUS {(res['reason'] == L.MIN_RADIUS).sum()} (oracle "
          f"{(rz['reason'] == L.MIN_RADIUS).sum()}) of {c.B}, iterations {sorted(set(res['iterations'].tolist()))}")


# ---------------------------------------------------------------------------------------------------------------------
# e. mixed launches, f. re-used slots

GROUPS = (L.README, ZERO_PRM, PIN_PRM)  # scene b takes GROUPS[b % 3]'s weights and bounds


def cycle(B):
    return np.arange(B) % len(GROUPS)


def mixed(sc):
    return sc.with_scene_params(scene_param_rows(GROUPS, cycle(sc.B)))


@pytest.mark.parametrize("N", L.SIZES)
@pytest.mark.parametrize("fixed_iterations", [0, 1])
def test_mixed_exits_equal_uniform_launches(Solver, N, fixed_iterations, monkeypatch):
    """One launch whose scenes cycle through README / zero weights / a pinned box, two scenes per wave: a scene that leaves
    at iteration 0 (with fixed_iterations: fails after five invalid steps, or runs into the minimum radius) shares its wave
    with one that runs on. Every result array and every row equals, bit for bit, the launch in which all scenes take that
    scene's parameters (the pattern of test_mixed_presets_equal_uniform_launches)."""
    monkeypatch.setenv("SMPC_SOLVE_WIDTH", "32")
    sc = L.scenes_of("param_tol", N).select(np.arange(48))
    which = cycle(sc.B)
    handle = lambda p: Solver(p.replace(fixed_iterations=fixed_iterations))
    s = handle(L.README)
    assert s.solve_slot_width(sc.B, L.T, N) == 32
    got = s.solve_trace(mixed(sc))
    same(s.solve(mixed(sc)), got, RESULT_KEYS, what="traced")
    for k, p in enumerate(GROUPS):
        same(got, handle(p).solve_trace(sc), RESULT_KEYS + TRACE_KEYS, where=np.where(which == k)[0], what=("uniform", k))
    check_rows(got, L.README.max_iterations)
    zero, pin, run = (got["reason"][which == k] for k in (1, 2, 0))
    if fixed_iterations:
        assert (zero == L.INVALID_STEPS).all() and set(pin.tolist()) <= {L.MIN_RADIUS, L.MAX_ITERATIONS}
        assert ((got["iterations"][which == 0] == L.README.max_iterations) | (run == L.MIN_RADIUS) | (run == L.INVALID_STEPS)).all()
        assert (got["iterations"][which == 0] > 5).all()
    else:
        assert (zero == L.GRADIENT_TOL).all() and (pin == L.GRADIENT_TOL).all() and not got["iterations"][which != 0].any()
        assert (got["iterations"][which == 0] > 0).all()


@pytest.mark.parametrize("N", L.SIZES)
@pytest.mark.parametrize("fixed_iterations", [0, 1])
def test_mixed_exits_with_horizons_and_short_paths(Solver, N, fixed_iterations, monkeypatch):
    """The same with a horizon per scene (the kVT instantiation) and three scenes without a path (T_scene = 0, one of each
    group): SHORT_PATH, an exit at iteration 0 and a running scene in the same waves."""
    monkeypatch.setenv("SMPC_SOLVE_WIDTH", "32")
    from test_gpu_instantiations import horizons
    sc = L.scenes_of("param_tol", N).select(np.arange(48))
    sc = sc.with_horizons(horizons(sc.B, L.T, 31))
    which, short = cycle(sc.B), [1, 5, 9]
    assert sorted(which[short].tolist()) == [0, 1, 2]
    handle = lambda p: Solver(p.replace(fixed_iterations=fixed_iterations))
    plain, got = on_device(handle(L.README), mixed(sc), short=short)
    same(plain, got, RESULT_KEYS, what="traced")
    assert (got["reason"][short] == 8).all() and (got["status"][short] == L.FAILURE).all() and not got["trace_rows"][short].any()
    for k, p in enumerate(GROUPS):
        uniform = on_device(handle(p), sc, short=short)[1]
        same(got, uniform, RESULT_KEYS + TRACE_KEYS, where=np.where(which == k)[0], what=("uniform", k))
    check_rows(got, L.README.max_iterations)
    rest = np.setdiff1d(np.arange(sc.B), short)
    want = (L.INVALID_STEPS if fixed_iterations else L.GRADIENT_TOL)
    assert (got["reason"][rest][which[rest] == 1] == want).all()


@pytest.mark.parametrize("fixed_iterations", [0, 1])
def test_slots_that_take_further_scenes_behind_a_rare_exit(Solver, fixed_iterations, monkeypatch):
    """More scenes than the persistent grid has slots (test_gpu_fixed_shape's batch of 8192 + 37), cycling through the three
    groups: a slot takes its next scene behind one that left at iteration 0, failed after five invalid steps (its count of
    invalid steps, its flags and the radius divisor must not reach the next scene) or ran into the minimum radius. About
    200 scenes spread over the batch, the first and the last among them, equal bit for bit what launches of 48 scenes at
    the same slot width give for them. No oracle at this size."""
    from nav2_social_mpc_controller_amd.scenes import make_scenes
    monkeypatch.setenv("SMPC_SOLVE_WIDTH", "32")
    Bq, N = 8192 + 37, 8
    sc = make_scenes(L.README, 1024, N, T=L.T, seed=2803, map_cells=L.MAP_CELLS)  # 1024 different scenes, repeated
    big = mixed(sc.select(np.arange(Bq) % 1024))
    s = Solver(L.README.replace(fixed_iterations=fixed_iterations))
    assert s.solve_slot_width(Bq, L.T, N) == 32 and s.solve_slot_width(48, L.T, N) == 32
    got = s.solve_trace(big)
    same(s.solve(big), got, RESULT_KEYS, what="traced")
    pick = np.unique(np.concatenate([[0, 1, 2, Bq - 3, Bq - 2, Bq - 1], np.linspace(0, Bq - 1, 200).astype(np.int64)]))
    assert set(cycle(Bq)[pick].tolist()) == {0, 1, 2}
    for lo in range(0, len(pick), 48):
        idx = pick[lo:lo + 48]
        small = s.solve_trace(big.select(idx))
        for k in RESULT_KEYS + TRACE_KEYS:
            assert np.array_equal(small[k].view(np.uint8), np.ascontiguousarray(got[k][idx]).view(np.uint8)), (k, lo)
    which = cycle(Bq)
    if fixed_iterations:
        assert (got["reason"][which == 1] == L.INVALID_STEPS).all() and (got["iterations"][which == 1] == 5).all()
        assert (got["trace_rows"][which == 1] == 5).all()
        assert set(got["reason"][which == 2].tolist()) <= {L.MIN_RADIUS, L.MAX_ITERATIONS}
    else:
        assert (got["reason"][which != 0] == L.GRADIENT_TOL).all() and not got["iterations"][which != 0].any()
    assert (got["status"][which == 0] != L.FAILURE).all()
