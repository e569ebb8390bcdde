"""The frame of a solve trip (`-m gpu`): what csrc/smpc_solve_body.inc and the lone-trip agent loop of csrc/smpc_sweep.hpp
do around the arithmetic — the people record fetched one unit ahead over the one just used, the reductions over the
parameters (one sum, two sums, a sum and a maximum taken by a bare v_max_f64), the state machine's flags word, the trip
counters that only a reporting launch keeps, and the division of the trust-region radius by 2, 4, 8, ... as a product
with the exact reciprocal. None of it may change a bit of a result.

Batches of 1, 3 and 5 scenes at SMPC_SOLVE_WIDTH=32: an odd batch leaves a wave half idle, its last scene runs lone trips
(helped, or paired under SMPC_NO_LONE_HELP: the two must agree in every byte), and the record fetched ahead meets the end
of the list at N = 1, 2, an odd N (the helper's last unit) and the headline's 8. Against the oracle by the rules of
tests/parity_checks.py, scene by scene (populations this small are not judged as populations)."""
import numpy as np
import pytest

from parity_checks import check_solve
from nav2_social_mpc_controller_amd.params import OptimizerParams
from nav2_social_mpc_controller_amd.scenes import make_scenes
from test_gpu_instantiations import RESULT_KEYS, same
from test_gpu_trace import INT_COLS, REAL_COLS, oracle_rows, rel
from test_trace_oracle_rules import COL, ulps

pytestmark = pytest.mark.gpu

README = OptimizerParams.readme()
T = 28
BATCHES = (1, 3, 5)
FAILURE, EVAL_FAILED = 2, 7


@pytest.fixture(scope="module")
def Solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    return BatchSolver


@pytest.fixture
def run(Solver, monkeypatch):
    """run(scenes, help=True, fixed=True) -> results of one solve launch of the two-scenes-per-wave kernel"""
    monkeypatch.setenv("SMPC_SOLVE_WIDTH", "32")

    def go(sc, help=True, fixed=True, prm=README):
        if help:
            monkeypatch.delenv("SMPC_NO_LONE_HELP", raising=False)
        else:
            monkeypatch.setenv("SMPC_NO_LONE_HELP", "1")
        s = Solver(prm)
        s.set_fixed_shapes(fixed)
        assert s.solve_slot_width(sc.B, sc.T, sc.N) == 32
        return s.solve(sc)
    return go


def on_off(run, sc, what, **kw):
    a = run(sc, help=True, **kw)
    same(a, run(sc, help=False, **kw), RESULT_KEYS, what=what)
    return a


def frame_case(Solver, run, N, Th, seed):
    """Nine scenes solved as batches of 1, 3 and 5; the oracle judges the nine together (its rules are stated per scene,
    but a batch of one may leave none of its scenes for a rule to look at)."""
    pool = make_scenes(README, sum(BATCHES), N, T=Th, seed=seed, map_cells=80)
    parts, at = [], 0
    for B in BATCHES:
        sc = pool.select(np.arange(at, at + B))
        at += B
        what = f"T = {Th}, N = {N}, B = {B}"
        a = on_off(run, sc, what)
        if Solver(README).solve_shape_is_fixed(B, Th, N):  # the headline shape: its own kernel and the run-time-shape one
            same(a, on_off(run, sc, what + ", run-time shape", fixed=False), RESULT_KEYS, what=what + ": fixed against run-time shape")
        parts.append(a)
    res = {k: np.concatenate([a[k] for a in parts]) for k in RESULT_KEYS}
    counts, worst = check_solve(README, pool, res)
    print(f"\n[trip frame] T = {Th}, N = {N}: {counts['firm']}/{counts['scenes']} scenes firm, {counts['clean']} clean, "
          f"{counts['moved']} moved, worst command error of a firm scene {worst:.1e}")
    assert counts["firm"] >= 5 and counts["clean"] >= 1, counts


@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_headline_horizon_helped_and_paired_agree_and_match_the_oracle(Solver, run, N):
    if N == 8:
        assert Solver(README).solve_shape_is_fixed(BATCHES[0], T, N)
    frame_case(Solver, run, N, T, 3100 + 10 * N)


def test_shortest_horizon_helped_and_paired_agree_and_match_the_oracle(Solver, run):
    """test_gpu_parity's t1_shortest_horizon: T = 1, N = 3 (one parameter block, an odd agent count)"""
    frame_case(Solver, run, 3, 1, 117)


def test_scenes_without_people_beside_scenes_with_people(run):
    sc = make_scenes(README, 5, 8, T=T, seed=3201, map_cells=80)
    sc.has_people[[1, 4]] = 0  # the last scene, alone in its wave, among them
    a = on_off(run, sc, "has_people = 0 for scenes 1 and 4")
    check_solve(README, sc, a)


def test_every_agent_invalid(run):
    sc = make_scenes(README, 3, 3, T=T, seed=3202, map_cells=80, n_valid=0)
    a = on_off(run, sc, "all agents invalid")
    assert (a["status"] == FAILURE).all(), a["status"]  # rejected at the initial evaluation, like the reference


@pytest.mark.parametrize("B", BATCHES)
def test_a_nan_start_command_fails_its_initial_evaluation(run, B):
    """The last scene — the lone one — starts from a NaN command: one evaluation, SMPC_FAILURE / evaluation failed, and the
    scenes beside it are what they are in the clean batch."""
    sc = make_scenes(README, B, 8, T=T, seed=3300 + B, map_cells=80)
    clean = on_off(run, sc, f"clean, B = {B}")
    bad = sc.select(np.arange(B))
    bad.init_params[B - 1, 1] = np.nan
    a = on_off(run, bad, f"NaN start, B = {B}")
    assert a["status"][B - 1] == FAILURE and a["reason"][B - 1] == EVAL_FAILED, (a["status"], a["reason"])
    assert a["evaluations"][B - 1] == 1 and a["iterations"][B - 1] == 0
    same(a, clean, RESULT_KEYS, where=slice(0, B - 1), what="beside the NaN scene")


# ---------------------------------------------------------------------------------------------------------------------
# rejected steps: the radius is divided by 2, 4, 8, ...

REJECT_SCENES = dict(B=24, N=8, T=T, seed=3400, map_cells=80)


def rejected_in_a_row(tr):
    """the longest run of rows that are not accepted (row 0 is)"""
    best = cur = 0
    for acc in tr[1:, COL["accepted"]]:
        cur = 0 if acc == 1 else cur + 1
        best = max(best, cur)
    return best


def test_rows_of_rejected_steps_match_the_oracles(Solver, oracle):
    """test_gpu_trace.test_rows_match_the_oracles' rule on a batch with scenes whose steps are rejected twice and more in a
    row (divisors 2 and 4 at least); and on every row that is not accepted the radius is the previous row's divided by its
    power of two with no rounding at all (the quotient by a power of two is exact)."""
    sc = make_scenes(README, **REJECT_SCENES)
    rz, rows, usable, spread = oracle_rows(oracle, README, sc)
    res = Solver(README).solve_trace(sc)
    compared = usable & (res["iterations"] == rz["iterations"])
    worst, deepest = np.zeros(9), 0
    for b in np.where(compared)[0]:
        want = rows[b]
        got = res["trace"][b, :res["trace_rows"][b]]
        assert got.shape == want.shape, (b, got.shape, want.shape)
        assert np.array_equal(got[:, INT_COLS], want[:, INT_COLS]), b
        worst = np.maximum(worst, rel(got, want).max(axis=0))
        deepest = max(deepest, rejected_in_a_row(got))
    print(f"\n[trip frame] rejected steps: {compared.sum()}/{sc.B} compared, up to {deepest} rejected in a row; " +
          " ".join(f"{c}: oracle {spread[COL[c]]:.1e} device {worst[COL[c]]:.1e}" for c in COL if COL[c] in REAL_COLS))
    assert compared.mean() >= 0.85, float(compared.mean())
    assert deepest >= 2, deepest
    for j in REAL_COLS:
        assert worst[j] <= 10.0 * spread[j], (list(COL)[j], worst[j], spread[j])
    for b in range(sc.B):  # every scene, compared or not
        tr = res["trace"][b, :res["trace_rows"][b]]
        divisor = 2.0
        for i in range(1, len(tr)):
            if tr[i, COL["accepted"]] == 1:
                divisor = 2.0
            elif not (i == len(tr) - 1 and int(res["reason"][b]) in (2, 3)):  # (a tolerance exit keeps the radius)
                assert ulps(tr[i, COL["radius"]], tr[i - 1, COL["radius"]] / divisor) == 0, (b, i)
                divisor *= 2.0
