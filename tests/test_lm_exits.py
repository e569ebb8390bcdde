"""The rare exits and branches of the LM solver on the CPU oracle alone (no GPU): every case of tests/lm_exit_cases.py
reaches what it is there for on enough firm scenes for tests/test_gpu_lm_exits.py to compare the device with, the exact
cases give the integers and rows the device is held to, the oracle's rows obey the radius recurrence on these paths
too, and oracle/pyref.py (the independent restatement of SURVEY Appendix A) takes the same exits."""
import numpy as np
import pytest

import lm_exit_cases as L
from test_trace_oracle_rules import COL, TOLERANCE, check_radius_recurrence

TRACED = 16  # scenes per case and N whose rows are read here: the oracle's traces come one scene at a time
CASE_SIZES = [(name, N) for name in L.CASES for N in L.SIZES]
OTHER_COLS = [COL[c] for c in COL if c not in ("iter", "radius")]


def rows_of(name, N, alt=False):
    return [L.oracle_trace(name, N, b, alt) for b in range(min(TRACED, L.CASES[name].B))]


def bins(reasons):
    return np.bincount(reasons, minlength=9).tolist()


def flag_effect(N):
    """successful_step_rule on the oracle: (scenes firm under both flags, those whose iteration count the flag changes,
    the firm scenes of flag 0 that stop in their first iteration)"""
    (r0, f0), (r1, f1) = L.oracle_of("successful_step_rule", N), L.oracle_of("successful_step_rule", N, alt=True)
    both = f0 & f1
    return both, both & (r0["iterations"] != r1["iterations"]), f0 & (r0["iterations"] == 1)


@pytest.mark.parametrize("name,N", [(n, N) for n in L.PARITY for N in L.SIZES])
def test_parity_cases_have_enough_firm_scenes_by_their_exit(oracle, name, N):
    """(no GPU) what the device comparison may rely on, before any device result is known"""
    c = L.CASES[name]
    for alt in (False, True) if c.alt else (False,):
        rz, firm = L.oracle_of(name, N, alt)
        named = firm & (rz["reason"] == c.named)
        print(f"\n[lm exits oracle] {name} N={N} alt={alt}: {firm.sum()}/{c.B} firm, by reason {bins(rz['reason'][firm])}, "
              f"{named.sum()} by {c.named}")
        assert firm.mean() >= L.FIRM_SHARE, (name, N, float(firm.mean()))
        assert named.sum() >= L.NAMED_SCENES, (name, N, int(named.sum()))
        assert set(rz["reason"][firm].tolist()) <= c.reasons
    if name == "gradient_tol":  # behind an accepted step, not before iteration 1 (that is zero_gradient's and pinned_box's)
        assert rz["iterations"][named].min() >= 1
    if name == "successful_step_rule":
        both, changed, first = flag_effect(N)
        r1, f1 = L.oracle_of(name, N, alt=True)
        print(f"[lm exits oracle] {name} N={N}: {both.sum()} firm under both flags, the flag changes the iteration count of "
              f"{changed.sum()}; {first.sum()} firm scenes stop in iteration 1 with flag 0; least iterations with flag 1: "
              f"{r1['iterations'][f1].min()}")
        # on a cold start the flag changes nothing: the warm start is what makes the case tell the two orders apart
        assert changed.sum() >= L.FLAG_CHANGES[N] and first.sum() >= L.FIRST_ITERATION_STOPS[N]
        assert r1["iterations"][f1].min() >= 2  # an accepted step, then the iteration whose tolerance test ends the solve


@pytest.mark.parametrize("name,N", [(n, N) for n in L.EXACT for N in L.SIZES])
def test_exact_cases_on_the_oracle(oracle, name, N):
    c = L.CASES[name]
    rz, firm = L.oracle_of(name, N)
    sc = L.scenes_of(name, N)
    print(f"\n[lm exits oracle] {name} N={N}: {firm.sum()}/{c.B} firm, by reason {bins(rz['reason'])}, "
          f"initial cost {rz['initial_cost'].min():.4g} .. {rz['initial_cost'].max():.4g}")
    assert firm.all()
    assert (rz["reason"] == c.named).all() and (rz["evaluations"] == 1).all()
    assert np.array_equal(rz["params"], L.projected_start(name, N))
    assert np.array_equal(rz["final_cost"], rz["initial_cost"])
    if name == "invalid_steps":
        assert (rz["status"] == L.FAILURE).all() and (rz["iterations"] == 5).all()
    else:
        assert (rz["status"] == L.CONVERGENCE).all() and (rz["iterations"] == 0).all()
    if name == "pinned_box":  # a cost far from zero whose projected gradient is zero
        assert np.array_equal(rz["params"], np.tile(L.PIN_POINT, (c.B, 1))) and rz["initial_cost"].min() > 1.0
    else:
        assert not rz["initial_cost"].any()
    for b, tr in enumerate(rows_of(name, N)):
        if name == "invalid_steps":
            # row 0 and the four invalid steps that halve the radius; the fifth ends the solve without a row
            assert tr.shape == (5, 9) and np.array_equal(tr[:, COL["iter"]], np.arange(5)), b
            assert np.array_equal(tr[:, COL["radius"]], L.INVALID_RADII), b
            assert tr[0, COL["accepted"]] == 1 and not tr[1:, OTHER_COLS].any() and not tr[0, OTHER_COLS[:-1]].any(), b
        else:
            assert np.array_equal(tr, [[0, rz["initial_cost"][b], 0, 0, 0, 0, 1e4, 0, 1]]), b
        check_radius_recurrence(tr, c.named, max_ulp=4)
    assert sc.B == c.B


@pytest.mark.parametrize("N", L.SIZES)
def test_pinned_box_fixed_on_the_oracle(oracle, N):
    """The invariants tests/test_gpu_lm_exits.py holds the device to, on the oracle: no scene is firm (each sample's cost
    equals the start cost), so nothing else of its path is compared."""
    name = "pinned_box_fixed"
    c = L.CASES[name]
    rz, firm = L.oracle_of(name, N)
    print(f"\n[lm exits oracle] {name} N={N}: {firm.sum()}/{c.B} firm, by reason {bins(rz['reason'])}, iterations "
          f"{sorted(set(rz['iterations'].tolist()))}")
    assert set(rz["reason"].tolist()) <= c.reasons and (rz["reason"] == L.MIN_RADIUS).sum() >= 8
    assert np.array_equal(rz["params"], np.tile(L.PIN_POINT, (c.B, 1)))
    assert np.array_equal(rz["final_cost"], rz["initial_cost"])
    noise = 0
    for b, tr in enumerate(rows_of(name, N)):
        # The oracle evaluates a candidate's cost without the Jacobian and the adopted point's with it: the two costs of
        # the one point differ in their last bits, and once the radius is small that noise over a tiny model cost change
        # can pass for a relative decrease ("accepted" rows at the same point, the same cost). The device takes both
        # from one sweep, and is held to "no accepted row" (tests/test_gpu_lm_exits.py).
        noise += int(tr[1:, COL["accepted"]].sum())
        assert np.ptp(tr[:, COL["cost"]]) <= 1e-12 * tr[0, COL["cost"]], b
        assert tr[:, COL["ls_evals"]].max() >= 5, b  # the failing line search ran
        check_radius_recurrence(tr, int(rz["reason"][b]), max_ulp=4)
        if rz["reason"][b] == L.MIN_RADIUS:
            assert tr[-1, COL["radius"]] <= 1e-32 < tr[-2, COL["radius"]], b
    print(f"[lm exits oracle] {name} N={N}: {noise} rows of the first {TRACED} scenes accepted on rounding noise")


def test_the_cases_reach_every_exit_and_branch(oracle):
    """The census: the firm scenes end by GRADIENT_TOL, PARAMETER_TOL, FUNCTION_TOL, MAX_ITERATIONS and INVALID_STEPS;
    MIN_RADIUS, rows of invalid steps, rejected steps and line searches of five samples and more occur on some scene."""
    firm_reasons, reasons, invalid, rejected, long_search = set(), set(), 0, 0, 0
    for name, N in CASE_SIZES:
        for alt in (False, True) if L.CASES[name].alt else (False,):
            rz, firm = L.oracle_of(name, N, alt)
            firm_reasons |= set(rz["reason"][firm].tolist())
            reasons |= set(rz["reason"].tolist())
            for b, tr in enumerate(rows_of(name, N, alt)):
                invalid += int((tr[1:, COL["ls_evals"]] == 0).sum())
                steps = tr[1:-1] if rz["reason"][b] in TOLERANCE else tr[1:]  # a tolerance exit's last row is no rejection
                rejected += int(((steps[:, COL["accepted"]] == 0) & (steps[:, COL["ls_evals"]] >= 1)).sum())
                long_search += int((tr[:, COL["ls_evals"]] >= 5).sum())
    print(f"\n[lm exits census] firm scenes end by {sorted(firm_reasons)}, all by {sorted(reasons)}; rows: {invalid} invalid, "
          f"{rejected} rejected, {long_search} with ls_evals >= 5")
    assert firm_reasons >= {L.GRADIENT_TOL, L.PARAMETER_TOL, L.FUNCTION_TOL, L.MAX_ITERATIONS, L.INVALID_STEPS}
    assert L.MIN_RADIUS in reasons and invalid > 0 and rejected > 0 and long_search > 0


@pytest.mark.parametrize("name,N", [(n, N) for n in L.PARITY + ["pinned_box_fixed"] for N in L.SIZES])
def test_oracle_rows_obey_the_radius_recurrence(oracle, name, N):
    """(the exact cases' rows are checked with their values above)"""
    for alt in (False, True) if L.CASES[name].alt else (False,):
        rz, _ = L.oracle_of(name, N, alt)
        for b, tr in enumerate(rows_of(name, N, alt)):
            assert len(tr) == rz["iterations"][b] + 1, (b, len(tr))
            check_radius_recurrence(tr, int(rz["reason"][b]), max_ulp=4)


PYREF_REASON = {"gradient_tol": L.GRADIENT_TOL, "parameter_tol": L.PARAMETER_TOL, "function_tol": L.FUNCTION_TOL,
                "min_radius": L.MIN_RADIUS, "max_iterations": L.MAX_ITERATIONS, "invalid_steps": L.INVALID_STEPS}
PYREF_SCENES = {"pinned_box": 3, "param_tol": 2, "gradient_tol": 2}


@pytest.mark.parametrize("name", list(PYREF_SCENES))
def test_pyref_takes_the_same_exit(oracle, name):
    """oracle/pyref.py against the reference-literal oracle (pyref has no theta convention; nobody stands in these scenes, so
    the two conventions are one), N = 3: the same exit, the same iteration count, x within the bound of
    test_oracle_solve_matches_pyref_golden."""
    from nav2_social_mpc_controller_amd.scenes import make_scenes
    from oracle import pyref

    c = L.CASES[name]
    sc = make_scenes(c.prm, c.B, 3, map_cells=L.MAP_CELLS, seed=c.seed, standing_fraction=0.0)
    ro = oracle.solve(c.prm, sc, nthreads=16)
    assert not ro["sign_noise_events"].any()
    # pyref takes half a second per evaluation: of the scenes that end by the case's exit with firm decisions, the ones
    # the oracle needs the fewest evaluations for
    mine = np.where((ro["marginal_decisions"] == 0) & (ro["reason"] == c.named))[0]
    mine = mine[np.argsort(ro["evaluations"][mine], kind="stable")][:PYREF_SCENES[name]]
    assert len(mine) == PYREF_SCENES[name]
    for b in mine:
        got = pyref.solve(c.prm, sc, b)
        print(f"\n[lm exits pyref] {name} scene {b}: {got['reason']} after {got['iterations']} iterations, "
              f"max |dx| {np.abs(got['x'] - ro['params'][b]).max():.2e}")
        assert PYREF_REASON[got["reason"]] == ro["reason"][b], (b, got["reason"], int(ro["reason"][b]))
        assert got["iterations"] == ro["iterations"][b], b
        assert np.abs(got["x"] - ro["params"][b]).max() < 1e-7, b
