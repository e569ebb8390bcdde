"""The row rules of a solve's per-iteration trace, pinned on the CPU oracle (oracle/smpc_oracle.cpp: Minimizer::Run,
TraceRow) over the committed golden scenes. The device's rows (smpc_solve_trace_batch) follow the same rules;
tests/test_gpu_trace.py asserts them on the device and relies on their holding here. No GPU."""
import numpy as np
import pytest

from conftest import GOLDEN_CASES, load_golden

COL = {n: i for i, n in enumerate(["iter", "cost", "cost_change", "gradient_max_norm", "step_norm", "rho", "radius", "ls_evals",
                                   "accepted"])}
# reasons (enum smpc_reason) behind which every iteration has its row: the tolerances write the row of the iteration they
# end; the cap, the gradient test and the minimum radius end the solve before the next iteration starts
ROW_PER_ITERATION = (1, 2, 3, 4, 5)
TOLERANCE = (2, 3)  # parameter / function tolerance: the last row keeps the radius (no accept / reject update)


def ulps(a, b):
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))


def check_radius_recurrence(tr, reason, max_ulp):
    """Row by row from the previous row's radius: accepted -> min(1e16, r / max(1/3, 1 - (2 rho - 1)^3)); rejected or invalid
    -> r / 2, r / 4, ... (the divisor doubles with every step in a row that is not accepted and restarts at 2 behind an
    accepted one); the row of a tolerance exit keeps r. max_ulp: the cube and the division are rounded once each, by
    whatever power / reciprocal routine the implementation uses."""
    assert tr[0, COL["radius"]] == 1e4
    divisor = 2.0
    for i in range(1, len(tr)):
        prev, row = tr[i - 1, COL["radius"]], tr[i]
        if row[COL["accepted"]] == 1:
            t = 2.0 * row[COL["rho"]] - 1.0
            want, divisor = min(1e16, prev / max(1.0 / 3.0, 1.0 - t * t * t)), 2.0
        elif i == len(tr) - 1 and reason in TOLERANCE:
            want = prev
        else:
            want, divisor = prev / divisor, divisor * 2.0
        assert ulps(row[COL["radius"]], want) <= max_ulp, (i, row[COL["radius"]], want)


def candidate_rows(tr):
    """rows of iterations that evaluated a candidate: every row but row 0 and those of invalid steps (no line search)"""
    return int((tr[1:, COL["ls_evals"]] >= 1).sum())


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_oracle_rows_follow_the_rules(oracle, name):
    prm, sc, _ = load_golden(name)
    res = oracle.solve(prm, sc, nthreads=4)
    for b in range(sc.B):
        tr = oracle.trace(prm, sc, b, max_rows=prm.max_iterations + 2)
        reason, iters = int(res["reason"][b]), int(res["iterations"][b])
        assert reason in ROW_PER_ITERATION, (b, reason)  # what the golden scenes end by
        assert len(tr) == iters + 1, (b, len(tr), iters)
        assert np.array_equal(tr[:, COL["iter"]], np.arange(len(tr)))
        assert np.array_equal(tr[0, [COL[c] for c in ("cost_change", "step_norm", "rho", "ls_evals", "accepted")]], [0, 0, 0, 0, 1])
        assert tr[0, COL["cost"]] == res["initial_cost"][b]
        accepted = tr[tr[:, COL["accepted"]] == 1]
        assert accepted[:, COL["cost"]].min() == res["final_cost"][b]
        # the cube is std::pow there and t * t * t here
        check_radius_recurrence(tr, reason, max_ulp=4)
        # Every sweep is counted: the initial one, the line-search samples, the candidate's cost, and — the oracle only —
        # the Jacobian at the adopted point of every accepted step (the device adopts the last line-search sample, whose
        # Gram it already has: its count is 1 + sum(ls_evals), tests/test_gpu_trace.py).
        n_accepted = int((tr[1:, COL["accepted"]] == 1).sum())
        assert res["evaluations"][b] == 1 + int(tr[:, COL["ls_evals"]].sum()) + candidate_rows(tr) + n_accepted, b


def test_golden_scenes_cover_an_iteration_cap_and_a_rejected_step(oracle):
    reasons, rejected = set(), 0
    for name in GOLDEN_CASES:
        prm, sc, _ = load_golden(name)
        reasons |= set(oracle.solve(prm, sc, nthreads=4)["reason"].tolist())
        for b in range(sc.B):
            tr = oracle.trace(prm, sc, b, max_rows=prm.max_iterations + 2)
            rejected += int(((tr[1:-1, COL["accepted"]] == 0) & (tr[1:-1, COL["ls_evals"]] >= 1)).sum())
    assert {3, 5} <= reasons and rejected > 0
