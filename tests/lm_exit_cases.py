"""The inputs that drive the Levenberg-Marquardt state machine to its rare exits and branches, shared by
tests/test_lm_exits.py (which shows, with the CPU oracle alone, that each case reaches what it is there for on enough firm
scenes) and tests/test_gpu_lm_exits.py (which runs them on the device). Not a test module; imported like conftest.

Every case is the README parameter set (T = 28, three bounded parameter blocks) on make_scenes(prm, B, N, map_cells=80,
seed) with N = 4 and N = 8; a case differs from the seeded parity cases of test_gpu_parity only in its parameters:

  param_tol             a loose parameter tolerance and no function tolerance: PARAMETER_TOL
  gradient_tol          a loose gradient tolerance and no function tolerance: GRADIENT_TOL behind an accepted step
  zero_gradient         every critic weight 0: zero cost and gradient, GRADIENT_TOL before iteration 1
  invalid_steps         the same with fixed_iterations = 1 (no gradient test): the zero step has no model cost change, five
                        invalid steps in a row, FAILURE by INVALID_STEPS, the projected start point handed back
  pinned_box            v_min = v_max, w_min = w_max: a cost above zero whose projected gradient is zero
  pinned_box_fixed      the same with fixed_iterations = 1: every step is valid and every candidate is the start point, so
                        every line search fails behind its first sample and every step is rejected until the radius falls
                        to its minimum (MIN_RADIUS) or the iterations run out. Each sample's cost equals the start cost:
                        every decision of such a scene is marginal, and the oracle's own path moves under 1e-13 of its
                        input, so the case is held to invariants, not to the oracle's rows
  successful_step_rule  a warm start (init_params = the oracle's optimum of the same scenes): with
                        tol_needs_successful_step = 0 the tolerances may end the solve in its first iteration, with 1 (the
                        Ceres >= 2.1 order, `alt`) only behind an accepted step"""
from typing import NamedTuple, Optional

import numpy as np

from conftest import well_conditioned
from nav2_social_mpc_controller_amd.params import OptimizerParams
from nav2_social_mpc_controller_amd.scenes import make_scenes

README = OptimizerParams.readme()
T, P = 28, 6
SIZES = (4, 8)          # N = 8 is the fixed-shape headline kernel's shape
MAP_CELLS = 80
GRADIENT_TOL, PARAMETER_TOL, FUNCTION_TOL, MIN_RADIUS, MAX_ITERATIONS, INVALID_STEPS = 1, 2, 3, 4, 5, 6
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2

WEIGHTS = ("distance_weight", "social_weight", "velocity_weight", "angle_weight", "agent_angle_weight", "proxemics_weight",
           "velocity_feasibility_weight", "obstacle_weight", "goal_align_weight")
ZERO = {w: 0.0 for w in WEIGHTS}
PIN = dict(v_min=0.3, v_max=0.3, w_min=0.1, w_max=0.1)
PIN_POINT = np.tile([0.3, 0.1], P // 2)
# the radius behind each of the four invalid steps that get a row: 1e4 / 2 / 4 / 8 / 16, exactly
INVALID_RADII = np.array([1e4, 5e3, 1250.0, 156.25, 9.765625])


class Case(NamedTuple):
    prm: OptimizerParams
    kind: str                     # "parity": parity_checks.check_solve; "exact": every scene; "invariants": no oracle rows
    named: int                    # the exit the case is there for
    reasons: frozenset            # what a firm scene of the oracle ends by (every scene where no scene is firm)
    B: int = 64
    seed: int = 910
    warm: bool = False            # init_params := the oracle's optimum under README
    alt: Optional[OptimizerParams] = None


CASES = {
    "param_tol": Case(README.replace(param_tol=1e-3, fn_tol=1e-12), "parity", PARAMETER_TOL,
                      frozenset({PARAMETER_TOL, MAX_ITERATIONS})),
    # seed 910 has 5 firm scenes by GRADIENT_TOL at N = 4; 912 has 14 (N = 4) and 9 (N = 8)
    "gradient_tol": Case(README.replace(gradient_tol=0.1, fn_tol=1e-12), "parity", GRADIENT_TOL,
                         frozenset({GRADIENT_TOL, PARAMETER_TOL, MAX_ITERATIONS}), seed=912),
    "zero_gradient": Case(README.replace(**ZERO), "exact", GRADIENT_TOL, frozenset({GRADIENT_TOL})),
    "invalid_steps": Case(README.replace(fixed_iterations=1, **ZERO), "exact", INVALID_STEPS, frozenset({INVALID_STEPS})),
    "pinned_box": Case(README.replace(**PIN), "exact", GRADIENT_TOL, frozenset({GRADIENT_TOL}), B=32),
    "pinned_box_fixed": Case(README.replace(fixed_iterations=1, **PIN), "invariants", MIN_RADIUS,
                             frozenset({MIN_RADIUS, MAX_ITERATIONS}), B=32),
    "successful_step_rule": Case(README, "parity", FUNCTION_TOL, frozenset({FUNCTION_TOL, MAX_ITERATIONS}), warm=True,
                                 alt=README.replace(tol_needs_successful_step=1)),
}
PARITY = [n for n, c in CASES.items() if c.kind == "parity"]
EXACT = [n for n, c in CASES.items() if c.kind == "exact"]
# What the oracle alone must show of a parity case, on each N (tests/test_lm_exits.py asserts it): the share of firm
# scenes and the firm scenes that end by the case's exit
FIRM_SHARE, NAMED_SCENES = 0.8, 8
# successful_step_rule, per N: the scenes firm under both flags whose iteration count the flag changes (the oracle has 27
# and 31), and the firm scenes flag 0 stops in their first iteration (20 and 22). Floors a third below what the oracle
# has: what the device must reproduce is that the flag decides on a large share of the scenes, not the oracle's count on
# one libm
FLAG_CHANGES, FIRST_ITERATION_STOPS = {4: 18, 8: 20}, {4: 13, 8: 14}

_cache = {}


def scenes_of(name, N):
    """The case's scenes with N agents (computed once per session)."""
    key = ("scenes", name, N)
    if key not in _cache:
        c = CASES[name]
        sc = make_scenes(c.prm, c.B, N, map_cells=MAP_CELLS, seed=c.seed)
        assert sc.T == T and sc.init_params.shape[1] == P
        if c.warm:
            from oracle import oracle_py as oracle
            cold = oracle.solve(README, sc, nthreads=16, theta_zero_convention=True)
            sc.init_params = np.ascontiguousarray(cold["params"])
        _cache[key] = sc
    return _cache[key]


def params_of(name, alt=False):
    return CASES[name].alt if alt else CASES[name].prm


def oracle_of(name, N, alt=False):
    """(result of the oracle under the theta := 0 convention, firm scenes): firm as parity_checks.check_solve has it,
    marginal_decisions == 0 and conftest.well_conditioned(samples=2). Computed once per session and left unchanged."""
    key = ("oracle", name, N, alt)
    if key not in _cache:
        from oracle import oracle_py as oracle
        prm, sc = params_of(name, alt), scenes_of(name, N)
        rz = oracle.solve(prm, sc, nthreads=16, theta_zero_convention=True)
        stable = well_conditioned(oracle, prm, sc, rz, nthreads=16, theta_zero_convention=True, samples=2)
        _cache[key] = (rz, (rz["marginal_decisions"] == 0) & stable)
    return _cache[key]


def oracle_trace(name, N, b, alt=False):
    """The oracle's rows of scene b under the device's theta convention."""
    key = ("trace", name, N, alt, b)
    if key not in _cache:
        from oracle import oracle_py as oracle
        prm = params_of(name, alt)
        oracle.set_theta_zero_convention(True)
        try:
            _cache[key] = oracle.trace(prm, scenes_of(name, N), b, max_rows=prm.max_iterations + 2)
        finally:
            oracle.set_theta_zero_convention(False)
    return _cache[key]


def projected_start(name, N):
    """Plus(x, 0) of the case's scenes: init_params clipped into the box (all three blocks of T = 28 are bounded)."""
    prm, sc = CASES[name].prm, scenes_of(name, N)
    return np.clip(sc.init_params, [prm.v_min, prm.w_min] * (P // 2), [prm.v_max, prm.w_max] * (P // 2))
