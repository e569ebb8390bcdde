"""Every solve and K1 instantiation the library compiles (pick() in csrc/smpc_sweep_host.hpp: parameter blocks NB = 1..10 x
slot width W = 32 / 64 x plain / per-scene horizon `vt` / per-scene weights and bounds `sp` x solve / K1), each launched
on a shape of its own and checked against the CPU oracle, plus the identities between the variants that do not depend
on the conditioning of a scene. The case table names the W each case takes; test_the_table_names_every_instantiation
(no GPU) checks that the table reaches every instantiation."""
import itertools
import os
import re
from typing import NamedTuple, Optional

import numpy as np
import pytest

from conftest import cmd_err, well_conditioned
from parity_checks import CMD_TOL, add_counts, check_population, check_solve
from nav2_social_mpc_controller_amd.params import OptimizerParams, scene_param_rows
from nav2_social_mpc_controller_amd.scenes import make_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
README = OptimizerParams.readme()
JAC_RTOL = 1e-9     # K1 rows vs the dual-number oracle, relative to max(1, |value|) (test_gpu_parity)
RESULT_KEYS = ("params", "cmds", "path", "status", "reason", "iterations", "evaluations", "initial_cost", "final_cost")
EVAL_KEYS = ("residuals", "jacobian", "cost", "gradient")
VARIANTS = ("plain", "vt", "sp")


class Case(NamedTuple):
    ch: int                       # control_horizon
    bl: int                       # parameter_block_length
    T: int
    N: int
    B: int
    W: int                        # slot width of the solve (and of K1: slot_width(T, N))
    seed: int
    n_valid: Optional[int] = None  # agents n_valid..N-1 invalid
    no_people: int = 0            # every no_people-th scene has has_people = 0

    @property
    def prm(self):
        return README.replace(control_horizon=self.ch, parameter_block_length=self.bl)


# One case per (NB, W). W = 32: T <= 31 and N <= 32, the solve forced to two scenes per wave (the batches are small);
# W = 64: T >= 32 or N >= 33, one scene per wave whatever the batch size. Per NB one case has bl dividing CH and one has
# an unbounded last block (NB = 1 has no such shape: one block is always the whole horizon).
CASES = {
    "nb1_w32": Case(4, 6, 28, 5, 24, 32, 1701, n_valid=3),
    "nb1_w64": Case(5, 5, 40, 3, 16, 64, 1702, no_people=5),
    "nb2_w32": Case(10, 5, 31, 8, 32, 32, 1703, no_people=7),
    "nb2_w64": Case(11, 6, 38, 16, 16, 64, 1704, n_valid=12),
    "nb3_w32": Case(17, 6, 28, 4, 32, 32, 1705),
    "nb3_w64": Case(18, 6, 30, 40, 16, 64, 1706, n_valid=35),
    "nb4_w32": Case(20, 5, 31, 3, 32, 32, 1707, n_valid=2, no_people=6),
    "nb4_w64": Case(15, 4, 36, 8, 24, 64, 1708),
    "nb5_w32": Case(18, 4, 28, 6, 32, 32, 1709, no_people=8),
    "nb5_w64": Case(20, 4, 38, 3, 24, 64, 1710, n_valid=2),
    "nb6_w32": Case(18, 3, 31, 16, 24, 32, 1711, n_valid=13),
    "nb6_w64": Case(23, 4, 33, 3, 24, 64, 1712, no_people=4),
    "nb7_w32": Case(20, 3, 28, 5, 32, 32, 1713, no_people=9),
    "nb7_w64": Case(21, 3, 44, 16, 16, 64, 1714),
    "nb8_w32": Case(24, 3, 31, 4, 32, 32, 1715, n_valid=3),
    "nb8_w64": Case(30, 4, 38, 8, 24, 64, 1716, no_people=6),
    "nb9_w32": Case(26, 3, 28, 3, 32, 32, 1717),
    "nb9_w64": Case(27, 3, 29, 36, 16, 64, 1718, n_valid=30, no_people=5),
    "nb10_w32": Case(30, 3, 31, 5, 32, 32, 1719, no_people=6),
    "nb10_w64": Case(28, 3, 40, 3, 24, 64, 1720, n_valid=2),
}


def slot_width(T, N):
    """K1's slot width (smpc::slot_width): two scenes per wave when the poses and the agents fit half a wave."""
    return 32 if T + 1 <= 32 and N <= 32 else 64


def helper_owner_agents(T, N, W):
    """smpc::helper_owner_agents: the agents an owner lane walks itself (N: no helper lanes)."""
    R = W - T
    if W != 64 or R < 1 or N < 2:
        return N
    U = (T + R - 1) // R
    A = (U * N + U) // (U + 1)
    if A >= N:
        return N
    return A if (N - A) * 250 > 2 * (60 * U + 120) else N


def other_params(prm):
    """The second parameter set of the sp launches: other weights, another target speed, bounds that bite."""
    return prm.replace(distance_weight=35.0, social_weight=300.0, velocity_weight=6.0, angle_weight=150.0,
                       agent_angle_weight=20.0, proxemics_weight=60.0, velocity_feasibility_weight=8.0,
                       goal_align_weight=4.0, obstacle_weight=0.25, desired_linear_vel=0.3, v_max=0.35, w_max=0.6)


def horizons(B, T, seed):
    """every T_b of 1..T when B allows (the rest random), else B values spread over 1..T with 1 and T among them"""
    g = np.random.default_rng(seed)
    if B >= T:
        Ts = np.concatenate([np.arange(1, T + 1), g.integers(1, T + 1, size=B - T)])
    else:
        Ts = np.round(np.linspace(1, T, B)).astype(np.int64)
    g.shuffle(Ts)
    return Ts.astype(np.int32)


def scenes_of(c, B=None):
    sc = make_scenes(c.prm, c.B if B is None else B, c.N, T=c.T, seed=c.seed, map_cells=120, n_valid=c.n_valid)
    if c.no_people:
        sc.has_people[::c.no_people] = 0
    return sc


def planned_launches():
    """(kind, NB, W, variant) of every launch the table makes: the solve at the case's W, K1 at slot_width(T, N)."""
    out = set()
    for c in CASES.values():
        nb = c.prm.dims(c.T)[2]
        for v in VARIANTS:
            out.add(("solve", nb, c.W, v))
            out.add(("eval", nb, slot_width(c.T, c.N), v))
    return out


def test_the_table_names_every_instantiation():
    src = open(os.path.join(ROOT, "include", "smpc.h")).read()
    max_blocks = int(re.search(r"#define SMPC_MAX_BLOCKS (\d+)", src).group(1))
    # the variants pick() selects among: plain and one per flag of pick_w() after `kind`
    hip = open(os.path.join(ROOT, "nav2_social_mpc_controller_amd", "csrc", "smpc_sweep_host.hpp")).read()
    flags = re.search(r"KernelFn pick_w\(int W, Sweep kind, ([^)]*)\)", hip).group(1)
    assert ("plain",) + tuple(f.split()[-1] for f in flags.split(",")) == VARIANTS
    want = set(itertools.product(("solve", "eval"), range(1, max_blocks + 1), (32, 64), VARIANTS))
    assert planned_launches() == want
    for name, c in CASES.items():
        # K1 runs at the case's W, and a W = 64 solve needs no knob; W = 32 shapes are the two-slot ones
        assert slot_width(c.T, c.N) == c.W, name
        assert 16 <= c.B <= 32, name
    # both two-slot horizons, and at least one unbounded last block per NB > 1
    assert {c.T for c in CASES.values() if c.W == 32} >= {28, 31}
    for nb in range(2, max_blocks + 1):
        assert any(c.prm.dims(c.T)[2] == nb and min(c.ch, c.T) % min(c.bl, c.ch, c.T) for c in CASES.values()), nb


# ---------------------------------------------------------------------------------------------------------------------
# GPU


@pytest.fixture(scope="module")
def Solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    return BatchSolver


def solver_for(Solver, c, monkeypatch):
    if c.W == 32:
        monkeypatch.setenv("SMPC_SOLVE_WIDTH", "32")
    s = Solver(c.prm)
    assert s.solve_slot_width(c.B, c.T, c.N) == c.W
    return s


def same(a, b, keys, where=slice(None), what=""):
    for k in keys:
        x, y = np.asarray(a[k])[where], np.asarray(b[k])[where]
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)


def subset(r, idx):
    return {k: v[idx] for k, v in r.items()}


def oracle_view(sc, idx):
    """scenes idx as the oracle takes them (it knows nothing of scene_params: the group's own params are passed)"""
    sub = sc.select(idx)
    sub.scene_params = None
    return sub


def sp_batch(c, sc):
    """sc with the case's parameter set on the even scenes and other_params() on the odd ones"""
    which = np.arange(sc.B) % 2
    groups = [(c.prm, np.where(which == 0)[0]), (other_params(c.prm), np.where(which == 1)[0])]
    return sc.with_scene_params(scene_param_rows([c.prm, other_params(c.prm)], which)), groups


def critic_major_rows(prm, T, Tb, has_people):
    """rows[r]: the critic-major row (smpc_eval_batch_out.row_order = 1) of reference row r of a scene with Tb of the
    batch's T steps: critic c of step t at c * T + t, feasibility row q at rps * T + q."""
    rps = 8 if has_people else 5
    M_b = prm.dims(Tb, has_people)[4]
    nfeas = M_b - rps * Tb
    rows = np.empty(M_b, np.int64)
    for t in range(Tb):
        base = rps * t + min(max(t - 1, 0), nfeas)
        for k in range(rps):
            rows[base + k] = k * T + t
        if 1 <= t <= nfeas:
            rows[base + rps] = rps * T + (t - 1)
    return rows


def check_k1(s, groups, sc, x):
    """K1 at x in both row orders: the reference order against the oracle (each group of scenes under its own params),
    the critic-major order as the reference rows permuted, bit for bit. Returns the worst relative Jacobian error."""
    from oracle import oracle_py as oracle
    eg = s.evaluate(sc, x, row_order=0)
    worst = 0.0
    for prm, idx in groups:
        eo = oracle.evaluate(prm, oracle_view(sc, idx), x[idx])
        for key, tol in (("residuals", JAC_RTOL), ("jacobian", JAC_RTOL), ("gradient", 1e-8)):
            err = np.abs(eo[key] - eg[key][idx]) / np.maximum(1.0, np.abs(eo[key]))
            assert np.max(err) < tol, (key, float(np.max(err)), np.unravel_index(np.argmax(err), err.shape))
            if key == "jacobian":
                worst = max(worst, float(np.max(err)))
        assert np.max(np.abs(eo["cost"] - eg["cost"][idx]) / np.maximum(1.0, eo["cost"])) < 1e-11
    ec = s.evaluate(sc, x, row_order=1)
    assert np.array_equal(eg["cost"], ec["cost"]) and np.array_equal(eg["gradient"], ec["gradient"])
    prm = groups[0][0]
    for b in range(sc.B):
        Tb = sc.T if sc.T_scene is None else int(sc.T_scene[b])
        hp = bool(sc.has_people[b]) and sc.N > 0
        rows = critic_major_rows(prm, sc.T, Tb, hp)
        if Tb == sc.T:
            assert np.array_equal(rows, s.row_permutation(sc.T, hp))
        for key in ("residuals", "jacobian"):
            assert np.array_equal(ec[key][b][rows], eg[key][b][:len(rows)]), (key, b)
            rest = np.ones(ec[key].shape[1], bool)
            rest[rows] = False
            assert not ec[key][b][rest].any() and not eg[key][b][len(rows):].any(), (key, b)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_k1_matches_oracle(Solver, name, monkeypatch):
    c = CASES[name]
    s = solver_for(Solver, c, monkeypatch)
    sc = scenes_of(c)
    rng = np.random.default_rng(3)
    dx = 0.05 * rng.standard_normal(sc.init_params.shape)
    worst = {}
    # plain
    worst["plain"] = max(check_k1(s, [(c.prm, np.arange(sc.B))], sc, x) for x in (sc.init_params, sc.init_params + dx))
    # vt: a batch large enough that every horizon 1..T occurs
    big = scenes_of(c, B=max(c.B, c.T))
    sv = big.with_horizons(horizons(big.B, c.T, c.seed))
    assert set(sv.T_scene) == set(range(1, c.T + 1))
    dxv = 0.05 * rng.standard_normal(sv.init_params.shape)
    worst["vt"] = max(check_k1(s, [(c.prm, np.arange(sv.B))], sv, x) for x in (sv.init_params, sv.init_params + dxv))
    # sp: two parameter sets, alternately
    ssp, groups = sp_batch(c, sc)
    worst["sp"] = max(check_k1(s, groups, ssp, x) for x in (sc.init_params, sc.init_params + dx))
    print(f"\n[k1] {name} NB={c.prm.dims(c.T)[2]} W={c.W}: worst rel |dJ| " +
          " ".join(f"{k}={v:.2e}" for k, v in worst.items()))


POPULATION = {}  # the check_solve() counts of each case's launches, for test_set_aside_scenes_are_few_over_the_table


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_solve_matches_oracle(Solver, name, monkeypatch):
    c = CASES[name]
    s = solver_for(Solver, c, monkeypatch)
    prm = c.prm
    sc = scenes_of(c)
    counts, worst = None, {}

    def check(v, p, scenes, result):
        nonlocal counts
        n, e = check_solve(p, scenes, result)
        counts = add_counts(counts, n)
        worst[v] = max(worst.get(v, 0.0), e)

    check("plain", prm, sc, s.solve(sc))
    # vt
    sv = sc.with_horizons(horizons(sc.B, c.T, c.seed + 1))
    rv = s.solve(sv)
    check("vt", prm, sv, rv)
    for b in range(sc.B):  # nothing behind a scene's own horizon / parameter count
        Tb = int(sv.T_scene[b])
        assert not rv["cmds"][b, Tb + 1:].any() and not rv["path"][b, Tb + 1:].any()
        assert not rv["params"][b, prm.dims(Tb, True)[3]:].any()
    # sp: each group against the oracle under its own parameter set
    ssp, groups = sp_batch(c, sc)
    rs = s.solve(ssp)
    for p, idx in groups:
        check("sp", p, oracle_view(ssp, idx), subset(rs, idx))
    # the tight bounds hold and bite: the case's own set goes beyond them, the other one sits on them
    nbnd = prm.dims(c.T)[5]
    tight = groups[1][0]
    v0 = rs["params"][groups[0][1], 0:2 * nbnd:2]
    v1, w1 = rs["params"][groups[1][1], 0:2 * nbnd:2], rs["params"][groups[1][1], 1:2 * nbnd:2]
    assert v1.max() <= tight.v_max and w1.max() <= tight.w_max and v1.min() >= tight.v_min and w1.min() >= tight.w_min
    assert v0.max() > tight.v_max and (v1 == tight.v_max).any()
    POPULATION[name] = counts
    print(f"\n[solve] {name} NB={prm.dims(c.T)[2]} W={c.W}: worst firm |dcmd| " +
          " ".join(f"{k}={v:.2e}" for k, v in worst.items()) +
          f"; set aside {counts['scenes'] - counts['firm']}/{counts['scenes']}")


@pytest.mark.gpu
def test_set_aside_scenes_are_few_over_the_table():
    """check_population() over every solve of test_solve_matches_oracle: the launches of one case are too small for a
    share of scenes to mean anything, the table's 1512 are not."""
    if set(POPULATION) != set(CASES):
        pytest.skip("needs test_solve_matches_oracle of every case in the same run")
    total = None
    for n in POPULATION.values():
        total = add_counts(total, n)
    print(f"\n[population] {total['scenes']} scenes: {total['stable']} well conditioned, {total['firm']} firm, "
          f"{total['moved']} moved, {total['clean']} of {total['noise_free']} clean")
    check_population(total)


def same_lm_path(a, b, what, N):
    """the rule of test_slot_widths_agree where the sums over the agents are split differently (its median bound was
    taken at N = 8; the rounding of a sum over N agents grows with N)"""
    one = (a["iterations"] == b["iterations"]) & (a["evaluations"] == b["evaluations"])
    assert one.mean() >= 0.98, (what, np.where(~one)[0])
    d = cmd_err(a["cmds"], b["cmds"])
    assert np.median(d) <= 1e-13 * max(1.0, N / 8) and np.max(d[one]) <= 1e-6, (what, float(np.median(d)), float(np.max(d[one])))
    assert np.array_equal(a["status"], b["status"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_identities(Solver, oracle, name, monkeypatch):
    c = CASES[name]
    s = solver_for(Solver, c, monkeypatch)
    prm = c.prm
    NB = prm.dims(c.T)[2]
    sc = scenes_of(c)
    plain = s.solve(sc)
    # vt with every T_scene == T: the plain solve bit for bit; K1 within its parity bound (test_neutral_rows_are_invisible)
    full = sc.with_horizons(np.full(sc.B, c.T, np.int32))
    same(plain, s.solve(full), RESULT_KEYS, what="vt full")
    # sp with neutral rows: the plain solve bit for bit, and the vt K1 bit for bit
    neutral = sc.with_scene_params(scene_param_rows([prm], np.zeros(sc.B, int)))
    same(plain, s.solve(neutral), RESULT_KEYS, what="sp neutral")
    x = sc.init_params + 0.02 * np.random.default_rng(5).standard_normal(sc.init_params.shape)
    for row_order in (0, 1):
        ev = s.evaluate(full, x, row_order=row_order)
        same(ev, s.evaluate(neutral, x, row_order=row_order), EVAL_KEYS, what=("sp K1", row_order))
        e0 = s.evaluate(sc, x, row_order=row_order)
        for k in EVAL_KEYS:
            assert np.all(np.abs(e0[k] - ev[k]) <= JAC_RTOL * np.maximum(1.0, np.abs(e0[k]))), (k, row_order)
    # a short scene inside a long batch against the batch of its own horizon: bit for bit with the same instantiation
    # and the same split of the agent sums, otherwise the same iteration path
    Ts = horizons(sc.B, c.T, c.seed + 2)
    sv = sc.with_horizons(Ts)
    rv = s.solve(sv)
    A = helper_owner_agents(c.T, c.N, c.W)
    for Tb in sorted(set(Ts.tolist()) - {c.T}):
        idx = np.where(Ts == Tb)[0]
        nb_b, P_b = prm.dims(Tb, True)[2:4]
        W_b = s.solve_slot_width(len(idx), Tb, c.N)
        alone_in = sv.cut(idx, Tb, P_b)
        alone = s.solve(alone_in)
        mine = {k: rv[k][idx] for k in RESULT_KEYS}
        mine["params"], mine["cmds"], mine["path"] = rv["params"][idx][:, :P_b], rv["cmds"][idx][:, :Tb + 1], rv["path"][idx][:, :Tb + 1]
        assert np.array_equal(alone["iterations"], mine["iterations"]), Tb
        assert np.array_equal(alone["status"], mine["status"]), Tb
        if helper_owner_agents(Tb, c.N, W_b) == A and nb_b == NB:
            same(alone, mine, ("params", "cmds", "path", "final_cost"), what=("short scene", Tb))
            continue
        # another instantiation, whose fused multiply-adds may differ in the last bit, or the agent sums split otherwise
        # between owner and helper lanes: the same iteration path; the values agree on every scene that does not
        # amplify one ulp of its input (the oracle's well_conditioned(): e.g. an unbounded last block of one step)
        ok = well_conditioned(oracle, prm, alone_in, oracle.solve(prm, alone_in, nthreads=16), nthreads=16)
        if helper_owner_agents(Tb, c.N, W_b) != A:
            assert np.array_equal(alone["evaluations"], mine["evaluations"]), Tb
            assert np.max(cmd_err(alone["cmds"], mine["cmds"])[ok], initial=0.0) <= 1e-6, (Tb, ok)
        else:
            assert np.max(np.abs(alone["params"] - mine["params"])[ok], initial=0.0) <= 1e-9, (Tb, ok)
            assert np.allclose(alone["final_cost"][ok], mine["final_cost"][ok], rtol=1e-10), Tb
    # W = 32 against W = 64 on the same scenes: bit for bit without helper lanes, the same LM path with them
    if c.W == 32:
        ssp, _ = sp_batch(c, sc)
        w32 = {"plain": plain, "vt": rv, "sp": s.solve(ssp)}
        monkeypatch.setenv("SMPC_SOLVE_WIDTH", "64")
        assert s.solve_slot_width(c.B, c.T, c.N) == 64
        w64 = {"plain": s.solve(sc), "vt": s.solve(sv), "sp": s.solve(ssp)}
        for v in VARIANTS:
            if helper_owner_agents(c.T, c.N, 64) == c.N:
                same(w32[v], w64[v], RESULT_KEYS, what=("W", v))
            else:
                same_lm_path(w32[v], w64[v], ("W", v), c.N)


# ---------------------------------------------------------------------------------------------------------------------
# two launches at the size users run them (no knob: the library picks W = 32 itself)

FULL_SIZE = {
    # the README shape with a horizon per scene: the closed-loop kernel <3, 32, vt>
    "readme_vt_b4096": (README, dict(B=4096, N=8, seed=0x5EED0002), True),
    # ten blocks (P = 20) on the last two-slot horizon
    "nb10_t31_b2048": (README.replace(control_horizon=30, parameter_block_length=3),
                       dict(B=2048, N=3, T=31, seed=0x5EED0003), False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FULL_SIZE))
def test_full_size(Solver, oracle, name):
    prm, kw, vt = FULL_SIZE[name]
    sc = make_scenes(prm, **kw)
    B, T = sc.B, sc.T
    if vt:
        sc = sc.with_horizons(horizons(B, T, 13))
    s = Solver(prm)
    assert s.solve_slot_width(B, T, sc.N) == 32
    a = s.solve(sc)
    b = s.solve(sc)
    for k in a:
        assert np.array_equal(a[k], b[k]), f"non-deterministic output {k}"
    assert np.all(a["status"] != 2)
    assert np.all(a["final_cost"] <= a["initial_cost"] * (1 + 1e-12))
    assert np.all((a["iterations"] >= 0) & (a["iterations"] <= prm.max_iterations))
    Ts = sc.T_scene if vt else np.full(B, T, np.int32)
    x0 = np.zeros_like(sc.init_params)
    for Tb in sorted(set(Ts.tolist())):
        idx = np.where(Ts == Tb)[0]
        CH, bl, nb, P, M, nbnd = prm.dims(Tb)
        p = a["params"][idx]
        v, w = p[:, 0:2 * nbnd:2], p[:, 1:2 * nbnd:2]      # the bounded blocks (src/optimizer.cpp:373-379)
        assert v.min() >= prm.v_min and v.max() <= prm.v_max and w.min() >= prm.w_min and w.max() <= prm.w_max, Tb
        for i in range(Tb + 1):                                                         # a12 expansion
            blk = i // bl if i < CH else (CH - 1) // bl
            assert np.array_equal(a["cmds"][idx, i, 0], p[:, 2 * blk]), (Tb, i)
            assert np.array_equal(a["cmds"][idx, i, 1], p[:, 2 * blk + 1]), (Tb, i)
        assert not a["cmds"][idx, Tb + 1:].any() and not p[:, P:].any(), Tb
        x0[idx, :P] = np.clip(sc.init_params[idx, :P], [prm.v_min, prm.w_min] * nbnd + [-np.inf, -np.inf] * (nb - nbnd),
                              [prm.v_max, prm.w_max] * nbnd + [np.inf, np.inf] * (nb - nbnd))
    # initial cost reported by the solve == cost of the K1 sweep at the projected start point
    pick = np.arange(0, B, max(1, B // 512))
    ev = s.evaluate(sc.select(pick), x0[pick])
    assert np.allclose(ev["cost"], a["initial_cost"][pick], rtol=1e-12)
    # the oracle on a sample: every firm, well-conditioned scene within the tolerance, same status and iteration count
    sample = 256
    sub = sc.select(np.arange(sample))
    rz = oracle.solve(prm, sub, nthreads=16, theta_zero_convention=True)
    stable = well_conditioned(oracle, prm, sub, rz, nthreads=16, theta_zero_convention=True)
    firm = (rz["marginal_decisions"] == 0) & stable
    assert stable.mean() >= 0.97 and firm.mean() >= 0.9, (float(stable.mean()), float(firm.mean()))
    err = cmd_err(a["cmds"][:sample], rz["cmds"])
    assert np.max(err[firm]) <= CMD_TOL, float(np.max(err[firm]))
    assert np.array_equal(a["status"][:sample][firm], rz["status"][firm])
    assert np.array_equal(a["iterations"][:sample][firm], rz["iterations"][firm])
    moved = ~firm & (err > CMD_TOL)
    assert moved.mean() <= 0.03
    if moved.any():
        worse = (a["final_cost"][:sample][moved] - rz["final_cost"][moved]) / rz["final_cost"][moved]
        assert np.all(worse <= 10 * prm.fn_tol), worse
    print(f"\n[full size] {name}: worst firm |dcmd| {np.max(err[firm]):.2e} over {firm.sum()}/{sample} firm scenes")
