"""GPU parity tests proper (`-m gpu`): every call goes through the C ABI (libsmpc_hip.so); the CPU oracle and
the committed golden fixtures are the checkers. Tolerance: max |delta cmd| <= 1e-5 on the optimised command
sequence (BASELINE.json north_star), everything f64.

One documented convention: the reference's social force takes sign(theta) (critics/social_work_cost_function.hpp:210)
of theta = atan2(dir) - atan2(interaction dir). When the two velocities are EXACTLY equal (robot command clamped to
v = 0 beside a standing person) theta is mathematically 0 and the reference's value is its libm's last-bit noise, so
its sign — hence the solve — is not reproducible even between two builds of the reference. The HIP path takes
theta := 0 there. The oracle can be run reference-literal (default) or with that convention; it also counts the
evaluations where the noise decided (`sign_noise_events`) and the LM decisions (Armijo, function tolerance, accept)
taken with a margin below 1e-12 of the cost, i.e. inside the rounding noise of summing the squared residuals in a
different order (`marginal_decisions`). Tests compare every firm-decision scene against the
convention oracle, and the literal oracle on every scene it flagged for neither."""
import numpy as np
import pytest

from conftest import GOLDEN_CASES, cmd_err, load_golden, well_conditioned, yaw_err
from parity_checks import check_population, check_solve
from nav2_social_mpc_controller_amd.params import OptimizerParams
from nav2_social_mpc_controller_amd.scenes import make_scenes

pytestmark = pytest.mark.gpu

CMD_TOL = 1e-5      # north_star: outputs match the reference solve within 1e-5 on the optimised command sequence
JAC_RTOL = 1e-9     # K1 rows vs the dual-number oracle, relative to max(1, |value|)


@pytest.fixture(scope="module")
def Solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    return BatchSolver


README = OptimizerParams.readme()
EVAL_CASES = {
    "ref_n3_phantom": (README, dict(B=64, N=3, n_valid=2, map_cells=80, seed=101)),
    "cfg2_n4": (README, dict(B=64, N=4, seed=102)),
    "cfg3_n8": (README, dict(B=64, N=8, seed=103)),
    "cfg5_n16_h30": (README.replace(control_horizon=30, max_time=2.0), dict(B=32, N=16, seed=104)),
    "params_yaml_n3": (OptimizerParams.params_yaml(), dict(B=32, N=3, seed=105)),
    "cfg1_nopeople": (OptimizerParams.params_yaml().replace(control_horizon=18, linear_solver_type="DENSE_QR"),
                      dict(B=32, N=3, seed=106, people_present=False)),
    "quirk_bl_not_dividing_ch": (README.replace(time_step=0.1), dict(B=32, N=3, seed=107)),
    "all_agents_invalid": (README, dict(B=16, N=3, n_valid=0, seed=108)),
    "single_block": (README.replace(control_horizon=4, parameter_block_length=6), dict(B=16, N=5, seed=109)),
    # T=28 (two scenes per wave) with 5 parameter blocks: [J r] has 11 columns (66 Gram entries, five reduction chunks)
    "w32_five_blocks_valu_gram": (README.replace(parameter_block_length=4), dict(B=32, N=6, seed=110)),
    "six_blocks": (README.replace(parameter_block_length=3), dict(B=16, N=4, seed=111)),
    # up to SMPC_MAX_BLOCKS = 10 parameter blocks (P = 20): control_horizon 30 over T = 38
    "eight_blocks": (README.replace(control_horizon=30, parameter_block_length=4, max_time=2.0), dict(B=8, N=4, seed=118)),
    "ten_blocks": (README.replace(control_horizon=30, parameter_block_length=3, max_time=2.0), dict(B=8, N=4, seed=119)),
    # the largest supported shape: T = 63 rollout steps (max_time 3.25 s), 64 agents (K1 stages 129 KB of people in LDS)
    "max_T63_N64": (README.replace(max_time=3.25), dict(B=4, N=64, seed=112, map_cells=120)),
    "n33_needs_wide_slot": (README, dict(B=6, N=33, seed=113, map_cells=120)),
    # slot-width boundaries: T + 1 = 32 poses and N = 32 agents still share a wave between two scenes, one more does not
    "t31_last_two_slot_shape": (README.replace(max_time=1.65), dict(B=6, N=5, seed=114, map_cells=100)),
    "t32_first_one_slot_shape": (README.replace(max_time=1.70), dict(B=6, N=5, seed=115, map_cells=100)),
    "n32_last_two_slot_shape": (README, dict(B=6, N=32, seed=116, map_cells=120)),
    "t1_shortest_horizon": (README, dict(B=6, N=3, T=1, seed=117, map_cells=80)),
    # the reference's shipped benchmark parameter sets (params/*_in_benchmark.yaml:104-149): 80 x 80 local costmap, three
    # agents; obst_only: people present, social_weight = agent_angle_weight = 0 (rows exist, all zero)
    "soc_work_obst_benchmark": (OptimizerParams.soc_work_obst_benchmark(), dict(B=64, N=3, n_valid=2, map_cells=80, seed=120)),
    "obst_only_benchmark": (OptimizerParams.obst_only_benchmark(), dict(B=64, N=3, map_cells=80, seed=121)),
}


@pytest.mark.parametrize("name", list(EVAL_CASES))
def test_k1_rows_match_oracle(Solver, oracle, name):
    prm, kw = EVAL_CASES[name]
    sc = make_scenes(prm, **kw)
    s = Solver(prm)
    rng = np.random.default_rng(3)
    for x in (sc.init_params, sc.init_params + 0.05 * rng.standard_normal(sc.init_params.shape)):
        eo = oracle.evaluate(prm, sc, x)
        eg = s.evaluate(sc, x)
        if name == "all_agents_invalid":
            # No valid agent: the reference's dual-number proxemics row has NaN tangents (-max/d0^2 = -inf, inf*0),
            # which makes Ceres reject the evaluation. Both sides must flag the same rows; finite entries must agree.
            bad_o = ~np.isfinite(eo["jacobian"]).all(axis=2)
            bad_g = ~np.isfinite(eg["jacobian"]).all(axis=2)
            assert bad_o.any() and np.array_equal(bad_o, bad_g)
            for key in ("residuals", "jacobian"):
                m = np.isfinite(eo[key]) & np.isfinite(eg[key])
                assert np.max(np.abs(eo[key][m] - eg[key][m]) / np.maximum(1.0, np.abs(eo[key][m]))) < JAC_RTOL
            continue
        for key, tol in (("residuals", JAC_RTOL), ("jacobian", JAC_RTOL), ("gradient", 1e-8)):
            err = np.abs(eo[key] - eg[key]) / np.maximum(1.0, np.abs(eo[key]))
            assert np.max(err) < tol, (key, float(np.max(err)))
        assert np.max(np.abs(eo["cost"] - eg["cost"]) / np.maximum(1.0, eo["cost"])) < 1e-11


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_solve_matches_committed_golden(Solver, name):
    prm, sc, exp = load_golden(name)
    res = Solver(prm).solve(sc)
    # the oracle under the theta := 0 convention (see module docstring), on every scene whose LM decisions were firm
    firm = exp["oraclez_marginal_decisions"] == 0
    assert firm.sum() >= len(firm) - 1      # the fixtures hold 2..4 scenes; cfg3_n8 has one marginal scene
    assert np.max(cmd_err(res["cmds"][firm], exp["oraclez_cmds"][firm])) <= CMD_TOL
    assert np.max(np.abs(res["params"][firm] - exp["oraclez_params"][firm])) <= CMD_TOL
    assert res["status"][firm].tolist() == exp["oraclez_status"][firm].tolist()
    assert res["iterations"][firm].tolist() == exp["oraclez_iterations"][firm].tolist()
    assert np.max(np.abs(res["path"][firm][:, :, :2] - exp["oraclez_path"][firm][:, :, :2])) <= 1e-5
    assert np.max(yaw_err(res["path"][firm][:, :, 2], exp["oraclez_path"][firm][:, :, 2])) <= 1e-5
    assert np.allclose(res["final_cost"][firm], exp["oraclez_final_cost"][firm], rtol=1e-8)
    # the reference-literal oracle on every scene whose sign(theta) never hung on libm noise
    clean = (exp["oracle_sign_noise_events"] == 0) & (exp["oracle_marginal_decisions"] == 0)
    assert np.max(cmd_err(res["cmds"][clean], exp["oracle_cmds"][clean]), initial=0.0) <= CMD_TOL
    # ... and the independent Python restatement's optimum (literal semantics) on its clean scenes
    n = exp["pyref_x"].shape[0]
    cl = clean[:n]
    assert np.max(np.abs(res["params"][:n][cl] - exp["pyref_x"][cl]), initial=0.0) <= CMD_TOL


SOLVE_CASES = {
    "ref_n3_phantom": (README, dict(B=256, N=3, n_valid=2, map_cells=80, seed=201)),
    "cfg2_n4": (README, dict(B=512, N=4, seed=202)),
    "cfg3_n8": (README, dict(B=512, N=8, seed=203)),
    "cfg5_n16_h30": (README.replace(control_horizon=30, max_time=2.0), dict(B=128, N=16, seed=204)),
    "params_yaml_n3": (OptimizerParams.params_yaml(), dict(B=128, N=3, seed=205)),
    "cfg1_nopeople_qr": (OptimizerParams.params_yaml().replace(control_horizon=18, linear_solver_type="DENSE_QR"),
                         dict(B=128, N=3, seed=206, people_present=False)),
    "quirk_bl_not_dividing_ch": (README.replace(time_step=0.1), dict(B=128, N=3, seed=207)),
    "single_block": (README.replace(control_horizon=4, parameter_block_length=6), dict(B=64, N=5, seed=209)),
    "w32_five_blocks_valu_gram": (README.replace(parameter_block_length=4), dict(B=128, N=6, seed=210)),
    "eight_blocks": (README.replace(control_horizon=30, parameter_block_length=4, max_time=2.0), dict(B=48, N=4, seed=218)),
    "ten_blocks": (README.replace(control_horizon=30, parameter_block_length=3, max_time=2.0), dict(B=48, N=4, seed=219)),
    "max_T63_N64": (README.replace(max_time=3.25), dict(B=24, N=64, seed=212, map_cells=120)),
    "t31_last_two_slot_shape": (README.replace(max_time=1.65), dict(B=48, N=5, seed=214, map_cells=100)),
    "t32_first_one_slot_shape": (README.replace(max_time=1.70), dict(B=48, N=5, seed=215, map_cells=100)),
    "n32_last_two_slot_shape": (README, dict(B=32, N=32, seed=216, map_cells=120, standing_fraction=0.0)),
    "soc_work_obst_benchmark": (OptimizerParams.soc_work_obst_benchmark(), dict(B=256, N=3, n_valid=2, map_cells=80, seed=220)),
    "obst_only_benchmark": (OptimizerParams.obst_only_benchmark(), dict(B=256, N=3, map_cells=80, seed=221)),
}


@pytest.mark.parametrize("name", list(SOLVE_CASES))
def test_solve_matches_oracle_on_seeded_scenes(Solver, oracle, name):
    check_solve_case(Solver, oracle, name)


# Batches this small run one scene per wave (the W = 64 kernel, helper lanes from four people up: solve_slot_width() in
# csrc/smpc_plan.hpp); the two-scenes-per-wave kernel that the large batches of the same shapes take is put through the
# same cases here (SMPC_SOLVE_WIDTH is read at every launch), next to the full-size tests below.
TWO_SLOT_CASES = ["cfg2_n4", "cfg3_n8", "single_block", "w32_five_blocks_valu_gram", "t31_last_two_slot_shape",
                  "n32_last_two_slot_shape"]


@pytest.mark.parametrize("name", TWO_SLOT_CASES)
def test_solve_matches_oracle_two_scenes_per_wave(Solver, oracle, name, monkeypatch):
    monkeypatch.setenv("SMPC_SOLVE_WIDTH", "32")
    check_solve_case(Solver, oracle, name)


def test_slot_widths_agree(Solver, monkeypatch):
    """One scene per wave against two: bit-identical without helper lanes (three people: the same sums in the same
    order), the same LM path with them (eight people: the sums over the agents are split between owner and helper)."""
    for N, exact in ((3, True), (8, False)):
        sc = make_scenes(README, 256, N, seed=0x51D7 + N)
        res = {}
        for width in ("32", "64"):
            monkeypatch.setenv("SMPC_SOLVE_WIDTH", width)
            res[width] = Solver(README).solve(sc)
        a, b = res["32"], res["64"]
        if exact:
            for key in ("cmds", "path", "params", "final_cost", "iterations", "evaluations", "status"):
                assert np.array_equal(a[key], b[key]), key
        else:
            same = (a["iterations"] == b["iterations"]) & (a["evaluations"] == b["evaluations"])
            assert same.mean() >= 0.98
            d = cmd_err(a["cmds"], b["cmds"])
            assert np.median(d) <= 1e-13 and np.max(d[same]) <= 1e-6
            assert np.array_equal(a["status"], b["status"])


def check_solve_case(Solver, oracle, name):
    prm, kw = SOLVE_CASES[name]
    sc = make_scenes(prm, **kw)
    counts, _ = check_solve(prm, sc, Solver(prm).solve(sc))
    check_population(counts)


def test_moving_crowd_has_no_noisy_scene(Solver, oracle):
    """Without standing agents sign(theta) is never evaluated at theta == 0: the literal oracle flags nothing and
    every scene must agree."""
    sc = make_scenes(README, 512, 8, seed=301, standing_fraction=0.0)
    ro = oracle.solve(README, sc, nthreads=16)
    assert np.all(ro["sign_noise_events"] == 0)
    rg = Solver(README).solve(sc)
    firm = (ro["marginal_decisions"] == 0) & well_conditioned(oracle, README, sc, ro, nthreads=16)
    assert firm.mean() >= 0.93
    assert np.max(cmd_err(rg["cmds"][firm], ro["cmds"][firm])) <= CMD_TOL
    assert np.array_equal(rg["iterations"][firm], ro["iterations"][firm])


def test_full_size_moving_crowd_against_the_literal_oracle(Solver, oracle):
    """BASELINE config 3 at full size (B = 8192, N = 8) with nobody standing: the reference-literal oracle is defined on
    every scene (no sign(theta) at theta == 0), so the whole batch is compared with it — the population the 22 % of
    standing-person scenes of the headline workload are excluded from."""
    sc = make_scenes(README, 8192, 8, seed=0x5EED0001, standing_fraction=0.0)
    ro = oracle.solve(README, sc, nthreads=16)
    assert np.all(ro["sign_noise_events"] == 0)
    rg = Solver(README).solve(sc)
    firm = ro["marginal_decisions"] == 0
    err = cmd_err(rg["cmds"], ro["cmds"])
    over = err > CMD_TOL
    print(f"full-size literal comparison: firm {firm.mean():.4f}, scenes over 1e-5: {over.sum()} (firm: {(over & firm).sum()}), "
          f"max firm err {err[firm].max():.3e}")
    assert firm.mean() >= 0.93
    # firm scenes over the tolerance must be ill conditioned ones (the oracle itself moves under one ulp of input)
    bad = np.where(over & firm)[0]
    assert len(bad) <= 8
    if len(bad):
        sub = sc.select(bad)
        base = {"cmds": ro["cmds"][bad]}
        assert not well_conditioned(oracle, README, sub, base, nthreads=16).any()
    assert over.mean() <= 0.01
    assert np.array_equal(rg["iterations"][firm & ~over], ro["iterations"][firm & ~over])
    assert np.all(rg["status"] != 2)


def test_full_size_properties_cfg3(Solver):
    """BASELINE config 3 at full size (B=8192, N=8, 200x200 maps): size-independent properties."""
    prm = README
    sc = make_scenes(prm, 8192, 8, seed=0x5EED0001)
    s = Solver(prm)
    a = s.solve(sc)
    b = s.solve(sc)
    for k in a:
        assert np.array_equal(a[k], b[k]), f"non-deterministic output {k}"           # idempotent / deterministic
    CH, bl, nb, P, M, nbnd = prm.dims(sc.T)
    assert np.all(a["status"] != 2)
    assert np.all(a["final_cost"] <= a["initial_cost"] * (1 + 1e-12))
    assert np.all((a["iterations"] >= 0) & (a["iterations"] <= prm.max_iterations))
    v, w = a["params"][:, 0::2], a["params"][:, 1::2]
    assert v.min() >= prm.v_min and v.max() <= prm.v_max and w.min() >= prm.w_min and w.max() <= prm.w_max
    T = sc.T
    for i in range(T + 1):                                                              # a12 expansion
        blk = i // bl if i < CH else (CH - 1) // bl
        assert np.array_equal(a["cmds"][:, i, 0], a["params"][:, 2 * blk])
        assert np.array_equal(a["cmds"][:, i, 1], a["params"][:, 2 * blk + 1])
    # re-solving from the optimum must not move it by more than the tolerance band and must not raise the cost
    sc2 = sc.select(np.arange(0, 8192, 16))
    sc2.init_params = np.ascontiguousarray(a["params"][::16])
    r2 = s.solve(sc2)
    assert np.all(r2["final_cost"] <= a["final_cost"][::16] * (1 + 1e-9))
    # initial cost reported by the solve == cost of the K1 sweep at the projected start point
    x0 = np.clip(sc2.init_params, [prm.v_min, prm.w_min] * nb, [prm.v_max, prm.w_max] * nb)
    ev = s.evaluate(sc2, x0)
    assert np.allclose(ev["cost"], r2["initial_cost"], rtol=1e-12)


FULL_SIZE_SHAPES = {
    # BASELINE configs at the size they are stated at (per GPU): the one-scene-per-wave shapes (T = 38) and cfg2
    "cfg5_n16_h30_t38": (README.replace(control_horizon=30, max_time=2.0), dict(B=8192, N=16, seed=0x5EED0001), 512),
    "params_yaml_n3_t38": (OptimizerParams.params_yaml(), dict(B=8192, N=3, seed=0x5EED0001), 512),
    "cfg2_n4_b1024": (README, dict(B=1024, N=4, seed=0x5EED0001), 1024),
}


@pytest.mark.parametrize("name", list(FULL_SIZE_SHAPES))
def test_full_size_properties_other_shapes(Solver, oracle, name):
    """The properties of test_full_size_properties_cfg3 on the other BASELINE shapes at full size, plus the oracle on a
    sample of the batch (the first `sample` scenes)."""
    prm, kw, sample = FULL_SIZE_SHAPES[name]
    sc = make_scenes(prm, **kw)
    B, T = sc.B, sc.T
    s = Solver(prm)
    a = s.solve(sc)
    b = s.solve(sc)
    for k in a:
        assert np.array_equal(a[k], b[k]), f"non-deterministic output {k}"
    CH, bl, nb, P, M, nbnd = prm.dims(T)
    assert np.all(a["status"] != 2)
    assert np.all(a["final_cost"] <= a["initial_cost"] * (1 + 1e-12))
    assert np.all((a["iterations"] >= 0) & (a["iterations"] <= prm.max_iterations))
    v, w = a["params"][:, 0:2 * nbnd:2], a["params"][:, 1:2 * nbnd:2]      # the bounded blocks (src/optimizer.cpp:373-379)
    assert v.min() >= prm.v_min and v.max() <= prm.v_max and w.min() >= prm.w_min and w.max() <= prm.w_max
    for i in range(T + 1):                                                              # a12 expansion
        blk = i // bl if i < CH else (CH - 1) // bl
        assert np.array_equal(a["cmds"][:, i, 0], a["params"][:, 2 * blk])
        assert np.array_equal(a["cmds"][:, i, 1], a["params"][:, 2 * blk + 1])
    stride = max(1, B // 512)
    sc2 = sc.select(np.arange(0, B, stride))
    x0 = np.clip(sc2.init_params, [prm.v_min, prm.w_min] * nbnd + [-np.inf, -np.inf] * (nb - nbnd),
                 [prm.v_max, prm.w_max] * nbnd + [np.inf, np.inf] * (nb - nbnd))
    ev = s.evaluate(sc2, x0)
    assert np.allclose(ev["cost"], a["initial_cost"][::stride], rtol=1e-12)
    # the oracle on a sample: every firm, well-conditioned scene within the tolerance, same status and iteration count
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


def test_edge_cases(Solver, oracle):
    prm = README
    s = Solver(prm)
    # B = 1 (the plugin's use) and B = 0 (empty batch)
    one = make_scenes(prm, 1, 3, n_valid=3, map_cells=80, seed=401)
    assert np.max(cmd_err(s.solve(one)["cmds"], oracle.solve(prm, one, theta_zero_convention=True)["cmds"])) <= CMD_TOL
    empty = one.select(np.array([], dtype=np.int64))
    out = s.solve(empty)
    assert out["cmds"].shape[0] == 0
    # very short horizon: T = 2 < control_horizon
    def agree(scenes):
        ref = oracle.solve(prm, scenes, theta_zero_convention=True)
        firm = ref["marginal_decisions"] == 0
        assert firm.any()
        return np.max(cmd_err(s.solve(scenes)["cmds"][firm], ref["cmds"][firm])) <= CMD_TOL
    short = make_scenes(prm, 8, 3, T=2, map_cells=80, seed=402, standing_fraction=0.0)
    assert agree(short)
    # robot driving off the costmap: clamp-to-edge interpolation (aimed at cell by cell in tests/test_gpu_obstacle_edges.py)
    edge = make_scenes(prm, 8, 3, map_cells=20, seed=403, standing_fraction=0.0)
    assert agree(edge)
    # shared costmap
    shared = make_scenes(prm, 8, 4, map_cells=80, seed=404, standing_fraction=0.0)
    shared.costmap = np.ascontiguousarray(shared.costmap[:1]); shared.costmap_origin = np.ascontiguousarray(shared.costmap_origin[:1])
    shared.costmap_shared = True
    assert agree(shared)
    # iteration cap 0: parameters are only projected into the box
    capped = Solver(prm.replace(max_iterations=0)).solve(one)
    assert capped["iterations"][0] == 0 and capped["status"][0] == 1
    # unsupported shapes are refused with an error code, not a crash
    from nav2_social_mpc_controller_amd.solver import SmpcError
    too_long = make_scenes(prm, 1, 3, T=70, map_cells=40, seed=405)
    with pytest.raises(SmpcError):
        s.solve(too_long)


def test_no_valid_agent_fails_like_the_reference(Solver, oracle):
    """people present but every projected agent invalid (e.g. all dropped by project_people, src/optimizer.cpp:598-603):
    Ceres rejects the initial evaluation -> FAILURE -> Optimizer::optimize returns false (src/optimizer.cpp:384-388)."""
    sc = make_scenes(README, 8, 3, n_valid=0, map_cells=80, seed=108)
    ro = oracle.solve(README, sc)
    rg = Solver(README).solve(sc)
    assert np.all(ro["status"] == 2) and np.all(rg["status"] == 2)
    assert np.all(rg["reason"] == 7) and np.all(rg["iterations"] == 0)
    assert np.array_equal(rg["params"], ro["params"])        # the projected start point is handed back


def test_fixed_iteration_mode_runs_all_iterations(Solver):
    prm = README.replace(fixed_iterations=1)
    sc = make_scenes(prm, 64, 8, seed=501)
    r = Solver(prm).solve(sc)
    assert np.all((r["iterations"] == prm.max_iterations) | (r["reason"] == 4) | (r["reason"] == 6))


def test_device_resident_path_matches_host_path(Solver):
    import torch
    prm = README
    sc = make_scenes(prm, 256, 8, seed=601)
    s = Solver(prm)
    host = s.solve(sc)
    sb, tens = sc.to_device()
    rb, rt = s.alloc_results(sc.B, sc.T)
    stream = torch.cuda.Stream()
    s.set_stream(stream.cuda_stream)
    s.solve_device(sb, rb)
    stream.synchronize()
    assert s.last_kernel_ms() > 0.0
    for k in host:
        assert np.array_equal(rt[k].cpu().numpy(), host[k]), k


def _random_params(rng):
    bl = int(rng.integers(2, 8))
    ch = int(rng.integers(bl, min(6 * bl, 30) + 1))          # 1..6 parameter blocks
    return README.replace(
        control_horizon=ch, parameter_block_length=bl, max_time=float(rng.choice([1.0, 1.5, 2.0])),
        distance_weight=float(rng.uniform(5, 60)), social_weight=float(rng.uniform(0, 800)),
        velocity_weight=float(rng.uniform(1, 15)), angle_weight=float(rng.uniform(0, 300)),
        agent_angle_weight=float(rng.choice([0.0, rng.uniform(1, 60)])), proxemics_weight=float(rng.uniform(0, 120)),
        velocity_feasibility_weight=float(rng.uniform(0, 10)), goal_align_weight=float(rng.uniform(0, 15)),
        obstacle_weight=float(rng.uniform(0, 0.3)), max_iterations=int(rng.choice([5, 20, 40])),
        linear_solver_type=str(rng.choice(["DENSE_SCHUR", "DENSE_QR", "SPARSE_NORMAL_CHOLESKY"])),
        fn_tol=float(rng.choice([1e-5, 1e-7])))


@pytest.mark.parametrize("case", range(8))
def test_randomised_parameter_sets(Solver, oracle, case):
    """Random weights / horizons / block lengths / solver types / iteration caps (1..6 parameter blocks, T 18..38)."""
    rng = np.random.default_rng(7000 + case)
    prm = _random_params(rng)
    N = int(rng.integers(1, 12))
    sc = make_scenes(prm, 48, N, seed=8000 + case, map_cells=int(rng.choice([60, 120, 200])),
                     n_valid=int(rng.integers(1, N + 1)))
    CH, bl, nb, P, M, _ = prm.dims(sc.T)
    assert 1 <= nb <= 6
    s = Solver(prm)
    ev_o, ev_g = oracle.evaluate(prm, sc, sc.init_params), s.evaluate(sc, sc.init_params)
    assert np.max(np.abs(ev_o["jacobian"] - ev_g["jacobian"]) / np.maximum(1.0, np.abs(ev_o["jacobian"]))) < JAC_RTOL
    rz = oracle.solve(prm, sc, nthreads=16, theta_zero_convention=True)
    rg = s.solve(sc)
    stable = well_conditioned(oracle, prm, sc, rz, nthreads=16, theta_zero_convention=True)
    assert stable.mean() >= 0.97, f"only {stable.sum()}/{len(stable)} scenes are well conditioned"
    firm = (rz["marginal_decisions"] == 0) & stable
    assert firm.mean() >= 0.8
    assert np.max(cmd_err(rg["cmds"][firm], rz["cmds"][firm])) <= CMD_TOL
    assert np.array_equal(rg["iterations"][firm], rz["iterations"][firm])
    assert np.array_equal(rg["status"][firm], rz["status"][firm])


@pytest.mark.timeout(120)
def test_non_finite_inputs_terminate_and_fail_cleanly(Solver):
    """Every wave must reach its exit whatever the input (a hung wave can take the GPU down): scenes with NaN / inf in
    their people, path or start pose end as FAILURE (non-finite initial evaluation, like Ceres), neighbours are not
    affected."""
    prm = README
    sc = make_scenes(prm, 64, 8, seed=601, map_cells=80)
    clean = Solver(prm).solve(sc)
    bad = sc.select(np.arange(64))
    bad.people[3, :, 0, 2] = np.nan           # one agent's x
    bad.people[7, :, 2, :] = np.inf           # every yaw of a scene
    bad.pose0[11, 2] = np.nan                 # start heading
    bad.path_pts[13, 5, 0] = np.inf           # one path point
    bad.init_params[17, 1] = np.nan           # warm-start command
    out = Solver(prm).solve(bad)
    hit = np.array([3, 7, 11, 13, 17])
    assert np.all(out["status"][hit] == 2), out["status"][hit]
    rest = np.setdiff1d(np.arange(64), hit)
    assert np.array_equal(out["status"][rest], clean["status"][rest])
    assert np.max(np.abs(out["cmds"][rest] - clean["cmds"][rest])) == 0.0


def test_staged_people_block(Solver):
    """smpc_stage_people_batch: the records / aux the sweep reads, against a numpy statement of the same conversion;
    a solve and a sweep fed with the staged block give bit-identical results to the ones that stage internally."""
    from nav2_social_mpc_controller_amd._abi import SmpcResultBatch, SmpcEvalOut
    prm = README
    sc = make_scenes(prm, 96, 5, seed=77, map_cells=80)
    sc.people[3, :, 3, 2] = -1.0            # a phantom agent
    sc.has_people[5] = 0
    s = Solver(prm)
    rec, aux = s.stage_people(sc)
    T, N = sc.T, sc.N
    ppl = sc.people[:, 1:]                  # people_proj[t + 1]
    want = np.stack([ppl[:, :, 0], ppl[:, :, 1], ppl[:, :, 4] * np.cos(ppl[:, :, 2]), ppl[:, :, 4] * np.sin(ppl[:, :, 2])], axis=-1)
    want = want.transpose(0, 2, 1, 3)       # [B][N][T][4]
    live = sc.has_people != 0
    assert np.abs(rec[live] - want[live]).max() <= 1e-15
    mask = aux[..., 0].copy().view(np.uint64)
    want_mask = ((ppl[:, :, 3] != -1.0) * (1 << np.arange(N))[None, None, :]).sum(axis=2).astype(np.uint64)
    assert np.array_equal(mask[live], want_mask[live])
    assert int(mask[3, 0]) & 4 == 0 and int(mask[2, 0]) & 4 == 4
    tgt = aux[..., 1]
    active = tgt != 1e300
    assert active[live].any() and (~active[live]).any()
    d = np.abs(np.abs(tgt - sc.pose0[:, None, 2]) - np.pi / 6)
    assert d[active & live[:, None]].max() <= 1e-15
    # same results with the caller-staged block (host pointers)
    a = s.solve(sc)
    ea = s.evaluate(sc, sc.init_params)
    sb = sc.to_c()
    sb.people_records, sb.people_aux = rec.ctypes.data, aux.ctypes.data
    sb.people = None
    CH, bl, nb, P, M, _ = prm.dims(T, True)
    out = {"params": np.zeros((sc.B, P)), "cmds": np.zeros((sc.B, T + 1, 2)), "iterations": np.zeros(sc.B, np.int32)}
    rb = SmpcResultBatch()
    for k, v in out.items():
        setattr(rb, k, v.ctypes.data)
    import ctypes
    assert s.lib.smpc_solve_batch(s._h, ctypes.byref(sb), ctypes.byref(rb)) == 0
    for k in out:
        assert np.array_equal(out[k], a[k]), k
    J = np.zeros((sc.B, M, P))
    eo = SmpcEvalOut()
    eo.jacobian = J.ctypes.data
    x = np.ascontiguousarray(sc.init_params)
    assert s.lib.smpc_eval_batch(s._h, ctypes.byref(sb), x.ctypes.data, ctypes.byref(eo)) == 0
    assert np.array_equal(J, ea["jacobian"])


def test_critic_major_row_order(Solver):
    """smpc_eval_batch_out.row_order = 1 (the coalesced store path of K1) holds the same rows as the reference order,
    permuted as the header says; cost and gradient do not depend on the order. With and without people, with a phantom,
    with the feasibility rows of P = 10, for both slot widths."""
    for prm, N, T, kw in ((README, 8, None, {}), (README, 3, None, {"people_present": False}),
                          (README.replace(control_horizon=30, max_time=2.0), 16, None, {}),
                          (README.replace(control_horizon=20, parameter_block_length=4, max_time=2.0), 3, None, {})):
        sc = make_scenes(prm, 70, N, seed=11, map_cells=80, **kw)
        if sc.has_people.all():
            sc.has_people[4] = 0
        s = Solver(prm)
        a = s.evaluate(sc, sc.init_params, row_order=0)
        b = s.evaluate(sc, sc.init_params, row_order=1)
        assert np.array_equal(a["cost"], b["cost"]) and np.array_equal(a["gradient"], b["gradient"])
        for i in range(sc.B):
            hp = bool(sc.has_people[i]) and N > 0
            perm = s.row_permutation(sc.T, hp)
            assert np.array_equal(a["residuals"][i, :len(perm)], b["residuals"][i][perm]), i
            assert np.array_equal(a["jacobian"][i, :len(perm)], b["jacobian"][i][perm]), i
            assert not a["jacobian"][i, len(perm):].any() and not b["jacobian"][i, len(perm):].any()
