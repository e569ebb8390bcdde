"""Per-scene critic weights and velocity bounds (`smpc_scene_batch.scene_params`, `-m gpu`): scene b of a batch with rows
is solved / evaluated bit for bit as a handle holding row b's values would solve / evaluate it in the same batch."""
import json
import os

import numpy as np
import pytest

from conftest import cmd_err, well_conditioned
from nav2_social_mpc_controller_amd import _abi
from nav2_social_mpc_controller_amd.params import OptimizerParams, scene_param_rows
from nav2_social_mpc_controller_amd.scenes import make_scenes, uniform

pytestmark = pytest.mark.gpu

README = OptimizerParams.readme()
CMD_TOL = 1e-5
RESULT_KEYS = ("params", "cmds", "path", "status", "reason", "iterations", "evaluations", "initial_cost", "final_cost")
EVAL_KEYS = ("residuals", "jacobian", "cost", "gradient")
FIELD = {f: i for i, f in enumerate(_abi.SCENE_PARAM_FIELDS)}


@pytest.fixture(scope="module")
def Solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    return BatchSolver


def presets(tmp_path_factory):
    """The two benchmark presets as the YAML reader returns them from the shipped files (tests/golden)."""
    import yaml

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "benchmark_params.json")) as f:
        shipped = json.load(f)
    out = []
    for name in ("soc_work_obst_parameters_in_benchmark.yaml", "obst_only_parameters_in_benchmark.yaml"):
        doc = {"controller_server": {"ros__parameters": {"FollowPath": dict(
            plugin="nav2_social_mpc_controller::SocialMPCController", **shipped[name])}}}
        p = tmp_path_factory.mktemp("presets") / name
        p.write_text(yaml.safe_dump(doc))
        out.append(OptimizerParams.from_yaml(str(p)))
    return out


def same(a, b, keys, where=slice(None)):
    for k in keys:
        x, y = np.asarray(a[k])[where], np.asarray(b[k])[where]
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k  # bits, NaN included


def close(a, b, keys, rtol=1e-9):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert np.all(np.abs(x - y) <= rtol * np.maximum(1.0, np.abs(x))), (k, float(np.max(np.abs(x - y))))


def solve_device(s, sc):
    sb, keep = sc.to_device()
    rb, t = s.alloc_results(sc.B, sc.T)
    s.solve_device(sb, rb)
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def eval_device(s, sc, x, row_order):
    import torch
    sb, keep = sc.to_device()
    eo, t = s.alloc_eval(sc.B, sc.T, row_order=row_order)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    s.eval_device(sb, xd.data_ptr(), eo)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


# large batch: two scenes per wave (W = 32); small batch: one scene per wave, helper lanes from N = 8 (W = 64)
NEUTRAL = {"w32_b2560_n4": dict(B=2560, N=4, seed=601, map_cells=80), "w64_b40_n8": dict(B=40, N=8, seed=602)}


@pytest.mark.parametrize("name", list(NEUTRAL))
@pytest.mark.parametrize("horizons", [False, True])
def test_neutral_rows_are_invisible(Solver, name, horizons):
    sc = make_scenes(README, **NEUTRAL[name])
    if horizons:
        g = np.random.default_rng(3)
        sc = sc.with_horizons(g.integers(1, sc.T + 1, size=sc.B).astype(np.int32))
    s = Solver(README)
    assert s.solve_slot_width(sc.B, sc.T, sc.N) == (32 if name.startswith("w32") else 64)
    sp = sc.with_scene_params(scene_param_rows([README], np.zeros(sc.B, int)))
    base = s.solve(sc)
    same(base, s.solve(sp), RESULT_KEYS)
    same(base, solve_device(s, sp), RESULT_KEYS)
    # K1: the sp kernels read the horizon per scene, and the per-scene-horizon K1 is not bit-equal to the fixed-horizon
    # K1 (some Jacobian entries differ in their last bits, whatever the rows): the sp call is checked bit for bit against
    # the per-scene-horizon call with every T_scene = T, and both against the fixed-horizon call to K1's parity bound
    vt = sc if horizons else sc.with_horizons(np.full(sc.B, sc.T, np.int32))
    x = sc.init_params + 0.02 * np.random.default_rng(5).standard_normal(sc.init_params.shape)
    for row_order in (0, 1):
        eb = s.evaluate(vt, x, row_order=row_order)
        same(eb, s.evaluate(sp, x, row_order=row_order), EVAL_KEYS)
        same(eb, eval_device(s, sp, x, row_order), EVAL_KEYS)
        close(s.evaluate(sc, x, row_order=row_order), eb, EVAL_KEYS)


def test_mixed_presets_equal_uniform_launches(Solver, oracle, tmp_path_factory):
    a, b = presets(tmp_path_factory)
    assert a == OptimizerParams.soc_work_obst_benchmark() and b == OptimizerParams.obst_only_benchmark()
    sc = make_scenes(a, 256, 3, n_valid=2, map_cells=80, seed=603)
    which = np.arange(sc.B) % 2
    got = Solver(a).solve(sc.with_scene_params(scene_param_rows([a, b], which)))
    for k, p in enumerate((a, b)):
        idx = np.where(which == k)[0]
        same(got, Solver(p).solve(sc), RESULT_KEYS, idx)  # the uniform launch of the same batch
        sub = sc.select(idx)
        ro = oracle.solve(p, sub, nthreads=16)
        firm = (ro["marginal_decisions"] == 0) & well_conditioned(oracle, p, sub, ro, nthreads=16)
        assert firm.mean() >= 0.9, firm.sum()
        err = cmd_err(got["cmds"][idx], ro["cmds"])
        assert np.max(err[firm]) <= CMD_TOL, (k, float(np.max(err[firm])))
    # the presets differ in the social rows: the two halves must not have been solved alike
    assert not np.array_equal(got["cmds"][which == 0], Solver(b).solve(sc)["cmds"][which == 0])


# critic-major K1 rows (smpc_eval_batch_out.row_order = 1) with people: critic c of step t at c * T + t
CRITIC_OF = {"agent_angle_w": 0, "socialwork_w": 1, "proxemics_w": 2, "velocity_w": 3, "goal_align_w": 4,
             "distance_w": 5, "angle_w": 6, "obstacle_w": 7, "velocity_feasibility_w": 8}  # 8: the feasibility rows


def critic_rows(T, M, c):
    return np.arange(8 * T, M) if c == 8 else np.arange(c * T, (c + 1) * T)


def test_each_value_reaches_its_critic(Solver):
    sc = make_scenes(README, 32, 3, seed=604, map_cells=80, standing_fraction=0.0)
    T, B = sc.T, sc.B
    _, _, _, P, M, _ = README.dims(T, True)
    s = Solver(README)
    x = sc.init_params + 0.05 * np.random.default_rng(9).standard_normal(sc.init_params.shape)
    base_rows = scene_param_rows([README], np.zeros(B, int))
    base = s.evaluate(sc.with_scene_params(base_rows), x, row_order=1)
    active = [v for v in range(B) if all(np.any(base["residuals"][v][critic_rows(T, M, c)] != 0.0) for c in range(9))]
    assert active, "no scene with every critic active"
    victim = active[0]  # every doubled critic has non-zero rows, so each check below has teeth
    for field, c in CRITIC_OF.items():
        rows = base_rows.copy()
        rows[victim, FIELD[field]] *= 2.0
        got = s.evaluate(sc.with_scene_params(rows), x, row_order=1)
        mine = np.zeros(M, bool)
        mine[critic_rows(T, M, c)] = True
        r0, r1 = base["residuals"][victim], got["residuals"][victim]
        j0, j1 = base["jacobian"][victim], got["jacobian"][victim]
        assert np.array_equal(r1[mine], 2.0 * r0[mine]) and np.array_equal(j1[mine], 2.0 * j0[mine]), field
        assert np.array_equal(r1[~mine], r0[~mine]) and np.array_equal(j1[~mine], j0[~mine]), field
        others = np.arange(B) != victim
        same(base, got, ("residuals", "jacobian", "cost", "gradient"), others)
    rows = base_rows.copy()
    rows[victim, FIELD["desired_linear_vel"]] = 0.45
    got = s.evaluate(sc.with_scene_params(rows), x, row_order=1)
    vel = np.zeros(M, bool)
    vel[critic_rows(T, M, 3)] = True
    assert np.array_equal(got["residuals"][victim][~vel], base["residuals"][victim][~vel])
    assert np.array_equal(got["jacobian"][victim][~vel], base["jacobian"][victim][~vel])
    assert not np.array_equal(got["residuals"][victim][vel], base["residuals"][victim][vel])
    same(base, got, ("residuals", "jacobian"), np.arange(B) != victim)


def test_per_scene_bounds(Solver):
    sc = make_scenes(README, 64, 3, seed=605, map_cells=80)
    tight = README.replace(v_max=0.3, w_max=0.7)
    which = (np.arange(sc.B) % 3 == 1).astype(int)
    got = Solver(README).solve(sc.with_scene_params(scene_param_rows([README, tight], which)))
    idx = np.where(which == 1)[0]
    cm = got["cmds"][idx]
    assert cm[:, :, 0].max() <= 0.3 and cm[:, :, 1].max() <= 0.7 and cm[:, :, 1].min() >= -1.4
    same(got, Solver(tight).solve(sc), RESULT_KEYS, idx)
    same(got, Solver(README).solve(sc), RESULT_KEYS, np.where(which == 0)[0])
    assert README.v_max > 0.3 and got["cmds"][which == 0][:, :, 0].max() > 0.3  # the bound bites


def test_bad_host_rows_are_refused_before_anything_is_launched(Solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError

    sc = make_scenes(README, 8, 3, seed=606, map_cells=40)
    good = scene_param_rows([README], np.zeros(sc.B, int))
    for f, v in (("v_min", 0.7), ("w_min", 1.5), ("socialwork_w", np.nan), ("v_max", np.inf)):
        rows = good.copy()
        rows[3, FIELD[f]] = v
        s = Solver(README)
        with pytest.raises(SmpcError, match="scene_params"):
            s.solve(sc.with_scene_params(rows))
        with pytest.raises(SmpcError, match="scene_params"):
            s.evaluate(sc.with_scene_params(rows), sc.init_params)
        assert s.last_kernel_ms() < 0.0  # nothing was launched on this handle


def _episode(prm, sc, w_ref, rows=None):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode

    od = (np.zeros((480, 480), np.uint32), np.array([-16.0, -16.0]), float(np.float32(0.1)))
    return BatchEpisode(prm, sc, w_ref, *od, scene_params=rows)


def _run(ep, ticks):
    out = []
    for _ in range(ticks):
        ep.tick()
        ep.synchronize()
        out.append({"cmds": ep.res["cmds"].cpu().numpy().copy(), "path": ep.res["path"].cpu().numpy().copy(),
                    "status": ep.res["status"].cpu().numpy().copy(), "pose": ep.pose.cpu().numpy().copy(),
                    "cmd_vel": ep.cmd_vel.cpu().numpy().copy()})
    return out


def test_episodes(Solver, tmp_path_factory):
    a, b = presets(tmp_path_factory)
    B, N = 48, 3
    sc = make_scenes(a, B, N, n_valid=2, map_cells=80, seed=607)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    keys = ("cmds", "path", "status", "pose", "cmd_vel")
    plain = _run(_episode(a, sc, w_ref), 4)
    neutral = _run(_episode(a, sc, w_ref, scene_param_rows([a], np.zeros(B, int))), 4)
    for t0, t1 in zip(plain, neutral):
        same(t0, t1, keys)
    which = np.arange(B) % 2
    mixed = _run(_episode(a, sc, w_ref, scene_param_rows([a, b], which)), 4)
    only_b = _run(_episode(b, sc, w_ref), 4)
    for tm, ta, tb in zip(mixed, plain, only_b):
        same(tm, ta, keys, which == 0)
        same(tm, tb, keys, which == 1)
    assert not np.array_equal(plain[-1]["pose"][which == 1], only_b[-1]["pose"][which == 1])
