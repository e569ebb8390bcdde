"""The fixed-shape kernels of the headline configuration (`-m gpu`): smpc_solve_fixed_kernel / smpc_eval_fixed_kernel
<FixedShape<28, 8, 18, 6>> give, bit for bit, what the run-time-shape kernels <3, 32, false, false> give, and only the
listed shape at the two-scenes-per-wave width runs them (csrc/smpc_launch.hpp SMPC_FIXED_SHAPES, smpc_plan.hpp
plan_sweep()).

Two batches. B = 5 on three waves of two slots: one wave runs with an empty slot, a scene without people sits beside
scenes with people, one agent of every scene is invalid (a batch this small runs one scene per wave unless
SMPC_SOLVE_WIDTH says otherwise, as in test_gpu_instantiations; its grid has a slot for every scene). And B = 8192 + 37,
more scenes than the persistent grid has slots: every slot takes further scenes from the queue, so the second
load_scene(), the state's re-initialisation and the output stage of a re-used slot are compared too."""
import numpy as np
import pytest

from parity_checks import check_solve
from nav2_social_mpc_controller_amd.params import OptimizerParams
from nav2_social_mpc_controller_amd.scenes import make_scenes
from test_gpu_instantiations import EVAL_KEYS, RESULT_KEYS, same
from test_gpu_scene_params import eval_device

pytestmark = pytest.mark.gpu

README = OptimizerParams.readme()
T, N, B = 28, 8, 5


@pytest.fixture(scope="module")
def Solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    return BatchSolver


@pytest.fixture(scope="module")
def scenes():
    sc = make_scenes(README, B, N, T=T, seed=2801, map_cells=120, n_valid=N - 1)   # a 120 x 120 map, agent 7 invalid
    sc.has_people[1] = 0
    assert sc.T == T and sc.N == N and sc.costmap.shape[-2:] == (120, 120)
    assert README.dims(T, True)[:3] == (18, 6, 3)
    return sc


def test_solve_is_bit_equal_with_and_without_the_fixed_shape_kernel(Solver, scenes, monkeypatch):
    monkeypatch.setenv("SMPC_SOLVE_WIDTH", "32")
    s = Solver(README)
    assert s.solve_slot_width(B, T, N) == 32
    assert s.solve_shape_is_fixed(B, T, N)          # on by default
    fixed = s.solve(scenes)
    s.set_fixed_shapes(False)
    assert not s.solve_shape_is_fixed(B, T, N)
    plain = s.solve(scenes)
    s.set_fixed_shapes(True)
    assert s.solve_shape_is_fixed(B, T, N)
    same(plain, fixed, RESULT_KEYS, what="fixed shape solve")
    same(fixed, s.solve(scenes), RESULT_KEYS, what="fixed shape solve, again")
    assert np.all(fixed["status"] != 2) and np.all(fixed["evaluations"] > 1)


def test_slots_that_take_further_scenes_from_the_queue_are_bit_equal(Solver):
    """More scenes than slots (the library sizes a lone launch at eight waves per CU, two slots each: test_gpu_order's
    batch). Every result array, the re-rolled path's headings among them, bit for bit."""
    Bq = 8192 + 37
    sc = make_scenes(README, 1024, N, T=T, seed=2803, map_cells=80)   # 1024 different scenes, repeated to fill the batch
    sc.has_people[::97] = 0
    sc = sc.select(np.arange(Bq) % 1024)
    assert sc.B == Bq
    s = Solver(README)
    assert s.solve_slot_width(Bq, T, N) == 32 and s.solve_shape_is_fixed(Bq, T, N)
    fixed = s.solve(sc)
    s.set_fixed_shapes(False)
    assert not s.solve_shape_is_fixed(Bq, T, N)
    same(s.solve(sc), fixed, RESULT_KEYS, what="fixed shape solve, queue")
    assert np.all(fixed["status"] != 2) and np.all(fixed["evaluations"] > 1)


@pytest.mark.parametrize("row_order", [0, 1])
def test_k1_is_bit_equal_with_and_without_the_fixed_shape_kernel(Solver, scenes, row_order):
    s = Solver(README)
    assert s.eval_shape_is_fixed(T, N) and not s.eval_shape_is_fixed(T, N - 1) and not s.eval_shape_is_fixed(T - 1, N)
    x = scenes.init_params + 0.02 * np.random.default_rng(5).standard_normal(scenes.init_params.shape)
    fixed = eval_device(s, scenes, x, row_order)
    s.set_fixed_shapes(False)
    assert not s.eval_shape_is_fixed(T, N)
    plain = eval_device(s, scenes, x, row_order)
    same(plain, fixed, EVAL_KEYS, what=("fixed shape K1", row_order))
    same(plain, s.evaluate(scenes, x, row_order=row_order), EVAL_KEYS, what=("host-pointer K1", row_order))
    assert np.isfinite(fixed["cost"]).all() and fixed["jacobian"].any()


@pytest.mark.parametrize("shape", [dict(T=T, N=N - 1), dict(T=T - 1, N=N)], ids=["n7", "t27"])
def test_neighbouring_shapes_run_the_run_time_shape_kernel(Solver, shape, monkeypatch):
    """N = 7 and T = 27 are not listed: the query says so and the solve is the oracle's (parity_checks.check_solve; its
    population shares mean nothing over 16 scenes, so the counts are printed; at least half the scenes must be firm, so
    that the scene-by-scene comparison is not an empty one)."""
    monkeypatch.setenv("SMPC_SOLVE_WIDTH", "32")
    s = Solver(README)
    sc = make_scenes(README, 16, shape["N"], T=shape["T"], seed=2802, map_cells=120)
    assert s.solve_slot_width(sc.B, sc.T, sc.N) == 32 and README.dims(sc.T, True)[2] == 3
    assert not s.solve_shape_is_fixed(sc.B, sc.T, sc.N)
    counts, worst = check_solve(README, sc, s.solve(sc))
    print(f"\n[fixed shape neighbour] T={sc.T} N={sc.N}: worst firm |dcmd| {worst:.2e}, firm {counts['firm']}/{counts['scenes']}")
    assert counts["firm"] >= 8


def test_a_single_scene_still_takes_the_one_scene_per_wave_kernel(Solver, scenes):
    s = Solver(README)
    assert s.solve_slot_width(1, T, N) == 64
    assert not s.solve_shape_is_fixed(1, T, N)
    one = scenes.select(np.arange(1))
    a = s.solve(one)
    s.set_fixed_shapes(False)
    same(a, s.solve(one), RESULT_KEYS, what="B = 1")
