"""Lone trips of the two-scenes-per-wave solve kernels (`-m gpu`): once one slot of a wave is idle for good, its lanes
evaluate every other agent for the scene in the other slot (csrc/smpc_sweep.hpp, kLone). The owner lane still does every
accumulation, in agent order, on the values its own evaluation would have produced — so a solve with lone trips and one
with SMPC_NO_LONE_HELP (every trip paired) must agree in every bit of every result array. That is what is compared here,
on the shapes and scenes where the helped loop can go wrong, next to the oracle on the smallest batches and the count of
helped trips the launch reports under SMPC_DEBUG_GRID. Everything runs at SMPC_SOLVE_WIDTH=32 (batches this small take
the one-scene-per-wave kernel otherwise)."""
import re

import numpy as np
import pytest

from parity_checks import check_solve
from nav2_social_mpc_controller_amd.params import OptimizerParams
from nav2_social_mpc_controller_amd.scenes import make_scenes
from test_gpu_instantiations import RESULT_KEYS, same

pytestmark = pytest.mark.gpu

README = OptimizerParams.readme()
T = 28
SEED_B8 = 2905   # chosen with the oracle (test_sweep_plan_lone.py): of its pairs (0,1) .. (6,7) some end first in each order
TRIPS = re.compile(r"\[smpc\] solve kernel: (\d+) trips, (\d+) with one slot idle for good, (\d+) helped")


@pytest.fixture(scope="module")
def Solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    return BatchSolver


@pytest.fixture
def run(Solver, monkeypatch, capfd):
    """run(scenes, help=True, fixed=True) -> (results, (trips, one slot idle, helped)) of one solve launch"""
    monkeypatch.setenv("SMPC_SOLVE_WIDTH", "32")
    monkeypatch.setenv("SMPC_DEBUG_GRID", "1")

    def go(sc, help=True, fixed=True, prm=README):
        if help:
            monkeypatch.delenv("SMPC_NO_LONE_HELP", raising=False)
        else:
            monkeypatch.setenv("SMPC_NO_LONE_HELP", "1")
        s = Solver(prm)
        s.set_fixed_shapes(fixed)
        assert s.solve_slot_width(sc.B, sc.T, sc.N) == 32
        capfd.readouterr()
        res = s.solve(sc)
        found = TRIPS.findall(capfd.readouterr().err)
        assert len(found) == 1, found
        return res, tuple(int(v) for v in found[0])
    return go


def on_off(run, sc, what, **kw):
    """both solves of `sc`, bit-equal; returns the helped one with its counts and the paired one's"""
    a, ca = run(sc, help=True, **kw)
    b, cb = run(sc, help=False, **kw)
    print(f"\n[lone help] {what}: trips {ca[0]}, one slot idle {ca[1]}, helped {ca[2]} (without help: {cb})")
    same(a, b, RESULT_KEYS, what=what)
    assert cb[2] == 0, (what, cb)                       # the knob: every trip paired
    assert ca[:2] == cb[:2], (what, ca, cb)             # the same trips either way: the help changes no decision
    return a, ca


def test_a_single_scene_is_helped_from_its_first_trip_and_matches_the_oracle(run):
    sc = make_scenes(README, 1, 8, T=T, seed=2901, map_cells=80)
    a, (trips, half, helped) = on_off(run, sc, "B = 1")
    assert trips == int(a["evaluations"][0])            # one sweep per trip
    assert half == trips and helped == trips            # slot 1 never had a scene
    check_solve(README, sc, a)


def test_three_scenes_match_the_oracle(run):
    sc = make_scenes(README, 3, 8, T=T, seed=2902, map_cells=80)
    a, (trips, half, helped) = on_off(run, sc, "B = 3")
    assert helped >= int(a["evaluations"].min())        # one of the scenes has a wave to itself
    counts, worst = check_solve(README, sc, a)
    assert counts["firm"] >= 2, counts


@pytest.mark.parametrize("fixed", [True, False], ids=["fixed_shape_kernel", "run_time_shape_kernel"])
def test_eight_headline_scenes_with_both_halves_as_owner(Solver, run, fixed):
    sc = make_scenes(README, 8, 8, T=T, seed=SEED_B8, map_cells=80)
    assert Solver(README).solve_shape_is_fixed(8, T, 8)
    a, (trips, half, helped) = on_off(run, sc, f"B = 8, fixed = {fixed}", fixed=fixed)
    ev = a["evaluations"].reshape(4, 2)                 # a wave's two slots take neighbouring scenes from the queue
    assert (ev[:, 0] > ev[:, 1]).any(), ev              # slot 0 outlives slot 1: the low half owns lone trips
    assert (ev[:, 0] < ev[:, 1]).any(), ev              # ... and the high half
    assert helped > 0


@pytest.mark.parametrize("N", [2, 3, 7])
def test_agent_counts_even_odd_and_one_short_of_the_headline(run, N):
    sc = make_scenes(README, 3, N, T=T, seed=2910 + N, map_cells=80)
    a, (trips, half, helped) = on_off(run, sc, f"N = {N}")
    assert helped > 0


def test_one_agent_is_never_helped(run):
    sc = make_scenes(README, 1, 1, T=T, seed=2920, map_cells=80)
    a, (trips, half, helped) = on_off(run, sc, "N = 1")
    assert half == trips > 0 and helped == 0


def test_a_scene_without_people_beside_scenes_with_people(run):
    sc = make_scenes(README, 3, 8, T=T, seed=2921, map_cells=80)
    sc.has_people[1] = 0
    a, (trips, half, helped) = on_off(run, sc, "has_people = 0 beside people")
    assert helped > 0
    alone = sc.select(np.array([1]))                    # the scene without people alone in its wave: lone trips, none helped
    b, (trips, half, helped) = on_off(run, alone, "has_people = 0 alone")
    assert half == trips > 0 and helped == 0
    same(b, {k: v[1:2] for k, v in a.items()}, RESULT_KEYS, what="the scene without people, alone and in the batch")


def test_a_scene_whose_agents_are_all_invalid(run):
    sc = make_scenes(README, 1, 3, T=T, seed=2922, map_cells=80, n_valid=0)
    a, (trips, half, helped) = on_off(run, sc, "all agents invalid")
    assert helped > 0 and a["status"][0] == 2           # rejected at the initial evaluation, like the reference


def redo_scene(kind):
    """One scene whose agent 1 — odd: the helper half evaluates it — is a pair the fast form does not cover at the first
    sweep: `coincident` stands where the robot stands (the start command is zero, so every step's pose is the start pose),
    `collinear` stands 2 m straight ahead of a robot that drives straight at it (theta within 1e-6 of 0 with different
    velocities: pair_force() flags it `special`), `equal_velocity` stands beside a robot that stands too (theta := 0)."""
    sc = make_scenes(README, 1, 4, T=T, seed=2930, map_cells=80, standing_fraction=0.0)
    x0, y0, yaw0 = sc.pose0[0]
    sc.init_params[0, :] = 0.0
    ahead = 0.0 if kind == "coincident" else 2.0
    side = 1.0 if kind == "equal_velocity" else 0.0
    if kind == "collinear":
        sc.init_params[0, 0::2] = 0.3
    sc.people[0, :, 0, 1] = x0 + ahead * np.cos(yaw0) - side * np.sin(yaw0)
    sc.people[0, :, 1, 1] = y0 + ahead * np.sin(yaw0) + side * np.cos(yaw0)
    sc.people[0, :, 4, 1] = 0.0
    return sc


@pytest.mark.parametrize("kind", ["coincident", "collinear", "equal_velocity"])
def test_the_helper_meets_a_pair_that_needs_the_general_form(run, kind):
    sc = redo_scene(kind)
    a, (trips, half, helped) = on_off(run, sc, kind)
    assert helped > 0 and np.isfinite(a["final_cost"][0]) and a["status"][0] != 2
