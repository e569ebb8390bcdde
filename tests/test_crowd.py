"""The crowd step (smpc_crowd_step_batch) without a GPU: the plumbing of the new entry point, the CPU checker
(tests/crowd_ref.py) against the oracle's people projection on the one configuration where the two models coincide, the
checker's closed forms, and the margins of the seeded inputs that tests/test_gpu_crowd.py runs on the device."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import crowd_cases as G
import crowd_ref as R
from nav2_social_mpc_controller_amd import _abi
from nav2_social_mpc_controller_amd import solver as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc.h")


# ---- plumbing -------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_listed_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+smpc_crowd_step_batch\s*\(", src)
    assert "smpc_crowd_step_batch" in _abi.EXPORTED_SYMBOLS
    assert os.path.exists(S.LIB_PATH), "run __graft_entry__.build() first"
    out = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    assert "smpc_crowd_step_batch" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert _abi.SMPC_ABI_VERSION == 6 and int(re.search(r"#define SMPC_ABI_VERSION (\d+)", src).group(1)) == 6
    assert int(re.search(r"#define SMPC_MAX_WAYPOINTS (\d+)", src).group(1)) == _abi.SMPC_MAX_WAYPOINTS == 8


def test_crowd_params_defaults_and_refusals():
    from nav2_social_mpc_controller_amd.params import CrowdParams
    cp = CrowdParams()
    assert (cp.goal_radius, cp.person_radius, cp.desired_speed, cp.cyclic, cp.robot_visible) == (0.25, 0.35, 0.6, True, True)
    cb = S.BatchSolver.crowd_c(cp, 5, 4, 2, 0.05, 1)
    assert (cb.B, cb.Np, cb.K, cb.on_device, cb.cyclic, cb.robot_visible) == (5, 4, 2, 1, 1, 1)
    assert (cb.dt, cb.goal_radius, cb.person_radius, cb.desired_speed) == (0.05, 0.25, 0.35, 0.6)
    for bad in (dict(goal_radius=-0.1), dict(person_radius=-0.1), dict(desired_speed=0.0)):
        with pytest.raises(ValueError):
            CrowdParams(**bad)


def test_crowd_waypoints_are_seeded_free_inside_and_ahead():
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    from nav2_social_mpc_controller_amd.scenes import crowd_waypoints, make_scenes
    sc = make_scenes(OptimizerParams.readme(), 48, 4)
    wp, n = crowd_waypoints(sc, K=2)
    assert wp.shape == (48, 4, 2, 2) and n.shape == (48, 4) and n.dtype == np.int32
    again = crowd_waypoints(sc.select(np.arange(8, 16)), K=2, first_scene=8)
    assert np.array_equal(again[0], wp[8:16]) and np.array_equal(again[1], n[8:16])   # a function of the scene's id
    side = sc.size_x * sc.resolution
    rel = wp - sc.costmap_origin[:, None, None, :]
    assert (rel >= 0.5).all() and (rel <= side - 0.5).all()
    cell = np.floor(rel / sc.resolution).astype(int)
    assert (sc.costmap[np.arange(48)[:, None, None], cell[..., 1], cell[..., 0]] == 0).all()
    st0 = sc.people[:, 0]
    walking = st0[:, 4, :] > 0.0
    assert np.array_equal(n, np.where(walking, 2, 0)) and walking.any() and not walking.all()
    d = wp[:, :, 0] - st0[:, 0:2, :].transpose(0, 2, 1)
    off = np.arctan2(d[..., 1], d[..., 0]) - st0[:, 2, :]
    ahead = np.abs(np.arctan2(np.sin(off), np.cos(off))) < 1e-9
    assert ahead[walking].mean() > 0.9   # (a person about to leave the map has no free cell ahead: it gets a seeded one)


# ---- the checker against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 5, 8])
def test_checker_agrees_with_the_oracle_projection_where_the_models_coincide(n):
    """project_people with the robot at robot_path[0]: persons with desired speed 0.5, one waypoint each at
    p + max_time * v, goal radius 0.25. The oracle's obstacle term (its quirk) is a function of the far grid corner alone,
    of order 1e-16; the checker runs without a grid."""
    from nav2_social_mpc_controller_amd.episode import far_obstacle_grid
    from oracle import pyref_sfm

    g = np.random.default_rng(100 + n)
    max_time, time_step = 1.5, 0.05
    init = np.zeros((n, 6))
    init[:, 0:2] = g.uniform(-2.5, 2.5, (n, 2))
    init[:, 2] = g.uniform(-math.pi, math.pi, n)
    init[:, 4] = g.uniform(0.1, 0.45, n)
    init[n - 1, 4] = 0.0                                     # one stands
    robot_path = np.zeros((3, 6))
    robot_path[:, 0:2] = [[0.1, -0.2], [0.13, -0.2], [0.16, -0.2]]
    robot_path[:, 2], robot_path[:, 4] = 0.3, 0.55
    idx, origin, res = far_obstacle_grid()
    od = dict(indexes=idx, width=idx.shape[1], height=idx.shape[0], resolution=res, origin_x=origin[0], origin_y=origin[1])
    want = pyref_sfm.project_people(init, robot_path, od, max_time, time_step, theta_zero_convention=True)[1]
    vel = init[:, 4:5] * np.stack([np.cos(init[:, 2]), np.sin(init[:, 2])], axis=1)
    people = np.concatenate([init[:, 0:2], vel, np.zeros((n, 1))], axis=1)
    wp = (init[:, 0:2] + float(np.float32(max_time)) * vel)[:, None, :]
    got, _ = R.step(float(np.float32(time_step)), people, np.zeros(n, np.int32), robot_path[0, 0:3], [robot_path[0, 4], 0.0], n,
                    wp, np.ones(n, np.int32), goal_radius=0.25, desired_speed=0.5, robot_visible=True)
    assert np.abs(got[:, 0:2] - want[:, 0:2]).max() <= 1e-9
    wv = want[:, 4:5] * np.stack([np.cos(want[:, 2]), np.sin(want[:, 2])], axis=1)
    assert np.abs(got[:, 2:4] - wv).max() <= 1e-9


# ---- closed forms ---------------------------------------------------------------------------------------------------------
def _one(people, **kw):
    people = np.asarray(people, np.float64)
    n = people.shape[0]
    args = dict(cursor=np.zeros(n, np.int32), pose=np.zeros(3), twist=np.zeros(2), count=n, waypoints=np.zeros((n, 1, 2)),
                n_waypoints=np.zeros(n, np.int32), robot_visible=False)
    args.update(kw)
    return R.step(G.DT, people, **args)


def test_a_lone_person_without_waypoints_slows_down_on_its_heading():
    v = np.array([0.3, -0.4])
    got, cur = _one([[1.0, 2.0, v[0], v[1], 0.7]])
    assert np.allclose(got[0, 2:4], v * (1.0 - 2.0 * G.DT), rtol=0, atol=1e-16)
    assert abs(math.hypot(*got[0, 2:4]) - 0.5 * (1.0 - 2.0 * G.DT)) <= 1e-16
    assert abs(got[0, 4]) <= 1e-14 and cur[0] == 0                       # the heading is kept
    assert np.allclose(got[0, 0:2], [1.0, 2.0] + got[0, 2:4] * G.DT, rtol=0, atol=1e-16)


def test_two_standing_persons_get_exactly_opposite_velocities():
    got, _ = _one([[0.25, 0.5, 0.0, 0.0, 0.0], [1.0, -0.75, 0.0, 0.0, 0.0]])
    assert np.abs(got[0, 2:4] + got[1, 2:4]).max() <= 1e-15
    assert math.hypot(*got[0, 2:4]) > 1e-3                               # they do push each other
    d = np.array([0.75, -1.25])
    assert abs(got[1, 2] * d[1] - got[1, 3] * d[0]) <= 1e-15                        # along the line between them: thetaSign = 0


def test_cursor_wraps_when_cyclic_and_stops_otherwise():
    people = [[0.0, 0.0, 0.5, 0.0, 0.0]]
    wp = np.array([[[0.2, 0.0], [5.0, 5.0]]])
    for cyclic, n_wp, start, want in ((True, 2, 0, 1), (False, 2, 0, 1), (True, 1, 0, 0), (False, 1, 0, 1), (False, 1, 1, 1),
                                      (True, 2, 2, 0), (True, 0, 0, 0), (False, 0, 0, 0)):
        _, cur = _one(people, waypoints=wp, n_waypoints=np.array([n_wp], np.int32), cursor=np.array([start], np.int32), cyclic=cyclic)
        assert cur[0] == want, (cyclic, n_wp, start)
    # a person without a goal left comes to rest: only the relaxation term acts
    got, _ = _one(people, waypoints=wp, n_waypoints=np.array([1], np.int32), cursor=np.array([1], np.int32), cyclic=False)
    assert got[0, 2] == 0.5 - (0.5 / 0.5) * G.DT and got[0, 3] == 0.0


# ---- the inputs of the GPU tests stay clear of every decision ---------------------------------------------------------
@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: f"B{s[0]}_Np{s[1]}")
def test_generated_inputs_keep_their_margins(shape):
    d = G.case(shape)
    if d["B"] >= 2:
        assert (d["count"] == 0).any() and (d["count"] == d["Np"]).any()
    on_grid = off_grid = 0
    for ci, cfg in enumerate(G.CONFIGS):
        pos, kw = G.arguments(d, cfg)
        least = dict.fromkeys(G.CONDITIONS, math.inf)
        for b in range(d["B"]):
            rpos, one = G.robot_arguments(pos, kw, b)
            m = R.margins(*rpos, **one)
            for name in least:
                least[name] = min(least[name], m[name])
            if cfg["grid"] == "per":
                for i in range(d["count"][b]):
                    hit = R.obstacle_of(d["people"][b, i, 0], d["people"][b, i, 1], d["grids"][b], d["origin"][b], G.RES)
                    on_grid, off_grid = on_grid + (hit is not None), off_grid + (hit is None)
        print(shape, cfg, least)
        for name, need in G.CONDITIONS.items():
            assert least[name] >= need, (shape, ci, name, least[name])
    assert R.obstacle_of(*d["people"][0, 0, 0:2], d["grids"][0], d["origin"][0], G.RES) is None   # the out-of-range entry
    assert d["grids"][0, 11, 7] == G.CELLS * G.CELLS
    if d["B"] >= 3:
        assert on_grid > 0 and off_grid > 0
        ev = G.reference(shape, 0)[2]
        assert ev.get("arrived", 0) > 0 and ev.get("wrapped", 0) > 0


def test_checker_shows_the_person_gives_way_to_a_visible_robot():
    def stepper(people, cursor, d, visible):
        return R.step_batch(G.DT, people, cursor, d["pose"], d["twist"], d["count"], d["waypoints"], d["n_waypoints"],
                            robot_visible=visible, cyclic=False, **G.PARAMS)
    seen, unseen = G.closest_approach(stepper, True), G.closest_approach(stepper, False)
    print(f"closest approach: robot visible {seen:.4f} m, invisible {unseen:.4f} m")
    assert unseen <= 0.15 and seen - unseen >= 0.2
