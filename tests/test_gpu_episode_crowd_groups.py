"""Pedestrian groups in the closed loop (BatchEpisode(crowd=..., person_groups=...)): the set-up of
tests/test_gpu_episode_crowd.py (48 robots on global plans, 12 ticks, distance grids from the scenes' costmaps), here with
8 persons each, half of the walking ones in pairs and triples (scenes.crowd_groups). One eager episode is run once, with
records, and shared: the groups checker replays every tick's step from the recorded states, and the graph-replayed and
the three-shard episodes are compared with it bit for bit."""
import numpy as np
import pytest

import crowd_groups_ref as GR
import crowd_ref as CR
from nav2_social_mpc_controller_amd.params import CrowdGroupParams, CrowdParams, OptimizerParams, TrajectorizerParams

pytestmark = pytest.mark.gpu

B, N, TICKS = 48, 8, 12
CP, GP = CrowdParams(), CrowdGroupParams()


def setup():
    from nav2_social_mpc_controller_amd.episode import arc_plans
    from nav2_social_mpc_controller_amd.scenes import crowd_groups, make_scenes, uniform

    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    sc = make_scenes(prm, B, N)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    gid, wp, n_wp = crowd_groups(sc, K=2)
    kw = dict(plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=1.2, obstacles_from_costmap=True)
    crowd = dict(crowd=CP, person_waypoints=wp, person_n_waypoints=n_wp)
    return prm, sc, w_ref, kw, crowd, gid


@pytest.fixture(scope="module")
def eager():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode

    prm, sc, w_ref, kw, crowd, gid = setup()
    ep = BatchEpisode(prm, sc, w_ref, person_groups=gid, crowd_groups=GP, **kw, **crowd)
    start = ep.persons.cpu().numpy().copy()
    recs = [ep.tick(record=True) for _ in range(TICKS)]
    ep.synchronize()
    return dict(ep=ep, recs=recs, start=start, pose=ep.pose.cpu().numpy().copy(), persons=ep.persons.cpu().numpy().copy(),
                cursor=ep.person_cursor.cpu().numpy().copy(), sc=sc, prm=prm, wp=crowd["person_waypoints"],
                n_wp=crowd["person_n_waypoints"], gid=gid)


def test_every_tick_is_the_checkers_step_from_the_recorded_state(eager):
    ep, prm, gid = eager["ep"], eager["prm"], eager["gid"]
    grids = ep.od_indexes.cpu().numpy().view(np.uint32)
    origin = ep.od_origin.cpu().numpy()
    assert (gid >= 0).sum() >= B and np.array_equal(ep.person_groups.cpu().numpy(), gid)
    differs = 0
    for k, r in enumerate(eager["recs"]):
        args = (prm.dt, r.persons, r.cursor_before, r.robot_pose, r.cmd_vel, r.person_count, eager["wp"], eager["n_wp"])
        opts = dict(od_indexes=grids, od_origin=origin, od_resolution=ep.od_resolution, goal_radius=CP.goal_radius,
                    person_radius=CP.person_radius, desired_speed=CP.desired_speed, cyclic=CP.cyclic, robot_visible=CP.robot_visible)
        want = GR.step_batch(*args, group_id=gid, factors=(GP.factor_gaze, GP.factor_coherence, GP.factor_repulsion), **opts)
        CR.compare(r.persons_after, r.cursor_after, want[0], want[1], prm.dt, r.person_count, f"tick {k + 1}")
        if k == 0:
            plain = CR.step_batch(*args, **opts)
            differs = float(np.abs(plain[0][..., 2:4] - want[0][..., 2:4]).max())
        if k > 0:   # a tick starts from what the last one left
            assert np.array_equal(r.persons, eager["recs"][k - 1].persons_after) and np.array_equal(r.cursor_before, eager["recs"][k - 1].cursor_after)
    assert differs > 1e-3                                   # the group force acts in this episode


def test_graph_replay_and_three_shards_equal_the_eager_chain(eager):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode

    prm, sc, w_ref, kw, crowd, gid = setup()
    g = BatchEpisode(prm, sc, w_ref, person_groups=gid, **kw, **crowd)
    g.capture_graph()
    g.synchronize()
    assert np.array_equal(g.persons.cpu().numpy(), eager["start"]) and not g.person_cursor.cpu().numpy().any()   # warm-up undone
    assert np.array_equal(g.person_groups.cpu().numpy(), gid)
    for _ in range(TICKS):
        g.replay()
    g.synchronize()
    assert g.persons.cpu().numpy().tobytes() == eager["persons"].tobytes()
    assert g.person_cursor.cpu().numpy().tobytes() == eager["cursor"].tobytes()
    assert np.array_equal(g.pose.cpu().numpy(), eager["pose"])

    three = ShardedEpisode(prm, sc, w_ref, None, None, None, shards=3, graphs=True, person_groups=gid, crowd_groups=GP, **kw, **crowd)
    assert [p.B for p in three.parts] == [16, 16, 16]
    assert np.array_equal(three.gather("person_groups").cpu().numpy(), gid)
    for _ in range(TICKS):
        three.tick()
    assert three.gather("persons").cpu().numpy().tobytes() == eager["persons"].tobytes()
    assert three.gather("person_cursor").cpu().numpy().tobytes() == eager["cursor"].tobytes()
    assert np.array_equal(three.gather("pose").cpu().numpy(), eager["pose"])


def test_without_person_groups_the_episode_is_todays(eager):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode

    prm, sc, w_ref, kw, crowd, gid = setup()
    plain = BatchEpisode(prm, sc, w_ref, **kw, **crowd)
    assert plain.person_groups is None and not hasattr(plain, "crowd_group_params")
    none = BatchEpisode(prm, sc, w_ref, person_groups=np.full((B, N), -1), **kw, **crowd)   # ids that form no group
    for _ in range(TICKS):
        plain.tick()
        none.tick()
    plain.synchronize()
    # the plain episode's ticks are the plain checker's (tests/test_gpu_episode_crowd.py); every id < 0 is the same bit for bit
    assert none.persons.cpu().numpy().tobytes() == plain.persons.cpu().numpy().tobytes()
    assert none.person_cursor.cpu().numpy().tobytes() == plain.person_cursor.cpu().numpy().tobytes()
    assert np.array_equal(none.pose.cpu().numpy(), plain.pose.cpu().numpy())
    assert plain.persons.cpu().numpy().tobytes() != eager["persons"].tobytes()
    with pytest.raises(ValueError):
        BatchEpisode(prm, sc, w_ref, person_groups=gid, **kw)   # groups need a crowd
