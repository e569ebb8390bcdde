"""Episode metrics in the closed loop (BatchEpisode(metrics=...)): 48 robots with 4 agents each on global plans, half of them
short enough to be driven to their end within the 12 ticks, distance grids from the scenes' costmaps. One eager episode is
run once, with records, and shared: the checker replays its recorded post-move states, and the episode without
metrics, the graph-replayed one and the three-shard one are compared with it bit for bit."""
import numpy as np
import pytest

import metrics_ref as R
from nav2_social_mpc_controller_amd.params import MetricsParams, OptimizerParams, TrajectorizerParams

pytestmark = pytest.mark.gpu

B, N, TICKS = 48, 4, 12
MP = MetricsParams()
I = R.I


def setup():
    from nav2_social_mpc_controller_amd.episode import arc_plans
    from nav2_social_mpc_controller_amd.scenes import make_scenes, uniform

    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    sc = make_scenes(prm, B, N)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    short = np.arange(B) % 2 == 1
    # plans of 6 .. 12 poses, 0.05 m apart: 0.25 .. 0.55 m to drive at up to 0.03 m per tick; goal_tolerance 0.25
    plan_len = np.where(short, 6 + 2 * ((np.arange(B) // 2) % 4), plan_len).astype(np.int32)
    kw = dict(plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=1.2, obstacles_from_costmap=True)
    return prm, sc, w_ref, kw, plan[np.arange(B), plan_len - 1]


@pytest.fixture(scope="module")
def eager():
    """The eager single-chain episode with metrics, ticked TICKS times with records."""
    from nav2_social_mpc_controller_amd.episode import BatchEpisode

    prm, sc, w_ref, kw, goal = setup()
    ep = BatchEpisode(prm, sc, w_ref, metrics=MP, **kw)
    assert np.array_equal(ep.goal.cpu().numpy(), goal)   # default goal in plan mode: the last pose of each plan
    recs = [ep.tick(record=True) for _ in range(TICKS)]
    ep.synchronize()
    out = dict(ep=ep, recs=recs, acc=ep.metrics(), pose=ep.pose.cpu().numpy().copy(), cmd_vel=ep.cmd_vel.cpu().numpy().copy(),
               res={k: v.cpu().numpy().copy() for k, v in ep.res.items()}, goal=goal, sc=sc, prm=prm)
    return out


def test_checker_over_the_recorded_states_reproduces_the_metrics(eager):
    ep, sc = eager["ep"], eager["sc"]
    grids = ep.od_distances.cpu().numpy()
    assert grids.dtype == np.float32 and grids.shape == (B, sc.size_y, sc.size_x)
    acc = np.zeros((B, R.NCOLS))
    for r in eager["recs"]:
        assert r.pose_after is not None and r.persons_after.shape == (B, N, 5)
        acc = R.update(acc, MP, eager["prm"].dt, r.pose_after, r.cmd_vel, r.persons_after, r.person_count, eager["goal"], grids,
                       sc.costmap_origin, ep.od_resolution, r.result["status"], r.cmd_source)
    got = eager["acc"]
    R.compare(got, acc, f"episode, {TICKS} ticks")
    ttg = got[:, I["time_to_goal"]]
    print("arrived:", int((ttg >= 0).sum()), "of", B, "samples:", np.unique(got[:, I["samples"]]).tolist())
    assert (ttg >= 0).any() and (ttg < 0).any()                      # some robots arrive, the long plans do not end
    assert (got[ttg < 0, I["samples"]] == TICKS).all() and (got[ttg >= 0, I["samples"]] * eager["prm"].dt == ttg[ttg >= 0]).all()
    assert (got[:, I["people_samples"]] > 0).any() and (got[:, I["social_work"]] > 0).any()
    assert (got[:, I["min_clearance"]] < np.inf).any() and (got[:, I["path_length"]] > 0).any()
    from nav2_social_mpc_controller_amd.solver import summarize_metrics
    s = summarize_metrics(got, eager["prm"].dt)
    assert np.array_equal(s["success"], ttg >= 0)


def test_metrics_do_not_change_the_episode(eager):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode

    prm, sc, w_ref, kw, _ = setup()
    plain = BatchEpisode(prm, sc, w_ref, **kw)
    assert not hasattr(plain, "metrics_acc") and not hasattr(plain, "od_distances")   # nothing allocated
    for _ in range(TICKS):
        plain.tick()
    plain.synchronize()
    assert np.array_equal(plain.pose.cpu().numpy(), eager["pose"])
    assert np.array_equal(plain.cmd_vel.cpu().numpy(), eager["cmd_vel"])
    for k, v in eager["res"].items():
        assert np.array_equal(plain.res[k].cpu().numpy(), v, equal_nan=True), k
    with pytest.raises(ValueError):
        plain.metrics()


def test_graph_replay_and_three_shards_equal_the_eager_chain(eager):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode

    prm, sc, w_ref, kw, goal = setup()
    g = BatchEpisode(prm, sc, w_ref, metrics=MP, **kw)
    g.capture_graph()
    g.synchronize()
    assert not g.metrics_acc.cpu().numpy().any()          # the warm-up tick left no sample behind
    for _ in range(TICKS):
        g.replay()
    assert g.metrics().tobytes() == eager["acc"].tobytes()
    assert np.array_equal(g.pose.cpu().numpy(), eager["pose"])

    three = ShardedEpisode(prm, sc, w_ref, None, None, None, shards=3, graphs=True, metrics=MP, goal=goal, **kw)
    assert [p.B for p in three.parts] == [16, 16, 16]
    assert not three.gather("metrics_acc").cpu().numpy().any()
    for _ in range(TICKS):
        three.tick()
    assert three.gather("metrics_acc").cpu().numpy().tobytes() == eager["acc"].tobytes()
    assert np.array_equal(three.gather("pose").cpu().numpy(), eager["pose"])
