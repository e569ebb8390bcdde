"""Closed-loop episodes whose global plans are smoothed where the planner walks them
(BatchEpisode(planner=GlobalPlanParams(smoother=PlanSmootherParams()), goal=...)): 7 robots on a 128 x 96 world with discs,
40 x 40 windows. ep.plan_raw is, bit for bit, the plan of the same episode without a smoother; ep.plan, ep.smooth_status,
ep.smooth_info and ep.smooth_change are the yardstick's (tests/plan_smoother_ref.py) on plan_raw and the world map; both hold
again after replan() from moved poses; three ticks run eagerly and from a captured graph and agree; without a smoother nothing
is allocated.

No assertion on how well the robots then drive."""
import numpy as np
import pytest

import plan_smoother_ref as R
from nav2_social_mpc_controller_amd.params import GlobalPlanParams, OptimizerParams, PlanSmootherParams, TrajectorizerParams

pytestmark = pytest.mark.gpu

B, N, SIZE, TICKS, L = 7, 2, 40, 3, 300
SP = PlanSmootherParams(max_its=200)
GP_RAW, GP = GlobalPlanParams(max_poses=L), GlobalPlanParams(max_poses=L, smoother=SP)
PLAN_STATE = ("plan", "plan_len", "plan_error")
SMOOTH_STATE = ("plan_raw", "smooth_status", "smooth_info", "smooth_change")
STATE = ("pose", "speed", "persons", "cmd_vel", "costmap", "costmap_origin", "plan", "plan_len", "plan_start")


def setup():
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world, uniform, world_goals
    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    world = make_world(128, 96, 0.05, seed=0x5EED0004, origin=(-1.3, 0.45))
    sc = scenes_in_world(prm, world, B, N, size_x=SIZE, size_y=SIZE, margin=1.2, people_reach=2.0)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    goal = world_goals(world, sc.pose0[:, :2], margin=0.8, min_dist=2.0)
    kw = dict(traj_params=tp, fov_angle=1.2, plan_window=(4.0, 10.0), obstacles_from_costmap=True, goal=goal, world=world)
    return prm, world, sc, w_ref, kw


def build(planner):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup()
    return BatchEpisode(prm, sc, w_ref, planner=planner, **kw), world


def host(ep, names):
    ep.synchronize()
    return {k: getattr(ep, k).cpu().numpy().copy() for k in names}


def state(ep):
    out = host(ep, STATE)
    out.update({"res_" + k: v.cpu().numpy().copy() for k, v in ep.res.items()})
    return out


def yardstick(world, raw, plan_len):
    c = dict(plan=raw, plan_len=plan_len, range=None, world=world.map, origin=np.asarray(world.origin, np.float64), res=world.resolution,
             w_data=SP.w_data, w_smooth=SP.w_smooth, tolerance=SP.tolerance, max_its=SP.max_its, refinement_num=SP.refinement_num,
             lethal_min_cost=GP.lethal_min_cost, allow_unknown=GP.allow_unknown)
    return R.run(c)


def check_smoothing(ep, world, raw_ep, what):
    """ep's raw plans are raw_ep's plans, and its plans the yardstick's on them."""
    got, raw = host(ep, PLAN_STATE + SMOOTH_STATE), host(raw_ep, PLAN_STATE)
    assert got["plan_raw"].tobytes() == raw["plan"].tobytes() and got["plan_len"].tobytes() == raw["plan_len"].tobytes(), what
    assert got["plan_error"].tobytes() == raw["plan_error"].tobytes() and not raw["plan_error"].any(), what
    want = yardstick(world, got["plan_raw"], got["plan_len"])
    for k, name in (("plan", "plan"), ("status", "smooth_status"), ("info", "smooth_info"), ("change", "smooth_change")):
        assert got[name].tobytes() == want[k].tobytes(), (what, k, got["smooth_status"], want["status"], got["smooth_info"].tolist(), want["info"].tolist())
    assert (want["status"] <= R.MAX_ITS).all() and (got["plan_len"] >= 20).all() and got["plan"].tobytes() != got["plan_raw"].tobytes(), what
    turn = [(R.turning(got["plan_raw"][b, :n]), R.turning(got["plan"][b, :n])) for b, n in enumerate(got["plan_len"])]
    print(what, "poses", got["plan_len"].tolist(), "sweeps", got["smooth_info"][:, 0].tolist(), "rejected", got["smooth_info"][:, 2].tolist(),
          "turning raw -> smoothed", [(round(a, 2), round(b, 2)) for a, b in turn])
    assert sum(b for _, b in turn) < sum(a for a, _ in turn)
    return got


@pytest.fixture(scope="module")
def pair():
    """The smoothed episode and the raw one beside it, after construction."""
    ep, world = build(GP)
    raw_ep, _ = build(GP_RAW)
    return dict(ep=ep, raw_ep=raw_ep, world=world)


def test_construction_smooths_the_plans_the_planner_walked(pair):
    ep, raw_ep = pair["ep"], pair["raw_ep"]
    assert ep.plan_raw.shape == ep.plan.shape == (B, L, 2) and ep.plan_raw.data_ptr() != ep.plan.data_ptr()
    assert ep.smooth_status.shape == (B,) and ep.smooth_info.shape == (B, 4) and ep.smooth_change.shape == (B,)
    assert ep.smooth_status.dtype == ep.smooth_info.dtype == ep.torch.int32 and ep.smooth_change.dtype == ep.torch.float64
    si = ep._c.smooth
    assert (si.B, si.L, si.on_device, si.world_x, si.world_y, si.world_shared, si.max_its, si.refinement_num) == (B, L, 1, 128, 96, 1, 200, 2)
    assert (si.lethal_min_cost, si.allow_unknown, si.resolution, si.w_data, si.w_smooth, si.tolerance) == (253, 0, 0.05, 0.2, 0.3, 1e-10)
    assert (si.world, si.world_origin, si.plan_len, si.range) == (ep.world_map.data_ptr(), ep.world_origin.data_ptr(), ep.plan_len.data_ptr(), None)
    assert not hasattr(raw_ep, "plan_raw") and not hasattr(raw_ep, "smooth_status") and not hasattr(raw_ep._c, "smooth")
    check_smoothing(ep, pair["world"], raw_ep, "construction")


def test_ticks_replan_and_graph_replay(pair):
    """Three eager ticks of the smoothed episode; replan() from the moved poses smooths the new walk (the raw episode, put on
    the same poses, walks the same raw plans); a second episode replays the three ticks from a captured graph and agrees."""
    ep, raw_ep, world = pair["ep"], pair["raw_ep"], pair["world"]
    addresses = [getattr(ep, k).data_ptr() for k in PLAN_STATE + SMOOTH_STATE]
    first = host(ep, ("plan", "plan_raw"))
    states = []
    for _ in range(TICKS):
        ep.tick()
        states.append(state(ep))
    assert host(ep, ("plan",))["plan"].tobytes() == first["plan"].tobytes()          # a tick leaves the plans alone
    moved = np.hypot(*(states[-1]["pose"][:, :2] - states[0]["pose"][:, :2]).T)
    assert (moved > 0.0).any()
    raw_ep.pose.copy_(ep.pose)
    ep.replan()
    raw_ep.replan()
    after = check_smoothing(ep, world, raw_ep, "replan")
    assert after["plan_raw"].tobytes() != first["plan_raw"].tobytes() and not host(ep, ("plan_start",))["plan_start"].any()
    assert addresses == [getattr(ep, k).data_ptr() for k in PLAN_STATE + SMOOTH_STATE]

    g, _ = build(GP)
    assert host(g, ("plan",))["plan"].tobytes() == first["plan"].tobytes()
    g.capture_graph()
    for k in range(TICKS):
        g.replay()
        got = state(g)
        for name, v in states[k].items():
            assert got[name].tobytes() == v.tobytes(), (k, name)
    g.replan()                                                    # between replays, on the capture stream, outside the graph
    g_after = host(g, PLAN_STATE + SMOOTH_STATE)
    for name in PLAN_STATE + SMOOTH_STATE:
        assert g_after[name].tobytes() == after[name].tobytes(), name
