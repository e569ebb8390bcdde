"""Closed-loop episodes whose global plans come from the world map (BatchEpisode(planner=GlobalPlanParams(), goal=...)): the
placement of tests/test_gpu_episode_world.py (48 robots with 4 persons each on the 256 x 192 world, 40 x 40 windows), the
goals of scenes.world_goals mapped onto 6 distinct ones by b % 6, 12 ticks.

Checked on the CPU with the reference rule (tests/global_plan_ref.py) on that world, and asserted again by `reference()`
below before anything runs on the device: all 48 robots find a goal candidate (no goal is the fallback cell), every
passable cell of the world is reachable from each of the 6 goals, all 48 starts are reachable, the plans have 22 to 125
poses (at stride 1 as many path cells; the b % 6 mapping hands a robot another robot's goal, so min_dist does not bind)
and the largest potential is 79,938. Hence every `error` is 0 and max_poses = 400 truncates nobody. (scenes.world_goals draws its
candidates in an order of this package's choosing, so these figures are this package's; they are recomputed, not copied.)

No assertion on how well the robots then drive."""
import dataclasses

import numpy as np
import pytest

import global_plan_ref as R
from nav2_social_mpc_controller_amd.params import CrowdParams, GlobalPlanParams, MetricsParams, OptimizerParams, TrajectorizerParams

pytestmark = pytest.mark.gpu

B, N, TICKS, SIZE, REPLAN_AT = 48, 4, 12, 40, 6
GP = GlobalPlanParams()


def setup():
    from nav2_social_mpc_controller_amd.scenes import crowd_waypoints, make_world, scenes_in_world, uniform, world_goals

    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    world = make_world(256, 192, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15))
    place = dict(margin=4.3, people_reach=2.5)
    sc = scenes_in_world(prm, world, B, N, size_x=SIZE, size_y=SIZE, **place)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    own = world_goals(world, sc.pose0[:, :2])
    goal = np.ascontiguousarray(own[np.arange(B) % 6])
    wp, n_wp = crowd_waypoints(scenes_in_world(prm, world, B, N, size_x=120, size_y=120, **place), K=2)
    kw = dict(traj_params=tp, fov_angle=1.2, plan_window=(4.0, 10.0), obstacles_from_costmap=True, metrics=MetricsParams(),
              crowd=CrowdParams(), person_waypoints=wp, person_n_waypoints=n_wp, goal=goal)
    return prm, world, sc, w_ref, kw, own


def reference_plans(world, fields, goals, robot_goal, pose):
    """(plan [B,400,2] with zero rows beyond plan_len, as the episode's buffer starts out; plan_len; error)."""
    return R.extract_plan(world.map, world.origin, world.resolution, fields, goals, robot_goal, pose, GP.max_poses, GP.stride,
                          plan=np.zeros((len(pose), GP.max_poses, 2)))


@pytest.fixture(scope="module")
def reference():
    """The reference's fields of the 6 goals and plans from the start poses, with the facts the docstring states."""
    from nav2_social_mpc_controller_amd.scenes import world_goals
    prm, world, sc, w_ref, kw, own = setup()
    far = world_goals(world, sc.pose0[:, :2], min_dist=1e3)[0]                   # the fallback cell's centre
    assert not (own == far).all(axis=1).any() and (np.hypot(*(own - sc.pose0[:, :2]).T) >= 3.0).all()
    goals, robot_goal = np.unique(kw["goal"], axis=0, return_inverse=True)
    robot_goal = np.asarray(robot_goal).reshape(B).astype(np.int32)
    assert len(goals) == 6
    fields, status = R.goal_fields(world.map, world.origin, world.resolution, goals)
    assert not status.any() and ((fields != R.UNREACHABLE) == R.passable(world.map, R.Cost())[None]).all()
    plan, plan_len, error = reference_plans(world, fields, goals, robot_goal, sc.pose0)
    print("plan poses", plan_len.min(), "..", plan_len.max(), "; largest potential", fields[fields != R.UNREACHABLE].max())
    assert not error.any() and (plan_len.min(), plan_len.max()) == (22, 125) and plan_len.max() < GP.max_poses
    assert fields[fields != R.UNREACHABLE].max() == 79938
    return dict(goals=goals, robot_goal=robot_goal, fields=fields, plan=plan, plan_len=plan_len)


def state(ep):
    names = ["pose", "speed", "persons", "person_cursor", "metrics_acc", "cmd_vel", "proj_error", "costmap", "costmap_origin", "costmap_cell",
             "plan", "plan_len", "plan_start"]
    out = {k: getattr(ep, k).cpu().numpy().copy() for k in names}
    out.update({"res_" + k: v.cpu().numpy().copy() for k, v in ep.res.items()})
    return out


def same_state(got, want, what):
    for k, v in want.items():
        assert R.same_bits(got[k], v), (what, k)


@pytest.fixture(scope="module")
def eager(reference):
    """The planner episode, run once with a replan before tick REPLAN_AT: its state after every tick, the poses it
    replanned from and the plans it then had."""
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw, _ = setup()
    ep = BatchEpisode(prm, sc, w_ref, world=world, planner=GP, **kw)
    first = {k: getattr(ep, k).cpu().numpy().copy() for k in ("plan", "plan_len", "plan_error", "robot_goal", "plan_goals", "goal_field", "goal_status")}
    states, replanned = [], None
    for k in range(TICKS):
        if k == REPLAN_AT:
            pose = ep.pose.cpu().numpy().copy()
            ep.replan()
            ep.synchronize()
            replanned = dict(pose=pose, plan=ep.plan.cpu().numpy().copy(), plan_len=ep.plan_len.cpu().numpy().copy(),
                             plan_error=ep.plan_error.cpu().numpy().copy(), plan_start=ep.plan_start.cpu().numpy().copy())
        ep.tick()
        ep.synchronize()
        states.append(state(ep))
    return dict(first=first, states=states, replanned=replanned)


def test_construction_computes_the_reference_fields_and_plans(eager, reference):
    first = eager["first"]
    assert R.same_bits(first["plan_goals"], reference["goals"]) and np.array_equal(first["robot_goal"], reference["robot_goal"])
    assert R.same_bits(first["goal_field"].view(np.uint32), reference["fields"]) and not first["goal_status"].any()
    assert not first["plan_error"].any() and np.array_equal(first["plan_len"], reference["plan_len"])
    assert R.same_bits(first["plan"], reference["plan"])


def test_planner_is_the_episode_given_the_reference_plans_tick_by_tick(eager, reference):
    """Up to the replan the planner episode is, bit for bit, the one handed the reference's plans as plan=; from the replan
    on, the one whose plans are swapped for the reference walk from the recorded poses at the same tick."""
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw, _ = setup()
    ep = BatchEpisode(prm, sc, w_ref, world=world, plan=reference["plan"], plan_len=reference["plan_len"], **kw)
    assert not hasattr(ep, "goal_field") and ep.planner is None
    for k in range(TICKS):
        if k == REPLAN_AT:
            pose = ep.pose.cpu().numpy().copy()
            assert R.same_bits(pose, eager["replanned"]["pose"])
            plan, plan_len, error = reference_plans(world, reference["fields"], reference["goals"], reference["robot_goal"], pose)
            assert not error.any()
            # replan() writes the first plan_len rows of the buffer and leaves the others: so does the yardstick
            merged = ep.plan.cpu().numpy().copy()
            for b in range(B):
                merged[b, :plan_len[b]] = plan[b, :plan_len[b]]
            assert R.same_bits(eager["replanned"]["plan"], merged) and np.array_equal(eager["replanned"]["plan_len"], plan_len)
            assert not eager["replanned"]["plan_error"].any() and not eager["replanned"]["plan_start"].any()
            ep.plan.copy_(ep.torch.from_numpy(merged).to(ep.dev))
            ep.plan_len.copy_(ep.torch.from_numpy(plan_len).to(ep.dev))
            ep.plan_start.zero_()
        ep.tick()
        ep.synchronize()
        same_state(state(ep), eager["states"][k], f"tick {k}")
    moved = np.hypot(*(eager["states"][-1]["pose"][:, :2] - sc.pose0[:, :2]).T)
    print("metres driven in 12 ticks: min %.3f max %.3f" % (moved.min(), moved.max()))
    assert not R.same_bits(eager["replanned"]["plan"], reference["plan"])      # the replan did change the plans


def test_three_shards_and_graph_replay_equal_the_eager_chain(eager):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode
    prm, world, sc, w_ref, kw, _ = setup()
    want = eager["states"][REPLAN_AT - 1]
    g = BatchEpisode(prm, sc, w_ref, world=world, planner=GP, **kw)
    g.capture_graph()
    for _ in range(REPLAN_AT):
        g.replay()
    g.synchronize()
    same_state(state(g), want, "graph")
    g.replan()                                                # between replays, on the capture stream, outside the graph
    for _ in range(TICKS - REPLAN_AT):
        g.replay()
    g.synchronize()
    same_state(state(g), eager["states"][-1], "graph after replan")

    three = ShardedEpisode(prm, sc, w_ref, None, None, None, shards=3, graphs=True, world=world, planner=GP, **kw)
    assert [p.B for p in three.parts] == [16, 16, 16] and all(p.planner is GP for p in three.parts)
    assert all(int(p.goal_field.shape[0]) == 6 for p in three.parts)          # b % 6: every shard of 16 has all six goals
    for _ in range(REPLAN_AT):
        three.tick()
    for k in ("pose", "persons", "person_cursor", "metrics_acc", "costmap", "costmap_cell", "plan", "plan_len", "plan_start"):
        assert R.same_bits(three.gather(k).cpu().numpy(), want[k]), k
    for k in ("cmds", "path", "status", "iterations"):
        assert R.same_bits(three.gather(k).cpu().numpy(), want["res_" + k]), k


def test_planner_none_is_the_episode_without_the_argument_and_misuse_is_refused(reference):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw, _ = setup()
    kw = dict(kw, plan=reference["plan"], plan_len=reference["plan_len"])
    plain, none = BatchEpisode(prm, sc, w_ref, world=world, **kw), BatchEpisode(prm, sc, w_ref, world=world, planner=None, **kw)
    for ep in (plain, none):
        assert ep.planner is None and not hasattr(ep._c, "extract")
        for name in ("goal_field", "goal_status", "plan_goals", "robot_goal", "plan_error"):
            assert not hasattr(ep, name), name
        with pytest.raises(ValueError):
            ep.replan()
    for k in range(3):
        a, b = plain.tick(record=True), none.tick(record=True)
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, dict):
                assert all(R.same_bits(x[n], y[n]) for n in x), (k, f.name)
            elif x is not None:
                assert R.same_bits(x, y), (k, f.name)
        same_state(state(none), state(plain), f"tick {k}")
    with pytest.raises(ValueError):                           # planner and plan
        BatchEpisode(prm, sc, w_ref, world=world, planner=GP, **kw)
    bare = {k: v for k, v in kw.items() if k not in ("plan", "plan_len")}
    with pytest.raises(ValueError):                           # planner without world
        BatchEpisode(prm, sc, w_ref, planner=GP, **bare)
    with pytest.raises(ValueError):                           # planner without goal
        BatchEpisode(prm, sc, w_ref, world=world, planner=GP, **dict(bare, goal=None))
    with pytest.raises(ValueError):                           # planner without traj_params
        BatchEpisode(prm, sc, w_ref, world=world, planner=GP, **dict(bare, traj_params=None))
