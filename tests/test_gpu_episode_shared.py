"""Closed-loop episodes in one shared world (BatchEpisode(shared=SharedWorldParams(), pool=...)): 48 robots and a pool of 96
pedestrians (scenes.shared_pool) on a 512 x 384-cell floor (25.6 m x 19.2 m), 120 x 120 windows, plans from the world's goal
fields, the line-of-sight filter and metrics on, 12 ticks. Robots 0 and 1 are started 2 m apart, facing each other, with a
free sight line. One eager episode is run once, with records, and shared.

Checked on the CPU with the reference rule (tests/nearest_ref.py) and asserted again by `setup()` before anything runs on
the device: at the start robot 1 is among robot 0's N = 8 nearest agents and robot 0 among robot 1's, every robot has
more than N agents within the 10 m range (the cut to the nearest N binds everywhere) and at least 48 of the 384 perceived
rows are other robots.

No assertion on how well the robots then drive."""
import dataclasses

import numpy as np
import pytest

import metrics_ref as MR
import nearest_ref as R
import visibility_ref as V
from nav2_social_mpc_controller_amd.params import (CrowdParams, GlobalPlanParams, MetricsParams, OptimizerParams, SharedWorldParams,
                                                   TrajectorizerParams, VisibilityParams)

pytestmark = pytest.mark.gpu

B, N, M, TICKS, SIZE, FOV = 48, 8, 96, 12, 120, 1.2
VP, SP, MP = VisibilityParams(), SharedWorldParams(), MetricsParams()
SELF = np.arange(M, M + B, dtype=np.int32)


def setup(people_present=True):
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world, shared_pool, uniform, world_goals

    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    world = make_world(512, 384, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15))
    sc = scenes_in_world(prm, world, B, N, size_x=SIZE, size_y=SIZE, people_present=people_present)
    # robot 1 stands 2 m from robot 0, the two facing each other: the first of 16 bearings whose far end is a free cell in sight
    for k in range(16):
        ang = 2.0 * np.pi * k / 16.0
        spot = sc.pose0[0, :2] + 2.0 * np.array([np.cos(ang), np.sin(ang)])
        cell = np.floor((spot - world.origin) / world.resolution).astype(int)
        if world.map[cell[1], cell[0]] == 0 and V.classify(world.map, world.origin, world.resolution, sc.pose0[0, :2], spot, 10.0) == V.SEEN:
            break
    else:
        raise AssertionError("no free spot 2 m from robot 0")
    sc.pose0[0, 2], sc.pose0[1] = ang, [spot[0], spot[1], ang - np.pi if ang > 0 else np.pi]
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    goal = np.ascontiguousarray(world_goals(world, sc.pose0[:, :2])[np.arange(B) % 6])
    pool = shared_pool(world, M)
    kw = dict(traj_params=tp, fov_angle=FOV, plan_window=(4.0, 10.0), obstacles_from_costmap=True, metrics=MP, goal=goal,
              planner=GlobalPlanParams(), visibility=VP, world=world)
    # the facts of the docstring, from the reference alone
    table = np.concatenate([pool, np.concatenate([sc.pose0[:, :2], np.zeros((B, 3))], axis=1)])
    ok, _ = R.qualifying(table, sc.pose0, SP.max_range, SELF)
    _, count, source = R.nearest_people(table, sc.pose0, N, SP.max_range, SELF)
    assert M + 1 in source[0] and M in source[1]
    assert (ok.sum(axis=1) > N).all() and (count == N).all() and (source >= M).sum() >= B
    return prm, world, sc, w_ref, kw, pool


def gathered(agents, pose):
    """The reference's gather, with zero rows and sources -1 beyond the counts."""
    return R.nearest_people(agents, pose, N, SP.max_range, SELF, people=np.zeros((B, N, 5)), source=np.full((B, N), -1, np.int32))


def state(ep):
    names = ["pose", "speed", "persons", "person_count", "metrics_acc", "cmd_vel", "proj_error", "costmap", "costmap_origin",
             "costmap_cell", "people", "has_people", "plan", "plan_len", "plan_start"]
    names += ["agents", "seen_persons", "seen_count"] if ep.shared is not None else []
    out = {k: getattr(ep, k).cpu().numpy().copy() for k in names}
    out.update({"res_" + k: v.cpu().numpy().copy() for k, v in ep.res.items()})
    return out


def same_state(got, want, what):
    for k, v in want.items():
        assert V.same_bits(got[k], v) if v.dtype == np.float64 else np.array_equal(got[k], v), (what, k)


def same_records(a, b, what):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, dict):
            assert all(np.array_equal(x[n], y[n], equal_nan=True) for n in x), (what, f.name)
        elif x is not None:
            assert np.array_equal(x, y, equal_nan=True), (what, f.name)


@pytest.fixture(scope="module")
def eager():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw, pool = setup()
    ep = BatchEpisode(prm, sc, w_ref, shared=SP, pool=pool, **kw)
    assert ep.agents.shape == (M + B, 5) and ep.persons.shape == (B, N, 5) and ep.person_source.shape == (B, N)
    assert np.array_equal(ep.agent_self.cpu().numpy(), SELF) and not ep.persons.cpu().numpy().any()
    assert ep.nearest_workspace.numel() == ep.solver.nearest_workspace_bytes(M + B, *ep.shared_grid[:2]) > 0
    names = ("agents", "agent_self", "persons", "person_count", "person_source", "nearest_workspace")
    addresses = [getattr(ep, k).data_ptr() for k in names]
    recs, states = [], []
    for _ in range(TICKS):
        recs.append(ep.tick(record=True))
        ep.synchronize()
        states.append(state(ep))
    assert addresses == [getattr(ep, k).data_ptr() for k in names]
    return dict(ep=ep, recs=recs, states=states, world=world, sc=sc, pool=pool, prm=prm, goal=kw["goal"], acc=ep.metrics())


def test_every_ticks_gather_is_the_reference_on_the_recorded_table(eager):
    recs, dt = eager["recs"], eager["prm"].dt
    cut = others = 0
    for k, r in enumerate(recs):
        # the table: the pool, then the robots as persons
        assert r.agents.shape == (M + B, 5) and r.agents_after.shape == (M + B, 5)
        assert V.same_bits(r.agents[:M], eager["pool"] if k == 0 else recs[k - 1].agents_after[:M]), k
        assert V.same_bits(r.agents_after[:M, 0:2], r.agents[:M, 0:2] + r.agents[:M, 2:4] * dt) and V.same_bits(r.agents_after[:M, 2:], r.agents[:M, 2:]), k
        for table, pose, speed in ((r.agents, r.robot_pose, r.speed), (r.agents_after, r.pose_after, r.cmd_vel)):
            assert V.same_bits(table[M:, 0:2], pose[:, 0:2]) and V.same_bits(table[M:, 4], speed[:, 1]), k
            want = speed[:, 0:1] * np.stack([np.cos(pose[:, 2]), np.sin(pose[:, 2])], axis=1)
            assert np.abs(table[M:, 2:4] - want).max() <= 1e-12, k
        # what the tick's chain read, and what its metrics sample read
        for table, pose, persons, count, source in ((r.agents, r.robot_pose, r.persons, r.person_count, r.person_source),
                                                    (r.agents_after, r.pose_after, r.persons_after, None, None)):
            want, n, src = gathered(table, pose)
            rows = np.arange(N)[None, :] < n[:, None]
            assert V.same_bits(persons[rows], want[rows]), k
            if count is not None:
                assert np.array_equal(count, n) and count.dtype == np.int32 and np.array_equal(source[rows], src[rows]), k
                cut += int((R.qualifying(table, pose, SP.max_range, SELF)[0].sum(axis=1) > N).sum())
                others += int((src[rows] >= M).sum())
    print("robot-ticks where the cut to N binds:", cut, "; robots among the perceived rows:", others)
    assert cut > 0 and others > 0
    assert V.same_bits(eager["states"][-1]["agents"], recs[-1].agents_after)


def test_people_to_status_reads_the_gathered_rows_after_the_line_of_sight_filter(eager):
    world, s = eager["world"], eager["ep"].solver
    for k, r in enumerate(eager["recs"]):
        rows, n, _ = gathered(r.agents, r.robot_pose)
        vis, m, seen = V.visible_people(world.map, world.origin, world.resolution, r.robot_pose, rows, n, VP.max_range, VP.occlusion_min_cost,
                                        VP.unknown_occludes, visible=np.zeros(rows.shape), seen=np.zeros(rows.shape[:2], np.uint8))
        assert np.array_equal(r.seen_count, m), k
        want, has = s.people_to_status(vis, m, N, robot_pose=r.robot_pose, fov_angle=FOV, costmap_origin=r.costmap_origin, size_x=SIZE,
                                       size_y=SIZE, resolution=world.resolution)
        assert V.same_bits(r.init_people, want) and np.array_equal(r.has_people, has), k


def test_two_robots_facing_each_other_perceive_each_other_at_tick_0(eager):
    r = eager["recs"][0]
    assert abs(np.hypot(*(r.robot_pose[0, :2] - r.robot_pose[1, :2])) - 2.0) < 1e-9
    for me, other in ((0, 1), (1, 0)):
        assert M + other in r.person_source[me, :r.person_count[me]]
        valid = r.init_people[me][r.init_people[me][:, 3] != -1.0]
        assert r.has_people[me] and any(V.same_bits(row[0:2], r.robot_pose[other, 0:2]) for row in valid), (me, r.init_people[me])


def test_the_metrics_are_the_references_on_the_gathers_after_the_move(eager):
    ep, world = eager["ep"], eager["world"]
    grid = ep.od_distances.cpu().numpy()
    assert grid.shape == (1, world.cells_y, world.cells_x)
    acc = np.zeros((B, MR.NCOLS))
    for r in eager["recs"]:
        people, count, _ = gathered(r.agents_after, r.pose_after)
        acc = MR.update(acc, MP, eager["prm"].dt, r.pose_after, r.cmd_vel, people, count, eager["goal"], grid[0], world.origin,
                        ep.od_resolution, r.result["status"], r.cmd_source)
    MR.compare(eager["acc"], acc, f"shared world, {TICKS} ticks")
    assert (eager["acc"][:, MR.I["people_samples"]] > 0).all() and (eager["acc"][:, MR.I["social_work"]] > 0).any()


def test_graph_replay_equals_the_eager_chain(eager):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw, pool = setup()
    g = BatchEpisode(prm, sc, w_ref, shared=SP, pool=pool, **kw)
    g.capture_graph()
    g.synchronize()
    assert not g.metrics_acc.cpu().numpy().any() and V.same_bits(g.agents[:M].cpu().numpy(), pool)   # the warm-up tick left nothing behind
    for _ in range(TICKS):
        g.replay()
    g.synchronize()
    same_state(state(g), eager["states"][-1], "graph")
    assert np.array_equal(g.person_source.cpu().numpy(), eager["ep"].person_source.cpu().numpy())


def test_shared_none_is_the_plain_episode_and_the_refusals():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw, pool = setup()
    plain, none = BatchEpisode(prm, sc, w_ref, **kw), BatchEpisode(prm, sc, w_ref, shared=None, pool=None, **kw)
    for ep in (plain, none):
        assert ep.shared is None and not hasattr(ep._c, "nearest")
        for name in ("agents", "agent_self", "person_source", "nearest_workspace", "shared_grid"):
            assert not hasattr(ep, name), name
        assert ep.person_count.cpu().numpy().sum() == B * N                  # the scenes' own people
    for k in range(4):
        a, b = plain.tick(record=True), none.tick(record=True)
        assert a.agents is None and a.person_source is None and a.agents_after is None
        same_records(a, b, f"tick {k}")
        same_state(state(none), state(plain), f"tick {k}")
    for bad in (dict(shared=SP, pool=pool, world=None), dict(pool=pool), dict(shared=SP, crowd=CrowdParams()),
                dict(shared=SP, person_speed=np.ones((B, N))), dict(shared=SP, person_groups=np.zeros((B, N), np.int32)),
                dict(shared=SP, person_waypoints=np.zeros((B, N, 2, 2)), person_n_waypoints=np.ones((B, N), np.int32))):
        if "world" in bad:
            args = {k: v for k, v in kw.items() if k not in ("world", "planner", "visibility")}
            bad = {k: v for k, v in bad.items() if k != "world"}
        else:
            args = kw
        with pytest.raises(ValueError):
            BatchEpisode(prm, sc, w_ref, **args, **bad)


def test_a_fleet_without_pedestrians_and_without_mutual_perception_solves_scenes_without_people():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw, _ = setup()
    alone = BatchEpisode(prm, sc, w_ref, shared=SharedWorldParams(robots_as_people=False), pool=None, **kw)
    assert alone.agents.shape == (0, 5) and (alone.agent_self.cpu().numpy() == -1).all()
    _, _, empty_sc, _, _, _ = setup(people_present=False)
    assert V.same_bits(empty_sc.pose0, sc.pose0) and not empty_sc.has_people.any()
    empty = BatchEpisode(prm, empty_sc, w_ref, **kw)
    for k in range(4):
        a, b = alone.tick(record=True), empty.tick(record=True)
        assert not a.person_count.any() and not a.has_people.any() and not b.has_people.any(), k
        for name in ("pose", "speed", "cmd_vel", "metrics_acc", "people", "has_people", "plan", "plan_len", "costmap"):
            assert np.array_equal(getattr(alone, name).cpu().numpy(), getattr(empty, name).cpu().numpy(), equal_nan=True), (k, name)
        for name, v in alone.res.items():
            assert np.array_equal(v.cpu().numpy(), empty.res[name].cpu().numpy(), equal_nan=True), (k, name)
    # the fleet alone, perceiving each other: robots only in the table
    fleet = BatchEpisode(prm, sc, w_ref, shared=SP, pool=None, **kw)
    r = fleet.tick(record=True)
    want, n, src = R.nearest_people(r.agents, r.robot_pose, N, SP.max_range, np.arange(B, dtype=np.int32), people=np.zeros((B, N, 5)))
    assert r.agents.shape == (B, 5) and np.array_equal(r.person_count, n) and n.min() >= 1
    assert V.same_bits(r.persons[np.arange(N)[None, :] < n[:, None]], want[np.arange(N)[None, :] < n[:, None]])
