"""Closed-loop episodes whose robots perceive only the persons in line of sight (BatchEpisode(visibility=VisibilityParams())):
48 robots with 4 persons each on the 256 x 192 world, placed by scenes_in_world at its defaults, 40 x 40 windows, arc plans
with the plan window, the reactive crowd and metrics, 12 ticks. One eager episode is run once, with records, and shared.

Checked on the CPU with the reference rule (tests/visibility_ref.py) and asserted again below before anything is compared:
at the start 34 of the 192 persons are hidden from their robot (18 %); over the recorded ticks the share of hidden
person-ticks has to lie between 10 % and 50 %, or the comparisons would show little (on the MI355X: 401 of 2304, 17.4 %).
The field-of-view stage of people_to_status keeps, as the reference does, only persons on the robot's own window, 2 m wide
here, where hardly anybody is hidden: in this configuration the filter changes what people_to_status is handed, not yet
what it hands on.

No assertion on how well the robots then drive."""
import dataclasses

import numpy as np
import pytest

import visibility_ref as V
from nav2_social_mpc_controller_amd.params import CrowdParams, MetricsParams, OptimizerParams, TrajectorizerParams, VisibilityParams

pytestmark = pytest.mark.gpu

B, N, TICKS, SIZE, FOV = 48, 4, 12, 40, 1.2
VP = VisibilityParams()


def setup():
    from nav2_social_mpc_controller_amd.episode import arc_plans
    from nav2_social_mpc_controller_amd.scenes import crowd_waypoints, make_world, scenes_in_world, uniform

    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    world = make_world(256, 192, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15))
    sc = scenes_in_world(prm, world, B, N, size_x=SIZE, size_y=SIZE)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    wp, n_wp = crowd_waypoints(scenes_in_world(prm, world, B, N, size_x=120, size_y=120), K=2)
    kw = dict(plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=FOV, plan_window=(4.0, 10.0), obstacles_from_costmap=True,
              metrics=MetricsParams(), crowd=CrowdParams(), person_waypoints=wp, person_n_waypoints=n_wp)
    return prm, world, sc, w_ref, kw


def reference(world, pose, persons, count, vp=VP):
    """(visible with zero rows beyond the counts, as the episode's buffer starts out; visible_count; seen with zeros)."""
    return V.visible_people(world.map, world.origin, world.resolution, pose, persons, count, vp.max_range, vp.occlusion_min_cost,
                            vp.unknown_occludes, visible=np.zeros(persons.shape), seen=np.zeros(persons.shape[:2], np.uint8))


def state(ep):
    names = ["pose", "speed", "persons", "person_cursor", "metrics_acc", "cmd_vel", "proj_error", "costmap", "costmap_origin", "costmap_cell",
             "people", "has_people"]
    names += ["seen_persons", "seen_count", "person_seen"] if ep.visibility is not None else []
    out = {k: getattr(ep, k).cpu().numpy().copy() for k in names}
    out.update({"res_" + k: v.cpu().numpy().copy() for k, v in ep.res.items()})
    return out


def same_state(got, want, what):
    for k, v in want.items():
        assert V.same_bits(got[k], v), (what, k)


def same_records(a, b, what):
    """Every array the record `a` has is, bit for bit, in `b`."""
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, dict):
            assert all(V.same_bits(x[n], y[n]) for n in x), (what, f.name)
        elif x is not None:
            assert V.same_bits(x, y), (what, f.name)


@pytest.fixture(scope="module")
def eager():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup()
    ep = BatchEpisode(prm, sc, w_ref, world=world, visibility=VP, **kw)
    zero = {k: getattr(ep, k).cpu().numpy().copy() for k in ("seen_persons", "seen_count", "person_seen")}
    assert all(not v.any() for v in zero.values()) and zero["person_seen"].dtype == np.uint8 and zero["seen_persons"].shape == (B, N, 5)
    addresses = [getattr(ep, k).data_ptr() for k in zero]
    recs, states = [], []
    for _ in range(TICKS):
        recs.append(ep.tick(record=True))
        ep.synchronize()
        states.append(state(ep))
    assert addresses == [getattr(ep, k).data_ptr() for k in zero]
    assert (ep._c.people.people, ep._c.people.count) == (ep.seen_persons.data_ptr(), ep.seen_count.data_ptr())
    return dict(ep=ep, recs=recs, states=states, world=world, sc=sc)


def test_every_tick_has_the_reference_flags_counts_and_rows_and_a_share_is_hidden(eager):
    world, recs = eager["world"], eager["recs"]
    hidden = valid = 0
    for k, r in enumerate(recs):
        vis, n, seen = reference(world, r.robot_pose, r.persons, r.person_count)
        below = np.arange(N)[None, :] < np.clip(r.person_count, 0, N)[:, None]
        assert r.person_seen.dtype == np.uint8 and np.array_equal(r.person_seen[below], seen[below]), k
        assert np.array_equal(r.seen_count, n) and r.seen_count.dtype == np.int32, k
        rows = np.arange(N)[None, :] < n[:, None]
        assert V.same_bits(r.seen_persons[rows], vis[rows]), k
        hidden, valid = hidden + int((seen[below] == V.HIDDEN).sum()), valid + int(below.sum())
        if k == 0:
            print("tick 0: hidden", int((seen[below] == V.HIDDEN).sum()), "of", int(below.sum()))
            assert (int((seen[below] == V.HIDDEN).sum()), int(below.sum())) == (34, 192)
            assert set(seen[below]) == {V.HIDDEN, V.SEEN}                   # nobody is 10 m away or not finite here
    print("hidden person-ticks", hidden, "of", valid)
    # the condition, from the reference alone: without it the comparisons above could pass on a floor that hides nobody
    assert 0.10 * valid <= hidden <= 0.50 * valid


def test_people_to_status_reads_the_compacted_rows(eager):
    """The recorded init_people is solver.people_to_status (field-of-view filter included) on the reference's compacted rows
    of the tick, with the tick's windows."""
    world, s = eager["world"], eager["ep"].solver
    fewer = 0
    for k, r in enumerate(eager["recs"]):
        vis, n, _ = reference(world, r.robot_pose, r.persons, r.person_count)
        want, has = s.people_to_status(vis, n, N, robot_pose=r.robot_pose, fov_angle=FOV, costmap_origin=r.costmap_origin, size_x=SIZE,
                                       size_y=SIZE, resolution=world.resolution)
        assert V.same_bits(r.init_people, want) and np.array_equal(r.has_people, has), k
        # the compaction is what is handed on: without the field-of-view stage (which, as in the reference, also drops every
        # person off the robot's 2 m window, hidden or not) the status rows of the compacted and of all persons differ
        fewer += not V.same_bits(s.people_to_status(vis, n, N)[0], s.people_to_status(r.persons, r.person_count, N)[0])
    assert fewer == TICKS
    # the world keeps every person: the crowd step moved them all, hidden or not
    first, last = eager["recs"][0], eager["recs"][-1]
    assert np.array_equal(last.person_count, first.person_count) and not V.same_bits(last.persons_after, first.persons)


def test_graph_replay_and_three_shards_equal_the_eager_chain(eager):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode
    prm, world, sc, w_ref, kw = setup()
    want = eager["states"][-1]
    g = BatchEpisode(prm, sc, w_ref, world=world, visibility=VP, **kw)
    g.capture_graph()
    for _ in range(TICKS):
        g.replay()
    g.synchronize()
    same_state(state(g), want, "graph")

    three = ShardedEpisode(prm, sc, w_ref, None, None, None, shards=3, graphs=True, world=world, visibility=VP, **kw)
    assert [p.B for p in three.parts] == [16, 16, 16] and all(p.visibility is VP for p in three.parts)
    for _ in range(TICKS):
        three.tick()
    for k in ("pose", "persons", "person_cursor", "metrics_acc", "costmap", "costmap_cell", "people", "seen_persons", "seen_count", "person_seen"):
        assert V.same_bits(three.gather(k).cpu().numpy(), want[k]), k
    for k in ("cmds", "path", "status", "iterations"):
        assert V.same_bits(three.gather(k).cpu().numpy(), want["res_" + k]), k


def test_visibility_none_and_a_filter_that_hides_nobody_are_the_plain_episode(eager):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup()
    plain, none = BatchEpisode(prm, sc, w_ref, world=world, **kw), BatchEpisode(prm, sc, w_ref, world=world, visibility=None, **kw)
    open_eyes = VisibilityParams(max_range=1000.0, occlusion_min_cost=255, unknown_occludes=False)     # no cell occludes
    nobody = BatchEpisode(prm, sc, w_ref, world=world, visibility=open_eyes, **kw)
    for ep in (plain, none):
        assert ep.visibility is None and not hasattr(ep._c, "visibility")
        assert (ep._c.people.people, ep._c.people.count) == (ep.persons.data_ptr(), ep.person_count.data_ptr())
        for name in ("seen_persons", "seen_count", "person_seen"):
            assert not hasattr(ep, name), name
    for k in range(TICKS):
        a, b, c = plain.tick(record=True), none.tick(record=True), nobody.tick(record=True)
        assert a.person_seen is None and a.seen_count is None and a.seen_persons is None
        same_records(a, b, f"visibility=None, tick {k}")
        same_records(a, c, f"nobody hidden, tick {k}")
        below = np.arange(N)[None, :] < np.clip(c.person_count, 0, N)[:, None]
        assert (c.person_seen[below] == V.SEEN).all() and np.array_equal(c.seen_count, np.clip(c.person_count, 0, N))
        same_state(state(none), state(plain), f"tick {k}")
        same_state({k_: v for k_, v in state(nobody).items()}, state(plain), f"nobody hidden, tick {k}")
    assert any((r.seen_count < np.clip(r.person_count, 0, N)).any() for r in eager["recs"])   # the default filter does hide
    with pytest.raises(ValueError):                                         # visibility without world
        BatchEpisode(prm, sc, w_ref, visibility=VP, **kw)
    with pytest.raises(ValueError):                                         # a range beyond 32768 cells
        BatchEpisode(prm, sc, w_ref, world=world, visibility=VisibilityParams(max_range=2000.0), **kw)
