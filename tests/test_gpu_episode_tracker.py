"""Closed-loop episodes whose controller is handed tracks (BatchEpisode(visibility=..., tracker=TrackerParams())):
test_gpu_episode_sensed.py's 12 robots with 4 private persons each, 80 x 80 windows on the 256 x 192 world, arc plans, with
the line-of-sight filter in front of the tracker, 8 recorded ticks. Every tick's tracker state and outputs are the
yardstick's (tests/tracker_ref.py) on that tick's recorded detections, pose and state; the tick's init_people are
people_to_status of the tracked rows; graph replay equals the eager ticks; tracker=None is the plain episode.

And one constructed scene: a standing robot and one pedestrian at a constant 1.2 m/s who is in sight for 28 ticks and then
behind a wall. It is first checked with the yardsticks alone on the CPU (tests/visibility_ref.py, tests/tracker_ref.py):
while hidden, seen_count is 0 and the tracked row persists for max_missed ticks, then disappears; the coasted position
stays within 1 cm of the pedestrian's true one (an alpha-beta filter with the defaults has 3e-4 m/s of velocity error left
after 20 updates at this speed: 0.3 mm over 20 coasted ticks), and the estimated speed is within 1 % of 1.2 m/s at the
moment of occlusion. Then the episode's records are held against the same yardsticks.

No assertion on how well the robots then drive."""
import dataclasses

import numpy as np
import pytest

import tracker_ref as R
import visibility_ref as V
from nav2_social_mpc_controller_amd.params import OptimizerParams, TrackerParams, TrajectorizerParams, VisibilityParams
from test_gpu_episode_sensed import B, FOV, N, SIZE, setup

pytestmark = pytest.mark.gpu

TICKS = 8
VP, TP = VisibilityParams(), TrackerParams()
STATE = ("pose", "speed", "persons", "person_count", "cmd_vel", "costmap", "costmap_origin", "costmap_cell", "people", "has_people",
         "seen_persons", "seen_count", "person_seen")
TRACKER_STATE = ("tracks", "track_meta", "track_next_id", "tracked_persons", "tracked_count", "tracked_source")


def ref_params(prm, tp=TP, Np=N):
    return R.params(alpha=tp.alpha, beta=tp.beta, gate=tp.gate, confirm_hits=tp.confirm_hits, max_missed=tp.max_missed, slots=tp.slots,
                    dt=prm.dt, Np=Np)


def build(tracker=TP):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup("private")
    return BatchEpisode(prm, sc, w_ref, visibility=VP, tracker=tracker, **kw), prm, world


def state(ep):
    names = STATE + (TRACKER_STATE if ep.tracker is not None else ())
    out = {k: getattr(ep, k).cpu().numpy().copy() for k in names}
    out.update({"res_" + k: v.cpu().numpy().copy() for k, v in ep.res.items()})
    return out


@pytest.fixture(scope="module")
def eager():
    ep, prm, world = build()
    zero = {k: getattr(ep, k).cpu().numpy().copy() for k in TRACKER_STATE}
    assert all(not v.any() for v in zero.values())
    assert zero["tracks"].shape == (B, TP.slots, 4) and zero["track_meta"].shape == (B, TP.slots, 4) and zero["track_next_id"].shape == (B,)
    assert zero["tracked_persons"].shape == (B, N, 5) and zero["tracked_source"].shape == (B, N, 2)
    assert all(zero[k].dtype == np.int32 for k in ("track_meta", "track_next_id", "tracked_count", "tracked_source"))
    c = ep._c
    assert (c.tracker.detections, c.tracker.det_count) == (ep.seen_persons.data_ptr(), ep.seen_count.data_ptr())
    assert (c.people.people, c.people.count) == (ep.tracked_persons.data_ptr(), ep.tracked_count.data_ptr())
    assert (c.tracker.Nd, c.tracker.Nt, c.tracker.Np, c.tracker.dt, c.tracker.gain) == (N, TP.slots, N, prm.dt, TP.gain(prm.dt))
    addresses = [getattr(ep, k).data_ptr() for k in TRACKER_STATE]
    recs, states = [], []
    for _ in range(TICKS):
        timing = {}
        recs.append(ep.tick(record=True, timing=timing))
        ep.synchronize()
        assert timing["tracker_ms"] > 0.0
        states.append(state(ep))
    assert addresses == [getattr(ep, k).data_ptr() for k in TRACKER_STATE]
    return dict(ep=ep, recs=recs, states=states, world=world, prm=prm)


def test_every_ticks_tracks_and_rows_are_the_yardsticks(eager):
    p = ref_params(eager["prm"])
    carried = R.zero_state(B, TP.slots)
    people, source = np.zeros((B, N, 5)), np.zeros((B, N, 2), np.int32)
    handed = hidden = 0
    for k, (r, st) in enumerate(zip(eager["recs"], eager["states"])):
        before = (r.tracks_before, r.track_meta_before, r.track_next_id_before)
        assert all(V.same_bits(a, b) for a, b in zip(before, carried)), k                      # the state is fed forward
        new, (people, count, source), counters = R.step(before, r.seen_persons, r.seen_count, r.robot_pose, p, people, source)
        for got, want in zip((r.tracks_after, r.track_meta_after, r.track_next_id_after, r.tracked_persons, r.tracked_count, r.tracked_source),
                             (*new, people, count, source)):
            assert got.dtype == want.dtype and V.same_bits(got, want), k
        for name, want in zip(TRACKER_STATE, (*new, people, count, source)):
            assert V.same_bits(st[name], want), (k, name)
        carried = new
        handed, hidden = handed + int(count.sum()), hidden + int((np.clip(r.person_count, 0, N) - r.seen_count).sum())
        assert (counters["sanitised"] == 0).all() and (counters["dropped"] == 0).all(), k      # 16 slots for 4 persons, and no garbage
    print("tracked rows handed on:", handed, "person-ticks out of sight:", hidden)
    # tracks are confirmed and handed on, of the persons in sight only (whoever stays hidden these 8 ticks never gets a track;
    # a track that outlives its person's sight is the constructed scene's subject below)
    assert handed >= B and hidden >= 1


def test_people_to_status_reads_the_tracked_rows(eager):
    world, s = eager["world"], eager["ep"].solver
    differs = 0
    for k, r in enumerate(eager["recs"]):
        want, has = s.people_to_status(r.tracked_persons, r.tracked_count, N, robot_pose=r.robot_pose, fov_angle=FOV, costmap_origin=r.costmap_origin,
                                       size_x=SIZE, size_y=SIZE, resolution=world.resolution)
        assert V.same_bits(r.init_people, want) and np.array_equal(r.has_people, has), k
        differs += not V.same_bits(s.people_to_status(r.tracked_persons, r.tracked_count, N)[0], s.people_to_status(r.seen_persons, r.seen_count, N)[0])
    assert differs == TICKS                                                                    # tracks are not the detections
    first, last = eager["recs"][0], eager["recs"][-1]                                          # the world keeps its true persons
    assert np.array_equal(last.person_count, first.person_count) and not V.same_bits(last.persons_after, first.persons)


def test_graph_replay_equals_the_eager_ticks(eager):
    g, _, _ = build()
    g.capture_graph()
    assert not g.tracks.any() and not g.track_meta.any() and not g.track_next_id.any()         # the warm-up tick's tracks are taken back
    for _ in range(TICKS):
        g.replay()
    g.synchronize()
    want = eager["states"][-1]
    for k, v in state(g).items():
        assert V.same_bits(v, want[k]), k


def test_tracker_none_is_the_plain_episode(eager):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup("private")
    plain, none = BatchEpisode(prm, sc, w_ref, visibility=VP, **kw), BatchEpisode(prm, sc, w_ref, visibility=VP, tracker=None, **kw)
    for ep in (plain, none):
        assert ep.tracker is None and not hasattr(ep._c, "tracker")
        assert (ep._c.people.people, ep._c.people.count) == (ep.seen_persons.data_ptr(), ep.seen_count.data_ptr())
        for name in TRACKER_STATE:
            assert not hasattr(ep, name), name
    for k in range(3):
        timing = {}
        a, b = plain.tick(record=True), none.tick(record=True, timing=timing)
        assert "tracker_ms" not in timing
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if f.name.startswith(("tracks_", "track_meta_", "track_next_id_", "tracked_")):
                assert x is None and y is None, f.name
            elif isinstance(x, dict):
                assert all(V.same_bits(x[n], y[n]) for n in x), (k, f.name)
            elif x is not None:
                assert V.same_bits(x, y), (k, f.name)
        r = eager["recs"][k]                                                                   # the tracked episode perceives the same world
        assert V.same_bits(a.persons, r.persons) and (k > 0 or V.same_bits(a.seen_persons, r.seen_persons))
    with pytest.raises(ValueError):
        BatchEpisode(prm, sc, w_ref, visibility=VP, tracker=TrackerParams(slots=65), **kw)
    with pytest.raises(ValueError):
        BatchEpisode(prm, sc, w_ref, visibility=VP, tracker="tracks", **kw)
    without = BatchEpisode(prm, sc, w_ref, tracker=TP, **kw)                                   # without visibility the detections are the persons
    assert (without._c.tracker.detections, without._c.tracker.det_count) == (without.persons.data_ptr(), without.person_count.data_ptr())


# ---- a pedestrian steps behind a wall -----------------------------------------------------------------------------------------
# Robot 0 stands in the middle of an empty floor, facing +x. A wall two cells thick stands 1 m in front of it and reaches from
# the robot's own y to 2.5 m beside it (+y). A pedestrian walks along +y, 2 m in front of the robot, at 1.2 m/s (0.06 m per
# tick of 0.05 s), starting 1.7 m to the side (-y): in sight until the sight line meets the wall's end near y = 0, then hidden
# until far beyond the ticks run here.
SCENE_B, SPEED, START, SCENE_TICKS = 2, 1.2, -1.7, 56


def scene():
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world
    prm = OptimizerParams.readme()
    world = make_world(256, 192, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15), discs=0)
    sc = scenes_in_world(prm, world, SCENE_B, N, size_x=SIZE, size_y=SIZE)
    robot = np.array(world.origin, np.float64) + [5.025, 3.525]                                 # the centre of a cell
    sc.pose0[0] = [robot[0], robot[1], 0.0]
    c = np.floor((robot + [1.0, 0.0] - world.origin) / world.resolution).astype(int)
    world.map[c[1]:c[1] + 50, c[0]:c[0] + 2] = 254
    row = np.array([robot[0] + 2.0, robot[1] + START, 0.0, SPEED, 0.0])
    return prm, world, sc, robot, row


def walk_on_the_cpu(prm, world, robot, row, ticks=SCENE_TICKS):
    """The yardsticks alone on the pedestrian's true positions: per tick (true xy, seen_count, tracked_count, tracked row)."""
    p, st = ref_params(prm, Np=N), R.zero_state(1, TP.slots)
    pose, out = np.array([[robot[0], robot[1], 0.0]]), []
    for t in range(ticks):
        persons = np.zeros((1, N, 5))
        persons[0, 0] = row
        persons[0, 0, 1] = row[1] + SPEED * float(prm.dt) * t
        vis, n, _ = V.visible_people(world.map, world.origin, world.resolution, pose, persons, np.array([1], np.int32), VP.max_range,
                                     VP.occlusion_min_cost, VP.unknown_occludes, visible=np.zeros(persons.shape), seen=np.zeros((1, N), np.uint8))
        st, (people, count, _), _ = R.step(st, vis, n, pose, p)
        out.append((persons[0, 0, :2].copy(), int(n[0]), int(count[0]), people[0, 0].copy()))
    return out


def check_walk(steps, tp=TP):
    """What the scene is built to show, on (true xy, seen_count, tracked_count, tracked row) per tick."""
    seen = [s[1] for s in steps]
    n_seen = seen.index(0)
    assert n_seen >= 25 and all(v == 1 for v in seen[:n_seen]) and not any(seen[n_seen:])       # in sight, then behind the wall for good
    tracked = [s[2] for s in steps]
    last = n_seen + tp.max_missed                                                              # the first tick without the row
    assert tracked[:tp.confirm_hits - 1] == [0] * (tp.confirm_hits - 1) and all(v == 1 for v in tracked[tp.confirm_hits - 1:last])
    assert len(steps) > last + 2 and not any(tracked[last:])                                   # persists for max_missed ticks, then disappears
    speed = float(np.hypot(*steps[n_seen - 1][3][2:4]))
    assert abs(speed - SPEED) <= 0.01 * SPEED, speed                                           # at the moment of occlusion
    worst = max(float(np.hypot(*(s[3][:2] - s[0]))) for s in steps[n_seen:last])
    assert worst <= 0.01, worst                                                                # the coasted row follows the true pedestrian
    return n_seen, speed, worst


def test_a_pedestrian_who_steps_behind_a_wall_is_tracked_on():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, arc_plans
    prm, world, sc, robot, row = scene()
    n_seen, speed, worst = check_walk(walk_on_the_cpu(prm, world, robot, row))                 # first the yardsticks alone, on the CPU
    print(f"yardstick: in sight {n_seen} ticks, speed at occlusion {speed:.6f} m/s, worst coasted error {worst * 1e3:.3f} mm")
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    plan, plan_len = arc_plans(sc.pose0, np.zeros(SCENE_B))
    ep = BatchEpisode(prm, sc, np.zeros(SCENE_B), visibility=VP, tracker=TP, plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=FOV,
                      plan_window=(4.0, 10.0), obstacles_from_costmap=True, world=world)
    torch = ep.torch
    pose0, speed0 = ep.pose.clone(), ep.speed.clone()
    ep.persons[0, 0] = torch.tensor(row, dtype=torch.float64, device=ep.dev)
    ep.person_count[0] = 1
    recs = []
    for _ in range(SCENE_TICKS):
        ep.pose.copy_(pose0)                                                                   # the robots stand
        ep.speed.copy_(speed0)
        recs.append(ep.tick(record=True))
    ep.synchronize()
    p, st = ref_params(prm), R.zero_state(SCENE_B, TP.slots)
    people, source = np.zeros((SCENE_B, N, 5)), np.zeros((SCENE_B, N, 2), np.int32)
    for k, r in enumerate(recs):                                                               # the episode is the yardsticks', tick by tick
        vis, n, _ = V.visible_people(world.map, world.origin, world.resolution, r.robot_pose, r.persons, r.person_count, VP.max_range,
                                     VP.occlusion_min_cost, VP.unknown_occludes, visible=np.zeros(r.persons.shape),
                                     seen=np.zeros(r.persons.shape[:2], np.uint8))
        assert np.array_equal(r.seen_count, n) and V.same_bits(r.seen_persons[0, :n[0]], vis[0, :n[0]]), k
        st, (people, count, source), _ = R.step(st, r.seen_persons, r.seen_count, r.robot_pose, p, people, source)
        assert V.same_bits(r.tracked_persons, people) and np.array_equal(r.tracked_count, count) and V.same_bits(r.tracks_after, st[0]), k
    steps = [(r.persons[0, 0, :2], int(r.seen_count[0]), int(r.tracked_count[0]), r.tracked_persons[0, 0]) for r in recs]
    got = check_walk(steps)
    print(f"episode:   in sight {got[0]} ticks, speed at occlusion {got[1]:.6f} m/s, worst coasted error {got[2] * 1e3:.3f} mm")
    assert got[0] == n_seen
