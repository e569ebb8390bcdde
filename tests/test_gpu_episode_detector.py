"""Closed-loop episodes whose controller is handed what a detector would report (BatchEpisode(visibility=..., detector=
DetectorParams(...), tracker=TrackerParams())): test_gpu_episode_sensed.py's 12 robots with 4 private persons each, 80 x 80
windows on the 256 x 192 world, arc plans, the line-of-sight filter in front of the detector and the tracker behind it, 8
recorded ticks. Every tick's draw state and detections are the yardstick's (tests/detector_ref.py) on that tick's recorded
persons in sight, pose and state; the tracker's recorded input is the detector's output; graph replay equals the eager
ticks, the counters included; detector=None is the episode before; a detector that hides, misses, perturbs and invents nothing
leaves the tracked episode bit for bit; two shards draw what the same robots draw unsharded.

And one constructed scene: a standing robot and two pedestrians who walk away from it in file at 1.2 m/s, 0.8 m apart, on a
line that passes 0.3 m beside the robot. While they pass the robot it sees both. The sight line to the one in front then
swings onto the one behind, 0.24 m / range from that one's centre, which is within the body radius of 0.25 m from a range of
0.96 m on: the one in front is body-occluded for the rest of the run, and the tracker coasts it for max_missed ticks. It is
first run with the two yardsticks alone on the CPU (tests/detector_ref.py, tests/tracker_ref.py).

No assertion on how well the robots then drive."""
import dataclasses

import numpy as np
import pytest

import detector_ref as R
import tracker_ref as TR
import visibility_ref as V
from nav2_social_mpc_controller_amd.params import DetectorParams, OptimizerParams, TrackerParams, TrajectorizerParams, VisibilityParams
from test_gpu_episode_sensed import B, FOV, N, SIZE, setup
from test_gpu_episode_tracker import TRACKER_STATE
from test_gpu_episode_tracker import ref_params as tracker_ref_params

pytestmark = pytest.mark.gpu

TICKS = 8
VP, TP = VisibilityParams(), TrackerParams()
# four persons a robot: a high miss and clutter probability, so that 8 ticks of 12 robots show every effect
DP = DetectorParams(body_radius=0.25, p_miss=0.25, sigma=0.03, sigma_growth=0.002, clutter_candidates=3, p_clutter=0.3, clutter_range=5.0,
                    seed=0x0123456789ABCDEF)
IDENTITY = DetectorParams(body_radius=0.0, p_miss=0.0, sigma=0.0, sigma_growth=0.0, clutter_candidates=0, p_clutter=0.0)
ND = N + DP.clutter_candidates
STATE = ("pose", "speed", "persons", "person_count", "cmd_vel", "costmap", "costmap_origin", "costmap_cell", "people", "has_people",
         "seen_persons", "seen_count", "person_seen")
DETECTOR_STATE = ("draw_state", "detected_persons", "detected_count", "detected_source", "person_outcome")


def ref_params(dp=DP, Nd=ND):
    return R.params(body_radius=dp.body_radius, p_miss=dp.p_miss, sigma=dp.sigma, sigma_growth=dp.sigma_growth,
                    clutter_candidates=dp.clutter_candidates, p_clutter=dp.p_clutter, clutter_range=dp.clutter_range, seed=dp.seed, Nd=Nd)


def build(detector=DP, tracker=TP):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup("private")
    return BatchEpisode(prm, sc, w_ref, visibility=VP, tracker=tracker, detector=detector, **kw), prm, world


def state(ep, detector=True):
    names = STATE + (TRACKER_STATE if ep.tracker is not None else ()) + (DETECTOR_STATE if detector and ep.detector is not None else ())
    out = {k: getattr(ep, k).cpu().numpy().copy() for k in names}
    out.update({"res_" + k: v.cpu().numpy().copy() for k, v in ep.res.items()})
    return out


@pytest.fixture(scope="module")
def eager():
    ep, prm, world = build()
    start = {k: getattr(ep, k).cpu().numpy().copy() for k in DETECTOR_STATE}
    assert start["draw_state"].tolist() == [[b, 0] for b in range(B)] and all(not start[k].any() for k in DETECTOR_STATE[1:])
    assert start["detected_persons"].shape == (B, ND, 5) and start["detected_source"].shape == (B, ND) and start["person_outcome"].shape == (B, N)
    assert start["person_outcome"].dtype == np.uint8 and all(start[k].dtype == np.int32 for k in ("draw_state", "detected_count", "detected_source"))
    c = ep._c
    assert (c.detector.people, c.detector.count, c.detector.robot_pose) == (ep.seen_persons.data_ptr(), ep.seen_count.data_ptr(), ep.pose.data_ptr())
    assert (c.tracker.detections, c.tracker.det_count) == (ep.detected_persons.data_ptr(), ep.detected_count.data_ptr())
    assert (c.people.people, c.people.count, c.people.Np) == (ep.tracked_persons.data_ptr(), ep.tracked_count.data_ptr(), N)
    assert (c.detector.Np, c.detector.Nd, c.detector.Kc, c.tracker.Nd, c.tracker.Np) == (N, ND, DP.clutter_candidates, ND, N)
    assert (c.detector.seed_lo, c.detector.seed_hi, c.detector.miss_threshold, c.detector.clutter_threshold) == (*DP.key(), *DP.thresholds())
    addresses = [getattr(ep, k).data_ptr() for k in DETECTOR_STATE]
    recs, states = [], []
    for _ in range(TICKS):
        timing = {}
        recs.append(ep.tick(record=True, timing=timing))
        ep.synchronize()
        assert timing["detector_ms"] > 0.0 and timing["tracker_ms"] > 0.0
        states.append(state(ep))
    assert addresses == [getattr(ep, k).data_ptr() for k in DETECTOR_STATE]
    return dict(ep=ep, recs=recs, states=states, world=world, prm=prm)


def test_every_ticks_detections_are_the_yardsticks(eager):
    p = ref_params()
    carried = np.stack([np.arange(B), np.zeros(B)], axis=1).astype(np.uint32)
    det, source, outcome = np.zeros((B, ND, 5)), np.zeros((B, ND), np.int32), np.zeros((B, N), np.uint8)
    total = dict.fromkeys(R.COUNTERS, 0)
    for k, (r, st) in enumerate(zip(eager["recs"], eager["states"])):
        assert r.draw_state_before.dtype == np.uint32 and V.same_bits(r.draw_state_before, carried), k   # the state is fed forward
        new, (det, det_count, source, outcome), counters = R.step(r.draw_state_before, r.seen_persons, r.seen_count, r.robot_pose, p, det, source, outcome)
        for got, want in zip((r.draw_state_after, r.detected_persons, r.detected_count, r.detected_source, r.person_outcome),
                             (new, det, det_count, source, outcome)):
            assert got.dtype == want.dtype and V.same_bits(got, want), k
        for name, want in zip(DETECTOR_STATE, (new.view(np.int32), det, det_count, source, outcome)):
            assert V.same_bits(st[name], want), (k, name)
        carried = new
        for name in R.COUNTERS:
            total[name] += int(counters[name].sum())
    print("episode counters:", total)
    assert carried[:, 1].tolist() == [TICKS] * B and carried[:, 0].tolist() == list(range(B))
    assert total["detected"] >= B and total["missed"] >= 1 and total["clutter"] >= 1 and total["pose_not_finite"] == 0
    first, last = eager["recs"][0], eager["recs"][-1]                                          # the world keeps its true persons
    assert np.array_equal(last.person_count, first.person_count) and not V.same_bits(last.persons_after, first.persons)


def test_the_trackers_input_is_the_detectors_output(eager):
    p = tracker_ref_params(eager["prm"])
    carried = TR.zero_state(B, TP.slots)
    people, source = np.zeros((B, N, 5)), np.zeros((B, N, 2), np.int32)
    world, s = eager["world"], eager["ep"].solver
    for k, r in enumerate(eager["recs"]):
        before = (r.tracks_before, r.track_meta_before, r.track_next_id_before)
        assert all(V.same_bits(a, b) for a, b in zip(before, carried)), k
        new, (people, count, source), _ = TR.step(before, r.detected_persons, r.detected_count, r.robot_pose, p, people, source)
        for got, want in zip((r.tracks_after, r.track_meta_after, r.track_next_id_after, r.tracked_persons, r.tracked_count, r.tracked_source),
                             (*new, people, count, source)):
            assert got.dtype == want.dtype and V.same_bits(got, want), k
        carried = new
        want, has = s.people_to_status(r.tracked_persons, r.tracked_count, N, robot_pose=r.robot_pose, fov_angle=FOV, costmap_origin=r.costmap_origin,
                                       size_x=SIZE, size_y=SIZE, resolution=world.resolution)
        assert V.same_bits(r.init_people, want) and np.array_equal(r.has_people, has), k


def test_graph_replay_equals_the_eager_ticks_and_their_counters(eager):
    g, _, _ = build()
    g.capture_graph()
    assert g.draw_state.cpu().numpy().tolist() == [[b, 0] for b in range(B)]                   # the warm-up tick's draw is taken back
    for _ in range(TICKS):
        g.replay()
    g.synchronize()
    want = eager["states"][-1]
    assert want["draw_state"][:, 1].tolist() == [TICKS] * B                                    # a replayed graph draws fresh numbers every tick
    for k, v in state(g).items():
        assert V.same_bits(v, want[k]), k


def test_detector_none_is_the_episode_before():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup("private")
    plain = BatchEpisode(prm, sc, w_ref, visibility=VP, tracker=TP, **kw)
    none = BatchEpisode(prm, sc, w_ref, visibility=VP, tracker=TP, detector=None, **kw)
    for ep in (plain, none):
        assert ep.detector is None and not hasattr(ep._c, "detector")
        assert (ep._c.tracker.detections, ep._c.tracker.det_count, ep._c.tracker.Nd) == (ep.seen_persons.data_ptr(), ep.seen_count.data_ptr(), N)
        for name in DETECTOR_STATE:
            assert not hasattr(ep, name), name
    for k in range(3):
        timing = {}
        a, b = plain.tick(record=True), none.tick(record=True, timing=timing)
        assert "detector_ms" not in timing
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if f.name.startswith(("draw_state_", "detected_", "person_outcome")):
                assert x is None and y is None, f.name
            elif isinstance(x, dict):
                assert all(V.same_bits(x[n], y[n]) for n in x), (k, f.name)
            elif x is not None:
                assert V.same_bits(x, y), (k, f.name)
    with pytest.raises(ValueError):
        BatchEpisode(prm, sc, w_ref, visibility=VP, detector=DetectorParams(clutter_candidates=65), **kw)
    with pytest.raises(ValueError):
        BatchEpisode(prm, sc, w_ref, visibility=VP, detector="detector", **kw)
    with pytest.raises(ValueError):
        plain.set_detector_streams(np.arange(B))
    # without visibility the detector reads the persons; without a tracker people_to_status reads the detections
    bare = BatchEpisode(prm, sc, w_ref, detector=DP, **kw)
    c = bare._c
    assert (c.detector.people, c.detector.count) == (bare.persons.data_ptr(), bare.person_count.data_ptr()) and not hasattr(c, "tracker")
    assert (c.people.people, c.people.count, c.people.Np) == (bare.detected_persons.data_ptr(), bare.detected_count.data_ptr(), ND)
    r = bare.tick(record=True)
    want, has = bare.solver.people_to_status(r.detected_persons, r.detected_count, N, robot_pose=r.robot_pose, fov_angle=FOV,
                                             costmap_origin=r.costmap_origin, size_x=SIZE, size_y=SIZE, resolution=world.resolution)
    assert V.same_bits(r.init_people, want) and np.array_equal(r.has_people, has)


def test_a_detector_that_changes_nothing_leaves_the_tracked_episode_bit_for_bit():
    with_detector, _, _ = build(IDENTITY)
    without, _, _ = build(None)
    assert int(with_detector.detected_persons.shape[1]) == N
    for k in range(TICKS):
        with_detector.tick()
        without.tick()
        got, want = state(with_detector, detector=False), state(without)
        assert sorted(got) == sorted(want) and all(V.same_bits(got[n], want[n]) for n in want), k
        seen, n = with_detector.seen_persons.cpu().numpy(), with_detector.seen_count.cpu().numpy()
        det = with_detector.detected_persons.cpu().numpy()
        assert np.array_equal(with_detector.detected_count.cpu().numpy(), n) and all(V.same_bits(det[b, :n[b]], seen[b, :n[b]]) for b in range(B))
    assert with_detector.draw_state.cpu().numpy()[:, 1].tolist() == [TICKS] * B


def test_two_shards_draw_what_the_same_robots_draw_unsharded(eager):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode
    prm, world, sc, w_ref, kw = setup("private")
    two = ShardedEpisode(prm, sc, w_ref, None, None, None, shards=2, graphs=True, visibility=VP, tracker=TP, detector=DP, **kw)
    assert [p.B for p in two.parts] == [6, 6] and two.parts[1].draw_state.cpu().numpy().tolist() == [[b, 0] for b in range(6, 12)]
    for _ in range(TICKS):
        two.tick()
    want = eager["states"][-1]
    for name in DETECTOR_STATE + TRACKER_STATE + ("pose", "cmd_vel"):
        assert V.same_bits(two.gather(name).cpu().numpy(), want[name]), name
    # streams of the caller's own: robots 6 .. 11 alone, as a plain episode that is told who they are
    idx = np.arange(6, 12)
    from nav2_social_mpc_controller_amd.episode import shard_kwargs
    half = BatchEpisode(prm, sc.select(idx), np.asarray(w_ref)[idx], visibility=VP, tracker=TP, detector=DP, **shard_kwargs(kw, idx, B))
    half.set_detector_streams(idx)
    for _ in range(TICKS):
        half.tick()
    half.synchronize()
    for name in DETECTOR_STATE:
        assert V.same_bits(getattr(half, name).cpu().numpy(), want[name][idx]), name
    with pytest.raises(ValueError):
        half.set_detector_streams(np.arange(5))
    with pytest.raises(ValueError):
        half.set_detector_streams(-np.ones(6))
    with pytest.raises(ValueError):
        ShardedEpisode(prm, sc, w_ref, None, None, None, shards=2, graphs=False, visibility=VP, detector_streams=np.arange(B), **kw)


# ---- two pedestrians in file -------------------------------------------------------------------------------------------------
# Robot 0 stands in the middle of an empty floor, facing +x. Two pedestrians walk along +x on the line 0.3 m beside it (+y), 0.8 m
# apart, at 1.2 m/s (0.06 m per tick of 0.05 s); the one behind starts 0.9 m behind the robot's x. The detector neither misses
# nor perturbs nor invents anything here: what is asserted is the body occlusion alone.
SCENE_B, SPEED, SIDE, GAP, START, SCENE_TICKS = 2, 1.2, 0.3, 0.8, -0.9, 48
FILE = DetectorParams(body_radius=0.25, p_miss=0.0, sigma=0.0, sigma_growth=0.0, clutter_candidates=0, p_clutter=0.0)


def scene():
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world
    prm = OptimizerParams.readme()
    world = make_world(256, 192, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15), discs=0)
    sc = scenes_in_world(prm, world, SCENE_B, N, size_x=SIZE, size_y=SIZE)
    robot = np.array(world.origin, np.float64) + [5.025, 3.525]                                 # the centre of a cell
    sc.pose0[0] = [robot[0], robot[1], 0.0]
    rows = np.array([[robot[0] + START, robot[1] + SIDE, SPEED, 0.0, 0.0],                      # person 0 walks behind ...
                     [robot[0] + START + GAP, robot[1] + SIDE, SPEED, 0.0, 0.0]])               # ... person 1, who walks in front
    return prm, world, sc, robot, rows


def walk_on_the_cpu(prm, robot, rows, ticks=SCENE_TICKS):
    """The two yardsticks alone on the pedestrians' true positions (the floor is empty: both are in line of sight): per tick
    (true xy [2,2], outcome [2], tracked_count, tracked rows [N,5], tracked source [N,2])."""
    dp, tp = ref_params(FILE, Nd=N), tracker_ref_params(prm)
    draw, st = np.zeros((1, 2), np.uint32), TR.zero_state(1, TP.slots)
    pose, out = np.array([[robot[0], robot[1], 0.0]]), []
    for t in range(ticks):
        persons = np.zeros((1, N, 5))
        persons[0, :2] = rows
        persons[0, :2, 0] = rows[:, 0] + SPEED * float(prm.dt) * t
        draw, (det, det_count, _, outcome), _ = R.step(draw, persons, np.array([2], np.int32), pose, dp)
        st, (people, count, source), _ = TR.step(st, det, det_count, pose, tp)
        out.append((persons[0, :2, :2].copy(), outcome[0, :2].copy(), int(count[0]), people[0].copy(), source[0].copy()))
    return out


def check_walk(steps, tp=TP):
    """What the scene is built to show, on (true xy, outcome, tracked_count, tracked rows, tracked source) per tick."""
    hidden = [int(s[1][1]) == R.BODY_OCCLUDED for s in steps]
    first = hidden.index(True)
    assert first >= 10 and not any(hidden[:first]) and all(hidden[first:])                      # in sight, then behind the other's body for good
    assert all(int(s[1][0]) == R.DETECTED for s in steps)                                      # the one behind is never hidden by the one in front
    # the very tick: person 0 is then the first whose offset x from the robot satisfies 0.24^2 <= 0.0625 * ((x + 0.8)^2 + 0.09)
    x = [s[0][0][0] for s in steps]
    reach = x[0] - START + np.sqrt(0.24 ** 2 / 0.0625 - SIDE ** 2) - GAP
    assert x[first - 1] < reach <= x[first] + 1e-9
    tracked = [s[2] for s in steps]
    last = first + tp.max_missed                                                               # the first tick without the row
    assert tracked[tp.confirm_hits - 1:first] == [2] * (first - tp.confirm_hits + 1) and tracked[first:last] == [2] * tp.max_missed
    assert len(steps) > last + 2 and tracked[last:] == [1] * (len(steps) - last)               # coasted for max_missed ticks, then dropped
    ids = [sorted(s[4][:s[2], 1].tolist()) for s in steps]
    assert all(v == [0, 1] for v in ids[tp.confirm_hits - 1:last]) and all(v == [0] for v in ids[last:])   # the same two tracks throughout
    worst = 0.0
    for s in steps[first:last]:
        row = s[3][:2][s[4][:2, 1] == 1][0]                                                    # the coasted track: id 1, born of person 1
        worst = max(worst, float(np.hypot(*(row[:2] - s[0][1]))))
    assert worst <= FILE.body_radius, worst                                                    # the coasted row still lies on the hidden person's body
    return first, worst


def test_the_pedestrian_in_front_is_hidden_by_the_one_behind_and_tracked_on():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, arc_plans
    prm, world, sc, robot, rows = scene()
    first, worst = check_walk(walk_on_the_cpu(prm, robot, rows))                               # first the yardsticks alone, on the CPU
    print(f"yardsticks: both in sight {first} ticks, worst coasted error {worst * 1e3:.1f} mm")
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    plan, plan_len = arc_plans(sc.pose0, np.zeros(SCENE_B))
    ep = BatchEpisode(prm, sc, np.zeros(SCENE_B), visibility=VP, detector=FILE, tracker=TP, plan=plan, plan_len=plan_len, traj_params=tp,
                      fov_angle=FOV, plan_window=(4.0, 10.0), obstacles_from_costmap=True, world=world)
    torch = ep.torch
    pose0, speed0 = ep.pose.clone(), ep.speed.clone()
    ep.persons[0, :2] = torch.tensor(rows, dtype=torch.float64, device=ep.dev)
    ep.person_count[0] = 2
    recs = []
    for _ in range(SCENE_TICKS):
        ep.pose.copy_(pose0)                                                                   # the robots stand
        ep.speed.copy_(speed0)
        recs.append(ep.tick(record=True))
    ep.synchronize()
    dp, tr = ref_params(FILE, Nd=N), tracker_ref_params(prm)
    draw, st = np.stack([np.arange(SCENE_B), np.zeros(SCENE_B)], axis=1).astype(np.uint32), TR.zero_state(SCENE_B, TP.slots)
    det, source, outcome = np.zeros((SCENE_B, N, 5)), np.zeros((SCENE_B, N), np.int32), np.zeros((SCENE_B, N), np.uint8)
    people, tracked_source = np.zeros((SCENE_B, N, 5)), np.zeros((SCENE_B, N, 2), np.int32)
    for k, r in enumerate(recs):                                                               # the episode is the yardsticks', tick by tick
        assert r.seen_count[0] == 2, k                                                         # the floor hides nobody
        draw, (det, det_count, source, outcome), _ = R.step(draw, r.seen_persons, r.seen_count, r.robot_pose, dp, det, source, outcome)
        assert V.same_bits(r.detected_persons, det) and np.array_equal(r.detected_count, det_count) and V.same_bits(r.person_outcome, outcome), k
        assert V.same_bits(r.detected_source, source) and V.same_bits(r.draw_state_after, draw), k
        st, (people, count, tracked_source), _ = TR.step(st, r.detected_persons, r.detected_count, r.robot_pose, tr, people, tracked_source)
        assert V.same_bits(r.tracked_persons, people) and np.array_equal(r.tracked_count, count) and V.same_bits(r.tracks_after, st[0]), k
    seen_order = [r.seen_persons[0, :2, 0].argsort() for r in recs]                            # seen rows in the persons' order: person 0 behind
    steps = [(r.seen_persons[0, :2][o][:, :2], r.person_outcome[0, :2][o], int(r.tracked_count[0]), r.tracked_persons[0], r.tracked_source[0])
             for r, o in zip(recs, seen_order)]
    got = check_walk(steps)
    print(f"episode:    both in sight {got[0]} ticks, worst coasted error {got[1] * 1e3:.1f} mm")
    assert got[0] == first
