"""Closed-loop episodes whose people come from the scan (BatchEpisode(sensor=..., scan_detector=ScanDetectorParams())): 6 robots
on the 256 x 192 world of tests/test_gpu_episode_sensed.py with 40 x 40 windows and private persons, a pedestrian standing 1 m
from robot 0, 8 recorded ticks; with the tracker at 360 and at 72 beams, with the scan's memory, and without the tracker. Every
tick's scan_persons, scan_count, scan_segment and scan_stats are the yardstick's (tests/scan_people_ref.py) on that tick's
recorded beam_kind, beam_cell and pose; the tracker read those rows and its outputs are tests/tracker_ref.py's on them; the
rows people_to_status read are the tracker's, or without one the scan's; graph replay equals the eager ticks byte for byte;
without the keyword nothing is allocated and the episode is the one before; the keyword is refused without `sensor` and beside
`visibility` or `detector`.

No assertion on how well the robots then drive."""
import dataclasses

import numpy as np
import pytest

import scan_people_ref as R
import test_gpu_episode_sensed as SE
import tracker_ref as TR
import visibility_ref as V
from nav2_social_mpc_controller_amd.params import (DetectorParams, ObstacleMemoryParams, OptimizerParams, ScanDetectorParams, SensorParams, TrackerParams,
                                                   TrajectorizerParams, VisibilityParams)
from test_gpu_episode_tracker import TRACKER_STATE
from test_gpu_episode_tracker import ref_params as tracker_ref_params

pytestmark = pytest.mark.gpu

B, N, SIZE, TICKS, FOV = 6, 4, 40, 8, SE.FOV
SD, TP = ScanDetectorParams(), TrackerParams()
ND = SD.max_detections
KINDS = {"tracker_360": dict(sensor=SensorParams(), tracker=TP), "tracker_72": dict(sensor=SensorParams(n_beams=72), tracker=TP),
         "memory_360": dict(sensor=SensorParams(), sensor_memory=ObstacleMemoryParams(), tracker=TP), "bare_72": dict(sensor=SensorParams(n_beams=72))}
SCAN_STATE = ("scan_persons", "scan_count", "scan_segment", "scan_stats")
STATE = SE.STATE + ("beam_kind", "beam_cell")


def setup():
    from nav2_social_mpc_controller_amd.episode import arc_plans
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world, uniform
    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    world = make_world(256, 192, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15))
    sc = scenes_in_world(prm, world, B, N, size_x=SIZE, size_y=SIZE)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    kw = dict(plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=FOV, plan_window=(4.0, 10.0), obstacles_from_costmap=True, world=world)
    return prm, world, sc, w_ref, kw


def build(kind, scan_detector=SD):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup()
    ep = BatchEpisode(prm, sc, w_ref, scan_detector=scan_detector, **KINDS[kind], **kw)
    spot = SE.spot_in_front(world, sc.pose0[0])                           # a pedestrian stands 1 m from robot 0
    ep.persons[0, 0] = ep.torch.tensor([spot[0], spot[1], 0.0, 0.0, 0.0], dtype=ep.torch.float64, device=ep.dev)
    ep.person_count[0] = max(int(ep.person_count[0]), 1)
    return ep, world, prm, spot


def ref_params(world, sensor):
    res = world.resolution
    wmin, wmax = SD.width_d2(res)
    return R.params(SD.link_d2(res), SD.min_points, wmin, wmax, SD.range_d2(res, sensor), int(SD.subtract_map), SD.body_offset, res, tuple(world.origin))


def state(ep):
    names = STATE + (SCAN_STATE if ep.scan_detector is not None else ()) + (TRACKER_STATE if ep.tracker is not None else ())
    out = {k: getattr(ep, k).cpu().numpy().copy() for k in names}
    out.update({"res_" + k: v.cpu().numpy().copy() for k, v in ep.res.items()})
    return out


@pytest.fixture(scope="module", params=list(KINDS))
def eager(request):
    kind = request.param
    ep, world, prm, spot = build(kind)
    n = KINDS[kind]["sensor"].n_beams
    start = {k: getattr(ep, k).cpu().numpy().copy() for k in SCAN_STATE}
    assert all(not v.any() for v in start.values()) and all(start[k].dtype == np.int32 for k in SCAN_STATE[1:])
    assert start["scan_persons"].shape == (B, ND, 5) and start["scan_count"].shape == (B,) and start["scan_segment"].shape == (B, ND, 4)
    assert start["scan_stats"].shape == (B, 4)
    c = ep._c
    si = c.scan_people
    assert (si.B, si.n_beams, si.Nd, si.on_device, si.subtract_map, si.min_points) == (B, n, ND, 1, 1, SD.min_points)
    assert (si.link_d2, si.width_d2_min, si.width_d2_max, si.range_d2, si.resolution, si.body_offset) == (25, 16, 256, 2500, world.resolution, SD.body_offset)
    assert tuple(si.world_origin) == tuple(world.origin)
    assert (si.robot_pose, si.beam_kind, si.beam_cell) == (ep.pose.data_ptr(), ep.beam_kind.data_ptr(), ep.beam_cell.data_ptr())
    if ep.tracker is not None:
        assert (c.tracker.detections, c.tracker.det_count, c.tracker.Nd, c.tracker.Np) == (ep.scan_persons.data_ptr(), ep.scan_count.data_ptr(), ND, N)
        assert (c.people.people, c.people.count, c.people.Np) == (ep.tracked_persons.data_ptr(), ep.tracked_count.data_ptr(), N)
    else:
        assert (c.people.people, c.people.count, c.people.Np) == (ep.scan_persons.data_ptr(), ep.scan_count.data_ptr(), ND)
    assert c.sensor.people == ep.persons.data_ptr() and c.sensor.count == ep.person_count.data_ptr()      # the scan keeps seeing the true persons
    addresses = [getattr(ep, k).data_ptr() for k in SCAN_STATE]
    recs, states = [], []
    for _ in range(TICKS):
        timing = {}
        recs.append(ep.tick(record=True, timing=timing))
        ep.synchronize()
        assert timing["scan_people_ms"] > 0.0
        states.append(state(ep))
    assert addresses == [getattr(ep, k).data_ptr() for k in SCAN_STATE]
    return dict(kind=kind, ep=ep, recs=recs, states=states, world=world, prm=prm, spot=spot)


def test_every_ticks_detections_are_the_yardsticks_on_the_recorded_beams(eager):
    p = ref_params(eager["world"], KINDS[eager["kind"]]["sensor"])
    det, seg = np.zeros((B, ND, 5)), np.zeros((B, ND, 4), np.int32)         # rows beyond the count keep what the tick before left
    sensor = KINDS[eager["kind"]]["sensor"]                                 # the bound tests/test_scan_people.py derives for a lone person
    bound = np.sqrt(sensor.agent_d2(eager["world"].resolution)) * eager["world"].resolution + eager["world"].resolution * np.sqrt(0.5) + SD.body_offset
    found = near = 0
    for k, (r, st) in enumerate(zip(eager["recs"], eager["states"])):
        want = R.run(p, ND, r.robot_pose, r.beam_kind, r.beam_cell, det, seg)
        got = dict(detections=r.scan_persons, det_count=r.scan_count, det_segment=r.scan_segment, seg_stats=r.scan_stats)
        assert R.same(got, want), (k, [n for n in got if got[n].tobytes() != want[n].tobytes()])
        for name, key in zip(SCAN_STATE, ("detections", "det_count", "det_segment", "seg_stats")):
            assert V.same_bits(st[name], want[key]), (k, name)
        det, seg = want["detections"], want["det_segment"]
        found += int(want["det_count"].sum())
        rows = want["detections"][0, :want["det_count"][0], :2]
        near += int((np.hypot(*(rows - eager["spot"]).T) <= bound).any())
    print(eager["kind"], "detections over the episode:", found, "ticks in which robot 0 finds its pedestrian:", near)
    assert found >= 1 and near >= 1                                         # by the yardstick alone: the pedestrian stands in robot 0's scan
    first, last = eager["recs"][0], eager["recs"][-1]                       # the world keeps its true persons
    assert np.array_equal(last.person_count, first.person_count)


def test_the_tracker_reads_the_detections_and_hands_tracks_to_the_solve(eager):
    world, s, prm = eager["world"], eager["ep"].solver, eager["prm"]
    handed = 0
    if eager["ep"].tracker is None:                                         # people_to_status reads the detections themselves
        for k, r in enumerate(eager["recs"]):
            assert r.tracked_persons is None
            want, has = s.people_to_status(r.scan_persons, r.scan_count, N, robot_pose=r.robot_pose, fov_angle=FOV, costmap_origin=r.costmap_origin,
                                           size_x=SIZE, size_y=SIZE, resolution=world.resolution)
            assert V.same_bits(r.init_people, want) and np.array_equal(r.has_people, has), k
        return
    p = tracker_ref_params(prm)
    carried = TR.zero_state(B, TP.slots)
    people, source = np.zeros((B, N, 5)), np.zeros((B, N, 2), np.int32)
    for k, r in enumerate(eager["recs"]):
        before = (r.tracks_before, r.track_meta_before, r.track_next_id_before)
        assert all(V.same_bits(a, b) for a, b in zip(before, carried)), k
        new, (people, count, source), _ = TR.step(before, r.scan_persons, r.scan_count, r.robot_pose, p, people, source)
        for got, want in zip((r.tracks_after, r.track_meta_after, r.track_next_id_after, r.tracked_persons, r.tracked_count, r.tracked_source),
                             (*new, people, count, source)):
            assert got.dtype == want.dtype and V.same_bits(got, want), k
        carried = new
        handed += int(count.sum())
        want, has = s.people_to_status(r.tracked_persons, r.tracked_count, N, robot_pose=r.robot_pose, fov_angle=FOV, costmap_origin=r.costmap_origin,
                                       size_x=SIZE, size_y=SIZE, resolution=world.resolution)
        assert V.same_bits(r.init_people, want) and np.array_equal(r.has_people, has), k
    print(eager["kind"], "tracks handed to people_to_status over the episode:", handed)
    assert handed >= 1                                                      # confirmed after confirm_hits = 3 detections of a person


def test_graph_replay_equals_the_eager_ticks(eager):
    g, _, _, _ = build(eager["kind"])
    g.capture_graph()
    for _ in range(TICKS):
        g.replay()
    g.synchronize()
    want = eager["states"][-1]
    for k, v in state(g).items():
        assert V.same_bits(v, want[k]), k


def test_without_the_keyword_nothing_is_allocated_and_the_episode_is_the_one_before():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup()
    more = KINDS["memory_360"]
    plain, none = BatchEpisode(prm, sc, w_ref, **more, **kw), BatchEpisode(prm, sc, w_ref, scan_detector=None, **more, **kw)
    for ep in (plain, none):
        assert ep.scan_detector is None and not hasattr(ep._c, "scan_people") and ep._c.tracker.detections == ep.persons.data_ptr()
        for name in SCAN_STATE:
            assert not hasattr(ep, name), name
    for k in range(3):
        timing = {}
        a, b = plain.tick(record=True, timing=timing), none.tick(record=True)
        assert "scan_people_ms" not in timing
        for name in SCAN_STATE:
            assert getattr(a, name) is None and getattr(b, name) is None, name
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, dict):
                assert all(V.same_bits(x[n], y[n]) for n in x), (k, f.name)
            elif x is not None:
                assert V.same_bits(x, y), (k, f.name)
        for name, v in state(plain).items():
            assert V.same_bits(state(none)[name], v), (k, name)
    with pytest.raises(ValueError, match=r"scan_detector needs sensor=SensorParams\(\.\.\.\): it reads the scan"):
        BatchEpisode(prm, sc, w_ref, scan_detector=SD, **kw)
    with pytest.raises(ValueError, match="alternatives"):
        BatchEpisode(prm, sc, w_ref, scan_detector=SD, sensor=SensorParams(), visibility=VisibilityParams(), **kw)
    with pytest.raises(ValueError, match="alternatives"):
        BatchEpisode(prm, sc, w_ref, scan_detector=SD, sensor=SensorParams(), detector=DetectorParams(), **kw)
    with pytest.raises(ValueError):
        BatchEpisode(prm, sc, w_ref, scan_detector=dict(min_points=3), sensor=SensorParams(), **kw)
