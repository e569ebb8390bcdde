"""Closed-loop episodes on sensed local costmaps (BatchEpisode(sensor=SensorParams())): 12 robots on the 256 x 192 world, 80 x 80
windows (the 4 m of the reference's local costmap), arc plans with the plan window, 3 recorded ticks; once with private
persons (4 per robot, constant velocity; one is stood 1 m in front of robot 0, in free space and in sight) and once in a shared
world (a pool of 24 pedestrians and the other robots). Every tick's windows and beams are the yardstick's
(tests/sensed_costmap_ref.py) on that tick's recorded pose, persons and window cells; graph replay equals the eager ticks;
without `sensor` nothing changes.

No assertion on how well the robots then drive."""
import dataclasses

import numpy as np
import pytest

import sensed_costmap_ref as R
import visibility_ref as V
from nav2_social_mpc_controller_amd.params import OptimizerParams, SensorParams, SharedWorldParams, TrajectorizerParams

pytestmark = pytest.mark.gpu

B, N, M, TICKS, SIZE, FOV = 12, 4, 24, 3, 80, 1.2
SENSOR = SensorParams()
STATE = ("pose", "speed", "persons", "person_count", "cmd_vel", "costmap", "costmap_origin", "costmap_cell", "people", "has_people")


def setup(kind):
    from nav2_social_mpc_controller_amd.episode import arc_plans
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world, shared_pool, uniform

    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    world = make_world(256, 192, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15))
    sc = scenes_in_world(prm, world, B, N, size_x=SIZE, size_y=SIZE)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    kw = dict(plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=FOV, plan_window=(4.0, 10.0), obstacles_from_costmap=True, world=world)
    if kind == "shared":
        kw.update(shared=SharedWorldParams(), pool=shared_pool(world, M))
    return prm, world, sc, w_ref, kw


def spot_in_front(world, pose0):
    """The first of 16 bearings whose point 1 m from the robot is a free cell of the world, in sight of it."""
    for k in range(16):
        spot = pose0[:2] + np.array([np.cos(2.0 * np.pi * k / 16.0), np.sin(2.0 * np.pi * k / 16.0)])
        cell = np.floor((spot - world.origin) / world.resolution).astype(int)
        if world.map[cell[1], cell[0]] == 0 and V.classify(world.map, world.origin, world.resolution, pose0[:2], spot, 10.0) == V.SEEN:
            return spot
    raise AssertionError("no free spot 1 m from robot 0")


def build(kind, sensor=SENSOR):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup(kind)
    ep = BatchEpisode(prm, sc, w_ref, sensor=sensor, **kw)
    if kind == "private":                                                   # a pedestrian stands 1 m from robot 0
        spot = spot_in_front(world, sc.pose0[0])
        ep.persons[0, 0] = ep.torch.tensor([spot[0], spot[1], 0.0, 0.0, 0.0], dtype=ep.torch.float64, device=ep.dev)
        ep.person_count[0] = max(int(ep.person_count[0]), 1)
    return ep, world


def state(ep):
    names = STATE + (("beam_kind", "beam_cell") if ep.sensor is not None else ())
    out = {k: getattr(ep, k).cpu().numpy().copy() for k in names}
    out.update({"res_" + k: v.cpu().numpy().copy() for k, v in ep.res.items()})
    return out


def reference(world, r, sp=SENSOR):
    table, _ = sp.inflation_table(world.resolution)
    return R.sensed_costmap(world.map, world.origin, world.resolution, r.robot_pose, r.persons, r.person_count, r.costmap_cell, SIZE, SIZE,
                            sp.beam_cells(world.resolution), sp.agent_d2(world.resolution), table, sp.BASES.index(sp.base), 255,
                            sp.occlusion_min_cost, sp.unknown_occludes)


@pytest.fixture(scope="module", params=["private", "shared"])
def eager(request):
    ep, world = build(request.param)
    assert ep.beam_kind.shape == (B, 360) and ep.beam_cell.shape == (B, 360, 2) and ep._c.sensor.cell == ep.costmap_cell.data_ptr()
    recs, states = [], []
    for _ in range(TICKS):
        timing = {}
        recs.append(ep.tick(record=True, timing=timing))
        ep.synchronize()
        assert timing["sensed_costmap_ms"] > 0.0
        states.append(state(ep))
    return dict(kind=request.param, ep=ep, recs=recs, states=states, world=world)


def test_every_ticks_windows_and_beams_are_the_yardsticks(eager):
    world = eager["world"]
    kinds = np.zeros(6, np.int64)
    for k, (r, st) in enumerate(zip(eager["recs"], eager["states"])):
        cm, kind, hit = reference(world, r)
        assert r.sensed_costmap.dtype == np.uint8 and np.array_equal(r.sensed_costmap, cm), k
        assert r.beam_kind.dtype == np.uint8 and np.array_equal(r.beam_kind, kind) and np.array_equal(r.beam_cell, hit), k
        assert np.array_equal(st["costmap"], cm), k                         # what the tick's solve read is what the scan wrote
        kinds += np.bincount(kind.ravel(), minlength=6)
    print(eager["kind"], "beams none / world / agent / pair:", kinds[:4].tolist())
    assert kinds[R.NONE] > 0 and kinds[R.WORLD] > 0 and kinds[R.AGENT] > 0 and kinds[R.INVALID] == 0 and kinds[R.NO_ROBOT] == 0
    if eager["kind"] == "shared":                                           # the persons are the gather's, the other robots among them
        assert all((r.person_source >= M).any() for r in eager["recs"])
        return
    # private: the pedestrian 1 m in front of robot 0 puts lethal cells into the window where the world cut has none
    from nav2_social_mpc_controller_amd.scenes import crop_windows
    r = eager["recs"][0]
    cut = crop_windows(world.map, r.costmap_cell, SIZE, SIZE, 255)
    person = np.floor((r.persons[0, 0, :2] - world.origin) / world.resolution).astype(int) - r.costmap_cell[0]   # its window cell
    new = np.argwhere((r.sensed_costmap[0] == 254) & (cut[0] != 254))                                              # (y, x)
    near = new[np.hypot(new[:, 1] - person[0], new[:, 0] - person[1]) <= 6.0]                                      # on its disc of 6 cells
    assert len(near) >= 3 and (r.beam_kind[0] == R.AGENT).sum() >= 10


def test_graph_replay_equals_the_eager_ticks(eager):
    g, _ = build(eager["kind"])
    g.capture_graph()
    for _ in range(TICKS):
        g.replay()
    g.synchronize()
    want = eager["states"][-1]
    for k, v in state(g).items():
        assert V.same_bits(v, want[k]), k


def test_without_sensor_nothing_is_allocated_and_the_episode_is_the_plain_one():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.scenes import crop_windows
    prm, world, sc, w_ref, kw = setup("private")
    plain, none = BatchEpisode(prm, sc, w_ref, **kw), BatchEpisode(prm, sc, w_ref, sensor=None, **kw)
    based = BatchEpisode(prm, sc, w_ref, sensor=SensorParams(base="world"), **kw)
    for ep in (plain, none):
        assert ep.sensor is None and not hasattr(ep._c, "sensor")
        for name in ("beam_kind", "beam_cell", "sensor_beams", "sensor_table"):
            assert not hasattr(ep, name), name
    for k in range(TICKS):
        a, b, c = plain.tick(record=True), none.tick(record=True), based.tick(record=True)
        assert a.sensed_costmap is None and a.beam_kind is None and a.beam_cell is None
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, dict):
                assert all(V.same_bits(x[n], y[n]) for n in x), (k, f.name)
            elif x is not None:
                assert V.same_bits(x, y), (k, f.name)
        for name, v in state(plain).items():
            assert V.same_bits(state(none)[name], v), (k, name)
        # base "world": the larger of the free-base scan and the world cut, cell by cell
        free = reference(world, c)
        assert np.array_equal(c.beam_kind, free[1]) and np.array_equal(c.beam_cell, free[2])
        assert np.array_equal(c.sensed_costmap, np.maximum(free[0], crop_windows(world.map, c.costmap_cell, SIZE, SIZE, 255))), k
    with pytest.raises(ValueError):                                         # sensor without world
        BatchEpisode(prm, sc, w_ref, sensor=SENSOR, **{k: v for k, v in kw.items() if k not in ("world", "obstacles_from_costmap")})
    with pytest.raises(ValueError):                                         # a range beyond 127 cells
        BatchEpisode(prm, sc, w_ref, sensor=SensorParams(max_range=6.5), **kw)
