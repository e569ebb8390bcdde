"""Closed-loop episodes with the collision monitor (BatchEpisode(monitor=MonitorParams(...), sensor=...)): 16 robots on the
256 x 192 world of tests/test_gpu_episode_sensed.py with private persons, a pedestrian standing 1 m from robot 0, 10 recorded
ticks, once with the memoryless scan and the motion model and once with the scan's memory and the robot plant. Every tick's
cmd_safe, monitor_action, monitor_points and monitor_ratio are the yardstick's (tests/collision_monitor_ref.py) on that
tick's recorded pose, cmd_vel and beams, given the recorded cosines and sines; the plant (tests/plant_ref.py) or the motion
model was handed cmd_safe; graph replay equals the eager ticks; two shards equal the unsharded rows; monitor=None is the
episode without the keyword bit for bit, and the keyword without `sensor` is refused.

No assertion on how well the robots then drive."""
import dataclasses

import numpy as np
import pytest

import collision_monitor_ref as R
import plant_ref
import test_gpu_episode_plant as EP
import test_gpu_episode_sensed as SE
import visibility_ref as V
from nav2_social_mpc_controller_amd.params import (MonitorParams, MonitorZone, ObstacleMemoryParams, OptimizerParams, PlantParams, SensorParams,
                                                   TrajectorizerParams)

pytestmark = pytest.mark.gpu

B, N, SIZE, TICKS = 16, 4, 80, 10
SENSOR = SensorParams()
PLANT = PlantParams(substeps=4)
# a STOP circle just beyond the body, a wide SLOWDOWN circle that the pedestrian 1 m from robot 0 stands in, a LIMIT box ahead
# and the footprint as APPROACH zone over 1.2 s
MONITOR = MonitorParams(zones=(MonitorZone(action="stop", radius=0.3, min_points=2),
                               MonitorZone(action="slowdown", radius=1.3, min_points=1, slowdown_ratio=0.75),
                               MonitorZone(action="limit", vertices=((0.0, -0.5), (1.6, -0.5), (1.6, 0.5), (0.0, 0.5)), min_points=3, linear_limit=0.3,
                                           angular_limit=0.5),
                               MonitorZone(action="approach", vertices=MonitorParams.nav2_like(0.24).zones[2].vertices, min_points=2)),
                        time_before_collision=1.2, simulation_time_step=0.1)
KINDS = {"model": {}, "memory_plant": dict(sensor_memory=ObstacleMemoryParams(), plant=PLANT)}
MONITOR_STATE = ("cmd_safe", "monitor_action", "monitor_points", "monitor_ratio", "monitor_heading_cs", "monitor_step_cs")
STATE = EP.STATE + ("beam_kind", "beam_cell")


def setup():
    from nav2_social_mpc_controller_amd.episode import arc_plans
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world, uniform
    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    world = make_world(256, 192, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15))
    sc = scenes_in_world(prm, world, B, N, size_x=SIZE, size_y=SIZE)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    kw = dict(plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=SE.FOV, plan_window=(4.0, 10.0), obstacles_from_costmap=True, world=world,
              sensor=SENSOR)
    return prm, world, sc, w_ref, kw


def place_pedestrian(ep, world, pose0):
    """A pedestrian stands 1 m from robot 0 (of `ep`: a whole episode or the shard that holds robot 0)."""
    spot = SE.spot_in_front(world, pose0)
    ep.persons[0, 0] = ep.torch.tensor([spot[0], spot[1], 0.0, 0.0, 0.0], dtype=ep.torch.float64, device=ep.dev)
    ep.person_count[0] = max(int(ep.person_count[0]), 1)


def build(kind, monitor=MONITOR):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup()
    ep = BatchEpisode(prm, sc, w_ref, monitor=monitor, **KINDS[kind], **kw)
    place_pedestrian(ep, world, sc.pose0[0])
    return ep, world, prm


def ref_params(world):
    act = {"stop": R.STOP, "slowdown": R.SLOWDOWN, "limit": R.LIMIT, "approach": R.APPROACH}
    zones = [R.circle(act[z.action], z.radius, z.min_points, z.slowdown_ratio, z.linear_limit, z.angular_limit) if z.vertices is None else
             R.polygon(act[z.action], z.vertices, z.min_points, z.slowdown_ratio, z.linear_limit, z.angular_limit) for z in MONITOR.zones]
    return R.params(zones, M=MONITOR.steps(), sim_dt=MONITOR.simulation_time_step, res=world.resolution, origin=tuple(world.origin))


def state(ep):
    names = STATE + (MONITOR_STATE if ep.monitor is not None else ()) + (EP.PLANT_STATE if ep.plant is not None else ())
    out = {k: getattr(ep, k).cpu().numpy().copy() for k in names}
    out.update({"res_" + k: v.cpu().numpy().copy() for k, v in ep.res.items()})
    return out


@pytest.fixture(scope="module", params=sorted(KINDS))
def eager(request):
    ep, world, prm = build(request.param)
    Z = len(MONITOR.zones)
    assert ep.cmd_safe.shape == (B, 2) and ep.monitor_action.shape == (B, 4) and ep.monitor_points.shape == (B, Z) and ep.monitor_ratio.shape == (B,)
    c = ep._c.monitor
    assert (c.B, c.n_beams, c.Z, c.M, c.on_device) == (B, SENSOR.n_beams, Z, 12, 1) and c.resolution == world.resolution
    assert c.robot_pose == ep.pose.data_ptr() and c.cmd == ep.cmd_vel.data_ptr() and c.beam_kind == ep.beam_kind.data_ptr() and c.beam_cell == ep.beam_cell.data_ptr()
    if ep.plant is not None:
        assert ep._c.plant.cmd == ep.cmd_safe.data_ptr()
    recs, states = [], []
    for _ in range(TICKS):
        timing = {}
        recs.append(ep.tick(record=True, timing=timing))
        ep.synchronize()
        assert timing["monitor_ms"] > 0.0
        states.append(state(ep))
    return dict(kind=request.param, ep=ep, recs=recs, states=states, world=world, prm=prm)


def test_every_ticks_safe_command_is_the_yardsticks_and_is_what_was_executed(eager):
    p, prm, world = ref_params(eager["world"]), eager["prm"], eager["world"]
    plant_p = EP.ref_params(PLANT, prm, world)
    dt = np.float64(prm.dt)
    changed, deciders = 0, set()
    for k, (r, st) in enumerate(zip(eager["recs"], eager["states"])):
        got = dict(cmd_out=r.cmd_safe, action=r.monitor_action, zone_points=r.monitor_points, ratio=r.monitor_ratio)
        want = R.run(p, r.robot_pose, r.cmd_vel, r.beam_kind, r.beam_cell, r.monitor_heading_cs, r.monitor_step_cs)
        assert R.same(got, want), (k, [n for n in got if got[n].tobytes() != want[n].tobytes()])
        assert R.angles_close(r.monitor_heading_cs, r.monitor_step_cs, r.robot_pose, r.cmd_vel, p["sim_dt"], p["M"]) and want["finite"].all(), k
        assert V.same_bits(st["cmd_safe"], r.cmd_safe) and V.same_bits(st["cmd_vel"], r.cmd_vel), k        # cmd_vel stays the controller's
        slowed = r.monitor_ratio < 1.0
        changed += int(slowed.sum())
        deciders |= set(r.monitor_action[slowed, 1].tolist())
        assert V.same_bits(r.cmd_safe[~slowed], r.cmd_vel[~slowed]) and (r.monitor_action[:, 3] > 0).any(), k
        if eager["kind"] == "memory_plant":                                 # the plant executed cmd_safe
            before = (r.robot_pose, r.speed, r.plant_queue_before, r.plant_tick_before)
            tick = {"cmd": r.cmd_safe, "agents": r.plant_agents, "count": r.plant_agent_count}
            (pose, twist, queue, _), contact, _ = plant_ref.step(before, tick, plant_p, r.heading_cs)
            assert V.same_bits(r.pose_after, pose) and V.same_bits(r.speed_after, twist) and np.array_equal(r.plant_contact, contact), k
            assert V.same_bits(r.plant_queue_after, queue), k
        else:                                                               # the motion model moved what the monitor changed, with cmd_safe
            onpath = (r.cmd_source == 0) & ~slowed
            assert V.same_bits(r.pose_after[onpath], r.result["path"][onpath, 0, :]), k
            x, y, th, v, w = r.robot_pose[:, 0], r.robot_pose[:, 1], r.robot_pose[:, 2], r.cmd_safe[:, 0], r.cmd_safe[:, 1]
            moved = np.stack([x + v * np.cos(th) * dt, y + v * np.sin(th) * dt, th + w * dt], axis=1)
            assert np.abs(r.pose_after[~onpath] - moved[~onpath]).max(initial=0.0) <= 1e-12, k
            assert V.same_bits(st["speed"], r.cmd_safe), k                   # ... and is the next warm start's speed
    print(eager["kind"], "robot-ticks with ratio < 1:", changed, "deciding zones:", sorted(deciders))
    assert changed >= TICKS and 1 in deciders                                # robot 0 stands within 1.3 m of the pedestrian all along


def test_graph_replay_equals_the_eager_ticks(eager):
    g, _, _ = build(eager["kind"])
    g.capture_graph()
    for _ in range(TICKS):
        g.replay()
    g.synchronize()
    want = eager["states"][-1]
    for k, v in state(g).items():
        assert V.same_bits(v, want[k]), k


def test_two_shards_equal_the_unsharded_rows(eager):
    from nav2_social_mpc_controller_amd.episode import ShardedEpisode
    prm, world, sc, w_ref, kw = setup()
    two = ShardedEpisode(prm, sc, w_ref, None, None, None, shards=2, graphs=True, monitor=MONITOR, **KINDS[eager["kind"]], **kw)
    assert [p.B for p in two.parts] == [8, 8] and all(p.monitor is MONITOR for p in two.parts)
    place_pedestrian(two.parts[0], world, sc.pose0[0])
    for _ in range(TICKS):
        two.tick()
    want = eager["states"][-1]
    for name in MONITOR_STATE[:4] + ("pose", "cmd_vel", "speed"):
        assert V.same_bits(two.gather(name).cpu().numpy(), want[name]), name


def test_without_monitor_nothing_is_allocated_and_the_episode_is_the_one_without_the_keyword():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup()
    more = KINDS["memory_plant"]
    plain, none = BatchEpisode(prm, sc, w_ref, **more, **kw), BatchEpisode(prm, sc, w_ref, monitor=None, **more, **kw)
    for ep in (plain, none):
        assert ep.monitor is None and not hasattr(ep._c, "monitor") and ep._c.plant.cmd == ep.cmd_vel.data_ptr()
        for name in MONITOR_STATE:
            assert not hasattr(ep, name), name
    for k in range(3):
        timing = {}
        a, b = plain.tick(record=True, timing=timing), none.tick(record=True)
        assert "monitor_ms" not in timing
        for name in MONITOR_STATE:
            assert getattr(a, name) is None and getattr(b, name) is None, name
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, dict):
                assert all(V.same_bits(x[n], y[n]) for n in x), (k, f.name)
            elif x is not None:
                assert V.same_bits(x, y), (k, f.name)
        for name, v in state(plain).items():
            assert V.same_bits(state(none)[name], v), (k, name)
    no_sensor = {n: v for n, v in kw.items() if n != "sensor"}
    with pytest.raises(ValueError, match=r"monitor needs sensor=SensorParams\(\.\.\.\): it reads the scan"):
        BatchEpisode(prm, sc, w_ref, monitor=MONITOR, **no_sensor)
    with pytest.raises(ValueError):
        BatchEpisode(prm, sc, w_ref, monitor=dict(zones=()), **kw)
