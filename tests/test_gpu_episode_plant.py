"""Closed-loop episodes with the robot plant (BatchEpisode(plant=PlantParams(...))): the 12 robots of
tests/test_gpu_episode_sensed.py on the 256 x 192 world (private persons, and a shared world with a pool of 24 pedestrians and
the other robots), 8 recorded ticks. Every tick's pose, speed, queue, counter and contact are the yardstick's
(tests/plant_ref.py) on that tick's recorded inputs, given the recorded heading_cs; the next tick's `speed` is the executed
twist; graph replay equals the eager ticks; plant=None is the plain episode bit for bit; PlantParams.ideal() is the motion
model itself. Two constructed scenes, checked on the CPU with the yardstick alone first: a robot planned straight through a
wall stops in front of it (and its obstacle_collision_samples stay 0 where the episode without the plant counts some), and
two robots of a shared world driven head-on end no closer than they were when contact began.

No assertion on how well the robots then drive."""
import dataclasses

import numpy as np
import pytest

import plant_ref as R
import visibility_ref as V
from nav2_social_mpc_controller_amd.params import MetricsParams, OptimizerParams, PlantParams, SharedWorldParams, TrajectorizerParams
import test_gpu_episode_sensed as SE

pytestmark = pytest.mark.gpu

B, M, N, SIZE = SE.B, SE.M, SE.N, SE.SIZE
TICKS = 8
PLANT = PlantParams(max_accel=2.5, max_decel=4.0, max_ang_accel=3.2, latency_ticks=2, substeps=4, robot_radius=0.24, agent_radius=0.3)
STATE = ("pose", "speed", "persons", "person_count", "cmd_vel", "costmap", "costmap_origin", "costmap_cell", "people", "has_people")
PLANT_STATE = ("plant_queue", "plant_tick", "plant_contact", "heading_cs")


def ref_params(plant, prm, world):
    """The yardstick's parameters of an episode's plant: what BatchSolver.plant_c hands the library."""
    dv_up, dv_down, dw = plant.deltas(prm.dt)
    walls = world is not None
    return R.params(S=plant.substeps, L=plant.latency_ticks, dt=prm.dt, v_min=prm.v_min, v_max=prm.v_max, w_max=prm.w_max, dv_up=dv_up,
                    dv_down=dv_down, dw=dw, contact_dist=plant.contact_dist(), world=world.map if walls else None,
                    origin=world.origin if walls else (0.0, 0.0), res=world.resolution if walls else 1.0,
                    footprint_d2=plant.footprint_d2(world.resolution if walls else 1.0), wall_min_cost=plant.wall_min_cost,
                    unknown_is_wall=plant.unknown_is_wall, outside_is_wall=plant.outside_is_wall)


def held_to_the_yardstick(r, p, rows=None):
    """One recorded tick against the yardstick on its recorded inputs (rows: the robots looked at; default all)."""
    rows = slice(None) if rows is None else rows
    before = (r.robot_pose[rows], r.speed[rows], r.plant_queue_before[rows], r.plant_tick_before[rows])
    tick = {"cmd": r.cmd_vel[rows], "agents": r.plant_agents[rows], "count": r.plant_agent_count[rows]}
    (pose, twist, queue, ticks), contact, counters = R.step(before, tick, p, r.heading_cs[rows])
    assert V.same_bits(r.pose_after[rows], pose) and V.same_bits(r.speed_after[rows], twist)
    assert V.same_bits(r.plant_queue_after[rows], queue) and np.array_equal(r.plant_tick_after[rows], ticks) and r.plant_tick_after.dtype == np.uint32
    assert r.plant_contact.dtype == np.int32 and np.array_equal(r.plant_contact[rows], contact)
    assert R.heading_close(r.heading_cs[rows], before)
    return counters


def build(kind, plant=PLANT, **more):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = SE.setup(kind)
    kw.update(more)
    return BatchEpisode(prm, sc, w_ref, plant=plant, **kw), world, prm


def state(ep):
    names = STATE + (PLANT_STATE if ep.plant is not None else ())
    out = {k: getattr(ep, k).cpu().numpy().copy() for k in names}
    out.update({"res_" + k: v.cpu().numpy().copy() for k, v in ep.res.items()})
    return out


@pytest.fixture(scope="module", params=["private", "shared"])
def eager(request):
    ep, world, prm = build(request.param)
    assert ep.plant_queue.shape == (B, 8, 2) and ep.plant_tick.shape == (B,) and ep.plant_contact.shape == (B, 2) and ep.heading_cs.shape == (B, 2)
    assert ep._c.plant.agents == ep.persons.data_ptr() and ep._c.plant.count == ep.person_count.data_ptr() and ep._c.plant.cmd == ep.cmd_vel.data_ptr()
    assert ep._c.plant.world == ep.world_map.data_ptr() and (ep._c.plant.Hx, ep._c.plant.Hy) == (256, 192)
    recs, states = [], []
    for _ in range(TICKS):
        timing = {}
        recs.append(ep.tick(record=True, timing=timing))
        ep.synchronize()
        assert timing["plant_ms"] > 0.0
        states.append(state(ep))
    return dict(kind=request.param, ep=ep, recs=recs, states=states, world=world, prm=prm)


def test_every_ticks_pose_speed_queue_counter_and_contact_are_the_yardsticks(eager):
    p = ref_params(PLANT, eager["prm"], eager["world"])
    total = dict.fromkeys(R.COUNTERS, 0)
    for k, (r, st) in enumerate(zip(eager["recs"], eager["states"])):
        counters = held_to_the_yardstick(r, p)
        for name in R.COUNTERS:
            total[name] += int(counters[name].sum())
        assert V.same_bits(st["pose"], r.pose_after) and V.same_bits(st["speed"], r.speed_after), k    # the episode's state is what the call wrote
        assert (r.plant_tick_after == k + 1).all() and V.same_bits(r.plant_queue_after[:, k % 2], r.cmd_vel), k
        if k > 0:                                                           # the next tick's measured twist is the executed one
            assert V.same_bits(r.speed, eager["recs"][k - 1].speed_after) and V.same_bits(r.robot_pose, eager["recs"][k - 1].pose_after), k
            assert V.same_bits(r.plant_queue_before, eager["recs"][k - 1].plant_queue_after), k
        if k < 2:                                                           # two ticks of latency: (0, 0) is executed first, from the start speed
            assert (np.abs(r.speed_after[:, 0]) <= np.abs(r.speed[:, 0])).all(), k
    print(eager["kind"], {name: v for name, v in total.items() if v})
    assert total["full"] > 0 and total["rate_limited"] > 0 and total["bad_state"] == 0
    if eager["kind"] == "shared":                                           # the agents are the gather's rows, the other robots among them
        assert all((r.person_source >= M).any() for r in eager["recs"])


def test_graph_replay_equals_the_eager_ticks(eager):
    g, _, _ = build(eager["kind"])
    g.capture_graph()
    for _ in range(TICKS):
        g.replay()
    g.synchronize()
    want = eager["states"][-1]
    for k, v in state(g).items():
        assert V.same_bits(v, want[k]), k


def test_without_plant_nothing_is_allocated_and_the_episode_is_the_plain_one():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = SE.setup("private")
    plain, none = BatchEpisode(prm, sc, w_ref, **kw), BatchEpisode(prm, sc, w_ref, plant=None, **kw)
    for ep in (plain, none):
        assert ep.plant is None and not hasattr(ep._c, "plant")
        for name in PLANT_STATE:
            assert not hasattr(ep, name), name
    for k in range(3):
        timing = {}
        a, b = plain.tick(record=True, timing=timing), none.tick(record=True)
        assert "plant_ms" not in timing
        for name in ("plant_agents", "plant_agent_count", "plant_queue_before", "plant_tick_before", "plant_queue_after", "plant_tick_after",
                     "plant_contact", "heading_cs", "speed_after"):
            assert getattr(a, name) is None and getattr(b, name) is None, name
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, dict):
                assert all(V.same_bits(x[n], y[n]) for n in x), (k, f.name)
            elif x is not None:
                assert V.same_bits(x, y), (k, f.name)
        for name, v in state(plain).items():
            assert V.same_bits(state(none)[name], v), (k, name)
        # the plain episode's move: an optimised robot lands on the first optimised pose, speed is the command
        assert V.same_bits(a.pose_after[a.cmd_source == 0], a.result["path"][a.cmd_source == 0, 0, :]) and V.same_bits(state(plain)["speed"], a.cmd_vel)
    with pytest.raises(ValueError):
        BatchEpisode(prm, sc, w_ref, plant=dict(max_accel=1.0), **kw)
    with pytest.raises(ValueError):                                         # a footprint beyond 15 cells of 0.05 m
        BatchEpisode(prm, sc, w_ref, plant=PlantParams(robot_radius=0.8), **kw)


def test_the_ideal_plant_is_the_motion_model():
    ep, world, prm = build("private", plant=PlantParams.ideal())
    dt = np.float64(prm.dt)
    clamp = lambda a, lo, hi: np.where(a < lo, lo, np.where(a > hi, hi, a))
    for k in range(TICKS):
        r = ep.tick(record=True)
        x, y, th, v, w = r.robot_pose[:, 0], r.robot_pose[:, 1], r.robot_pose[:, 2], r.speed[:, 0], r.speed[:, 1]
        v1 = v + (clamp(r.cmd_vel[:, 0], np.float64(prm.v_min), np.float64(prm.v_max)) - v)
        w1 = w + (clamp(r.cmd_vel[:, 1], -np.float64(prm.w_max), np.float64(prm.w_max)) - w)
        c, s = r.heading_cs[:, 0], r.heading_cs[:, 1]
        assert V.same_bits(r.speed_after, np.stack([v1, w1], axis=1)), k
        assert V.same_bits(r.pose_after, np.stack([x + (v1 * c) * dt, y + (v1 * s) * dt, th + w1 * dt], axis=1)), k   # every row, usable solve or not
        assert np.array_equal(r.plant_contact, np.tile(np.array([0, 1], np.int32), (B, 1))) and R.heading_close(r.heading_cs, (r.robot_pose, r.speed)), k
        # ... and the command itself up to the two roundings of v + (vt - v), at magnitudes below 4
        assert np.abs(r.speed_after - np.stack([clamp(r.cmd_vel[:, 0], prm.v_min, prm.v_max), clamp(r.cmd_vel[:, 1], -prm.w_max, prm.w_max)], axis=1)).max() <= 2.0 ** -50
        held_to_the_yardstick(r, ref_params(PlantParams.ideal(), prm, world))


# ---- two constructed scenes ---------------------------------------------------------------------------------------------------
WALL_PLANT = PlantParams(substeps=4, robot_radius=0.35, agent_radius=None)     # one cell more than the metrics' robot_radius of 0.3 m
WALL_TICKS, WALL_AHEAD, WALL_HALF = 48, 1.2, 6


def wall_scene(block=True):
    """The 12 robots on an empty floor, straight plans, no obstacle critic; block: 13 x 13 lethal cells 1.2 m in front of
    robot 0, across its plan."""
    from nav2_social_mpc_controller_amd.episode import arc_plans
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world
    prm = dataclasses.replace(OptimizerParams.readme(), obstacle_weight=0.0)
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    world = make_world(256, 192, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15), discs=0)
    pose0 = scenes_in_world(prm, world, B, N, size_x=SIZE, size_y=SIZE).pose0
    centre = pose0[0, :2] + WALL_AHEAD * np.array([np.cos(pose0[0, 2]), np.sin(pose0[0, 2])])
    cx, cy = np.floor((centre - world.origin) / world.resolution).astype(int)
    assert WALL_HALF + 4 <= cx < 256 - WALL_HALF - 4 and WALL_HALF + 4 <= cy < 192 - WALL_HALF - 4
    if block:
        world.map[cy - WALL_HALF:cy + WALL_HALF + 1, cx - WALL_HALF:cx + WALL_HALF + 1] = 254
    sc = scenes_in_world(prm, world, B, N, size_x=SIZE, size_y=SIZE)
    assert np.array_equal(sc.pose0, pose0)                                     # the block took nobody's start cell
    plan, plan_len = arc_plans(sc.pose0, np.zeros(B))
    kw = dict(plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=1.2, plan_window=(4.0, 10.0), obstacles_from_costmap=True, world=world,
              metrics=MetricsParams(robot_radius=0.3))
    return prm, world, sc, kw


def wall_distance_cells(world, xy):
    """The distance in cells from the cell of xy to the nearest lethal cell of the world."""
    cell = np.floor((np.asarray(xy) - world.origin) / world.resolution)
    ys, xs = np.nonzero(world.map >= 254)
    return float(np.sqrt(((xs - cell[0]) ** 2 + (ys - cell[1]) ** 2).min()))


def test_a_robot_planned_through_a_wall_stops_in_front_of_it():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.solver import METRIC_COLS
    prm, world, sc, kw = wall_scene()
    p = ref_params(WALL_PLANT, prm, world)
    reach = np.sqrt(WALL_PLANT.footprint_d2(world.resolution))
    # the yardstick alone: robot 0 at full command straight at the block stops with no wall cell within its footprint
    st = (sc.pose0[:1].copy(), np.zeros((1, 2)), np.zeros((1, 8, 2)), np.zeros(1, np.uint32))
    tick = {"cmd": np.array([[0.6, 0.0]]), "agents": np.zeros((1, 1, 5)), "count": np.zeros(1, np.int32)}
    assert wall_distance_cells(world, st[0][0, :2]) > reach + 4
    flags = []
    for _ in range(WALL_TICKS):
        st, contact, _ = R.step(st, tick, p, R.numpy_heading(st[0]))
        flags.append(int(contact[0, 0]))
        assert wall_distance_cells(world, st[0][0, :2]) > reach
    assert flags[0] == 0 and 1 in flags and wall_distance_cells(world, st[0][0, :2]) <= reach + 2.0      # ... one cell's step in front of it
    # the device: the same episode with and without the plant
    with_plant, without = BatchEpisode(prm, sc, sc.pose0[:, 0] * 0.0, plant=WALL_PLANT, **kw), BatchEpisode(prm, sc, sc.pose0[:, 0] * 0.0, **kw)
    recs = [with_plant.tick(record=True) for _ in range(WALL_TICKS)]
    for _ in range(WALL_TICKS):
        without.tick()
    for k, r in enumerate(recs):
        held_to_the_yardstick(r, p)
        assert wall_distance_cells(world, r.pose_after[0, :2]) > reach, k
    col = METRIC_COLS.index("obstacle_collision_samples")
    collisions = with_plant.metrics()[0, col], without.metrics()[0, col]
    print("robot 0: obstacle_collision_samples with / without the plant:", collisions, "flags:", [int(r.plant_contact[0, 0]) for r in recs])
    assert collisions[0] == 0.0 and collisions[1] > 0.0
    assert any(int(r.plant_contact[0, 0]) & 1 for r in recs)                          # stopped by the wall, and in front of it
    assert wall_distance_cells(world, recs[-1].pose_after[0, :2]) <= reach + 2.0


HEAD_ON_TICKS, HEAD_ON_GAP = 30, 1.5


def test_two_robots_driven_head_on_end_no_closer_than_when_contact_began():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, arc_plans
    prm, world, sc, kw = wall_scene(block=False)
    prm = dataclasses.replace(prm, social_weight=0.0, agent_angle_weight=0.0, proxemics_weight=0.0)   # the controllers do not give way
    plant = PlantParams(substeps=4)
    p = ref_params(plant, prm, world)
    dist = lambda pose: float(np.hypot(*(pose[0, :2] - pose[1, :2])))
    # robots 0 and 1 face each other on free floor, 1.5 m apart, where the other ten do not come within 30 ticks
    mid = world.origin + 0.5 * np.array([256, 192]) * world.resolution + np.array([-3.0, -2.0])
    sc.pose0[0], sc.pose0[1] = (mid[0] - HEAD_ON_GAP / 2, mid[1], 0.0), (mid[0] + HEAD_ON_GAP / 2, mid[1], np.pi)
    assert wall_distance_cells(world, sc.pose0[0, :2]) > 20 and wall_distance_cells(world, sc.pose0[1, :2]) > 20
    assert np.hypot(*(sc.pose0[2:, None, :2] - sc.pose0[None, :2, :2]).reshape(-1, 2).T).min() > 2.0   # the others are out of the way
    # the yardstick alone: both at full command, each seeing the other where the period started
    st = (sc.pose0[:2].copy(), np.zeros((2, 2)), np.zeros((2, 8, 2)), np.zeros(2, np.uint32))
    began = None
    for _ in range(HEAD_ON_TICKS):
        agents = np.zeros((2, 1, 5))
        agents[:, 0, :2] = st[0][::-1, :2]
        d0 = dist(st[0])
        st, contact, _ = R.step(st, {"cmd": np.array([[0.6, 0.0]] * 2), "agents": agents, "count": np.ones(2, np.int32)}, p, R.numpy_heading(st[0]))
        if began is None and (contact[:, 0] & 8).any():
            began = d0
    assert began is not None and began < plant.contact_dist() and dist(st[0]) >= began and (contact[:, 0] & 2).all() and (st[1][:, 0] == 0.0).all()
    # the device: a shared world without a pool, the robots in each other's rows
    plan, plan_len = arc_plans(sc.pose0, np.zeros(B))
    kw.update(plan=plan, plan_len=plan_len, shared=SharedWorldParams(robots_as_people=True))
    ep = BatchEpisode(prm, sc, sc.pose0[:, 0] * 0.0, plant=plant, **kw)
    recs = [ep.tick(record=True) for _ in range(HEAD_ON_TICKS)]
    began = None
    for k, r in enumerate(recs):
        held_to_the_yardstick(r, p)
        if began is None and (r.plant_contact[:2, 0] & 8).any():
            began = dist(r.robot_pose)
    print("head-on: distance at the start", dist(recs[0].robot_pose), "when contact began", began, "at the end", dist(recs[-1].pose_after),
          "flags", [r.plant_contact[:2, 0].tolist() for r in recs[-3:]])
    assert began is not None and began < plant.contact_dist()
    assert dist(recs[-1].pose_after) >= began
