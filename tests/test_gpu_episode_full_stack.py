"""The closed-loop tick with every optional stage switched on at once, as two stacks (scan_detector excludes visibility and
detector, shared excludes the private crowd): 7 robots (one short of two workgroups of four) on an open 96 x 96 world at
0.05 m with 40 x 40 windows, a 72-beam scan, 8 recorded ticks. As in tests/test_gpu_episode_plan_repair.py every robot's plan
runs straight along an axis or a diagonal and a person (in `fleet` a pedestrian of the pool) stands on it 0.6 m ahead; the
robot's heading is turned 0.1 rad off the plan, so that no pair of the crowd steps is exactly head-on.

  fleet    world, planner + goal, plan window, field of view, grids from the world map, order hint, scene parameters; a shared
           world with a reactive pool; the scan with its memory; detections from the scan, tracker, plan repair, collision
           monitor, plant, metrics
  private  world, arc plans, plan window, field of view, grids from the world map; a private reactive crowd with groups; line
           of sight (1 m), detector, tracker; the memoryless scan; plan repair, collision monitor, plant, metrics

tests/episode_chain_checks.py walks every recorded tick in launch order and holds every stage against its own yardstick on
what the record holds of the stage before it; graph replay, two shards and a recording, timed episode are held against the
eager ticks byte for byte. One test needs no GPU: the two stacks together switch on every keyword BatchEpisode declares.

No assertion on how well the robots then drive."""
import numpy as np
import pytest

import episode_chain_checks as CC
import test_gpu_episode_collision_monitor as CMT
import test_gpu_episode_detector as DE
import test_gpu_episode_plan_repair as PRT
import test_gpu_episode_plant as EP
import test_gpu_episode_scan_people as SPT
from nav2_social_mpc_controller_amd.params import (CrowdGroupParams, CrowdParams, DetectorParams, GlobalPlanParams, MetricsParams, MonitorParams,
                                                   MonitorZone, ObstacleMemoryParams, OptimizerParams, PlantParams, PoolCrowdParams, SensorParams,
                                                   SharedWorldParams, TrackerParams, TrajectorizerParams, VisibilityParams, scene_param_rows)
from test_gpu_episode_tracker import TRACKER_STATE

B, N, SIZE, TICKS, FOV, L, M = 7, 3, 40, 8, 1.2, 200, 8
AHEAD, TURNED, GOAL_AHEAD = 0.6, 0.1, 1.5
WINDOW = (4.0, 10.0)
STACKS = ("fleet", "private")
ORACLE_TICK = 3                                                             # the tracker has confirmed its tracks: the scenes have people
SENSOR = SensorParams(n_beams=72, agent_radius=0.2)                       # the robots beside a robot, 0.5 m away, stay out of its STOP circle
# every effect of the detector within 8 ticks of 7 robots, and misses rare enough for the person ahead to be confirmed
DETECTOR = DetectorParams(body_radius=0.25, p_miss=0.1, sigma=0.03, sigma_growth=0.002, clutter_candidates=3, p_clutter=0.3, clutter_range=5.0,
                          seed=10)
# the person 0.6 m ahead stands in the SLOWDOWN circle all along; the STOP circle ends short of its body, so the robots keep moving
MONITOR = MonitorParams(zones=(MonitorZone(action="stop", radius=0.2, min_points=2),
                               MonitorZone(action="slowdown", radius=1.3, min_points=1, slowdown_ratio=0.75),
                               MonitorZone(action="limit", vertices=((0.0, -0.5), (1.6, -0.5), (1.6, 0.5), (0.0, 0.5)), min_points=3, linear_limit=0.45,
                                           angular_limit=0.8),
                               MonitorZone(action="approach", vertices=((-0.1, -0.1), (0.1, -0.1), (0.1, 0.1), (-0.1, 0.1)), min_points=2)),
                        time_before_collision=1.2, simulation_time_step=0.1)
PLANT = PlantParams(max_accel=2.5, max_decel=4.0, max_ang_accel=3.2, latency_ticks=1, substeps=4, robot_radius=0.24, agent_radius=0.15)
# keywords neither stack switches on, each with its reason
NOT_SWITCHED_ON = ("device",               # the one GPU
                   "outside_cost",         # a number the roll's own test varies; the default is what the yardsticks are given
                   "obstacle_min_cost",    # of the grid computed once at construction, not of a tick
                   "unknown_is_obstacle",  # the same
                   "person_speed",         # desired speeds: a value of the crowd step, no hand-over
                   "pool_speed",           # the same for the pool
                   "od_resolution")        # of host-given grids (od_indexes, od_origin): obstacles_from_costmap takes their place


def floor():
    """The world, the robots, the direction of every robot's plan (angle and unit vector) and where its person stands: AHEAD
    down the plan."""
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world
    prm = OptimizerParams.readme()
    world = make_world(96, 96, 0.05, origin=(-1.0, 0.5), discs=0)
    options = dict(size_x=SIZE, size_y=SIZE, margin=1.3, people_reach=1.2, standing_fraction=0.0)
    sc = place(scenes_in_world(prm, world, B, N, **options), world)
    along = np.array([slot(k, world)[1] for k in range(B)])
    ahead = np.stack([np.cos(along), np.sin(along)], axis=1)
    return prm, world, sc, options, along, ahead, sc.pose0[:, :2] + AHEAD * ahead


def slot(k, world):
    """(position, direction of the plan) of slot k: a row across the middle of the floor, 0.5 m apart, the even ones headed up the
    floor and the odd ones down it. A body 0.6 m ahead of one slot is 0.78 m from the slots beside it and 1 m or more from every
    other such body, so a scan shows it as a segment of its own, and 1.5 m ahead of every slot is free floor. With a person in
    their way the robots creep, a few centimetres in 8 ticks: the even slots lie 2 .. 5 mm short of the line at which the window
    rolls on by a cell (include/smpc_local_costmap.h: the pose passes origin + (cell + 1) * resolution + the half window), so
    that the roll has windows to move; the odd ones a centimetre apart off the row (no two robots mirror each other)."""
    res, (ox, oy) = world.resolution, world.origin
    x, y = ox + 0.5 * 96 * res - 1.5 + 0.5 * k, oy + 0.5 * 96 * res
    if k % 2:
        return np.array([x, y + 0.01 * k]), -np.pi / 2
    half = ((SIZE - 1.0 + 0.5) * res) / 2.0
    line = oy + half + np.ceil((y - half - oy) / res) * res
    return np.array([x, line - 0.002 - 0.0005 * k]), np.pi / 2


def place(sc, world):
    """The robots of `sc` (their persons with them) on slots 0 .. 6, turned TURNED off the slot's direction: 7 robots with
    a person in front of each get in each other's way anywhere else on a floor of 4.8 m. The windows follow at the first tick's
    roll."""
    start = np.stack([slot(k, world)[0] for k in range(B)])
    sc.people[:, :, 0:2, :] += (start - sc.pose0[:, :2])[:, None, :, None]
    sc.pose0[:, :2] = start
    sc.pose0[:, 2] = np.array([slot(k, world)[1] for k in range(B)]) + TURNED
    return sc


def stack_kwargs(stack):
    """(params, world, scenes, w_ref, BatchEpisode's keywords, the parameter sets of scene_params and every robot's) of a
    stack, on the host alone."""
    from nav2_social_mpc_controller_amd.episode import arc_plans
    from nav2_social_mpc_controller_amd.scenes import crowd_groups, pool_waypoints, scenes_in_world
    prm, world, sc, options, along, ahead, spot = floor()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    kw = dict(world=world, traj_params=tp, plan_window=WINDOW, fov_angle=FOV, obstacles_from_costmap=True, sensor=SENSOR, tracker=TrackerParams(),
              repair=PRT.RP, monitor=MONITOR, plant=PLANT, metrics=MetricsParams())
    if stack == "fleet":
        presets = [prm, prm.replace(distance_weight=1.5 * prm.distance_weight)]
        which = np.arange(B) % 2
        centre = np.asarray(world.origin) + 0.5 * 96 * 0.05
        walker = np.concatenate([centre + [1.0, 1.4], [-0.5, 0.05, 0.0]])      # along the far side of the floor, 0.9 m from the nearest body
        pool = np.concatenate([np.concatenate([spot, np.zeros((B, 3))], axis=1), walker[None]])   # a standing pedestrian per robot, and one who walks past
        wp, n_wp = pool_waypoints(world, pool, K=2)
        kw.update(planner=GlobalPlanParams(max_poses=L), goal=np.ascontiguousarray(sc.pose0[:, :2] + GOAL_AHEAD * ahead), order_hint=True,
                  scene_params=scene_param_rows(presets, which), shared=SharedWorldParams(), pool=pool, pool_crowd=PoolCrowdParams(),
                  pool_waypoints=wp, pool_n_waypoints=n_wp, sensor_memory=ObstacleMemoryParams(), scan_detector=SPT.SD)
        return prm, world, sc, np.zeros(B), kw, presets, which
    # private: person 0 of every robot stands on its plan (at every step of the scenes' constant-velocity people)
    wide = place(scenes_in_world(prm, world, B, N, **dict(options, size_x=96, size_y=96)), world)   # the same people; waypoints on the whole floor
    for scenes in (sc, wide):
        scenes.people[:, :, 0:2, 0] = spot[:, None, :]
        scenes.people[:, :, 4:6, 0] = 0.0
    gid, wp, n_wp = crowd_groups(wide, share=1.0, K=2)
    plan, plan_len = arc_plans(np.concatenate([sc.pose0[:, :2], along[:, None]], axis=1), np.zeros(B), L=L, ds=0.05)
    kw.update(plan=plan, plan_len=plan_len, crowd=CrowdParams(), person_waypoints=wp, person_n_waypoints=n_wp, person_groups=gid,
              crowd_groups=CrowdGroupParams(), visibility=VisibilityParams(max_range=1.0), detector=DETECTOR)
    return prm, world, sc, np.zeros(B), kw, None, None


def build(stack):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw, presets, which = stack_kwargs(stack)
    return BatchEpisode(prm, sc, w_ref, **kw), (world, kw, prm, presets, which)


def carried(ep):
    """The buffers a tick reads before it writes them: what a warm-up tick has to give back."""
    names = ["pose", "speed", "persons", "person_count", "mem_path", "mem_cmds", "mem_valid", "mem_length", "order", "plan", "plan_len", "plan_start",
             "metrics_acc", "tracks", "track_meta", "track_next_id", "plant_queue", "plant_tick"]
    names += ["agents", "person_source", "pool_cursor", "obstacle_memory", "obstacle_memory_cell"] if ep.shared is not None else ["person_cursor", "draw_state"]
    return names


def outputs(ep):
    """The output buffers the stage tests' STATE tuples name, of the stages this episode has."""
    names = set(EP.STATE + EP.PLANT_STATE + CMT.MONITOR_STATE + PRT.REPAIR_STATE + TRACKER_STATE + ("beam_kind", "beam_cell", "cmd_source", "proj_error"))
    names |= set(SPT.SCAN_STATE + ("pool_next",)) if ep.shared is not None else set(DE.DETECTOR_STATE + ("seen_persons", "seen_count", "person_seen"))
    return sorted(names)


def state(ep, names=None):
    ep.synchronize()
    out = {k: getattr(ep, k).cpu().numpy().copy() for k in (sorted(set(carried(ep)) | set(outputs(ep))) if names is None else names)}
    if names is None:
        out.update({"res_" + k: v.cpu().numpy().copy() for k, v in ep.res.items()})
    return out


def assert_same_state(got, want, what):
    assert sorted(got) == sorted(want), what
    for k, v in want.items():
        assert CC.same_bits(got[k], v), (what, k)


def assert_launch_order(ep, keys):
    """The keys of a tick's timing dict (insertion order: the real launch order) are BatchEpisode.STAGES restricted to the stages
    the episode launches (the obstacle memory launches in the sensed costmap's place), with the core chain at Core's position."""
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.episode_stages import Core, ObstacleMemory, Sensed
    order = [S for S in BatchEpisode.STAGES if S is Core or (S in ep.stages and not (S is Sensed and ObstacleMemory in ep.stages))]
    assert len(order) == 11                                                 # either stack launches ten optional stages
    stage_keys = {S.TIMING + "_ms" for S in BatchEpisode.STAGES if S is not Core}
    core = ["people_ms", "format_ms", "project_ms", "solve_ms", "store_ms"]
    want = sum((core if S is Core else [S.TIMING + "_ms"] for S in order), [])
    assert [k for k in keys if k in stage_keys or k in core] == want, keys
    assert [k for k in keys if k not in want] == ["window_ms", "trajectorize_ms"] + (["nearest_after_ms"] if ep.shared is not None else []), keys
    assert keys.index("local_costmap_ms") < keys.index("window_ms") < keys.index("trajectorize_ms") < keys.index(want[1])
    if ep.shared is not None:
        assert keys.index("nearest_after_ms") == keys.index("metrics_ms") - 1


@pytest.fixture(scope="module", params=STACKS)
def eager(request):
    ep, (world, kw, prm, presets, which) = build(request.param)
    info = CC.episode_info(ep, world, kw, prm, presets, which)
    start = state(ep, carried(ep))
    recs, states = [], []
    for _ in range(TICKS):
        recs.append(ep.tick(record=True))
        states.append(state(ep))
    return dict(stack=request.param, ep=ep, info=info, recs=recs, states=states, start=start)


@pytest.mark.gpu
def test_every_stage_reads_what_the_stage_before_wrote(eager):
    recs, info, stack = eager["recs"], eager["info"], eager["stack"]
    facts = [CC.check_tick(r, recs[k + 1] if k + 1 < TICKS else None, info, oracle=k == ORACLE_TICK) for k, r in enumerate(recs)]
    # the conditions under which the walk above shows something, on the yardsticks' outputs alone
    repaired = np.sum([f["repaired"] for f in facts], axis=0)
    slowed = int(np.sum([f["monitor_slowed"] for f in facts]))
    found = np.array([f["scan_count" if stack == "fleet" else "detected_count"] > 0 for f in facts])
    handed = np.array([f["people_handed"] > 0 for f in facts])
    moved = int(np.sum([f["costmap_moved"] == 1 for f in facts]))
    since = [min(k for k in range(TICKS + 1) if found[k:, b].all()) for b in range(B)]      # TICKS: not in the last tick
    print(stack, "REPAIRED ticks per robot:", repaired.tolist(), "; robot-ticks with ratio < 1:", slowed, "; tick from which each robot detects:", since,
          "; ticks in which tracks reach people_to_status, per robot:", handed.sum(axis=0).tolist(), "; window moves after the first tick:", moved,
          "; firm scenes of tick", ORACLE_TICK, "against the oracle:", facts[ORACLE_TICK]["firm_scenes"], "; usable solves:",
          int(np.sum([f["usable"] for f in facts])), "of", B * TICKS)
    assert (repaired >= 1).all(), repaired
    assert slowed >= TICKS
    assert max(since) < TICKS, since
    assert handed.any(axis=0).all(), handed
    assert moved >= 1
    assert facts[ORACLE_TICK]["firm_scenes"] >= 1
    assert sum(f["agent_beams"] for f in facts) > 0
    if stack == "fleet":
        others = sum(f["robots_perceived"] for f in facts)
        print(stack, "robot rows among the perceived persons:", others)
        assert others >= 1
    else:
        force = max(f["group_force"] for f in facts)
        hidden, changed = sum(f["out_of_sight"] for f in facts), sum(f["detector_changed"] for f in facts)
        print(stack, "largest velocity change by the group force:", force, "; person-ticks out of sight:", hidden, "; misses and clutter:", changed)
        assert force > 0.0 and hidden >= 1 and changed >= 1                  # the rows in sight are not the persons, the detections not the rows in sight
    assert CC.same_bits(eager["states"][-1]["metrics_acc"], recs[-1].metrics_acc)


@pytest.mark.gpu
def test_graph_replay_equals_the_eager_ticks(eager):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    g, _ = build(eager["stack"])
    declared = BatchEpisode.CORE_STATE + ("plan_start",) + sum((S.STATE for S in g.stages), ())   # the core's state and the present stages'
    assert sorted(declared) == sorted(g.saved_state()) and set(declared) <= set(carried(g)) <= set(declared) | {"person_count"}
    before = state(g, declared)
    g.capture_graph()
    assert_same_state(state(g, declared), before, "after capture_graph: every declared state buffer holds the bytes it held before")
    assert_same_state(state(g, carried(g)), eager["start"], "after capture_graph: the warm-up tick is taken back")
    for _ in range(TICKS):
        g.replay()
    assert_same_state(state(g), eager["states"][-1], f"after {TICKS} replays")


@pytest.mark.gpu
@pytest.mark.parametrize("eager", ["private"], indirect=True)              # ShardedEpisode refuses a shared world
def test_two_shards_equal_the_single_chain(eager):
    from nav2_social_mpc_controller_amd.episode import ShardedEpisode
    prm, world, sc, w_ref, kw, _, _ = stack_kwargs("private")
    two = ShardedEpisode(prm, sc, w_ref, None, None, None, shards=2, graphs=True, **kw)
    assert [p.B for p in two.parts] == [3, 4]
    for _ in range(TICKS):
        two.tick()
    want = eager["states"][-1]
    for name in ("pose", "cmd_vel", "metrics_acc", "plan", "plan_len", "tracks", "track_meta", "track_next_id", "draw_state"):
        assert CC.same_bits(two.gather(name).cpu().numpy(), want[name]), name


@pytest.mark.gpu
def test_recording_and_timing_do_not_change_the_episode(eager):
    bare, _ = build(eager["stack"])
    watched, _ = build(eager["stack"])
    for _ in range(4):
        bare.tick()
        timing = {}
        watched.tick(record=True, timing=timing)
        assert all(v >= 0.0 for v in timing.values()) and {"solve_ms", "plant_ms", "monitor_ms", "repair_ms", "tracker_ms"} <= set(timing)
        assert_launch_order(watched, list(timing))
    assert_same_state(state(watched), state(bare), "recorded and timed against bare")
    assert_same_state(state(bare), eager["states"][3], "bare against the recorded fixture")


def test_the_two_stacks_switch_on_every_keyword():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    on = set()
    for stack in STACKS:
        kw = stack_kwargs(stack)[4]
        assert all(v is not None and v is not False for v in kw.values()), stack
        on |= set(kw)
    declared = set(BatchEpisode.PER_ROBOT + BatchEpisode.FORWARDED)
    assert on <= declared, on - declared
    assert not on & set(NOT_SWITCHED_ON), on & set(NOT_SWITCHED_ON)
    assert declared - on == set(NOT_SWITCHED_ON), (sorted(declared - on - set(NOT_SWITCHED_ON)), sorted(set(NOT_SWITCHED_ON) - declared))
    assert B % 4 == 3                                                       # a ragged last group in the kernels that take four robots a workgroup
