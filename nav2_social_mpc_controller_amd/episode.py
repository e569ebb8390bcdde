"""Closed-loop (receding-horizon) batch episodes: B independent robots, every tick runs the whole
`Optimizer::optimize` chain of the reference on the device,

    field-of-view filter + people_to_status (src/social_mpc_controller.cpp:196-214, src/optimizer.cpp:454-482)
                                                                                   -> smpc_people_to_status_batch
    format_to_optimize + TrajectoryMemory   (src/optimizer.cpp:172-190, 484-551)  -> smpc_format_to_optimize_batch
    ObstacleDistance grid (optional, once)   (src/optimizer.cpp:593-605, 'TODO')   -> smpc_obstacle_distance_batch
    rolling local costmap (optional)         (Nav2's LayeredCostmap::updateMap)    -> smpc_local_costmap_batch
    nearest-agent gather (optional)          (none: the library's own rule)        -> smpc_nearest_people_batch
    sensed local costmap (optional)          (Nav2's ObstacleLayer + InflationLayer;
                                              the library's own memoryless scan)   -> smpc_sensed_costmap_batch
      ... with memory (optional)             (its persistent marking and ray-trace
                                              clearing; the library's own rule)     -> smpc_obstacle_memory_batch
    line-of-sight filter (optional)          (none: the library's own rule)        -> smpc_visible_people_batch
    people detections (optional)             (the deployment's own detector; the
                                              library's own rule)                   -> smpc_detect_people_batch
    people detections from the scan          (the deployment's own leg detector;
      (optional, in place of the two above)   the library's own rule)               -> smpc_scan_people_batch
    people tracks (optional)                 (the deployment's own tracker behind
                                              people_msgs::People; the library's rule) -> smpc_track_people_batch
    global plans (optional, at the start and   (Nav2's planner server; the library's -> smpc_goal_field_batch,
    on replan(), never inside a tick)          own integer cost rule)                 smpc_extract_plan_batch
    project_people                           (src/optimizer.cpp:554-728)           -> smpc_project_people_batch
    problem assembly + ceres::Solve + unpack (src/optimizer.cpp:197-446)           -> smpc_solve_batch
    memory store                             (src/optimizer.cpp:448-449)           -> smpc_memory_store_batch
    collision monitor (optional)             (Nav2's collision_monitor behind the
                                              controller; the library's own rule)   -> smpc_collision_monitor_batch
    robot plant (optional)                   (the deployment's base behind cmd_vel;
                                              the library's own rule)               -> smpc_robot_plant_batch

preceded, when global plans are given, by PathTrajectorizer::trajectorize (src/path_trajectorizer.cpp:120-288 ->
smpc_trajectorize_path_batch) as in SocialMPCController::computeVelocityCommands (src/social_mpc_controller.cpp:176-189),
with all state resident in HBM (torch tensors are only the allocator here). What the reference gets from outside is
stood in for by the simplest thing that has the same shape:
  * without global plans: a constant-curvature arc from the current pose in place of the trajectorizer output;
  * the world: the robot executes the command computeVelocityCommands returns for one period — the first optimised
    command (it lands on the first pose of the optimised path), the trajectorizer's first command when the solve was
    not usable (src/social_mpc_controller.cpp:241-245), 0.1 m/s straight ahead when there is no trajectory (:180-189);
    with BatchEpisode(plant=PlantParams(...)) that command is executed by a model of the base instead
    (smpc_robot_plant_batch): delayed, clamped, limited in its rate of change, and stopped by walls and agents;
    people move with constant velocity, walking through the robot, the walls and off the map, or, with
    BatchEpisode(crowd=CrowdParams(...)), as a reactive crowd: every period smpc_crowd_step_batch moves every robot's
    persons one step of the Social Force Model the controller itself predicts them with (sfm.hpp computeForces /
    updatePosition): each person heads for its current waypoint (scenes.crowd_waypoints), gives way to the other persons
    and to the robot as it was at the start of the period, is pushed back by the nearest obstacle of its cell of the
    ObstacleDistance grid, and takes the next waypoint on arrival. The robot is seen but not pushed.
  * the ground: without a world map every robot keeps the local costmap it was created with, centred on its start pose,
    and can be scored for the few metres that window covers. With BatchEpisode(world=World(...)) the robots drive on one
    world map as the reference controller does on Nav2's rolling local costmap: every tick starts with
    smpc_local_costmap_batch, which moves each robot's window to its pose by whole cells and cuts the windows that moved
    out of the world map into the buffers the solve reads; the ObstacleDistance grid of the projection, the crowd and
    the metrics is the world's, computed once. With BatchEpisode(sensor=SensorParams(...)) the windows hold what a
    laser scan from the robot hits, walls, persons and other robots alike, inflated (smpc_sensed_costmap_batch), as the
    reference's shipped local costmap does, in place of the cut of the pre-inflated world map.
"""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from ._abi import (SmpcFormatBatch, SmpcFormatOut, SmpcMemoryBatch, SmpcPeopleBatch, SmpcProjectionBatch, SmpcSceneBatch,
                   SmpcTrajectorizeOut, SmpcPlanWindowBatch)
from .params import (CrowdGroupParams, CrowdParams, DetectorParams, GlobalPlanParams, MetricsParams, MonitorParams, ObstacleMemoryParams, OptimizerParams, PlanRepairParams, PoolCrowdParams,
                     PlantParams, ScanDetectorParams, SensorParams, TrackerParams, TrajectorizerParams, SharedWorldParams, VisibilityParams, check_scene_param_rows)
from .scenes import SceneBatch, World
from .solver import BatchSolver, point, set_od_grid


@dataclass
class TickRecord:
    """Host copies of one tick's intermediate results (only filled when `record=True`; tests replay them on the CPU)."""
    plan_path: np.ndarray
    plan_cmds: np.ndarray
    speed: np.ndarray
    init_people: np.ndarray
    memory_before: dict
    robot_status: np.ndarray
    pose0: np.ndarray
    init_params: np.ndarray
    path_pts: np.ndarray
    goal_yaw: np.ndarray
    people_proj: np.ndarray
    proj_error: np.ndarray
    result: dict
    memory_after: dict
    robot_pose: np.ndarray = None   # [B,3] pose the tick started from
    traj_n_poses: np.ndarray = None
    window: np.ndarray = None       # [B,L,2] plan window handed to the trajectorizer (plan_window episodes)
    window_len: np.ndarray = None
    plan_start: np.ndarray = None   # [B] pruned start of every plan after this tick's window
    persons: np.ndarray = None      # [B,Np,5] world people (px, py, vx, vy, vz) the tick started from
    person_count: np.ndarray = None
    has_people: np.ndarray = None
    T_scene: np.ndarray = None      # [B] horizon every robot was solved with (plan episodes: from its own path length)
    window_err: np.ndarray = None   # [B] smpc_window_error of the tick's transformGlobalPlan (plan_window episodes)
    # the world after the tick's move: what the tick's metrics sample is taken from (BatchEpisode(metrics=...))
    pose_after: np.ndarray = None     # [B,3]
    persons_after: np.ndarray = None  # [B,Np,5]
    cmd_vel: np.ndarray = None        # [B,2] the executed command
    cmd_source: np.ndarray = None     # [B]
    metrics_acc: np.ndarray = None    # [B,24] the metrics rows with the tick's sample folded in (solver.METRIC_COLS)
    # the persons' waypoint cursors around the tick's crowd step (BatchEpisode(crowd=...))
    cursor_before: np.ndarray = None  # [B,Np]
    cursor_after: np.ndarray = None   # [B,Np]
    # the rolling local costmaps after the tick's roll (BatchEpisode(world=...)): what the tick's solve read
    costmap_cell: np.ndarray = None    # [B,2] world cell of every window's cell (0,0)
    costmap_origin: np.ndarray = None  # [B,2]
    costmap_moved: np.ndarray = None   # [B] smpc_local_costmap_batch's moved
    # the line-of-sight filter's outputs (BatchEpisode(visibility=...)): what the tick's people_to_status read
    person_seen: np.ndarray = None     # [B,Np] uint8 enum smpc_seen_code (flags from person_count[b] on: not written)
    seen_count: np.ndarray = None      # [B]
    seen_persons: np.ndarray = None    # [B,Np,5] (rows from seen_count[b] on: not written)
    # the shared world (BatchEpisode(shared=...)): the table the tick's gather read (`persons`, `person_count` and
    # `person_source` are what it wrote), and with metrics the table the gather in front of the sample read
    agents: np.ndarray = None          # [M+B,5] or [M,5]
    person_source: np.ndarray = None   # [B,Np] rows of `agents` (from person_count[b] on: not written)
    agents_after: np.ndarray = None    # as agents, after the move (persons_after is gathered from it)
    # the reactive pool (BatchEpisode(pool_crowd=...)): what the tick's pool step wrote from `agents`, and the pedestrians'
    # waypoint cursors around it
    pool_next: np.ndarray = None           # [M,5]
    pool_cursor_before: np.ndarray = None  # [M]
    pool_cursor_after: np.ndarray = None   # [M]
    # the sensed local costmaps (BatchEpisode(sensor=...)): what the tick's scan wrote from robot_pose, persons, person_count
    # and costmap_cell, and what the tick's solve read
    sensed_costmap: np.ndarray = None      # [B,size_y,size_x] uint8
    beam_kind: np.ndarray = None           # [B,n_beams] uint8 enum smpc_beam_kind
    beam_cell: np.ndarray = None           # [B,n_beams,2] int32
    # the scan's memory (BatchEpisode(sensor=..., sensor_memory=...)): the mark bitmaps and their window cells the tick's
    # smpc_obstacle_memory_batch read, and the bitmaps it wrote (their window cells are costmap_cell)
    obstacle_memory_before: np.ndarray = None       # [B,size_y,(size_x + 31) // 32] int32 (the bits of the call's uint32 words)
    obstacle_memory_cell_before: np.ndarray = None  # [B,2] int32
    obstacle_memory_after: np.ndarray = None        # as obstacle_memory_before
    # the people tracks (BatchEpisode(tracker=...)): the state the tick's smpc_track_people_batch read (its detections are
    # seen_persons / seen_count with visibility, else persons / person_count) and wrote, and what the tick's
    # people_to_status read
    tracks_before: np.ndarray = None          # [B,slots,4] x, y, vx, vy
    track_meta_before: np.ndarray = None      # [B,slots,4] int32 state, hits, missed, id
    track_next_id_before: np.ndarray = None   # [B] int32
    tracks_after: np.ndarray = None
    track_meta_after: np.ndarray = None
    track_next_id_after: np.ndarray = None
    tracked_persons: np.ndarray = None        # [B,Np,5] (rows from tracked_count[b] on: not written)
    tracked_count: np.ndarray = None          # [B]
    tracked_source: np.ndarray = None         # [B,Np,2] int32 slot, id (rows from tracked_count[b] on: not written)
    # the people detections (BatchEpisode(detector=...)): the state the tick's smpc_detect_people_batch read (its persons are
    # seen_persons / seen_count with visibility, else persons / person_count) and wrote, and what the tracker (or, without
    # one, people_to_status) read
    draw_state_before: np.ndarray = None      # [B,2] uint32 stream id, tick counter
    draw_state_after: np.ndarray = None
    detected_persons: np.ndarray = None       # [B,Nd,5] (rows from detected_count[b] on: not written)
    detected_count: np.ndarray = None         # [B]
    detected_source: np.ndarray = None        # [B,Nd] int32 person j, or -1 - c of clutter candidate c (rows from detected_count[b] on: not written)
    person_outcome: np.ndarray = None         # [B,Np] uint8 smpc_detect_outcome (persons from the count on: not written)
    # the robot plant (BatchEpisode(plant=...)): what the tick's smpc_robot_plant_batch read besides robot_pose, speed (the twist
    # the tick started with) and cmd_vel, and what it wrote besides pose_after
    plant_agents: np.ndarray = None           # [B,Np,5] the true persons as the call saw them (after the tick's crowd step)
    plant_agent_count: np.ndarray = None      # [B]
    plant_queue_before: np.ndarray = None     # [B,8,2] the commands under way
    plant_tick_before: np.ndarray = None      # [B] uint32
    plant_queue_after: np.ndarray = None
    plant_tick_after: np.ndarray = None
    plant_contact: np.ndarray = None          # [B,2] int32 enum smpc_plant_flag bits, substeps advanced
    heading_cs: np.ndarray = None             # [B,2] cosine and sine of the heading the period started with
    speed_after: np.ndarray = None            # [B,2] the executed twist: the next tick's `speed`
    # the collision monitor (BatchEpisode(monitor=...)): what the tick's smpc_collision_monitor_batch wrote, having read robot_pose,
    # cmd_vel, beam_kind and beam_cell; cmd_safe is the command the crowd, the plant or the motion model were handed
    cmd_safe: np.ndarray = None               # [B,2]
    monitor_action: np.ndarray = None         # [B,4] int32 enum smpc_monitor_flag bits, the deciding zone, its collision step, the points
    monitor_points: np.ndarray = None         # [B,Z] int32 points inside each zone at step 0
    monitor_ratio: np.ndarray = None          # [B]
    monitor_heading_cs: np.ndarray = None     # [B,2] cosine and sine of the heading the monitor obtained (rows of robots not finite: not written)
    monitor_step_cs: np.ndarray = None        # [B,2] ... of one simulation step's angle
    # the scan-based people detector (BatchEpisode(scan_detector=...)): what the tick's smpc_scan_people_batch wrote, having read
    # robot_pose, beam_kind and beam_cell; the tracker (or, without one, people_to_status) read the first two
    scan_persons: np.ndarray = None           # [B,Nd,5] x, y, 0, 0, 0; the rows below scan_count
    scan_count: np.ndarray = None             # [B] int32
    scan_segment: np.ndarray = None           # [B,Nd,4] int32 start beam, beams, summed offsets
    scan_stats: np.ndarray = None             # [B,4] int32 segments, rejected by points, rejected by width, accepted
    # the plan repair (BatchEpisode(repair=...)): the plans the tick's smpc_repair_plan_batch was handed and what it made of them,
    # having read robot_pose, the tick's sensed costmap (or `costmap` without a sensor), costmap_origin and plan_start
    repair_plan_before: np.ndarray = None     # [B,L,2]
    repair_plan_len_before: np.ndarray = None  # [B] int32
    repair_plan_after: np.ndarray = None      # [B,L,2]: what the next tick's plan stage reads
    repair_plan_len_after: np.ndarray = None  # [B] int32
    repair_status: np.ndarray = None          # [B] int32 enum smpc_repair_status
    repair_info: np.ndarray = None            # [B,4] int32 i0, i1, j, m; -1 where not determined
    repair_costmap: np.ndarray = None         # the windows the repair read, when no sensing stage recorded them


class BatchEpisode:
    # The keyword arguments of __init__, by what a shard of the robots gets of them (shard_kwargs, ShardedEpisode):
    # one row per robot, sliced along axis 0
    PER_ROBOT = ("plan", "plan_len", "scene_params", "goal", "person_waypoints", "person_n_waypoints", "person_speed",
                 "person_groups")
    # one row per robot exactly when the grids are per scene (od_indexes [B,h,w]), else shared by all shards
    PER_GRID = ("od_indexes", "od_origin", "od_distances")
    # the same object for every shard
    FORWARDED = ("od_resolution", "device", "traj_params", "fov_angle", "order_hint", "plan_window", "obstacles_from_costmap",
                 "obstacle_min_cost", "unknown_is_obstacle", "metrics", "crowd", "crowd_groups", "world", "outside_cost", "planner",
                 "visibility", "shared", "pool", "pool_crowd", "pool_waypoints", "pool_n_waypoints", "pool_speed", "sensor",
                 "sensor_memory", "tracker", "detector", "plant", "monitor", "scan_detector", "repair")

    def __init__(self, params: OptimizerParams, scenes: SceneBatch, w_ref: np.ndarray, od_indexes: np.ndarray = None,
                 od_origin: np.ndarray = None, od_resolution: float = None, device: int = 0, plan: np.ndarray = None,
                 plan_len: np.ndarray = None, traj_params: TrajectorizerParams = None, fov_angle: float = None,
                 order_hint: bool = False, plan_window: tuple = None, obstacles_from_costmap: bool = False,
                 obstacle_min_cost: int = 254, unknown_is_obstacle: bool = False, scene_params: np.ndarray = None,
                 metrics: MetricsParams = None, goal: np.ndarray = None, od_distances: np.ndarray = None,
                 crowd: CrowdParams = None, person_waypoints: np.ndarray = None, person_n_waypoints: np.ndarray = None,
                 person_speed: np.ndarray = None, person_groups: np.ndarray = None,
                 crowd_groups: CrowdGroupParams = None, world: World = None, outside_cost: int = 255,
                 planner: GlobalPlanParams = None, visibility: VisibilityParams = None,
                 shared: SharedWorldParams = None, pool: np.ndarray = None, pool_crowd: PoolCrowdParams = None,
                 pool_waypoints: np.ndarray = None, pool_n_waypoints: np.ndarray = None, pool_speed: np.ndarray = None,
                 sensor: SensorParams = None, sensor_memory: ObstacleMemoryParams = None, tracker: TrackerParams = None,
                 detector: DetectorParams = None, plant: PlantParams = None, monitor: MonitorParams = None,
                 scan_detector: ScanDetectorParams = None, repair: PlanRepairParams = None):
        """scenes: the start state (pose0, people at step 0, costmaps); w_ref [B]: curvature of the arc stand-in;
        od_*: the ObstacleDistance grid of people projection: od_indexes [h,w] + od_origin [2] one grid shared by all
        scenes, od_indexes [B,h,w] + od_origin [B,2] one per scene. obstacles_from_costmap: od_* are not needed; the grids
        are computed on the device from the scenes' costmaps once, here (smpc_obstacle_distance_batch with
        obstacle_min_cost / unknown_is_obstacle; without `world` an episode's costmaps are fixed): one per scene, or one for a
        shared costmap, with the costmap's origin and resolution; with `world` the one grid of the world map.
        plan [B,L,2] + plan_len [B] + traj_params: global plans,
        trajectorized on the device every tick (the plan must stay longer than the horizon for the whole episode).
        fov_angle: field-of-view half angle of the people filter (reference default pi/4); None = no filter.
        plan_window: (max_robot_pose_search_dist, dist_threshold): every tick starts with PathHandler::transformGlobalPlan
        (smpc_transform_global_plan_batch; plan frame = costmap frame) and trajectorizes the window instead of the whole
        plan, as computeVelocityCommands does (src/social_mpc_controller.cpp:171-180; the reference passes 4.0 m and half
        the costmap's larger side); the plans are pruned as the robots
        advance. None: the global plans go to the trajectorizer as they are.
        order_hint: hand the solve kernel's queue the scenes sorted by the previous tick's sweep counts, longest first
        (smpc_scene_batch.order; the results are the same, the lone launch is shorter).
        scene_params [B,14]: critic weights, target speed and velocity bounds of every robot (smpc_scene_batch.scene_params,
        e.g. params.scene_param_rows), handed to every tick's solve; None: `params`' values for every robot. Only the
        solve takes them: the trajectorizer and the rest of the tick keep the episode-wide parameters.
        metrics: score every robot on the device (smpc_episode_metrics_batch): each tick ends with one sample of the world
        after its move — the new pose, the executed command, the moved persons, the tick's solve status and command source —
        folded into self.metrics_acc [B,24] (solver.METRIC_COLS; metrics() returns the host copy, solver.summarize_metrics
        the derived values). goal [B,2]: where each robot is headed (default with global plans: the last pose of each plan;
        otherwise none, and the goal columns stay unset); a robot's row is frozen once it is within metrics.goal_tolerance
        of it. The clearance columns need the distances of the ObstacleDistance grid: with obstacles_from_costmap they are
        computed along with the indexes, with host-given od_indexes they are fed only when od_distances (float32, shaped
        like od_indexes) is passed too. None: nothing is allocated and nothing is launched.
        crowd: the persons move as a reactive crowd (smpc_crowd_step_batch, one launch per tick, in place of the
        constant-velocity move): person_waypoints [B,Np,K,2] and person_n_waypoints [B,Np] (e.g. scenes.crowd_waypoints) are
        each person's goals, self.person_cursor [B,Np] the index of its current one (0 at the start); person_speed [B,Np]:
        desired speeds (default crowd.desired_speed for everybody). The step sees the pose the period started from and the
        command being executed, and the episode's ObstacleDistance grid. None: nothing is allocated and the persons move
        with constant velocity.
        person_groups [B,Np] int32 (with crowd; e.g. scenes.crowd_groups): the persons' group ids (< 0: none); companions
        are held together by the Social Force Model's group force (smpc_crowd_step_groups_batch) with the factors of
        crowd_groups (default CrowdGroupParams()). Uploaded once and constant over the episode. None: nothing is
        allocated and the plain crowd step runs.
        world: the map the robots drive on (scenes.World, e.g. scenes.make_world with scenes.scenes_in_world): the scenes'
        costmaps (one per robot, of the world's resolution) become rolling windows of it. The world is uploaded once and
        self.costmap_cell [B,2] holds the world cell of every window's cell (0,0); every tick starts, before the plan window
        and the trajectorizer, with smpc_local_costmap_batch at the robots' current poses, which rewrites the windows (and
        costmap_origin) of the robots whose window moved and leaves the others alone; window cells beyond the world read
        outside_cost. The first tick, and the first replay of a captured graph, write every window (`force`). With
        obstacles_from_costmap the ObstacleDistance grid is computed from the world map, once, shared by all robots, with
        the world's origin (with distances when metrics ask for them); host-given od_* are taken as they are. None:
        nothing is allocated and nothing is launched.
        planner: the global plans come from the world map (include/smpc_global_plan.h) instead of `plan`, which is refused:
        needs `world`, `traj_params` and goal [B,2]. One goal field per distinct row of `goal` (found on the host;
        self.robot_goal [B] maps the robots onto them) is computed here, once (smpc_goal_field_batch), and every robot's
        plan is walked down its field from its start pose (smpc_extract_plan_batch) into self.plan [B,planner.max_poses,2],
        self.plan_len and self.plan_error [B] (enum smpc_plan_error; a robot with an error other than TRUNCATED has
        plan_len 0 and gets no command). From there on this is the episode that was handed these arrays as `plan`.
        replan() walks again from the current poses. None: nothing is allocated and nothing is launched.
        visibility: the robots perceive only the persons they have in line of sight on the world map
        (include/smpc_visibility.h): needs `world`. Every tick, after the roll and the plan stage and directly before
        people_to_status, smpc_visible_people_batch compacts the persons within visibility.max_range whose sight line no
        cell of the world occludes into self.seen_persons [B,Np,5] / self.seen_count [B] (with self.person_seen [B,Np]
        uint8, enum smpc_seen_code), and people_to_status reads those in place of self.persons / self.person_count. The
        crowd step, the metrics and the world's move keep the true persons. None: nothing is allocated and nothing is
        launched.
        shared: one world for all robots (include/smpc_nearest.h): needs `world`; `crowd` and the person_* arguments are
        refused (they move private rows). The scenes' own people are not uploaded. self.agents [M+B,5] is one table of
        people_msgs::Person rows: the M rows of pool [M,5] (e.g. scenes.shared_pool; None: no pedestrians) followed, with
        shared.robots_as_people, by one row per robot (x, y, v cos yaw, v sin yaw, w), which self.agent_self [B] = M + b
        keeps a robot from perceiving as somebody else (without robots_as_people the table is the pool alone and
        agent_self is -1). Every tick, after the roll and the plan stage and before the line-of-sight filter, the robots'
        rows are refreshed from self.pose and self.speed and smpc_nearest_people_batch writes each robot's at most
        Np = shared.max_people (default: the scenes' N) nearest agents within shared.max_range, nearest first, into
        self.persons [B,Np,5] / self.person_count [B] (self.person_source [B,Np]: their rows of the table), the addresses
        everything behind it reads. The pool moves with constant velocity, in place; the caller may rewrite
        self.agents[:M] between ticks. With `metrics` the rows are refreshed and gathered a second time after the move, so
        that the sample sees the world as the period leaves it, the other robots at their new poses included. None (then
        pool must be None too): nothing is allocated and nothing is launched.
        pool_crowd: the pool moves as a reactive crowd (include/smpc_crowd_pool.h; needs shared and pool): every period one
        smpc_crowd_pool_step_batch on the bins the tick's gather built (which are then sized for the larger of
        shared.max_range and pool_crowd.interaction_range) takes the constant-velocity move's place: every pedestrian heads
        for its current waypoint of pool_waypoints [M,K,2] / pool_n_waypoints [M] (e.g. scenes.pool_waypoints) and gives way
        to the other pedestrians and, with shared.robots_as_people, to the robots, which it sees at the pose and speed the
        period started from. pool_speed [M]: desired speeds (default pool_crowd.desired_speed for everybody). None (the
        other three must be None too): nothing is allocated, nothing is launched and the pool walks straight on.
        sensor: the robots' windows are sensed (include/smpc_sensed_costmap.h): needs `world`. Every tick, after the roll, the
        plan stage and the shared world's gather and before the line-of-sight filter, one smpc_sensed_costmap_batch casts
        sensor.n_beams beams from self.pose over the world map and the true self.persons / self.person_count (with `shared`
        the other robots among them), marks the cells they stop at in the windows at self.costmap_cell, inflates the marks
        and rewrites self.costmap, which the solve reads; self.beam_kind [B,n_beams] (enum smpc_beam_kind) and
        self.beam_cell [B,n_beams,2] hold each beam's outcome. sensor.base "world" keeps the world cut underneath. The
        ObstacleDistance grid stays the world's. None: nothing is allocated and nothing is launched.
        sensor_memory: the scan has a memory (include/smpc_obstacle_memory.h): needs `sensor`. One
        smpc_obstacle_memory_batch takes the place of the tick's smpc_sensed_costmap_batch: the beams reach out to
        sensor_memory.raytrace_range and clear the cells they pass, hits are marked within sensor.max_range, the cells
        under the robot are cleared, and a mark stays until a beam passes it. The state is self.obstacle_memory
        [B,size_y,(size_x + 31) // 32] int32 (one bit per window cell, zero at the start) and self.obstacle_memory_cell
        [B,2]. None: nothing is allocated, nothing new is launched and the episode is the sensed one bit for bit.
        tracker: the controller is handed tracks instead of the simulator's rows (include/smpc_tracker.h). Every tick,
        directly in front of people_to_status, one smpc_track_people_batch associates the tick's detections (with
        `visibility` self.seen_persons / self.seen_count, else self.persons / self.person_count; only x and y are read) with
        the robot's tracks, estimates their velocity from positions alone with dt = params.dt, coasts a track whose person
        is not detected for at most tracker.max_missed ticks, and writes the confirmed tracks nearest first into
        self.tracked_persons [B,Np,5] / self.tracked_count [B] (self.tracked_source [B,Np,2]: slot and id), which
        people_to_status reads. The state is self.tracks [B,slots,4], self.track_meta [B,slots,4] int32 and
        self.track_next_id [B] int32, zero at the start. The world model, the crowd steps, the scan and the metrics keep
        reading the true self.persons. None: nothing is allocated, nothing is launched and the episode is the one without
        bit for bit.
        detector: the controller is handed what a detector would report (include/smpc_detector.h). Every tick, behind the
        line-of-sight filter and in front of the tracker, one smpc_detect_people_batch reads self.seen_persons /
        self.seen_count with `visibility`, else self.persons / self.person_count: persons behind another person's body
        and missed persons leave, the others are reported with range-dependent position noise, clutter is appended, into
        self.detected_persons [B,Nd,5] / self.detected_count [B] (self.detected_source [B,Nd], self.person_outcome [B,Np]
        uint8), Nd = min(64, Np + detector.clutter_candidates), which the tracker (or, without one, people_to_status)
        reads. The state is self.draw_state [B,2] int32 (the bits of the call's uint32 words): the robot's stream id
        (its index; set_detector_streams() gives a part of a larger batch the ids of its robots there, as ShardedEpisode
        does) and its tick counter, zero at the start, which lives on the device so that a replayed graph draws fresh
        numbers every tick. The world model, the crowd steps, the scan and the metrics keep reading the true self.persons.
        None: nothing is allocated, nothing is launched and the episode is the one without bit for bit.
        plant: the command is executed by a model of the base (include/smpc_plant.h) instead of being taken for the motion.
        Every tick, after the command selection and the crowd steps, one smpc_robot_plant_batch takes the place of the torch
        move of pose and speed: the command selected plant.latency_ticks periods ago is clamped to params' velocity bounds,
        limited by plant.max_accel / max_decel / max_ang_accel, and integrated with the motion model (x, y with the old
        heading, then the heading) in plant.substeps steps that end in front of a wall cell of the world map (with `world`;
        else there are no walls) or an agent of the true self.persons / self.person_count (with `shared` the other robots
        among them). Every robot is moved by the motion model, whether its solve was usable or not. self.speed becomes the
        executed twist, which the next warm start and the metrics read. The state is self.plant_queue [B,8,2],
        self.plant_tick [B] int32 (the bits of the call's uint32 words), zero at the start; self.plant_contact [B,2] int32
        holds each robot's flags (enum smpc_plant_flag) and substeps, self.heading_cs [B,2] the heading's cosine and sine.
        None: nothing is allocated, nothing is launched and the episode is the one without bit for bit.
        monitor: the selected command passes a collision monitor (include/smpc_collision_monitor.h) before anything executes
        it; needs `sensor`, with or without `sensor_memory`: the monitor reads the tick's scan. Directly behind the command
        selection one smpc_collision_monitor_batch judges self.cmd_vel at self.pose against the cells the tick's beams
        stopped at (self.beam_kind / self.beam_cell) and writes self.cmd_safe [B,2], self.monitor_action [B,4] int32
        (enum smpc_monitor_flag bits, the deciding zone or -1, its collision step or -1, the robot's points),
        self.monitor_points [B,Z] int32 and self.monitor_ratio [B]. Everything behind it that took self.cmd_vel for the
        command being executed takes self.cmd_safe: the crowd steps, the plant, and without a plant the motion model, the next
        warm start's speed and the metrics' twist; self.cmd_vel stays the controller's command. Without a plant a robot whose
        command the monitor changed (ratio < 1) is moved by the motion model with the safe command instead of being placed
        on the first optimised pose.
        None: nothing is allocated, nothing is launched and the episode is the one without bit for bit.
        scan_detector: the controller is handed what its own scan shows of the people (include/smpc_scan_people.h); needs
        `sensor`, with or without `sensor_memory`, and excludes `visibility` and `detector`: those start from the simulator's
        person rows, this starts from the beams, and the two paths are alternatives. Every tick, right behind the sensed (or
        memory) call and in front of the tracker, one smpc_scan_people_batch clusters the cells the tick's beams stopped at
        (self.beam_kind / self.beam_cell) into segments and writes the person-sized ones into self.scan_persons [B,Nd,5]
        (x, y, 0, 0, 0) and self.scan_count [B] int32, Nd = scan_detector.max_detections, with self.scan_segment [B,Nd,4] int32
        (start beam, beams, the summed offsets) and self.scan_stats [B,4] int32 (segments, rejected by points, rejected by
        width, accepted). The tracker reads them, or without one people_to_status does; a detection has no velocity, so
        without a tracker the solve plans around people who stand still: use tracker=TrackerParams(). The crowd, the plant,
        the metrics and the scan itself keep seeing the true persons.
        None: nothing is allocated, nothing is launched and the episode is the one without bit for bit.
        repair: the plans give way to what the windows show (include/smpc_plan_repair.h); needs `plan` or `planner`. Every
        tick, right behind the sensing stage (the sensed or memory call; without a sensor, the plan stage), one
        smpc_repair_plan_batch reads self.pose, self.costmap, self.costmap_origin and, with a plan window, self.plan_start: a
        robot whose plan runs into impassable cells of its window within repair.radius gets the least-cost detour inside that
        region spliced into self.plan / self.plan_len in place (self.plan_scratch [B,L,2] is the call's workspace), and
        self.repair_status [B] int32 (enum smpc_repair_status) and self.repair_info [B,4] int32 (i0, i1, j, m) say what
        happened. The tick's own roll and trajectorizer ran before the scan, so a repaired plan takes effect at the next
        tick's plan stage. The call is part of a captured graph. replan() replaces repaired plans like any other.
        None: nothing is allocated, nothing is launched and the episode is the one without bit for bit."""
        import torch

        self.torch = torch
        self.params = params
        self.solver = BatchSolver(params, device)
        self.dev = f"cuda:{device}"
        # library kernels and the few torch ops of the world model share one stream, so they are ordered
        self.solver.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
        self.B, self.T, self.N = scenes.B, scenes.T, scenes.N
        if planner is not None:
            if plan is not None or plan_len is not None:
                raise ValueError("planner computes the global plans: plan / plan_len cannot be given as well")
            if world is None or traj_params is None or goal is None:
                raise ValueError("planner needs world, traj_params and goal [B,2]")
        if visibility is not None and world is None:
            raise ValueError("visibility needs world: the sight lines run over the world map")
        if sensor is not None and world is None:
            raise ValueError("sensor needs world: the scan runs over the world map")
        if sensor_memory is not None and sensor is None:
            raise ValueError("sensor_memory needs sensor=SensorParams(...): it is the scan's memory")
        if shared is None and pool is not None:
            raise ValueError("pool needs shared=SharedWorldParams(...)")
        if pool_crowd is None:
            given = sorted(k for k, v in dict(pool_waypoints=pool_waypoints, pool_n_waypoints=pool_n_waypoints,
                                              pool_speed=pool_speed).items() if v is not None)
            if given:
                raise ValueError(f"{', '.join(given)} need pool_crowd=PoolCrowdParams(...)")
        elif shared is None or pool is None:
            raise ValueError("pool_crowd needs shared=SharedWorldParams(...) and pool [M,5]")
        elif pool_waypoints is None or pool_n_waypoints is None:
            raise ValueError("pool_crowd needs pool_waypoints [M,K,2] and pool_n_waypoints [M]")
        if shared is not None:
            if world is None:
                raise ValueError("shared needs world: the robots and the pool share its floor")
            private = dict(crowd=crowd, person_waypoints=person_waypoints, person_n_waypoints=person_n_waypoints,
                           person_speed=person_speed, person_groups=person_groups)
            given = sorted(k for k, v in private.items() if v is not None)
            if given:
                raise ValueError(f"shared refuses {', '.join(given)}: the reactive crowd step moves private rows")
        if plan is not None or planner is not None:
            # Plan mode: every robot is solved with the horizon its own trajectorized path gives it (smpc_format_batch.n_poses
            # -> T_scene). The arrays are sized for the longest one: a path of exactly max_poses = round(max_time / dt)
            # poses is not cut by format_to_optimize (src/optimizer.cpp:491-497) and so has one step more than the longer,
            # cut, paths: T = max_poses - 1 = rollout_steps + 1.
            assert self.T == params.rollout_steps
            self.T += 1
        self.P = params.dims(self.T, True)[3]
        self._init_world(scenes, w_ref, fov_angle, shared)
        self._init_rolling(world, outside_cost)
        self._init_grid(od_indexes, od_origin, od_resolution, od_distances, obstacles_from_costmap, obstacle_min_cost,
                        unknown_is_obstacle, distances=metrics is not None)
        self._init_memory()
        self._init_plan(plan, plan_len, traj_params, plan_window, planner, goal)
        self._init_solve(order_hint, scene_params)
        self._init_metrics(metrics, goal, plan, plan_len)
        self._init_crowd(crowd, person_waypoints, person_n_waypoints, person_speed, person_groups, crowd_groups)
        self._init_visibility(visibility)
        self._init_shared(shared, pool, pool_crowd, pool_waypoints, pool_n_waypoints, pool_speed)
        self._init_sensor(sensor, sensor_memory)
        self._init_tracker(tracker)
        self._init_detector(detector)
        self._init_plant(plant)
        self._init_monitor(monitor)
        self._init_scan_detector(scan_detector)
        self._init_repair(repair)
        self._bind()
        self.graph = None
        self.gstream = None
        self.ticks = 0
        if planner is not None:
            self.replan()

    # -- construction, by concern: device buffers first, then (_bind) the structs that point into them -----------------
    def _upload(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.dev)

    def _zeros(self, *shape, dtype=None):
        return self.torch.zeros(shape, dtype=dtype or self.torch.float64, device=self.dev)

    def _init_world(self, scenes, w_ref, fov_angle, shared=None):
        """The robots, the persons and the costmaps."""
        i32 = self.torch.int32
        self.pose = self._upload(scenes.pose0.copy(), np.float64)                 # [B,3] current robot pose
        self.speed = self._upload(scenes.init_params[:, 0:2].copy(), np.float64)  # [B,2] current twist
        self.w_ref = self._upload(w_ref, np.float64)
        self.cmd_vel = self._zeros(self.B, 2)            # the command returned to the robot this tick
        self.cmd_source = self._zeros(self.B, dtype=i32)  # 0 optimised, 1 trajectorizer, 2 creep, 3 none
        # world people as people_msgs::Person rows [B,Np,5]: position x, y, velocity x, y, z (scene people at step 0;
        # make_scenes keeps the invalid ones at the end, so the first `count` rows are the persons)
        st0 = scenes.people[:, 0].transpose(0, 2, 1)                                    # [B,N,6] x, y, yaw, t, lv, av
        persons = np.stack([st0[:, :, 0], st0[:, :, 1], st0[:, :, 4] * np.cos(st0[:, :, 2]), st0[:, :, 4] * np.sin(st0[:, :, 2]),
                            st0[:, :, 5]], axis=-1)
        count = np.where(scenes.has_people != 0, (st0[:, :, 3] != -1.0).sum(axis=1), 0)
        if shared is not None:  # the gather writes them every tick; the scenes' own people stay on the host
            Np = int(shared.max_people) if shared.max_people is not None else self.N
            if not 1 <= Np <= 64:
                raise ValueError(f"shared needs 1 <= max_people <= 64 rows per robot, got {Np}")
            self.persons = self._zeros(self.B, Np, 5)
            self.person_count = self._zeros(self.B, dtype=i32)
        else:
            self.persons = self._upload(persons, np.float64)
            self.person_count = self._upload(count, np.int32)
        self.fov_angle = fov_angle
        self.people = self._zeros(self.B, self.N, 6)                                    # people_to_status output
        self.has_people = self._zeros(self.B, dtype=self.torch.uint8)
        self.costmap = self.torch.from_numpy(scenes.costmap).to(self.dev)
        self.costmap_origin = self.torch.from_numpy(scenes.costmap_origin).to(self.dev)
        self.costmap_shared = scenes.costmap_shared
        self.size_x, self.size_y, self.resolution = scenes.size_x, scenes.size_y, scenes.resolution

    def _init_rolling(self, world, outside_cost):
        """The world map the costmaps are rolling windows of, and where every window is."""
        self.world = world
        if world is None:
            return
        if self.costmap_shared:
            raise ValueError("world needs a costmap per robot (costmap_shared = False, e.g. scenes.scenes_in_world)")
        if float(world.resolution) != float(self.resolution):
            raise ValueError("the world and the scenes' costmaps differ in resolution")
        self.world_map = self._upload(world.map, np.uint8)                              # [Hy,Hx]
        self.world_origin = self._upload(np.asarray(world.origin, np.float64).reshape(1, 2), np.float64)
        self.outside_cost = int(outside_cost)
        self.costmap_cell = self._zeros(self.B, 2, dtype=self.torch.int32)
        self.costmap_moved = self._zeros(self.B, dtype=self.torch.int32)
        self._force_roll = True  # the next roll writes every window: the first tick, the first replay of a graph

    def _init_grid(self, od_indexes, od_origin, od_resolution, od_distances, from_costmap, obstacle_min_cost,
                   unknown_is_obstacle, distances):
        """The ObstacleDistance grid(s): od_indexes, od_origin, od_shared, od_h, od_w, od_resolution and, when the metrics
        read them (`distances`) and they are there, od_distances (else the attribute does not exist)."""
        torch, B = self.torch, self.B
        if from_costmap:
            # of the world map when the costmaps are rolling windows of it, else of the (fixed) costmaps themselves
            rolling = self.world is not None
            costmap, shared = (self.world_map, True) if rolling else (self.costmap, self.costmap_shared)
            size_y, size_x = int(costmap.shape[-2]), int(costmap.shape[-1])
            shape = (1 if shared else B, size_y, size_x)
            self.od_shared = 1 if shared else 0
            self.od_resolution = float(np.float32(self.resolution))
            self.od_origin = self.world_origin if rolling else self.costmap_origin
            self.od_indexes = torch.empty(shape, dtype=torch.int32, device=self.dev)
            if distances:  # the clearance columns read the distances: one more array, once
                self.od_distances = torch.empty(shape, dtype=torch.float32, device=self.dev)
            ob = BatchSolver.obstacle_distance_c(B, size_x, size_y, shared, self.resolution, 1, obstacle_min_cost, unknown_is_obstacle)
            ob.costmap = costmap.data_ptr()
            self.solver.obstacle_distance_device(ob, self.od_indexes.data_ptr(), self.od_distances.data_ptr() if distances else 0)
        else:
            if od_indexes is None or od_origin is None or od_resolution is None:
                raise ValueError("od_indexes, od_origin and od_resolution are needed unless obstacles_from_costmap=True")
            od_indexes = np.asarray(od_indexes)
            per_scene = od_indexes.ndim == 3 and od_indexes.shape[0] > 1
            if per_scene:
                assert od_indexes.shape[0] == B and np.shape(od_origin) == (B, 2), "per-scene grids: od_indexes [B,h,w], od_origin [B,2]"
            self.od_shared = 0 if per_scene else 1
            self.od_indexes = self._upload(np.ascontiguousarray(od_indexes, np.uint32).view(np.int32), np.int32)
            self.od_origin = self._upload(np.asarray(od_origin, np.float64).reshape(-1 if per_scene else 1, 2), np.float64)
            self.od_resolution = float(od_resolution)
            if distances and od_distances is not None:
                assert np.shape(od_distances) == od_indexes.shape, "od_distances is shaped like od_indexes"
                self.od_distances = self._upload(od_distances, np.float32)
        self.od_h, self.od_w = int(self.od_indexes.shape[-2]), int(self.od_indexes.shape[-1])

    def _init_memory(self):
        """TrajectoryMemory, one record per scene."""
        B, T, i32 = self.B, self.T, self.torch.int32
        self.mem_path = self._zeros(B, T + 1, 3)
        self.mem_cmds = self._zeros(B, T + 1, 2)
        self.mem_valid = self._zeros(B, dtype=i32)
        self.mem_length = self._zeros(B, 2, dtype=i32)                              # poses / commands of every record
        self.T_scene = self.torch.full((B,), T, dtype=i32, device=self.dev)         # horizon of every robot this tick
        self.max_poses = int(np.round(np.float32(self.params.max_time) / np.float32(self.params.time_step)))

    def _init_planner(self, planner, goal):
        """The goal fields of the robots' distinct goals, computed once, and the buffers every (re)plan is walked into."""
        B, i32 = self.B, self.torch.int32
        goal = np.ascontiguousarray(goal, np.float64)
        assert goal.shape == (B, 2), "goal [B,2]"
        goals, robot_goal = np.unique(goal, axis=0, return_inverse=True)
        G = goals.shape[0]
        self.plan_goals = self._upload(goals, np.float64)                              # [G,2]
        self.robot_goal = self._upload(np.asarray(robot_goal).reshape(B), np.int32)    # [B]
        self.goal_field = self.torch.empty((G, self.world.cells_y, self.world.cells_x), dtype=i32, device=self.dev)  # uint32 bits
        self.goal_status = self._zeros(G, dtype=i32)
        gf = point(BatchSolver.goal_field_c(planner, G, self.world.cells_x, self.world.cells_y, True, self.resolution, 1),
                   {"world": self.world_map, "world_origin": self.world_origin, "goal": self.plan_goals})
        self.solver.goal_field_device(gf, self.goal_field.data_ptr(), self.goal_status.data_ptr())
        self.plan_error = self._zeros(B, dtype=i32)
        return self._zeros(B, planner.max_poses, 2), self._zeros(B, dtype=i32)

    def _init_plan(self, plan, plan_len, traj_params, plan_window, planner=None, goal=None):
        """The global plans with the trajectorizer's (and the plan window's) outputs, or the rows of the arc stand-in."""
        B, i32 = self.B, self.torch.int32
        self.traj = traj_params
        self.planner = planner
        self.plan, self.plan_window, self.rows = None, None, self.T + 1
        if plan is not None or planner is not None:
            assert traj_params is not None and traj_params.max_steps + 1 >= self.T + 1
            if planner is not None:
                self.plan, self.plan_len = self._init_planner(planner, goal)
            else:
                self.plan = self._upload(plan, np.float64)
                self.plan_len = self._upload(plan_len, np.int32)
            self.rows = traj_params.max_steps + 1
            self.traj_n = self._zeros(B, dtype=i32)
            self.traj_err = self._zeros(B, dtype=i32)
            self.traj_vy = self._zeros(B, self.rows)
            self.plan_window = plan_window
            if plan_window is not None:
                self.plan_start = self._zeros(B, dtype=i32)
                self.window = self.torch.zeros_like(self.plan)
                self.window_len = self._zeros(B, dtype=i32)
                self.window_err = self._zeros(B, dtype=i32)
        self.plan_path = self._zeros(B, self.rows, 3)
        self.plan_cmds = self._zeros(B, self.rows, 2)

    def _init_solve(self, order_hint, scene_params):
        """What format_to_optimize, project_people and the solve write every tick."""
        B, T = self.B, self.T
        self.robot_status = self._zeros(B, T + 1, 6)
        self.pose0 = self._zeros(B, 3)
        self.init_params = self._zeros(B, self.P)
        self.path_pts = self._zeros(B, T + 1, 2)
        self.goal_yaw = self._zeros(B)
        self.people_proj = self._zeros(B, T + 1, 6, self.N)
        self.proj_error = self._zeros(B, dtype=self.torch.int32)
        self.rb, self.res = self.solver.alloc_results(B, T, self.dev)
        self.order_hint = order_hint
        # queue order for the next solve (from the last solve's sweep counts; index order before the first one)
        self.order = self.torch.arange(B, dtype=self.torch.int32, device=self.dev)
        self.scene_params = None
        if scene_params is not None:  # device rows: checked here, not by the library
            self.scene_params = self.torch.from_numpy(check_scene_param_rows(scene_params, B)).to(self.dev)

    def _init_metrics(self, metrics, goal, plan, plan_len):
        self.metrics_params = metrics
        if metrics is None:
            return
        B = self.B
        self.metrics_acc = self._zeros(B, 24)  # zero rows: no samples yet
        if goal is None and plan is not None:
            L = np.asarray(plan_len).astype(np.int64)
            goal = np.asarray(plan, np.float64)[np.arange(B), np.maximum(L, 1) - 1]
        self.goal = None
        if goal is not None:
            assert np.shape(goal) == (B, 2), "goal [B,2]"
            self.goal = self._upload(goal, np.float64)

    def _init_crowd(self, crowd, person_waypoints, person_n_waypoints, person_speed, person_groups, crowd_groups):
        B, Np = self.B, int(self.persons.shape[1])
        self.crowd_params = crowd
        self.person_groups = None
        if person_groups is not None and crowd is None:
            raise ValueError("person_groups needs crowd=CrowdParams(...)")
        if crowd is None:
            return
        if person_waypoints is None or person_n_waypoints is None:
            raise ValueError("crowd needs person_waypoints [B,Np,K,2] and person_n_waypoints [B,Np]")
        wp = np.ascontiguousarray(person_waypoints, np.float64)
        assert wp.ndim == 4 and wp.shape[:2] == (B, Np) and wp.shape[3] == 2, "person_waypoints [B,Np,K,2]"
        assert np.shape(person_n_waypoints) == (B, Np), "person_n_waypoints [B,Np]"
        self.person_wp = self._upload(wp, np.float64)
        self.person_nwp = self._upload(person_n_waypoints, np.int32)
        self.person_cursor = self._zeros(B, Np, dtype=self.torch.int32)
        self.person_speed = None
        if person_speed is not None:
            assert np.shape(person_speed) == (B, Np), "person_speed [B,Np]"
            self.person_speed = self._upload(person_speed, np.float64)
        if person_groups is not None:
            assert np.shape(person_groups) == (B, Np), "person_groups [B,Np]"
            self.person_groups = self._upload(person_groups, np.int32)
            self.crowd_group_params = crowd_groups if crowd_groups is not None else CrowdGroupParams()

    def _init_visibility(self, visibility):
        """What the line-of-sight filter writes every tick: fixed addresses, people_to_status reads the first two."""
        self.visibility = visibility
        if visibility is None:
            return
        if not visibility.supported(self.resolution):
            raise ValueError("visibility.max_range / resolution exceeds 32768 cells")
        B, Np = self.B, int(self.persons.shape[1])
        self.seen_persons = self._zeros(B, Np, 5)
        self.seen_count = self._zeros(B, dtype=self.torch.int32)
        self.person_seen = self._zeros(B, Np, dtype=self.torch.uint8)

    def _init_tracker(self, tracker):
        """The tracks of every robot (zero: no tracks) and what the tracker writes every tick: fixed addresses,
        people_to_status reads the first two."""
        self.tracker = tracker
        if tracker is None:
            return
        if not isinstance(tracker, TrackerParams):
            raise ValueError("tracker must be a TrackerParams")
        if not tracker.supported(self.params.dt):
            raise ValueError("tracker: more than 64 slots, or no finite beta / dt with params.dt")
        B, Np, Nt = self.B, int(self.persons.shape[1]), int(tracker.slots)
        self.tracks = self._zeros(B, Nt, 4)
        self.track_meta = self._zeros(B, Nt, 4, dtype=self.torch.int32)
        self.track_next_id = self._zeros(B, dtype=self.torch.int32)
        self.tracked_persons = self._zeros(B, Np, 5)
        self.tracked_count = self._zeros(B, dtype=self.torch.int32)
        self.tracked_source = self._zeros(B, Np, 2, dtype=self.torch.int32)

    def _init_detector(self, detector):
        """The draw state of every robot (stream id = its index, counter 0) and what the detector writes every tick: fixed
        addresses, the tracker or people_to_status reads the first two."""
        self.detector = detector
        if detector is None:
            return
        if not isinstance(detector, DetectorParams):
            raise ValueError("detector must be a DetectorParams")
        if not detector.supported():
            raise ValueError("detector: more than 64 clutter candidates")
        B, Np = self.B, int(self.persons.shape[1])
        Nd = min(64, Np + int(detector.clutter_candidates))
        self.draw_state = self._zeros(B, 2, dtype=self.torch.int32)
        self.draw_state[:, 0] = self.torch.arange(B, dtype=self.torch.int32, device=self.draw_state.device)
        self.detected_persons = self._zeros(B, Nd, 5)
        self.detected_count = self._zeros(B, dtype=self.torch.int32)
        self.detected_source = self._zeros(B, Nd, dtype=self.torch.int32)
        self.person_outcome = self._zeros(B, Np, dtype=self.torch.uint8)

    @staticmethod
    def check_scan_detector(scan_detector, sensor, visibility, detector, resolution: float):
        """What BatchEpisode(scan_detector=...) refuses (sensor, visibility, detector: the episode's; resolution: the world's)."""
        if not isinstance(scan_detector, ScanDetectorParams):
            raise ValueError("scan_detector must be a ScanDetectorParams")
        if sensor is None:
            raise ValueError("scan_detector needs sensor=SensorParams(...): it reads the scan")
        if visibility is not None:
            raise ValueError("scan_detector and visibility are alternatives: the scan-based or the ground-truth path")
        if detector is not None:
            raise ValueError("scan_detector and detector are alternatives: the scan-based or the ground-truth path")
        if not scan_detector.supported(resolution, sensor):
            raise ValueError("scan_detector: more than 64 detections, or a squared cell distance beyond int32 at the world's resolution")

    def _init_scan_detector(self, scan_detector):
        """What the scan-based detector writes every tick: fixed addresses, the tracker or people_to_status reads the first
        two. It has no state."""
        self.scan_detector = scan_detector
        if scan_detector is None:
            return
        self.check_scan_detector(scan_detector, self.sensor, self.visibility, self.detector, self.resolution)
        B, Nd = self.B, int(scan_detector.max_detections)
        self.scan_persons = self._zeros(B, Nd, 5)
        self.scan_count = self._zeros(B, dtype=self.torch.int32)
        self.scan_segment = self._zeros(B, Nd, 4, dtype=self.torch.int32)
        self.scan_stats = self._zeros(B, 4, dtype=self.torch.int32)

    @staticmethod
    def check_repair(repair, planned: bool, resolution: float):
        """What BatchEpisode(repair=...) refuses (planned: the episode has plan= or planner=; resolution: the windows')."""
        if not isinstance(repair, PlanRepairParams):
            raise ValueError("repair must be a PlanRepairParams")
        if not planned:
            raise ValueError("repair needs plan= or planner=: there is no plan to repair")
        if not repair.supported(resolution):
            raise ValueError("repair: a radius beyond 63 cells at the windows' resolution, or costs whose potentials do not fit 32 bits")

    def _init_repair(self, repair):
        """The plan repair's workspace and what it reports."""
        self.repair = repair
        if repair is None:
            return
        self.check_repair(repair, self.plan is not None, self.resolution)
        self.plan_scratch = self.torch.zeros_like(self.plan)
        self.repair_status = self._zeros(self.B, dtype=self.torch.int32)
        self.repair_info = self.torch.full((self.B, 4), -1, dtype=self.torch.int32, device=self.dev)

    @staticmethod
    def check_plant(plant, resolution: float = None):
        """What BatchEpisode(plant=...) refuses (resolution: the world's, None without one)."""
        if not isinstance(plant, PlantParams):
            raise ValueError("plant must be a PlantParams")
        if not plant.supported(resolution):
            raise ValueError("plant: robot_radius beyond 15 cells at the world's resolution")

    def _init_plant(self, plant):
        """The commands under way and the tick counter of every robot (zero: at rest, nothing under way), and what the plant
        writes every tick besides pose and speed: fixed addresses."""
        self.plant = plant
        if plant is None:
            return
        self.check_plant(plant, self.resolution if self.world is not None else None)
        B = self.B
        self.plant_queue = self._zeros(B, 8, 2)
        self.plant_tick = self._zeros(B, dtype=self.torch.int32)
        self.plant_contact = self._zeros(B, 2, dtype=self.torch.int32)
        self.heading_cs = self._zeros(B, 2)

    @staticmethod
    def check_monitor(monitor, sensor):
        """What BatchEpisode(monitor=...) refuses (sensor: the episode's)."""
        if not isinstance(monitor, MonitorParams):
            raise ValueError("monitor must be a MonitorParams")
        if sensor is None:
            raise ValueError("monitor needs sensor=SensorParams(...): it reads the scan")
        if not monitor.supported():
            raise ValueError("monitor: more than 8 zones or more than 32 simulation steps")

    def _init_monitor(self, monitor):
        """What the monitor writes every tick: fixed addresses. It has no state."""
        self.monitor = monitor
        if monitor is None:
            return
        self.check_monitor(monitor, self.sensor)
        B = self.B
        self.cmd_safe = self._zeros(B, 2)
        self.monitor_action = self._zeros(B, 4, dtype=self.torch.int32)
        self.monitor_points = self._zeros(B, len(monitor.zones), dtype=self.torch.int32)
        self.monitor_ratio = self._zeros(B)
        self.monitor_heading_cs = self._zeros(B, 2)
        self.monitor_step_cs = self._zeros(B, 2)

    def set_detector_streams(self, streams):
        """streams [B] (0 .. 2^32 - 1): the stream ids of this episode's robots in place of their indices, so that a part of a
        larger batch draws what the same robots draw there. In place: a captured graph reads the new ids."""
        if self.detector is None:
            raise ValueError("this episode was built without detector")
        ids = np.asarray(streams)
        if ids.shape != (self.B,) or (ids != ids.astype(np.uint32)).any():
            raise ValueError("set_detector_streams: one id in 0 .. 2^32 - 1 per robot")
        self.draw_state[:, 0].copy_(self.torch.from_numpy(ids.astype(np.uint32).view(np.int32).copy()))

    def _init_shared(self, shared, pool, pool_crowd=None, pool_waypoints=None, pool_n_waypoints=None, pool_speed=None):
        """The table of a shared world, the gather's bins and workspace, and what it writes besides persons / person_count;
        with pool_crowd what the pool's crowd step reads and writes."""
        self.shared = shared
        self.pool_crowd = pool_crowd
        if shared is None:
            return
        torch, B = self.torch, self.B
        pool = np.zeros((0, 5)) if pool is None else np.ascontiguousarray(pool, np.float64)
        assert pool.ndim == 2 and pool.shape[1] == 5, "pool [M,5]"
        self.M = M = int(pool.shape[0])
        rows = B if shared.robots_as_people else 0
        self.agents = self._zeros(M + rows, 5)
        if M > 0:
            self.agents[:M].copy_(self._upload(pool, np.float64))
        self.agent_self = (torch.arange(M, M + B, dtype=torch.int32, device=self.dev) if rows
                           else torch.full((B,), -1, dtype=torch.int32, device=self.dev))
        self.person_source = torch.full((B, int(self.persons.shape[1])), -1, dtype=torch.int32, device=self.dev)
        self.shared_grid = shared.grid(self.world) if pool_crowd is None else shared.grid(self.world, pool_crowd.interaction_range)
        nbytes = self.solver.nearest_workspace_bytes(M + rows, self.shared_grid[0], self.shared_grid[1])
        if nbytes == 0:
            raise ValueError("the shared world's table or bins exceed the library's limits (include/smpc_nearest.h)")
        self.nearest_workspace = torch.zeros(nbytes, dtype=torch.uint8, device=self.dev)
        if pool_crowd is None:
            return
        if not self.od_shared:
            raise ValueError("pool_crowd needs ONE ObstacleDistance grid for the floor (od_indexes [h,w], or obstacles_from_costmap)")
        wp = np.ascontiguousarray(pool_waypoints, np.float64)
        assert wp.ndim == 3 and wp.shape[0] == M and wp.shape[1] >= 1 and wp.shape[2] == 2, "pool_waypoints [M,K,2]"
        assert np.shape(pool_n_waypoints) == (M,), "pool_n_waypoints [M]"
        self.pool_wp = self._upload(wp, np.float64)
        self.pool_nwp = self._upload(pool_n_waypoints, np.int32)
        self.pool_next = self._zeros(M, 5)
        self.pool_cursor = self._zeros(M, dtype=torch.int32)
        self.pool_speed = None
        if pool_speed is not None:
            assert np.shape(pool_speed) == (M,), "pool_speed [M]"
            self.pool_speed = self._upload(pool_speed, np.float64)

    def _init_sensor(self, sensor, sensor_memory=None):
        """The scan's tables (fixed for the episode), what it writes besides the windows, and its memory."""
        self.sensor = sensor
        self.sensor_memory = sensor_memory
        if sensor is None:
            return
        if not sensor.supported(self.resolution):
            raise ValueError("sensor: max_range beyond 127 cells or inflation_radius beyond 32 cells at the world's resolution")
        if self.size_x > 256 or self.size_y > 256:
            raise ValueError("sensor needs windows of at most 256 x 256 cells")
        table, _ = sensor.inflation_table(self.resolution)
        beams = sensor.beam_cells(self.resolution)
        if sensor_memory is not None:
            if not sensor_memory.supported(sensor, self.resolution):
                raise ValueError("sensor_memory: raytrace_range beyond 127 cells at the world's resolution")
            beams = sensor_memory.beam_cells(sensor, self.resolution)                      # the same directions, out to the clearing range
            self.obstacle_memory = self._zeros(self.B, self.size_y, (self.size_x + 31) // 32, dtype=self.torch.int32)
            self.obstacle_memory_cell = self._zeros(self.B, 2, dtype=self.torch.int32)
        self.sensor_beams = self._upload(beams, np.int32)                                  # [n_beams,2]
        self.sensor_table = self._upload(table, np.uint8)                                  # [d2_max + 1]
        self.beam_kind = self._zeros(self.B, int(sensor.n_beams), dtype=self.torch.uint8)
        self.beam_cell = self._zeros(self.B, int(sensor.n_beams), 2, dtype=self.torch.int32)

    def _bind(self):
        """Every struct a tick hands to the library, built once: every buffer the kernels read keeps its address from tick
        to tick (the state is updated in place), and the stream lives in the solver's handle, so nothing here changes
        when capture_graph moves the episode to another stream."""
        prm, B, T, N = self.params, self.B, self.T, self.N
        Np, planned, od = int(self.persons.shape[1]), self.plan is not None, (self.od_shared, self.od_h, self.od_w)
        c = self._c = SimpleNamespace()
        if self.world is not None:  # two structs that differ in `force`: a captured graph keeps the one its tick was given
            c.roll = {force: point(BatchSolver.local_costmap_c(B, self.size_x, self.size_y, self.world.cells_x, self.world.cells_y, True,
                                                               self.resolution, 1, self.outside_cost, force),
                                   {"world": self.world_map, "world_origin": self.world_origin, "pose": self.pose})
                      for force in (False, True)}
        if self.planner is not None:
            c.extract = point(BatchSolver.extract_plan_c(self.planner, B, int(self.plan_goals.shape[0]), self.world.cells_x,
                                                         self.world.cells_y, True, self.resolution, 1),
                              {"world": self.world_map, "world_origin": self.world_origin, "field": self.goal_field,
                               "goal": self.plan_goals, "robot_goal": self.robot_goal, "pose": self.pose})
        if planned:
            L = int(self.plan.shape[1])
            c.traj = point(BatchSolver.trajectorize_c(self.traj, B, L, 1),
                           {"plan": self.plan, "plan_len": self.plan_len, "robot_pose": self.pose})
            if self.plan_window is not None:  # the trajectorizer sees the window of the plan around the robot
                c.window = point(SmpcPlanWindowBatch(B=B, L=L, on_device=1, max_robot_pose_search_dist=float(self.plan_window[0]),
                                                     dist_threshold=float(self.plan_window[1])),
                                 {"plan": self.plan, "plan_len": self.plan_len, "plan_start": self.plan_start, "robot_pose": self.pose})
                point(c.traj, {"plan": self.window, "plan_len": self.window_len})
            c.traj_out = point(SmpcTrajectorizeOut(), {"path": self.plan_path, "cmds": self.plan_cmds, "cmds_vy": self.traj_vy,
                                                       "n_poses": self.traj_n, "error": self.traj_err})
        c.people = point(SmpcPeopleBatch(B=B, Np=Np, N=N, on_device=1), {"people": self.persons, "count": self.person_count})
        if self.shared is not None:
            gx, gy, origin, bin_size = self.shared_grid
            c.nearest = point(BatchSolver.nearest_c(B, Np, int(self.agents.shape[0]), gx, gy, origin, bin_size, self.shared.max_range, 1),
                              {"agents": self.agents if int(self.agents.shape[0]) > 0 else None, "robot_pose": self.pose,
                               "self": self.agent_self, "workspace": self.nearest_workspace})
            c.nearest.workspace_bytes = int(self.nearest_workspace.numel())
            if self.pool_crowd is not None and self.M > 0:  # the step reads the bins the tick's gather built: bins_ready
                c.pool = point(BatchSolver.crowd_pool_c(self.pool_crowd, self.M, int(self.agents.shape[0]), int(self.pool_wp.shape[1]),
                                                        prm.dt, gx, gy, origin, bin_size, 1, bins_ready=1),
                               {"agents": self.agents, "waypoints": self.pool_wp, "n_waypoints": self.pool_nwp,
                                "desired_speeds": self.pool_speed, "workspace": self.nearest_workspace})
                c.pool.workspace_bytes = int(self.nearest_workspace.numel())
                if self.od_indexes is not None and self.od_shared and self.od_h * self.od_w > 0:  # the world's one grid
                    point(c.pool, {"od_indexes": self.od_indexes, "od_origin": self.od_origin})
                    c.pool.od_height, c.pool.od_width, c.pool.od_resolution = int(self.od_h), int(self.od_w), float(self.od_resolution)
        if self.visibility is not None:  # the controller gets the persons in line of sight; the world keeps them all
            c.visibility = point(BatchSolver.visibility_c(self.visibility, B, Np, self.world.cells_x, self.world.cells_y, True,
                                                          self.resolution, 1),
                                 {"world": self.world_map, "world_origin": self.world_origin, "robot_pose": self.pose,
                                  "people": self.persons, "count": self.person_count})
            point(c.people, {"people": self.seen_persons, "count": self.seen_count})
        Nd = Np
        if self.detector is not None:  # what a detector would report of them: behind line of sight, in front of the tracker
            Nd = int(self.detected_persons.shape[1])
            c.detector = point(BatchSolver.detector_c(self.detector, B, Np, Nd, 1),
                               {"people": c.people.people, "count": c.people.count, "robot_pose": self.pose})
            point(c.people, {"people": self.detected_persons, "count": self.detected_count})
            c.people.Np = Nd
        if self.scan_detector is not None:  # what the robot's own scan shows of the people: in place of the ground-truth path
            Nd = int(self.scan_persons.shape[1])
            c.scan_people = point(BatchSolver.scan_people_c(self.scan_detector, B, int(self.sensor.n_beams), Nd, 1, self.resolution,
                                                            np.asarray(self.world.origin, np.float64).reshape(2), self.sensor, self.sensor_memory),
                                  {"robot_pose": self.pose, "beam_kind": self.beam_kind, "beam_cell": self.beam_cell})
            point(c.people, {"people": self.scan_persons, "count": self.scan_count})
            c.people.Np = Nd
        if self.repair is not None:  # the plans give way to what the windows show, in place
            c.repair = point(BatchSolver.repair_plan_c(self.repair, B, int(self.plan.shape[1]), self.size_x, self.size_y, self.costmap_shared,
                                                       self.resolution, 1),
                             {"costmap": self.costmap, "costmap_origin": self.costmap_origin, "robot_pose": self.pose,
                              "plan_start": self.plan_start if self.plan_window is not None else None})
        if self.tracker is not None:  # the controller gets tracks of what is detected: the last stage in front of the filter
            c.tracker = point(BatchSolver.tracker_c(self.tracker, B, Nd, Np, prm.dt, 1),
                              {"detections": c.people.people, "det_count": c.people.count, "robot_pose": self.pose})
            point(c.people, {"people": self.tracked_persons, "count": self.tracked_count})
            c.people.Np = Np
        if self.sensor is not None:  # the scan sees the true persons, whatever the controller is told of them
            sp = self.sensor
            c.sensor = point(BatchSolver.sensed_costmap_c(B, Np, self.size_x, self.size_y, self.world.cells_x, self.world.cells_y, True,
                                                          self.resolution, 1, int(sp.n_beams), sp.agent_d2(self.resolution),
                                                          int(self.sensor_table.numel()) - 1, sp.BASES.index(sp.base), self.outside_cost,
                                                          sp.occlusion_min_cost, sp.unknown_occludes),
                             {"world": self.world_map, "world_origin": self.world_origin, "robot_pose": self.pose,
                              "people": self.persons, "count": self.person_count, "cell": self.costmap_cell,
                              "beam_cells": self.sensor_beams, "inflation_cost": self.sensor_table})
            if self.sensor_memory is not None:
                c.sensor_memory = BatchSolver.obstacle_memory_c(c.sensor, self.sensor_memory.mark_d2(sp, self.resolution),
                                                                self.sensor_memory.footprint_d2(self.resolution))
        if self.fov_angle is not None:
            point(c.people, {"robot_pose": self.pose, "costmap_origin": self.costmap_origin})
            c.people.fov_angle, c.people.costmap_shared = float(self.fov_angle), 1 if self.costmap_shared else 0
            c.people.size_x, c.people.size_y, c.people.resolution = self.size_x, self.size_y, self.resolution
        c.memory = point(SmpcMemoryBatch(), {"prev_path": self.mem_path, "prev_cmds": self.mem_cmds, "valid": self.mem_valid,
                                             "length": self.mem_length})
        c.format = point(SmpcFormatBatch(B=B, T=T, path_rows=self.rows, on_device=1, time_step=float(prm.dt),
                                         current_path_w=float(prm.current_path_weight),
                                         current_cmds_w=float(prm.current_cmds_weight), memory=c.memory),
                         {"path": self.plan_path, "cmds": self.plan_cmds, "speed": self.speed})
        if planned:  # every robot with the horizon of its own trajectorized path
            c.format.n_poses, c.format.max_poses = self.traj_n.data_ptr(), self.max_poses
        c.format_out = point(SmpcFormatOut(), {"robot_status": self.robot_status, "pose0": self.pose0, "init_params": self.init_params,
                                               "path_pts": self.path_pts, "goal_yaw": self.goal_yaw, "T_scene": self.T_scene})
        c.projection = point(SmpcProjectionBatch(B=B, T=T, N=N, on_device=1, max_time=float(prm.max_time), time_step=float(prm.time_step)),
                             {"init_people": self.people, "robot_path": self.robot_status})
        set_od_grid(c.projection, "od_indexes", self.od_indexes, self.od_origin, self.od_resolution, od)
        c.scenes = point(SmpcSceneBatch(B=B, T=T, N=N, on_device=1, dt=prm.dt, costmap_shared=1 if self.costmap_shared else 0,
                                        size_x=self.size_x, size_y=self.size_y, resolution=self.resolution),
                         {"pose0": self.pose0, "init_params": self.init_params, "path_pts": self.path_pts, "goal_yaw": self.goal_yaw,
                          "people": self.people_proj, "has_people": self.has_people, "costmap": self.costmap,
                          "costmap_origin": self.costmap_origin,
                          "order": self.order if self.order_hint else None,  # longest scenes of the previous period first
                          "T_scene": self.T_scene if planned else None, "scene_params": self.scene_params})
        executed = self.cmd_vel  # the command that is executed: the monitor's when there is one
        if self.monitor is not None:
            c.monitor = point(BatchSolver.collision_monitor_c(self.monitor, B, int(self.sensor.n_beams), 1, self.resolution,
                                                              np.asarray(self.world.origin, np.float64).reshape(2)),
                              {"robot_pose": self.pose, "cmd": self.cmd_vel, "beam_kind": self.beam_kind, "beam_cell": self.beam_cell})
            executed = self.cmd_safe
        if self.crowd_params is not None:
            c.crowd = point(BatchSolver.crowd_c(self.crowd_params, B, Np, int(self.person_wp.shape[2]), prm.dt, 1),
                            {"robot_pose": self.pose, "robot_twist": executed, "count": self.person_count,
                             "waypoints": self.person_wp, "n_waypoints": self.person_nwp, "desired_speeds": self.person_speed})
            set_od_grid(c.crowd, "od_indexes", self.od_indexes, self.od_origin, self.od_resolution, od)
            c.groups = None
            if self.person_groups is not None:
                c.groups = BatchSolver.crowd_groups_c(self.crowd_group_params, self.person_groups.data_ptr())
        if self.plant is not None:  # the plant sees the true persons and the world's walls, whatever the controller is told
            if self.world is not None:
                c.plant = point(BatchSolver.plant_c(self.plant, prm, B, Np, 1, self.world.cells_x, self.world.cells_y, self.resolution,
                                                    np.asarray(self.world.origin, np.float64).reshape(2)), {"world": self.world_map})
            else:
                c.plant = BatchSolver.plant_c(self.plant, prm, B, Np, 1)
            point(c.plant, {"cmd": executed, "agents": self.persons, "count": self.person_count})
        if self.metrics_params is not None:
            c.metrics = point(BatchSolver.metrics_c(self.metrics_params, B, Np, prm.dt, 1),
                              {"robot_pose": self.pose, "robot_twist": executed if self.plant is None else self.speed,  # the twist executed
                               "people": self.persons, "count": self.person_count, "goal": self.goal, "status": self.res["status"],
                               "source": self.cmd_source})
            if hasattr(self, "od_distances"):  # the clearance columns
                set_od_grid(c.metrics, "od_distances", self.od_distances, self.od_origin, self.od_resolution, od)

    # -- trajectorizer (row f3) on the global plans, or the arc stand-in: v = 0.6, w = w_ref from the current pose --
    def _plan(self, timing: dict = None):
        torch, s, c = self.torch, self.solver, self._c
        if self.plan is not None:
            if self.plan_window is not None:
                s.transform_global_plan_device(c.window, self.window.data_ptr(), self.window_len.data_ptr(), self.window_err.data_ptr())
                if timing is not None:
                    timing["window_ms"] = s.last_kernel_ms()
            s.trajectorize_device(c.traj, c.traj_out)
            return
        dt = self.params.dt
        k = torch.arange(self.T + 1, dtype=torch.float64, device=self.dev)[None, :]
        th = self.pose[:, 2:3] + self.w_ref[:, None] * dt * k
        inc = 0.6 * dt * torch.stack([torch.cos(th), torch.sin(th)], dim=-1)           # step k -> k+1
        xy = self.pose[:, None, 0:2] + torch.cumsum(inc, dim=1) - inc                  # exclusive prefix sum
        self.plan_path[:, :, 0:2] = xy
        self.plan_path[:, :, 2] = th
        self.plan_cmds[:, :, 0] = 0.6
        self.plan_cmds[:, :, 1] = self.w_ref[:, None]

    def _roll(self):
        """The rolling costmaps follow the robots: one launch; every window is written when none has been yet."""
        self.solver.local_costmap_device(self._c.roll[self._force_roll], self.costmap_cell.data_ptr(), self.costmap.data_ptr(),
                                         self.costmap_origin.data_ptr(), self.costmap_moved.data_ptr())
        self._force_roll = False

    def _gather(self):
        """The shared world as the robots perceive it now: the robots' rows of the table from pose and speed (x, y,
        v cos yaw, v sin yaw, w), then every robot's nearest agents into persons / person_count / person_source."""
        torch, M = self.torch, self.M
        if self.shared.robots_as_people:
            v, th = self.speed[:, 0], self.pose[:, 2]
            self.agents[M:, 0:2] = self.pose[:, 0:2]
            self.agents[M:, 2] = v * torch.cos(th)
            self.agents[M:, 3] = v * torch.sin(th)
            self.agents[M:, 4] = self.speed[:, 1]
        self.solver.nearest_people_device(self._c.nearest, self.persons.data_ptr(), self.person_count.data_ptr(),
                                          self.person_source.data_ptr())

    def replan(self):
        """Every robot's plan again, from its current pose down its goal's field, into the same self.plan / self.plan_len /
        self.plan_error; the plan window starts at the head of the new plans. Between ticks; never inside a captured one."""
        if self.planner is None:
            raise ValueError("this episode was built without planner")
        torch = self.torch
        if self.gstream is not None and torch.cuda.current_stream(self.dev) != self.gstream:
            with torch.cuda.stream(self.gstream):  # after capture_graph the library's handle lives on the capture stream
                return self.replan()
        self.solver.extract_plan_device(self._c.extract, self.plan.data_ptr(), self.plan_len.data_ptr(), self.plan_error.data_ptr())
        if self.plan_window is not None:
            self.plan_start.zero_()

    def _host(self, *names, **renamed) -> dict:
        """Host copies of device buffers for a TickRecord: {name: self.<name>} and {key: self.<attribute>}."""
        return {k: getattr(self, a).cpu().numpy().copy() for k, a in [(n, n) for n in names] + list(renamed.items())}

    def _memory_host(self) -> dict:
        return self._host(prev_path="mem_path", prev_cmds="mem_cmds", valid="mem_valid", length="mem_length")

    def tick(self, record: bool = False, timing: dict = None):
        """One controller period for all B robots. Returns a TickRecord when `record`, else None. `timing`: a dict
        that receives the HIP-event duration (ms) of each stage's kernel (synchronises after every stage)."""
        torch = self.torch
        if self.gstream is not None and torch.cuda.current_stream(self.dev) != self.gstream:
            with torch.cuda.stream(self.gstream):  # after capture_graph the library's handle lives on the capture stream
                return self.tick(record, timing)
        s, c, B, T = self.solver, self._c, self.B, self.T
        planned, windowed, crowd = self.plan is not None, self.plan_window is not None, self.crowd_params is not None
        pool_crowd = self.shared is not None and self.pool_crowd is not None and self.M > 0

        def timed(stage):
            if timing is not None:
                timing[stage + "_ms"] = s.last_kernel_ms()

        rec = {}
        if record:
            rec.update(self._host(robot_pose="pose"))
        if self.world is not None:  # the ground first: everything below reads the windows where the robots are now
            self._roll()
            timed("local_costmap")
            if record:
                rec.update(self._host("costmap_cell", "costmap_origin", "costmap_moved"))
        self._plan(timing)
        if planned:
            timed("trajectorize")
        if self.shared is not None:  # one crowd for everybody, the other robots in it
            self._gather()
            timed("nearest")
            if record:
                rec.update(self._host("agents", "person_source"))
        if record:
            if planned:
                rec.update(self._host(traj_n_poses="traj_n"))
                if windowed:
                    rec.update(self._host("window", "window_len", "plan_start"))
            rec.update(self._host("persons", "person_count"))
            if crowd:
                rec.update(self._host(cursor_before="person_cursor"))
        if self.sensor_memory is not None:  # the scan with its memory: marks stay until a beam passes them
            if record:
                rec.update(self._host(obstacle_memory_before="obstacle_memory", obstacle_memory_cell_before="obstacle_memory_cell"))
            s.obstacle_memory_device(c.sensor_memory, self.obstacle_memory.data_ptr(), self.obstacle_memory_cell.data_ptr(),
                                     self.costmap.data_ptr(), self.beam_kind.data_ptr(), self.beam_cell.data_ptr())
            timed("obstacle_memory")
            if record:
                rec.update(self._host("beam_kind", "beam_cell", sensed_costmap="costmap", obstacle_memory_after="obstacle_memory"))
        elif self.sensor is not None:  # what the scan hits, inflated, into the windows the solve reads
            s.sensed_costmap_device(c.sensor, self.costmap.data_ptr(), self.beam_kind.data_ptr(), self.beam_cell.data_ptr())
            timed("sensed_costmap")
            if record:
                rec.update(self._host("beam_kind", "beam_cell", sensed_costmap="costmap"))
        if self.repair is not None:  # behind the sensing stage: detours around what the windows show, for the next tick's plan stage
            if record:
                rec.update(self._host(repair_plan_before="plan", repair_plan_len_before="plan_len"))
                if self.sensor is None:
                    rec.update(self._host(repair_costmap="costmap"))
            s.repair_plan_device(c.repair, self.plan.data_ptr(), self.plan_len.data_ptr(), self.plan_scratch.data_ptr(),
                                 self.repair_status.data_ptr(), self.repair_info.data_ptr())
            timed("repair")
            if record:
                rec.update(self._host("repair_status", "repair_info", repair_plan_after="plan", repair_plan_len_after="plan_len"))
        if self.scan_detector is not None:  # the tick's beam hits clustered into person-sized segments: detections from the scan
            s.scan_people_device(c.scan_people, self.scan_persons.data_ptr(), self.scan_count.data_ptr(), self.scan_segment.data_ptr(),
                                 self.scan_stats.data_ptr())
            timed("scan_people")
            if record:
                rec.update(self._host("scan_persons", "scan_count", "scan_segment", "scan_stats"))
        if self.visibility is not None:  # the persons in line of sight, directly in front of the filter that reads them
            s.visible_people_device(c.visibility, self.seen_persons.data_ptr(), self.seen_count.data_ptr(), self.person_seen.data_ptr())
            timed("visibility")
            if record:
                rec.update(self._host("person_seen", "seen_count", "seen_persons"))
        if self.detector is not None:  # what a detector would report: body occlusion, misses, noise, clutter
            if record:
                rec["draw_state_before"] = self.draw_state.cpu().numpy().view(np.uint32).copy()
            s.detect_people_device(c.detector, self.draw_state.data_ptr(), self.detected_persons.data_ptr(), self.detected_count.data_ptr(),
                                   self.detected_source.data_ptr(), self.person_outcome.data_ptr())
            timed("detector")
            if record:
                rec.update(self._host("detected_persons", "detected_count", "detected_source", "person_outcome"))
                rec["draw_state_after"] = self.draw_state.cpu().numpy().view(np.uint32).copy()
        if self.tracker is not None:  # tracks of the detections: velocities from positions, and a memory of who stepped out of sight
            if record:
                rec.update(self._host(tracks_before="tracks", track_meta_before="track_meta", track_next_id_before="track_next_id"))
            s.track_people_device(c.tracker, self.tracks.data_ptr(), self.track_meta.data_ptr(), self.track_next_id.data_ptr(),
                                  self.tracked_persons.data_ptr(), self.tracked_count.data_ptr(), self.tracked_source.data_ptr())
            timed("tracker")
            if record:
                rec.update(self._host("tracked_persons", "tracked_count", "tracked_source", tracks_after="tracks",
                                      track_meta_after="track_meta", track_next_id_after="track_next_id"))
        # 0. field-of-view filter + people_to_status
        s.people_to_status_device(c.people, self.people.data_ptr(), self.has_people.data_ptr())
        timed("people")
        if record:
            rec.update(self._host("plan_path", "plan_cmds", "speed", "has_people", init_people="people"),
                       memory_before=self._memory_host())
        # 1. format_to_optimize + memory
        s.format_device(c.format, c.format_out)
        timed("format")
        # 2. project_people
        s.project_people_device(c.projection, self.people_proj.data_ptr(), self.proj_error.data_ptr())
        timed("project")
        # 3. solve
        s.solve_device(c.scenes, self.rb)
        timed("solve")
        if self.order_hint:
            self.order.copy_(BatchSolver.longest_first(self.res["evaluations"]))
        # 4. memory store (usable solves only; T_scene + 1 poses and commands of each)
        s.memory_store_device(B, T, self.res["status"].data_ptr(), self.res["path"].data_ptr(), self.res["cmds"].data_ptr(),
                              c.memory, self.T_scene.data_ptr() if planned else 0)
        timed("store")
        if record:
            rec.update(self._host("T_scene", "robot_status", "pose0", "init_params", "path_pts", "goal_yaw", "people_proj",
                                  "proj_error"), result={k: v.cpu().numpy().copy() for k, v in self.res.items()},
                       memory_after=self._memory_host())
            if windowed:
                rec.update(self._host("window_err"))
        # 5. the command computeVelocityCommands returns (fallbacks included), then the world moves one period with it:
        #    a usable solve lands the robot on the first optimised pose, a fallback command is integrated with the
        #    trajectorizer's own motion model (x, y with the old heading, then the heading)
        s.select_command_device(B, T, self.rows, self.traj_n.data_ptr() if planned else 0,
                                self.plan_cmds.data_ptr(), self.res["status"].data_ptr(), self.res["cmds"].data_ptr(),
                                self.cmd_vel.data_ptr(), self.cmd_source.data_ptr(), self.window_err.data_ptr() if windowed else 0)
        executed = self.cmd_vel
        if self.monitor is not None:  # the safety layer between the controller and the base: the tick's scan against its zones
            s.collision_monitor_device(c.monitor, self.cmd_safe.data_ptr(), self.monitor_action.data_ptr(), self.monitor_points.data_ptr(),
                                       self.monitor_ratio.data_ptr(), self.monitor_heading_cs.data_ptr(), self.monitor_step_cs.data_ptr())
            timed("monitor")
            executed = self.cmd_safe
            if record:
                rec.update(self._host("cmd_safe", "monitor_action", "monitor_points", "monitor_ratio", "monitor_heading_cs", "monitor_step_cs"))
        dt = self.params.dt
        if crowd:  # the persons' period: they see the pose it starts from and the command executed
            self._crowd_step()
            timed("crowd")
        if pool_crowd:  # the pedestrians' period, from the table the tick's gather read: the robots where the period started
            if record:
                rec.update(self._host(pool_cursor_before="pool_cursor"))
            s.crowd_pool_step_device(c.pool, self.pool_next.data_ptr(), self.pool_cursor.data_ptr())
            timed("pool_crowd")
            if record:
                rec.update(self._host("pool_next", pool_cursor_after="pool_cursor"))
        if self.plant is not None:  # the base executes the command: limits, latency, and contacts with walls and agents
            if record:
                rec.update(self._host(plant_agents="persons", plant_agent_count="person_count", plant_queue_before="plant_queue"))
                rec["plant_tick_before"] = self.plant_tick.cpu().numpy().view(np.uint32).copy()
            s.robot_plant_device(c.plant, self.pose.data_ptr(), self.speed.data_ptr(), self.plant_queue.data_ptr(),
                                 self.plant_tick.data_ptr(), self.plant_contact.data_ptr(), self.heading_cs.data_ptr())
            timed("plant")
            if record:
                rec.update(self._host("plant_contact", "heading_cs", plant_queue_after="plant_queue", speed_after="speed"))
                rec["plant_tick_after"] = self.plant_tick.cpu().numpy().view(np.uint32).copy()
        else:
            v, w, th = executed[:, 0], executed[:, 1], self.pose[:, 2]
            moved = torch.stack([self.pose[:, 0] + v * torch.cos(th) * dt, self.pose[:, 1] + v * torch.sin(th) * dt, th + w * dt], dim=1)
            optimised = (self.cmd_source == 0)[:, None]
            if self.monitor is not None:  # a command the monitor changed is not the one the optimised path was planned with
                optimised = optimised & (self.monitor_ratio == 1.0)[:, None]
            # state is updated in place: every buffer the kernels read keeps its address from tick to tick (_bind)
            self.pose.copy_(torch.where(optimised, self.res["path"][:, 0, :], moved))
            self.speed.copy_(executed)
        if self.shared is not None:  # the pool walks on; what a robot perceives of it is gathered, not moved
            M = self.M
            if pool_crowd:
                self.agents[:M].copy_(self.pool_next)
            else:
                self.agents[:M, 0] += self.agents[:M, 2] * dt
                self.agents[:M, 1] += self.agents[:M, 3] * dt
        elif not crowd:
            self.persons[:, :, 0] += self.persons[:, :, 2] * dt
            self.persons[:, :, 1] += self.persons[:, :, 3] * dt
        if self.metrics_params is not None:  # 6. one metrics sample of the world as the period leaves it
            if self.shared is not None:  # ... the other robots at their new poses included
                self._gather()
                timed("nearest_after")
                if record:
                    rec.update(self._host(agents_after="agents"))
            self._metrics_sample()
            timed("metrics")
            if record:
                rec.update(self._host("metrics_acc"))
        if record:
            rec.update(self._host("cmd_vel", "cmd_source", pose_after="pose", persons_after="persons"))
            if crowd:
                rec.update(self._host(cursor_after="person_cursor"))
        self.ticks += 1
        return TickRecord(**rec) if record else None

    def _crowd_step(self, groups: bool = True):
        """One crowd period; groups=False: the plain step even when the episode has groups."""
        self.solver.crowd_step_device(self._c.crowd, self.persons.data_ptr(), self.person_cursor.data_ptr(),
                                      self._c.groups if groups else None)

    def _metrics_sample(self):
        self.solver.episode_metrics_device(self._c.metrics, self.metrics_acc.data_ptr())

    def metrics(self) -> np.ndarray:
        """Host copy of the metrics rows [B,24] (columns solver.METRIC_COLS) accumulated so far."""
        if self.metrics_params is None:
            raise ValueError("this episode was built without metrics")
        self.torch.cuda.synchronize()
        return self.metrics_acc.cpu().numpy().copy()

    def capture_graph(self, stream=None):
        """Record one tick (every kernel of the chain and the torch ops of the world model) into a HIP graph on `stream`
        (a new side stream by default) and make tick() replay it: one graph launch per control period instead of ~25
        kernel launches from Python, which is what lets several independent shards keep the GPU busy (ShardedEpisode).
        One warm-up tick runs first (the library's buffers grow on first use); the episode's state is put back after it."""
        torch = self.torch
        self.gstream = stream if stream is not None else torch.cuda.Stream(device=self.dev)
        self.gstream.wait_stream(torch.cuda.current_stream(self.dev))
        self.solver.set_stream(self.gstream.cuda_stream)
        state = ("pose", "speed", "persons", "mem_path", "mem_cmds", "mem_valid", "mem_length", "order") + (("plan_start",) if self.plan_window is not None else ())
        if self.metrics_params is not None:
            state += ("metrics_acc",)  # the warm-up tick's sample does not count
        if self.crowd_params is not None:
            state += ("person_cursor",)
        if self.shared is not None:
            state += ("agents", "person_count", "person_source")
            if self.pool_crowd is not None:
                state += ("pool_cursor",)
        if self.sensor_memory is not None:
            state += ("obstacle_memory", "obstacle_memory_cell")
        if self.tracker is not None:
            state += ("tracks", "track_meta", "track_next_id")
        if self.detector is not None:
            state += ("draw_state",)
        if self.plant is not None:
            state += ("plant_queue", "plant_tick")
        if self.repair is not None:
            state += ("plan", "plan_len")  # the warm-up tick may have spliced a detour in
        with torch.cuda.stream(self.gstream):
            saved = {k: getattr(self, k).clone() for k in state}
            ticks = self.ticks
            self.tick()  # warm-up on the capture stream: the library's buffers grow, torch's allocator settles
        self.gstream.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.gstream):
            self.tick()
        with torch.cuda.stream(self.gstream):  # the world is where it was before the warm-up tick
            for k in state:
                getattr(self, k).copy_(saved[k])
        self.ticks = ticks
        if self.world is not None:
            self._force_roll = True
        return self.graph

    def replay(self):
        """One control period through the captured graph (on the capture stream)."""
        with self.torch.cuda.stream(self.gstream):
            if self.world is not None and self._force_roll:
                # the first replay: every window is written from cell (0,0), as an eager episode's first tick does; the
                # graph's own roll (captured without `force`) then finds every window in place
                self._roll()
            self.graph.replay()
        self.ticks += 1

    def synchronize(self):
        self.torch.cuda.synchronize()


def shard_kwargs(kwargs: dict, idx: np.ndarray, B: int) -> dict:
    """BatchEpisode's keyword arguments for the robots `idx` of a batch of B, from those for the whole batch: the rows idx
    of the per-robot arrays (BatchEpisode.PER_ROBOT, and PER_GRID when there is a grid per scene: od_indexes [B,h,w] with
    B > 1), every other one (FORWARDED) as it is. A name BatchEpisode declares in none of the three is refused."""
    unknown = set(kwargs) - set(BatchEpisode.PER_ROBOT + BatchEpisode.PER_GRID + BatchEpisode.FORWARDED)
    if unknown:
        raise TypeError(f"BatchEpisode declares {sorted(unknown)} neither per robot nor forwarded")
    od = kwargs.get("od_indexes")
    per_scene = od is not None and np.ndim(od) == 3 and np.shape(od)[0] > 1
    rows = BatchEpisode.PER_ROBOT + (BatchEpisode.PER_GRID if per_scene else ())
    out = {}
    for k, v in kwargs.items():
        if k in rows and v is not None:
            assert np.shape(v)[0] == B, f"{k}: one row per robot"
            v = np.asarray(v)[idx]
        out[k] = v
    return out


def concurrent_streams(n: int, device: str, candidates: int = 12):
    """n torch streams that really run side by side. Streams are mapped onto a few hardware queues by the runtime; two
    streams that share a queue execute one after the other, and which pool stream lands where is not visible from
    here (three shards were measured at 2.7 ms or 4.1 ms per tick depending on nothing but the streams the pool
    handed out). Candidates are probed with a pair of spin kernels: a pair that takes as long as the two spins in a
    row shares a queue. Falls back to the first n pool streams when the probe kernel is not available."""
    import time

    import torch

    pool = [torch.cuda.Stream(device=device) for _ in range(max(n, candidates))]
    spin = getattr(torch.cuda, "_sleep", None)
    if spin is None or n < 2:
        return pool[:n]
    cycles = 1_000_000  # a few hundred microseconds

    def pair_time(a, b):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for st in ((a,) if b is None else (a, b)):
            with torch.cuda.stream(st):
                spin(cycles)
        torch.cuda.synchronize(device)
        return time.perf_counter() - t0

    pair_time(pool[0], pool[1])  # warm-up
    alone = min(pair_time(pool[0], None) for _ in range(3))
    chosen = [pool[0]]
    for cand in pool[1:]:
        if len(chosen) == n:
            break
        if all(min(pair_time(c, cand) for _ in range(2)) < 1.5 * alone for c in chosen):
            chosen.append(cand)
    for cand in pool:  # not enough independent queues: fill up with whatever is left
        if len(chosen) == n:
            break
        if cand not in chosen:
            chosen.append(cand)
    return chosen


class ShardedEpisode:
    """The robots of a batch are independent of each other (every scene has its own plan, people, memory; a shared world,
    BatchEpisode(shared=...), is therefore refused), so a tick of
    B robots can be issued as `shards` chains of B / shards robots on separate HIP streams: while one shard's solve
    launch drains its last long-running scenes, the other shards' kernels keep the CUs busy (the same overlap the
    serving bench gets from independent batches; a single chain pays the tail of every launch). Three things make it
    pay (measured at 8192 robots, 8 people, tools/gpu_episode.py / tools/shard_caps.sh): every shard's tick is one HIP
    graph launch (from Python the ~25 launches per shard-tick make the host the bottleneck); every solve launch sizes its
    persistent grid to 1 / shards of the resident wavefronts (smpc_set_solve_share: oversubscribed grids leave the other
    shards' small kernels waiting for wave slots); the small kernels run at the highest wave priority (next to another
    shard's solve they took 5-10x longer at equal priority). Three shards: 2.72 ms per tick against 3.24-3.32 ms for
    the single chain; two: 2.87; four and more fall behind again (more streams than hardware queues). Per-robot results
    are those of the one-stream episode bit for bit (kernels take every decision per scene / per lane)."""

    def __init__(self, params: OptimizerParams, scenes: SceneBatch, w_ref: np.ndarray, od_indexes: np.ndarray,
                 od_origin: np.ndarray, od_resolution: float, device: int = 0, shards: int = 3, graphs: bool = True,
                 solve_share: int = None, **episode_kw):
        """episode_kw: the other keyword arguments of BatchEpisode, for all B robots; every shard gets its robots' part
        of them (shard_kwargs). detector_streams [B] (with detector=; default arange(B)): the robots' stream ids; every
        shard gets its robots' (BatchEpisode.set_detector_streams), so a shard draws what the same robots draw unsharded."""
        import torch

        if episode_kw.get("shared") is not None or episode_kw.get("pool") is not None:
            raise ValueError("ShardedEpisode refuses shared / pool: its shards are independent by construction")
        self.torch = torch
        B = scenes.B
        detector_streams = episode_kw.pop("detector_streams", None)
        if detector_streams is not None and episode_kw.get("detector") is None:
            raise ValueError("detector_streams needs detector")
        shards = max(1, min(shards, B))
        edges = [B * k // shards for k in range(shards + 1)]
        self.slices = [slice(edges[k], edges[k + 1]) for k in range(shards) if edges[k + 1] > edges[k]]
        self.streams = concurrent_streams(len(self.slices), f"cuda:{device}")
        self.parts = []
        kw = dict(episode_kw, od_indexes=od_indexes, od_origin=od_origin, od_resolution=od_resolution, device=device)
        for sl, st in zip(self.slices, self.streams):
            idx = np.arange(sl.start, sl.stop)
            with torch.cuda.stream(st):  # the shard's solver handle binds to the stream current at construction
                self.parts.append(BatchEpisode(params, scenes.select(idx), np.asarray(w_ref)[idx], **shard_kwargs(kw, idx, B)))
                if self.parts[-1].detector is not None:
                    self.parts[-1].set_detector_streams(idx if detector_streams is None else np.asarray(detector_streams)[idx])
        self.B = B
        self.graphs = graphs
        for part in self.parts:  # every shard's persistent solve grid takes its share of the resident wavefronts
            part.solver.set_solve_share(solve_share if solve_share else len(self.parts))
        if graphs:  # one HIP graph per shard: a tick is `shards` graph launches
            for part, st in zip(self.parts, self.streams):
                part.capture_graph(st)

    def tick(self):
        for part, st in zip(self.parts, self.streams):
            if self.graphs:
                part.replay()
            else:
                with self.torch.cuda.stream(st):
                    part.tick()

    def synchronize(self):
        self.torch.cuda.synchronize()

    def gather(self, name: str):
        """Concatenated per-robot tensor: a key of BatchEpisode.res ("status", "cmds", ...) or an attribute ("pose",
        "cmd_vel", "cmd_source", "proj_error", "metrics_acc", "persons", "person_cursor")."""
        self.synchronize()
        return self.torch.cat([p.res[name] if name in p.res else getattr(p, name) for p in self.parts], dim=0)


def far_obstacle_grid(cells: int = 120, resolution: float = 0.1, origin=(-6.0, -6.0)):
    """An ObstacleDistance grid whose every cell points at one far corner obstacle (valid, but inert for the crowd)."""
    idx = np.zeros((cells, cells), np.uint32)  # all cells -> cell 0 (the grid corner)
    return idx, np.asarray(origin, np.float64), float(np.float32(resolution))


def arc_plans(pose0: np.ndarray, curvature: np.ndarray, L: int = 400, ds: float = 0.05):
    """Synthetic global plans: constant-curvature arcs of L poses (spacing ds) from each robot's start pose.
    Returns (plan [B,L,2], plan_len [B])."""
    B = pose0.shape[0]
    plan = np.zeros((B, L, 2))
    x, y, th = pose0[:, 0].copy(), pose0[:, 1].copy(), pose0[:, 2].copy()
    for i in range(L):
        plan[:, i, 0], plan[:, i, 1] = x, y
        x, y, th = x + ds * np.cos(th), y + ds * np.sin(th), th + curvature * ds
    return plan, np.full(B, L, np.int32)
