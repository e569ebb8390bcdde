"""Closed-loop (receding-horizon) batch episodes: B independent robots, every tick runs the whole
`Optimizer::optimize` chain of the reference on the device. The launch order of a tick, which tick() reads against; the
optional stages are BatchEpisode.STAGES, one class each in episode_stages, [Core] the chain tick() writes out:

    once, at construction:
    ObstacleDistance grid (optional)         (src/optimizer.cpp:593-605, 'TODO')   -> smpc_obstacle_distance_batch
    global plans (optional; Planner; again     (Nav2's planner server; the library's -> smpc_goal_field_batch,
    on replan(), never inside a tick)          own integer cost rule)                 smpc_extract_plan_batch
      ... smoothed (planner.smoother), behind   (Nav2's smoother server; the library's
      every walk                                own Jacobi rule)                    -> smpc_smooth_plan_batch
    every tick:
    rolling local costmap (Rolling)          (Nav2's LayeredCostmap::updateMap)    -> smpc_local_costmap_batch
    plan window, trajectorizer (with plans)  (src/social_mpc_controller.cpp:171-189,
                                              src/path_trajectorizer.cpp:120-288)  -> smpc_transform_global_plan_batch,
                                                                                      smpc_trajectorize_path_batch
    nearest-agent gather (Shared)            (none: the library's own rule)        -> smpc_nearest_people_batch
    sensed local costmap (Sensed)            (Nav2's ObstacleLayer + InflationLayer;
                                              the library's own memoryless scan)   -> smpc_sensed_costmap_batch
      ... or with memory (ObstacleMemory)    (its persistent marking and ray-trace
                                              clearing; the library's own rule)     -> smpc_obstacle_memory_batch
    plan repair (Repair)                     (none: the library's own rule)        -> smpc_repair_plan_batch
    people detections from the scan          (the deployment's own leg detector;
      (ScanPeople, or the next two)           the library's own rule)               -> smpc_scan_people_batch
    line-of-sight filter (Visibility)        (none: the library's own rule)        -> smpc_visible_people_batch
    people detections (Detector)             (the deployment's own detector; the
                                              library's own rule)                   -> smpc_detect_people_batch
    people tracks (Tracker)                  (the deployment's own tracker behind
                                              people_msgs::People; the library's rule) -> smpc_track_people_batch
    [Core] field-of-view filter + people_to_status (src/social_mpc_controller.cpp:196-214, src/optimizer.cpp:454-482)
                                                                                   -> smpc_people_to_status_batch
    [Core] format_to_optimize + TrajectoryMemory (src/optimizer.cpp:172-190, 484-551) -> smpc_format_to_optimize_batch
    [Core] project_people                    (src/optimizer.cpp:554-728)           -> smpc_project_people_batch
    [Core] problem assembly + ceres::Solve + unpack (src/optimizer.cpp:197-446)    -> smpc_solve_batch
    [Core] memory store                      (src/optimizer.cpp:448-449)           -> smpc_memory_store_batch
    [Core] command selection                 (src/social_mpc_controller.cpp:180-189, 241-245) -> smpc_select_command_batch
    collision monitor (Monitor)              (Nav2's collision_monitor behind the
                                              controller; the library's own rule)   -> smpc_collision_monitor_batch
    reactive crowd (Crowd)                   (sfm.hpp computeForces / updatePosition) -> smpc_crowd_step_batch
    reactive pool (PoolCrowd)                (the same on the shared pool)         -> smpc_crowd_pool_step_batch
    robot plant (Plant), else the torch      (the deployment's base behind cmd_vel;
      motion model                            the library's own rule)               -> smpc_robot_plant_batch
    the persons' or the pool's move (torch), with Shared and Metrics a second nearest-agent gather
    episode metrics (Metrics)                (none: the library's own rule)        -> smpc_episode_metrics_batch

as in SocialMPCController::computeVelocityCommands,
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
from .episode_stages import (Core, Crowd, Detector, Metrics, Monitor, ObstacleMemory, Perception, Planner, Plant, PoolCrowd, Repair, Rolling,
                             ScanPeople, Sensed, Shared, Told, Tracker, Visibility)
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
    # The optional stages in launch order (episode_stages; the module docstring above), around the chain tick() writes out.
    # ObstacleMemory launches in Sensed's place; Planner launches at construction and in replan(), never in a tick.
    STAGES = (Rolling, Shared, Sensed, ObstacleMemory, Repair, ScanPeople, Visibility, Detector, Tracker, Core,
              Monitor, Crowd, PoolCrowd, Plant, Metrics)
    # what the core chain and the world model carry from tick to tick (capture_graph; `plan_start` with a plan window)
    CORE_STATE = ("pose", "speed", "persons", "mem_path", "mem_cmds", "mem_valid", "mem_length", "order")
    UINT32 = ("draw_state", "plant_tick")  # int32 tensors that hold the bits of the library's uint32 words: recorded as such
    check_plant = staticmethod(Plant.check)
    check_monitor = staticmethod(Monitor.check)
    check_scan_detector = staticmethod(ScanPeople.check)
    check_repair = staticmethod(Repair.check)

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
        The optional stages, each None by default: nothing is allocated and nothing is launched. The docstring of the stage's
        class in episode_stages says what the keyword, and the arguments that go with it, mean:
        world (with outside_cost): Rolling, the costmaps as rolling windows of one world map.
        planner (with goal): Planner, global plans from the world map.
        shared (with pool): Shared, one world of pedestrians and robots for all robots.
        pool_crowd (with pool_waypoints, pool_n_waypoints, pool_speed): PoolCrowd, the shared pool as a reactive crowd.
        sensor: Sensed, the windows hold what a scan hits.
        sensor_memory: ObstacleMemory, the scan's marks persist until a beam clears them.
        repair: Repair, detours around what the windows show, spliced into the plans.
        scan_detector: ScanPeople, people detections from the scan.
        visibility: Visibility, only the persons in line of sight are perceived.
        detector: Detector, what a detector would report of them.
        tracker: Tracker, tracks in place of detections.
        monitor: Monitor, the command passes a collision monitor.
        crowd (with person_waypoints, person_n_waypoints, person_speed, person_groups, crowd_groups): Crowd, the robots' own
        persons as a reactive crowd.
        plant: Plant, the command is executed by a model of the base.
        metrics (with goal, od_distances): Metrics, every robot is scored on the device."""
        import torch

        kw = dict(locals())  # every argument by its name: a stage finds its own under its KEY
        res, planned = scenes.resolution, plan is not None or planner is not None

        def refuse(S, *context):  # what a stage that is asked for refuses, before anything touches the device
            if kw[S.KEY] is not None:
                S.check(kw[S.KEY], *context)

        refuse(Planner, plan, plan_len, world, traj_params, goal)
        refuse(Rolling, scenes.costmap_shared, res)
        refuse(Visibility, world, res)
        refuse(Sensed, world, res, scenes.size_x, scenes.size_y)
        refuse(ObstacleMemory, sensor, res)
        # these three also refuse the arguments that go with them when they are absent themselves
        Shared.check(shared, pool, world, scenes.N, crowd=crowd, person_waypoints=person_waypoints, person_n_waypoints=person_n_waypoints,
                     person_speed=person_speed, person_groups=person_groups)
        PoolCrowd.check(pool_crowd, shared, pool, pool_waypoints, pool_n_waypoints, pool_speed)
        Crowd.check(crowd, person_waypoints, person_n_waypoints, person_groups)
        refuse(Tracker, params.dt)
        refuse(Detector)
        refuse(Plant, res if world is not None else None)
        refuse(Monitor, sensor)
        refuse(ScanPeople, sensor, visibility, detector, res)
        refuse(Repair, planned, res)
        for S in (Planner,) + self.STAGES:  # self.world, self.tracker, ...: the stages' parameters, None where absent
            if S is not Core:
                setattr(self, S.ATTR or S.KEY, kw[S.KEY])
        self.stages = tuple(S for S in self.STAGES if S is not Core and kw[S.KEY] is not None)
        self.torch, self.params, self.dev = torch, params, f"cuda:{device}"
        self.solver = BatchSolver(params, device)
        # library kernels and the few torch ops of the world model share one stream, so they are ordered
        self.solver.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
        self.B, self.T, self.N = scenes.B, scenes.T, scenes.N
        if planned:
            # Plan mode: every robot is solved with the horizon its own trajectorized path gives it (smpc_format_batch.n_poses
            # -> T_scene). The arrays are sized for the longest one: a path of exactly max_poses = round(max_time / dt)
            # poses is not cut by format_to_optimize (src/optimizer.cpp:491-497) and so has one step more than the longer,
            # cut, paths: T = max_poses - 1 = rollout_steps + 1.
            assert self.T == params.rollout_steps
            self.T += 1
        self.P = params.dims(self.T, True)[3]
        self._init_world(scenes, w_ref, fov_angle, outside_cost)
        self._init_grid(od_indexes, od_origin, od_resolution, od_distances, obstacles_from_costmap, obstacle_min_cost,
                        unknown_is_obstacle, distances=metrics is not None)
        self._init_memory()
        self._init_plan(kw)
        self._init_solve(order_hint, scene_params)
        for S in self.stages:
            S.allocate(self, kw)
        self._bind()
        self.graph, self.gstream, self.ticks = None, None, 0
        if planner is not None:
            self.replan()

    # -- construction: device buffers first (the core's here, a stage's in its allocate), then (_bind) the structs that point into them
    def _upload(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.dev)

    def _zeros(self, *shape, dtype=None):
        return self.torch.zeros(shape, dtype=dtype or self.torch.float64, device=self.dev)

    def _init_world(self, scenes, w_ref, fov_angle, outside_cost):
        """The robots, the persons, the costmaps and the world map they are windows of."""
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
        if self.shared is not None:  # the gather writes them every tick; the scenes' own people stay on the host
            self.persons = self._zeros(self.B, self.N if self.shared.max_people is None else int(self.shared.max_people), 5)
            self.person_count = self._zeros(self.B, dtype=i32)
        else:
            self.persons = self._upload(persons, np.float64)
            self.person_count = self._upload(count, np.int32)
        self.person_groups = None
        self.fov_angle = fov_angle
        self.people = self._zeros(self.B, self.N, 6)                                    # people_to_status output
        self.has_people = self._zeros(self.B, dtype=self.torch.uint8)
        self.costmap = self.torch.from_numpy(scenes.costmap).to(self.dev)
        self.costmap_origin = self.torch.from_numpy(scenes.costmap_origin).to(self.dev)
        self.costmap_shared = scenes.costmap_shared
        self.size_x, self.size_y, self.resolution = scenes.size_x, scenes.size_y, scenes.resolution
        if self.world is not None:  # the grid, the planner and most stages read it
            self.world_map = self._upload(self.world.map, np.uint8)                     # [Hy,Hx]
            self.world_origin = self._upload(np.asarray(self.world.origin, np.float64).reshape(1, 2), np.float64)
            self.outside_cost = int(outside_cost)

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

    def _init_plan(self, kw):
        """The global plans with the trajectorizer's (and the plan window's) outputs, or the rows of the arc stand-in."""
        B, i32 = self.B, self.torch.int32
        self.traj = traj_params = kw["traj_params"]
        self.plan, self.plan_window, self.rows = None, None, self.T + 1
        if kw["plan"] is not None or self.planner is not None:
            assert traj_params is not None and traj_params.max_steps + 1 >= self.T + 1
            if self.planner is not None:
                Planner.allocate(self, kw)
            else:
                self.plan = self._upload(kw["plan"], np.float64)
                self.plan_len = self._upload(kw["plan_len"], np.int32)
            self.rows = traj_params.max_steps + 1
            self.traj_n = self._zeros(B, dtype=i32)
            self.traj_err = self._zeros(B, dtype=i32)
            self.traj_vy = self._zeros(B, self.rows)
            self.plan_window = kw["plan_window"]
            if self.plan_window is not None:
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

    def set_detector_streams(self, streams):
        """streams [B] (0 .. 2^32 - 1): the stream ids of this episode's robots in place of their indices, so that a part of a
        larger batch draws what the same robots draw there. In place: a captured graph reads the new ids."""
        if self.detector is None:
            raise ValueError("this episode was built without detector")
        ids = np.asarray(streams)
        if ids.shape != (self.B,) or (ids != ids.astype(np.uint32)).any():
            raise ValueError("set_detector_streams: one id in 0 .. 2^32 - 1 per robot")
        self.draw_state[:, 0].copy_(self.torch.from_numpy(ids.astype(np.uint32).view(np.int32).copy()))

    def _bind(self):
        """Every struct a tick hands to the library, built once: every buffer the kernels read keeps its address from tick
        to tick (the state is updated in place), and the stream lives in the solver's handle, so nothing here changes
        when capture_graph moves the episode to another stream. The core's structs here, a stage's in its bind."""
        prm, B, T, N = self.params, self.B, self.T, self.N
        planned, od = self.plan is not None, (self.od_shared, self.od_h, self.od_w)
        c = self._c = SimpleNamespace()
        self.executed = self.cmd_vel if self.monitor is None else self.cmd_safe  # the command that is executed
        if self.planner is not None:
            Planner.bind(self)
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
        told = Told(self.persons, self.person_count, int(self.persons.shape[1]))  # the simulator's rows: the world keeps them all
        for S in self.stages:
            if issubclass(S, Perception):
                told = S.bind(self, told)
            else:
                S.bind(self)
        c.people = point(SmpcPeopleBatch(B=B, Np=told.Np, N=N, on_device=1), {"people": told.rows, "count": told.count})
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

    # -- trajectorizer (row f3) on the global plans, or the arc stand-in: v = 0.6, w = w_ref from the current pose --
    def _plan(self, timing: dict = None):
        torch, s, c = self.torch, self.solver, self._c
        if self.plan is not None:
            if self.plan_window is not None:
                s.transform_global_plan_device(c.window, self.window.data_ptr(), self.window_len.data_ptr(), self.window_err.data_ptr())
                self._timed(timing, "window")
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

    def replan(self):
        """Every robot's plan again, from its current pose down its goal's field, into the same self.plan / self.plan_len /
        self.plan_error; the plan window starts at the head of the new plans. Between ticks; never inside a captured one."""
        if self.planner is None:
            raise ValueError("this episode was built without planner")
        torch = self.torch
        if self.gstream is not None and torch.cuda.current_stream(self.dev) != self.gstream:
            with torch.cuda.stream(self.gstream):  # after capture_graph the library's handle lives on the capture stream
                return self.replan()
        Planner.launch(self)
        if self.plan_window is not None:
            self.plan_start.zero_()

    def _host(self, *names, **renamed) -> dict:
        """Host copies of device buffers for a TickRecord: {name: self.<name>} and {key: self.<attribute>}, the UINT32 ones as
        such; {key: function}: what the function returns."""
        pairs = dict(zip(names, names), **renamed)
        out = {k: a() if callable(a) else getattr(self, a).cpu().numpy().copy() for k, a in pairs.items()}
        return dict(out, **{k: out[k].view(np.uint32) for k, a in pairs.items() if a in self.UINT32})

    def _memory_host(self) -> dict:
        return self._host(prev_path="mem_path", prev_cmds="mem_cmds", valid="mem_valid", length="mem_length")

    def _result_host(self) -> dict:
        return {k: v.cpu().numpy().copy() for k, v in self.res.items()}

    def _timed(self, timing: dict, key: str):
        """The HIP-event duration of the launch just made, when the tick is timed."""
        if timing is not None:
            timing[key + "_ms"] = self.solver.last_kernel_ms()

    def _run(self, stage, rec: dict, timing: dict):
        """An optional stage's slot of the tick, when the episode has the stage: its launch, with the record's copies before
        and after it and its kernel's time."""
        if stage not in self.stages:
            return
        if rec is not None:
            rec.update(self._host(**stage.BEFORE))
        stage.launch(self)
        self._timed(timing, stage.TIMING)
        if rec is not None:
            rec.update(self._host(**stage.AFTER))

    def tick(self, record: bool = False, timing: dict = None):
        """One controller period for all B robots, in the module docstring's order. Returns a TickRecord when `record`, else
        None. `timing`: a dict that receives the HIP-event duration (ms) of each stage's kernel (synchronises after every stage)."""
        torch = self.torch
        if self.gstream is not None and torch.cuda.current_stream(self.dev) != self.gstream:
            with torch.cuda.stream(self.gstream):  # after capture_graph the library's handle lives on the capture stream
                return self.tick(record, timing)
        s, c, B, T, dt, st = self.solver, self._c, self.B, self.T, self.params.dt, self.stages
        planned, windowed = self.plan is not None, self.plan_window is not None
        rec = {} if record else None

        def run(stage):
            self._run(stage, rec, timing)

        def keep(*names, **renamed):  # host copies into the record: buffers by name, or what a function returns
            if record:
                rec.update(self._host(*names, **renamed))

        keep(robot_pose="pose")
        run(Rolling)  # the ground first: everything below reads the windows where the robots are now
        self._force_roll = False
        self._plan(timing)
        if planned:
            self._timed(timing, "trajectorize")
            keep(traj_n_poses="traj_n")
            if windowed:
                keep("window", "window_len", "plan_start")
        run(Shared)  # one crowd for everybody, the other robots in it
        keep("persons", "person_count")
        run(ObstacleMemory if ObstacleMemory in st else Sensed)  # the scan into the windows the solve reads, with or without its memory
        if Repair in st and Sensed not in st:
            keep(repair_costmap="costmap")  # the windows the repair reads, when no sensing stage recorded them
        run(Repair)  # detours around what the windows show, for the next tick's plan stage
        run(ScanPeople)
        run(Visibility)
        run(Detector)
        run(Tracker)
        # 0. field-of-view filter + people_to_status
        s.people_to_status_device(c.people, self.people.data_ptr(), self.has_people.data_ptr())
        self._timed(timing, "people")
        keep("plan_path", "plan_cmds", "speed", "has_people", init_people="people", memory_before=self._memory_host)
        # 1. format_to_optimize + memory
        s.format_device(c.format, c.format_out)
        self._timed(timing, "format")
        # 2. project_people
        s.project_people_device(c.projection, self.people_proj.data_ptr(), self.proj_error.data_ptr())
        self._timed(timing, "project")
        # 3. solve
        s.solve_device(c.scenes, self.rb)
        self._timed(timing, "solve")
        if self.order_hint:
            self.order.copy_(BatchSolver.longest_first(self.res["evaluations"]))
        # 4. memory store (usable solves only; T_scene + 1 poses and commands of each)
        s.memory_store_device(B, T, self.res["status"].data_ptr(), self.res["path"].data_ptr(), self.res["cmds"].data_ptr(),
                              c.memory, self.T_scene.data_ptr() if planned else 0)
        self._timed(timing, "store")
        keep("T_scene", "robot_status", "pose0", "init_params", "path_pts", "goal_yaw", "people_proj", "proj_error", *(("window_err",) if windowed else ()),
             result=self._result_host, memory_after=self._memory_host)
        # 5. the command computeVelocityCommands returns (fallbacks included), then the world moves one period with it:
        #    a usable solve lands the robot on the first optimised pose, a fallback command is integrated with the
        #    trajectorizer's own motion model (x, y with the old heading, then the heading)
        s.select_command_device(B, T, self.rows, self.traj_n.data_ptr() if planned else 0,
                                self.plan_cmds.data_ptr(), self.res["status"].data_ptr(), self.res["cmds"].data_ptr(),
                                self.cmd_vel.data_ptr(), self.cmd_source.data_ptr(), self.window_err.data_ptr() if windowed else 0)
        run(Monitor)  # the safety layer between the controller and the base: self.executed is its command from here on
        run(Crowd)  # the persons' period: they see the pose it starts from and the command executed
        pool_crowd = PoolCrowd in st and self.M > 0
        if pool_crowd:  # the pedestrians' period, from the table the tick's gather read: the robots where the period started
            run(PoolCrowd)
        if Plant in st:  # the base executes the command: limits, latency, and contacts with walls and agents
            run(Plant)
        else:
            v, w, th = self.executed[:, 0], self.executed[:, 1], self.pose[:, 2]
            moved = torch.stack([self.pose[:, 0] + v * torch.cos(th) * dt, self.pose[:, 1] + v * torch.sin(th) * dt, th + w * dt], dim=1)
            optimised = (self.cmd_source == 0)[:, None]
            if Monitor in st:  # a command the monitor changed is not the one the optimised path was planned with
                optimised = optimised & (self.monitor_ratio == 1.0)[:, None]
            # state is updated in place: every buffer the kernels read keeps its address from tick to tick (_bind)
            self.pose.copy_(torch.where(optimised, self.res["path"][:, 0, :], moved))
            self.speed.copy_(self.executed)
        if Shared in st:  # the pool walks on; what a robot perceives of it is gathered, not moved
            if pool_crowd:
                self.agents[:self.M].copy_(self.pool_next)
            else:
                self.agents[:self.M, 0] += self.agents[:self.M, 2] * dt
                self.agents[:self.M, 1] += self.agents[:self.M, 3] * dt
        elif Crowd not in st:
            self.persons[:, :, 0] += self.persons[:, :, 2] * dt
            self.persons[:, :, 1] += self.persons[:, :, 3] * dt
        if Metrics in st and Shared in st:  # the sample sees the other robots at their new poses
            Shared.launch(self)
            self._timed(timing, "nearest_after")
            keep(agents_after="agents")
        run(Metrics)  # 6. one metrics sample of the world as the period leaves it
        keep("cmd_vel", "cmd_source", pose_after="pose", persons_after="persons")
        self.ticks += 1
        return TickRecord(**rec) if record else None

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
        One warm-up tick runs first (the library's buffers grow on first use); the episode's state, the core's and every
        stage's STATE, is put back after it."""
        torch = self.torch
        self.gstream = stream if stream is not None else torch.cuda.Stream(device=self.dev)
        self.gstream.wait_stream(torch.cuda.current_stream(self.dev))
        self.solver.set_stream(self.gstream.cuda_stream)
        state = self.saved_state()
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
        self._force_roll = True
        return self.graph

    def saved_state(self) -> tuple:
        """The attributes a tick reads before it writes them: what capture_graph puts back after its warm-up tick."""
        return self.CORE_STATE + (("plan_start",) if self.plan_window is not None else ()) + sum((S.STATE for S in self.stages), ())

    def replay(self):
        """One control period through the captured graph (on the capture stream)."""
        with self.torch.cuda.stream(self.gstream):
            if Rolling in self.stages and self._force_roll:
                # the first replay: every window is written from cell (0,0), as an eager episode's first tick does; the
                # graph's own roll (captured without `force`) then finds every window in place
                Rolling.launch(self)
                self._force_roll = False
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
