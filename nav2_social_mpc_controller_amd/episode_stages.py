"""The optional stages of the closed-loop tick (episode.BatchEpisode), one class each. A class is a namespace and is never
instantiated: its functions take the episode `ep` (there is no self) and are called on the class, Tracker.launch(ep). It says
everything the episode has to know of its stage:

    KEY      the keyword of BatchEpisode.__init__ that switches the stage on (ATTR: the episode's attribute that keeps its
             value, where that is not the keyword itself)
    TIMING   its key in tick(timing=...), without the "_ms"
    STATE    the episode's buffers the stage carries from tick to tick: capture_graph saves them around its warm-up tick
    BEFORE   TickRecord field -> episode attribute, copied to the host before the launch when a tick is recorded
    AFTER    the same, after the launch
    check    what the stage refuses, without a GPU: its own parameters first, then what the refusals depend on (Shared, PoolCrowd
             and Crowd take None as well: they refuse the arguments that go with them when the stage itself is absent)
    allocate its buffers, as attributes of the episode (kw: BatchEpisode.__init__'s arguments by name)
    bind     its struct, once, into ep._c (an absent stage leaves no entry there)
    launch   its one library call

Two values are handed from stage to stage when the structs are bound. What the controller is told about people is a `Told`
(rows, count, Np): the perception stages (Perception) take the one upstream of them and return their own, in their tick order:
the simulator's rows, line of sight, detector or scan detector, tracker; people_to_status reads the last. The command that is
executed is ep.executed: cmd_vel, or cmd_safe behind a monitor; the crowd, the plant, the motion model and the metrics take it.

BatchEpisode.STAGES lists the classes in launch order; adding a stage is a class here, its position there, its keyword and its
TickRecord fields."""
from collections import namedtuple

import numpy as np

from .params import (CrowdGroupParams, DetectorParams, MonitorParams, PlanRepairParams, PlanSmootherParams, PlantParams, ScanDetectorParams,
                     TrackerParams)
from .solver import BatchSolver, point, set_od_grid

Told = namedtuple("Told", "rows count Np")  # what the controller is told about people: two device tensors, rows per robot


def same(*names, **renamed) -> dict:
    """A BEFORE / AFTER table: the fields that carry their attribute's name, and the renamed ones."""
    return dict({n: n for n in names}, **renamed)


def given(**named) -> str:
    return ", ".join(sorted(k for k, v in named.items() if v is not None))


def world_origin(ep):
    return np.asarray(ep.world.origin, np.float64).reshape(2)


class Stage:
    KEY, ATTR, TIMING = None, None, None
    STATE = ()
    BEFORE, AFTER = {}, {}


class Perception(Stage):
    """A stage between the simulator's person rows and people_to_status: bind(ep, told) returns what it tells on."""


class Core:
    """Place marker in BatchEpisode.STAGES for the chain that tick() writes out: people_to_status, format, projection, solve,
    memory store and command selection."""


class Planner(Stage):
    """planner: the global plans come from the world map (include/smpc_global_plan.h) instead of `plan`, which is refused:
    needs `world`, `traj_params` and goal [B,2]. One goal field per distinct row of `goal` (found on the host;
    ep.robot_goal [B] maps the robots onto them) is computed at construction, once (smpc_goal_field_batch), and every robot's
    plan is walked down its field from its start pose (smpc_extract_plan_batch) into ep.plan [B,planner.max_poses,2],
    ep.plan_len and ep.plan_error [B] (enum smpc_plan_error; a robot with an error other than TRUNCATED has plan_len 0 and
    gets no command). From there on this is the episode that was handed these arrays as `plan`. replan() walks again from the
    current poses. Never inside a tick, so not in BatchEpisode.STAGES. None: nothing is allocated and nothing is launched.
    planner.smoother (PlanSmootherParams; include/smpc_plan_smoother.h): every walk goes into ep.plan_raw (which is therefore,
    stale rows behind plan_len included, the plan buffer of the episode without a smoother), the whole buffer is copied to
    ep.plan and one smpc_smooth_plan_batch relaxes ep.plan in place on the world map; ep.smooth_status [B] int32
    (enum smpc_smooth_status), ep.smooth_info [B,4] int32 (sweeps, rounds, rejected, n) and ep.smooth_change [B] say how it
    ended. Everything behind it reads the smoothed rows. None: nothing more is allocated or launched and the episode is the
    one without bit for bit."""
    KEY = "planner"

    def check(planner, plan, plan_len, world, traj_params, goal):
        if plan is not None or plan_len is not None:
            raise ValueError("planner computes the global plans: plan / plan_len cannot be given as well")
        if world is None or traj_params is None or goal is None:
            raise ValueError("planner needs world, traj_params and goal [B,2]")
        smoother = getattr(planner, "smoother", None)
        if smoother is not None:
            if not isinstance(smoother, PlanSmootherParams):
                raise ValueError("planner.smoother must be a PlanSmootherParams")
            if not smoother.supported(planner.max_poses):
                raise ValueError("planner.smoother: more than 1024 poses, more than 100000 sweeps a round or more than 8 refinements")

    def allocate(ep, kw):
        """The goal fields of the robots' distinct goals, computed once, and the buffers every (re)plan is walked into."""
        B, i32 = ep.B, ep.torch.int32
        goal = np.ascontiguousarray(kw["goal"], np.float64)
        assert goal.shape == (B, 2), "goal [B,2]"
        goals, robot_goal = np.unique(goal, axis=0, return_inverse=True)
        G = goals.shape[0]
        ep.plan_goals = ep._upload(goals, np.float64)                              # [G,2]
        ep.robot_goal = ep._upload(np.asarray(robot_goal).reshape(B), np.int32)    # [B]
        ep.goal_field = ep.torch.empty((G, ep.world.cells_y, ep.world.cells_x), dtype=i32, device=ep.dev)  # uint32 bits
        ep.goal_status = ep._zeros(G, dtype=i32)
        gf = point(BatchSolver.goal_field_c(ep.planner, G, ep.world.cells_x, ep.world.cells_y, True, ep.resolution, 1),
                   {"world": ep.world_map, "world_origin": ep.world_origin, "goal": ep.plan_goals})
        ep.solver.goal_field_device(gf, ep.goal_field.data_ptr(), ep.goal_status.data_ptr())
        ep.plan_error = ep._zeros(B, dtype=i32)
        ep.plan, ep.plan_len = ep._zeros(B, ep.planner.max_poses, 2), ep._zeros(B, dtype=i32)
        if ep.planner.smoother is not None:  # the plans as walked, and how their smoothing ended
            ep.plan_raw = ep.torch.zeros_like(ep.plan)
            ep.smooth_status = ep._zeros(B, dtype=i32)
            ep.smooth_info = ep._zeros(B, 4, dtype=i32)
            ep.smooth_change = ep._zeros(B)

    def bind(ep):
        ep._c.extract = point(BatchSolver.extract_plan_c(ep.planner, ep.B, int(ep.plan_goals.shape[0]), ep.world.cells_x,
                                                         ep.world.cells_y, True, ep.resolution, 1),
                              {"world": ep.world_map, "world_origin": ep.world_origin, "field": ep.goal_field,
                               "goal": ep.plan_goals, "robot_goal": ep.robot_goal, "pose": ep.pose})
        if ep.planner.smoother is not None:
            gp = ep.planner
            ep._c.smooth = point(BatchSolver.smooth_plan_c(gp.smoother, ep.B, int(gp.max_poses), ep.world.cells_x, ep.world.cells_y, True,
                                                           ep.resolution, 1, gp.lethal_min_cost, gp.allow_unknown),
                                 {"world": ep.world_map, "world_origin": ep.world_origin, "plan_len": ep.plan_len})

    def launch(ep):
        if ep.planner.smoother is None:
            ep.solver.extract_plan_device(ep._c.extract, ep.plan.data_ptr(), ep.plan_len.data_ptr(), ep.plan_error.data_ptr())
        else:
            # The walk goes into plan_raw and the whole buffer is copied: a walk writes its first plan_len rows only, so the rows
            # behind a shorter new plan keep what the walk before left there, as they do without a smoother, not smoothed rows.
            ep.solver.extract_plan_device(ep._c.extract, ep.plan_raw.data_ptr(), ep.plan_len.data_ptr(), ep.plan_error.data_ptr())
            ep.plan.copy_(ep.plan_raw)
            ep.solver.smooth_plan_device(ep._c.smooth, ep.plan.data_ptr(), ep.smooth_status.data_ptr(), ep.smooth_info.data_ptr(),
                                         ep.smooth_change.data_ptr())


class Rolling(Stage):
    """world: the map the robots drive on (scenes.World, e.g. scenes.make_world with scenes.scenes_in_world): the scenes'
    costmaps (one per robot, of the world's resolution) become rolling windows of it. The world is uploaded once and
    ep.costmap_cell [B,2] holds the world cell of every window's cell (0,0); every tick starts, before the plan window
    and the trajectorizer, with smpc_local_costmap_batch at the robots' current poses, which rewrites the windows (and
    costmap_origin) of the robots whose window moved and leaves the others alone; window cells beyond the world read
    outside_cost. The first tick, and the first replay of a captured graph, write every window (`force`). With
    obstacles_from_costmap the ObstacleDistance grid is computed from the world map, once, shared by all robots, with
    the world's origin (with distances when metrics ask for them); host-given od_* are taken as they are. None:
    nothing is allocated and nothing is launched."""
    KEY, TIMING = "world", "local_costmap"
    AFTER = same("costmap_cell", "costmap_origin", "costmap_moved")

    def check(world, costmap_shared, resolution):
        if costmap_shared:
            raise ValueError("world needs a costmap per robot (costmap_shared = False, e.g. scenes.scenes_in_world)")
        if float(world.resolution) != float(resolution):
            raise ValueError("the world and the scenes' costmaps differ in resolution")

    def allocate(ep, kw):
        """Where every window is. (The world map itself is the episode's: the grid and the planner read it before any stage.)"""
        ep.costmap_cell = ep._zeros(ep.B, 2, dtype=ep.torch.int32)
        ep.costmap_moved = ep._zeros(ep.B, dtype=ep.torch.int32)
        ep._force_roll = True  # the next roll writes every window: the first tick, the first replay of a graph

    def bind(ep):  # two structs that differ in `force`: a captured graph keeps the one its tick was given
        ep._c.roll = {force: point(BatchSolver.local_costmap_c(ep.B, ep.size_x, ep.size_y, ep.world.cells_x, ep.world.cells_y, True,
                                                               ep.resolution, 1, ep.outside_cost, force),
                                   {"world": ep.world_map, "world_origin": ep.world_origin, "pose": ep.pose})
                      for force in (False, True)}

    def launch(ep):
        """The rolling costmaps follow the robots: one launch; every window is written when none has been yet (the caller
        then clears ep._force_roll)."""
        ep.solver.local_costmap_device(ep._c.roll[ep._force_roll], ep.costmap_cell.data_ptr(), ep.costmap.data_ptr(),
                                       ep.costmap_origin.data_ptr(), ep.costmap_moved.data_ptr())


class Shared(Stage):
    """shared: one world for all robots (include/smpc_nearest.h): needs `world`; `crowd` and the person_* arguments are
    refused (they move private rows). The scenes' own people are not uploaded. ep.agents [M+B,5] is one table of
    people_msgs::Person rows: the M rows of pool [M,5] (e.g. scenes.shared_pool; None: no pedestrians) followed, with
    shared.robots_as_people, by one row per robot (x, y, v cos yaw, v sin yaw, w), which ep.agent_self [B] = M + b
    keeps a robot from perceiving as somebody else (without robots_as_people the table is the pool alone and
    agent_self is -1). Every tick, after the roll and the plan stage and before the line-of-sight filter, the robots'
    rows are refreshed from ep.pose and ep.speed and smpc_nearest_people_batch writes each robot's at most
    Np = shared.max_people (default: the scenes' N) nearest agents within shared.max_range, nearest first, into
    ep.persons [B,Np,5] / ep.person_count [B] (ep.person_source [B,Np]: their rows of the table), the addresses
    everything behind it reads. The pool moves with constant velocity, in place; the caller may rewrite
    ep.agents[:M] between ticks. With `metrics` the rows are refreshed and gathered a second time after the move, so
    that the sample sees the world as the period leaves it, the other robots at their new poses included. None (then
    pool must be None too): nothing is allocated and nothing is launched."""
    KEY, TIMING = "shared", "nearest"
    STATE = ("agents", "person_count", "person_source")
    AFTER = same("agents", "person_source")  # `persons` and `person_count`, which the gather wrote, are the core's fields

    def check(shared, pool, world, N, **private):
        """private: crowd and the person_* arguments."""
        if shared is None:
            if pool is not None:
                raise ValueError("pool needs shared=SharedWorldParams(...)")
            return
        if world is None:
            raise ValueError("shared needs world: the robots and the pool share its floor")
        if given(**private):
            raise ValueError(f"shared refuses {given(**private)}: the reactive crowd step moves private rows")
        Np = int(shared.max_people) if shared.max_people is not None else N  # person rows per robot
        if not 1 <= Np <= 64:
            raise ValueError(f"shared needs 1 <= max_people <= 64 rows per robot, got {Np}")

    def allocate(ep, kw):
        """The table, the gather's bins and workspace, and what it writes besides persons / person_count."""
        torch, B, pool = ep.torch, ep.B, kw["pool"]
        pool = np.zeros((0, 5)) if pool is None else np.ascontiguousarray(pool, np.float64)
        assert pool.ndim == 2 and pool.shape[1] == 5, "pool [M,5]"
        ep.M = M = int(pool.shape[0])
        rows = B if ep.shared.robots_as_people else 0
        ep.agents = ep._zeros(M + rows, 5)
        if M > 0:
            ep.agents[:M].copy_(ep._upload(pool, np.float64))
        ep.agent_self = (torch.arange(M, M + B, dtype=torch.int32, device=ep.dev) if rows
                         else torch.full((B,), -1, dtype=torch.int32, device=ep.dev))
        ep.person_source = torch.full((B, int(ep.persons.shape[1])), -1, dtype=torch.int32, device=ep.dev)
        ep.shared_grid = ep.shared.grid(ep.world) if ep.pool_crowd is None else ep.shared.grid(ep.world, ep.pool_crowd.interaction_range)
        nbytes = ep.solver.nearest_workspace_bytes(M + rows, ep.shared_grid[0], ep.shared_grid[1])
        if nbytes == 0:
            raise ValueError("the shared world's table or bins exceed the library's limits (include/smpc_nearest.h)")
        ep.nearest_workspace = torch.zeros(nbytes, dtype=torch.uint8, device=ep.dev)

    def bind(ep):
        gx, gy, origin, bin_size = ep.shared_grid
        A = int(ep.agents.shape[0])
        ep._c.nearest = point(BatchSolver.nearest_c(ep.B, int(ep.persons.shape[1]), A, gx, gy, origin, bin_size, ep.shared.max_range, 1),
                              {"agents": ep.agents if A > 0 else None, "robot_pose": ep.pose, "self": ep.agent_self, "workspace": ep.nearest_workspace})
        ep._c.nearest.workspace_bytes = int(ep.nearest_workspace.numel())

    def launch(ep):
        """The shared world as the robots perceive it now: the robots' rows of the table from pose and speed (x, y,
        v cos yaw, v sin yaw, w), then every robot's nearest agents into persons / person_count / person_source."""
        torch, M = ep.torch, ep.M
        if ep.shared.robots_as_people:
            v, th = ep.speed[:, 0], ep.pose[:, 2]
            ep.agents[M:, 0:2] = ep.pose[:, 0:2]
            ep.agents[M:, 2] = v * torch.cos(th)
            ep.agents[M:, 3] = v * torch.sin(th)
            ep.agents[M:, 4] = ep.speed[:, 1]
        ep.solver.nearest_people_device(ep._c.nearest, ep.persons.data_ptr(), ep.person_count.data_ptr(), ep.person_source.data_ptr())


class Sensed(Stage):
    """sensor: the robots' windows are sensed (include/smpc_sensed_costmap.h): needs `world`. Every tick, after the roll, the
    plan stage and the shared world's gather and before the line-of-sight filter, one smpc_sensed_costmap_batch casts
    sensor.n_beams beams from ep.pose over the world map and the true ep.persons / ep.person_count (with `shared`
    the other robots among them), marks the cells they stop at in the windows at ep.costmap_cell, inflates the marks
    and rewrites ep.costmap, which the solve reads; ep.beam_kind [B,n_beams] (enum smpc_beam_kind) and
    ep.beam_cell [B,n_beams,2] hold each beam's outcome. sensor.base "world" keeps the world cut underneath. The
    ObstacleDistance grid stays the world's. None: nothing is allocated and nothing is launched."""
    KEY, TIMING = "sensor", "sensed_costmap"
    AFTER = same("beam_kind", "beam_cell", sensed_costmap="costmap")

    def check(sensor, world, resolution, size_x, size_y):
        if world is None:
            raise ValueError("sensor needs world: the scan runs over the world map")
        if not sensor.supported(resolution):
            raise ValueError("sensor: max_range beyond 127 cells or inflation_radius beyond 32 cells at the world's resolution")
        if size_x > 256 or size_y > 256:
            raise ValueError("sensor needs windows of at most 256 x 256 cells")

    def allocate(ep, kw):
        """The scan's tables (fixed for the episode) and what it writes besides the windows."""
        sensor, memory = ep.sensor, ep.sensor_memory
        # with a memory the same directions, out to the clearing range
        beams = sensor.beam_cells(ep.resolution) if memory is None else memory.beam_cells(sensor, ep.resolution)
        ep.sensor_beams = ep._upload(beams, np.int32)                                       # [n_beams,2]
        ep.sensor_table = ep._upload(sensor.inflation_table(ep.resolution)[0], np.uint8)    # [d2_max + 1]
        ep.beam_kind = ep._zeros(ep.B, int(sensor.n_beams), dtype=ep.torch.uint8)
        ep.beam_cell = ep._zeros(ep.B, int(sensor.n_beams), 2, dtype=ep.torch.int32)

    def bind(ep):  # the scan sees the true persons, whatever the controller is told of them
        sp = ep.sensor
        ep._c.sensor = point(BatchSolver.sensed_costmap_c(ep.B, int(ep.persons.shape[1]), ep.size_x, ep.size_y, ep.world.cells_x,
                                                          ep.world.cells_y, True, ep.resolution, 1, int(sp.n_beams), sp.agent_d2(ep.resolution),
                                                          int(ep.sensor_table.numel()) - 1, sp.BASES.index(sp.base), ep.outside_cost,
                                                          sp.occlusion_min_cost, sp.unknown_occludes),
                             {"world": ep.world_map, "world_origin": ep.world_origin, "robot_pose": ep.pose, "people": ep.persons,
                              "count": ep.person_count, "cell": ep.costmap_cell, "beam_cells": ep.sensor_beams, "inflation_cost": ep.sensor_table})

    def launch(ep):
        ep.solver.sensed_costmap_device(ep._c.sensor, ep.costmap.data_ptr(), ep.beam_kind.data_ptr(), ep.beam_cell.data_ptr())


class ObstacleMemory(Stage):
    """sensor_memory: the scan has a memory (include/smpc_obstacle_memory.h): needs `sensor`. One
    smpc_obstacle_memory_batch takes the place of the tick's smpc_sensed_costmap_batch: the beams reach out to
    sensor_memory.raytrace_range and clear the cells they pass, hits are marked within sensor.max_range, the cells
    under the robot are cleared, and a mark stays until a beam passes it. The state is ep.obstacle_memory
    [B,size_y,(size_x + 31) // 32] int32 (one bit per window cell, zero at the start) and ep.obstacle_memory_cell
    [B,2]. None: nothing is allocated, nothing new is launched and the episode is the sensed one bit for bit."""
    KEY, TIMING = "sensor_memory", "obstacle_memory"
    STATE = ("obstacle_memory", "obstacle_memory_cell")
    BEFORE = same(obstacle_memory_before="obstacle_memory", obstacle_memory_cell_before="obstacle_memory_cell")
    AFTER = dict(Sensed.AFTER, obstacle_memory_after="obstacle_memory")  # it launches in the scan's place: the scan's outputs too

    def check(sensor_memory, sensor, resolution):
        if sensor is None:
            raise ValueError("sensor_memory needs sensor=SensorParams(...): it is the scan's memory")
        if not sensor_memory.supported(sensor, resolution):
            raise ValueError("sensor_memory: raytrace_range beyond 127 cells at the world's resolution")

    def allocate(ep, kw):
        ep.obstacle_memory = ep._zeros(ep.B, ep.size_y, (ep.size_x + 31) // 32, dtype=ep.torch.int32)
        ep.obstacle_memory_cell = ep._zeros(ep.B, 2, dtype=ep.torch.int32)

    def bind(ep):  # behind Sensed: the scan's struct inside
        ep._c.sensor_memory = BatchSolver.obstacle_memory_c(ep._c.sensor, ep.sensor_memory.mark_d2(ep.sensor, ep.resolution),
                                                            ep.sensor_memory.footprint_d2(ep.resolution))

    def launch(ep):
        ep.solver.obstacle_memory_device(ep._c.sensor_memory, ep.obstacle_memory.data_ptr(), ep.obstacle_memory_cell.data_ptr(),
                                         ep.costmap.data_ptr(), ep.beam_kind.data_ptr(), ep.beam_cell.data_ptr())


class Repair(Stage):
    """repair: the plans give way to what the windows show (include/smpc_plan_repair.h); needs `plan` or `planner`. Every
    tick, right behind the sensing stage (the sensed or memory call; without a sensor, the plan stage), one
    smpc_repair_plan_batch reads ep.pose, ep.costmap, ep.costmap_origin and, with a plan window, ep.plan_start: a
    robot whose plan runs into impassable cells of its window within repair.radius gets the least-cost detour inside that
    region spliced into ep.plan / ep.plan_len in place (ep.plan_scratch [B,L,2] is the call's workspace), and
    ep.repair_status [B] int32 (enum smpc_repair_status) and ep.repair_info [B,4] int32 (i0, i1, j, m) say what
    happened. The tick's own roll and trajectorizer ran before the scan, so a repaired plan takes effect at the next
    tick's plan stage. The call is part of a captured graph, whose warm-up tick may have spliced a detour in (STATE).
    replan() replaces repaired plans like any other. None: nothing is allocated, nothing is launched and the episode is the
    one without bit for bit."""
    KEY, TIMING = "repair", "repair"
    STATE = ("plan", "plan_len")
    BEFORE = same(repair_plan_before="plan", repair_plan_len_before="plan_len")
    AFTER = same("repair_status", "repair_info", repair_plan_after="plan", repair_plan_len_after="plan_len")

    def check(repair, planned: bool, resolution: float):
        """What BatchEpisode(repair=...) refuses (planned: the episode has plan= or planner=; resolution: the windows')."""
        if not isinstance(repair, PlanRepairParams):
            raise ValueError("repair must be a PlanRepairParams")
        if not planned:
            raise ValueError("repair needs plan= or planner=: there is no plan to repair")
        if not repair.supported(resolution):
            raise ValueError("repair: a radius beyond 63 cells at the windows' resolution, or costs whose potentials do not fit 32 bits")

    def allocate(ep, kw):
        """The plan repair's workspace and what it reports."""
        ep.plan_scratch = ep.torch.zeros_like(ep.plan)
        ep.repair_status = ep._zeros(ep.B, dtype=ep.torch.int32)
        ep.repair_info = ep.torch.full((ep.B, 4), -1, dtype=ep.torch.int32, device=ep.dev)

    def bind(ep):
        ep._c.repair = point(BatchSolver.repair_plan_c(ep.repair, ep.B, int(ep.plan.shape[1]), ep.size_x, ep.size_y, ep.costmap_shared,
                                                       ep.resolution, 1),
                             {"costmap": ep.costmap, "costmap_origin": ep.costmap_origin, "robot_pose": ep.pose,
                              "plan_start": ep.plan_start if ep.plan_window is not None else None})

    def launch(ep):
        ep.solver.repair_plan_device(ep._c.repair, ep.plan.data_ptr(), ep.plan_len.data_ptr(), ep.plan_scratch.data_ptr(),
                                     ep.repair_status.data_ptr(), ep.repair_info.data_ptr())


class ScanPeople(Perception):
    """scan_detector: the controller is handed what its own scan shows of the people (include/smpc_scan_people.h); needs
    `sensor`, with or without `sensor_memory`, and excludes `visibility` and `detector`: those start from the simulator's
    person rows, this starts from the beams, and the two paths are alternatives. Every tick, right behind the sensed (or
    memory) call and in front of the tracker, one smpc_scan_people_batch clusters the cells the tick's beams stopped at
    (ep.beam_kind / ep.beam_cell) into segments and writes the person-sized ones into ep.scan_persons [B,Nd,5]
    (x, y, 0, 0, 0) and ep.scan_count [B] int32, Nd = scan_detector.max_detections, with ep.scan_segment [B,Nd,4] int32
    (start beam, beams, the summed offsets) and ep.scan_stats [B,4] int32 (segments, rejected by points, rejected by
    width, accepted). The tracker reads them, or without one people_to_status does; a detection has no velocity, so
    without a tracker the solve plans around people who stand still: use tracker=TrackerParams(). The crowd, the plant,
    the metrics and the scan itself keep seeing the true persons. It has no state.
    None: nothing is allocated, nothing is launched and the episode is the one without bit for bit."""
    KEY, TIMING = "scan_detector", "scan_people"
    AFTER = same("scan_persons", "scan_count", "scan_segment", "scan_stats")

    def check(scan_detector, sensor, visibility, detector, resolution: float):
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

    def allocate(ep, kw):
        B, Nd = ep.B, int(ep.scan_detector.max_detections)
        ep.scan_persons = ep._zeros(B, Nd, 5)
        ep.scan_count = ep._zeros(B, dtype=ep.torch.int32)
        ep.scan_segment = ep._zeros(B, Nd, 4, dtype=ep.torch.int32)
        ep.scan_stats = ep._zeros(B, 4, dtype=ep.torch.int32)

    def bind(ep, told):  # it starts from the beams, not from what is upstream
        Nd = int(ep.scan_persons.shape[1])
        ep._c.scan_people = point(BatchSolver.scan_people_c(ep.scan_detector, ep.B, int(ep.sensor.n_beams), Nd, 1, ep.resolution,
                                                            world_origin(ep), ep.sensor, ep.sensor_memory),
                                  {"robot_pose": ep.pose, "beam_kind": ep.beam_kind, "beam_cell": ep.beam_cell})
        return Told(ep.scan_persons, ep.scan_count, Nd)

    def launch(ep):
        ep.solver.scan_people_device(ep._c.scan_people, ep.scan_persons.data_ptr(), ep.scan_count.data_ptr(), ep.scan_segment.data_ptr(),
                                     ep.scan_stats.data_ptr())


class Visibility(Perception):
    """visibility: the robots perceive only the persons they have in line of sight on the world map
    (include/smpc_visibility.h): needs `world`. Every tick, after the roll and the plan stage and in front of the other
    perception stages, smpc_visible_people_batch compacts the persons within visibility.max_range whose sight line no
    cell of the world occludes into ep.seen_persons [B,Np,5] / ep.seen_count [B] (with ep.person_seen [B,Np]
    uint8, enum smpc_seen_code), and the next perception stage, or people_to_status, reads those in place of ep.persons /
    ep.person_count. The crowd step, the metrics and the world's move keep the true persons. None: nothing is allocated and
    nothing is launched."""
    KEY, TIMING = "visibility", "visibility"
    AFTER = same("person_seen", "seen_count", "seen_persons")

    def check(visibility, world, resolution):
        if world is None:
            raise ValueError("visibility needs world: the sight lines run over the world map")
        if not visibility.supported(resolution):
            raise ValueError("visibility.max_range / resolution exceeds 32768 cells")

    def allocate(ep, kw):
        B, Np = ep.B, int(ep.persons.shape[1])
        ep.seen_persons = ep._zeros(B, Np, 5)
        ep.seen_count = ep._zeros(B, dtype=ep.torch.int32)
        ep.person_seen = ep._zeros(B, Np, dtype=ep.torch.uint8)

    def bind(ep, told):
        ep._c.visibility = point(BatchSolver.visibility_c(ep.visibility, ep.B, told.Np, ep.world.cells_x, ep.world.cells_y, True,
                                                          ep.resolution, 1),
                                 {"world": ep.world_map, "world_origin": ep.world_origin, "robot_pose": ep.pose,
                                  "people": told.rows, "count": told.count})
        return Told(ep.seen_persons, ep.seen_count, told.Np)

    def launch(ep):
        ep.solver.visible_people_device(ep._c.visibility, ep.seen_persons.data_ptr(), ep.seen_count.data_ptr(), ep.person_seen.data_ptr())


class Detector(Perception):
    """detector: the controller is handed what a detector would report (include/smpc_detector.h). Every tick, behind the
    line-of-sight filter and in front of the tracker, one smpc_detect_people_batch reads ep.seen_persons /
    ep.seen_count with `visibility`, else ep.persons / ep.person_count: persons behind another person's body
    and missed persons leave, the others are reported with range-dependent position noise, clutter is appended, into
    ep.detected_persons [B,Nd,5] / ep.detected_count [B] (ep.detected_source [B,Nd], ep.person_outcome [B,Np]
    uint8), Nd = min(64, Np + detector.clutter_candidates), which the tracker (or, without one, people_to_status)
    reads. The state is ep.draw_state [B,2] int32 (the bits of the call's uint32 words): the robot's stream id
    (its index; set_detector_streams() gives a part of a larger batch the ids of its robots there, as ShardedEpisode
    does) and its tick counter, zero at the start, which lives on the device so that a replayed graph draws fresh
    numbers every tick. The world model, the crowd steps, the scan and the metrics keep reading the true ep.persons.
    None: nothing is allocated, nothing is launched and the episode is the one without bit for bit."""
    KEY, TIMING = "detector", "detector"
    STATE = ("draw_state",)
    BEFORE = same(draw_state_before="draw_state")
    AFTER = same("detected_persons", "detected_count", "detected_source", "person_outcome", draw_state_after="draw_state")

    def check(detector):
        if not isinstance(detector, DetectorParams):
            raise ValueError("detector must be a DetectorParams")
        if not detector.supported():
            raise ValueError("detector: more than 64 clutter candidates")

    def allocate(ep, kw):
        """The draw state of every robot (stream id = its index, counter 0) and what the detector writes every tick."""
        B, Np = ep.B, int(ep.persons.shape[1])
        Nd = min(64, Np + int(ep.detector.clutter_candidates))
        ep.draw_state = ep._zeros(B, 2, dtype=ep.torch.int32)
        ep.draw_state[:, 0] = ep.torch.arange(B, dtype=ep.torch.int32, device=ep.draw_state.device)
        ep.detected_persons = ep._zeros(B, Nd, 5)
        ep.detected_count = ep._zeros(B, dtype=ep.torch.int32)
        ep.detected_source = ep._zeros(B, Nd, dtype=ep.torch.int32)
        ep.person_outcome = ep._zeros(B, Np, dtype=ep.torch.uint8)

    def bind(ep, told):
        Nd = int(ep.detected_persons.shape[1])
        ep._c.detector = point(BatchSolver.detector_c(ep.detector, ep.B, told.Np, Nd, 1),
                               {"people": told.rows, "count": told.count, "robot_pose": ep.pose})
        return Told(ep.detected_persons, ep.detected_count, Nd)

    def launch(ep):
        ep.solver.detect_people_device(ep._c.detector, ep.draw_state.data_ptr(), ep.detected_persons.data_ptr(), ep.detected_count.data_ptr(),
                                       ep.detected_source.data_ptr(), ep.person_outcome.data_ptr())


class Tracker(Perception):
    """tracker: the controller is handed tracks instead of the simulator's rows (include/smpc_tracker.h). Every tick,
    directly in front of people_to_status, one smpc_track_people_batch associates the tick's detections (what the perception
    stage upstream tells on: the detector's or the scan detector's, with `visibility` alone ep.seen_persons / ep.seen_count,
    else ep.persons / ep.person_count; only x and y are read) with
    the robot's tracks, estimates their velocity from positions alone with dt = params.dt, coasts a track whose person
    is not detected for at most tracker.max_missed ticks, and writes the confirmed tracks nearest first into
    ep.tracked_persons [B,Np,5] / ep.tracked_count [B] (ep.tracked_source [B,Np,2]: slot and id), which
    people_to_status reads. The state is ep.tracks [B,slots,4], ep.track_meta [B,slots,4] int32 and
    ep.track_next_id [B] int32, zero at the start (no tracks). The world model, the crowd steps, the scan and the metrics keep
    reading the true ep.persons. None: nothing is allocated, nothing is launched and the episode is the one without
    bit for bit."""
    KEY, TIMING = "tracker", "tracker"
    STATE = ("tracks", "track_meta", "track_next_id")
    BEFORE = same(tracks_before="tracks", track_meta_before="track_meta", track_next_id_before="track_next_id")
    AFTER = same("tracked_persons", "tracked_count", "tracked_source", tracks_after="tracks", track_meta_after="track_meta",
                 track_next_id_after="track_next_id")

    def check(tracker, dt):
        if not isinstance(tracker, TrackerParams):
            raise ValueError("tracker must be a TrackerParams")
        if not tracker.supported(dt):
            raise ValueError("tracker: more than 64 slots, or no finite beta / dt with params.dt")

    def allocate(ep, kw):
        B, Np, Nt = ep.B, int(ep.persons.shape[1]), int(ep.tracker.slots)
        ep.tracks = ep._zeros(B, Nt, 4)
        ep.track_meta = ep._zeros(B, Nt, 4, dtype=ep.torch.int32)
        ep.track_next_id = ep._zeros(B, dtype=ep.torch.int32)
        ep.tracked_persons = ep._zeros(B, Np, 5)
        ep.tracked_count = ep._zeros(B, dtype=ep.torch.int32)
        ep.tracked_source = ep._zeros(B, Np, 2, dtype=ep.torch.int32)

    def bind(ep, told):
        Np = int(ep.persons.shape[1])
        ep._c.tracker = point(BatchSolver.tracker_c(ep.tracker, ep.B, told.Np, Np, ep.params.dt, 1),
                              {"detections": told.rows, "det_count": told.count, "robot_pose": ep.pose})
        return Told(ep.tracked_persons, ep.tracked_count, Np)

    def launch(ep):
        ep.solver.track_people_device(ep._c.tracker, ep.tracks.data_ptr(), ep.track_meta.data_ptr(), ep.track_next_id.data_ptr(),
                                      ep.tracked_persons.data_ptr(), ep.tracked_count.data_ptr(), ep.tracked_source.data_ptr())


class Monitor(Stage):
    """monitor: the selected command passes a collision monitor (include/smpc_collision_monitor.h) before anything executes
    it; needs `sensor`, with or without `sensor_memory`: the monitor reads the tick's scan. Directly behind the command
    selection one smpc_collision_monitor_batch judges ep.cmd_vel at ep.pose against the cells the tick's beams
    stopped at (ep.beam_kind / ep.beam_cell) and writes ep.cmd_safe [B,2], ep.monitor_action [B,4] int32
    (enum smpc_monitor_flag bits, the deciding zone or -1, its collision step or -1, the robot's points),
    ep.monitor_points [B,Z] int32 and ep.monitor_ratio [B]. Everything behind it that took ep.cmd_vel for the
    command being executed takes ep.cmd_safe (ep.executed): the crowd steps, the plant, and without a plant the motion model,
    the next warm start's speed and the metrics' twist; ep.cmd_vel stays the controller's command. Without a plant a robot whose
    command the monitor changed (ratio < 1) is moved by the motion model with the safe command instead of being placed
    on the first optimised pose. It has no state.
    None: nothing is allocated, nothing is launched and the episode is the one without bit for bit."""
    KEY, TIMING = "monitor", "monitor"
    AFTER = same("cmd_safe", "monitor_action", "monitor_points", "monitor_ratio", "monitor_heading_cs", "monitor_step_cs")

    def check(monitor, sensor):
        """What BatchEpisode(monitor=...) refuses (sensor: the episode's)."""
        if not isinstance(monitor, MonitorParams):
            raise ValueError("monitor must be a MonitorParams")
        if sensor is None:
            raise ValueError("monitor needs sensor=SensorParams(...): it reads the scan")
        if not monitor.supported():
            raise ValueError("monitor: more than 8 zones or more than 32 simulation steps")

    def allocate(ep, kw):
        ep.cmd_safe = ep._zeros(ep.B, 2)
        ep.monitor_action = ep._zeros(ep.B, 4, dtype=ep.torch.int32)
        ep.monitor_points = ep._zeros(ep.B, len(ep.monitor.zones), dtype=ep.torch.int32)
        ep.monitor_ratio = ep._zeros(ep.B)
        ep.monitor_heading_cs = ep._zeros(ep.B, 2)
        ep.monitor_step_cs = ep._zeros(ep.B, 2)

    def bind(ep):
        ep._c.monitor = point(BatchSolver.collision_monitor_c(ep.monitor, ep.B, int(ep.sensor.n_beams), 1, ep.resolution, world_origin(ep)),
                              {"robot_pose": ep.pose, "cmd": ep.cmd_vel, "beam_kind": ep.beam_kind, "beam_cell": ep.beam_cell})

    def launch(ep):
        ep.solver.collision_monitor_device(ep._c.monitor, ep.cmd_safe.data_ptr(), ep.monitor_action.data_ptr(), ep.monitor_points.data_ptr(),
                                           ep.monitor_ratio.data_ptr(), ep.monitor_heading_cs.data_ptr(), ep.monitor_step_cs.data_ptr())


class Crowd(Stage):
    """crowd: the persons move as a reactive crowd (smpc_crowd_step_batch, one launch per tick, in place of the
    constant-velocity move): person_waypoints [B,Np,K,2] and person_n_waypoints [B,Np] (e.g. scenes.crowd_waypoints) are
    each person's goals, ep.person_cursor [B,Np] the index of its current one (0 at the start); person_speed [B,Np]:
    desired speeds (default crowd.desired_speed for everybody). The step sees the pose the period started from and the
    command being executed, and the episode's ObstacleDistance grid. None: nothing is allocated and the persons move
    with constant velocity.
    person_groups [B,Np] int32 (with crowd; e.g. scenes.crowd_groups): the persons' group ids (< 0: none); companions
    are held together by the Social Force Model's group force (smpc_crowd_step_groups_batch) with the factors of
    crowd_groups (default CrowdGroupParams()). Uploaded once and constant over the episode. None: nothing is
    allocated and the plain crowd step runs."""
    KEY, ATTR, TIMING = "crowd", "crowd_params", "crowd"
    STATE = ("person_cursor",)
    BEFORE = same(cursor_before="person_cursor")
    AFTER = same(cursor_after="person_cursor")

    def check(crowd, person_waypoints, person_n_waypoints, person_groups):
        if crowd is None:
            if person_groups is not None:
                raise ValueError("person_groups needs crowd=CrowdParams(...)")
            return
        if person_waypoints is None or person_n_waypoints is None:
            raise ValueError("crowd needs person_waypoints [B,Np,K,2] and person_n_waypoints [B,Np]")

    def allocate(ep, kw):
        B, Np, person_speed, person_groups = ep.B, int(ep.persons.shape[1]), kw["person_speed"], kw["person_groups"]
        wp = np.ascontiguousarray(kw["person_waypoints"], np.float64)
        assert wp.ndim == 4 and wp.shape[:2] == (B, Np) and wp.shape[3] == 2, "person_waypoints [B,Np,K,2]"
        assert np.shape(kw["person_n_waypoints"]) == (B, Np), "person_n_waypoints [B,Np]"
        ep.person_wp = ep._upload(wp, np.float64)
        ep.person_nwp = ep._upload(kw["person_n_waypoints"], np.int32)
        ep.person_cursor = ep._zeros(B, Np, dtype=ep.torch.int32)
        ep.person_speed = None
        if person_speed is not None:
            assert np.shape(person_speed) == (B, Np), "person_speed [B,Np]"
            ep.person_speed = ep._upload(person_speed, np.float64)
        if person_groups is not None:
            assert np.shape(person_groups) == (B, Np), "person_groups [B,Np]"
            ep.person_groups = ep._upload(person_groups, np.int32)
            ep.crowd_group_params = kw["crowd_groups"] if kw["crowd_groups"] is not None else CrowdGroupParams()

    def bind(ep):
        c = ep._c
        c.crowd = point(BatchSolver.crowd_c(ep.crowd_params, ep.B, int(ep.persons.shape[1]), int(ep.person_wp.shape[2]), ep.params.dt, 1),
                        {"robot_pose": ep.pose, "robot_twist": ep.executed, "count": ep.person_count,
                         "waypoints": ep.person_wp, "n_waypoints": ep.person_nwp, "desired_speeds": ep.person_speed})
        set_od_grid(c.crowd, "od_indexes", ep.od_indexes, ep.od_origin, ep.od_resolution, (ep.od_shared, ep.od_h, ep.od_w))
        c.groups = None
        if ep.person_groups is not None:
            c.groups = BatchSolver.crowd_groups_c(ep.crowd_group_params, ep.person_groups.data_ptr())

    def launch(ep, groups: bool = True):
        """One crowd period; groups=False: the plain step even when the episode has groups."""
        ep.solver.crowd_step_device(ep._c.crowd, ep.persons.data_ptr(), ep.person_cursor.data_ptr(), ep._c.groups if groups else None)


class PoolCrowd(Stage):
    """pool_crowd: the pool moves as a reactive crowd (include/smpc_crowd_pool.h; needs shared and pool): every period one
    smpc_crowd_pool_step_batch on the bins the tick's gather built (which are then sized for the larger of
    shared.max_range and pool_crowd.interaction_range) takes the constant-velocity move's place: every pedestrian heads
    for its current waypoint of pool_waypoints [M,K,2] / pool_n_waypoints [M] (e.g. scenes.pool_waypoints) and gives way
    to the other pedestrians and, with shared.robots_as_people, to the robots, which it sees at the pose and speed the
    period started from. pool_speed [M]: desired speeds (default pool_crowd.desired_speed for everybody). With an empty
    pool the stage is bound and launched nowhere. None (the other three must be None too): nothing is allocated, nothing is
    launched and the pool walks straight on."""
    KEY, TIMING = "pool_crowd", "pool_crowd"
    STATE = ("pool_cursor",)
    BEFORE = same(pool_cursor_before="pool_cursor")
    AFTER = same("pool_next", pool_cursor_after="pool_cursor")

    def check(pool_crowd, shared, pool, pool_waypoints, pool_n_waypoints, pool_speed):
        if pool_crowd is None:
            named = given(pool_waypoints=pool_waypoints, pool_n_waypoints=pool_n_waypoints, pool_speed=pool_speed)
            if named:
                raise ValueError(f"{named} need pool_crowd=PoolCrowdParams(...)")
            return
        if shared is None or pool is None:
            raise ValueError("pool_crowd needs shared=SharedWorldParams(...) and pool [M,5]")
        if pool_waypoints is None or pool_n_waypoints is None:
            raise ValueError("pool_crowd needs pool_waypoints [M,K,2] and pool_n_waypoints [M]")

    def allocate(ep, kw):
        """What the pool's crowd step reads and writes."""
        M, pool_n_waypoints, pool_speed = ep.M, kw["pool_n_waypoints"], kw["pool_speed"]
        if not ep.od_shared:
            raise ValueError("pool_crowd needs ONE ObstacleDistance grid for the floor (od_indexes [h,w], or obstacles_from_costmap)")
        wp = np.ascontiguousarray(kw["pool_waypoints"], np.float64)
        assert wp.ndim == 3 and wp.shape[0] == M and wp.shape[1] >= 1 and wp.shape[2] == 2, "pool_waypoints [M,K,2]"
        assert np.shape(pool_n_waypoints) == (M,), "pool_n_waypoints [M]"
        ep.pool_wp = ep._upload(wp, np.float64)
        ep.pool_nwp = ep._upload(pool_n_waypoints, np.int32)
        ep.pool_next = ep._zeros(M, 5)
        ep.pool_cursor = ep._zeros(M, dtype=ep.torch.int32)
        ep.pool_speed = None
        if pool_speed is not None:
            assert np.shape(pool_speed) == (M,), "pool_speed [M]"
            ep.pool_speed = ep._upload(pool_speed, np.float64)

    def bind(ep):  # the step reads the bins the tick's gather built: bins_ready
        if ep.M == 0:
            return
        gx, gy, origin, bin_size = ep.shared_grid
        pool = point(BatchSolver.crowd_pool_c(ep.pool_crowd, ep.M, int(ep.agents.shape[0]), int(ep.pool_wp.shape[1]),
                                              ep.params.dt, gx, gy, origin, bin_size, 1, bins_ready=1),
                     {"agents": ep.agents, "waypoints": ep.pool_wp, "n_waypoints": ep.pool_nwp, "desired_speeds": ep.pool_speed, "workspace": ep.nearest_workspace})
        pool.workspace_bytes = int(ep.nearest_workspace.numel())
        if ep.od_indexes is not None and ep.od_shared and ep.od_h * ep.od_w > 0:  # the world's one grid
            point(pool, {"od_indexes": ep.od_indexes, "od_origin": ep.od_origin})
            pool.od_height, pool.od_width, pool.od_resolution = int(ep.od_h), int(ep.od_w), float(ep.od_resolution)
        ep._c.pool = pool

    def launch(ep):
        ep.solver.crowd_pool_step_device(ep._c.pool, ep.pool_next.data_ptr(), ep.pool_cursor.data_ptr())


class Plant(Stage):
    """plant: the command is executed by a model of the base (include/smpc_plant.h) instead of being taken for the motion.
    Every tick, after the command selection and the crowd steps, one smpc_robot_plant_batch takes the place of the torch
    move of pose and speed: the command selected plant.latency_ticks periods ago is clamped to params' velocity bounds,
    limited by plant.max_accel / max_decel / max_ang_accel, and integrated with the motion model (x, y with the old
    heading, then the heading) in plant.substeps steps that end in front of a wall cell of the world map (with `world`;
    else there are no walls) or an agent of the true ep.persons / ep.person_count (with `shared` the other robots
    among them), whatever the controller is told of them. Every robot is moved by the motion model, whether its solve was
    usable or not. ep.speed becomes the executed twist, which the next warm start and the metrics read. The state is
    ep.plant_queue [B,8,2], ep.plant_tick [B] int32 (the bits of the call's uint32 words), zero at the start (at rest, nothing
    under way); ep.plant_contact [B,2] int32 holds each robot's flags (enum smpc_plant_flag) and substeps, ep.heading_cs [B,2]
    the heading's cosine and sine.
    None: nothing is allocated, nothing is launched and the episode is the one without bit for bit."""
    KEY, TIMING = "plant", "plant"
    STATE = ("plant_queue", "plant_tick")
    BEFORE = same(plant_agents="persons", plant_agent_count="person_count", plant_queue_before="plant_queue", plant_tick_before="plant_tick")
    AFTER = same("plant_contact", "heading_cs", plant_queue_after="plant_queue", speed_after="speed", plant_tick_after="plant_tick")

    def check(plant, resolution: float = None):
        """What BatchEpisode(plant=...) refuses (resolution: the world's, None without one)."""
        if not isinstance(plant, PlantParams):
            raise ValueError("plant must be a PlantParams")
        if not plant.supported(resolution):
            raise ValueError("plant: robot_radius beyond 15 cells at the world's resolution")

    def allocate(ep, kw):
        ep.plant_queue = ep._zeros(ep.B, 8, 2)
        ep.plant_tick = ep._zeros(ep.B, dtype=ep.torch.int32)
        ep.plant_contact = ep._zeros(ep.B, 2, dtype=ep.torch.int32)
        ep.heading_cs = ep._zeros(ep.B, 2)

    def bind(ep):
        B, Np = ep.B, int(ep.persons.shape[1])
        if ep.world is not None:
            plant = point(BatchSolver.plant_c(ep.plant, ep.params, B, Np, 1, ep.world.cells_x, ep.world.cells_y, ep.resolution, world_origin(ep)),
                          {"world": ep.world_map})
        else:
            plant = BatchSolver.plant_c(ep.plant, ep.params, B, Np, 1)
        ep._c.plant = point(plant, {"cmd": ep.executed, "agents": ep.persons, "count": ep.person_count})

    def launch(ep):
        ep.solver.robot_plant_device(ep._c.plant, ep.pose.data_ptr(), ep.speed.data_ptr(), ep.plant_queue.data_ptr(),
                                     ep.plant_tick.data_ptr(), ep.plant_contact.data_ptr(), ep.heading_cs.data_ptr())


class Metrics(Stage):
    """metrics: score every robot on the device (smpc_episode_metrics_batch): each tick ends with one sample of the world
    after its move — the new pose, the executed command, the moved persons, the tick's solve status and command source —
    folded into ep.metrics_acc [B,24] (solver.METRIC_COLS; metrics() returns the host copy, solver.summarize_metrics
    the derived values; a captured graph's warm-up sample does not count: STATE). goal [B,2]: where each robot is headed
    (default with global plans: the last pose of each plan; otherwise none, and the goal columns stay unset); a robot's row is
    frozen once it is within metrics.goal_tolerance of it. The clearance columns need the distances of the ObstacleDistance
    grid: with obstacles_from_costmap they are computed along with the indexes, with host-given od_indexes they are fed only
    when od_distances (float32, shaped like od_indexes) is passed too. None: nothing is allocated and nothing is launched."""
    KEY, ATTR, TIMING = "metrics", "metrics_params", "metrics"
    STATE = ("metrics_acc",)
    AFTER = same("metrics_acc")

    def allocate(ep, kw):
        B, goal, plan, plan_len = ep.B, kw["goal"], kw["plan"], kw["plan_len"]
        ep.metrics_acc = ep._zeros(B, 24)  # zero rows: no samples yet
        if goal is None and plan is not None:
            L = np.asarray(plan_len).astype(np.int64)
            goal = np.asarray(plan, np.float64)[np.arange(B), np.maximum(L, 1) - 1]
        ep.goal = None
        if goal is not None:
            assert np.shape(goal) == (B, 2), "goal [B,2]"
            ep.goal = ep._upload(goal, np.float64)

    def bind(ep):
        c = ep._c
        c.metrics = point(BatchSolver.metrics_c(ep.metrics_params, ep.B, int(ep.persons.shape[1]), ep.params.dt, 1),
                          {"robot_pose": ep.pose, "robot_twist": ep.executed if ep.plant is None else ep.speed,  # the twist executed
                           "people": ep.persons, "count": ep.person_count, "goal": ep.goal, "status": ep.res["status"],
                           "source": ep.cmd_source})
        if hasattr(ep, "od_distances"):  # the clearance columns
            set_od_grid(c.metrics, "od_distances", ep.od_distances, ep.od_origin, ep.od_resolution, (ep.od_shared, ep.od_h, ep.od_w))

    def launch(ep):
        ep.solver.episode_metrics_device(ep._c.metrics, ep.metrics_acc.data_ptr())
