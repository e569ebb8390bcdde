"""Worked example: compare a handful of controller tunings in closed loop, in ONE episode. Every parameter set drives the
same --scenes scenes (same start poses, crowds, costmaps and global plans), as rows set * scenes .. (set + 1) * scenes - 1
of a batch whose solve takes each robot's own critic weights and velocity bounds (params.scene_param_rows ->
BatchEpisode(scene_params=...)); the device scores every robot as it drives (BatchEpisode(metrics=...)), and one line of
summarize_metrics means is printed per set. Nothing but the final [B,24] metrics rows leaves the device.

    python tools/tune_sweep.py [--scenes 256] [--agents 8] [--ticks 200] [--plan-poses 120] [--reactive [--groups]] [--tracker] [--detector] [--plant]
                                [--world-plans [--occlusion [RANGE]] [--shared-crowd M] [--sensed-costmap [--obstacle-memory] [--collision-monitor] [--scan-detector]] [--plan-repair]]

--reactive: the persons are a reactive crowd (BatchEpisode(crowd=CrowdParams()), waypoints from scenes.crowd_waypoints)
instead of walking straight on with constant velocity. --groups (with --reactive): half of the walking persons go in pairs
and triples (scenes.crowd_groups -> BatchEpisode(person_groups=...)): companions share their waypoints and are held
together by the Social Force Model's group force.
--world-plans: the robots drive on one world map (scenes.make_world, 20 m x 20 m) with rolling local costmaps, each to a seeded
goal of its own (scenes.world_goals) along a plan walked down the goal's field (BatchEpisode(world=, planner=, goal=): a pose
every second path cell, pruned by the plan window as the robot advances) instead of along an arc from its start pose.
--occlusion [RANGE] (with --world-plans): the robots perceive only the persons they have in line of sight on that map, within
RANGE metres (default 10; BatchEpisode(visibility=VisibilityParams(max_range=RANGE))): a person behind a pillar or a wall is
not planned around until it steps out. The metrics keep scoring the true persons.
--shared-crowd M (with --world-plans): instead of a private list of persons per robot, one pool of M pedestrians
(scenes.shared_pool) walks that floor and every robot perceives its nearest --agents of them within 10 m, or within RANGE with
--occlusion (BatchEpisode(shared=SharedWorldParams(robots_as_people=False), pool=...)). The sets do not perceive each other's
robots, which start from the same poses, and the pool does not see them either, so every parameter set meets the same
crowd. The metrics score what a robot perceives. With --reactive the pool is a reactive crowd (BatchEpisode(pool_crowd=
PoolCrowdParams()), waypoints from scenes.pool_waypoints): the pedestrians head for their waypoints and give way to each
other within 5 m. --groups with it is refused: the pool's step has no group forces.
--sensed-costmap (with --world-plans): the windows the solve's ObstacleCost critic reads hold what a laser scan from the robot
hits, walls and persons alike, inflated (BatchEpisode(sensor=SensorParams()): 360 beams out to 2.5 m, inflation 0.7 m with
scaling 3.0 and no static layer, the local costmap of the reference's shipped parameter files), in place of the cut of the
pre-inflated world map: the map obstacle_weight has to be tuned against.
--obstacle-memory (with --sensed-costmap): the scan has Nav2's memory (BatchEpisode(sensor_memory=ObstacleMemoryParams()):
a mark stays until a later beam passes its cell, the beams clear out to 3.0 m and mark out to 2.5 m, the cells under the
robot are always free), so a person who steps out of sight leaves lethal cells where last seen, as on the reference's costmap.
--tracker (with or without --world-plans --occlusion): the controller is handed tracks of what it detects instead of the
simulator's own rows (BatchEpisode(tracker=TrackerParams())): velocities estimated from positions alone by an alpha-beta
filter, a new person handed on at the third detection, and a person who steps out of sight coasted on for up to 20 ticks.
The tuning then meets the velocities a deployed tracker would deliver. The metrics keep scoring the true persons.
--detector (with or without --tracker and --world-plans --occlusion): the rows the tracker (or, without one, the controller) is
handed are what a detector would report (BatchEpisode(detector=DetectorParams())): a person behind another person's body is
not reported, one in ten is missed, positions carry 3 cm of noise at the sensor and 23 cm at 10 m, and false detections
appear around the robot. With --tracker the tuning meets a perception a robot has. The metrics keep scoring the true persons.
--plant (with anything above): the command is executed by a model of the base (BatchEpisode(plant=PlantParams())): accelerations
of 2.5 m/s^2 and 3.2 rad/s^2, and a disc of 0.24 m that stops where it would come closer to a wall cell of the world map (with
--world-plans) or to a person it touches, instead of passing through. The velocity bounds are the base set's for every robot.
The collision and time-to-goal columns then describe a robot that exists; a last column counts the robot-ticks of the final
tick that a contact stopped.
--collision-monitor (with --world-plans --sensed-costmap): the selected command passes a collision monitor before it is executed
(BatchEpisode(monitor=MonitorParams.nav2_like(0.24))): a STOP circle just beyond the body, a SLOWDOWN polygon ahead and the
footprint as APPROACH zone over 1.2 s, judged against the cells the tick's scan stopped at. The tuning then meets the safety layer
a deployed controller runs under; a last column is the share of ticks in which the monitor changed the command (ratio < 1).
--scan-detector (with --world-plans --sensed-costmap, without --occlusion and --detector): the persons the controller is handed
are what its own scan shows (BatchEpisode(scan_detector=ScanDetectorParams())): the tick's beam hits clustered into person-sized
segments, so a person half hidden behind another, two persons who merge into one wide blob and the grid's quantisation come
from geometry and not from a noise model. A detection has no velocity: combine with --tracker.
--plan-repair (with --world-plans): every tick a robot whose plan runs into impassable cells of its own window gets the least-cost
detour inside the window spliced into its plan (BatchEpisode(repair=PlanRepairParams())); with --sensed-costmap those cells are
what the scan marked, persons included. Last columns: the share of robot-ticks that ended with each smpc_repair_status.
--smooth-plans (with --world-plans): the plans are smoothed where the planner walks them
(GlobalPlanParams(smoother=PlanSmootherParams()), include/smpc_plan_smoother.h), so the plan window, the trajectorizer and the
path-align critic read relaxed rows instead of the grid walk's staircase. Every run prints the mean path length and the mean
summed heading change of the drive (the metrics' own columns); compare a run with the flag and one without. Last columns: the
mean sweeps per plan and the share of plans with a rejected candidate.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parameter_sets(base):
    """name -> OptimizerParams. The sets may differ only in the values a scene can have of its own (the nine critic weights,
    desired_linear_vel and the velocity bounds: params.SCENE_ROW_FIELDS); scene_param_rows refuses anything else."""
    P = type(base)
    return {
        "readme": base,
        "soc_work_obst_benchmark": P.soc_work_obst_benchmark(),
        "obst_only_benchmark": P.obst_only_benchmark(),
        "social_x4": base.replace(social_weight=4.0 * base.social_weight),
        "slow_0.4": base.replace(desired_linear_vel=0.4, v_max=0.4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--agents", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--plan-poses", type=int, default=120, help="plan length in poses of 0.05 m (120: a 6 m drive)")
    ap.add_argument("--reactive", action="store_true", help="persons react: Social Force Model crowd with seeded waypoints")
    ap.add_argument("--groups", action="store_true", help="with --reactive: half of the walking persons go in pairs and triples")
    ap.add_argument("--world-plans", action="store_true", help="one world map, seeded goals, plans from the world's goal fields")
    ap.add_argument("--occlusion", type=float, nargs="?", const=10.0, default=None, metavar="RANGE",
                    help="with --world-plans: line-of-sight filter of the perceived persons, detector range in metres (default 10)")
    ap.add_argument("--shared-crowd", type=int, default=None, metavar="M",
                    help="with --world-plans: one pool of M pedestrians for all robots instead of a private list each")
    ap.add_argument("--sensed-costmap", action="store_true",
                    help="with --world-plans: the local costmaps are sensed (a scan marks walls and persons, then inflation)")
    ap.add_argument("--obstacle-memory", action="store_true",
                    help="with --sensed-costmap: marks persist until a beam clears them (Nav2's ObstacleLayer)")
    ap.add_argument("--tracker", action="store_true",
                    help="the controller is handed tracks of the detected persons (velocity from positions, coasting when hidden)")
    ap.add_argument("--detector", action="store_true",
                    help="the detections are a detector's: body occlusion, misses, range-dependent noise and clutter")
    ap.add_argument("--collision-monitor", action="store_true",
                    help="the command passes scan-based stop, slowdown and approach zones (needs --world-plans --sensed-costmap)")
    ap.add_argument("--scan-detector", action="store_true",
                    help="the detections are segments of the tick's scan (needs --world-plans --sensed-costmap; excludes --occlusion, --detector)")
    ap.add_argument("--plan-repair", action="store_true",
                    help="plans give way to impassable cells of the robot's window: detours spliced in every tick (needs --world-plans)")
    ap.add_argument("--smooth-plans", action="store_true",
                    help="the global plans are smoothed where the planner walks them (needs --world-plans)")
    ap.add_argument("--plant", action="store_true",
                    help="the command is executed under acceleration limits and stopped by contact with walls and persons")
    a = ap.parse_args()
    if a.collision_monitor and not (a.world_plans and a.sensed_costmap):
        ap.error("--collision-monitor needs --world-plans --sensed-costmap")
    if a.scan_detector and not (a.world_plans and a.sensed_costmap):
        ap.error("--scan-detector needs --world-plans --sensed-costmap")
    if a.scan_detector and (a.occlusion is not None or a.detector):
        ap.error("--scan-detector excludes --occlusion and --detector: the scan-based and the ground-truth path are alternatives")
    if a.plan_repair and not a.world_plans:
        ap.error("--plan-repair needs --world-plans")
    if a.smooth_plans and not a.world_plans:
        ap.error("--smooth-plans needs --world-plans")
    if a.obstacle_memory and not a.sensed_costmap:
        ap.error("--obstacle-memory needs --sensed-costmap")
    if a.sensed_costmap and not a.world_plans:
        ap.error("--sensed-costmap needs --world-plans")
    if a.shared_crowd is not None and not a.world_plans:
        ap.error("--shared-crowd needs --world-plans")
    if a.shared_crowd is not None and a.groups:
        ap.error("--shared-crowd excludes --groups: the pool's crowd step has no group forces")
    if a.groups and not a.reactive:
        ap.error("--groups needs --reactive")
    if a.occlusion is not None and not a.world_plans:
        ap.error("--occlusion needs --world-plans")

    import numpy as np

    from nav2_social_mpc_controller_amd.episode import BatchEpisode, arc_plans
    from nav2_social_mpc_controller_amd.params import (CrowdParams, GlobalPlanParams, MetricsParams, ObstacleMemoryParams, OptimizerParams,
                                                       DetectorParams, MonitorParams, PlanRepairParams, PlanSmootherParams, PlantParams, PoolCrowdParams, ScanDetectorParams, SensorParams, SharedWorldParams, TrackerParams, TrajectorizerParams, VisibilityParams,
                                                       scene_param_rows)
    from nav2_social_mpc_controller_amd.scenes import (crowd_groups, crowd_waypoints, make_scenes, make_world, pool_waypoints, scenes_in_world,
                                                       shared_pool, uniform, world_goals)
    from nav2_social_mpc_controller_amd.solver import METRIC_COLS, summarize_metrics

    prm = OptimizerParams.readme()
    sets = parameter_sets(prm)
    S, n = len(sets), a.scenes
    if a.world_plans:
        world = make_world(400, 400, 0.05)                                  # one 20 m floor for everybody
        one = scenes_in_world(prm, world, n, a.agents, margin=3.0)
    else:
        one = make_scenes(prm, n, a.agents, map_cells=400)                  # 20 m maps: the drive stays inside
    sc = one.select(np.tile(np.arange(n), S))                               # every set sees the same scenes
    w_ref = np.tile((uniform(0x5EED0001, np.arange(n), 6)[:, 0] * 2.0 - 1.0) * 0.6, S)
    if a.world_plans:                                                       # every set drives to the same goals
        plans = dict(world=world, planner=GlobalPlanParams(stride=2, smoother=PlanSmootherParams() if a.smooth_plans else None), goal=np.tile(world_goals(world, one.pose0[:, :2]), (S, 1)),
                     plan_window=(4.0, 10.0))
        if a.occlusion is not None:
            plans["visibility"] = VisibilityParams(max_range=a.occlusion)
        if a.sensed_costmap:
            plans["sensor"] = SensorParams()
            if a.obstacle_memory:
                plans["sensor_memory"] = ObstacleMemoryParams()
        if a.shared_crowd is not None:                                      # one crowd for every set, the same for each
            plans.update(shared=SharedWorldParams(max_range=a.occlusion if a.occlusion is not None else 10.0, robots_as_people=False),
                         pool=shared_pool(world, a.shared_crowd))
            if a.reactive:                                                  # the pool reacts: one launch per tick on the gather's bins
                wp, n_wp = pool_waypoints(world, plans["pool"])
                plans.update(pool_crowd=PoolCrowdParams(), pool_waypoints=wp, pool_n_waypoints=n_wp)
    else:
        plan, plan_len = arc_plans(sc.pose0, 0.1 * w_ref, L=a.plan_poses)
        plans = dict(plan=plan, plan_len=plan_len)
    rows = scene_param_rows(list(sets.values()), np.repeat(np.arange(S), n))
    tp = TrajectorizerParams(desired_linear_vel=prm.desired_linear_vel, max_time=prm.max_time, time_step=prm.time_step)
    crowd = {}
    if a.reactive and a.shared_crowd is None:
        wp, n_wp = crowd_waypoints(one)                                     # every set meets the same crowd
        if a.groups:
            gid, wp, n_wp = crowd_groups(one)
            crowd["person_groups"] = np.tile(gid, (S, 1))
        crowd.update(crowd=CrowdParams(), person_waypoints=np.tile(wp, (S, 1, 1, 1)), person_n_waypoints=np.tile(n_wp, (S, 1)))
    if a.tracker:
        plans["tracker"] = TrackerParams(slots=max(16, min(64, 2 * a.agents)))
    if a.detector:
        plans["detector"] = DetectorParams(clutter_candidates=min(2, 64 - a.agents))
    if a.scan_detector:
        plans["scan_detector"] = ScanDetectorParams()
    if a.plan_repair:
        plans["repair"] = PlanRepairParams()
    if a.plant:
        plans["plant"] = PlantParams()
    if a.collision_monitor:
        plans["monitor"] = MonitorParams.nav2_like(0.24)
    ep = BatchEpisode(prm, sc, w_ref, traj_params=tp, fov_angle=np.pi / 4, obstacles_from_costmap=True, scene_params=rows,
                      metrics=MetricsParams(), **plans, **crowd)
    ep.capture_graph()
    changed = ep.torch.zeros(S * n, dtype=ep.torch.int64, device=ep.dev)   # ticks in which the monitor changed the robot's command
    n_status = 8                                                            # enum smpc_repair_status
    repair = ep.torch.zeros(S * n, n_status, dtype=ep.torch.int64, device=ep.dev)   # robot-ticks that ended with each status
    for _ in range(a.ticks):
        ep.replay()
        if a.plan_repair:
            with ep.torch.cuda.stream(ep.gstream):
                repair.scatter_add_(1, ep.repair_status.long()[:, None], ep.torch.ones_like(repair[:, :1]))
        if a.collision_monitor:
            with ep.torch.cuda.stream(ep.gstream):   # behind the tick, on its stream: nothing leaves the device
                changed += ep.monitor_ratio < 1.0
    acc = ep.metrics()
    m = summarize_metrics(acc, prm.dt)
    m["heading_change"] = acc[:, METRIC_COLS.index("heading_change")]
    smooth_info = ep.smooth_info.cpu().numpy() if a.smooth_plans else np.zeros((S * n, 4), np.int32)
    changed = changed.cpu().numpy()
    repair = repair.cpu().numpy()
    from nav2_social_mpc_controller_amd._abi_plan_repair import REPAIR_STATUS
    print(f"{S} parameter sets x {n} scenes, {a.agents} agents, {a.ticks} ticks of {prm.dt} s")
    stopped = (ep.plant_contact[:, 0].cpu().numpy() & 3) != 0 if a.plant else np.zeros(S * n, bool)
    for k, name in enumerate(sets):
        sl = slice(k * n, (k + 1) * n)
        mean = lambda key: float(np.nanmean(m[key][sl])) if np.isfinite(m[key][sl]).any() else float("nan")
        print(f"{name:24s} success {m['success'][sl].mean():.3f}  time_to_goal {mean('time_to_goal'):6.2f} s  "
              f"mean_speed {mean('mean_speed'):.3f}  mean_min_person_dist {mean('mean_min_person_dist'):.3f}  "
              f"intimate {mean('intimate_share'):.3f}  personal {mean('personal_share'):.3f}  "
              f"social_work/m {mean('social_work_per_metre'):8.3f}  person_coll {m['person_collision'][sl].mean():.3f}  "
              f"obstacle_coll {m['obstacle_collision'][sl].mean():.3f}  fallback {mean('fallback_share'):.3f}  "
              f"path_length {mean('path_length'):6.3f} m  heading_change {mean('heading_change'):6.3f} rad"
              + (f"  smooth_sweeps {smooth_info[sl, 0].mean():.1f}  smooth_rejecting {(smooth_info[sl, 2] > 0).mean():.3f}" if a.smooth_plans else "")
              + (f"  stopped_by_contact {stopped[sl].mean():.3f}" if a.plant else "")
              + (f"  monitor_share {changed[sl].mean() / max(a.ticks, 1):.3f}" if a.collision_monitor else "")
              + ("".join(f"  {REPAIR_STATUS[i].lower()} {repair[sl, i].sum() / max(a.ticks * n, 1):.3f}" for i in range(n_status)) if a.plan_repair else ""))


if __name__ == "__main__":
    main()
