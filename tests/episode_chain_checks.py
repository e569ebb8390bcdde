"""The hand-overs of one closed-loop tick (BatchEpisode.tick), stage by stage in launch order: every stage's own yardstick
(tests/*_ref.py; for the stages whose yardstick is the library's host-pointer call, that call) is run on the arrays the
TickRecord holds of the stage that should have produced its input, never on the consuming stage's own view, and held against
what the record holds of the stage's output with the comparison that stage's own test uses: bytes where that test asks for
bytes, the module's own compare / *_close elsewhere. No bound is defined here. Not a test module; imported like
parity_checks.

check_tick(rec, nxt, ep_info) walks one record (nxt: the following one, or None). ep_info is what episode_info() returns: the
episode's constants and `carry`, the only thing check_tick changes: what the yardsticks need of the tick before (the window
cells, and the rows an output buffer keeps beyond its count). It returns the yardsticks' own outputs that say whether the
tick gave every stage work, so that a caller's non-vacuity conditions do not rest on the device."""
import numpy as np

import collision_monitor_ref as CM
import crowd_groups_ref as GR
import crowd_pool_ref as CP
import crowd_ref as CR
import detector_ref as DR
import global_plan_ref as G
import local_costmap_ref as LR
import metrics_ref as MR
import nearest_ref as NR
import obstacle_memory_ref as OM
import plan_repair_ref as PR
import plant_ref
import scan_people_ref as SR
import sensed_costmap_ref as SC
import tracker_ref as TR
import visibility_ref as V
from parity_checks import CMD_TOL
from test_gpu_episode_detector import ref_params as detector_ref_params
from test_gpu_episode_plant import ref_params as plant_ref_params
from test_gpu_episode_scan_people import ref_params as scan_ref_params
from test_gpu_episode_tracker import ref_params as tracker_ref_params

same_bits = V.same_bits


def episode_info(ep, world, kw, prm, presets=None, which=None):
    """The constants of an episode built as BatchEpisode(prm, scenes, w_ref, **kw) on `world`, and an empty carry. presets /
    which: the OptimizerParams the rows of kw["scene_params"] were made of and every robot's index into them (the oracle takes
    one parameter set per call)."""
    info = dict(kw=kw, prm=prm, world=world, solver=ep.solver, B=ep.B, N=ep.N, T=ep.T, Np=int(ep.persons.shape[1]),
                size=(ep.size_x, ep.size_y), res=world.resolution, max_poses=ep.max_poses, presets=presets, which=which,
                od_indexes=ep.od_indexes.cpu().numpy().view(np.uint32), od_origin=ep.od_origin.cpu().numpy().reshape(-1, 2),
                od_resolution=ep.od_resolution, od_distances=ep.od_distances.cpu().numpy() if hasattr(ep, "od_distances") else None,
                goal=ep.goal.cpu().numpy() if kw.get("metrics") is not None and ep.goal is not None else None,
                M=ep.M if kw.get("shared") is not None else 0, carry=None)
    if kw.get("scan_detector") is not None:                                    # the parameters test_gpu_episode_scan_people.ref_params speaks for
        from test_gpu_episode_scan_people import SD
        assert kw["scan_detector"] == SD
    info["carry"] = new_carry(info)
    return info


def new_carry(info):
    """What the first tick of an episode finds: nothing rolled, zero output buffers, an empty metrics table."""
    kw, B, Np, N = info["kw"], info["B"], info["Np"], info["N"]
    c = dict(tick=0, cell=None, metrics=np.zeros((B, MR.NCOLS)), repair_info=np.full((B, 4), -1, np.int32))
    if kw.get("shared") is not None:
        c.update(persons=np.zeros((B, Np, 5)), source=np.full((B, Np), -1, np.int32))
    if kw.get("scan_detector") is not None:
        Nd = int(kw["scan_detector"].max_detections)
        c.update(scan=np.zeros((B, Nd, 5)), scan_segment=np.zeros((B, Nd, 4), np.int32))
    if kw.get("visibility") is not None:
        c.update(seen_persons=np.zeros((B, Np, 5)), person_seen=np.zeros((B, Np), np.uint8))
    if kw.get("detector") is not None:
        Nd = min(64, Np + int(kw["detector"].clutter_candidates))
        c.update(detected=np.zeros((B, Nd, 5)), detected_source=np.zeros((B, Nd), np.int32), outcome=np.zeros((B, Np), np.uint8))
    if kw.get("tracker") is not None:
        c.update(tracked=np.zeros((B, Np, 5)), tracked_source=np.zeros((B, Np, 2), np.int32))
    return c


def monitor_params(mp, world):
    """test_gpu_episode_collision_monitor.ref_params for any MonitorParams: what BatchSolver.collision_monitor_c hands the library."""
    act = {"stop": CM.STOP, "slowdown": CM.SLOWDOWN, "limit": CM.LIMIT, "approach": CM.APPROACH}
    zones = [CM.circle(act[z.action], z.radius, z.min_points, z.slowdown_ratio, z.linear_limit, z.angular_limit) if z.vertices is None else
             CM.polygon(act[z.action], z.vertices, z.min_points, z.slowdown_ratio, z.linear_limit, z.angular_limit) for z in mp.zones]
    return CM.params(zones, M=mp.steps(), sim_dt=mp.simulation_time_step, res=world.resolution, origin=tuple(world.origin))


def _rows(count, n):
    """[B,n] bool: the rows below every robot's count."""
    return np.arange(n)[None, :] < np.clip(count, 0, n)[:, None]


def _same_dict(got, want, what):
    for k in want:
        assert same_bits(got[k], want[k]), (what, k)


def detections_of(r, kw):
    """The rows the tracker (or, without one, people_to_status) was to read, by the record of the stage that wrote them:
    (name, rows, count)."""
    if kw.get("scan_detector") is not None:
        return "scan", r.scan_persons, r.scan_count
    if kw.get("detector") is not None:
        return "detected", r.detected_persons, r.detected_count
    if kw.get("visibility") is not None:
        return "seen", r.seen_persons, r.seen_count
    return "persons", r.persons, r.person_count


def oracle_solve(r, info):
    """The recorded solve against the oracle under the theta := 0 convention, as tests/test_episode.py builds its scenes from a
    record: every scene without a marginal decision within CMD_TOL. Returns the number of firm scenes."""
    from nav2_social_mpc_controller_amd.scenes import SceneBatch
    from oracle import oracle_py as oracle
    oracle.lib()
    prm, B = info["prm"], info["B"]
    presets = info["presets"] or [prm]
    which = info["which"] if info["presets"] else np.zeros(B, int)
    scene = SceneBatch(info["T"], info["N"], prm.dt, r.pose0, r.init_params, r.path_pts, r.goal_yaw, np.ascontiguousarray(r.people_proj),
                       r.has_people, r.sensed_costmap, r.costmap_origin, info["res"], False, r.T_scene)
    firm_scenes = 0
    for k, p in enumerate(presets):
        idx = np.flatnonzero(np.asarray(which) == k)
        if not len(idx):
            continue
        rz = oracle.solve(p, scene.select(idx), nthreads=8, theta_zero_convention=True)
        firm = rz["marginal_decisions"] == 0
        err = np.max(np.abs(r.result["cmds"][idx] - rz["cmds"]).reshape(len(idx), -1), axis=1)
        print("oracle: parameter set", k, "scenes", len(idx), "firm", int(firm.sum()), "worst command error of a firm scene", float(np.max(err[firm], initial=0.0)))
        assert np.max(err[firm], initial=0.0) <= CMD_TOL, (k, idx[firm & (err > CMD_TOL)], float(np.max(err[firm])))
        assert np.array_equal(r.result["status"][idx][firm], rz["status"][firm]), k
        firm_scenes += int(firm.sum())
    return firm_scenes


def check_tick(r, nxt, info, oracle=False):
    """One TickRecord `r` (and what the next one, `nxt`, starts from) against the yardsticks, in launch order. oracle: also hold
    the tick's solve against the oracle. Returns the yardsticks' facts of the tick (see the module docstring)."""
    kw, prm, world, s, c = info["kw"], info["prm"], info["world"], info["solver"], info["carry"]
    B, N, Np, T, M, res = info["B"], info["N"], info["Np"], info["T"], info["M"], info["res"]
    size_x, size_y = info["size"]
    k, dt = c["tick"], prm.dt
    shared, crowd, plant, monitor, sensor = (kw.get(n) is not None for n in ("shared", "crowd", "plant", "monitor", "sensor"))
    memory, tracker, windowed = kw.get("sensor_memory"), kw.get("tracker"), kw.get("plan_window") is not None
    facts = {}

    # -- the roll: the windows follow robot_pose by whole cells from where the tick before left them
    cell, origin, moved, _ = LR.roll(world.origin, res, c["cell"], r.robot_pose, size_x, size_y, force=c["cell"] is None)
    assert same_bits(r.costmap_cell, cell) and same_bits(r.costmap_moved, moved) and same_bits(r.costmap_origin, origin), (k, "roll")
    facts["costmap_moved"] = moved if k > 0 else np.zeros(B, np.int32)          # the first tick writes every window
    c["cell"] = cell

    # -- the shared world's gather: the table's robot rows are this tick's pose and speed, persons the nearest rows of it
    if shared:
        SELF = np.arange(M, M + B, dtype=np.int32)
        assert same_bits(r.agents[M:, 0:2], r.robot_pose[:, 0:2]) and same_bits(r.agents[M:, 4], r.speed[:, 1]), (k, "agents")
        want, n, src = NR.nearest_people(r.agents, r.robot_pose, Np, kw["shared"].max_range, SELF, people=c["persons"], source=c["source"])
        assert same_bits(r.person_count, n) and same_bits(r.persons, want) and same_bits(r.person_source, src), (k, "gather")
        assert not (src[_rows(n, Np)] == SELF[:, None].repeat(Np, 1)[_rows(n, Np)]).any(), (k, "a robot perceives itself")
        c["persons"], c["source"] = want, src
        facts["robots_perceived"] = int((src[_rows(n, Np)] >= M).sum())
    # the true persons of the tick: what the scan, the crowd steps, the plant and the line-of-sight filter are to read
    persons, count = r.persons, r.person_count

    # -- the scan, with or without its memory: the true persons, the window cells of the tick's roll
    if sensor:
        sp = kw["sensor"]
        table, _ = sp.inflation_table(res)
        if memory is not None:
            before = (r.obstacle_memory_before.view(np.uint32), r.obstacle_memory_cell_before)
            cm, kind, hit, (marks, mcell), _ = OM.step(before, world.map, world.origin, res, r.robot_pose, persons, count, r.costmap_cell, size_x, size_y,
                                                       memory.beam_cells(sp, res), sp.agent_d2(res), table, memory.mark_d2(sp, res),
                                                       memory.footprint_d2(res), sp.BASES.index(sp.base), 255, sp.occlusion_min_cost, sp.unknown_occludes)
            assert same_bits(r.obstacle_memory_after.view(np.uint32), marks) and same_bits(mcell, r.costmap_cell), (k, "obstacle memory")
            if nxt is not None:
                assert same_bits(nxt.obstacle_memory_before, r.obstacle_memory_after) and same_bits(nxt.obstacle_memory_cell_before, r.costmap_cell), (k, "memory fed forward")
        else:
            cm, kind, hit = SC.sensed_costmap(world.map, world.origin, res, r.robot_pose, persons, count, r.costmap_cell, size_x, size_y,
                                              sp.beam_cells(res), sp.agent_d2(res), table, sp.BASES.index(sp.base), 255, sp.occlusion_min_cost,
                                              sp.unknown_occludes)
        assert same_bits(r.sensed_costmap, cm) and same_bits(r.beam_kind, kind) and same_bits(r.beam_cell, hit), (k, "scan")
        facts["agent_beams"] = int((kind == SC.AGENT).sum())

    # -- the plan repair: the tick's sensed windows (the memory's when there is one), their origins, plan_start when windowed
    if kw.get("repair") is not None:
        rp = kw["repair"]
        case = dict(costmap=r.sensed_costmap, origin=r.costmap_origin, res=res, pose=r.robot_pose, plan=r.repair_plan_before,
                    plan_len=r.repair_plan_len_before, plan_start=r.plan_start if windowed else None, R=rp.radius_cells(res), stride=rp.stride,
                    clearance_d2=rp.clearance_d2, cost=G.Cost(rp.neutral_cost, rp.cost_weight, rp.lethal_min_cost, rp.allow_unknown))
        want = PR.run(case, info=c["repair_info"], field=False)
        got = dict(plan=r.repair_plan_after, plan_len=r.repair_plan_len_after, status=r.repair_status, info=r.repair_info, field=None)
        assert PR.same(got, want), (k, "repair", [n for n in got if got[n] is not None and got[n].tobytes() != want[n].tobytes()], r.repair_status, want["status"])
        c["repair_info"] = want["info"]
        facts["repaired"] = want["status"] == PR.REPAIRED
        if nxt is not None:                                                     # the next tick's plan stage reads the repaired plans
            assert same_bits(nxt.repair_plan_before, r.repair_plan_after) and same_bits(nxt.repair_plan_len_before, r.repair_plan_len_after), (k, "plans fed forward")
            plan, plan_len = r.repair_plan_after, r.repair_plan_len_after
            if windowed:
                start = r.plan_start.copy()
                w = s.transform_global_plan(plan, plan_len, start, nxt.robot_pose, *kw["plan_window"])
                assert same_bits(w["window_len"], nxt.window_len) and same_bits(start, nxt.plan_start) and same_bits(w["error"], nxt.window_err), (k, "next window")
                assert all(same_bits(w["window"][b, :n], nxt.window[b, :n]) for b, n in enumerate(nxt.window_len)), (k, "next window rows")
                plan, plan_len = w["window"], w["window_len"]
            out = s.trajectorize(kw["traj_params"], plan, plan_len, nxt.robot_pose)
            assert same_bits(out["path"], nxt.plan_path) and same_bits(out["cmds"], nxt.plan_cmds) and same_bits(out["n_poses"], nxt.traj_n_poses), (k, "next trajectory")

    # -- detections from the scan: the tick's beams
    if kw.get("scan_detector") is not None:
        Nd = int(kw["scan_detector"].max_detections)
        want = SR.run(scan_ref_params(world, kw["sensor"]), Nd, r.robot_pose, r.beam_kind, r.beam_cell, c["scan"], c["scan_segment"])
        got = dict(detections=r.scan_persons, det_count=r.scan_count, det_segment=r.scan_segment, seg_stats=r.scan_stats)
        assert SR.same(got, want), (k, "scan people", [n for n in got if got[n].tobytes() != want[n].tobytes()])
        c["scan"], c["scan_segment"] = want["detections"], want["det_segment"]
        facts["scan_count"] = want["det_count"]

    # -- the line-of-sight filter: the true persons
    if kw.get("visibility") is not None:
        vp = kw["visibility"]
        vis, n, seen = V.visible_people(world.map, world.origin, res, r.robot_pose, persons, count, vp.max_range, vp.occlusion_min_cost,
                                        vp.unknown_occludes, visible=c["seen_persons"], seen=c["person_seen"])
        assert same_bits(r.seen_count, n) and same_bits(r.seen_persons, vis) and same_bits(r.person_seen, seen), (k, "visibility")
        c["seen_persons"], c["person_seen"] = vis, seen
        facts["out_of_sight"] = int((np.clip(count, 0, Np) - n).sum())

    # -- the detector: the rows in sight
    if kw.get("detector") is not None:
        dp = kw["detector"]
        people, n = (r.seen_persons, r.seen_count) if kw.get("visibility") is not None else (persons, count)
        new, (det, det_count, source, outcome), counters = DR.step(r.draw_state_before, people, n, r.robot_pose, detector_ref_params(dp, c["detected"].shape[1]),
                                                                    c["detected"], c["detected_source"], c["outcome"])
        for got, want in zip((r.draw_state_after, r.detected_persons, r.detected_count, r.detected_source, r.person_outcome), (new, det, det_count, source, outcome)):
            assert got.dtype == want.dtype and same_bits(got, want), (k, "detector")
        c["detected"], c["detected_source"], c["outcome"] = det, source, outcome
        facts["detected_count"] = det_count
        facts["detector_changed"] = int(counters["missed"].sum() + counters["clutter"].sum())
        if nxt is not None:
            assert same_bits(nxt.draw_state_before, r.draw_state_after), (k, "draw state fed forward")

    # -- the tracker: the last detecting stage's rows
    name, rows, n = detections_of(r, kw)
    if tracker is not None:
        before = (r.tracks_before, r.track_meta_before, r.track_next_id_before)
        new, (people, tcount, source), _ = TR.step(before, rows, n, r.robot_pose, tracker_ref_params(prm, tracker, Np), c["tracked"], c["tracked_source"])
        for got, want in zip((r.tracks_after, r.track_meta_after, r.track_next_id_after, r.tracked_persons, r.tracked_count, r.tracked_source),
                             (*new, people, tcount, source)):
            assert got.dtype == want.dtype and same_bits(got, want), (k, "tracker on " + name)
        c["tracked"], c["tracked_source"] = people, source
        if nxt is not None:
            assert all(same_bits(a, b) for a, b in zip((nxt.tracks_before, nxt.track_meta_before, nxt.track_next_id_before), new)), (k, "tracks fed forward")
        name, rows, n = "tracked", r.tracked_persons, r.tracked_count

    # -- the people filter: the last stage of that chain, the tick's pose and window origins
    fov = {} if kw.get("fov_angle") is None else dict(robot_pose=r.robot_pose, fov_angle=kw["fov_angle"], costmap_origin=r.costmap_origin, size_x=size_x,
                                                      size_y=size_y, resolution=res)
    want, has = s.people_to_status(rows, n, N, **fov)
    assert same_bits(r.init_people, want) and same_bits(r.has_people, has), (k, "people_to_status on " + name)
    facts["people_handed"] = (want[:, :, 3] != -1.0).sum(axis=1) * (has != 0)

    # -- format_to_optimize: the tick's trajectory, the measured twist, the memory the tick before stored
    mem = {n_: v.copy() for n_, v in r.memory_before.items()}
    planned = r.traj_n_poses is not None
    out = s.format_to_optimize(r.plan_path, r.plan_cmds, r.speed, mem, T=T, **(dict(n_poses=r.traj_n_poses, max_poses=info["max_poses"]) if planned else {}))
    assert same_bits(r.T_scene, out["T_scene"]) and same_bits(r.pose0, out["pose0"]) and same_bits(r.goal_yaw, out["goal_yaw"]), (k, "format")
    for b in range(B):                                                          # every robot's own horizon: the rows it has
        Tb = int(r.T_scene[b])
        Pb = prm.dims(Tb, True)[3]
        assert same_bits(r.robot_status[b, :Tb + 1], out["robot_status"][b, :Tb + 1]) and same_bits(r.path_pts[b, :Tb + 1], out["path_pts"][b, :Tb + 1]), (k, "format", b)
        assert same_bits(r.init_params[b, :Pb], out["init_params"][b, :Pb]), (k, "format", b)

    # -- the projection: init_people along the formatted robot path, on the world's grid
    proj, err = s.project_people(r.init_people, r.robot_status, info["od_indexes"], info["od_origin"], info["od_resolution"], prm.max_time, prm.time_step)
    assert same_bits(r.people_proj, proj) and same_bits(r.proj_error, err), (k, "projection")

    # -- the solve, stand-alone on the recorded inputs: the sensed windows and their origins among them
    from nav2_social_mpc_controller_amd.scenes import SceneBatch
    windows = r.sensed_costmap if sensor else r.repair_costmap
    assert windows is not None, "the record holds the solve's windows only with a sensor or the plan repair"
    scene = SceneBatch(T, N, prm.dt, r.pose0, r.init_params, r.path_pts, r.goal_yaw, np.ascontiguousarray(r.people_proj), r.has_people, windows,
                       r.costmap_origin, res, False, r.T_scene if planned else None,
                       scene_params=None if kw.get("scene_params") is None else np.ascontiguousarray(kw["scene_params"], np.float64))
    got = s.solve(scene)
    for n_, v in r.result.items():
        assert same_bits(got[n_], v), (k, "solve", n_, np.flatnonzero([got[n_][b].tobytes() != v[b].tobytes() for b in range(B)]))
    facts["usable"] = r.result["status"] != 2
    if oracle:
        facts["firm_scenes"] = oracle_solve(r, info)

    # -- the memory store: usable solves overwrite the record format left
    s.memory_store(r.result["status"], r.result["path"], r.result["cmds"], mem, r.T_scene if planned else None)
    _same_dict(r.memory_after, mem, (k, "memory store"))
    if nxt is not None:
        _same_dict(nxt.memory_before, r.memory_after, (k, "memory fed forward"))

    # -- the command selection: the solve's first command, or the trajectorizer's
    cmd, source = s.select_command(r.traj_n_poses, r.plan_cmds, r.result["status"], r.result["cmds"], r.window_err if windowed else None)
    assert same_bits(r.cmd_vel, cmd) and same_bits(r.cmd_source, source), (k, "command selection")

    # -- the collision monitor: cmd_vel against the tick's beams; cmd_safe is what everything behind it executes
    executed = r.cmd_vel
    if monitor:
        p = monitor_params(kw["monitor"], world)
        want = CM.run(p, r.robot_pose, r.cmd_vel, r.beam_kind, r.beam_cell, r.monitor_heading_cs, r.monitor_step_cs)
        got = dict(cmd_out=r.cmd_safe, action=r.monitor_action, zone_points=r.monitor_points, ratio=r.monitor_ratio)
        assert CM.same(got, want), (k, "monitor", [n_ for n_ in got if got[n_].tobytes() != want[n_].tobytes()])
        assert CM.angles_close(r.monitor_heading_cs, r.monitor_step_cs, r.robot_pose, r.cmd_vel, p["sim_dt"], p["M"]) and want["finite"].all(), (k, "monitor angles")
        slowed = want["ratio"] < 1.0
        assert same_bits(r.cmd_safe[~slowed], r.cmd_vel[~slowed]), (k, "monitor")
        facts["monitor_slowed"] = slowed
        executed = r.cmd_safe

    # -- the persons' period: the true persons, the pose the period started from, the executed command
    if crowd:
        cp, gp = kw["crowd"], kw.get("crowd_groups")
        od_shared = info["od_indexes"].shape[0] == 1
        args = (dt, persons, r.cursor_before, r.robot_pose, executed, count, kw["person_waypoints"], kw["person_n_waypoints"])
        opts = dict(desired_speeds=kw.get("person_speed"), od_indexes=info["od_indexes"][0] if od_shared else info["od_indexes"],
                    od_origin=info["od_origin"][0] if od_shared else info["od_origin"], od_resolution=info["od_resolution"], goal_radius=cp.goal_radius,
                    person_radius=cp.person_radius, desired_speed=cp.desired_speed, cyclic=cp.cyclic, robot_visible=cp.robot_visible)
        if kw.get("person_groups") is not None:
            from nav2_social_mpc_controller_amd.params import CrowdGroupParams
            gp = gp if gp is not None else CrowdGroupParams()
            want = GR.step_batch(*args, group_id=kw["person_groups"], factors=(gp.factor_gaze, gp.factor_coherence, gp.factor_repulsion), **opts)
            plain = CR.step_batch(*args, **opts)
            facts["group_force"] = float(np.abs(plain[0][..., 2:4] - want[0][..., 2:4])[_rows(count, Np)].max(initial=0.0))
        else:
            want = CR.step_batch(*args, **opts)
        CR.compare(r.persons_after, r.cursor_after, want[0], want[1], dt, count, f"tick {k}: crowd step")
        if nxt is not None:
            assert same_bits(nxt.persons, r.persons_after) and same_bits(nxt.cursor_before, r.cursor_after), (k, "persons fed forward")
    if shared and kw.get("pool_crowd") is not None and M > 0:
        pc = kw["pool_crowd"]
        assert same_bits(r.pool_cursor_before, np.zeros(M, np.int32)) if k == 0 else True, (k, "pool cursor")
        counts = []
        want, cur = CP.step(dt, r.agents, M, r.pool_cursor_before, kw["pool_waypoints"], kw["pool_n_waypoints"], pc.interaction_range,
                            goal_radius=pc.goal_radius, person_radius=pc.person_radius, desired_speed=pc.desired_speed, cyclic=pc.cyclic,
                            desired_speeds=kw.get("pool_speed"), od_indexes=info["od_indexes"][0], od_origin=info["od_origin"][0],
                            od_resolution=info["od_resolution"], counts=counts)
        CP.compare(r.pool_next, r.pool_cursor_after, want, cur, dt, max(counts), f"tick {k}: pool step")
        if nxt is not None:
            assert same_bits(nxt.agents[:M], r.pool_next) and same_bits(nxt.pool_cursor_before, r.pool_cursor_after), (k, "pool fed forward")

    # -- the plant: the executed command, the true persons as the crowd step left them, the twist the tick started with
    persons_end = r.persons_after if crowd else persons                         # a shared world's rows are gathered, not moved
    if plant:
        assert same_bits(r.plant_agents, persons_end) and same_bits(r.plant_agent_count, count), (k, "plant agents")
        before = (r.robot_pose, r.speed, r.plant_queue_before, r.plant_tick_before)
        (pose, twist, queue, ticks), contact, _ = plant_ref.step(before, {"cmd": executed, "agents": persons_end, "count": count},
                                                                 plant_ref_params(kw["plant"], prm, world), r.heading_cs)
        assert same_bits(r.pose_after, pose) and same_bits(r.speed_after, twist) and same_bits(r.plant_queue_after, queue), (k, "plant")
        assert r.plant_tick_after.dtype == np.uint32 and np.array_equal(r.plant_tick_after, ticks), (k, "plant")
        assert r.plant_contact.dtype == np.int32 and np.array_equal(r.plant_contact, contact), (k, "plant")
        assert plant_ref.heading_close(r.heading_cs, before), (k, "plant heading")
        twist_after = r.speed_after
        if nxt is not None:
            assert same_bits(nxt.plant_queue_before, r.plant_queue_after) and same_bits(nxt.plant_tick_before, r.plant_tick_after), (k, "plant state fed forward")
    else:
        twist_after = executed
    if nxt is not None:
        assert same_bits(nxt.robot_pose, r.pose_after) and same_bits(nxt.speed, twist_after), (k, "pose and speed fed forward")

    # -- the metrics sample: the world as the period leaves it (a shared world gathered again from the moved table)
    if kw.get("metrics") is not None:
        people_after, count_after = r.persons_after, count
        if shared:
            if kw.get("pool_crowd") is not None and M > 0:
                assert same_bits(r.agents_after[:M], r.pool_next), (k, "the pool is the step's")
            assert same_bits(r.agents_after[M:, 0:2], r.pose_after[:, 0:2]) and same_bits(r.agents_after[M:, 4], twist_after[:, 1]), (k, "agents after the move")
            people_after, count_after, src = NR.nearest_people(r.agents_after, r.pose_after, Np, kw["shared"].max_range, np.arange(M, M + B, dtype=np.int32),
                                                               people=c["persons"], source=c["source"])
            assert same_bits(r.persons_after, people_after), (k, "second gather")
            c["persons"], c["source"] = people_after, src                       # the buffers the next tick's gather writes into
        grid = None if info["od_distances"] is None else (info["od_distances"][0] if info["od_distances"].shape[0] == 1 else info["od_distances"])
        origin = info["od_origin"][0] if info["od_origin"].shape[0] == 1 else info["od_origin"]
        acc = MR.update(c["metrics"], kw["metrics"], dt, r.pose_after, twist_after, people_after, count_after, info["goal"], grid, origin,
                        info["od_resolution"], r.result["status"], r.cmd_source)
        MR.compare(r.metrics_acc, acc, f"tick {k}")
        c["metrics"] = r.metrics_acc                                            # the table the next sample is folded into
        facts["people_samples"] = acc[:, MR.I["people_samples"]]
    c["tick"] = k + 1
    return facts
