"""Closed-loop batch episodes (nav2_social_mpc_controller_amd/episode.py): every tick chains the device versions of
format_to_optimize (f2), project_people (f1) and the solve (a1-a12), then stores the TrajectoryMemory. Each stage of each
tick is replayed on the CPU from the inputs the device saw (teacher forcing, so errors do not compound over ticks)."""
import numpy as np
import pytest

CMD_TOL = 1e-5  # north_star tolerance on the optimised command sequence


@pytest.mark.gpu
def test_episode_ticks_match_cpu_chain(oracle):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    from nav2_social_mpc_controller_amd.scenes import SceneBatch, make_scenes, uniform
    from oracle import pyref_format, pyref_sfm

    prm = OptimizerParams.readme()
    B, N = 48, 3
    sc = make_scenes(prm, B, N, n_valid=2)
    T = sc.T
    CH, bl, nb, P, M, _ = prm.dims(T, True)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    cells, res, origin = 480, float(np.float32(0.1)), np.array([-16.0, -16.0])
    od_idx = np.zeros((cells, cells), np.uint32)
    ep = BatchEpisode(prm, sc, w_ref, od_idx, origin, res)
    od = dict(width=cells, height=cells, resolution=res, origin_x=origin[0], origin_y=origin[1], indexes=od_idx)
    n_checked = 0
    for tick in range(3):
        r = ep.tick(record=True)
        # the command handed to the robot: cmds[0] of the solve (no fallback is active in these scenes)
        assert (ep.cmd_source.cpu().numpy() == 0).all() and np.array_equal(ep.cmd_vel.cpu().numpy(), r.result["cmds"][:, 0])
        # --- f2: people_to_status (no field-of-view filter in this episode)
        st, has = pyref_format.people_to_status(r.persons, r.person_count, N)
        assert np.max(np.abs(r.init_people - st)) <= 1e-14 and np.array_equal(r.has_people, has)
        # --- f2: format_to_optimize + memory initialisation
        mem = {k: v.copy() for k, v in r.memory_before.items()}
        exp = pyref_format.format_to_optimize(r.plan_path, r.plan_cmds, r.speed, mem, prm.current_path_weight,
                                              prm.current_cmds_weight, prm.time_step, nb)
        for k in ("robot_status", "pose0", "init_params", "path_pts", "goal_yaw"):
            err = np.abs(getattr(r, k) - exp[k])
            err = np.minimum(err, np.abs(err - 2 * np.pi))
            assert np.max(err) <= 1e-13, (tick, k)
        assert (r.memory_before["valid"] == (0 if tick == 0 else 1)).all()
        assert (r.T_scene == T).all()   # no global plans: every robot has the batch's horizon
        # --- f1: project_people from the formatted robot status (a few scenes: the numpy restatement is slow)
        assert (r.proj_error == 0).all()
        for s in range(0, B, 12):
            pp = pyref_sfm.project_people(r.init_people[s], r.robot_status[s], od, prm.max_time, prm.time_step,
                                          theta_zero_convention=True)          # [T+1][N][6]
            got = r.people_proj[s].transpose(0, 2, 1)                           # [T+1][6][N] -> [T+1][N][6]
            assert np.max(np.abs(got - pp)) <= 1e-9, (tick, s)
        # --- a1-a12: the solve on exactly the inputs the device assembled
        scene = SceneBatch(T, N, prm.dt, r.pose0, r.init_params, r.path_pts, r.goal_yaw,
                           np.ascontiguousarray(r.people_proj), r.has_people, sc.costmap, sc.costmap_origin,
                           sc.resolution, False)
        rz = oracle.solve(prm, scene, nthreads=8, theta_zero_convention=True)
        firm = rz["marginal_decisions"] == 0
        assert firm.mean() >= 0.8
        err = np.max(np.abs(r.result["cmds"] - rz["cmds"]).reshape(B, -1), axis=1)
        assert np.max(err[firm]) <= CMD_TOL, (tick, float(np.max(err[firm])))
        assert np.array_equal(r.result["status"][firm], rz["status"][firm])
        n_checked += int(firm.sum())
        # --- memory store: usable solves overwrite their record with the optimised path / cmds
        ok = r.result["status"] != 2
        assert np.array_equal(r.memory_after["prev_path"][ok], r.result["path"][ok])
        assert np.array_equal(r.memory_after["prev_cmds"][ok], r.result["cmds"][ok])
        assert (r.memory_after["valid"] == 1).all()
    assert n_checked >= 100
    # the robots actually moved: closed loop, not three solves of the same scene
    assert np.max(np.abs(ep.pose.cpu().numpy()[:, :2] - sc.pose0[:, :2])) > 0.02


@pytest.mark.gpu
def test_episode_with_trajectorizer_matches_cpu_chain(oracle):
    """Plan mode: trajectorize (f3) -> format (f2, cut to T + 1 of the max_steps + 1 poses) -> project (f1) -> solve."""
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, arc_plans
    from nav2_social_mpc_controller_amd.params import OptimizerParams, TrajectorizerParams
    from nav2_social_mpc_controller_amd.scenes import SceneBatch, make_scenes, uniform
    from oracle import pyref_format, pyref_trajectorize

    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    B, N = 32, 3
    sc = make_scenes(prm, B, N, n_valid=2)
    T = sc.T + 1                                                   # plan mode: sized for a path of exactly max_poses poses
    max_poses = tp.max_steps
    assert T == max_poses - 1 and prm.rollout_steps == max_poses - 2
    CH, bl, nb, P, M, _ = prm.dims(T, True)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)  # radius >= 4.2 m: the 20 m arc never closes on itself
    fov = 1.2  # wider than the reference default (pi/4) so that a good share of the scenes keeps somebody in view
    ep = BatchEpisode(prm, sc, w_ref, np.zeros((480, 480), np.uint32), np.array([-16.0, -16.0]), float(np.float32(0.1)),
                      plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=fov)
    seen = 0
    for tick in range(3):
        r = ep.tick(record=True)
        # the command handed to the robot: cmds[0] of the solve (no fallback is active in these scenes)
        assert (ep.cmd_source.cpu().numpy() == 0).all() and np.array_equal(ep.cmd_vel.cpu().numpy(), r.result["cmds"][:, 0])
        assert (r.traj_n_poses == tp.max_steps + 1).all()
        # f4 / f2: field-of-view filter + people_to_status from the world people and the pose the tick started from
        for s in range(B):
            keep = pyref_format.fov_filter(r.persons[s], r.person_count[s], r.robot_pose[s], fov, sc.costmap_origin[s],
                                           sc.size_x, sc.size_y, sc.resolution)
            sel = r.persons[s][keep][None] if keep else np.zeros((1, 1, 5))
            st, has = pyref_format.people_to_status(sel, np.array([len(keep)]), N)
            assert np.max(np.abs(r.init_people[s] - st[0])) <= 1e-14 and r.has_people[s] == has[0], (tick, s)
            seen += len(keep)
        for s in range(0, B, 5):  # f3 on the pose the tick started from
            p, c, err = pyref_trajectorize.trajectorize(plan[s], r.robot_pose[s], tp.omnidirectional, tp.desired_linear_vel,
                                                        tp.lookahead_dist, tp.max_angular_vel, tp.time_step, tp.max_time)
            assert err == 0
            dyaw = np.abs(r.plan_path[s, :, 2] - p[:, 2])
            assert np.max(np.abs(r.plan_path[s, :, :2] - p[:, :2])) <= 1e-11 and np.max(np.minimum(dyaw, np.abs(dyaw - 2 * np.pi))) <= 1e-11
            assert np.max(np.abs(r.plan_cmds[s, :-1] - c[:, [0, 2]])) <= 1e-11
        mem = {k: v.copy() for k, v in r.memory_before.items()}
        exp = pyref_format.format_to_optimize(r.plan_path, r.plan_cmds, r.speed, mem, prm.current_path_weight,
                                              prm.current_cmds_weight, prm.time_step, nb, n_poses=r.traj_n_poses,
                                              max_poses=max_poses, T=T)
        for k in ("robot_status", "pose0", "init_params", "path_pts", "goal_yaw"):
            err = np.abs(getattr(r, k) - exp[k])
            assert np.max(np.minimum(err, np.abs(err - 2 * np.pi))) <= 1e-13, (tick, k)
        # full-length paths (max_steps + 1 poses) are cut to max_poses - 1 poses: the horizon of README's T = 28
        assert np.array_equal(r.T_scene, exp["T_scene"]) and (r.T_scene == prm.rollout_steps).all()
        scene = SceneBatch(T, N, prm.dt, r.pose0, r.init_params, r.path_pts, r.goal_yaw,
                           np.ascontiguousarray(r.people_proj), r.has_people, sc.costmap, sc.costmap_origin,
                           sc.resolution, False, r.T_scene)
        rz = oracle.solve(prm, scene, nthreads=8, theta_zero_convention=True)
        firm = rz["marginal_decisions"] == 0
        err = np.max(np.abs(r.result["cmds"] - rz["cmds"]).reshape(B, -1), axis=1)
        assert firm.mean() >= 0.8 and np.max(err[firm]) <= CMD_TOL, (tick, float(np.max(err[firm])))
    assert np.max(np.abs(ep.pose.cpu().numpy()[:, :2] - sc.pose0[:, :2])) > 0.02
    assert 0 < seen < 3 * B * 2   # the filter kept some persons and dropped some


@pytest.mark.gpu
def test_short_plans_are_solved_on_their_own_horizon_and_reach_the_goal(oracle):
    """The reference solves whatever horizon the tick produces (T = optim_velocities.size(), src/optimizer.cpp:237,
    248-249) and falls back only when the solve is unusable (src/social_mpc_controller.cpp:241-245): a robot whose
    trajectorized path ends inside the batch's horizon is solved with its own T_b, and keeps driving on MPC commands
    until the trajectorizer stops producing steps at the goal."""
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, arc_plans
    from nav2_social_mpc_controller_amd.params import OptimizerParams, TrajectorizerParams
    from nav2_social_mpc_controller_amd.scenes import SceneBatch, make_scenes, uniform
    from oracle import pyref_format

    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    B, N = 32, 3
    sc = make_scenes(prm, B, N, n_valid=2)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    long_plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    short = np.arange(B) % 2 == 1
    plan_len = np.where(short, 12, plan_len).astype(np.int32)     # 12 poses x 0.05 m = 0.55 m: reached in < T steps
    ep = BatchEpisode(prm, sc, w_ref, np.zeros((480, 480), np.uint32), np.array([-16.0, -16.0]), float(np.float32(0.1)),
                      plan=long_plan, plan_len=plan_len, traj_params=tp, fov_angle=1.2)
    T, max_poses = ep.T, tp.max_steps
    nb = prm.dims(T, True)[2]
    goal = long_plan[np.arange(B), plan_len - 1]
    d0 = np.hypot(*(sc.pose0[:, :2] - goal).T)
    dmin = d0.copy()
    horizons = []
    for tick in range(30):
        r = ep.tick(record=True)
        src = ep.cmd_source.cpu().numpy()
        assert (src == 0).all(), (tick, src)                       # MPC commands all the way, for short paths too
        assert (r.result["status"] != 2).all()
        assert np.array_equal(ep.cmd_vel.cpu().numpy(), r.result["cmds"][:, 0])
        mem = {k: v.copy() for k, v in r.memory_before.items()}
        exp = pyref_format.format_to_optimize(r.plan_path, r.plan_cmds, r.speed, mem, prm.current_path_weight,
                                              prm.current_cmds_weight, prm.time_step, nb, n_poses=r.traj_n_poses,
                                              max_poses=max_poses, T=T)
        assert np.array_equal(r.T_scene, exp["T_scene"])
        assert (r.T_scene[~short] == prm.rollout_steps).all() and r.T_scene.min() >= 1
        # on its way to the goal a short-plan robot has a short horizon (once it has arrived the goal checker of the
        # controller server would stop calling the plugin; here the loop just keeps ticking)
        d = np.hypot(*(r.robot_pose[:, :2] - goal).T)
        on_the_way = short & (d > 0.3) & (dmin > 0.3)
        assert (r.T_scene[on_the_way] < prm.rollout_steps).all(), (tick, r.T_scene[on_the_way])
        dmin = np.minimum(dmin, d)
        horizons.append(np.where(on_the_way, r.T_scene, -1))
        if tick in (0, 7, 15, 29):   # the solve of every robot against the oracle run with the robot's own horizon
            scene = SceneBatch(T, N, prm.dt, r.pose0, r.init_params, r.path_pts, r.goal_yaw,
                               np.ascontiguousarray(r.people_proj), r.has_people, sc.costmap, sc.costmap_origin,
                               sc.resolution, False, r.T_scene)
            rz = oracle.solve(prm, scene, nthreads=8, theta_zero_convention=True)
            firm = rz["marginal_decisions"] == 0
            err = np.max(np.abs(r.result["cmds"] - rz["cmds"]).reshape(B, -1), axis=1)
            # (short horizons end on tiny costs, where many decisions sit inside the rounding noise the oracle flags)
            assert firm.mean() >= 0.5 and np.max(err[firm]) <= CMD_TOL, (tick, float(firm.mean()), float(np.max(err[firm])))
            assert np.array_equal(r.result["iterations"][firm], rz["iterations"][firm])
            assert (r.result["status"][~firm] != 2).all()
        # the record of a usable solve holds T_b + 1 poses and commands
        assert np.array_equal(r.memory_after["length"], np.stack([r.T_scene + 1, r.T_scene + 1], axis=1))
    horizons = np.array(horizons)
    assert (horizons[0][short] > 1).all()
    # the trajectorizer stops within 0.2 m of the plan's end (src/path_trajectorizer.cpp:150-152): the robots that the MPC
    # lets drive (one that stands beside a person may wait there for the whole test) arrive on optimised commands, and
    # their horizon shrinks on the way
    arrived = short & (dmin < 0.3)
    assert arrived.sum() >= 0.6 * short.sum(), (int(arrived.sum()), dmin[short])
    for b in np.where(arrived)[0]:
        h = horizons[:, b][horizons[:, b] >= 0]
        assert len(h) >= 3 and h[-1] < h[0], (b, h)


@pytest.mark.gpu
def test_sharded_episode_equals_the_single_chain():
    """The robots of a batch do not interact: four shards on four HIP streams must return, robot by robot, the very
    numbers of the one-stream episode (three ticks, people + global plans + field-of-view filter)."""
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode, arc_plans
    from nav2_social_mpc_controller_amd.params import OptimizerParams, TrajectorizerParams
    from nav2_social_mpc_controller_amd.scenes import make_scenes, uniform

    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    B, N = 203, 8   # not a multiple of the shard count
    sc = make_scenes(prm, B, N)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    od = (np.zeros((480, 480), np.uint32), np.array([-16.0, -16.0]), float(np.float32(0.1)))
    kw = dict(plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=2.0, plan_window=(4.0, 10.0))  # pruning state included
    one = BatchEpisode(prm, sc, w_ref, *od, **kw)
    four = ShardedEpisode(prm, sc, w_ref, *od, shards=4, graphs=True, **kw)  # every shard's tick replayed from a HIP graph
    assert [p.B for p in four.parts] == [50, 51, 51, 51]
    for _ in range(3):
        one.tick()
        four.tick()
    one.synchronize()
    for name in ("status", "iterations", "cmds", "path", "final_cost"):
        assert np.array_equal(one.res[name].cpu().numpy(), four.gather(name).cpu().numpy()), name
    for name in ("pose", "cmd_vel", "cmd_source", "proj_error", "plan_start", "window_len"):
        assert np.array_equal(getattr(one, name).cpu().numpy(), four.gather(name).cpu().numpy()), name
    # a shard can still be ticked outside its graph (recording / per-stage timing): same numbers again
    one.tick()
    r = four.parts[1].tick(record=True)
    one.synchronize()
    sl = four.slices[1]
    assert np.array_equal(r.result["cmds"], one.res["cmds"].cpu().numpy()[sl])


@pytest.mark.gpu
def test_episode_with_the_plan_window_of_the_path_handler():
    """computeVelocityCommands' order (src/social_mpc_controller.cpp:171-180): transformGlobalPlan, then trajectorize on
    the window. Replayed on the CPU from what the device saw: window and pruning against pyref_path_handler, the
    trajectorized path against pyref_trajectorize on that window."""
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, arc_plans
    from nav2_social_mpc_controller_amd.params import OptimizerParams, TrajectorizerParams
    from nav2_social_mpc_controller_amd.scenes import make_scenes, uniform
    from oracle import pyref_path_handler, pyref_trajectorize

    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    B, N = 24, 3
    sc = make_scenes(prm, B, N, n_valid=2)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    plan_len = plan_len.copy()
    lost = np.zeros(B, bool)
    lost[[5, 17]] = True
    plan_len[5] = 0                  # "Received plan with zero length" (src/path_handler.cpp:44-47)
    plan[17] += 40.0                 # a plan far from the robot: "Resulting plan has 0 poses in it." (:100-103)
    search, thr = 2.0, 3.0
    ep = BatchEpisode(prm, sc, w_ref, np.zeros((480, 480), np.uint32), np.array([-16.0, -16.0]), float(np.float32(0.1)),
                      plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=1.2, plan_window=(search, thr))
    start = np.zeros(B, np.int32)
    pose_lost = sc.pose0[lost].copy()
    for tick in range(8):
        r = ep.tick(record=True)
        # a robot whose transformGlobalPlan throws gets NO command in that cycle (the exception leaves
        # computeVelocityCommands before the trajectorizer and its 0.1 m/s fallback): source 3, it does not move
        src = ep.cmd_source.cpu().numpy()
        assert (r.window_err[lost] != 0).all() and (r.window_err[~lost] == 0).all()
        assert (src[lost] == 3).all() and not ep.cmd_vel.cpu().numpy()[lost].any()
        assert np.array_equal(ep.pose.cpu().numpy()[lost], pose_lost)
        for s in np.where(~lost)[0]:
            win, ns, err = pyref_path_handler.transform_global_plan(plan[s, :plan_len[s]], int(start[s]), r.robot_pose[s], search, thr)
            assert err == 0 and r.plan_start[s] == ns and r.window_len[s] == len(win), (tick, s)
            assert np.array_equal(r.window[s, :len(win)], win)
            if s % 4 == 0:
                p, c, terr = pyref_trajectorize.trajectorize(win, r.robot_pose[s], tp.omnidirectional, tp.desired_linear_vel,
                                                             tp.lookahead_dist, tp.max_angular_vel, tp.time_step, tp.max_time)
                assert terr == 0 and r.traj_n_poses[s] == p.shape[0]
                assert np.max(np.abs(r.plan_path[s, :p.shape[0], :2] - p[:, :2])) <= 1e-11
        start = r.plan_start.copy()
        assert (src[~lost] == 0).all()
    assert start.max() >= 1 and (r.window_len[~lost] < plan_len[~lost]).all()   # the plans were pruned and clipped


@pytest.mark.gpu
def test_concurrent_streams_returns_distinct_streams():
    import torch

    from nav2_social_mpc_controller_amd.episode import concurrent_streams
    for n in (1, 3, 4):
        st = concurrent_streams(n, "cuda:0")
        assert len(st) == n and len({s.cuda_stream for s in st}) == n
        assert all(s.cuda_stream != torch.cuda.default_stream("cuda:0").cuda_stream for s in st)


# ---- what a shard gets of the episode's arguments ---------------------------------------------------------------------
def test_every_episode_argument_is_declared_per_robot_or_forwarded():
    """ShardedEpisode hands BatchEpisode's keyword arguments on by declaration (episode.shard_kwargs): every one of them is
    declared per robot, per grid or forwarded, so a new argument that is declared nowhere fails here, not on a GPU. Arrays
    whose row i holds the value i come back as exactly the rows of the shard; everything else is the very same object."""
    import inspect

    from nav2_social_mpc_controller_amd.episode import BatchEpisode, shard_kwargs

    E = BatchEpisode
    sig = inspect.signature(E.__init__).parameters
    keywords = [n for n, p in sig.items() if p.default is not inspect.Parameter.empty]
    declared = E.PER_ROBOT + E.PER_GRID + E.FORWARDED
    assert [n for n in sig if n not in keywords] == ["self", "params", "scenes", "w_ref"]
    assert len(set(declared)) == len(declared) and sorted(declared) == sorted(keywords)
    assert sorted(E.PER_ROBOT) == sorted(("plan", "plan_len", "scene_params", "goal", "person_waypoints", "person_n_waypoints",
                                          "person_speed", "person_groups"))
    assert E.PER_GRID == ("od_indexes", "od_origin", "od_distances")

    B, idx = 7, np.array([2, 3, 4])

    def rows(*tail):  # [B, *tail], row i filled with i
        return np.broadcast_to(np.arange(B).reshape((B,) + (1,) * len(tail)), (B,) + tail).copy()

    tails = dict(plan=(9, 2), plan_len=(), scene_params=(14,), goal=(2,), person_waypoints=(3, 2, 2), person_n_waypoints=(3,),
                 person_speed=(3,), person_groups=(3,))
    per_robot = {k: rows(*tails[k]) for k in E.PER_ROBOT}
    forwarded = {k: object() for k in E.FORWARDED}
    shared = dict(od_indexes=np.zeros((4, 5), np.uint32), od_origin=np.zeros(2), od_distances=np.zeros((4, 5), np.float32))
    per_scene = dict(od_indexes=rows(4, 5).astype(np.uint32), od_origin=rows(2).astype(np.float64), od_distances=rows(4, 5).astype(np.float32))
    one = dict(od_indexes=np.zeros((1, 4, 5), np.uint32), od_origin=np.zeros((1, 2)), od_distances=None)  # [1,h,w]: shared
    for grid, sliced in ((shared, False), (per_scene, True), (one, False)):
        kwargs = dict(per_robot, **forwarded, **grid)
        got = shard_kwargs(kwargs, idx, B)
        assert sorted(got) == sorted(kwargs)
        for k in E.PER_ROBOT + (E.PER_GRID if sliced else ()):
            assert got[k].shape == (3,) + kwargs[k].shape[1:] and got[k].dtype == kwargs[k].dtype, k
            assert all((got[k][j] == i).all() for j, i in enumerate(idx)), k
        for k in E.FORWARDED + (() if sliced else E.PER_GRID):
            assert got[k] is kwargs[k], k
    none = shard_kwargs(dict.fromkeys(declared), idx, B)     # nothing given: nothing to slice
    assert sorted(none) == sorted(declared) and all(v is None for v in none.values())
    with pytest.raises(TypeError, match="per_robot_extra"):
        shard_kwargs(dict(per_robot, per_robot_extra=rows(2)), idx, B)
    with pytest.raises(AssertionError, match="person_speed"):
        shard_kwargs(dict(per_robot, person_speed=rows(3)[:5]), idx, B)


def _every_option(B, N):
    """(params, scenes, w_ref, keyword arguments) of an episode with every optional argument at once, every per-robot
    array with a different row per robot."""
    from nav2_social_mpc_controller_amd import _abi
    from nav2_social_mpc_controller_amd.episode import arc_plans
    from nav2_social_mpc_controller_amd.params import CrowdGroupParams, CrowdParams, MetricsParams, OptimizerParams, TrajectorizerParams
    from nav2_social_mpc_controller_amd.scenes import crowd_groups, make_scenes, uniform

    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    sc = make_scenes(prm, B, N, map_cells=80, standing_fraction=0.0)
    assert not sc.costmap_shared and len({c.tobytes() for c in sc.costmap}) == B      # a costmap (so a grid) per scene
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    plan_len = (plan_len - 10 * np.arange(B)).astype(np.int32)
    gid, wp, n_wp = crowd_groups(sc, share=1.0, K=2)
    assert (gid >= 0).any() and len({g.tobytes() + w.tobytes() for g, w in zip(gid, wp)}) == B
    rows = np.tile(prm.scene_row(), (B, 1))
    col = {f: i for i, f in enumerate(_abi.SCENE_PARAM_FIELDS)}
    rows[:, col["desired_linear_vel"]] -= 0.02 * np.arange(B)
    rows[:, col["distance_w"]] *= 1.0 + 0.1 * np.arange(B)
    kw = dict(plan=plan, plan_len=plan_len, traj_params=tp, plan_window=(4.0, 10.0), fov_angle=2.0, order_hint=True,
              scene_params=rows, metrics=MetricsParams(), goal=plan[np.arange(B), 40 + 5 * np.arange(B)],
              crowd=CrowdParams(), person_waypoints=wp, person_n_waypoints=n_wp,
              person_speed=0.4 + 0.05 * np.arange(B)[:, None] + 0.01 * np.arange(N)[None, :], person_groups=gid,
              crowd_groups=CrowdGroupParams(2.0, 1.5, 0.5))
    return prm, sc, w_ref, kw


def _assert_two_shards_equal_the_single_chain(prm, sc, w_ref, od, kw, ticks=2):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode

    one = BatchEpisode(prm, sc, w_ref, *od, **kw)
    two = ShardedEpisode(prm, sc, w_ref, *od, shards=2, graphs=True, **kw)
    assert [p.B for p in two.parts] == [2, 3]
    for _ in range(ticks):
        one.tick()
        two.tick()
    one.synchronize()
    for name in ("status", "iterations", "cmds", "path", "final_cost"):
        assert np.array_equal(one.res[name].cpu().numpy(), two.gather(name).cpu().numpy()), name
    for name in ("pose", "cmd_vel", "cmd_source", "persons", "person_cursor", "metrics_acc"):
        assert np.array_equal(getattr(one, name).cpu().numpy(), two.gather(name).cpu().numpy()), name
    return one


@pytest.mark.gpu
def test_two_shards_get_their_rows_of_every_optional_argument():
    """Five robots (odd, so the shards differ in size) with plans and their window, the field-of-view filter, the order
    hint, scene parameters, metrics with a goal, a crowd with speeds and groups, and grids from per-scene costmaps: the
    two-shard graph episode returns the single chain's numbers robot by robot. Then the same with host-given grids per
    scene, distances included."""
    from nav2_social_mpc_controller_amd.solver import BatchSolver

    B, N = 5, 3
    prm, sc, w_ref, kw = _every_option(B, N)
    one = _assert_two_shards_equal_the_single_chain(prm, sc, w_ref, (None, None, None), dict(kw, obstacles_from_costmap=True))
    assert one.od_shared == 0 and one.od_distances is not None
    grid = BatchSolver(prm).obstacle_distance(sc.costmap, sc.resolution)
    assert grid["indexes"].shape == (B, 80, 80) and sc.costmap_origin.shape == (B, 2)
    od = (grid["indexes"], sc.costmap_origin, float(np.float32(sc.resolution)))
    host = _assert_two_shards_equal_the_single_chain(prm, sc, w_ref, od, dict(kw, od_distances=grid["distances"]))
    assert host.od_shared == 0 and host.od_distances is not None


# ---- the optional stages' declarations --------------------------------------------------------------------------------
def test_every_stage_declares_its_keyword_and_its_record_fields():
    """Every optional stage (episode_stages) is one class with its keyword, its timing key and the TickRecord fields copied
    before and after its launch. A stage whose keyword or record field was forgotten, or claimed twice, fails here: every
    BEFORE / AFTER key is an optional TickRecord field, no field has two owners (the obstacle memory launches in the sensed
    costmap's place and records the scan's outputs too), every optional field is a stage's or on the core's list, every
    keyword is one of BatchEpisode.__init__ with default None, and no two stages share a timing key."""
    import dataclasses
    import inspect

    from nav2_social_mpc_controller_amd.episode import BatchEpisode, TickRecord
    from nav2_social_mpc_controller_amd.episode_stages import Core, ObstacleMemory, Planner, Sensed, Stage

    assert BatchEpisode.STAGES.count(Core) == 1 and len(set(BatchEpisode.STAGES)) == len(BatchEpisode.STAGES)
    stages = (Planner,) + tuple(S for S in BatchEpisode.STAGES if S is not Core)
    assert len(stages) == 15 and all(issubclass(S, Stage) for S in stages)
    optional = {f.name for f in dataclasses.fields(TickRecord) if f.default is None}
    required = {f.name for f in dataclasses.fields(TickRecord) if f.default is dataclasses.MISSING}
    assert len(optional) + len(required) == len(TickRecord.__dataclass_fields__)
    sig = inspect.signature(BatchEpisode.__init__).parameters
    owner = {}
    for S in stages:
        assert S.KEY in sig and sig[S.KEY].default is None, S
        assert isinstance(S.STATE, tuple) and all(isinstance(a, str) for a in S.STATE), S
        assert not set(S.BEFORE) & set(S.AFTER), S
        for field in list(S.BEFORE) + list(S.AFTER):
            assert field in optional, (S, field)
            if not (S is ObstacleMemory and field in Sensed.AFTER):
                assert field not in owner, (field, S, owner.get(field))
                owner[field] = S
    assert set(Sensed.AFTER) < set(ObstacleMemory.AFTER)
    # the optional fields that tick() itself fills: the core chain's, the world before and after the move, the second gather in front
    # of the metrics sample, and the windows a repair without a sensing stage reads
    core = ("robot_pose", "traj_n_poses", "window", "window_len", "plan_start", "persons", "person_count", "has_people", "T_scene", "window_err",
            "pose_after", "persons_after", "cmd_vel", "cmd_source", "agents_after", "repair_costmap")
    assert len(set(core)) == len(core) and set(core) <= optional and not set(core) & set(owner)
    assert set(core) | set(owner) == optional, sorted(optional - set(core) - set(owner))
    timing = [S.TIMING for S in stages if S is not Planner]                     # the planner never launches inside a tick
    assert all(isinstance(t, str) and t for t in timing) and len(set(timing)) == len(timing) and Planner.TIMING is None
    for name in BatchEpisode.UINT32:                                            # the uint32 views are state, named in one place
        assert any(name in S.STATE for S in stages), name
