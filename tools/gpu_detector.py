"""Cost of the people detector (smpc_detect_people_batch) and what the tracker makes of its output, one JSON line:
  kernel: HIP-event time of the kernel alone (smpc_last_kernel_ms) on device pointers, B robots with Np persons and Kc = 2
          clutter candidates each, on the state of a moving episode (one shared --world x --world floor, line-of-sight filter
          in front, tracker behind, reactive crowd) after --warm ticks; beside smpc_people_to_status_batch,
          smpc_visible_people_batch and smpc_track_people_batch in the same loop, alternating: median (min .. max) of --reps
          rounds. In the same loop the same call with noise scales, miss_threshold and clutter_threshold of 0 (the same
          geometry, no Philox call at all): the difference of the two whole launches is what the generator costs. With it
          the outcomes of the timed call.
  limit:  the same call at 64 persons x 64 rows x 64 clutter candidates on synthetic persons inside an 8 m square.
  tick:   the closed-loop tick of two episodes on the same scenes, one with detector=None (the tick of the commit before,
          bit for bit) and one with the detector, each replayed from its HIP graph: --rounds blocks of --ticks ticks,
          alternating between the two; median ms per tick of each and the spread (min .. max) of the blocks.
  noise:  what the tracker does under this noise, on a seeded episode of --study-B robots over --study-ticks recorded ticks
          (no line-of-sight filter, so that row j of the detections' sources is person j): the RMS error of the tracked rows'
          velocities against the true velocities of the persons they lie nearest to, beside that of finite differences of
          consecutive raw detections of the same person.

    python tools/gpu_detector.py [--B 8192] [--Np 8] [--world 1024] [--range 10.0] [--warm 12] [--reps 20] [--rounds 7] [--ticks 20]
                                 [--study-B 256] [--study-ticks 60] [--no-tick] [--no-study]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--Np", type=int, default=8)
    ap.add_argument("--world", type=int, default=1024)
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--reach", type=float, default=3.5, help="largest start distance of a person from its robot (scenes_in_world)")
    ap.add_argument("--warm", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--study-B", type=int, default=256)
    ap.add_argument("--study-ticks", type=int, default=60)
    ap.add_argument("--no-tick", action="store_true")
    ap.add_argument("--no-study", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd._abi import SmpcPeopleBatch
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.params import CrowdParams, DetectorParams, OptimizerParams, TrackerParams, VisibilityParams
    from nav2_social_mpc_controller_amd.scenes import crowd_waypoints, make_world, scenes_in_world, uniform
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point

    B, Np = a.B, a.Np
    prm, vp, tp, dp = OptimizerParams.readme(), VisibilityParams(max_range=a.range), TrackerParams(), DetectorParams(seed=0x5EED0007)
    out = {"B": B, "Np": Np, "Kc": dp.clutter_candidates, "world": a.world, "max_range": a.range, "warm": a.warm}
    spread = lambda v, scale, digits=2: {"median": round(float(np.median(v)) * scale, digits), "min": round(min(v) * scale, digits),
                                         "max": round(max(v) * scale, digits)}
    world = make_world(a.world, a.world, 0.05)
    sc = scenes_in_world(prm, world, B, Np, size_x=40, size_y=40, people_reach=a.reach)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    wp, n_wp = crowd_waypoints(scenes_in_world(prm, world, B, Np, size_x=120, size_y=120, people_reach=a.reach), K=2)
    kw = dict(obstacles_from_costmap=True, world=world, crowd=CrowdParams(), person_waypoints=wp, person_n_waypoints=n_wp, visibility=vp, tracker=tp)

    # ---- the kernel alone, on the state of an episode after --warm ticks
    ep = BatchEpisode(prm, sc, w_ref, detector=dp, **kw)
    for _ in range(a.warm):
        ep.tick()
    ep.synchronize()
    s, c = ep.solver, ep._c
    s.visible_people_device(c.visibility, ep.seen_persons.data_ptr(), ep.seen_count.data_ptr(), ep.person_seen.data_ptr())   # the next tick's persons in sight
    Nd = int(ep.detected_persons.shape[1])
    quiet = BatchSolver.detector_c(dp, B, Np, Nd, 1)                                           # the same geometry, no draw
    quiet.miss_threshold = quiet.clutter_threshold = 0
    quiet.noise_scale = quiet.noise_growth = 0.0
    point(quiet, {"people": ep.seen_persons, "count": ep.seen_count, "robot_pose": ep.pose})
    q_det, q_count = torch.zeros_like(ep.detected_persons), torch.zeros_like(ep.detected_count)
    q_state = ep.draw_state.clone()
    qb = SmpcPeopleBatch()
    qb.B, qb.Np, qb.N, qb.on_device = B, Np, Np, 1
    qb.people, qb.count = ep.seen_persons.data_ptr(), ep.seen_count.data_ptr()
    tracker_state0 = [t.clone() for t in (ep.tracks, ep.track_meta, ep.track_next_id)]
    ms = {"detect_people": [], "detect_people_no_draws": [], "people_to_status": [], "visible_people": [], "track_people": []}
    for r in range(a.reps + 2):
        s.detect_people_device(quiet, q_state.data_ptr(), q_det.data_ptr(), q_count.data_ptr(), 0, 0)
        t_q = s.last_kernel_ms()
        s.detect_people_device(c.detector, ep.draw_state.data_ptr(), ep.detected_persons.data_ptr(), ep.detected_count.data_ptr(),
                               ep.detected_source.data_ptr(), ep.person_outcome.data_ptr())
        t_d = s.last_kernel_ms()
        s.people_to_status_device(qb, ep.people.data_ptr(), ep.has_people.data_ptr())
        t_p = s.last_kernel_ms()
        s.visible_people_device(c.visibility, ep.seen_persons.data_ptr(), ep.seen_count.data_ptr(), ep.person_seen.data_ptr())
        t_v = s.last_kernel_ms()
        for t, t0 in zip((ep.tracks, ep.track_meta, ep.track_next_id), tracker_state0):
            t.copy_(t0)
        s.track_people_device(c.tracker, ep.tracks.data_ptr(), ep.track_meta.data_ptr(), ep.track_next_id.data_ptr(),
                              ep.tracked_persons.data_ptr(), ep.tracked_count.data_ptr(), ep.tracked_source.data_ptr())
        t_t = s.last_kernel_ms()
        if r >= 2:   # the first launches load the code object
            for k, v in zip(ms, (t_d, t_q, t_p, t_v, t_t)):
                ms[k].append(v)
    out["kernel_us"] = {k: spread(v, 1e3) for k, v in ms.items()}
    ep.synchronize()
    n_seen = np.clip(ep.seen_count.cpu().numpy(), 0, Np)
    oc = ep.person_outcome.cpu().numpy()
    valid = np.arange(Np)[None, :] < n_seen[:, None]
    out["steady_state"] = {"persons_in_sight": int(n_seen.sum()), **{name: int(((oc == code) & valid).sum()) for code, name in
                                                                    enumerate(("detected", "body_occluded", "missed", "not_finite"))},
                           "rows_reported": int(ep.detected_count.cpu().numpy().sum()),
                           "clutter_rows": int((ep.detected_source.cpu().numpy() < 0)[np.arange(Nd)[None, :] < ep.detected_count.cpu().numpy()[:, None]].sum())}
    del ep

    # ---- the limit: 64 x 64 x 64 on synthetic persons
    dev, n = "cuda:0", 64
    lim = DetectorParams(clutter_candidates=n, p_clutter=0.3, seed=0x5EED0008)
    g = torch.Generator(device=dev).manual_seed(7)
    people = torch.zeros(B, n, 5, dtype=torch.float64, device=dev)
    people[:, :, :2] = torch.rand(B, n, 2, dtype=torch.float64, device=dev, generator=g) * 8.0
    pose = torch.full((B, 3), 4.0, dtype=torch.float64, device=dev)
    cnt = torch.full((B,), n, dtype=torch.int32, device=dev)
    draw = torch.zeros(B, 2, dtype=torch.int32, device=dev)
    draw[:, 0] = torch.arange(B, dtype=torch.int32, device=dev)
    det, det_count = torch.zeros(B, n, 5, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    source, outcome = torch.zeros(B, n, dtype=torch.int32, device=dev), torch.zeros(B, n, dtype=torch.uint8, device=dev)
    di = point(BatchSolver.detector_c(lim, B, n, n, 1), {"people": people, "count": cnt, "robot_pose": pose})
    s2 = BatchSolver(prm, device=0)
    s2.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    lim_ms = []
    for r in range(a.reps + 2):
        s2.detect_people_device(di, draw.data_ptr(), det.data_ptr(), det_count.data_ptr(), source.data_ptr(), outcome.data_ptr())
        if r >= 2:
            lim_ms.append(s2.last_kernel_ms())
    torch.cuda.synchronize()
    oc = outcome.cpu().numpy()
    out["limit_64x64x64_us"] = spread(lim_ms, 1e3)
    out["limit_64x64x64"] = {name: int((oc == code).sum()) for code, name in enumerate(("detected", "body_occluded", "missed", "not_finite"))}
    s2.set_stream(0)
    s2.close()

    # ---- the tick with and without
    if not a.no_tick:
        eps = {"off": BatchEpisode(prm, sc, w_ref, **kw), "on": BatchEpisode(prm, sc, w_ref, detector=dp, **kw)}
        for e in eps.values():
            e.capture_graph()
        blocks = {"off": [], "on": []}
        for r in range(a.rounds + 1):
            for name, e in eps.items():
                e.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.ticks):
                    e.replay()
                e.synchronize()
                if r >= 1:   # one warm-up round
                    blocks[name].append((time.perf_counter() - t0) / a.ticks * 1e3)
        out["tick_ms_graph"] = {k: spread(v, 1.0, 4) for k, v in blocks.items()}
        del eps

    # ---- the tracker under noise
    if not a.no_study:
        Bs = min(a.study_B, B)
        idx = np.arange(Bs)
        kws = dict(obstacles_from_costmap=True, world=world, crowd=CrowdParams(), person_waypoints=wp[idx], person_n_waypoints=n_wp[idx], tracker=tp)
        study = BatchEpisode(prm, sc.select(idx), w_ref[idx], detector=dp, **kws)
        dt, prev, fd, tr = float(prm.dt), None, [], []
        for k in range(a.study_ticks):
            r = study.tick(record=True)
            true = r.persons                                                                   # [Bs,Np,5] at the tick the detector saw
            for b in range(Bs):
                for row in range(int(r.detected_count[b])):                                    # finite differences of the raw detections
                    j = int(r.detected_source[b, row])
                    if j >= 0 and prev is not None and (b, j) in prev:
                        fd.append((r.detected_persons[b, row, :2] - prev[b, j]) / dt - true[b, j, 2:4])
                if k >= a.study_ticks // 3:                                                    # the tracks, once they had time to settle
                    n_true = int(np.clip(r.person_count[b], 0, Np))
                    for row in range(int(r.tracked_count[b])):
                        d = np.hypot(*(true[b, :n_true, :2] - r.tracked_persons[b, row, :2]).T) if n_true else np.array([np.inf])
                        if d.min() <= 0.5:
                            tr.append(r.tracked_persons[b, row, 2:4] - true[b, int(d.argmin()), 2:4])
            prev = {(b, int(r.detected_source[b, row])): r.detected_persons[b, row, :2].copy()
                    for b in range(Bs) for row in range(int(r.detected_count[b])) if r.detected_source[b, row] >= 0}
        rms = lambda v: round(float(np.sqrt(np.mean(np.sum(np.square(np.array(v)), axis=1)))), 4) if v else None
        out["tracker_under_noise"] = {"robots": Bs, "ticks": a.study_ticks, "sigma": dp.sigma, "sigma_growth": dp.sigma_growth, "p_miss": dp.p_miss,
                                      "rms_velocity_error_tracked": rms(tr), "tracked_samples": len(tr),
                                      "rms_velocity_error_finite_differences": rms(fd), "finite_difference_samples": len(fd)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
