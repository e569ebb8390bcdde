"""Cost of the people tracker (smpc_track_people_batch), three measurements, one JSON line:
  kernel: HIP-event time of the kernel alone (smpc_last_kernel_ms) on device pointers, B robots with Np detections and
          --slots track slots each, in steady state: the tracks of a moving episode (one shared --world x --world floor,
          line-of-sight filter in front, reactive crowd) after --warm ticks, restored before every call; beside
          smpc_people_to_status_batch and smpc_visible_people_batch in the same loop, alternating: median (min .. max) of
          --reps rounds. With it what the timed call does: matched, coasted and free slots, and rows handed on. In the
          same loop the same call from the same tracks with every det_count at 0 (all state read and written, every track
          coasts, no association round and no birth): the difference of the two whole launches is what association and
          births cost.
  limit:  the same call at 64 detections x 64 slots x 64 rows on synthetic persons (constant velocity inside an 8 m square,
          each seen with probability 0.8 per tick), also after --warm ticks.
  tick:   the closed-loop tick of two episodes on the same scenes, one with tracker=None (the tick without this stage) and one
          with the tracker, each replayed from its HIP graph: --rounds blocks of --ticks ticks, alternating between the two;
          median ms per tick of each and the spread (min .. max) of the blocks.

    python tools/gpu_tracker.py [--B 8192] [--Np 8] [--slots 16] [--world 1024] [--range 10.0] [--warm 12] [--reps 20] [--rounds 7]
                                [--ticks 20] [--no-tick]
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
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--world", type=int, default=1024)
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--reach", type=float, default=3.5, help="largest start distance of a person from its robot (scenes_in_world)")
    ap.add_argument("--warm", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--no-tick", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd._abi import SmpcPeopleBatch
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.params import CrowdParams, OptimizerParams, TrackerParams, VisibilityParams
    from nav2_social_mpc_controller_amd.scenes import crowd_waypoints, make_world, scenes_in_world, uniform
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point

    B, Np = a.B, a.Np
    prm, vp, tp = OptimizerParams.readme(), VisibilityParams(max_range=a.range), TrackerParams(slots=a.slots)
    out = {"B": B, "Np": Np, "slots": a.slots, "world": a.world, "max_range": a.range, "warm": a.warm}
    spread = lambda v, scale, digits=2: {"median": round(float(np.median(v)) * scale, digits), "min": round(min(v) * scale, digits),
                                         "max": round(max(v) * scale, digits)}
    world = make_world(a.world, a.world, 0.05)
    sc = scenes_in_world(prm, world, B, Np, size_x=40, size_y=40, people_reach=a.reach)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    wp, n_wp = crowd_waypoints(scenes_in_world(prm, world, B, Np, size_x=120, size_y=120, people_reach=a.reach), K=2)
    kw = dict(obstacles_from_costmap=True, world=world, crowd=CrowdParams(), person_waypoints=wp, person_n_waypoints=n_wp, visibility=vp)

    # ---- the kernel alone, on the tracks of an episode after --warm ticks
    ep = BatchEpisode(prm, sc, w_ref, tracker=tp, **kw)
    for _ in range(a.warm):
        ep.tick()
    ep.synchronize()
    s, c = ep.solver, ep._c
    s.visible_people_device(c.visibility, ep.seen_persons.data_ptr(), ep.seen_count.data_ptr(), ep.person_seen.data_ptr())   # the next tick's detections
    state0 = [t.clone() for t in (ep.tracks, ep.track_meta, ep.track_next_id)]
    qb = SmpcPeopleBatch()
    qb.B, qb.Np, qb.N, qb.on_device = B, Np, Np, 1
    qb.people, qb.count = ep.seen_persons.data_ptr(), ep.seen_count.data_ptr()
    blind = BatchSolver.tracker_c(tp, B, Np, Np, prm.dt, 1)                                  # the same call, nobody detected
    no_count = torch.zeros(B, dtype=torch.int32, device=ep.dev)
    blind_people, blind_count = torch.zeros(B, Np, 5, dtype=torch.float64, device=ep.dev), torch.zeros(B, dtype=torch.int32, device=ep.dev)
    point(blind, {"detections": ep.seen_persons, "det_count": no_count, "robot_pose": ep.pose})
    ms = {"track_people": [], "track_people_no_detections": [], "people_to_status": [], "visible_people": []}

    def restore():
        for t, t0 in zip((ep.tracks, ep.track_meta, ep.track_next_id), state0):
            t.copy_(t0)

    for r in range(a.reps + 2):
        restore()
        s.track_people_device(blind, ep.tracks.data_ptr(), ep.track_meta.data_ptr(), ep.track_next_id.data_ptr(),
                              blind_people.data_ptr(), blind_count.data_ptr(), 0)
        t_b = s.last_kernel_ms()
        restore()
        s.track_people_device(c.tracker, ep.tracks.data_ptr(), ep.track_meta.data_ptr(), ep.track_next_id.data_ptr(),
                              ep.tracked_persons.data_ptr(), ep.tracked_count.data_ptr(), ep.tracked_source.data_ptr())
        t_t = s.last_kernel_ms()
        s.people_to_status_device(qb, ep.people.data_ptr(), ep.has_people.data_ptr())
        t_p = s.last_kernel_ms()
        s.visible_people_device(c.visibility, ep.seen_persons.data_ptr(), ep.seen_count.data_ptr(), ep.person_seen.data_ptr())
        t_v = s.last_kernel_ms()
        if r >= 2:   # the first launches load the code object
            ms["track_people"].append(t_t), ms["track_people_no_detections"].append(t_b), ms["people_to_status"].append(t_p), ms["visible_people"].append(t_v)
    out["kernel_us"] = {k: spread(v, 1e3) for k, v in ms.items()}
    ep.synchronize()
    before, after = state0[1].cpu().numpy(), ep.track_meta.cpu().numpy()
    live = (before[:, :, 0] == 1) | (before[:, :, 0] == 2)
    out["steady_state"] = {"detections": int(np.clip(ep.seen_count.cpu().numpy(), 0, Np).sum()), "live_slots": int(live.sum()),
                           "matched": int((live & (after[:, :, 0] > 0) & (after[:, :, 2] == 0) & (after[:, :, 1] > before[:, :, 1])).sum()),
                           "coasted": int((live & (after[:, :, 2] > before[:, :, 2])).sum()),
                           "rows_handed_on": int(ep.tracked_count.cpu().numpy().sum())}
    del ep

    # ---- the limit: 64 x 64 x 64 on synthetic persons
    dev, n = "cuda:0", 64
    lim = TrackerParams(slots=n)
    g = torch.Generator(device=dev).manual_seed(7)
    pos = torch.rand(B, n, 2, dtype=torch.float64, device=dev, generator=g) * 8.0
    vel = (torch.rand(B, n, 2, dtype=torch.float64, device=dev, generator=g) - 0.5) * 3.0
    pose = torch.full((B, 3), 4.0, dtype=torch.float64, device=dev)
    det, cnt = torch.zeros(B, n, 5, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    tracks, meta = torch.zeros(B, n, 4, dtype=torch.float64, device=dev), torch.zeros(B, n, 4, dtype=torch.int32, device=dev)
    next_id = torch.zeros(B, dtype=torch.int32, device=dev)
    people, count = torch.zeros(B, n, 5, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    source = torch.zeros(B, n, 2, dtype=torch.int32, device=dev)
    ti = point(BatchSolver.tracker_c(lim, B, n, n, prm.dt, 1), {"detections": det, "det_count": cnt, "robot_pose": pose})
    s2 = BatchSolver(prm, device=0)
    s2.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    call = lambda: s2.track_people_device(ti, tracks.data_ptr(), meta.data_ptr(), next_id.data_ptr(), people.data_ptr(), count.data_ptr(),
                                          source.data_ptr())

    def detect(t):
        seen = torch.rand(B, n, device=dev, generator=g) < 0.8
        order = torch.argsort((~seen).to(torch.int8), dim=1, stable=True)                    # the seen rows first, in their order
        here = pos + vel * (prm.dt * t)
        det[:, :, :2] = torch.gather(here, 1, order[:, :, None].expand(B, n, 2))
        cnt.copy_(seen.sum(dim=1).to(torch.int32))

    for t in range(a.warm):
        detect(t)
        call()
    detect(a.warm)
    torch.cuda.synchronize()
    state0 = [t.clone() for t in (tracks, meta, next_id)]
    lim_ms = []
    for r in range(a.reps + 2):
        for t, t0 in zip((tracks, meta, next_id), state0):
            t.copy_(t0)
        call()
        if r >= 2:
            lim_ms.append(s2.last_kernel_ms())
    torch.cuda.synchronize()
    out["limit_64x64x64_us"] = spread(lim_ms, 1e3)
    out["limit_64x64x64"] = {"detections": int(cnt.sum().item()), "live_slots": int(((state0[1][:, :, 0] == 1) | (state0[1][:, :, 0] == 2)).sum().item()),
                             "rows_handed_on": int(count.sum().item())}
    s2.set_stream(0)
    s2.close()

    # ---- the tick with and without
    if not a.no_tick:
        eps = {"off": BatchEpisode(prm, sc, w_ref, **kw), "on": BatchEpisode(prm, sc, w_ref, tracker=tp, **kw)}
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
