"""Cost of the line-of-sight filter (smpc_visible_people_batch), two measurements, one JSON line:
  kernel: HIP-event time of the kernel alone (smpc_last_kernel_ms) on device pointers, B robots with Np persons each on one
          shared --world x --world floor (scenes.make_world, 0.05 m) with --range metres of detector range, beside
          smpc_people_to_status_batch and the plain crowd step (smpc_crowd_step_batch) on the same persons in the same loop,
          alternating: median (min .. max) of --reps rounds. With it the share of the persons that are hidden and the mean
          length of a ray in cells (the larger of its two cell distances: the columns the lanes share out).
  tick:   the closed-loop tick (arc stand-in, rolling 40 x 40 windows, reactive crowd) of two episodes on the same scenes,
          one with visibility=None and one with the filter, each replayed from its HIP graph: --rounds blocks of --ticks
          ticks, alternating between the two; median ms per tick of each and the spread (min .. max) of the blocks.

    python tools/gpu_visibility.py [--B 8192] [--Np 8] [--world 1024] [--range 10.0] [--reach 3.5] [--reps 20] [--rounds 7] [--ticks 20]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=20)
    a = ap.parse_args()

    import numpy as np

    from nav2_social_mpc_controller_amd._abi import SmpcPeopleBatch
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.episode_stages import Crowd
    from nav2_social_mpc_controller_amd.params import CrowdParams, OptimizerParams, VisibilityParams
    from nav2_social_mpc_controller_amd.scenes import crowd_waypoints, make_world, scenes_in_world, uniform

    B, Np = a.B, a.Np
    prm, vp = OptimizerParams.readme(), VisibilityParams(max_range=a.range)
    out = {"B": B, "Np": Np, "world": a.world, "max_range": a.range}
    spread = lambda v, scale, digits=2: {"median": round(float(np.median(v)) * scale, digits), "min": round(min(v) * scale, digits),
                                         "max": round(max(v) * scale, digits)}
    world = make_world(a.world, a.world, 0.05)
    sc = scenes_in_world(prm, world, B, Np, size_x=40, size_y=40, people_reach=a.reach)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    wp, n_wp = crowd_waypoints(scenes_in_world(prm, world, B, Np, size_x=120, size_y=120, people_reach=a.reach), K=2)
    kw = dict(obstacles_from_costmap=True, world=world, crowd=CrowdParams(), person_waypoints=wp, person_n_waypoints=n_wp)

    # ---- the kernel alone, on the state of an episode after a few ticks
    ep = BatchEpisode(prm, sc, w_ref, visibility=vp, **kw)
    for _ in range(3):
        ep.tick()
    ep.synchronize()
    persons0, cursor0 = ep.persons.clone(), ep.person_cursor.clone()
    s = ep.solver
    qb = SmpcPeopleBatch()
    qb.B, qb.Np, qb.N, qb.on_device = B, Np, Np, 1
    qb.people, qb.count = ep.persons.data_ptr(), ep.person_count.data_ptr()
    ms = {"visible_people": [], "people_to_status": [], "crowd_step": []}
    for r in range(a.reps + 2):
        s.visible_people_device(ep._c.visibility, ep.seen_persons.data_ptr(), ep.seen_count.data_ptr(), ep.person_seen.data_ptr())
        t_v = s.last_kernel_ms()
        s.people_to_status_device(qb, ep.people.data_ptr(), ep.has_people.data_ptr())
        t_p = s.last_kernel_ms()
        Crowd.launch(ep)
        t_c = s.last_kernel_ms()
        ep.persons.copy_(persons0), ep.person_cursor.copy_(cursor0)
        if r >= 2:   # the first launches load the code object
            ms["visible_people"].append(t_v), ms["people_to_status"].append(t_p), ms["crowd_step"].append(t_c)
    out["kernel_us"] = {k: spread(v, 1e3) for k, v in ms.items()}
    ep.synchronize()
    seen, count = ep.person_seen.cpu().numpy(), np.clip(ep.person_count.cpu().numpy(), 0, Np)
    valid = np.arange(Np)[None, :] < count[:, None]
    pose, persons = ep.pose.cpu().numpy(), ep.persons.cpu().numpy()
    cell = lambda xy: np.floor((xy - world.origin) / world.resolution)
    steps = np.abs(cell(persons[:, :, :2]) - cell(pose[:, None, :2])).max(axis=2)
    out["persons"] = int(valid.sum())
    out["codes"] = {name: int((seen[valid] == code).sum()) for code, name in enumerate(("hidden", "seen", "out_of_range", "not_finite"))}
    out["hidden_share"] = round(float((seen[valid] == 0).mean()), 4)
    out["mean_ray_cells"] = round(float(steps[valid & (seen < 2)].mean()), 2)
    del ep

    # ---- the tick with and without
    eps = {"off": BatchEpisode(prm, sc, w_ref, **kw), "on": BatchEpisode(prm, sc, w_ref, visibility=vp, **kw)}
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
