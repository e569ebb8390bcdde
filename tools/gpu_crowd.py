"""Cost of the reactive crowd (smpc_crowd_step_batch, smpc_crowd_step_groups_batch), two measurements, one JSON line:
  kernel: HIP-event time of the crowd kernel alone (smpc_last_kernel_ms) on device pointers, B robots with Np persons each
          on per-robot --cells x --cells ObstacleDistance grids computed from the scenes' costmaps, median of --reps
          launches; smpc_people_to_status_batch and smpc_episode_metrics_batch on the same state beside it, alternating.
          The groups kernel (crowd_step_groups) runs in the same loop on the same inputs — the persons and cursors the
          plain launch started from are put back first —, with half of the walking persons in pairs and triples
          (scenes.crowd_groups).
  tick:   the closed-loop tick (arc stand-in, N = Np agents, grids from the costmaps) of two episodes on the same scenes,
          one with crowd=None (constant-velocity persons) and one with the crowd, each replayed from its HIP graph:
          --rounds blocks of --ticks ticks, alternating between the two; median ms per tick of each and the spread
          (min .. max) of the blocks.

    python tools/gpu_crowd.py [--B 8192] [--Np 8] [--cells 200] [--reps 20] [--rounds 7] [--ticks 20]
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
    ap.add_argument("--cells", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=20)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd._abi import SmpcPeopleBatch
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.episode_stages import Crowd, Metrics
    from nav2_social_mpc_controller_amd.params import CrowdParams, MetricsParams, OptimizerParams
    from nav2_social_mpc_controller_amd.scenes import crowd_groups, crowd_waypoints, make_scenes, uniform

    B, Np = a.B, a.Np
    prm, cp, mp = OptimizerParams.readme(), CrowdParams(), MetricsParams()
    out = {"B": B, "Np": Np, "cells": a.cells}
    sc = make_scenes(prm, B, Np, map_cells=a.cells)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    wp, n_wp = crowd_waypoints(sc, K=2)
    crowd = dict(crowd=cp, person_waypoints=wp, person_n_waypoints=n_wp)

    # ---- the kernel alone, on the state of an episode after a few ticks (its own buffers, its own grids)
    gid, _, _ = crowd_groups(sc, K=2)   # the ids alone are used: both kernels run on the plain waypoints
    ep = BatchEpisode(prm, sc, w_ref, obstacles_from_costmap=True, metrics=mp, person_groups=gid, **crowd)
    out["grouped_persons"] = int((gid >= 0).sum())
    for _ in range(3):
        ep.tick()
    ep.synchronize()
    persons0, cursor0 = ep.persons.clone(), ep.person_cursor.clone()
    s = ep.solver
    qb = SmpcPeopleBatch()
    qb.B, qb.Np, qb.N, qb.on_device = B, Np, Np, 1
    qb.people, qb.count = ep.persons.data_ptr(), ep.person_count.data_ptr()
    ms = {"crowd_step": [], "crowd_step_groups": [], "people_to_status": [], "episode_metrics": []}
    for r in range(a.reps + 2):
        ep.persons.copy_(persons0), ep.person_cursor.copy_(cursor0)
        Crowd.launch(ep, groups=False)
        t_c = s.last_kernel_ms()
        ep.persons.copy_(persons0), ep.person_cursor.copy_(cursor0)
        Crowd.launch(ep)
        t_g = s.last_kernel_ms()
        s.people_to_status_device(qb, ep.people.data_ptr(), ep.has_people.data_ptr())
        t_p = s.last_kernel_ms()
        Metrics.launch(ep)
        t_m = s.last_kernel_ms()
        if r >= 2:   # the first launches load the code object
            ms["crowd_step"].append(t_c)
            ms["crowd_step_groups"].append(t_g)
            ms["people_to_status"].append(t_p)
            ms["episode_metrics"].append(t_m)
    out["kernel_us"] = {k: {"median": round(float(np.median(v)) * 1e3, 2), "min": round(min(v) * 1e3, 2), "max": round(max(v) * 1e3, 2)}
                        for k, v in ms.items()}
    assert np.isfinite(ep.persons.cpu().numpy()).all()
    del ep

    # ---- the tick with and without
    eps = {"off": BatchEpisode(prm, sc, w_ref, obstacles_from_costmap=True),
           "on": BatchEpisode(prm, sc, w_ref, obstacles_from_costmap=True, **crowd)}
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
    out["tick_ms_graph"] = {k: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                            for k, v in blocks.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
