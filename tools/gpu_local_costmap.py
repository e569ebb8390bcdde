"""Cost of the rolling local costmaps (smpc_local_costmap_batch), two measurements, one JSON line:
  kernel: HIP-event times on device pointers, B robots with --cells x --cells windows over one shared --world x --world map,
          median (min .. max) of --reps rounds that alternate between
            forced: every window is written (B x cells^2 bytes of stores);
            period: the roll after one control period at 0.6 m/s (dt 0.05 s: 0.6 cell) from the forced state, the stored
                    cells put back first: only the windows that moved are written (`moved_share` of them);
            copy:   a device-to-device copy of the same B x cells^2 bytes (torch, HIP events), the yardstick.
          forced is also given as a share of copy and of 8 TB/s.
  tick:   the closed-loop tick (global plans with the plan window, N persons, the world's ObstacleDistance grid) of two
          episodes on the same scenes, one with world=None (the windows the scenes were made with stay; the grid is handed
          over from the host) and one with world=, eager on one stream: --rounds blocks of --ticks ticks, alternating
          between the two; median ms per tick of each and the spread (min .. max) of the blocks.

    python tools/gpu_local_costmap.py [--B 8192] [--N 8] [--cells 200] [--world 1024] [--reps 20] [--rounds 5] [--ticks 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v, scale=1.0, digits=2):
    import numpy as np

    return {"median": round(float(np.median(v)) * scale, digits), "min": round(min(v) * scale, digits), "max": round(max(v) * scale, digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--cells", type=int, default=200)
    ap.add_argument("--world", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd.episode import BatchEpisode, arc_plans
    from nav2_social_mpc_controller_amd.params import OptimizerParams, TrajectorizerParams
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world, uniform
    from nav2_social_mpc_controller_amd.solver import BatchSolver

    B, cells = a.B, a.cells
    prm = OptimizerParams.readme()
    world = make_world(a.world, a.world, 0.05)
    sc = scenes_in_world(prm, world, B, a.N, size_x=cells, size_y=cells, margin=min(6.0, 0.25 * a.world * 0.05))
    nbytes = B * cells * cells
    out = {"B": B, "cells": cells, "world": a.world, "window_bytes": nbytes}

    # ---- the kernel alone
    s = BatchSolver(prm)
    dev = "cuda:0"
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    wm, w0 = up(world.map), up(np.asarray(world.origin, np.float64).reshape(1, 2))
    pose0 = sc.pose0.copy()
    pose1 = pose0.copy()
    pose1[:, 0] += 0.6 * prm.dt * np.cos(pose0[:, 2])
    pose1[:, 1] += 0.6 * prm.dt * np.sin(pose0[:, 2])
    pose = up(pose0)
    pose_next = up(pose1)
    cell = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    moved = torch.zeros(B, dtype=torch.int32, device=dev)
    cm, cm2 = torch.zeros(nbytes, dtype=torch.uint8, device=dev), torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    origin = torch.zeros((B, 2), dtype=torch.float64, device=dev)
    lc = {}
    for force, p in ((True, pose), (False, pose_next)):
        lc[force] = s.local_costmap_c(B, cells, cells, a.world, a.world, True, world.resolution, 1, 255, force)
        lc[force].world, lc[force].world_origin, lc[force].pose = wm.data_ptr(), w0.data_ptr(), p.data_ptr()
    roll = lambda force: s.local_costmap_device(lc[force], cell.data_ptr(), cm.data_ptr(), origin.data_ptr(), moved.data_ptr())
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {"forced": [], "period": [], "copy": []}
    share = 0.0
    for r in range(a.reps + 2):
        roll(True)
        t_f = s.last_kernel_ms()
        cell0 = cell.clone()
        roll(False)
        t_p = s.last_kernel_ms()
        share = float((moved == 1).double().mean().item())
        cell.copy_(cell0)
        ev0.record()
        cm2.copy_(cm)
        ev1.record()
        ev1.synchronize()
        if r >= 2:   # the first launches load the code object
            ms["forced"].append(t_f), ms["period"].append(t_p), ms["copy"].append(ev0.elapsed_time(ev1))
    out["kernel_us"] = {k: spread(v, 1e3) for k, v in ms.items()}
    f, c = float(np.median(ms["forced"])), float(np.median(ms["copy"]))
    out["moved_share"] = round(share, 4)
    out["forced_over_copy"] = round(f / c, 3)
    out["forced_TBps"] = round(nbytes / (f * 1e-3) / 1e12, 3)
    out["forced_share_of_8TBps"] = round(nbytes / (f * 1e-3) / 8e12, 3)
    del cm, cm2

    # ---- the tick with and without
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    kw = dict(plan=plan, plan_len=plan_len, traj_params=TrajectorizerParams(desired_linear_vel=0.6, max_time=prm.max_time),
              plan_window=(10.0, 10.0))
    grid = s.obstacle_distance(world.map, world.resolution, distances=False)["indexes"]
    eps = {"off": BatchEpisode(prm, sc, w_ref, grid, world.origin, float(np.float32(world.resolution)), **kw),
           "on": BatchEpisode(prm, sc, w_ref, obstacles_from_costmap=True, world=world, **kw)}
    blocks = {"off": [], "on": []}
    for r in range(a.rounds + 1):
        for name, e in eps.items():
            e.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.ticks):
                e.tick()
            e.synchronize()
            if r >= 1:   # one warm-up round
                blocks[name].append((time.perf_counter() - t0) / a.ticks * 1e3)
    out["tick_ms"] = {k: spread(v, 1.0, 4) for k, v in blocks.items()}
    tm = {}
    eps["on"].tick(timing=tm)
    out["tick_on_local_costmap_us"] = round(tm["local_costmap_ms"] * 1e3, 2)
    out["tick_on_moved_share"] = round(float((eps["on"].costmap_moved == 1).double().mean().item()), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
