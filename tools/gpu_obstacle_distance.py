"""Kernel time of smpc_obstacle_distance_batch (the ObstacleDistance grid from the costmaps) for B scenes of the bench's
crowd maps (make_scenes, 200 x 200 cells by default), indexes alone and indexes + distances, on device pointers.
Achieved bytes/s = what the transform must move (costmap read once, every output written once) over the kernel time
(smpc_last_kernel_ms, HIP events); the share of the 8 TB/s HBM peak beside it. Prints one JSON line.

    python tools/gpu_obstacle_distance.py [--B 8192] [--cells 200] [--reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--cells", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd.params import OptimizerParams
    from nav2_social_mpc_controller_amd.scenes import make_scenes
    from nav2_social_mpc_controller_amd.solver import BatchSolver

    dev = "cuda:0"
    sc = make_scenes(OptimizerParams.readme(), a.B, 3, map_cells=a.cells)
    s = BatchSolver(OptimizerParams.readme())
    s.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    cm = torch.from_numpy(sc.costmap).to(dev)
    B, H, W = sc.costmap.shape
    idx = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    dist = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    n = torch.empty(B, dtype=torch.int32, device=dev)
    ob = BatchSolver.obstacle_distance_c(B, W, H, False, sc.resolution, 1)
    ob.costmap = cm.data_ptr()
    cells = B * H * W
    out = {"B": B, "H": H, "W": W, "mean_obstacle_cells": None}
    for name, dptr in (("indexes", 0), ("indexes_distances", dist.data_ptr())):
        ms = []
        for r in range(a.reps + 2):
            s.obstacle_distance_device(ob, idx.data_ptr(), dptr, n.data_ptr())
            t = s.last_kernel_ms()
            if r >= 2:   # the first launches load the code object
                ms.append(t)
        med = float(np.median(ms))
        nbytes = cells * (1 + 4 + (4 if dptr else 0)) + 4 * B
        out[name] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms), 4), "bytes": nbytes,
                     "GBps": round(nbytes / (med * 1e-3) / 1e9, 1),
                     "hbm_fraction": round(nbytes / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 3)}
    out["mean_obstacle_cells"] = float(n.double().mean().item())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
