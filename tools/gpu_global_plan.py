"""Cost of the global plans (smpc_goal_field_batch / smpc_extract_plan_batch): HIP-event times on device pointers, median
(min .. max) of --reps rounds, one JSON line:
  field_small: G goal fields on the 256 x 192 floor (make_world(256, 192, 0.05, seed 0x5EED0004));
  field_large: G goal fields on make_world(--world, --world), with smpc_obstacle_distance_batch on the same map in the same
               loop as the yardstick (od_large);
  extract:     B robots over the G fields of the large floor (max_poses 400, stride 1), with
               smpc_transform_global_plan_batch over the plans just written in the same loop as the yardstick (window).

    python tools/gpu_global_plan.py [--G 64] [--B 8192] [--world 1024] [--reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v, scale=1.0, digits=1):
    import numpy as np

    return {"median": round(float(np.median(v)) * scale, digits), "min": round(min(v) * scale, digits), "max": round(max(v) * scale, digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, default=64)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--world", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd._abi import SmpcPlanWindowBatch
    from nav2_social_mpc_controller_amd.params import GlobalPlanParams, OptimizerParams
    from nav2_social_mpc_controller_amd.scenes import make_world, uniform, world_goals
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point

    G, B = a.G, a.B
    gp = GlobalPlanParams()
    s = BatchSolver(OptimizerParams.readme())
    dev = "cuda:0"
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = {"G": G, "B": B, "reps": a.reps}

    def floor(world):
        """(device world, origin, goals, field buffer, the bound goal-field struct) of G goals on `world`."""
        goals = world_goals(world, np.tile(world.origin + 0.5, (G, 1)), min_dist=0.0)
        t = dict(world=up(world.map), world_origin=up(np.asarray(world.origin, np.float64).reshape(1, 2)), goal=up(goals))
        field = torch.empty((G, world.cells_y, world.cells_x), dtype=torch.int32, device=dev)
        status = torch.zeros(G, dtype=torch.int32, device=dev)
        gf = point(s.goal_field_c(gp, G, world.cells_x, world.cells_y, True, world.resolution, 1), t)
        return t, goals, field, status, gf

    small = make_world(256, 192, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15))
    large = make_world(a.world, a.world, 0.05)
    ts, _, field_s, status_s, gf_s = floor(small)
    tl, goals_l, field_l, status_l, gf_l = floor(large)
    od = s.obstacle_distance_c(1, a.world, a.world, True, large.resolution, 1)
    od.costmap = tl["world"].data_ptr()
    od_idx = torch.empty((1, a.world, a.world), dtype=torch.int32, device=dev)
    od_dist = torch.empty((1, a.world, a.world), dtype=torch.float32, device=dev)

    # robots: uniform over the free cells of the large floor, each with the goal b % G
    free = np.argwhere(large.map == 0)
    pick = (uniform(0x5EED0006, np.arange(B), 1)[:, 0] * len(free)).astype(np.int64)
    pose = np.zeros((B, 3))
    pose[:, 0] = large.origin[0] + (free[pick, 1] + 0.5) * large.resolution
    pose[:, 1] = large.origin[1] + (free[pick, 0] + 0.5) * large.resolution
    te = dict(tl, field=field_l, robot_goal=up((np.arange(B) % G).astype(np.int32)), pose=up(pose))
    ep = point(s.extract_plan_c(gp, B, G, a.world, a.world, True, large.resolution, 1), te)
    plan = torch.zeros((B, gp.max_poses, 2), dtype=torch.float64, device=dev)
    plan_len = torch.zeros(B, dtype=torch.int32, device=dev)
    error = torch.zeros(B, dtype=torch.int32, device=dev)
    plan_start = torch.zeros(B, dtype=torch.int32, device=dev)
    window, window_len = torch.zeros_like(plan), torch.zeros(B, dtype=torch.int32, device=dev)
    wb = point(SmpcPlanWindowBatch(B=B, L=gp.max_poses, on_device=1, max_robot_pose_search_dist=4.0, dist_threshold=10.0),
               {"plan": plan, "plan_len": plan_len, "plan_start": plan_start, "robot_pose": te["pose"]})

    ms = {"field_small": [], "field_large": [], "od_large": [], "extract": [], "window": []}
    for r in range(a.reps + 2):
        s.goal_field_device(gf_s, field_s.data_ptr(), status_s.data_ptr())
        t_fs = s.last_kernel_ms()
        s.goal_field_device(gf_l, field_l.data_ptr(), status_l.data_ptr())
        t_fl = s.last_kernel_ms()
        s.obstacle_distance_device(od, od_idx.data_ptr(), od_dist.data_ptr())
        t_od = s.last_kernel_ms()
        s.extract_plan_device(ep, plan.data_ptr(), plan_len.data_ptr(), error.data_ptr())
        t_ex = s.last_kernel_ms()
        plan_start.zero_()
        s.transform_global_plan_device(wb, window.data_ptr(), window_len.data_ptr())
        t_w = s.last_kernel_ms()
        if r >= 2:   # the first launches load the code object
            for k, v in zip(ms, (t_fs, t_fl, t_od, t_ex, t_w)):
                ms[k].append(v)
    out["kernel_us"] = {k: spread(v, 1e3) for k, v in ms.items()}
    err = error.cpu().numpy()
    n = plan_len.cpu().numpy()
    out["status_bad"] = int((status_s != 0).sum().item() + (status_l != 0).sum().item())
    out["plan_errors"] = {str(k): int(v) for k, v in enumerate(np.bincount(err, minlength=7)) if v}
    out["plan_poses"] = {"median": int(np.median(n)), "max": int(n.max())}
    out["field_large_over_od"] = round(float(np.median(ms["field_large"]) / np.median(ms["od_large"])), 2)
    out["extract_over_window"] = round(float(np.median(ms["extract"]) / np.median(ms["window"])), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
