"""Cost of the plan smoothing (smpc_smooth_plan_batch): HIP-event times on device pointers, median (min .. max) of --reps
alternating rounds, one JSON line:
  smooth:       B plans of up to 400 poses, extracted on make_world(--world, --world) as tools/gpu_global_plan.py extracts them,
                smoothed with PlanSmootherParams() on that map; smpc_extract_plan_batch on the same plans in the same loop is
                the yardstick (extract);
  smooth_r0:    the same call with refinement_num = 0;
  smooth_long:  --B-long plans of up to 1024 poses (the kernel's second slot count), extracted the same way.
With the times: the mean sweeps per plan, the share of plans with a rejected candidate, the status counts, and the summed
absolute heading change of the raw and of the smoothed plans (radians, mean per plan). Every round smooths a fresh copy of the
raw plans.

    python tools/gpu_plan_smoother.py [--G 64] [--B 8192] [--B-long 64] [--world 1024] [--reps 20]
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


def turning(plan, plan_len):
    """[B]: the summed absolute heading change of every plan's first plan_len rows (repeated points skipped)."""
    import numpy as np

    out = np.zeros(len(plan))
    for b, n in enumerate(plan_len):
        d = np.diff(plan[b, :n], axis=0)
        d = d[np.hypot(d[:, 0], d[:, 1]) > 0.0]
        dth = np.diff(np.arctan2(d[:, 1], d[:, 0]))
        out[b] = np.abs((dth + np.pi) % (2.0 * np.pi) - np.pi).sum()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, default=64)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--B-long", type=int, default=64, dest="B_long")
    ap.add_argument("--world", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()

    import dataclasses

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd._abi_plan_smoother import SMOOTH_STATUS
    from nav2_social_mpc_controller_amd.params import GlobalPlanParams, OptimizerParams, PlanSmootherParams
    from nav2_social_mpc_controller_amd.scenes import make_world, uniform, world_goals
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point

    G = a.G
    s = BatchSolver(OptimizerParams.readme())
    dev = "cuda:0"
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    world = make_world(a.world, a.world, 0.05)
    goals = world_goals(world, np.tile(world.origin + 0.5, (G, 1)), min_dist=0.0)
    tw = dict(world=up(world.map), world_origin=up(np.asarray(world.origin, np.float64).reshape(1, 2)))
    field = torch.empty((G, a.world, a.world), dtype=torch.int32, device=dev)
    gp0 = GlobalPlanParams()
    s.goal_field_device(point(s.goal_field_c(gp0, G, a.world, a.world, True, world.resolution, 1), dict(tw, goal=up(goals))), field.data_ptr())
    free = np.argwhere(world.map == 0)

    def plans(B, L):
        """B robots uniform over the free cells, goal b % G: (bound extract struct, plan, plan_len, error)."""
        gp = GlobalPlanParams(max_poses=L)
        pick = (uniform(0x5EED0006, np.arange(B), 1)[:, 0] * len(free)).astype(np.int64)
        pose = np.zeros((B, 3))
        pose[:, 0] = world.origin[0] + (free[pick, 1] + 0.5) * world.resolution
        pose[:, 1] = world.origin[1] + (free[pick, 0] + 0.5) * world.resolution
        te = dict(tw, field=field, goal=up(goals), robot_goal=up((np.arange(B) % G).astype(np.int32)), pose=up(pose))
        ex = point(s.extract_plan_c(gp, B, G, a.world, a.world, True, world.resolution, 1), te)
        plan = torch.zeros((B, L, 2), dtype=torch.float64, device=dev)
        plan_len, error = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        s.extract_plan_device(ex, plan.data_ptr(), plan_len.data_ptr(), error.data_ptr())
        return dict(ex=ex, keep=te, plan=plan, plan_len=plan_len, error=error, raw=plan.clone(), gp=gp, B=B, L=L,
                    status=torch.zeros(B, dtype=torch.int32, device=dev), info=torch.zeros((B, 4), dtype=torch.int32, device=dev),
                    change=torch.zeros(B, dtype=torch.float64, device=dev))

    def smoother(p, sp):
        return point(s.smooth_plan_c(sp, p["B"], p["L"], a.world, a.world, True, world.resolution, 1, p["gp"].lethal_min_cost, p["gp"].allow_unknown),
                     dict(tw, plan_len=p["plan_len"]))

    def smooth(p, si):
        p["plan"].copy_(p["raw"])
        s.smooth_plan_device(si, p["plan"].data_ptr(), p["status"].data_ptr(), p["info"].data_ptr(), p["change"].data_ptr())
        return s.last_kernel_ms()

    def report(p):
        n, info, st = p["plan_len"].cpu().numpy(), p["info"].cpu().numpy(), p["status"].cpu().numpy()
        raw, got = p["raw"].cpu().numpy(), p["plan"].cpu().numpy()
        return {"plan_poses": {"median": int(np.median(n)), "max": int(n.max())}, "plan_errors": int((p["error"] != 0).sum().item()),
                "mean_sweeps": round(float(info[:, 0].mean()), 1), "max_sweeps": int(info[:, 0].max()),
                "share_with_rejection": round(float((info[:, 2] > 0).mean()), 4),
                "status": {SMOOTH_STATUS[k]: int(v) for k, v in enumerate(np.bincount(st, minlength=4)) if v},
                "turning_raw": round(float(turning(raw, n).mean()), 3), "turning_smoothed": round(float(turning(got, n).mean()), 3)}

    sp = PlanSmootherParams()
    short, long_ = plans(a.B, 400), plans(a.B_long, 1024)
    si, si_r0, si_long = smoother(short, sp), smoother(short, dataclasses.replace(sp, refinement_num=0)), smoother(long_, sp)
    out = {"G": G, "B": a.B, "B_long": a.B_long, "world": a.world, "reps": a.reps}
    ms = {"extract": [], "smooth": [], "smooth_r0": [], "smooth_long": []}
    for r in range(a.reps + 2):
        s.extract_plan_device(short["ex"], short["raw"].data_ptr(), short["plan_len"].data_ptr(), short["error"].data_ptr())
        t_ex = s.last_kernel_ms()
        t_r0 = smooth(short, si_r0)
        if r == a.reps + 1:
            out["smooth_r0_report"] = report(short)
        t_sm = smooth(short, si)
        t_long = smooth(long_, si_long)
        if r >= 2:   # the first launches load the code object
            for k, v in zip(ms, (t_ex, t_sm, t_r0, t_long)):
                ms[k].append(v)
    out["kernel_us"] = {k: spread(v, 1e3) for k, v in ms.items()}
    out["smooth_report"], out["smooth_long_report"] = report(short), report(long_)
    out["smooth_over_extract"] = round(float(np.median(ms["smooth"]) / np.median(ms["extract"])), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
