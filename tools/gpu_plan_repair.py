"""Cost of the plan repair (smpc_repair_plan_batch), two measurements, one JSON line:
  kernel: HIP-event time of the call's two kernels (smpc_last_kernel_ms) on device pointers, B robots with --cells x --cells
          windows, --beams beams and a region of PlanRepairParams().radius (60 cells of 0.05 m), on the pose, the sensed windows,
          the plans and the plan starts of a moving episode (one shared --world x --world floor, arc plans, sensed costmaps)
          after --warm ticks; the plans are put back before every call, since the call edits them. Three variants of the call:
          on that state's own windows (the share of robots with each status is reported), on empty windows (every plan clear:
          the judging kernel and the field kernel's look at B status words) and on windows with a lethal block on every plan
          1 m ahead of its robot (every robot relaxes a field); beside smpc_transform_global_plan_batch, which reads the same
          plans, in the same loop, alternating: median (min .. max) of --reps rounds.
  tick:   the closed-loop tick of two episodes on the same scenes, both with sensor and plan window, one with repair=, each
          replayed from its HIP graph: --rounds blocks of --ticks ticks, alternating between the two; median ms per tick of
          each and the spread (min .. max) of the blocks, and the statuses of the last tick.

    python tools/gpu_plan_repair.py [--B 8192] [--Np 8] [--world 1024] [--cells 200] [--beams 360] [--warm 12] [--reps 20]
                                    [--rounds 7] [--ticks 20] [--no-tick]
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
    ap.add_argument("--cells", type=int, default=200, help="window side in cells")
    ap.add_argument("--beams", type=int, default=360)
    ap.add_argument("--reach", type=float, default=3.5, help="largest start distance of a person from its robot (scenes_in_world)")
    ap.add_argument("--warm", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--no-tick", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd._abi_plan_repair import REPAIR_STATUS
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, arc_plans
    from nav2_social_mpc_controller_amd.params import OptimizerParams, PlanRepairParams, SensorParams, TrajectorizerParams
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world, uniform
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point

    prm, rp = OptimizerParams.readme(), PlanRepairParams()
    tp = TrajectorizerParams(desired_linear_vel=prm.desired_linear_vel, max_time=prm.max_time, time_step=prm.time_step)
    world = make_world(a.world, a.world, 0.05)
    out = {"B": a.B, "Np": a.Np, "world": a.world, "cells": a.cells, "beams": a.beams, "radius_cells": rp.radius_cells(world.resolution),
           "stride": rp.stride, "warm": a.warm}
    spread = lambda v, scale, digits=2: {"median": round(float(np.median(v)) * scale, digits), "min": round(min(v) * scale, digits),
                                         "max": round(max(v) * scale, digits)}
    shares = lambda status: {REPAIR_STATUS[i].lower(): round(float((status == i).mean()), 4) for i in range(len(REPAIR_STATUS)) if (status == i).any()}

    def episode(**more):
        sc = scenes_in_world(prm, world, a.B, a.Np, size_x=a.cells, size_y=a.cells, people_reach=a.reach)
        w_ref = (uniform(0x5EED0001, np.arange(a.B), 6)[:, 0] * 2.0 - 1.0) * 0.6
        plan, plan_len = arc_plans(sc.pose0, 0.1 * w_ref)
        return BatchEpisode(prm, sc, w_ref, obstacles_from_costmap=True, world=world, sensor=SensorParams(n_beams=a.beams), plan=plan,
                            plan_len=plan_len, traj_params=tp, plan_window=(4.0, 10.0), **more)

    # ---- the call alone, on the state of an episode after --warm ticks (without repair=: the plans are the arcs still)
    ep = episode()
    for _ in range(a.warm):
        ep.tick()
    ep.synchronize()
    s, c, B, L = ep.solver, ep._c, a.B, int(ep.plan.shape[1])
    plan0, len0 = ep.plan.clone(), ep.plan_len.clone()
    scratch, status = torch.zeros_like(ep.plan), torch.zeros(B, dtype=torch.int32, device=ep.dev)
    info = torch.zeros(B, 4, dtype=torch.int32, device=ep.dev)
    # a lethal block of 3 x 3 cells on every plan, 1 m (20 poses) behind the pose nearest the robot
    pose, plan = ep.pose.cpu().numpy(), plan0.cpu().numpy()
    origin, start = ep.costmap_origin.cpu().numpy(), ep.plan_start.cpu().numpy()
    near = np.array([start[b] + np.argmin(((plan[b, start[b]:] - pose[b, :2]) ** 2).sum(axis=1)) for b in range(B)])
    spot = plan[np.arange(B), np.minimum(near + 20, L - 1)]
    cell = np.clip(np.floor((spot - origin) / world.resolution).astype(np.int64), 1, a.cells - 2)
    blocked = ep.costmap.clone()
    rows = torch.arange(B, device=ep.dev)
    cx, cy = torch.from_numpy(cell[:, 0]).to(ep.dev), torch.from_numpy(cell[:, 1]).to(ep.dev)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            blocked[rows, cy + dy, cx + dx] = 254
    maps = {"own_windows": ep.costmap, "every_plan_clear": torch.zeros_like(ep.costmap), "every_plan_blocked": blocked}
    calls = {k: point(BatchSolver.repair_plan_c(rp, B, L, a.cells, a.cells, False, world.resolution, 1),
                      {"costmap": m, "costmap_origin": ep.costmap_origin, "robot_pose": ep.pose, "plan_start": ep.plan_start}) for k, m in maps.items()}
    window, window_len, window_err = torch.zeros_like(ep.plan), torch.zeros_like(ep.plan_len), torch.zeros_like(ep.plan_len)
    start0 = ep.plan_start.clone()
    ms = {k: [] for k in list(calls) + ["transform_global_plan"]}
    found = {}
    for r in range(a.reps + 2):
        t = {}
        for k, ri in calls.items():
            ep.plan.copy_(plan0)
            ep.plan_len.copy_(len0)
            s.repair_plan_device(ri, ep.plan.data_ptr(), ep.plan_len.data_ptr(), scratch.data_ptr(), status.data_ptr(), info.data_ptr())
            t[k] = s.last_kernel_ms()
            if r == 0:
                st, nf = status.cpu().numpy(), info.cpu().numpy()
                found[k] = dict(shares(st), mean_walk_cells=round(float(nf[st == 1, 3].mean()), 1) if (st == 1).any() else None,
                                mean_rows_added=round(float((ep.plan_len.cpu().numpy() - len0.cpu().numpy())[st == 1].mean()), 1) if (st == 1).any() else None)
        ep.plan.copy_(plan0)
        ep.plan_len.copy_(len0)
        ep.plan_start.copy_(start0)
        s.transform_global_plan_device(c.window, window.data_ptr(), window_len.data_ptr(), window_err.data_ptr())
        t["transform_global_plan"] = s.last_kernel_ms()
        if r >= 2:   # the first launches load the code object
            for k, v in t.items():
                ms[k].append(v)
    ep.synchronize()
    out["kernel_us"] = {k: spread(v, 1e3) for k, v in ms.items()}
    out["status_shares"] = found
    blocked_robots = B * (1.0 - found["every_plan_blocked"].get("clear", 0.0))
    out["us_per_blocked_robot_at_full_occupancy"] = round((out["kernel_us"]["every_plan_blocked"]["median"] - out["kernel_us"]["every_plan_clear"]["median"])
                                                          / max(blocked_robots, 1.0), 4)
    del ep, maps, blocked, calls

    # ---- the tick with and without
    if not a.no_tick:
        eps = {"off": episode(), "on": episode(repair=rp)}
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
        out["tick_last_status_shares"] = shares(eps["on"].repair_status.cpu().numpy())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
