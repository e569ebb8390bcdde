"""Cost of the sensed local costmaps with memory (smpc_obstacle_memory_batch), two measurements, one JSON line:
  kernel: HIP-event times (smpc_last_kernel_ms) on device pointers, B robots with Np persons each and --cells x --cells
          windows on one shared --world x --world floor (scenes.make_world, 0.05 m), --beams beams, marks out to --range
          metres and clearing out to --raytrace metres, an inflation radius of --inflation metres; median (min .. max) of
          --reps rounds that alternate, in the same loop, between
            memory_steady: the call on the state of a moving episode after --warm ticks (the state the last of those ticks
                           read, put back before every launch, so that the roll moves what that tick moved);
            memory_zero:   the same call on zeroed memory;
            sensed_equal:  smpc_sensed_costmap_batch on the same beams of --raytrace metres (the yardstick);
            sensed_own:    smpc_sensed_costmap_batch on its own beams of --range metres.
          steady_over_sensed_equal is the ratio of the first to the third; the differences of whole launches say where it
          goes: (memory_zero - sensed_equal) is the state traffic, the clearing reads and the rowany pass, (memory_steady -
          memory_zero) is what a populated memory adds (clears, more marks to inflate), (sensed_equal - sensed_own) the
          longer beams. Not a profile.
  tick:   the closed-loop tick (arc plans with the plan window, rolling windows, N private persons) of two episodes on the
          same scenes, both with the sensor, one with sensor_memory=None and one with it, eager on one stream: --rounds
          blocks of --ticks ticks, alternating between the two; median ms per tick of each and the spread (min .. max) of
          the blocks, and the call's own time inside a tick.

    python tools/gpu_obstacle_memory.py [--B 8192] [--Np 8] [--cells 200] [--world 1024] [--beams 360] [--range 2.5] [--raytrace 3.0]
                                        [--footprint 0.24] [--inflation 0.7] [--warm 12] [--reps 20] [--rounds 5] [--ticks 20] [--no-tick]
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
    ap.add_argument("--Np", type=int, default=8)
    ap.add_argument("--cells", type=int, default=200)
    ap.add_argument("--world", type=int, default=1024)
    ap.add_argument("--beams", type=int, default=360)
    ap.add_argument("--range", type=float, default=2.5)
    ap.add_argument("--raytrace", type=float, default=3.0)
    ap.add_argument("--footprint", type=float, default=0.24)
    ap.add_argument("--inflation", type=float, default=0.7)
    ap.add_argument("--warm", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--no-tick", action="store_true", help="the kernels only")
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd.episode import BatchEpisode, arc_plans
    from nav2_social_mpc_controller_amd.params import ObstacleMemoryParams, OptimizerParams, SensorParams, TrajectorizerParams
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world, uniform
    from nav2_social_mpc_controller_amd.solver import point

    B, Np, cells = a.B, a.Np, a.cells
    prm = OptimizerParams.readme()
    sp = SensorParams(n_beams=a.beams, max_range=a.range, inflation_radius=a.inflation)
    mp = ObstacleMemoryParams(raytrace_range=a.raytrace, footprint_radius=a.footprint)
    world = make_world(a.world, a.world, 0.05)
    res = world.resolution
    sc = scenes_in_world(prm, world, B, Np, size_x=cells, size_y=cells, margin=min(6.0, 0.25 * a.world * 0.05))
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    kw = dict(plan=plan, plan_len=plan_len, traj_params=TrajectorizerParams(desired_linear_vel=0.6, max_time=prm.max_time),
              plan_window=(10.0, 10.0), obstacles_from_costmap=True, world=world, sensor=sp)
    out = {"B": B, "Np": Np, "cells": cells, "world": a.world, "beams": a.beams, "mark_cells": int(np.abs(sp.beam_cells(res)).max()),
           "reach_cells": int(np.abs(mp.beam_cells(sp, res)).max()), "mark_d2": mp.mark_d2(sp, res), "footprint_d2": mp.footprint_d2(res),
           "r": int(np.sqrt(sp.inflation_table(res)[1])), "window_bytes": B * cells * cells,
           "state_bytes": B * cells * ((cells + 31) // 32) * 4, "warm_ticks": a.warm, "reps": a.reps}

    # ---- the kernels alone, on the state of an episode after --warm ticks
    ep = BatchEpisode(prm, sc, w_ref, sensor_memory=mp, **kw)
    for _ in range(a.warm - 1):
        ep.tick()
    before = (ep.obstacle_memory.clone(), ep.obstacle_memory_cell.clone())   # what the last warm tick reads
    ep.tick()
    ep.synchronize()
    s, c = ep.solver, ep._c
    own_beams = torch.from_numpy(sp.beam_cells(res)).to(ep.dev)
    sensed_own = point(s.sensed_costmap_c(B, Np, cells, cells, world.cells_x, world.cells_y, True, res, 1, a.beams, sp.agent_d2(res),
                                          int(ep.sensor_table.numel()) - 1, 0, ep.outside_cost, sp.occlusion_min_cost, sp.unknown_occludes),
                       {"world": ep.world_map, "world_origin": ep.world_origin, "robot_pose": ep.pose, "people": ep.persons,
                        "count": ep.person_count, "cell": ep.costmap_cell, "beam_cells": own_beams, "inflation_cost": ep.sensor_table})
    scratch = torch.empty_like(ep.costmap)                                  # every variant writes beside the episode's windows
    memory, memory_cell = torch.empty_like(before[0]), torch.empty_like(before[1])
    names = ("memory_steady", "memory_zero", "sensed_equal", "sensed_own")
    ms = {k: [] for k in names}
    for r in range(a.reps + 2):
        t = {}
        for name in names:
            if name == "memory_steady":
                memory.copy_(before[0]); memory_cell.copy_(before[1])
            elif name == "memory_zero":
                memory.zero_(); memory_cell.zero_()
            if name.startswith("memory"):
                s.obstacle_memory_device(c.sensor_memory, memory.data_ptr(), memory_cell.data_ptr(), scratch.data_ptr(), ep.beam_kind.data_ptr(),
                                         ep.beam_cell.data_ptr())
            else:
                s.sensed_costmap_device(c.sensor if name == "sensed_equal" else sensed_own, scratch.data_ptr(), ep.beam_kind.data_ptr(),
                                        ep.beam_cell.data_ptr())
            t[name] = s.last_kernel_ms()
        if r >= 2:   # the first launches load the code object
            for k, v in t.items():
                ms[k].append(v)
    out["kernel_us"] = {k: spread(v, 1e3) for k, v in ms.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out["steady_over_sensed_equal"] = round(med["memory_steady"] / med["sensed_equal"], 3)
    out["steady_over_sensed_own"] = round(med["memory_steady"] / med["sensed_own"], 3)
    out["split_us"] = {"longer_beams": round((med["sensed_equal"] - med["sensed_own"]) * 1e3, 2),
                       "state_reads_rowany": round((med["memory_zero"] - med["sensed_equal"]) * 1e3, 2),
                       "populated_memory": round((med["memory_steady"] - med["memory_zero"]) * 1e3, 2)}
    ep.synchronize()
    bits = ep.obstacle_memory.cpu().numpy().view(np.uint32)
    marked = int(np.unpackbits(bits.view(np.uint8)).sum())
    out["marked_share_of_cells"] = round(marked / (B * cells * cells), 5)
    out["lethal_share_of_cells"] = round(float((ep.costmap == 254).double().mean().item()), 5)
    del ep, scratch, memory

    # ---- the tick with and without
    if not a.no_tick:
        eps = {"off": BatchEpisode(prm, sc, w_ref, **kw), "on": BatchEpisode(prm, sc, w_ref, sensor_memory=mp, **kw)}
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
        out["tick_rounds"], out["tick_ticks"] = a.rounds, a.ticks
        tm, tm_off = {}, {}
        eps["on"].tick(timing=tm)
        eps["off"].tick(timing=tm_off)
        out["tick_on_obstacle_memory_us"] = round(tm["obstacle_memory_ms"] * 1e3, 2)
        out["tick_off_sensed_costmap_us"] = round(tm_off["sensed_costmap_ms"] * 1e3, 2)
        out["tick_on_solve_us"] = round(tm["solve_ms"] * 1e3, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
