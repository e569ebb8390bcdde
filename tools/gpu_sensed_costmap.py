"""Cost of the sensed local costmaps (smpc_sensed_costmap_batch), three measurements, one JSON line:
  kernel: HIP-event times (smpc_last_kernel_ms) on device pointers, B robots with Np persons each and --cells x --cells
          windows on one shared --world x --world floor (scenes.make_world, 0.05 m), --beams beams of --range metres, an
          inflation radius of --inflation metres; median (min .. max) of --reps rounds that alternate, in the same loop, with
          smpc_local_costmap_batch under `force`, which stores the same bytes and is the floor; the ratio to that floor.
  phases: the same call on inputs that leave a phase nothing to do, in the same loop:
            store:   one beam of length 0 (nothing is marked: rows without marks are skipped, the windows are still written);
            scan_r0: all beams, an inflation table of one entry (d2_max = 0: a mark costs its own cell only).
          store / (scan_r0 - store) / (full - scan_r0) are given as the shares of store, scan and inflation of the full call.
          These are differences of whole launches, not a profile.
  tick:   the closed-loop tick (arc plans with the plan window, rolling windows, N private persons) of two episodes on the
          same scenes, one with sensor=None (the tick of an episode before this call existed) and one with the sensor,
          eager on one stream: --rounds blocks of --ticks ticks, alternating between the two; median ms per tick of each
          and the spread (min .. max) of the blocks, and the sensed call's own time inside a tick.

    python tools/gpu_sensed_costmap.py [--B 8192] [--Np 8] [--cells 200] [--world 1024] [--beams 360] [--range 2.5] [--inflation 0.7]
                                       [--reps 20] [--rounds 5] [--ticks 20] [--base free|world] [--no-tick]
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
    ap.add_argument("--inflation", type=float, default=0.7)
    ap.add_argument("--base", choices=("free", "world"), default="free")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--no-tick", action="store_true", help="the kernel and its phases only")
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd.episode import BatchEpisode, arc_plans
    from nav2_social_mpc_controller_amd.params import OptimizerParams, SensorParams, TrajectorizerParams
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world, uniform
    from nav2_social_mpc_controller_amd.solver import point

    B, Np, cells = a.B, a.Np, a.cells
    prm = OptimizerParams.readme()
    sp = SensorParams(n_beams=a.beams, max_range=a.range, inflation_radius=a.inflation, base=a.base)
    world = make_world(a.world, a.world, 0.05)
    res = world.resolution
    sc = scenes_in_world(prm, world, B, Np, size_x=cells, size_y=cells, margin=min(6.0, 0.25 * a.world * 0.05))
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    plan, plan_len = arc_plans(sc.pose0, 0.4 * w_ref)
    kw = dict(plan=plan, plan_len=plan_len, traj_params=TrajectorizerParams(desired_linear_vel=0.6, max_time=prm.max_time),
              plan_window=(10.0, 10.0), obstacles_from_costmap=True, world=world)
    table, d2_max = sp.inflation_table(res)
    out = {"B": B, "Np": Np, "cells": cells, "world": a.world, "beams": a.beams, "reach_cells": int(np.abs(sp.beam_cells(res)).max()),
           "r": int(np.sqrt(d2_max)), "base": a.base, "window_bytes": B * cells * cells, "reps": a.reps}

    # ---- the kernel alone, on the state of an episode after a few ticks
    ep = BatchEpisode(prm, sc, w_ref, sensor=sp, **kw)
    for _ in range(3):
        ep.tick()
    ep.synchronize()
    s, c = ep.solver, ep._c
    full = c.sensor
    variant = lambda beams, tab: point(s.sensed_costmap_c(B, Np, cells, cells, world.cells_x, world.cells_y, True, res, 1, int(beams.shape[0]),
                                                          sp.agent_d2(res), int(tab.numel()) - 1, sp.BASES.index(sp.base), ep.outside_cost,
                                                          sp.occlusion_min_cost, sp.unknown_occludes),
                                       {"world": ep.world_map, "world_origin": ep.world_origin, "robot_pose": ep.pose, "people": ep.persons,
                                        "count": ep.person_count, "cell": ep.costmap_cell, "beam_cells": beams, "inflation_cost": tab})
    no_beam = torch.zeros((1, 2), dtype=torch.int32, device=ep.dev)
    one_entry = ep.sensor_table[:1].clone()
    calls = {"sensed": full, "store": variant(no_beam, ep.sensor_table), "scan_r0": variant(ep.sensor_beams, one_entry)}
    scratch = torch.empty_like(ep.costmap)                                  # the variants and the floor write beside the episode's windows
    cell, origin = ep.costmap_cell.clone(), ep.costmap_origin.clone()
    ms = {k: [] for k in list(calls) + ["local_costmap_forced"]}
    for r in range(a.reps + 2):
        t = {}
        for name, si in calls.items():
            s.sensed_costmap_device(si, scratch.data_ptr(), ep.beam_kind.data_ptr() if name != "store" else 0,
                                    ep.beam_cell.data_ptr() if name != "store" else 0)
            t[name] = s.last_kernel_ms()
        s.local_costmap_device(c.roll[True], cell.data_ptr(), scratch.data_ptr(), origin.data_ptr(), 0)
        t["local_costmap_forced"] = s.last_kernel_ms()
        if r >= 2:   # the first launches load the code object
            for k, v in t.items():
                ms[k].append(v)
    out["kernel_us"] = {k: spread(v, 1e3) for k, v in ms.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out["sensed_over_floor"] = round(med["sensed"] / med["local_costmap_forced"], 2)
    out["phase_share"] = {"store": round(med["store"] / med["sensed"], 3),
                          "scan": round((med["scan_r0"] - med["store"]) / med["sensed"], 3),
                          "inflation": round((med["sensed"] - med["scan_r0"]) / med["sensed"], 3)}
    s.sensed_costmap_device(full, ep.costmap.data_ptr(), ep.beam_kind.data_ptr(), ep.beam_cell.data_ptr())
    ep.synchronize()
    kind = ep.beam_kind.cpu().numpy()
    out["beam_kinds"] = {name: int((kind == code).sum()) for code, name in enumerate(("none", "world", "agent", "corner_pair", "invalid", "no_robot"))}
    out["marked_share_of_cells"] = round(float((ep.costmap == 254).double().mean().item()), 5)
    del ep, scratch

    # ---- the tick with and without
    if not a.no_tick:
        eps = {"off": BatchEpisode(prm, sc, w_ref, **kw), "on": BatchEpisode(prm, sc, w_ref, sensor=sp, **kw)}
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
        tm = {}
        eps["on"].tick(timing=tm)
        out["tick_on_sensed_costmap_us"] = round(tm["sensed_costmap_ms"] * 1e3, 2)
        out["tick_on_local_costmap_us"] = round(tm["local_costmap_ms"] * 1e3, 2)
        out["tick_on_solve_us"] = round(tm["solve_ms"] * 1e3, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
