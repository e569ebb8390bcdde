"""Cost of the scan-based people detector (smpc_scan_people_batch), three measurements, one JSON line:
  kernel: HIP-event time of the kernel alone (smpc_last_kernel_ms) on device pointers, B robots with --beams beams and 16 rows
          each, on the pose and the scan of a moving episode (one shared --world x --world floor, sensed costmaps) after --warm
          ticks; beside smpc_people_to_status_batch, smpc_collision_monitor_batch with M = 0 (two zones, no simulation: it
          reads the same two arrays) and a device-to-device copy of the call's input bytes (B x beams x 9), in the same
          loop, alternating: median (min .. max) of --reps rounds, and the call as a multiple of the copy. In the same loop
          the same call with one row per robot and without seg_stats, so that the walk ends where the first row is out.
          With it what the timed call finds: segments, rejections and detections per robot.
  wide:   the same at --wide-B robots x --wide-beams beams.
  tick:   the closed-loop tick of two episodes on the same scenes, both with sensor and tracker, one without this stage (the
          tracker reads the true persons) and one with scan_detector=, each replayed from its HIP graph: --rounds blocks of
          --ticks ticks, alternating between the two; median ms per tick of each and the spread (min .. max) of the blocks.

    python tools/gpu_scan_people.py [--B 8192] [--Np 8] [--world 1024] [--cells 80] [--beams 360] [--warm 12] [--wide-B 64]
                                    [--wide-beams 4096] [--reps 20] [--rounds 7] [--ticks 20] [--no-tick] [--no-wide]
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
    ap.add_argument("--cells", type=int, default=80, help="window side in cells")
    ap.add_argument("--beams", type=int, default=360)
    ap.add_argument("--reach", type=float, default=3.5, help="largest start distance of a person from its robot (scenes_in_world)")
    ap.add_argument("--warm", type=int, default=12)
    ap.add_argument("--wide-B", type=int, default=64)
    ap.add_argument("--wide-beams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--no-tick", action="store_true")
    ap.add_argument("--no-wide", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd._abi import SmpcPeopleBatch
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.params import MonitorParams, OptimizerParams, ScanDetectorParams, SensorParams, TrackerParams
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world, uniform
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point

    prm, sd, tp = OptimizerParams.readme(), ScanDetectorParams(), TrackerParams()
    two_zones = MonitorParams(zones=MonitorParams.nav2_like(0.24).zones[:2], time_before_collision=0.0)
    Nd = sd.max_detections
    out = {"B": a.B, "Np": a.Np, "world": a.world, "cells": a.cells, "beams": a.beams, "Nd": Nd, "warm": a.warm}
    spread = lambda v, scale, digits=2: {"median": round(float(np.median(v)) * scale, digits), "min": round(min(v) * scale, digits),
                                         "max": round(max(v) * scale, digits)}
    world = make_world(a.world, a.world, 0.05)

    def episode(B, beams, **more):
        sc = scenes_in_world(prm, world, B, a.Np, size_x=a.cells, size_y=a.cells, people_reach=a.reach)
        w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
        return BatchEpisode(prm, sc, w_ref, obstacles_from_costmap=True, world=world, sensor=SensorParams(n_beams=beams), tracker=tp, **more)

    def kernel_times(ep, B, beams):
        """The call, its early-ending variant, people_to_status, the monitor without simulation and the copy of the input
        bytes on the state of `ep`, alternating in one loop."""
        s, c = ep.solver, ep._c
        origin = np.asarray(world.origin, np.float64).reshape(2)
        arrays = {"robot_pose": ep.pose, "beam_kind": ep.beam_kind, "beam_cell": ep.beam_cell}
        one_row = point(BatchSolver.scan_people_c(sd, B, beams, 1, 1, world.resolution, origin, ep.sensor), arrays)
        monitor = point(BatchSolver.collision_monitor_c(two_zones, B, beams, 1, world.resolution, origin), dict(arrays, cmd=ep.cmd_vel))
        det1, count1 = torch.zeros(B, 1, 5, dtype=torch.float64, device=ep.dev), torch.zeros(B, dtype=torch.int32, device=ep.dev)
        cmd_out, action = torch.zeros(B, 2, dtype=torch.float64, device=ep.dev), torch.zeros(B, 4, dtype=torch.int32, device=ep.dev)
        src = torch.zeros(B * beams * 9, dtype=torch.uint8, device=ep.dev)
        dst = torch.empty_like(src)
        qb = SmpcPeopleBatch()
        qb.B, qb.Np, qb.N, qb.on_device = B, a.Np, a.Np, 1
        qb.people, qb.count = ep.persons.data_ptr(), ep.person_count.data_ptr()
        ms = {k: [] for k in ("scan_people", "scan_people_one_row_no_stats", "people_to_status", "collision_monitor_M0", "copy_of_the_input_bytes")}
        for r in range(a.reps + 2):
            t = {}
            s.scan_people_device(c.scan_people, ep.scan_persons.data_ptr(), ep.scan_count.data_ptr(), ep.scan_segment.data_ptr(), ep.scan_stats.data_ptr())
            t["scan_people"] = s.last_kernel_ms()
            s.scan_people_device(one_row, det1.data_ptr(), count1.data_ptr())
            t["scan_people_one_row_no_stats"] = s.last_kernel_ms()
            s.people_to_status_device(qb, ep.people.data_ptr(), ep.has_people.data_ptr())
            t["people_to_status"] = s.last_kernel_ms()
            s.collision_monitor_device(monitor, cmd_out.data_ptr(), action.data_ptr())
            t["collision_monitor_M0"] = s.last_kernel_ms()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            t["copy_of_the_input_bytes"] = e0.elapsed_time(e1)
            if r >= 2:   # the first launches load the code object
                for k, v in t.items():
                    ms[k].append(v)
        ep.synchronize()
        stats, count = ep.scan_stats.cpu().numpy(), ep.scan_count.cpu().numpy()
        us = {k: spread(v, 1e3) for k, v in ms.items()}
        us["input_bytes"] = B * beams * 9
        us["scan_people_over_copy"] = round(us["scan_people"]["median"] / us["copy_of_the_input_bytes"]["median"], 2)
        found = dict(zip(("segments", "by_points", "by_width", "accepted"), (round(float(v), 2) for v in stats.mean(axis=0))))
        return us, dict(found, rows=round(float(count.mean()), 2), robots_with_a_detection=int((count > 0).sum()),
                        robots_with_a_row_in_the_one_row_call=int((count1.cpu().numpy() > 0).sum()),
                        true_persons=round(float(ep.person_count.cpu().numpy().mean()), 2))

    # ---- the kernel alone, on the state of an episode after --warm ticks
    ep = episode(a.B, a.beams, scan_detector=sd)
    for _ in range(a.warm):
        ep.tick()
    ep.synchronize()
    out["kernel_us"], out["found_per_robot"] = kernel_times(ep, a.B, a.beams)
    del ep
    if not a.no_wide:
        ep = episode(a.wide_B, a.wide_beams, scan_detector=sd)
        for _ in range(a.warm):
            ep.tick()
        ep.synchronize()
        us, found = kernel_times(ep, a.wide_B, a.wide_beams)
        out["wide"] = {"B": a.wide_B, "beams": a.wide_beams, "kernel_us": us, "found_per_robot": found}
        del ep

    # ---- the tick with and without
    if not a.no_tick:
        eps = {"off": episode(a.B, a.beams), "on": episode(a.B, a.beams, scan_detector=sd)}
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
