"""Cost of the collision monitor (smpc_collision_monitor_batch), two measurements, one JSON line:
  kernel: HIP-event time of the kernel alone (smpc_last_kernel_ms) on device pointers, on the state of a moving episode
          (sensed costmaps, robot plant, B robots with Np persons each on one shared --world x --world floor) after --warm
          ticks: the pose, the selected command and the scan's beam_kind / beam_cell of that tick. The call with
          MonitorParams.nav2_like (a STOP circle, a SLOWDOWN polygon, an APPROACH footprint over 12 steps), the same call
          without its APPROACH zone (M = 0: the difference is the simulation loop), beside smpc_people_to_status_batch and
          smpc_robot_plant_batch (its state restored before every call) in the same loop, alternating: median (min .. max)
          of --reps rounds. With it what the timed call decides: robots with a ratio < 1, by deciding zone, and the points a
          robot has. Then the same three-zone call at --wide-B robots x --wide-beams beams of a second episode.
  tick:   the closed-loop tick of two episodes on the same scenes, one with monitor=None and one with the preset, each
          replayed from its HIP graph: --rounds blocks of --ticks ticks, alternating between the two; median ms per tick of
          each and the spread (min .. max) of the blocks.

    python tools/gpu_collision_monitor.py [--B 8192] [--Np 8] [--world 1024] [--cells 80] [--beams 360] [--radius 0.24] [--warm 12]
                                          [--wide-B 64] [--wide-beams 4096] [--reps 20] [--rounds 7] [--ticks 20] [--no-tick] [--no-wide]
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
    ap.add_argument("--radius", type=float, default=0.24, help="robot_radius of the preset and the plant")
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
    from nav2_social_mpc_controller_amd.params import MonitorParams, OptimizerParams, PlantParams, SensorParams
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world, uniform
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point

    prm, pp = OptimizerParams.readme(), PlantParams(robot_radius=a.radius)
    preset = MonitorParams.nav2_like(a.radius)
    no_approach = MonitorParams(zones=preset.zones[:2], time_before_collision=0.0)
    out = {"B": a.B, "Np": a.Np, "world": a.world, "cells": a.cells, "beams": a.beams, "robot_radius": a.radius, "warm": a.warm,
           "zones": [f"{z.action} {z.shape}" for z in preset.zones], "M": preset.steps()}
    spread = lambda v, scale, digits=2: {"median": round(float(np.median(v)) * scale, digits), "min": round(min(v) * scale, digits),
                                         "max": round(max(v) * scale, digits)}
    world = make_world(a.world, a.world, 0.05)

    def episode(B, beams, **more):
        sc = scenes_in_world(prm, world, B, a.Np, size_x=a.cells, size_y=a.cells, people_reach=a.reach)
        w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
        return BatchEpisode(prm, sc, w_ref, obstacles_from_costmap=True, world=world, sensor=SensorParams(n_beams=beams), **more)

    def kernel_times(ep, B, beams):
        """The monitor's variants, people_to_status and the plant on the state of `ep`, alternating in one loop."""
        s, c = ep.solver, ep._c
        origin = np.asarray(world.origin, np.float64).reshape(2)
        arrays = {"robot_pose": ep.pose, "cmd": ep.cmd_vel, "beam_kind": ep.beam_kind, "beam_cell": ep.beam_cell}
        variants = {"collision_monitor": c.monitor,
                    "collision_monitor_no_approach": point(BatchSolver.collision_monitor_c(no_approach, B, beams, 1, world.resolution, origin), arrays)}
        Z = len(preset.zones)
        bufs = {k: (torch.zeros(B, 2, dtype=torch.float64, device=ep.dev), torch.zeros(B, 4, dtype=torch.int32, device=ep.dev),
                    torch.zeros(B, Z, dtype=torch.int32, device=ep.dev), torch.zeros(B, dtype=torch.float64, device=ep.dev)) for k in variants}
        state = (ep.pose, ep.speed, ep.plant_queue, ep.plant_tick)
        state0 = [t.clone() for t in state]
        qb = SmpcPeopleBatch()
        qb.B, qb.Np, qb.N, qb.on_device = B, a.Np, a.Np, 1
        qb.people, qb.count = ep.persons.data_ptr(), ep.person_count.data_ptr()
        ms = {k: [] for k in list(variants) + ["people_to_status", "robot_plant"]}
        for r in range(a.reps + 2):
            t = {}
            for k, mi in variants.items():
                cmd_out, action, points, ratio = bufs[k]
                s.collision_monitor_device(mi, cmd_out.data_ptr(), action.data_ptr(), points.data_ptr(), ratio.data_ptr())
                t[k] = s.last_kernel_ms()
            s.people_to_status_device(qb, ep.people.data_ptr(), ep.has_people.data_ptr())
            t["people_to_status"] = s.last_kernel_ms()
            s.robot_plant_device(c.plant, ep.pose.data_ptr(), ep.speed.data_ptr(), ep.plant_queue.data_ptr(), ep.plant_tick.data_ptr(),
                                 ep.plant_contact.data_ptr(), ep.heading_cs.data_ptr())
            t["robot_plant"] = s.last_kernel_ms()
            for buf, b0 in zip(state, state0):   # the plant moved the robots: back to the tick's pose for the next round
                buf.copy_(b0)
            if r >= 2:   # the first launches load the code object
                for k, v in t.items():
                    ms[k].append(v)
        ep.synchronize()
        action = bufs["collision_monitor"][1].cpu().numpy()
        ratio = bufs["collision_monitor"][3].cpu().numpy()
        decided = {f"by_zone_{z}": int((action[:, 1] == z).sum()) for z in range(Z)}
        return {k: spread(v, 1e3) for k, v in ms.items()}, dict(decided, ratio_below_1=int((ratio < 1.0).sum()), stopped=int((ratio == 0.0).sum()),
                                                               mean_points=round(float(action[:, 3].mean()), 1), robots_with_points=int((action[:, 3] > 0).sum()))

    # ---- the kernel alone, on the state of an episode after --warm ticks
    ep = episode(a.B, a.beams, plant=pp, monitor=preset)
    for _ in range(a.warm):
        ep.tick()
    ep.synchronize()
    out["kernel_us"], out["decisions"] = kernel_times(ep, a.B, a.beams)
    del ep
    if not a.no_wide:
        ep = episode(a.wide_B, a.wide_beams, plant=pp, monitor=preset)
        for _ in range(a.warm):
            ep.tick()
        ep.synchronize()
        us, decisions = kernel_times(ep, a.wide_B, a.wide_beams)
        out["wide"] = {"B": a.wide_B, "beams": a.wide_beams, "kernel_us": us, "decisions": decisions}
        del ep

    # ---- the tick with and without
    if not a.no_tick:
        eps = {"off": episode(a.B, a.beams, plant=pp), "on": episode(a.B, a.beams, plant=pp, monitor=preset)}
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
