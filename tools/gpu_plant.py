"""Cost of the robot plant (smpc_robot_plant_batch), two measurements, one JSON line:
  kernel: HIP-event time of the kernel alone (smpc_last_kernel_ms) on device pointers, B robots with Np persons each on one
          shared --world x --world floor, in steady state: the pose, twist and command queue of a moving episode (reactive
          crowd, plant on) after --warm ticks, restored before every call; beside smpc_people_to_status_batch in the same
          loop, alternating: median (min .. max) of --reps rounds. With it what the timed call does: robots that advanced
          all substeps, robots a contact stopped, robots in wall and in agent contact. In the same loop the same call with
          walls off (world NULL) and with every count at 0 (no agents): the differences are what the two scans cost.
  tick:   the closed-loop tick of two episodes on the same scenes, one with plant=None (the tick without this stage, the
          torch move of pose and speed in its place) and one with the plant, each replayed from its HIP graph: --rounds
          blocks of --ticks ticks, alternating between the two; median ms per tick of each and the spread (min .. max) of
          the blocks.

    python tools/gpu_plant.py [--B 8192] [--Np 8] [--world 1024] [--substeps 8] [--latency 0] [--radius 0.24] [--warm 12] [--reps 20]
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
    ap.add_argument("--substeps", type=int, default=8)
    ap.add_argument("--latency", type=int, default=0)
    ap.add_argument("--radius", type=float, default=0.24, help="robot_radius: 0.24 m is 4 cells of 0.05 m, 0.75 m the largest footprint")
    ap.add_argument("--reach", type=float, default=3.5, help="largest start distance of a person from its robot (scenes_in_world)")
    ap.add_argument("--warm", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--no-tick", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd._abi import SmpcPeopleBatch
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.params import CrowdParams, OptimizerParams, PlantParams
    from nav2_social_mpc_controller_amd.scenes import crowd_waypoints, make_world, scenes_in_world, uniform
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point

    B, Np = a.B, a.Np
    prm, pp = OptimizerParams.readme(), PlantParams(substeps=a.substeps, latency_ticks=a.latency, robot_radius=a.radius)
    out = {"B": B, "Np": Np, "world": a.world, "substeps": a.substeps, "latency_ticks": a.latency, "robot_radius": a.radius, "warm": a.warm}
    spread = lambda v, scale, digits=2: {"median": round(float(np.median(v)) * scale, digits), "min": round(min(v) * scale, digits),
                                         "max": round(max(v) * scale, digits)}
    world = make_world(a.world, a.world, 0.05)
    out["footprint_d2"] = pp.footprint_d2(world.resolution)
    sc = scenes_in_world(prm, world, B, Np, size_x=40, size_y=40, people_reach=a.reach)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    wp, n_wp = crowd_waypoints(scenes_in_world(prm, world, B, Np, size_x=120, size_y=120, people_reach=a.reach), K=2)
    kw = dict(obstacles_from_costmap=True, world=world, crowd=CrowdParams(), person_waypoints=wp, person_n_waypoints=n_wp)

    # ---- the kernel alone, on the state of an episode after --warm ticks
    ep = BatchEpisode(prm, sc, w_ref, plant=pp, **kw)
    for _ in range(a.warm):
        ep.tick()
    ep.synchronize()
    s, c = ep.solver, ep._c
    state = (ep.pose, ep.speed, ep.plant_queue, ep.plant_tick)
    state0 = [t.clone() for t in state]
    qb = SmpcPeopleBatch()
    qb.B, qb.Np, qb.N, qb.on_device = B, Np, Np, 1
    qb.people, qb.count = ep.persons.data_ptr(), ep.person_count.data_ptr()
    no_count = torch.zeros(B, dtype=torch.int32, device=ep.dev)
    variants = {"robot_plant": c.plant,
                "robot_plant_no_walls": point(BatchSolver.plant_c(pp, prm, B, Np, 1), {"cmd": ep.cmd_vel, "agents": ep.persons, "count": ep.person_count}),
                "robot_plant_no_agents": point(BatchSolver.plant_c(pp, prm, B, Np, 1, world.cells_x, world.cells_y, world.resolution, world.origin),
                                               {"world": ep.world_map, "cmd": ep.cmd_vel, "agents": ep.persons, "count": no_count})}
    contact = {k: torch.zeros(B, 2, dtype=torch.int32, device=ep.dev) for k in variants}
    ms = {k: [] for k in list(variants) + ["people_to_status"]}
    for r in range(a.reps + 2):
        t = {}
        for k, pi in variants.items():
            for buf, b0 in zip(state, state0):
                buf.copy_(b0)
            s.robot_plant_device(pi, ep.pose.data_ptr(), ep.speed.data_ptr(), ep.plant_queue.data_ptr(), ep.plant_tick.data_ptr(),
                                 contact[k].data_ptr(), ep.heading_cs.data_ptr())
            t[k] = s.last_kernel_ms()
        s.people_to_status_device(qb, ep.people.data_ptr(), ep.has_people.data_ptr())
        t["people_to_status"] = s.last_kernel_ms()
        if r >= 2:   # the first launches load the code object
            for k, v in t.items():
                ms[k].append(v)
    out["kernel_us"] = {k: spread(v, 1e3) for k, v in ms.items()}
    ep.synchronize()
    got = contact["robot_plant"].cpu().numpy()
    out["steady_state"] = {"advanced_all_substeps": int((got[:, 1] == a.substeps).sum()), "stopped_by_contact": int(((got[:, 0] & 3) != 0).sum()),
                           "in_wall_contact": int(((got[:, 0] & 4) != 0).sum()), "in_agent_contact": int(((got[:, 0] & 8) != 0).sum())}
    del ep

    # ---- the tick with and without
    if not a.no_tick:
        eps = {"off": BatchEpisode(prm, sc, w_ref, **kw), "on": BatchEpisode(prm, sc, w_ref, plant=pp, **kw)}
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
