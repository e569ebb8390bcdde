"""Cost of the reactive crowd step of a shared world's pedestrians (smpc_crowd_pool_step_batch), two measurements, one JSON line:
  call:  HIP-event time of the call's kernels (smpc_last_kernel_ms) on device pointers, a pool of pedestrians followed by B
         static rows (the robots) on a synthetic --extent x --extent metre floor (uniform positions, speeds up to 1 m/s, one
         waypoint each, no obstacle grid), at tools/gpu_nearest.py's two densities: `dense` (--dense-pool, --dense-range) and
         `sparse` (--sparse-pool, --sparse-range). Per density, alternating in one loop: the step with bins_ready = 0 (it bins
         the table itself) and with bins_ready = 1 (the step kernel alone, on the bins of the gather just before it),
         smpc_nearest_people_batch for the B robots, and the private smpc_crowd_step_batch on B x Np persons for context:
         median (min .. max) of --reps rounds. With it the in-range pair terms of the step (all pairs of a sample of 256
         movers, scaled) and the terms per microsecond of the bins_ready = 1 step.
  tick:  the closed-loop tick of tools/gpu_nearest.py's episode set-up (arc stand-in, rolling 40 x 40 windows on a --world x
         --world floor, one shared pool of B * Np pedestrians), each replayed from its HIP graph: the constant-velocity pool
         against the reactive pool (pool_crowd=PoolCrowdParams(interaction_range=--loop-reach)): --rounds blocks of --ticks
         ticks, alternating; median ms per tick and the spread (min .. max) of the blocks; then one eager tick's stage times.

    python tools/gpu_crowd_pool.py [--B 8192] [--Np 8] [--extent 200] [--dense-pool 65536] [--dense-range 5] [--sparse-pool 4096]
                                   [--sparse-range 10] [--world 1024] [--loop-range 10] [--loop-reach 5] [--reps 20] [--rounds 7]
                                   [--ticks 20] [--no-tick]
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
    ap.add_argument("--extent", type=float, default=200.0)
    ap.add_argument("--dense-pool", type=int, default=65536)
    ap.add_argument("--dense-range", type=float, default=5.0)
    ap.add_argument("--sparse-pool", type=int, default=4096)
    ap.add_argument("--sparse-range", type=float, default=10.0)
    ap.add_argument("--world", type=int, default=1024)
    ap.add_argument("--loop-range", type=float, default=10.0)
    ap.add_argument("--loop-reach", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--no-tick", action="store_true", help="the call alone")
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.params import CrowdParams, OptimizerParams, PoolCrowdParams, SharedWorldParams
    from nav2_social_mpc_controller_amd.scenes import make_world, pool_waypoints, scenes_in_world, shared_pool, uniform
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point

    B, Np = a.B, a.Np
    prm = OptimizerParams.readme()
    out = {"B": B, "Np": Np, "extent": a.extent}
    spread = lambda v, scale, digits=2: {"median": round(float(np.median(v)) * scale, digits), "min": round(min(v) * scale, digits),
                                         "max": round(max(v) * scale, digits)}
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    s = BatchSolver(prm, device=0)
    s.set_stream(torch.cuda.current_stream("cuda:0").cuda_stream)

    # the private crowd step on B x Np persons, for context (the same launch in every loop below)
    g = np.random.default_rng(1)
    persons = np.zeros((B, Np, 5))
    persons[..., 0:2], persons[..., 2:4] = g.uniform(-3.0, 3.0, (B, Np, 2)), g.uniform(-0.6, 0.6, (B, Np, 2))
    d_persons, d_pcur = dev(persons), torch.zeros((B, Np), dtype=torch.int32, device="cuda:0")
    cb = point(BatchSolver.crowd_c(CrowdParams(), B, Np, 1, prm.dt, 1),
               {"robot_pose": dev(np.zeros((B, 3))), "robot_twist": dev(np.zeros((B, 2))), "count": dev(np.full(B, Np, np.int32)),
                "waypoints": dev(g.uniform(-3.0, 3.0, (B, Np, 1, 2))), "n_waypoints": dev(np.ones((B, Np), np.int32))})

    for name, M, rng in (("dense", a.dense_pool, a.dense_range), ("sparse", a.sparse_pool, a.sparse_range)):
        g = np.random.default_rng(M)
        A = M + B
        agents = np.zeros((A, 5))
        agents[:, 0:2] = g.uniform(0.0, a.extent, (A, 2))
        agents[:, 2:4] = g.uniform(-1.0, 1.0, (A, 2)) / np.sqrt(2.0)
        pose = np.concatenate([agents[M:, 0:2], g.uniform(-3.0, 3.0, (B, 1))], axis=1)
        bin_size = max(float(np.float64(rng) * np.float64(1.0 + 2.0 ** -20)), a.extent / 256.0)
        gx = gy = max(1, int(np.ceil(a.extent / bin_size)))
        d_agents, d_pose, d_self = dev(agents), dev(pose), dev(np.arange(M, A, dtype=np.int32))
        ws = torch.zeros(s.nearest_workspace_bytes(A, gx, gy), dtype=torch.uint8, device="cuda:0")
        people, count = torch.zeros((B, Np, 5), dtype=torch.float64, device="cuda:0"), torch.zeros(B, dtype=torch.int32, device="cuda:0")
        ni = point(BatchSolver.nearest_c(B, Np, A, gx, gy, [0.0, 0.0], bin_size, rng, 1),
                   {"agents": d_agents, "robot_pose": d_pose, "self": d_self, "workspace": ws})
        ni.workspace_bytes = int(ws.numel())
        nxt, cur = torch.zeros((M, 5), dtype=torch.float64, device="cuda:0"), torch.zeros(M, dtype=torch.int32, device="cuda:0")
        arrays = {"agents": d_agents, "waypoints": dev(g.uniform(0.0, a.extent, (M, 1, 2))), "n_waypoints": dev(np.ones(M, np.int32)),
                  "workspace": ws}
        steps = {}
        for ready in (0, 1):
            ci = point(BatchSolver.crowd_pool_c(PoolCrowdParams(interaction_range=rng), M, A, 1, prm.dt, gx, gy, [0.0, 0.0], bin_size, 1,
                                                bins_ready=ready), arrays)
            ci.workspace_bytes = int(ws.numel())
            steps[ready] = ci
        ms = {"step_bins_ready_0": [], "nearest_people": [], "step_bins_ready_1": [], "private_crowd_step": []}
        for r in range(a.reps + 2):
            t = {}
            s.crowd_pool_step_device(steps[0], nxt.data_ptr(), cur.data_ptr())
            t["step_bins_ready_0"] = s.last_kernel_ms()
            s.nearest_people_device(ni, people.data_ptr(), count.data_ptr(), 0)
            t["nearest_people"] = s.last_kernel_ms()
            s.crowd_pool_step_device(steps[1], nxt.data_ptr(), cur.data_ptr())    # on the bins the gather just built
            t["step_bins_ready_1"] = s.last_kernel_ms()
            s.crowd_step_device(cb, d_persons.data_ptr(), d_pcur.data_ptr())
            t["private_crowd_step"] = s.last_kernel_ms()
            if r >= 2:   # the first launches load the code object
                for k, v in t.items():
                    ms[k].append(v)
        torch.cuda.synchronize()
        res = {"pool": M, "agents": A, "interaction_range": rng, "bins": [gx, gy], "bin_size": round(bin_size, 6),
               "kernel_us": {k: spread(v, 1e3) for k, v in ms.items()}}
        sample = g.choice(M, min(M, 256), replace=False)
        d2 = (agents[None, :, 0] - agents[sample, None, 0]) ** 2 + (agents[None, :, 1] - agents[sample, None, 1]) ** 2
        partners = float((d2 <= rng * rng).sum(axis=1).mean()) - 1.0                # less the mover itself
        res["mean_partners"] = round(partners, 1)
        res["pair_terms"] = int(partners * M)
        res["pair_terms_per_us"] = round(partners * M / res["kernel_us"]["step_bins_ready_1"]["median"], 1)
        out[name] = res
        del ws, d_agents, nxt, cur

    # ---- the tick: the constant-velocity pool against the reactive pool
    if not a.no_tick:
        world = make_world(a.world, a.world, 0.05)
        sc = scenes_in_world(prm, world, B, Np, size_x=40, size_y=40)
        w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
        pool = shared_pool(world, B * Np)
        wp, n_wp = pool_waypoints(world, pool)
        sp = SharedWorldParams(max_range=a.loop_range)
        kw = dict(obstacles_from_costmap=True, world=world, shared=sp, pool=pool)
        eps = {"constant_velocity": BatchEpisode(prm, sc, w_ref, **kw),
               "reactive": BatchEpisode(prm, sc, w_ref, pool_crowd=PoolCrowdParams(interaction_range=a.loop_reach), pool_waypoints=wp,
                                        pool_n_waypoints=n_wp, **kw)}
        out["tick"] = {"world": a.world, "pool": B * Np, "max_range": a.loop_range, "interaction_range": a.loop_reach,
                       "bins": list(eps["reactive"].shared_grid[:2])}
        for e in eps.values():
            e.capture_graph()
        blocks = {k: [] for k in eps}
        for r in range(a.rounds + 1):
            for name, e in eps.items():
                e.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.ticks):
                    e.replay()
                e.synchronize()
                if r >= 1:   # one warm-up round
                    blocks[name].append((time.perf_counter() - t0) / a.ticks * 1e3)
        out["tick"]["ms_graph"] = {k: spread(v, 1.0, 4) for k, v in blocks.items()}
        timing = {}
        eps["reactive"].tick(timing=timing)
        out["tick"]["stage_us"] = {k[:-3]: round(v * 1e3, 1) for k, v in timing.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
