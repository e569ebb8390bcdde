"""Cost of the nearest-agent gather of a shared world (smpc_nearest_people_batch), two measurements, one JSON line:
  call:  HIP-event time of the call's kernels (smpc_last_kernel_ms) on device pointers, B robots taking their Np nearest out of
         one table (a pool of pedestrians followed by the robots themselves) on a synthetic --extent x --extent metre floor
         (uniform positions; no map is needed), at two densities: `dense` (--dense-pool agents, --dense-range metres) and
         `sparse` (--sparse-pool, --sparse-range). Per density, alternating in one loop: the whole call, the call for ONE
         robot (memset + count + scan + scatter + a one-wave query: the binning passes), smpc_people_to_status_batch and
         smpc_visible_people_batch (on an empty map of 0.05 m cells) on the gathered rows: median (min .. max) of --reps
         rounds; query = whole call - binning. With it the mean number of candidates a robot examines (the population of
         its 3 x 3 bins) and of agents that qualify (from a sample of 256 robots), and the byte floor A * 40 B + B * Np * 44 B.
  tick:  the closed-loop tick (arc stand-in, rolling 40 x 40 windows on a --world x --world floor, constant-velocity persons)
         of episodes on the same robots, each replayed from its HIP graph: private crowds of Np persons per robot against
         one shared pool of B * Np pedestrians (shared=SharedWorldParams(max_range=--loop-range)), both without and with
         metrics (with metrics a shared tick gathers twice): --rounds blocks of --ticks ticks, alternating; median ms per tick
         and the spread (min .. max) of the blocks.

    python tools/gpu_nearest.py [--B 8192] [--Np 8] [--extent 200] [--dense-pool 65536] [--dense-range 5] [--sparse-pool 4096]
                                [--sparse-range 10] [--world 1024] [--loop-range 10] [--reps 20] [--rounds 7] [--ticks 20] [--no-tick]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--no-tick", action="store_true", help="the call alone")
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd._abi import SmpcPeopleBatch
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.params import MetricsParams, OptimizerParams, SharedWorldParams, VisibilityParams
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world, shared_pool, uniform
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point

    B, Np = a.B, a.Np
    prm = OptimizerParams.readme()
    out = {"B": B, "Np": Np, "extent": a.extent}
    spread = lambda v, scale, digits=2: {"median": round(float(np.median(v)) * scale, digits), "min": round(min(v) * scale, digits),
                                         "max": round(max(v) * scale, digits)}
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    s = BatchSolver(prm, device=0)
    s.set_stream(torch.cuda.current_stream("cuda:0").cuda_stream)

    # ---- the call alone, at two densities
    cells = int(np.ceil(a.extent / 0.05))
    empty_map, map_origin = torch.zeros((cells, cells), dtype=torch.uint8, device="cuda:0"), dev(np.zeros((1, 2)))
    for name, M, max_range in (("dense", a.dense_pool, a.dense_range), ("sparse", a.sparse_pool, a.sparse_range)):
        g = np.random.default_rng(M)
        A = M + B
        agents = np.zeros((A, 5))
        agents[:, 0:2] = g.uniform(0.0, a.extent, (A, 2))
        agents[:, 2:4] = g.uniform(-1.0, 1.0, (A, 2))
        pose = np.concatenate([agents[M:, 0:2], g.uniform(-3.0, 3.0, (B, 1))], axis=1)
        bin_size = max(float(np.float64(max_range) * np.float64(1.0 + 2.0 ** -20)), a.extent / 256.0)
        gx = gy = max(1, int(np.ceil(a.extent / bin_size)))
        d_agents, d_pose, d_self = dev(agents), dev(pose), dev(np.arange(M, A, dtype=np.int32))
        ws = torch.zeros(s.nearest_workspace_bytes(A, gx, gy), dtype=torch.uint8, device="cuda:0")
        people, count = torch.zeros((B, Np, 5), dtype=torch.float64, device="cuda:0"), torch.zeros(B, dtype=torch.int32, device="cuda:0")
        source = torch.zeros((B, Np), dtype=torch.int32, device="cuda:0")
        calls = {}
        for key, robots in (("call", B), ("binning", 1)):
            ni = point(BatchSolver.nearest_c(robots, Np, A, gx, gy, [0.0, 0.0], bin_size, max_range, 1),
                       {"agents": d_agents, "robot_pose": d_pose, "self": d_self, "workspace": ws})
            ni.workspace_bytes = int(ws.numel())
            calls[key] = ni
        qb = SmpcPeopleBatch()
        qb.B, qb.Np, qb.N, qb.on_device = B, Np, Np, 1
        qb.people, qb.count = people.data_ptr(), count.data_ptr()
        status, has = torch.zeros((B, Np, 6), dtype=torch.float64, device="cuda:0"), torch.zeros(B, dtype=torch.uint8, device="cuda:0")
        vi = point(BatchSolver.visibility_c(VisibilityParams(max_range=max_range), B, Np, cells, cells, True, 0.05, 1),
                   {"world": empty_map, "world_origin": map_origin, "robot_pose": d_pose, "people": people, "count": count})
        seen_rows, seen_count = torch.zeros_like(people), torch.zeros_like(count)
        ms = {"call": [], "binning": [], "people_to_status": [], "visible_people": []}
        for r in range(a.reps + 2):
            t = {}
            s.nearest_people_device(calls["call"], people.data_ptr(), count.data_ptr(), source.data_ptr())
            t["call"] = s.last_kernel_ms()
            s.nearest_people_device(calls["binning"], people.data_ptr(), count.data_ptr(), source.data_ptr())
            t["binning"] = s.last_kernel_ms()
            s.people_to_status_device(qb, status.data_ptr(), has.data_ptr())
            t["people_to_status"] = s.last_kernel_ms()
            s.visible_people_device(vi, seen_rows.data_ptr(), seen_count.data_ptr(), 0)
            t["visible_people"] = s.last_kernel_ms()
            if r >= 2:   # the first launches load the code object
                for k, v in t.items():
                    ms[k].append(v)
        torch.cuda.synchronize()
        res = {"pool": M, "agents": A, "max_range": max_range, "bins": [gx, gy], "bin_size": round(bin_size, 6),
               "kernel_us": {k: spread(v, 1e3) for k, v in ms.items()}}
        res["kernel_us"]["query"] = round(res["kernel_us"]["call"]["median"] - res["kernel_us"]["binning"]["median"], 2)
        # what a robot examines: the population of its 3 x 3 bins; what qualifies: a sample of 256 robots, all pairs
        bins = lambda p, n: np.clip(np.floor(p / bin_size), 0, n - 1).astype(np.int64)
        pop = np.zeros((gy + 2, gx + 2))
        np.add.at(pop, (bins(agents[:, 1], gy) + 1, bins(agents[:, 0], gx) + 1), 1)
        ry, rx = bins(pose[:, 1], gy) + 1, bins(pose[:, 0], gx) + 1
        res["mean_examined"] = round(float(np.mean(sum(pop[ry + dy, rx + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)))), 1)
        sample = g.choice(B, min(B, 256), replace=False)
        d2 = (agents[None, :, 0] - pose[sample, None, 0]) ** 2 + (agents[None, :, 1] - pose[sample, None, 1]) ** 2
        res["mean_qualifying"] = round(float((d2 <= max_range * max_range).sum(axis=1).mean()) - 1.0, 1)   # less the robot itself
        res["mean_count"] = round(float(count.cpu().numpy().mean()), 2)
        floor_bytes = A * 40 + B * Np * 44
        res["byte_floor"] = floor_bytes
        res["GBps_of_floor"] = round(floor_bytes / (res["kernel_us"]["call"]["median"] * 1e-6) / 1e9, 1)
        out[name] = res
        del ws, d_agents

    # ---- the tick: private crowds against one shared pool, without and with metrics
    if not a.no_tick:
        world = make_world(a.world, a.world, 0.05)
        sc = scenes_in_world(prm, world, B, Np, size_x=40, size_y=40)
        w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
        pool = shared_pool(world, B * Np)
        sp = SharedWorldParams(max_range=a.loop_range)
        kw = dict(obstacles_from_costmap=True, world=world)
        eps = {"private": BatchEpisode(prm, sc, w_ref, **kw), "shared": BatchEpisode(prm, sc, w_ref, shared=sp, pool=pool, **kw),
               "private_metrics": BatchEpisode(prm, sc, w_ref, metrics=MetricsParams(), **kw),
               "shared_metrics": BatchEpisode(prm, sc, w_ref, metrics=MetricsParams(), shared=sp, pool=pool, **kw)}
        out["tick"] = {"world": a.world, "pool": B * Np, "max_range": a.loop_range, "bins": list(eps["shared"].shared_grid[:2])}
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
        e = eps["shared_metrics"]
        e.tick(timing=timing)
        out["tick"]["gather_us"] = {k: round(timing[k + "_ms"] * 1e3, 1) for k in ("nearest", "nearest_after", "people")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
