"""Cost of the episode metrics (smpc_episode_metrics_batch), two measurements, one JSON line:
  kernel: HIP-event time of the metrics kernel alone (smpc_last_kernel_ms) on device pointers, B robots with Np persons
          each, per-robot distance grids and goals, median of --reps launches; smpc_select_command_batch on the same
          batch size beside it, alternating (the yardstick: another one-thread-of-work-per-robot kernel of the tick).
  tick:   the closed-loop tick (arc stand-in, N = Np agents) of two episodes on the same scenes, one with metrics and one
          without, each replayed from its HIP graph and also ticked eagerly: --rounds blocks of --ticks ticks,
          alternating between the two episodes; median ms per tick of each and the spread (min .. max) of the blocks.

    python tools/gpu_metrics.py [--B 8192] [--Np 8] [--reps 20] [--rounds 7] [--ticks 20]
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
    ap.add_argument("--cells", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=20)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    from nav2_social_mpc_controller_amd.params import MetricsParams, OptimizerParams
    from nav2_social_mpc_controller_amd.scenes import make_scenes, uniform
    from nav2_social_mpc_controller_amd.solver import BatchSolver

    dev = "cuda:0"
    B, Np = a.B, a.Np
    prm, mp = OptimizerParams.readme(), MetricsParams()
    out = {"B": B, "Np": Np}

    # ---- the kernel alone
    g = torch.Generator(device="cpu").manual_seed(1)
    f64 = dict(dtype=torch.float64, generator=g)
    pose = ((torch.rand((B, 3), **f64) - 0.5) * 4.0).to(dev)
    twist = (torch.rand((B, 2), **f64) * 0.6).to(dev)
    people = ((torch.rand((B, Np, 5), **f64) - 0.5) * 6.0).to(dev)
    count = torch.randint(0, Np + 1, (B,), generator=g, dtype=torch.int32).to(dev)
    goal = ((torch.rand((B, 2), **f64) - 0.5) * 40.0).to(dev)
    grids = torch.rand((B, a.cells, a.cells), dtype=torch.float32, device=dev)
    origin = torch.full((B, 2), -0.025 * a.cells, dtype=torch.float64, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    source = torch.zeros(B, dtype=torch.int32, device=dev)
    acc = torch.zeros((B, 24), dtype=torch.float64, device=dev)
    T = prm.rollout_steps
    traj_cmds = torch.zeros((B, T + 1, 2), dtype=torch.float64, device=dev)
    cmds = torch.zeros((B, T + 1, 2), dtype=torch.float64, device=dev)
    cmd_vel = torch.zeros((B, 2), dtype=torch.float64, device=dev)
    s = BatchSolver(prm)
    s.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    mb = s.metrics_c(mp, B, Np, prm.dt, 1)
    mb.robot_pose, mb.robot_twist, mb.people, mb.count = pose.data_ptr(), twist.data_ptr(), people.data_ptr(), count.data_ptr()
    mb.goal, mb.od_distances, mb.od_origin = goal.data_ptr(), grids.data_ptr(), origin.data_ptr()
    mb.od_shared, mb.od_width, mb.od_height, mb.od_resolution = 0, a.cells, a.cells, 0.05
    mb.status, mb.source = status.data_ptr(), source.data_ptr()
    ms = {"metrics": [], "select_command": []}
    for r in range(a.reps + 2):
        s.episode_metrics_device(mb, acc.data_ptr())
        t_m = s.last_kernel_ms()
        s.select_command_device(B, T, T + 1, 0, traj_cmds.data_ptr(), status.data_ptr(), cmds.data_ptr(), cmd_vel.data_ptr(),
                                source.data_ptr())
        t_s = s.last_kernel_ms()
        if r >= 2:   # the first launches load the code object
            ms["metrics"].append(t_m)
            ms["select_command"].append(t_s)
    out["kernel_us"] = {k: {"median": round(float(np.median(v)) * 1e3, 2), "min": round(min(v) * 1e3, 2), "max": round(max(v) * 1e3, 2)}
                        for k, v in ms.items()}
    assert float(acc[:, 0].max().item()) == a.reps + 2
    s.set_stream(0)

    # ---- the tick with and without
    sc = make_scenes(prm, B, Np)
    w_ref = (uniform(0x5EED0001, np.arange(B), 6)[:, 0] * 2.0 - 1.0) * 0.6
    od = (np.zeros((480, 480), np.uint32), np.array([-16.0, -16.0]), 0.1)
    goals = sc.pose0[:, 0:2] + 3.0
    for mode in ("graph", "eager"):
        eps = {"off": BatchEpisode(prm, sc, w_ref, *od),
               "on": BatchEpisode(prm, sc, w_ref, *od, metrics=mp, goal=goals, od_distances=np.ones((480, 480), np.float32))}
        if mode == "graph":
            for ep in eps.values():
                ep.capture_graph()
        step = (lambda ep: ep.replay()) if mode == "graph" else (lambda ep: ep.tick())
        blocks = {"off": [], "on": []}
        for r in range(a.rounds + 1):
            for name, ep in eps.items():
                ep.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.ticks):
                    step(ep)
                ep.synchronize()
                if r >= 1:   # one warm-up round
                    blocks[name].append((time.perf_counter() - t0) / a.ticks * 1e3)
        out["tick_ms_" + mode] = {k: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                                  for k, v in blocks.items()}
        assert np.array_equal(eps["on"].pose.cpu().numpy(), eps["off"].pose.cpu().numpy())
        assert float(eps["on"].metrics()[:, 0].max()) == (a.rounds + 1) * a.ticks
        del eps
    print(json.dumps(out))


if __name__ == "__main__":
    main()
