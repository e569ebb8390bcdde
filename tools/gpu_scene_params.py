"""Cost of per-scene weights and bounds (smpc_scene_batch.scene_params) on the headline batch (BASELINE configs[2]:
8192 scenes, N = 8, T = 28), lone solve launches on device-resident inputs, three variants alternated round by round:
  (a) the per-scene-horizon kernel with every T_scene = T          smpc_solve_kernel<3,32,true,false>
  (b) the sp kernel, every row equal to the handle's parameters    smpc_solve_kernel<3,32,true,true>
  (c) the sp kernel, the two benchmark presets alternating by scene
The same for K1. Prints the median kernel time of each and (b) / (a)."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from nav2_social_mpc_controller_amd.params import OptimizerParams, scene_param_rows  # noqa: E402
from nav2_social_mpc_controller_amd.scenes import make_scenes  # noqa: E402
from nav2_social_mpc_controller_amd.solver import BatchSolver  # noqa: E402


def main(rounds=15, B=8192, N=8):
    a, b = OptimizerParams.soc_work_obst_benchmark(), OptimizerParams.obst_only_benchmark()
    prm = OptimizerParams.readme()
    sc = make_scenes(prm, B, N, seed=0x5EED0001)
    T = sc.T
    variants = {
        "a_vt": (prm, sc.with_horizons(np.full(B, T, np.int32))),
        "b_sp_neutral": (prm, sc.with_scene_params(scene_param_rows([prm], np.zeros(B, int)))),
        "c_sp_presets": (a, sc.with_scene_params(scene_param_rows([a, b], np.arange(B) % 2))),
    }
    run = {}
    for name, (p, s_) in variants.items():
        s = BatchSolver(p)
        sb, keep = s_.to_device()
        rb, rt = s.alloc_results(B, T)
        eo, et = s.alloc_eval(B, T)
        stage = s.stage_people_device(sb)
        run[name] = (s, sb, keep, rb, rt, eo, et, stage)
    times = {k: {"solve": [], "k1": []} for k in run}
    for r in range(rounds + 2):
        for name, (s, sb, keep, rb, rt, eo, et, stage) in run.items():
            s.solve_device(sb, rb)
            ms = s.last_kernel_ms()
            s.eval_device(sb, keep["init_params"].data_ptr(), eo)
            k1 = s.last_kernel_ms()
            if r >= 2:  # two warm-up rounds
                times[name]["solve"].append(ms)
                times[name]["k1"].append(k1)
    torch.cuda.synchronize()
    med = {k: {m: float(np.median(v)) for m, v in d.items()} for k, d in times.items()}
    for name, (s, sb, keep, rb, rt, eo, et, stage) in run.items():
        ev = rt["evaluations"].cpu().numpy()
        d = times[name]
        print(f"{name:14s} solve median {med[name]['solve']:.3f} ms (min {min(d['solve']):.3f} max {max(d['solve']):.3f}), "
              f"K1 median {med[name]['k1'] * 1e3:.1f} us (min {min(d['k1']) * 1e3:.1f}); sweeps mean {ev.mean():.2f} "
              f"total {int(ev.sum())}")
    for m in ("solve", "k1"):
        print(f"{m}: (b)/(a) = {med['b_sp_neutral'][m] / med['a_vt'][m]:.4f}, (c)/(a) = {med['c_sp_presets'][m] / med['a_vt'][m]:.4f}")


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:]))
