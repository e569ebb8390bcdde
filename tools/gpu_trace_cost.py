"""Cost of the per-iteration trace (smpc_solve_trace_batch) on the headline batch (BASELINE configs[2]: 8192 scenes, N = 8,
T = 28), lone solve launches on device-resident inputs, alternated round by round:
  (a) the sp kernel, every row equal to the handle's parameters    smpc_solve_kernel<3,32,true,true>
  (b) the trace kernel on the plain batch (neutral rows filled by the library), every row kept   smpc_solve_kernel<3,32,true,true,true>
  (c) the trace kernel with max_rows = 0: the counts alone
Prints the median kernel time of each and (b) / (a), (c) / (a)."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from nav2_social_mpc_controller_amd.params import OptimizerParams, scene_param_rows  # noqa: E402
from nav2_social_mpc_controller_amd.scenes import make_scenes  # noqa: E402
from nav2_social_mpc_controller_amd.solver import BatchSolver  # noqa: E402


def main(rounds=15, B=8192, N=8):
    prm = OptimizerParams.readme()
    sc = make_scenes(prm, B, N, seed=0x5EED0001)
    T = sc.T
    s = BatchSolver(prm)
    sb_sp, keep_sp = sc.with_scene_params(scene_param_rows([prm], np.zeros(B, int))).to_device()
    sb, keep = sc.to_device()
    stage = [s.stage_people_device(sb_sp), s.stage_people_device(sb)]
    rb, rt = s.alloc_results(B, T)
    to_all, t_all = s.alloc_trace(B)
    to_none, t_none = s.alloc_trace(B, 0)
    run = {"a_sp_neutral": lambda: s.solve_device(sb_sp, rb), "b_trace": lambda: s.solve_trace_device(sb, rb, to_all),
           "c_trace_counts": lambda: s.solve_trace_device(sb, rb, to_none)}
    times = {k: [] for k in run}
    for r in range(rounds + 2):
        for name, fn in run.items():
            fn()
            ms = s.last_kernel_ms()
            if r >= 2:  # two warm-up rounds
                times[name].append(ms)
    torch.cuda.synchronize()
    med = {k: float(np.median(v)) for k, v in times.items()}
    rows = t_all["trace_rows"].cpu().numpy()
    for name, v in times.items():
        print(f"{name:15s} solve median {med[name]:.3f} ms (min {min(v):.3f} max {max(v):.3f})")
    print(f"rows per scene: mean {rows.mean():.2f} max {rows.max()}; {rows.sum() * 72 / 1e6:.1f} MB of rows per launch")
    print(f"(b)/(a) = {med['b_trace'] / med['a_sp_neutral']:.4f}, (c)/(a) = {med['c_trace_counts'] / med['a_sp_neutral']:.4f}")
    del stage, keep, keep_sp


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:]))
