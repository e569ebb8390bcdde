"""Development probe: find the first LM iteration where HIP and oracle part ways for the worst scene of a case.

One traced launch (BatchSolver.solve_trace) gives the device's rows of every scene; the oracle's rows of the worst scene
come from oracle_py.trace. Printed side by side from the first row that differs (integer columns unequal, or a real-valued
column further apart than --rtol relative to max(1, |value|)).

usage: python tools/gpu_trace_diff.py [--rtol 1e-9] [--scene B]"""
import argparse
import sys

import numpy as np

sys.path.insert(0, ".")
from nav2_social_mpc_controller_amd.params import OptimizerParams
from nav2_social_mpc_controller_amd.scenes import make_scenes
from nav2_social_mpc_controller_amd.solver import TRACE_COLS, BatchSolver
from oracle import oracle_py as O

ap = argparse.ArgumentParser()
ap.add_argument("--rtol", type=float, default=1e-9)
ap.add_argument("--scene", type=int, default=None, help="scene to print (default: the one with the largest command error)")
args = ap.parse_args()

README = OptimizerParams.readme()
prm = README.replace(control_horizon=30, max_time=2.0)
sc = make_scenes(prm, 128, 16, seed=204)
rg = BatchSolver(prm).solve_trace(sc)
rz = O.solve(prm, sc, nthreads=16, theta_zero_convention=True)
err = np.abs(rg["cmds"] - rz["cmds"]).reshape(sc.B, -1).max(axis=1)
b = int(np.argmax(err)) if args.scene is None else args.scene
print("scene", b, "max|dcmd|", err[b], "iters gpu/oracle", rg["iterations"][b], rz["iterations"][b], "reason", rg["reason"][b],
      rz["reason"][b], "cost", rg["final_cost"][b], rz["final_cost"][b], "events", rz["sign_noise_events"][b])
O.set_theta_zero_convention(True)
to = O.trace(prm, sc, b, max_rows=prm.max_iterations + 2)
O.set_theta_zero_convention(False)
tg = rg["trace"][b, :min(rg["trace_rows"][b], rg["trace"].shape[1])]
n = min(len(tg), len(to))
ints = [TRACE_COLS.index(c) for c in ("iter", "ls_evals", "accepted")]
differs = [i for i in range(n) if not np.array_equal(tg[i, ints], to[i, ints])
           or np.any(np.abs(tg[i] - to[i]) > args.rtol * np.maximum(1.0, np.abs(to[i])))]
first = differs[0] if differs else n
if first == n and len(tg) == len(to):
    print(f"all {n} rows agree within {args.rtol:g}")
    sys.exit(0)
print(f"first differing row: {first} (device has {len(tg)} rows, oracle {len(to)})")
print("     " + " ".join(f"{c[:13]:>22s}" for c in TRACE_COLS))
for i in range(max(0, first - 1), max(len(tg), len(to))):
    for who, t in (("gpu", tg), ("cpu", to)):
        if i < len(t):
            print(f"{who:>4s} " + " ".join(f"{v:22.15e}" for v in t[i]))
