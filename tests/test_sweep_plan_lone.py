"""Lone trips of the solve kernel, the part that needs no GPU: the knob is read where the others are, the kernels that
carry the helped loop are the ones the launch plan sends a headline batch to, and the eight scenes
tests/test_gpu_lone_help.py uses to make both halves of a wave the owner of lone trips do what they were picked for."""
import os

import numpy as np

from nav2_social_mpc_controller_amd.params import OptimizerParams
from nav2_social_mpc_controller_amd.scenes import make_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nav2_social_mpc_controller_amd", "csrc")


def test_the_knob_is_read_in_the_plan_header_and_documented():
    plan = open(os.path.join(CSRC, "smpc_plan.hpp")).read()
    assert plan.count('("SMPC_NO_LONE_HELP")') == 1
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".inc")) and name != "smpc_plan.hpp":
            assert "SMPC_NO_LONE_HELP\")" not in open(os.path.join(CSRC, name)).read(), name
    assert "SMPC_NO_LONE_HELP" in open(os.path.join(ROOT, "tools", "README.md")).read()


def test_only_the_plain_two_scenes_per_wave_solve_kernels_carry_lone_trips():
    launch = open(os.path.join(CSRC, "smpc_launch.hpp")).read()
    assert "lone_trip_kernel(int W, bool vt, bool sp, bool trace) { return W == 32 && !vt && !sp && !trace; }" in launch
    body = open(os.path.join(CSRC, "smpc_solve_body.inc")).read()
    assert "constexpr bool kLone = lone_trip_kernel(W, kVT, kSP, kTrace);" in body
    assert "kLone" not in open(os.path.join(CSRC, "smpc_eval_body.inc")).read()      # K1 has no trips


def test_the_eight_scene_batch_ends_its_pairs_in_both_orders(oracle):
    """The solve kernel's queue hands neighbouring scenes to the two slots of a wave. The oracle's evaluation counts (the
    device's sweeps of a firm scene) say which slot of each pair is left alone: both must occur."""
    from test_gpu_lone_help import SEED_B8, T
    prm = OptimizerParams.readme()
    sc = make_scenes(prm, 8, 8, T=T, seed=SEED_B8, map_cells=80)
    r = oracle.solve(prm, sc, nthreads=4, theta_zero_convention=True)
    ev = r["evaluations"].reshape(4, 2)
    firm = (r["marginal_decisions"] == 0).reshape(4, 2).all(axis=1)
    assert (firm & (ev[:, 0] > ev[:, 1] + 1)).any() and (firm & (ev[:, 0] + 1 < ev[:, 1])).any(), (ev, firm)
