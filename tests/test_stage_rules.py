"""csrc/smpc_stage.hpp on the host: stage_people() is one text with two callers, the staging kernel and the scene fetch of
the fixed-shape solve kernel. Here the host pass of hipcc compiles it (tests/native/stage_shim.hip, no device code) and
every lane of a slot runs it on hand-made steps that sit on the rules' edges:

  step 0, 1  two moving agents at the same distance: the first in index order is the nearest (either way round)
  step 2     the nearest agent moves at exactly 0.05 m/s: it does not count, the next one does
  step 3     the nearest moving agent at exactly 2 m: it still gives a steering target
  step 4     one ulp beyond 2 m: no target
  step 5     the nearest agent is invalid (t = -1): it still gives the target (the rule reads the speed alone), the mask
             leaves it out
  step 6     nobody moves: no target

The masks and tags are set against oracle/pyref.py, which states the critics straight from the reference: with the robot
kept at its start pose (v = 0) and turning (w != 0), the agent-angle row of a step is w_aa wrap(theta - tag)^2 (zero
without a tag; the two possible tags give different values once theta has left yaw0) and the proxemics row is taken over
the valid agents of the mask. Positions are small binary fractions, so every distance is exact however the compiler
contracts the sums."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from nav2_social_mpc_controller_amd.params import OptimizerParams
from nav2_social_mpc_controller_amd.scenes import make_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "stage_shim.hip")
OUT = os.path.join(ROOT, "tests", "native", "_build", "libstage_shim.so")
CSRC = os.path.join(ROOT, "nav2_social_mpc_controller_amd", "csrc")
NO_TARGET = 1e300
YAW0 = 0.25
UP, DOWN = YAW0 + math.pi / 6, YAW0 + (-(math.pi / 6))


@pytest.fixture(scope="module")
def shim():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("smpc_stage.hpp", "smpc_launch.hpp", "smpc_math.hpp")]
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", OUT, SRC])
    lib = ctypes.CDLL(OUT)
    lib.shim_stage_people.restype = ctypes.c_int
    return lib


def stage(lib, T, N, pose0, people, fixed=False):
    """(records [N,T,4], masks [T], tags [T]) of one scene: people [T+1,6,N]."""
    pose0, people = np.ascontiguousarray(pose0, np.float64), np.ascontiguousarray(people, np.float64)
    assert people.shape == (T + 1, 6, N)
    rec, mask, tag = np.full((N, T, 4), np.nan), np.zeros(T, np.uint64), np.full(T, np.nan)
    rc = lib.shim_stage_people(T, N, int(fixed), *(ctypes.c_void_p(a.ctypes.data) for a in (pose0, people, rec, mask, tag)))
    assert rc == 0
    return rec, mask, tag


def agent(x, y, yaw, lv, t=0.0):
    return (x, y, yaw, t, lv, 0.0)


FAR = [agent(3.0, 3.0, 0.5, 0.5), agent(3.0, -3.0, 0.5, 0.5)]
# with yaw0 = 0.25: an agent on the x axis heading -1 asks for yaw0 + pi/6, one on the y axis heading +1 for yaw0 - pi/6
STEPS = [
    ([agent(1.0, 0.0, -1.0, 0.5), agent(0.0, 1.0, 1.0, 0.5)] + FAR, UP, 0b1111),
    ([agent(0.0, 1.0, 1.0, 0.5), agent(1.0, 0.0, -1.0, 0.5)] + FAR, DOWN, 0b1111),
    ([agent(0.5, 0.0, -1.0, 0.05), agent(0.0, 1.5, 1.0, 0.0625), FAR[0], agent(3.0, -3.0, 0.5, 0.5, t=-1.0)], DOWN, 0b0111),
    ([agent(2.0, 0.0, -1.0, 0.5), agent(0.0, 2.5, 1.0, 0.5)] + FAR, UP, 0b1111),
    ([agent(np.nextafter(2.0, 3.0), 0.0, -1.0, 0.5), agent(0.0, 2.5, 1.0, 0.5)] + FAR, NO_TARGET, 0b1111),
    ([agent(0.25, 0.0, -1.0, 0.5, t=-1.0), agent(0.0, 1.0, 1.0, 0.5)] + FAR, UP, 0b1110),
    ([agent(1.0, 0.0, -1.0, 0.0), agent(0.0, 1.0, 1.0, 0.05), agent(3.0, 3.0, 0.5, 0.0), agent(3.0, -3.0, 0.5, 0.0)], NO_TARGET, 0b1111),
]


@pytest.fixture(scope="module")
def scene():
    """One scene whose steps are STEPS, robot at the origin with heading YAW0."""
    T, N = len(STEPS), 4
    prm = OptimizerParams.readme()
    sc = make_scenes(prm, 1, N, T=T, seed=11, map_cells=120)
    sc.pose0[0] = (0.0, 0.0, YAW0)
    sc.costmap_origin[0] = (-3.0, -3.0)      # the robot sits at the map's centre
    sc.people[0, 0] = np.array(STEPS[0][0]).T  # row 0 (the present) is read by nothing
    for t, (agents, _, _) in enumerate(STEPS):
        sc.people[0, t + 1] = np.array(agents).T
    return prm, sc


def test_masks_and_tags_on_the_rules_edges(shim, scene):
    prm, sc = scene
    T, N = sc.T, sc.N
    rec, mask, tag = stage(shim, T, N, sc.pose0[0], sc.people[0])
    for t, (_, want_tag, want_mask) in enumerate(STEPS):
        assert int(mask[t]) == want_mask, (t, bin(int(mask[t])))
        assert tag[t] == want_tag, (t, tag[t])
    ppl = sc.people[0, 1:]  # [T,6,N]
    assert np.array_equal(rec[..., 0], ppl[:, 0].T) and np.array_equal(rec[..., 1], ppl[:, 1].T)
    assert np.abs(rec[..., 2] - (ppl[:, 4] * np.cos(ppl[:, 2])).T).max() <= 1e-15
    assert np.abs(rec[..., 3] - (ppl[:, 4] * np.sin(ppl[:, 2])).T).max() <= 1e-15


def test_masks_and_tags_are_the_oracles(shim, scene):
    torch = pytest.importorskip("torch")
    from oracle import pyref

    prm, sc = scene
    T, N = sc.T, sc.N
    _, mask, tag = stage(shim, T, N, sc.pose0[0], sc.people[0])
    CH, bl, nb, P, M, _ = prm.dims(T, True)
    w = 0.4
    x = np.tile([0.0, w], nb)  # the robot stays where it is and turns: theta_{t+1} = yaw0 + (t + 1) w dt
    r = pyref.residuals(prm, sc, 0, torch.tensor(x)).numpy()
    assert r.shape == (M,)
    row = 0
    for t in range(T):
        theta = YAW0 + (t + 1) * w * sc.dt
        ad = 0.0 if tag[t] == NO_TARGET else math.atan2(math.sin(theta - tag[t]), math.cos(theta - tag[t]))
        assert abs(r[row] - prm.agent_angle_weight * ad * ad) <= 1e-12 * max(1.0, abs(r[row])), (t, "agent angle")
        d2 = [sc.people[0, t + 1, 0, a] ** 2 + sc.people[0, t + 1, 1, a] ** 2 for a in range(N) if (int(mask[t]) >> a) & 1]
        prox = prm.proxemics_weight * pyref.ALPHA * math.exp(-min(d2) / pyref.D0 ** 2)
        assert abs(r[row + 2] - prox) <= 1e-12 * max(1.0, abs(prox)), (t, "proxemics")
        row += 8 + (1 if (t != 0 and t < CH // bl) else 0)
    assert row == M
    # the edges decide something: the other tag, or none, gives another row
    t = 0
    theta = YAW0 + w * sc.dt
    other = math.atan2(math.sin(theta - DOWN), math.cos(theta - DOWN))
    assert abs(r[0] - prm.agent_angle_weight * other * other) > 1e-6


def test_the_fixed_shape_instantiation_stages_the_same(shim):
    """stage_people<32, FixedShape<28, 8, 18, 6>> (the scene fetch) against <32, RuntimeShape> (the staging kernel) on
    scenes of the headline shape, some agents invalid: every record, mask and tag bit for bit."""
    prm = OptimizerParams.readme()
    sc = make_scenes(prm, 12, 8, T=28, seed=2807, map_cells=80, standing_fraction=0.3)
    sc.people[3, :, 3, 2] = -1.0
    sc.people[5, 7:, 3, 6] = -1.0
    tags = []
    for b in range(sc.B):
        plain = stage(shim, 28, 8, sc.pose0[b], sc.people[b])
        fixed = stage(shim, 28, 8, sc.pose0[b], sc.people[b], fixed=True)
        for p, f in zip(plain, fixed):
            assert np.array_equal(p.view(np.uint64), f.view(np.uint64)), b
        tags.append(plain[2])
    tags = np.array(tags)
    assert (tags == NO_TARGET).any() and (tags != NO_TARGET).any()
