"""The reactive crowd step of a shared world's pedestrians on the CPU: the yardstick itself (tests/crowd_pool_ref.py) against
tests/crowd_ref.py on one robot's persons, the `__host__ __device__` rule of csrc/smpc_crowd_pool_rule.hpp compiled into a
host-only program (rule 4's rounding and its bound), the ctypes mirror against include/smpc_crowd_pool.h, the exported symbol,
PoolCrowdParams, SharedWorldParams.grid with a reach, scenes.pool_waypoints, the episode's arguments, and every seeded case
of tests/test_gpu_crowd_pool.py against the decisions the rules take (tests/crowd_pool_cases.py)."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import crowd_cases as CC
import crowd_pool_cases as PC
import crowd_pool_ref as P
import crowd_ref as R
from nav2_social_mpc_controller_amd import _abi_crowd_pool as PA
from nav2_social_mpc_controller_amd import solver as S
from nav2_social_mpc_controller_amd.params import PoolCrowdParams, SharedWorldParams
from nav2_social_mpc_controller_amd.scenes import World, make_world, pool_waypoints, shared_pool
from test_kernel_budget import CSRC, HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc_crowd_pool.h")


# ---- the yardstick against the private step's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 64), (130, 8)])
def test_checker_is_crowd_refs_step_on_one_robots_persons_up_to_the_rounding(shape):
    d = CC.case(shape)
    pos, kw = CC.arguments(d, dict(K=3, cyclic=True, robot_visible=False, speeds=True, grid="shared"))
    worst = 0.0
    for b in range(min(d["B"], 6)):
        (dt, people, cursor, pose, twist, count, wp, n_wp), one = CC.robot_arguments(pos, kw, b)
        n = int(count)
        want, want_cur = R.step(dt, people, cursor, pose, twist, count, wp, n_wp, **one)
        one.pop("robot_visible")
        speeds = one.pop("desired_speeds")
        got, got_cur = P.step(dt, people[:n], n, cursor[:n], wp[:n], n_wp[:n], 1e6, desired_speeds=speeds[:n], **one)
        assert np.array_equal(got_cur, want_cur[:n])
        if n:
            err = np.abs(got[:, 0:4] - want[:n, 0:4]).max()
            dz = (got[:, 4] - want[:n, 4]) * dt
            err = max(err, np.abs(np.arctan2(np.sin(dz), np.cos(dz))).max())
            worst = max(worst, err / (n * P.QUANTUM * dt))
            assert err <= n * P.QUANTUM * dt, (b, err)
    print(f"{shape}: largest difference = {worst:.3f} of n * 2^-36 * dt")


def test_checker_by_hand():
    # an inert mover keeps its bits and its cursor and is nobody's partner; a static row is a partner and does not move
    agents = np.array([[0.0, 0.0, 0.0, 0.0, 0.0], [np.nan, 0.0, 0.1, 0.0, 7.0], [1.0, 0.0, 0.0, 0.0, 0.0], [0.0, np.inf, 0.0, 0.0, 0.0]])
    wp, n_wp = np.zeros((2, 1, 2)), np.zeros(2, np.int32)
    nxt, cur = P.step(0.1, agents, 2, np.array([0, 5], np.int32), wp, n_wp, 5.0, cyclic=False)
    assert np.array_equal(nxt[1].view(np.uint64), agents[1].view(np.uint64)) and cur.tolist() == [0, 5]
    assert nxt[0, 2] < 0.0 and nxt[0, 3] == 0.0              # pushed away from the static row at (1, 0), by nobody else
    alone, _ = P.step(0.1, agents[[0, 2]], 1, np.zeros(1, np.int32), wp[:1], n_wp[:1], 5.0)
    assert np.array_equal(alone[0], nxt[0])
    # the gate is the gather's: 3-4-5 at range 5, and one ulp beyond
    tri = np.array([[1.0, 2.0, 0.0, 0.0, 0.0], [4.0, 6.0, 0.0, 0.0, 0.0]])
    assert P.partners_of(tri, 0, 5.0) == [1] and P.partners_of(tri, 0, np.nextafter(5.0, 0.0)) == []
    tri[1, 1] = np.nextafter(6.0, np.inf)
    assert P.partners_of(tri, 0, 5.0) == []
    # rule 4 in Python integers
    assert [P.quantize(v) for v in (0.0, -0.0, math.nan, 9.0, -math.inf, 1.5 * P.QUANTUM, 2.5 * P.QUANTUM, -0.5 * P.QUANTUM)] == \
        [0, 0, 0, 2 ** 39, -2 ** 39, 2, 2, 0]


# ---- the __host__ __device__ rule, compiled for the host -----------------------------------------------------------------
# one value per line as a hex float -> "<q, decimal> <bits of cp_force(q), hex>"; then the bound's arithmetic
PROBE = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "smpc_crowd_pool_rule.hpp"
int main() {
  static char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    double t;
    if (std::sscanf(line, "%la", &t) != 1 && std::sscanf(line, "%lf", &t) != 1) return 1;
    const int64_t q = smpc::cp_quantize(t);
    const double f = smpc::cp_force(q);
    uint64_t bits;
    std::memcpy(&bits, &f, sizeof bits);
    std::printf("%" PRId64 " %016" PRIx64 "\n", q, bits);
  }
  // rule 4's bound: 2^24 - 1 partners (a row is not its own) at the clamp, either sign, by arithmetic in 128 bits
  const __int128 worst = (__int128)smpc::kCpMaxPartners * smpc::cp_quantize(smpc::kCpClamp);
  const __int128 least = (__int128)smpc::kCpMaxPartners * smpc::cp_quantize(-smpc::kCpClamp);
  std::printf("%d %d %" PRId64 " %d\n", worst <= (__int128)INT64_MAX ? 1 : 0, least >= (__int128)INT64_MIN ? 1 : 0,
              smpc::cp_quantize(1e300), (int)smpc::cp_live(0.0, 1e300, -1e300, 0.0) + 2 * (int)smpc::cp_live(0.0, 0.0, __builtin_nan(""), 0.0) + 4 * (int)smpc::cp_live(__builtin_inf(), 0.0, 0.0, 0.0));
  return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    tmp = tmp_path_factory.mktemp("crowd_pool_rule")
    src, exe = tmp / "probe.hip", tmp / "probe"
    src.write_text(PROBE)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])

    def ask(values):
        out = subprocess.run([str(exe)], input="".join(float(v).hex() + "\n" for v in values), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(out) == len(values) + 1
        return [(int(l.split()[0]), int(l.split()[1], 16)) for l in out[:-1]], out[-1].split()

    return ask


def test_compiled_rounding_is_the_checkers_ties_to_even_clamp_nan_and_negative_zero(rule):
    g = np.random.default_rng(5)
    u = P.QUANTUM
    ties = [k * u / 2 for k in range(-9, 10)] + [(2 ** 20 + k) * u / 2 for k in range(6)]      # halves: ties to even
    edges = [8.0, -8.0, np.nextafter(8.0, 0.0), np.nextafter(8.0, 9.0), 8.5, -1e300, 1e300, np.inf, -np.inf, np.nan, 0.0, -0.0,
             5e-324, -5e-324, 2.1 * math.sqrt(2.0), -2.81]
    values = ties + edges + g.uniform(-3.0, 3.0, 500).tolist() + (g.uniform(-3.0, 3.0, 200) * 1e-9).tolist()
    got, last = rule(values)
    for v, (q, bits) in zip(values, got):
        assert q == P.quantize(v), (v, q)
        assert bits == int(np.float64(float(q) * P.QUANTUM).view(np.uint64)), v
    by = dict(zip([float(v).hex() for v in values], [q for q, _ in got]))
    assert by[(0.5 * u).hex()] == 0 and by[(1.5 * u).hex()] == 2 and by[(2.5 * u).hex()] == 2 and by[(-1.5 * u).hex()] == -2
    assert by[float(8.5).hex()] == 2 ** 39 == by[float(np.inf).hex()] and by[float(-1e300).hex()] == -2 ** 39
    assert by[float(np.nan).hex()] == 0 and by[float(-0.0).hex()] == 0
    # the bound: 2^24 - 1 worst-case terms fit, by arithmetic; 2^24 of them would not
    assert last == ["1", "1", str(2 ** 39), "1"]
    assert (2 ** 24 - 1) * 2 ** 39 < 2 ** 63 <= 2 ** 24 * 2 ** 39


# ---- the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mirror_matches_the_header_and_the_library_exports_the_function(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src))) == sorted(PA.FUNCTIONS) == ["smpc_crowd_pool_step_batch"]
    assert re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S) == [st.c_name for st in PA.STRUCTS]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' + "".join(f'printf("%zu\\n", offsetof({st.c_name}, {f[0]}));\n' for f in st._fields_)
                   for st in PA.STRUCTS)
    body += 'printf("%d\\n%a\\n", (int)SMPC_CROWD_POOL_FRACTION_BITS, (double)SMPC_CROWD_POOL_TERM_CLAMP);\n'
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc_crowd_pool.h"\nint main(void){\n' + body + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = subprocess.check_output([str(exe)], text=True).split()
    want = [v for st in PA.STRUCTS for v in [C.sizeof(st)] + [getattr(st, f[0]).offset for f in st._fields_]]
    assert [int(v) for v in values[:-2]] == want and C.sizeof(PA.SmpcCrowdPoolIn) == 176
    assert int(values[-2]) == PA.SMPC_CROWD_POOL_FRACTION_BITS == P.FRACTION_BITS == 36
    assert float.fromhex(values[-1]) == PA.SMPC_CROWD_POOL_TERM_CLAMP == P.CLAMP == 8.0
    exported = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    lib = S.load_library()
    for name, (restype, argtypes) in PA.FUNCTIONS.items():
        assert f" {name}\n" in exported
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes


def test_the_main_abi_is_as_it_was():
    from nav2_social_mpc_controller_amd import _abi
    assert _abi.SMPC_ABI_VERSION == 6 and len(_abi.FUNCTIONS) == 27 and not set(PA.FUNCTIONS) & set(_abi.FUNCTIONS)
    assert re.search(r"#define\s+SMPC_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "smpc.h")).read())


# ---- the parameters, the grid, the waypoints and the episode's arguments ---------------------------------------------------
def test_pool_crowd_params_defaults_and_checks():
    cp = PoolCrowdParams()
    assert (cp.interaction_range, cp.goal_radius, cp.person_radius, cp.desired_speed, cp.cyclic) == (5.0, 0.25, 0.35, 0.6, True)
    for bad in (dict(interaction_range=0.0), dict(interaction_range=-1.0), dict(interaction_range=np.inf), dict(interaction_range=np.nan),
                dict(goal_radius=-0.1), dict(person_radius=-1.0), dict(person_radius=np.nan), dict(desired_speed=0.0), dict(desired_speed=np.nan)):
        with pytest.raises(ValueError):
            PoolCrowdParams(**bad)
    ci = S.BatchSolver.crowd_pool_c(PoolCrowdParams(interaction_range=3.5, cyclic=False), 7, 11, 2, 0.1, 4, 3, [0.5, -2.0], 7.75, 1, bins_ready=1)
    assert (ci.M, ci.A, ci.K, ci.on_device, ci.cyclic, ci.bins_ready, ci.grid_x, ci.grid_y) == (7, 11, 2, 1, 0, 1, 4, 3)
    assert (list(ci.grid_origin), ci.bin_size, ci.interaction_range, ci.dt) == ([0.5, -2.0], 7.75, 3.5, 0.1)
    assert (ci.goal_radius, ci.person_radius, ci.desired_speed) == (0.25, 0.35, 0.6)


def test_grid_without_a_reach_is_unchanged_and_with_one_serves_both_ranges():
    flat = lambda cx, cy, res, origin=(0.0, 0.0): World(np.zeros((cy, cx), np.uint8), np.asarray(origin, np.float64), res)
    m = 1.0 + 2.0 ** -20
    for sp, world in ((SharedWorldParams(), flat(256, 192, 0.05, (-1.5, 2.0))), (SharedWorldParams(max_range=2.0), flat(400, 120, 0.05)),
                      (SharedWorldParams(max_range=1.0), flat(4000, 1000, 0.25))):
        a, b, c = sp.grid(world), sp.grid(world, None), sp.grid(world, sp.max_range / 2)      # a smaller reach changes nothing
        for other in (b, c):
            assert a[:2] == other[:2] and a[3] == other[3] and np.array_equal(a[2], other[2])
    gx, gy, origin, size = SharedWorldParams().grid(flat(256, 192, 0.05, (-1.5, 2.0)))
    assert (gx, gy, size) == (2, 1, 10.0 * m)                                               # today's numbers (tests/test_nearest.py)
    gx, gy, origin, size = SharedWorldParams(max_range=2.0).grid(flat(400, 120, 0.05), 5.0)   # 20 m x 6 m, the reach decides
    assert size == 5.0 * m and (gx, gy) == (4, 2) and origin.tolist() == [0.0, 0.0]
    gx, gy, origin, size = SharedWorldParams(max_range=1.0).grid(flat(4000, 1000, 0.25), 3.0)  # the 65536-bin cap still decides
    assert size == 1000.0 / 256.0 and (gx, gy) == (256, 64)


def test_pool_waypoints_are_seeded_lie_on_free_cells_and_start_straight_ahead():
    world = make_world(200, 160, 0.05, origin=(-2.0, 1.0))
    pool = shared_pool(world, 120)
    pool[5, 0] = np.nan
    wp, n_wp = pool_waypoints(world, pool, K=3)
    assert wp.shape == (120, 3, 2) and wp.dtype == np.float64 and n_wp.shape == (120,) and n_wp.dtype == np.int32
    ci = np.floor((wp[..., 0] - world.origin[0]) / world.resolution).astype(int)
    cj = np.floor((wp[..., 1] - world.origin[1]) / world.resolution).astype(int)
    assert (world.map[cj, ci] == 0).all()
    walking = np.hypot(pool[:, 2], pool[:, 3]) > 0.0
    walking[5] = False
    assert np.array_equal(n_wp, np.where(walking, 3, 0)) and 0 < walking.sum() < 120
    ahead = wp[:, 0] - pool[:, 0:2]
    dist = np.hypot(ahead[:, 0], ahead[:, 1])
    cross = ahead[:, 0] * pool[:, 3] - ahead[:, 1] * pool[:, 2]
    straight = walking & (np.abs(cross) < 1e-9) & (dist >= 0.5 - 1e-9) & (dist <= 6.0 + 1e-9)
    assert straight.sum() > 0.5 * walking.sum()                       # (the others had no free cell ahead and fell back)
    same = lambda a, b: np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])
    assert same((wp, n_wp), pool_waypoints(world, pool, K=3))
    assert not same((wp, n_wp), pool_waypoints(world, pool, K=3, seed=9))
    first = pool_waypoints(world, pool[:50], K=3)
    assert np.array_equal(first[0].view(np.uint64), wp[:50].view(np.uint64))      # keyed by the person's index
    assert pool_waypoints(world, np.zeros((0, 5)))[0].shape == (0, 2, 2)


def test_the_episode_declares_the_arguments_and_refuses_them_without_a_shared_pool():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode, TickRecord
    sig = inspect.signature(BatchEpisode.__init__).parameters
    for name in ("pool_crowd", "pool_waypoints", "pool_n_waypoints", "pool_speed"):
        assert name in BatchEpisode.FORWARDED and name not in BatchEpisode.PER_ROBOT and sig[name].default is None
    assert {"pool_next", "pool_cursor_before", "pool_cursor_after"} <= set(TickRecord.__dataclass_fields__)
    from nav2_social_mpc_controller_amd.episode_stages import PoolCrowd
    with pytest.raises(ValueError, match="pool_crowd needs shared"):
        PoolCrowd.check(PoolCrowdParams(), None, None, None, None, None)
    with pytest.raises(ValueError, match="need pool_crowd"):
        PoolCrowd.check(None, None, None, np.zeros((1, 2, 2)), None, None)
    with pytest.raises(ValueError, match="independent"):
        ShardedEpisode(None, None, None, None, None, None, shared=SharedWorldParams(), pool_crowd=PoolCrowdParams())


# ---- the seeded cases of the GPU tests, by the checker alone ----------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in PC.CASES if n != "chain"])
def test_every_seeded_case_stays_clear_of_the_decisions_and_within_its_own_tolerance(name):
    c = PC.case(name)
    m = PC.case_margins(c)
    print(f"{name}: A = {len(c['agents'])}, M = {c['M']}, largest partner count {m['partners']}, margins "
          + ", ".join(f"{k} {m[k]:.2e}" for k in ("theta", "pair", "goal", "edge", "speed")))
    for k, least in PC.CONDITIONS.items():
        assert m[k] >= least, (name, k, m[k])
    assert P.bound(m["partners"], c["dt"]) <= R.TOL / 2, (name, m["partners"])


def test_the_chained_case_stays_clear_over_its_twelve_steps():
    c = PC.case("chain")
    agents, cursor, most = c["agents"].copy(), c["cursor"].copy(), 0
    for k in range(12):
        m = PC.case_margins(c, agents, cursor)
        for key, least in PC.CONDITIONS.items():
            assert m[key] >= least, (k, key, m[key])
        most = max(most, m["partners"])
        agents[:c["M"]], cursor = PC.ref_step(c, agents, cursor)
    print(f"chain: largest partner count over 12 steps {most}")
    assert P.bound(most, c["dt"]) <= R.TOL / 2
