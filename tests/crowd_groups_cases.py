"""The seeded inputs of the crowd-groups tests: the inputs of tests/crowd_cases.py (plus the smallest group, 1 x 2) with
group ids on top. Shared by tests/test_crowd_groups.py, which shows with the checkers alone that they keep their margins,
and tests/test_gpu_crowd_groups.py, which runs them on the device."""
import math

import numpy as np

import crowd_cases as G
import crowd_groups_ref as GR

SHAPES = [(1, 1), (1, 2)] + G.SHAPES[1:]
SEEDS = dict(G.SEEDS)
SEEDS[(1, 2)] = 25
# the least distance of the generated inputs from each decision of the group force (tests/test_crowd_groups.py asserts
# them, and crowd_cases.CONDITIONS for the plain step's own decisions)
CONDITIONS = {"gaze": 1e-6, "reach": 1e-9, "rel": 1e-6, "goal": 1e-9}
SPARSE_IDS = [7, 1_000_000, 0, 3, 2_147_483_647, 12_345, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55]
ALL_ID = 1_000_000

_cache = {}


def group_ids(B, Np, count, seed):
    """[B,Np] int32. Robot 0 (count = Np) and every fourth robot: one group of all Np rows. The others: the rows, in a
    seeded order (those below the count first), cut into chunks of 2, 3, 1 and one row without a group, then at random, each chunk with the next id of SPARSE_IDS: the same
    ids in every robot, 7 and 1 000 000 first. Every row gets its id whatever the count, so rows at or beyond the count
    carry ids and a group may lose members to the count."""
    g = np.random.default_rng(seed + 1000)
    gid = np.full((B, Np), -1, np.int32)
    for b in range(B):
        if b % 4 == 0:
            gid[b] = ALL_ID
            continue
        n = int(count[b])
        rows, at, k = np.concatenate([g.permutation(n), n + g.permutation(Np - n)]), 0, 0   # the live rows first
        while at < Np:
            size = (2, 3, 1, 0)[k % 4] if k < 4 else int(g.integers(0, 4))   # 0: one row without a group
            take = rows[at:at + max(size, 1)]
            if size > 0:
                gid[b, take] = SPARSE_IDS[k % len(SPARSE_IDS)]
            at, k = at + len(take), k + 1
    return gid


def coinciding_ids(B, Np):
    """every robot's rows take the ids 0 and 1 in turn (robot b starts with b % 2): all robots of a wavefront use the same two"""
    return ((np.arange(Np)[None, :] + np.arange(B)[:, None]) % 2).astype(np.int32)


def case(shape):
    """crowd_cases' inputs of this shape with "group_id" added"""
    if shape not in _cache:
        d = dict(G.case(shape) if shape in G.SEEDS else G.generate(*shape, SEEDS[shape]))
        d["group_id"] = group_ids(shape[0], shape[1], d["count"], SEEDS[shape])
        if shape == (1, 1):
            d["group_id"][:] = 7          # a group of one
        if shape == (1, 2):
            d["group_id"][:] = 7          # the smallest group
        _cache[shape] = d
    return _cache[shape]


def reference(shape, ci):
    """(people, cursor) after one step of configuration crowd_cases.CONFIGS[ci] with the groups, by the checker: once per session"""
    key = (shape, ci)
    if key not in _cache:
        d = case(shape)
        pos, kw = G.arguments(d, G.CONFIGS[ci])
        _cache[key] = GR.step_batch(*pos, group_id=d["group_id"], **kw)
    return _cache[key]


# ---- behaviour: three companions 3 m apart with the same waypoints, 100 steps of 0.05 s
BEHAVIOUR_STEPS = 100


def behaviour_inputs():
    r = 3.0 / math.sqrt(3.0)                                   # an equilateral triangle of side 3 m around the origin
    pts = [(r * math.cos(a), r * math.sin(a)) for a in (math.pi / 2, math.pi / 2 + 2 * math.pi / 3, math.pi / 2 + 4 * math.pi / 3)]
    people = np.array([[[x, y, 0.0, 0.0, 0.0] for x, y in pts]])
    wp = np.tile(np.array([[12.0, 0.5], [-12.0, 0.5]])[None, None], (1, 3, 1, 1))
    return dict(people=people, cursor=np.zeros((1, 3), np.int32), pose=np.array([[50.0, 50.0, 0.0]]), twist=np.zeros((1, 2)),
                count=np.full(1, 3, np.int32), waypoints=wp, n_waypoints=np.full((1, 3), 2, np.int32),
                group_id=np.zeros((1, 3), np.int32))


def spread_after(stepper, grouped):
    """the largest member-to-centre distance after BEHAVIOUR_STEPS steps; stepper(people, cursor, d, group_id or None)"""
    d = behaviour_inputs()
    people, cursor = d["people"], d["cursor"]
    for _ in range(BEHAVIOUR_STEPS):
        people, cursor = stepper(people, cursor, d, d["group_id"] if grouped else None)
    centre = people[0, :, 0:2].mean(axis=0)
    return float(np.hypot(*(people[0, :, 0:2] - centre).T).max())


# the checker's two values (tests/test_crowd_groups.py reproduces them on the CPU to 1e-6) and their gap, of which
# tests/test_gpu_crowd_groups.py asserts at least half on the device
SPREAD_GROUPED, SPREAD_ALONE = 0.6205492097501201, 1.655592541437783   # metres; the gap is 1.0350 m


# ---- a person whose total force has a -0.0 component and whose velocity is zero (row 0): it stands without a goal, the
# robot stands 1e4 m away on the diagonal, so its social term underflows to (+0.0, -0.0); row 1 walks 40 m away
def negative_zero_inputs():
    people = np.array([[[0.0, 0.0, 0.0, 0.0, 0.0], [40.0, -3.0, 0.3, 0.2, 0.0], [41.0, -2.5, 0.1, -0.3, 0.0]]])
    return dict(people=people, cursor=np.zeros((1, 3), np.int32), pose=np.array([[1e4, 1e4, 0.0]]), twist=np.zeros((1, 2)),
                count=np.array([1], np.int32), waypoints=np.zeros((1, 3, 1, 2)), n_waypoints=np.zeros((1, 3), np.int32))
