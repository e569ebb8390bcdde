"""The seeded inputs of the pool-crowd-step tests, shared by tests/test_crowd_pool.py (which shows, with the checker alone,
that they stay clear of every decision the rules take, and states each case's largest partner count) and
tests/test_gpu_crowd_pool.py (which runs them on the device). A case is a dict: agents [A,5], M, cursor, waypoints,
n_waypoints, speeds (or None), dt, range, params (goal_radius, person_radius, desired_speed, cyclic), od (None or
(indexes, origin, resolution)) and grid (grid_x, grid_y, grid_origin, bin_size)."""
import math

import numpy as np

import crowd_pool_ref as P

MARGIN = 1.0 + 2.0 ** -20
KMAX, RES = 3, 0.25
# the least distance of every case from each decision the rules take (tests/test_crowd_pool.py asserts them)
CONDITIONS = {"theta": 1e-9, "goal": 1e-9, "edge": 1e-9, "speed": 1e-9}
PARAMS = dict(goal_radius=0.25, person_radius=0.35, desired_speed=0.6, cyclic=True)


def grid_for(rng, origin=(0.0, 0.0), gx=1, gy=1, factor=1.0):
    return dict(grid_x=int(gx), grid_y=int(gy), grid_origin=np.asarray(origin, np.float64),
                bin_size=float(np.float64(rng) * np.float64(MARGIN)) * factor)


def covering_grid(lo, hi, rng, factor=1.0):
    """bins of the least size (times factor) that cover the square [lo, hi]^2"""
    size = float(np.float64(rng) * np.float64(MARGIN)) * factor
    n = max(1, int(math.ceil((hi - lo) / size)))
    return grid_for(rng, (lo, lo), n, n, factor)


def walkers(g, n, lo, hi, standing=0.15):
    """n rows x, y, vx, vy, vz uniform on [lo, hi]^2; `standing` of them stand"""
    sp, hd = g.uniform(0.2, 0.8, n), g.uniform(-math.pi, math.pi, n)
    sp[g.random(n) < standing] = 0.0
    xy = g.uniform(lo, hi, (n, 2)) if np.ndim(lo) == 0 else lo + g.random((n, 2)) * (np.asarray(hi) - np.asarray(lo))
    return np.concatenate([xy, (sp * np.cos(hd))[:, None], (sp * np.sin(hd))[:, None], g.uniform(-1.0, 1.0, (n, 1))], axis=1)


def build(agents, M, g, rng, grid, dt=0.05, od=None, speeds=True, lo=-4.0, hi=4.0, **params):
    """A case around a table: seeded waypoints (every third walking mover is about to arrive at its own), cursors anywhere
    in 0 .. n_waypoints, desired speeds."""
    agents = np.ascontiguousarray(agents, np.float64)
    wp = g.uniform(lo, hi, (M, KMAX, 2))
    n_wp = g.integers(0, KMAX + 1, M).astype(np.int32)
    cursor = (g.integers(0, KMAX + 1, M) % (n_wp + 1)).astype(np.int32)
    near = g.uniform(0.255, 0.30, M)
    for i in range(0, M, 3):
        v = agents[i, 2:4]
        if np.isfinite(agents[i, 0:4]).all() and math.hypot(*v) > 0.0:
            wp[i] = agents[i, 0:2] + near[i] * v / math.hypot(*v)
    return dict(agents=agents, M=int(M), cursor=cursor, waypoints=wp, n_waypoints=n_wp,
                speeds=g.uniform(0.3, 0.9, M) if speeds else None, dt=dt, range=float(rng), params={**PARAMS, **params}, od=od,
                grid=grid)


def od_grid(g, cells, origin):
    idx = g.integers(0, cells * cells, (cells, cells)).astype(np.uint32)
    idx[cells // 2, cells // 3] = cells * cells      # an entry that is no cell of the grid
    return idx, np.asarray(origin, np.float64), RES


def random_case(seed, M, S, lo, hi, rng, grid=None, od_cells=0, **kw):
    g = np.random.default_rng(seed)
    agents = walkers(g, M + S, lo, hi)
    od = od_grid(g, od_cells, (lo + 0.37, lo + 0.41)) if od_cells else None   # smaller than the floor: some movers are off it
    return build(agents, M, g, rng, grid or covering_grid(lo, hi, rng), od=od, lo=lo, hi=hi, **kw)


def neighbourhood(seed, Q, movers=1):
    """`movers` movers around (10, 10) whose 3 x 3 block holds exactly Q other rows (about half of them in range) among rows
    further away: the candidate loop's chunk boundaries."""
    g = np.random.default_rng(seed)
    rng = 2.0
    centre = walkers(g, movers, 9.9, 10.1, standing=0.0)
    ang, rad = g.uniform(0, 2 * math.pi, Q), g.uniform(0.3, 3.4, Q)         # bins of 2 m around (10, 10): all within 3 x 3
    around = walkers(g, Q, 0.0, 1.0)
    around[:, 0], around[:, 1] = 10.0 + rad * np.cos(ang), 10.0 + rad * np.sin(ang)
    far = walkers(g, 40, 0.0, 1.0)
    far[:, 0], far[:, 1] = g.uniform(16.5, 19.5, 40), g.uniform(0.5, 19.5, 40)
    agents = np.concatenate([centre, around, far])
    perm = np.concatenate([np.arange(movers), movers + g.permutation(Q + 40)])
    return build(agents[perm], movers, g, rng, grid_for(rng, (9.0 - 4 * 2.0 * MARGIN, 9.0 - 4 * 2.0 * MARGIN), 10, 10), lo=5.0, hi=15.0)


def crowded_bin(seed, n, S=6):
    """n movers in ONE bin of 3 m (and S static rows in the bins around it), all within range of each other"""
    g = np.random.default_rng(seed)
    rng = 3.0
    s = rng * MARGIN
    agents = np.concatenate([walkers(g, n, s + 0.5, s + 2.5), walkers(g, S, 0.2, 3 * s - 0.2)])
    return build(agents, n, g, rng, grid_for(rng, (0.0, 0.0), 3, 3), lo=0.0, hi=9.0)


def one_bin_1500(seed=31, M=96):
    """1,500 rows within 2.4 m x 2.4 m in ONE bin, every row a partner of every other; the first M move (all-pairs Python
    for 1,500 movers would take a minute; the candidate loop is the same for 96). dt = 0.02: 1499 * 2^-36 * 0.02 <= TOL / 2."""
    g = np.random.default_rng(seed)
    return build(walkers(g, 1500, 1.0, 3.4), M, g, 4.0, grid_for(4.0), dt=0.02, lo=0.0, hi=4.4)


def border_case(gx, gy):
    """rows all over a small grid and around it (they land in the border bins), some far outside; movers among them"""
    g = np.random.default_rng(gx * 10 + gy)
    rng = 1.5
    grid = grid_for(rng, (-2.0, 3.0), gx, gy)
    lo, hi = np.array([-2.0, 3.0]), np.array([-2.0, 3.0]) + np.array([gx, gy]) * grid["bin_size"]
    agents = walkers(g, 260, lo - 0.6 * (hi - lo), lo + 1.6 * (hi - lo))
    agents[:6, 0:2] = [[1e12, 4.0], [-1e12, 4.0], [0.0, 1e12], [0.5, 1e12], [1e12, 1e12], [1e12 + 1.0, 4.5]]
    return build(agents, 200, g, rng, grid, lo=-6.0, hi=12.0)


def bin_edges_case(seed=41):
    """pairs that straddle bin edges and corners of a 5 x 4 grid, within a few ulps and within the range of them"""
    g = np.random.default_rng(seed)
    rng = 1.0
    grid = grid_for(rng, (0.1, -0.3), 5, 4)
    s = grid["bin_size"]
    rows = []
    for ix in range(1, 5):
        for iy in range(1, 4):
            cx, cy = 0.1 + ix * s, -0.3 + iy * s
            for dx, dy in ((0.0, 0.0), (-1e-9, 1e-9), (0.4, -0.45), (-0.45, 0.4), (np.nextafter(0.0, 1.0), -0.3), (0.3, 0.0)):
                rows.append([cx + dx, cy + dy])
            rows.append([np.nextafter(cx, -np.inf), cy - 0.7])
            rows.append([cx + 0.7, np.nextafter(cy, np.inf)])
    agents = walkers(g, len(rows), 0.0, 1.0)
    agents[:, 0:2] = np.asarray(rows) + g.uniform(-1e-3, 1e-3, (len(rows), 2)) * (np.arange(len(rows)) % 2)[:, None]
    agents = agents[g.permutation(len(rows))]
    return build(agents, len(rows) - 10, g, rng, grid, lo=0.0, hi=5.0)


def waypoint_case(seed, cyclic, speeds):
    """arrival, wrap and stop at the last waypoint, n_waypoints = 0 and out-of-range cursors, by hand on top of a seeded table"""
    c = random_case(seed, 18, 3, -3.0, 3.0, 2.0, cyclic=cyclic, speeds=speeds)
    a, wp = c["agents"], c["waypoints"]
    for i, (n, cur, dist) in enumerate([(3, 2, 0.10), (3, 0, 0.10), (1, 0, 0.10), (0, 0, 0.10), (2, 2, 0.10), (3, -1, 0.10),
                                        (3, 1, 0.26), (2, 1, 0.2499), (3, 7, 0.10)]):
        a[i, 2:4] = [0.5, 0.1 * (i + 1)]
        c["n_waypoints"][i], c["cursor"][i] = n, cur
        wp[i, :, :] = a[i, 0:2] + dist * a[i, 2:4] / math.hypot(*a[i, 2:4]) + a[i, 2:4] * c["dt"]
    return c


def chain_case(seed=61):
    return random_case(seed, 40, 4, -3.0, 3.0, 2.5, od_cells=20, dt=0.05)


CASES = {
    "dense_4096_256": lambda: random_case(11, 4096, 256, 0.0, 40.0, 3.0, dt=0.05),
    "small_with_grid": lambda: random_case(12, 60, 7, -3.0, 3.0, 2.0, od_cells=20),
    "small_no_grid_no_speeds": lambda: random_case(13, 33, 0, -3.0, 3.0, 2.0, speeds=False, cyclic=False),
    "grid_1x1": lambda: border_case(1, 1),
    "grid_1x7": lambda: border_case(1, 7),
    "grid_7x1": lambda: border_case(7, 1),
    "bin_edges": bin_edges_case,
    **{f"candidates_{q}": (lambda q=q: neighbourhood(100 + q, q)) for q in (63, 64, 65, 129, 257)},
    **{f"movers_per_bin_{n}": (lambda n=n: crowded_bin(200 + n, n)) for n in (1, 63, 65, 257)},
    "one_bin_1500": one_bin_1500,
    **{f"waypoints_cyclic{int(cy)}_speeds{int(sp)}": (lambda cy=cy, sp=sp: waypoint_case(51, cy, sp))
       for cy in (True, False) for sp in (True, False)},
    "chain": chain_case,
}
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def ref_kwargs(c):
    kw = dict(desired_speeds=c["speeds"], **c["params"])
    if c["od"] is not None:
        kw.update(od_indexes=c["od"][0], od_origin=c["od"][1], od_resolution=c["od"][2])
    return kw


def ref_step(c, agents=None, cursor=None, M=None, **kw):
    """the checker's step of a case (optionally from other states)"""
    return P.step(c["dt"], c["agents"] if agents is None else agents, c["M"] if M is None else M,
                  c["cursor"] if cursor is None else cursor, c["waypoints"], c["n_waypoints"], c["range"], **ref_kwargs(c), **kw)


def reference(name, poison=None):
    """(next, cursor, largest partner count) of a case by the checker: computed once per session"""
    key = (name, poison)
    if key not in _cache:
        c, counts = case(name), []
        nxt, cur = ref_step(c, next=None if poison is None else np.full((c["M"], 5), poison), counts=counts)
        _cache[key] = (nxt, cur, max(counts, default=0))
    return _cache[key]


def case_margins(c, agents=None, cursor=None):
    kw = ref_kwargs(c)
    return P.margins(c["dt"], c["agents"] if agents is None else agents, c["M"], c["cursor"] if cursor is None else cursor,
                     c["waypoints"], c["n_waypoints"], c["range"], coincident_ok=True, **kw)
