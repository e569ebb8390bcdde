"""The inputs that aim the obstacle critic's costmap gather (csrc/smpc_bicubic.hpp) at map borders, small and non-square
maps and mixed waves, shared by tests/test_obstacle_edges.py (which shows, with the checkers alone, that the table reaches
what it is there for) and tests/test_gpu_obstacle_edges.py (which runs it on the device). numpy only; not a test module,
imported like crowd_cases.py.

A case is make_scenes(prm, B, N, map_cells=2, ...) with the README parameter set, whose costmap, costmap_origin and
resolution are then replaced: the map has a value in every tap (`noise`: independent uniform bytes; `smooth`: three
sinusoids of period 5 .. 15 cells, quantised, 0 .. 253), and the map is laid under the trajectory, not the trajectory on
the map: front_points() restates the rollout of oracle/pyref.py and the 0.25 m front offset in numpy, and every scene's
origin is `reduce(front[b]) - target * resolution` per axis, by the scene's placement rule (the rules of a case are dealt
to its scenes in turn, so neighbouring scenes - the two slots of a wave - are placed differently unless the case has one
rule).

Where the robot stands: the reference forms the cell coordinate as (front - origin) / resolution, a difference of two world
coordinates. A rollout of 28 additions at |x| = 1000 m carries about 3e-13 m of rounding in the oracle itself; at 0.025 m
per cell on a noise map (second differences of several hundred per cell) that alone moves a Jacobian entry of order one by
1e-7, far beyond JAC_RTOL, for any implementation. So make_case() moves every scene to within half a metre of `offset`,
the offset is zero for the noise maps and the fine resolutions, and the cases whose origins are about 1e3 m away use
`smooth` maps at 0.1 and 0.3 m per cell, where the same rounding stays under 1e-9.
"""
from typing import NamedTuple, Optional, Tuple

import numpy as np

from nav2_social_mpc_controller_amd.params import OptimizerParams
from nav2_social_mpc_controller_amd.scenes import make_scenes

README = OptimizerParams.readme()
FRONT_OFFSET = 0.25                  # critics/obstacle_cost_function.hpp:152
EPS = 1e-9                           # how close to a cell boundary the "just inside / just outside" targets sit
BANDS = ("< -1", "-1", "0", "1", "2 .. size-4", "size-3", "size-2", "size-1", "size", "> size")
# (T, N): the README shape (two slots per wave, also the fixed-shape instantiation); T = 31, a slot without a lane behind
# T; T = 1; a one-slot shape; a one-slot shape with helper lanes
SHAPES = {"readme": (28, 8), "t31": (31, 5), "t1": (1, 3), "one_slot": (36, 4), "helpers": (40, 16)}
PAD_LIMIT = 128                      # cases further than this many cells from their map have no padded twin


def lo(off=0.0):
    return ("lo", off)               # off


def hi(off=0.0):
    return ("hi", off)               # size + off


def mid(off=0.0):
    return ("mid", off)              # size / 2 + off


def pin(sel, tx, ty, sely=None):
    """A placement rule: per axis (which front point, where it lands). sel: a step (negative: from the end), "half"
    (step T // 2), or "min" / "max" / "mid" of the axis' coordinate over the steps."""
    return ((sel, tx), (sel if sely is None else sely, ty))


def far(side_x, side_y, cells):
    """The whole trajectory `cells` cells and a half outside the map on the given side(s) (-1, 0: centred, +1)."""
    ax = lambda s: ("max", lo(-cells - 0.5)) if s < 0 else ("min", hi(cells + 0.5)) if s > 0 else ("mid", mid())
    return (ax(side_x), ax(side_y))


def edge(axis, which, inside):
    """The interior test's boundary: the minimum (maximum) over the steps of the axis' coordinate is 1 + EPS (size - 2 -
    EPS) when `inside`, so that a lane sits on the last interior cell, and 1 - EPS (size - 2 + EPS) otherwise, so that one
    lane falls out; the other axis is centred."""
    s = EPS if inside else -EPS
    r = ("min", lo(1.0 + s)) if which == "min" else ("max", hi(-2.0 - s))
    return (r, ("mid", mid())) if axis == "x" else (("mid", mid()), r)


DIRECTIONS = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)]
INSIDE = pin("mid", mid(), mid())
# around and across a map of any size: fractional parts 0 (on a cell boundary), 0.5, and EPS either side of an integer
AROUND = [pin(0, lo(-1.5), lo(-1.5)), INSIDE, pin(-1, hi(0.5), hi(0.5)), pin(0, lo(0.0), hi(0.0)),
          pin(-1, lo(1.0 + EPS), hi(-1.0 - EPS)), pin("mid", hi(-EPS), lo(EPS)), pin("half", lo(0.5), mid(0.5)),
          pin("half", mid(0.0), hi(-0.5)), pin("half", lo(1.0 - EPS), lo(2.0)), pin(0, hi(-2.0 + EPS), hi(-3.0)),
          pin("min", lo(-1.0 + EPS), lo(-1.0 - EPS), sely="max"), pin("max", hi(1.0), hi(-1.0), sely="min")]
# each scene crosses one of the four borders in the middle of its trajectory
CROSSING = [pin("half", lo(0.25), mid()), pin("half", hi(-0.75), mid()), pin("half", mid(), lo(0.5)),
            pin("half", mid(), hi(-0.5))]


class Case(NamedTuple):
    size_x: int
    size_y: int
    resolution: float
    kind: str                               # "noise" | "smooth"
    shared: bool                            # one map for the batch, else one per scene
    rules: tuple                            # dealt to the scenes in turn
    shape: str = "readme"
    B: int = 16
    seed: int = 0
    offset: Tuple[float, float] = (0.0, 0.0)
    heading: Optional[str] = None           # "x" / "y": every start heading within 0.2 rad of that axis
    no_people: int = 0                      # every no_people-th scene has has_people = 0
    claim: Optional[tuple] = None           # ("edge", axis, which, inside): what the coverage test holds the case to
    solve: bool = False                     # also run through the solve (smooth maps)


def _band_targets(size):
    """one cell per band of an axis of `size` cells (the bands of a small size coincide), as centre coordinates"""
    cells = {-3, -1, 0, 1, size - 3, size - 2, size - 1, size, size + 2}
    if size >= 6:
        cells.add(2)
    return [c + 0.5 for c in sorted(cells)]


def _band_rules(size_x, size_y):
    return [pin("half", lo(tx), lo(ty)) for ty in _band_targets(size_y) for tx in _band_targets(size_x)]


def _table():
    t = {}
    res4 = (0.3, 0.1, 0.05, 0.025)
    shapes = ("readme", "t31", "one_slot", "helpers", "t1")
    n = 0
    # maps narrower than one patch (the byte-by-byte path), 1 x 1 among them
    for sx in (1, 2, 3):
        for sy in (1, 3, 9):
            t[f"narrow_{sx}x{sy}"] = Case(sx, sy, res4[n % 4], "noise", n % 2 == 1, tuple(AROUND), shapes[n % 5],
                                          B=15 if n % 3 == 0 else 24, seed=100 + n, no_people=5 if n % 2 else 0)
            n += 1
    # the smallest maps that take the dword paths
    for sx in (4, 5):
        for sy in (1, 2, 3, 4, 7):
            t[f"small_{sx}x{sy}"] = Case(sx, sy, res4[n % 4], "noise", n % 2 == 1, tuple(AROUND), shapes[n % 5],
                                         B=15 if n % 3 == 0 else 24, seed=100 + n, no_people=4 if n % 2 else 0)
            n += 1
    # non-square maps, both ways, the trajectories along x and along y
    for sx, sy in ((37, 9), (9, 37), (64, 40), (40, 64)):
        for heading in ("x", "y"):
            t[f"nonsquare_{sx}x{sy}_{heading}"] = Case(sx, sy, res4[n % 4], "noise", n % 2 == 1, tuple(AROUND),
                                                       shapes[n % 4], B=24, seed=100 + n, heading=heading)
            n += 1
    # origins: negative and no multiple of the resolution; about 1e3 m away (smooth and coarse: the module docstring)
    t["origin_negative"] = Case(23, 17, 0.05, "noise", False, tuple(AROUND), B=24, seed=140, offset=(-3.3337, -7.7713))
    t["origin_1e3_a"] = Case(23, 17, 0.3, "smooth", False, tuple(AROUND), B=24, seed=141, offset=(-1234.5678, 987.654321))
    t["origin_1e3_b"] = Case(17, 23, 0.1, "smooth", True, tuple(AROUND), "one_slot", B=24, seed=142,
                             offset=(1000.1, -1000.3))
    # the whole trajectory 3, 10 and 1e6 cells outside, on the four sides and at the four corners
    for cells, (sx, sy), res, shape in ((3, (40, 64), 0.05, "readme"), (10, (9, 37), 0.1, "t31"),
                                        (10 ** 6, (5, 7), 0.3, "readme"), (3, (3, 9), 0.05, "helpers"),
                                        (10 ** 6, (2, 3), 0.025, "one_slot")):
        t[f"far_{cells}_{sx}x{sy}"] = Case(sx, sy, res, "noise", False, tuple(far(dx, dy, cells) for dx, dy in DIRECTIONS),
                                           shape, B=16, seed=150 + len(t))
    # the interior test's boundary cells; every scene of the batch placed the same way
    for sx, sy in ((64, 40), (40, 64)):
        for k, (axis, which) in enumerate((("x", "min"), ("x", "max"), ("y", "min"), ("y", "max"))):
            for inside in (True, False):
                shape = ("readme", "readme", "t31", "one_slot")[(k + (sx == 40)) % 4]
                t[f"edge_{'in' if inside else 'out'}_{sx}x{sy}_{axis}{which}"] = Case(
                    sx, sy, 0.05, "noise", False, (edge(axis, which, inside),), shape, B=15 if k == 3 else 16,
                    seed=160 + len(t), claim=("edge", axis, which, inside))
    # mixed waves: even scenes interior and odd scenes off the map, the reverse, and scenes that cross a border
    t["mixed_even_in"] = Case(40, 64, 0.05, "noise", False, (INSIDE, far(1, 0, 5)), B=16, seed=180)
    t["mixed_odd_in"] = Case(64, 40, 0.05, "noise", False, (far(0, -1, 5), INSIDE), B=15, seed=181, no_people=3)
    t["mixed_t31"] = Case(40, 64, 0.05, "noise", False, (INSIDE, far(-1, 1, 3)), "t31", B=16, seed=182)
    t["crossing"] = Case(64, 40, 0.05, "noise", False, tuple(CROSSING), B=16, seed=203)
    t["crossing_helpers"] = Case(40, 64, 0.1, "noise", False, tuple(CROSSING), "helpers", B=12, seed=184)
    # one (scene, step) on every pair of bands: a wide map (the dword paths) and a narrow one (the byte path)
    for name, (sx, sy), res in (("bands_wide", (13, 11), 0.1), ("bands_narrow", (3, 9), 0.1)):
        rules = _band_rules(sx, sy)
        half = (len(rules) + 1) // 2
        t[name + "_a"] = Case(sx, sy, res, "noise", False, tuple(rules[:half]), B=half, seed=190)
        t[name + "_b"] = Case(sx, sy, res, "noise", False, tuple(rules[half:]), B=len(rules) - half, seed=191)
    # the smooth-map cases that also go through the solve: narrow, non-square, border-crossing, far-off, mixed waves
    s = dict(kind="smooth", shared=False, B=32, solve=True)
    t["solve_narrow_3x9"] = Case(3, 9, 0.1, rules=tuple(AROUND), seed=200, **s)
    t["solve_narrow_2x3"] = Case(2, 3, 0.3, rules=tuple(AROUND), seed=201, **s)
    t["solve_nonsquare_37x9"] = Case(37, 9, 0.05, rules=tuple(AROUND), seed=202, heading="x", **s)
    t["solve_nonsquare_40x64"] = Case(40, 64, 0.025, rules=tuple(AROUND), seed=203, heading="y", **s)
    t["solve_crossing"] = Case(64, 40, 0.05, rules=tuple(CROSSING), seed=204, no_people=5, **s)
    t["solve_far"] = Case(9, 37, 0.1, rules=tuple(far(dx, dy, 3) for dx, dy in DIRECTIONS), seed=205, **s)
    t["solve_mixed"] = Case(40, 64, 0.05, rules=(INSIDE, far(1, 0, 5), far(0, -1, 3), INSIDE), seed=206, **s)
    return t


CASES = _table()
SOLVE_CASES = [n for n, c in CASES.items() if c.solve]


# ---------------------------------------------------------------------------------------------------------------------
# maps

def noise_map(n, size_y, size_x, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, size_y, size_x), dtype=np.uint8)


def smooth_map(n, size_y, size_x, seed):
    """Three sinusoids (along x, along y, diagonal) of period 5 .. 15 cells with seeded periods and phases, 0 .. 253."""
    g = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(size_y, dtype=np.float64), np.arange(size_x, dtype=np.float64), indexing="ij")
    period = g.uniform(5.0, 15.0, (n, 3))[:, :, None, None]
    phase = g.uniform(0.0, 2.0 * np.pi, (n, 3))[:, :, None, None]
    arg = np.stack([x, y, (x + y) / np.sqrt(2.0)])[None] * (2.0 * np.pi / period) + phase
    v = 126.5 + 42.0 * np.sin(arg).sum(axis=1)
    return np.ascontiguousarray(np.floor(np.clip(v, 0.0, 253.0)).astype(np.uint8))


def constant_windows(costmap):
    """How many 4 x 4 windows (clipped to the map on an axis shorter than 4) of maps [n, size_y, size_x] are constant."""
    n, sy, sx = costmap.shape
    wy, wx = min(4, sy), min(4, sx)
    count = 0
    for i in range(sy - wy + 1):
        for j in range(sx - wx + 1):
            w = costmap[:, i:i + wy, j:j + wx].reshape(n, -1)
            count += int((w.max(axis=1) == w.min(axis=1)).sum())
    return count


# ---------------------------------------------------------------------------------------------------------------------
# the rollout of the front point, and the placement of a map under it

def front_points(prm, sc, x):
    """front[b, i]: the point the obstacle critic of step i of scene b samples at parameters x [B, P] (oracle/pyref.py's
    rollout: the pose after i + 1 steps; block j // bl while j < CH, then the last block; 0.25 m ahead of the pose)."""
    T, dt = sc.T, sc.dt
    CH, bl = prm.dims(T, True)[0:2]
    last = (CH - 1) // bl
    px, py, th = sc.pose0[:, 0].copy(), sc.pose0[:, 1].copy(), sc.pose0[:, 2].copy()
    out = np.empty((sc.B, T, 2))
    for j in range(T):
        k = j // bl if j < CH else last
        v, w = x[:, 2 * k], x[:, 2 * k + 1]
        px = px + v * np.cos(th) * dt
        py = py + v * np.sin(th) * dt
        th = th + w * dt
        out[:, j, 0] = px + FRONT_OFFSET * np.cos(th)
        out[:, j, 1] = py + FRONT_OFFSET * np.sin(th)
    return out


def cell_coordinates(prm, sc, x):
    """(col, row) coordinates [B, T, 2] of every front point in its scene's map, by the reference's quotient."""
    origin = np.broadcast_to(sc.costmap_origin, (sc.B, 2))
    return (front_points(prm, sc, x) - origin[:, None, :]) / sc.resolution


def _target(t, size):
    base, off = t
    return {"lo": 0.0, "hi": float(size), "mid": 0.5 * size}[base] + off


def _reduce(sel, f):
    """f [T] -> the coordinate the rule speaks of"""
    if sel == "min":
        return f.min()
    if sel == "max":
        return f.max()
    if sel == "mid":
        return 0.5 * (f.min() + f.max())
    return f[len(f) // 2] if sel == "half" else f[sel]


def place(case, front):
    """costmap_origin [B, 2] by the case's rules: origin = reduce(front[b]) - target * resolution on each axis"""
    origin = np.empty((front.shape[0], 2))
    for b in range(front.shape[0]):
        rule = case.rules[b % len(case.rules)]
        for axis, size in ((0, case.size_x), (1, case.size_y)):
            sel, t = rule[axis]
            origin[b, axis] = _reduce(sel, front[b, :, axis]) - _target(t, size) * case.resolution
    return origin


def _move(sc, case):
    """every scene moved as a whole: its start position to case.offset + (what make_scenes drew around its map centre,
    within half a metre), and turned about it so that the start heading lies along case.heading"""
    B = sc.B
    old = sc.pose0[:, 0:2].copy()
    centre = sc.costmap_origin + 0.5 * sc.size_x * sc.resolution
    new = np.asarray(case.offset)[None, :] + (old - centre)
    phi = np.zeros(B)
    if case.heading is not None:
        jitter = 0.4 * (np.random.default_rng(case.seed + 7).random(B) - 0.5)
        phi = ({"x": 0.0, "y": 0.5 * np.pi}[case.heading] + jitter) - sc.pose0[:, 2]
    c, s = np.cos(phi), np.sin(phi)

    def turn(px, py):   # [B, ...] world points
        shape = (B,) + (1,) * (px.ndim - 1)
        dx, dy = px - old[:, 0].reshape(shape), py - old[:, 1].reshape(shape)
        cc, ss = c.reshape(shape), s.reshape(shape)
        return new[:, 0].reshape(shape) + cc * dx - ss * dy, new[:, 1].reshape(shape) + ss * dx + cc * dy

    sc.pose0[:, 0], sc.pose0[:, 1] = turn(sc.pose0[:, 0], sc.pose0[:, 1])
    sc.pose0[:, 2] += phi
    sc.path_pts[:, :, 0], sc.path_pts[:, :, 1] = turn(sc.path_pts[:, :, 0], sc.path_pts[:, :, 1])
    sc.goal_yaw += phi
    if sc.N > 0:
        sc.people[:, :, 0, :], sc.people[:, :, 1, :] = turn(sc.people[:, :, 0, :], sc.people[:, :, 1, :])
        sc.people[:, :, 2, :] += phi[:, None, None]


_cache = {}


def make_case(name):
    """(params, scenes) of a case; built once per session and left unchanged (callers copy with select())."""
    if name not in _cache:
        c = CASES[name]
        T, N = SHAPES[c.shape]
        sc = make_scenes(README, c.B, N, T=T, seed=0x0B57AC1E + c.seed, map_cells=2, resolution=c.resolution)
        _move(sc, c)
        if c.no_people:
            sc.has_people[::c.no_people] = 0
        n = 1 if c.shared else c.B
        make = noise_map if c.kind == "noise" else smooth_map
        sc.costmap = make(n, c.size_y, c.size_x, 1000 + c.seed)
        origin = place(c, front_points(README, sc, sc.init_params))
        if c.shared:  # one origin: the rules are applied to scene 0's trajectory and the others lie where they lie
            origin = origin[:1]
        sc.costmap_origin = np.ascontiguousarray(origin)
        sc.costmap_shared = bool(c.shared)
        sc.resolution = float(c.resolution)
        sc.validate(sc.init_params.shape[1])
        _cache[name] = (README, sc)
    return _cache[name]


def perturbed(sc):
    """init_params + 0.05 * randn, seeded: the second point K1 is evaluated at"""
    return sc.init_params + 0.05 * np.random.default_rng(3).standard_normal(sc.init_params.shape)


# ---------------------------------------------------------------------------------------------------------------------
# bands, and the padded twin of a case

def bands(cell, size):
    """The names of the bands an integer cell of an axis of `size` cells belongs to (several where they coincide)."""
    out = set()
    if cell < -1:
        out.add("< -1")
    if cell > size:
        out.add("> size")
    for name, v in (("-1", -1), ("0", 0), ("1", 1), ("size-3", size - 3), ("size-2", size - 2), ("size-1", size - 1),
                    ("size", size)):
        if cell == v:
            out.add(name)
    if 2 <= cell <= size - 4:
        out.add("2 .. size-4")
    return out


def possible_bands(size):
    return set(BANDS) - (set() if size >= 6 else {"2 .. size-4"})


def interior(col, row, size_x, size_y):
    """bicubic_interior on integer cells: no tap of the 4 x 4 patch is clamped"""
    return (row >= 1) & (row <= size_y - 3) & (col >= 1) & (col <= size_x - 3)


def pad_cells(prm, sc):
    """How far the map has to be edge-replicated so that no tap of the case is clamped at init_params or at perturbed():
    the farthest cell outside, plus the patch and a margin of 4 cells; None beyond PAD_LIMIT."""
    worst = 0.0
    for x in (sc.init_params, perturbed(sc)):
        cc = cell_coordinates(prm, sc, x)
        worst = max(worst, -cc.min(), (cc[..., 0] - sc.size_x).max(), (cc[..., 1] - sc.size_y).max())
    p = int(np.ceil(worst)) + 3 + 4
    return p if p <= PAD_LIMIT else None


def padded(sc, p):
    """The same scenes on the map edge-replicated by p cells, origin - p * resolution: Grid2D's clamp, stated on the data."""
    out = sc.select(np.arange(sc.B))
    out.costmap = np.ascontiguousarray(np.pad(sc.costmap, ((0, 0), (p, p), (p, p)), mode="edge"))
    out.costmap_origin = np.ascontiguousarray(sc.costmap_origin - p * sc.resolution)
    return out


def obstacle_rows(prm, T, has_people):
    """(reference rows [T], critic-major rows [T]) of the obstacle critic of a full-horizon scene: the last critic of a
    step in the reference's order (8 rows per step with people, 5 without, a feasibility row behind steps 1 .. nfeas)"""
    rps = 8 if has_people else 5
    nfeas = prm.dims(T, has_people)[4] - rps * T
    t = np.arange(T)
    return rps * t + np.minimum(np.maximum(t - 1, 0), nfeas) + (rps - 1), (rps - 1) * T + t
