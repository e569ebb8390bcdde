"""Pairs next to theta = 0 and |theta| = pi for the three kernels that share the pair term of smpc_sfm.hpp (the people
projection, the per-robot crowd step and the pool step), and a statement of that term in mpmath at DIGITS digits.
TEST INFRASTRUCTURE ONLY: tests/test_social_pair.py shows on the CPU that every input built here meets its conditions and
that the checkers agree with the mpmath statement on them; tests/test_gpu_social_pair.py runs them on the device.

theta is the angle from the interaction direction i to the direction e towards the partner; its sign multiplies the lateral
force. A generated pair has theta = target (or sign(target) pi - target) with |target| between 1e-12 and 1e-3: the smallest
is about 300 times what the roundings of any double-precision statement can move theta by, so the sign is a property of the
inputs. Both ordered pairs of two persons have the same theta (e and i both flip).

What is NOT generated: exactly parallel pairs in a general direction, where i x e is pure rounding. There the reference's
sign is the last-bit noise of its libm (as for equal velocities, where the library takes theta = 0 by convention) and no
statement is right about it. The exactly parallel pairs here are the hand-written EXACT_ROWS along the coordinate axes
with binary-exact coordinates, where every statement's arithmetic is exact: head-on gives theta == 0.0 (no lateral
force), walking apart along the axis gives theta == +pi for both orders (the wrap into (-pi, pi]) and exact negatives."""
import math

import mpmath as mp
import numpy as np

import crowd_cases as G
import crowd_pool_cases as PC
import crowd_ref as R

DIGITS = 50
MAGNITUDES = (1e-12, 1e-10, 1e-8, 3e-7, 0.9e-6, 1.1e-6, 1e-5, 1e-4, 1e-3)   # 0.9e-6 / 1.1e-6: the kernels' switch of forms
TARGETS = tuple(s * t for t in MAGNITUDES for s in (1.0, -1.0))
FAMILIES = (False, True)         # near_pi
PER_TARGET = 40
DT = G.DT
MIN_JUMP = 1e-6                  # 2 F_SOCIAL |fa| dt of a designed pair: what a wrong sign moves a velocity by (1000 TOL)
FREE_SPEED = 3.0                 # desired speed of the persons of the crowd and pool scenes: no clamp hides the jump
GENERIC = 2 * G.CONDITIONS["theta"]


# ---- the pair term at DIGITS digits -----------------------------------------------------------------------------------------
def social_term_mp(dx, dy, ux, uy):
    """(fx, fy, theta) of one partner as mpmath numbers, from sfm.hpp:237-281 with the reference's default constants and the
    contract's two conventions: diff = (dx, dy) = partner - me (closer than 1e-6 m: (1e-6, 0)), u = my velocity - the
    partner's (2 u == 0 exactly: theta = 0). The arguments are doubles and are taken exactly."""
    with mp.workdps(DIGITS):
        dx, dy, ux, uy = (mp.mpf(float(v)) for v in (dx, dy, ux, uy))
        if dx * dx + dy * dy < mp.mpf(1e-12):
            dx, dy = mp.mpf(1e-6), mp.mpf(0)
        nd = mp.sqrt(dx * dx + dy * dy)
        ex, ey = dx / nd, dy / nd
        ivx, ivy = 2 * ux + ex, 2 * uy + ey
        il = mp.sqrt(ivx * ivx + ivy * ivy)
        ix, iy = ivx / il, ivy / il
        if ux == 0 and uy == 0:
            theta = mp.mpf(0)
        else:
            theta = mp.atan2(ix * ey - iy * ex, ix * ex + iy * ey)      # the angle from i to e, in (-pi, pi]
        B = mp.mpf("0.35") * il
        fv = -mp.exp(-nd / B - (3 * B * theta) ** 2)
        sign = 0 if theta == 0 else (1 if theta > 0 else -1)
        fa = -sign * mp.exp(-nd / B - (2 * B * theta) ** 2)
        F = mp.mpf("2.1")
        return F * (fv * ix + fa * (-iy)), F * (fv * iy + fa * ix), theta


def conditions_mp(dx, dy, ux, uy, near_pi):
    """(distance of theta from 0, or of |theta| from pi; sign of theta; 2 F |fa| DT) of one ordered pair, from social_term_mp
    alone"""
    with mp.workdps(DIGITS):
        fx, fy, theta = social_term_mp(dx, dy, ux, uy)
        dist = (mp.pi - abs(theta)) if near_pi else abs(theta)
        # F |fa| is the component of the term along the left normal of i
        dxm, dym, uxm, uym = (mp.mpf(float(v)) for v in (dx, dy, ux, uy))
        nd = mp.sqrt(dxm * dxm + dym * dym)
        ivx, ivy = 2 * uxm + dxm / nd, 2 * uym + dym / nd
        il = mp.sqrt(ivx * ivx + ivy * ivy)
        lateral = abs(fx * (-ivy / il) + fy * (ivx / il))               # F |fa|
        return float(dist), (0 if theta == 0 else (1 if theta > 0 else -1)), float(2 * lateral * DT)


def ordered(a, b):
    """(dx, dy, ux, uy) of the pair me = a, partner = b, in the doubles' own arithmetic (as every statement forms them)"""
    return float(b[0]) - float(a[0]), float(b[1]) - float(a[1]), float(a[2]) - float(b[2]), float(a[3]) - float(b[3])


# ---- the generator ----------------------------------------------------------------------------------------------------------
def near_axis_pair(rng, target, near_pi, centre=(0.0, 0.0), jitter=1.0):
    """Two states (x, y, vx, vy), me and partner, whose forward pair has theta ~ target (near_pi: sign(target) pi - target).
    Direction uniform; |diff| in [0.5, 2.5] and |interaction vector| in [0.6, 2.5] (near_pi: [0.4, 0.8] and [0.2, 0.5], which
    keeps exp(-(2 B theta)^2) away from 0 at pi); the partner's velocity uniform in [-0.5, 0.5]^2; me within `jitter` of centre."""
    phi = rng.uniform(-math.pi, math.pi)
    nd = rng.uniform(0.4, 0.8) if near_pi else rng.uniform(0.5, 2.5)
    il = rng.uniform(0.2, 0.5) if near_pi else rng.uniform(0.6, 2.5)
    ex, ey = math.cos(phi), math.sin(phi)
    # i = e turned by -theta; for theta = +-pi - t: cos theta = -cos t, sin theta = sin t
    c, s = (-math.cos(target) if near_pi else math.cos(target)), math.sin(target)
    idx, idy = ex * c + ey * s, -ex * s + ey * c
    dvx, dvy = (il * idx - ex) / R.LAMBDA, (il * idy - ey) / R.LAMBDA
    wx, wy = rng.uniform(-0.5, 0.5, 2)
    px, py = centre[0] + rng.uniform(-jitter, jitter), centre[1] + rng.uniform(-jitter, jitter)
    return np.array([px, py, wx + dvx, wy + dvy]), np.array([px + nd * ex, py + nd * ey, wx, wy])


_cache = {}


def pairs(near_pi, target):
    """the PER_TARGET seeded pairs of one family and target"""
    key = ("pairs", near_pi, target)
    if key not in _cache:
        rng = np.random.default_rng(7000 + 100 * int(near_pi) + TARGETS.index(target))
        _cache[key] = [near_axis_pair(rng, target, near_pi) for _ in range(PER_TARGET)]
    return _cache[key]


def all_pairs():
    """(near_pi, target, k, me, partner) of every generated pair"""
    return [(f, t, k, a, b) for f in FAMILIES for t in TARGETS for k, (a, b) in enumerate(pairs(f, t))]


# ---- exact rows -------------------------------------------------------------------------------------------------------------
def _axis_row(kind, axis, sign, negzero):
    """me and partner on a line parallel to a coordinate axis, `sign` the direction from me to the partner. head_on: they
    walk towards each other with unequal speeds; apart: me walks away from a partner that follows more slowly, so that
    i = -e. negzero: the coordinate difference across the line is -0.0 (me at 0.0, the partner at -0.0)."""
    off_me, off_pa = (0.0, -0.0) if negzero else (0.5, 0.5)
    s0, gap = 0.25, 1.5
    vm, vp = (0.5, -0.25) if kind == "head_on" else (-0.75, 0.25)
    me, pa = [0.0] * 4, [0.0] * 4
    me[axis], pa[axis] = sign * s0, sign * (s0 + gap)
    me[1 - axis], pa[1 - axis] = off_me, off_pa
    me[2 + axis], pa[2 + axis] = sign * vm, sign * vp
    return dict(name=f"{kind}_{'xy'[axis]}{'+' if sign > 0 else '-'}{'_negzero' if negzero else ''}", kind=kind, axis=axis,
                me=np.array(me), partner=np.array(pa))


EXACT_ROWS = [_axis_row(kind, axis, sign, nz) for nz in (False, True) for kind in ("head_on", "apart")
              for axis in (0, 1) for sign in (1.0, -1.0)]


# ---- embedding: the crowd step ----------------------------------------------------------------------------------------------
def _generic(g, others, centre=(0.0, 0.0), spread=3.0):
    """a walking person that keeps the margins of tests/crowd_cases.py to every state of `others`"""
    while True:
        sp, hd = g.uniform(0.2, 0.8), g.uniform(-math.pi, math.pi)
        p = np.array([centre[0] + g.uniform(-spread, spread), centre[1] + g.uniform(-spread, spread), sp * math.cos(hd),
                      sp * math.sin(hd)])
        if all(G._pair_ok(p, o) for o in others):
            return p


def crowd_batch(layouts, seed, Np, goals=True, visible=False):
    """A batch for R.step_batch / BatchSolver.crowd_step. layouts: per robot (pair or None, count, (lane of me, lane of the
    partner) or None); the other lanes below count hold generic persons. visible: Np = 1 and the PARTNER is the robot
    (pose and twist from its state). d["designed"]: (robot, lane of me, lane of the partner or -1 for the robot)."""
    g = np.random.default_rng(seed)
    B = len(layouts)
    people = np.zeros((B, Np, 5))
    pose, twist = np.zeros((B, 3)), np.zeros((B, 2))
    count = np.zeros(B, np.int32)
    designed = []
    for b, (pair, n, lanes) in enumerate(layouts):
        count[b] = n
        rows = [None] * n
        if pair is not None and visible:
            rows[0] = pair[0]
            pose[b] = [pair[1][0], pair[1][1], math.atan2(pair[1][3], pair[1][2])]
            twist[b, 0] = math.hypot(pair[1][2], pair[1][3])
            designed.append((b, 0, -1))
        elif pair is not None:
            rows[lanes[0]], rows[lanes[1]] = pair[0], pair[1]
            designed.append((b, lanes[0], lanes[1]))
        for i in range(n):
            if rows[i] is None:
                rows[i] = _generic(g, [r for r in rows if r is not None])
            people[b, i, 0:4] = rows[i]
    people[..., 4] = g.uniform(-1.0, 1.0, (B, Np))
    waypoints = g.uniform(-4.0, 4.0, (B, Np, 1, 2))
    n_wp = np.full((B, Np), 1 if goals else 0, np.int32)
    return dict(B=B, Np=Np, people=people, cursor=np.zeros((B, Np), np.int32), pose=pose, twist=twist, count=count,
                waypoints=waypoints, n_waypoints=n_wp, speeds=np.full((B, Np), FREE_SPEED), designed=designed, visible=visible)


def crowd_arguments(d, rows=slice(None)):
    """(positional, keyword) arguments of R.step_batch; call() of tests/test_gpu_crowd.py takes the same"""
    pos = (DT, d["people"][rows], d["cursor"][rows], d["pose"][rows], d["twist"][rows], d["count"][rows], d["waypoints"][rows],
           d["n_waypoints"][rows])
    return pos, dict(cyclic=True, robot_visible=d["visible"], desired_speeds=d["speeds"][rows], **G.PARAMS)


def robot_state(d, b):
    """(x, y, vx, vy) of robot b as the checker forms its velocity"""
    return np.array([d["pose"][b, 0], d["pose"][b, 1], d["twist"][b, 0] * math.cos(d["pose"][b, 2]),
                     d["twist"][b, 0] * math.sin(d["pose"][b, 2])])


def crowd_margins(d):
    """R.margins of every robot; theta over all pairs EXCEPT the designed one (the margins of the robot without the one
    and without the other person of the pair), everything else from the whole robot."""
    pos, kw = crowd_arguments(d)
    worst = dict(theta=math.inf, pair=math.inf, goal=math.inf, edge=math.inf, speed=math.inf)
    designed = {b: (i, j) for b, i, j in d["designed"]}
    for b in range(d["B"]):
        one, okw = G.robot_arguments(pos, kw, b)
        m = R.margins(*one, **okw)
        theta = m["theta"]
        if b in designed:
            theta = math.inf
            i, j = designed[b]
            if j >= 0:
                for drop in (i, j):
                    less = [np.delete(a, drop, axis=0) if k in (1, 2, 6, 7) else a for k, a in enumerate(one)]
                    less[5] = one[5] - 1
                    lkw = dict(okw, desired_speeds=np.delete(okw["desired_speeds"], drop))
                    theta = min(theta, R.margins(*less, **lkw)["theta"])
        for k in worst:
            worst[k] = min(worst[k], theta if k == "theta" else m[k])
    return worst


# ---- embedding: the pool step -----------------------------------------------------------------------------------------------
POOL_RANGE, POOL_SPACING, POOL_GENERIC = 3.5, 10.0, 3


def pool_case(items, seed):
    """One table of clusters, POOL_SPACING apart (further than the range): per item (me, partner) built around
    pool_centre(k), then POOL_GENERIC generic agents within range of both. Every row moves. c["designed"]: (row of me, row of
    the partner)."""
    g = np.random.default_rng(seed)
    rows, designed = [], []
    for k, (me, pa) in enumerate(items):
        c = pool_centre(k)
        cluster = [me, pa]
        for _ in range(POOL_GENERIC):
            cluster.append(_generic(g, cluster, centre=((me[0] + pa[0]) / 2, (me[1] + pa[1]) / 2), spread=0.7))
        assert all(math.hypot(q[0] - c[0], q[1] - c[1]) < (POOL_SPACING - POOL_RANGE) / 2 for q in cluster)
        designed.append((len(rows), len(rows) + 1))
        rows += cluster
    agents = np.concatenate([np.array(rows), g.uniform(-1.0, 1.0, (len(rows), 1))], axis=1)
    M = len(rows)
    lo, hi = -POOL_SPACING * 3.6, POOL_SPACING * 3.6
    return dict(agents=agents, M=M, cursor=np.zeros(M, np.int32), waypoints=g.uniform(lo, hi, (M, 1, 2)),
                n_waypoints=np.ones(M, np.int32), speeds=np.full(M, FREE_SPEED), dt=DT, range=POOL_RANGE, params=dict(PC.PARAMS),
                od=None, grid=PC.covering_grid(lo, hi, POOL_RANGE), designed=designed)


def pool_centre(k, n=7):
    """cluster k of a lattice of n columns around the origin (small coordinates keep the positions' roundings small)"""
    return (POOL_SPACING * (k % n - n // 2), POOL_SPACING * (k // n - n // 2))


def pool_margins(c):
    """PC.case_margins with theta over all in-range pairs except the designed ones: once with every `me` of a designed pair
    inert, once with every partner inert; the rest from the whole table."""
    m = PC.case_margins(c)
    theta = math.inf
    for side in (0, 1):
        a = c["agents"].copy()
        a[[p[side] for p in c["designed"]], 2] = math.nan
        theta = min(theta, PC.case_margins(c, agents=a)["theta"])
    return dict(m, theta=theta)


# ---- embedding: the projection ----------------------------------------------------------------------------------------------
def yaw_speed(state):
    return math.atan2(state[3], state[2]), math.hypot(state[2], state[3])


def as_walked(x, y, yaw, lv):
    """(x, y, vx, vy) with the velocity as oracle/pyref_sfm.py forms it from a yaw and a speed"""
    return np.array([x, y, lv * math.cos(yaw), lv * math.sin(yaw)])


def projection_case(pair, kind, N, lanes, T, seed):
    """A scene for oracle.pyref_sfm.project_people / BatchSolver.project_people (the dict of tests/test_projection.py's
    make_case): N valid persons and the robot. kind "pp": the designed pair are the persons lanes[0] and lanes[1]; "pr": me is
    person lanes[0] and the partner is the robot. The grid's one obstacle entry is its far corner. c["designed"] holds the
    two states (x, y, yaw, lv)."""
    g = np.random.default_rng(seed)
    dt = float(np.float32(0.05))
    states = [None] * (N + 1)                                   # x, y, yaw, lv; the robot last
    me, pa = pair                                               # (x, y, vx, vy), or (x, y, yaw, lv) with kind "pp_states"
    if kind == "pp_states":
        states[lanes[0]], states[lanes[1]] = tuple(me), tuple(pa)
    else:
        states[lanes[0]] = (me[0], me[1]) + yaw_speed(me)
        states[N if kind == "pr" else lanes[1]] = (pa[0], pa[1]) + yaw_speed(pa)
    for k in [N] + list(range(N)):                              # the robot first, so that every person keeps clear of it
        while states[k] is None:
            r, phi, hd = g.uniform(0.8, 3.0), g.uniform(-math.pi, math.pi), g.uniform(-math.pi, math.pi)
            s = (r * math.cos(phi), r * math.sin(phi), hd, g.uniform(0.2, 0.6 if k == N else 1.2))
            if all(G._pair_ok(as_walked(*s), as_walked(*o)) for o in states if o is not None):
                states[k] = s
    init = np.zeros((N, 6))
    for k in range(N):
        init[k] = [states[k][0], states[k][1], states[k][2], 0.0, states[k][3], 0.0]
    path = np.zeros((T + 1, 6))
    x, y, th, lv = states[N]
    w = g.uniform(-0.6, 0.6)
    for k in range(T + 1):
        path[k] = [x, y, th, k * dt, lv, w]
        x, y, th = x + lv * math.cos(th) * dt, y + lv * math.sin(th) * dt, th + w * dt
    grid = 120
    return dict(init=init, path=path, idx=np.zeros((grid, grid), np.uint32), origin=np.array([-6.0, -6.0]),
                res=float(np.float32(0.1)), max_time=1.5, dt=0.05, T=T, N=N, grid=grid,
                designed=(states[lanes[0]], states[N if kind == "pr" else lanes[1]]), states=states,
                designed_lanes=(lanes[0], N if kind == "pr" else lanes[1]))


def projection_conditions(c, near_pi):
    """conditions_mp of both orders of the designed pair, its velocities formed at DIGITS digits from the (yaw, speed)
    actually passed"""
    with mp.workdps(DIGITS):
        a, b = ([mp.mpf(float(s[0])), mp.mpf(float(s[1])), mp.mpf(float(s[3])) * mp.cos(mp.mpf(float(s[2]))),
                 mp.mpf(float(s[3])) * mp.sin(mp.mpf(float(s[2])))] for s in c["designed"])
        return _theta_conditions(a, b, near_pi)


def projection_margin(c):
    """the least distance from theta = 0 and |theta| = pi over all pairs of the scene's first step except the designed one"""
    s = [as_walked(*q) for q in c["states"]]
    worst = math.inf
    for i, a in enumerate(s):
        for j, b in enumerate(s):
            if i != j and {i, j} != set(c["designed_lanes"]):
                th = abs(R.pair_theta(*ordered(a, b))[0])
                worst = min(worst, th, abs(th - math.pi))
    return worst


# ---- the scenes of tests/test_gpu_social_pair.py: one launch each ---------------------------------------------------------
def _tagged(family_sign=None):
    """(near_pi, target) of every family and target, or of one family and one sign of the target"""
    return [(f, t) for f in FAMILIES for t in TARGETS if family_sign is None or (f, t > 0) == family_sign]


# lanes of (me, partner) and the round k that evaluates the pair (lane i takes partner (i + k) mod n; a trip holds the rounds
# kk in slot h = 0 and kk + 1 in slot h = 1; for even n the round k = n / 2 is the mutual one, without a hand-over)
TRIP_LAYOUTS = [(5, (0, 1)),    # n = 5, k = 1: slot 0 of the trip (1, 2); slot 1 holds a generic pair
                (5, (3, 0)),    # n = 5, k = 2 (lane 3 takes lane 0): slot 1 of the trip (1, 2); slot 0 holds a generic pair
                (4, (2, 3)),    # n = 4, k = 1: slot 0 of the trip (1, 2) whose slot 1 is the mutual round of generic pairs
                (4, (1, 3))]    # n = 4, k = 2: slot 1 of the trip (1, 2), the mutual round; slot 0 holds a generic pair


def _mutual():
    tags = _tagged()                                            # Np = count = 2: the one round is the mutual one; 32 robots
    return crowd_batch([(pairs(f, t)[2], 2, (0, 1)) for f, t in tags], 301, 2, goals=False), tags      # per wave, 36 robots


def _mutual_opposite():
    """the scene `mutual` with every pair's velocities shifted to exact negatives of each other: the positions and the
    velocity difference (halving and doubling are exact), and with them the pair term, are those of `mutual`"""
    d, tags = _mutual()
    half = (d["people"][:, 0, 2:4] - d["people"][:, 1, 2:4]) / 2
    d["people"][:, 0, 2:4], d["people"][:, 1, 2:4] = half, -half
    return d, tags


def _trips(f, positive):
    tags = [ft for ft in _tagged((f, positive)) for _ in TRIP_LAYOUTS]
    lay = [(pairs(f, t)[3 + k], n, lanes) for f, t in _tagged((f, positive)) for k, (n, lanes) in enumerate(TRIP_LAYOUTS)]
    return crowd_batch(lay + [(None, 5, None)], 310 + 2 * f + positive, 5), tags      # 8 robots per wave, 37 robots


def _wave(f, positive):
    """Np = 8, eight robots per wave: in wave w only robot 8 w + (w mod 8) holds a designed pair, at lane distance 1 + w mod 4
    (n = 8: the rounds 1 .. 4 in the trips (1, 2) and (3, 4), 4 the mutual one); three generic robots fill a last wave"""
    tags = _tagged((f, positive))
    lay = []
    for w, (ff, t) in enumerate(tags):
        for r in range(8):
            a = w % 3
            lay.append((pairs(ff, t)[7], 8, (a, a + 1 + w % 4)) if r == w % 8 else (None, 8, None))
    return crowd_batch(lay + [(None, 8, None)] * 3, 320 + 2 * f + positive, 8), tags


def _robot():
    tags = _tagged()                                            # Np = 1: 64 robots per wave, 36 robots
    return crowd_batch([(pairs(f, t)[8], 1, None) for f, t in tags], 330, 1, visible=True), tags


def _exact():
    return (crowd_batch([((r["me"], r["partner"]), 2, (0, 1)) for r in EXACT_ROWS], 340, 2, goals=False),
            [(r["name"], None) for r in EXACT_ROWS])


def _exact_trips():
    """every exact row in every slot of TRIP_LAYOUTS, among generic persons; one generic robot fills the last wave"""
    lay = [((r["me"], r["partner"]), n, lanes) for r in EXACT_ROWS for n, lanes in TRIP_LAYOUTS]
    return crowd_batch(lay + [(None, 5, None)], 341, 5), [(r["name"], None) for r in EXACT_ROWS for _ in TRIP_LAYOUTS]


CROWD_SCENES = {"mutual": _mutual, "exact_trips": _exact_trips, "mutual_opposite": _mutual_opposite, "robot": _robot, "exact": _exact,
                **{f"trips_{'pi' if f else '0'}_{'plus' if p else 'minus'}": (lambda f=f, p=p: _trips(f, p)) for f in FAMILIES for p in (True, False)},
                **{f"wave_{'pi' if f else '0'}_{'plus' if p else 'minus'}": (lambda f=f, p=p: _wave(f, p)) for f in FAMILIES for p in (True, False)}}


def crowd_scene(name):
    """(batch, [(near_pi, target) or (name of the exact row, None) per designed pair]), built once"""
    if ("crowd", name) not in _cache:
        _cache[("crowd", name)] = CROWD_SCENES[name]()
    return _cache[("crowd", name)]


def crowd_reference(name):
    """the checker's step of a crowd scene, computed once"""
    if ("crowd_ref", name) not in _cache:
        pos, kw = crowd_arguments(crowd_scene(name)[0])
        _cache[("crowd_ref", name)] = R.step_batch(*pos, **kw)
    return _cache[("crowd_ref", name)]


def robot_conditions(d, b, near_pi):
    """[(distance of theta from its axis, sign)] of both orders of person 0 and the robot of robot b, the robot's velocity
    formed at DIGITS digits from the (yaw, v) actually passed"""
    with mp.workdps(DIGITS):
        f = lambda v: mp.mpf(float(v))
        p = [f(v) for v in d["people"][b, 0, 0:4]]
        q = [f(d["pose"][b, 0]), f(d["pose"][b, 1]), f(d["twist"][b, 0]) * mp.cos(f(d["pose"][b, 2])),
             f(d["twist"][b, 0]) * mp.sin(f(d["pose"][b, 2]))]
        return _theta_conditions(p, q, near_pi)


def _theta_conditions(a, b, near_pi):
    out = []
    for p, q in ((a, b), (b, a)):
        dx, dy, ux, uy = q[0] - p[0], q[1] - p[1], p[2] - q[2], p[3] - q[3]
        nd = mp.sqrt(dx * dx + dy * dy)
        ivx, ivy = 2 * ux + dx / nd, 2 * uy + dy / nd
        theta = mp.atan2(ivx * dy - ivy * dx, ivx * dx + ivy * dy)
        out.append((float((mp.pi - abs(theta)) if near_pi else abs(theta)), 1 if theta > 0 else -1))
    return out


def pool_scene():
    """(case, tags): one cluster per family and target, then the exact rows apart_x+ and head_on_y-"""
    if "pool" not in _cache:
        tags = _tagged()
        rng = np.random.default_rng(350)
        items = [near_axis_pair(rng, t, f, centre=pool_centre(k), jitter=0.1) for k, (f, t) in enumerate(tags)]
        for name in ("apart_x+", "head_on_y-"):
            r = next(r for r in EXACT_ROWS if r["name"] == name)
            c = pool_centre(len(items))
            shift = np.array([c[0], c[1], 0.0, 0.0])            # a multiple of POOL_SPACING: the sums are exact
            items.append((r["me"] + shift, r["partner"] + shift))
            tags = tags + [(name, None)]
        _cache["pool"] = (pool_case(items, 351), tags)
    return _cache["pool"]


# N, kind, lanes, T, index into pairs(); lane g of a copy takes partner (g + k) mod (N + 1), the robot is lane N
PROJECTION_SCENES = {
    "n1_pr_T1": (1, "pr", (0,), 1, 9),       # n_act = 2: the mutual round of copy 0
    "n1_pr_T2": (1, "pr", (0,), 2, 10),
    "n3_pp_T1": (3, "pp", (0, 1), 1, 11),    # n_act = 4, H = 2: k = 1, the one round of copy 0 (copy 1 has the mutual round)
    "n3_pp_T2": (3, "pp", (0, 1), 2, 12),
    "n3_pr_T2": (3, "pr", (2,), 2, 13),      # lane 2 takes the robot in round 1
    "n8_pp_T2": (8, "pp", (0, 3), 2, 14),    # n_act = 9, H = 2: copy 0 has the trip (1, 3); k = 3 is its second slot
    "n8_pr_T1": (8, "pr", (5,), 1, 15),      # lane 5 takes the robot (lane 8) in round 3: the second slot of copy 0's trip
    "exact_T1": (2, "pp_states", (0, 1), 1, None),      # the exact rows along x: n_act = 3, the one round of copy 0
    "exact_n8_T1": (8, "pp_states", (0, 3), 1, None),   # the same rows in the second slot of copy 0's trip
}


def projection_scene(name):
    """[(near_pi, target, case)] of one launch; the exact rows (along x, where cos 0 = 1 and sin 0 = 0 keep the velocities
    exact: yaw = 0 and a signed speed) come as (name of the row, None, case)"""
    if ("proj", name) not in _cache:
        N, kind, lanes, T, k = PROJECTION_SCENES[name]
        if kind == "pp_states":
            out = []
            for n, r in enumerate(r for r in EXACT_ROWS if r["axis"] == 0):
                st = [(q[0], q[1], 0.0, q[2]) for q in (r["me"], r["partner"])]
                out.append((r["name"], None, projection_case(st, kind, N, lanes, T, 400 + 10 * N + n)))
        else:
            out = [(f, t, projection_case(pairs(f, t)[k], kind, N, lanes, T, 410 + 40 * k + n)) for n, (f, t) in enumerate(_tagged())]
        _cache[("proj", name)] = out
    return _cache[("proj", name)]
