"""CPU checker of smpc_crowd_pool_step_batch, written from the contract in include/smpc_crowd_pool.h: all pairs in plain
Python, no bins, libm exp / atan2 (through tests/crowd_ref.py's pair term), rule 4's sum in Python integers and none of the
library's code. TEST INFRASTRUCTURE ONLY.

step() advances the movers of one table and returns new arrays; margins() reports how far a step stays from every decision
the rules take and the largest number of partners a mover has."""
import math

import numpy as np

from crowd_ref import F_DESIRED, F_OBSTACLE, RELAX, SIGMA, TOL, heading, obstacle_of, pair_theta, social_term, wrap

FRACTION_BITS = 36
SCALE = 2.0 ** FRACTION_BITS
CLAMP = 8.0
QUANTUM = 2.0 ** -FRACTION_BITS


def quantize(t):
    """rule 4: round-to-nearest-even(clamp(t, -8, 8) * 2^36) as a Python integer; 0 for a NaN"""
    if t != t:
        return 0
    t = min(max(t, -CLAMP), CLAMP)
    return int(round(t * SCALE))     # the product is exact; Python's round() of a float rounds ties to even


def live(row):
    return all(math.isfinite(float(v)) for v in row[0:4])


def partners_of(agents, i, interaction_range):
    """rules 1 and 2: the rows c != i with finite x, y, vx, vy and d2 <= R * R, d2 = ddx * ddx + ddy * ddy with two products
    and a sum each rounded on its own (numpy's float64 does just that; an overflowing or NaN d2 fails the comparison)"""
    alive = np.isfinite(agents[:, 0:4]).all(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        ddx, ddy = agents[:, 0] - agents[i, 0], agents[:, 1] - agents[i, 1]
        xx, yy = ddx * ddx, ddy * ddy
        ok = alive & ((xx + yy) <= np.float64(interaction_range) * np.float64(interaction_range))
    ok[i] = False
    return np.nonzero(ok)[0].tolist()


def step(dt, agents, M, cursor, waypoints, n_waypoints, interaction_range, goal_radius=0.25, person_radius=0.35,
         desired_speed=0.6, cyclic=True, desired_speeds=None, od_indexes=None, od_origin=None, od_resolution=None,
         next=None, counts=None):
    """agents [A,5] (left alone), rows 0 .. M-1 move; cursor [M], waypoints [M,K,2], n_waypoints [M]. next [M,5]: the array
    before the call (default NaN). counts: a list that receives every mover's number of partners (-1: inert).
    Returns (next, cursor) as new arrays."""
    agents = np.array(agents, np.float64).reshape(-1, 5)
    cursor = np.array(cursor, np.int32)
    nxt = np.full((M, 5), np.nan) if next is None else np.array(next, np.float64)
    K = waypoints.shape[1] if M > 0 else 1
    for i in range(M):
        if not live(agents[i]):
            nxt[i] = agents[i]       # all five doubles (numpy copies the bits); the cursor stays
            if counts is not None:
                counts.append(-1)
            continue
        px, py, vx, vy = (float(v) for v in agents[i, 0:4])
        des = float(desired_speed if desired_speeds is None else desired_speeds[i])
        nwp = min(max(int(n_waypoints[i]), 0), K)
        cur = int(cursor[i])
        has_goal = 0 <= cur < nwp
        fx, fy = -vx / RELAX, -vy / RELAX
        if has_goal:
            gx, gy = (float(v) for v in waypoints[i, cur])
            d = math.sqrt((gx - px) ** 2 + (gy - py) ** 2)
            if d > goal_radius:
                fx = F_DESIRED * ((gx - px) / d * des - vx) / RELAX
                fy = F_DESIRED * ((gy - py) / d * des - vy) / RELAX
        sx = sy = 0                  # Python integers: rule 4
        who = partners_of(agents, i, interaction_range)
        for c in who:
            qx, qy, wx, wy = (float(v) for v in agents[c, 0:4])
            tx, ty = social_term(qx - px, qy - py, vx - wx, vy - wy)
            sx, sy = sx + quantize(tx), sy + quantize(ty)
        assert abs(sx) < 2 ** 63 and abs(sy) < 2 ** 63
        fx, fy = fx + float(sx) * QUANTUM, fy + float(sy) * QUANTUM
        if counts is not None:
            counts.append(len(who))
        o = obstacle_of(px, py, od_indexes, od_origin, od_resolution)
        if o is not None:
            mx, my = px - o[0], py - o[1]
            m = math.sqrt(mx * mx + my * my)
            e = F_OBSTACLE * math.exp(-(m - person_radius) / SIGMA)
            if m > 0.0:
                fx, fy = fx + e * mx / m, fy + e * my / m
        nvx, nvy = vx + fx * dt, vy + fy * dt
        sp = math.sqrt(nvx * nvx + nvy * nvy)
        if sp > des:
            nvx, nvy = nvx / sp * des, nvy / sp * des
        vz = wrap(heading(nvx, nvy) - heading(vx, vy)) / dt
        px, py = px + nvx * dt, py + nvy * dt
        if has_goal and math.sqrt((gx - px) ** 2 + (gy - py) ** 2) <= goal_radius:
            cur += 1
        if cyclic and cur >= nwp:
            cur = 0
        nxt[i] = [px, py, nvx, nvy, vz]
        cursor[i] = cur
    return nxt, cursor


def margins(dt, agents, M, cursor, waypoints, n_waypoints, interaction_range, goal_radius=0.25, od_indexes=None,
            od_origin=None, od_resolution=None, coincident_ok=False, **kw):
    """The least distances of one step from the rules' decisions, as crowd_ref.margins: theta (of an in-range pair with
    unequal velocities, from 0 and from +-pi), pair (metres between a mover and an in-range partner; exactly coincident
    ones are left out with coincident_ok), goal, edge, speed; and `partners`: the largest number of partners of a mover."""
    agents = np.array(agents, np.float64).reshape(-1, 5)
    counts = []
    new, _ = step(dt, agents, M, cursor, waypoints, n_waypoints, interaction_range, goal_radius=goal_radius,
                  od_indexes=od_indexes, od_origin=od_origin, od_resolution=od_resolution, counts=counts, **kw)
    m = dict(theta=math.inf, pair=math.inf, goal=math.inf, edge=math.inf, speed=math.inf, partners=max(counts, default=0))
    K = waypoints.shape[1] if M > 0 else 1
    for i in range(M):
        if not live(agents[i]):
            continue
        px, py, vx, vy = (float(v) for v in agents[i, 0:4])
        for c in partners_of(agents, i, interaction_range):
            qx, qy, wx, wy = (float(v) for v in agents[c, 0:4])
            d = math.hypot(qx - px, qy - py)
            if not (coincident_ok and d == 0.0):
                m["pair"] = min(m["pair"], d)
            if vx != wx or vy != wy:
                th = abs(pair_theta(qx - px, qy - py, vx - wx, vy - wy)[0])
                m["theta"] = min(m["theta"], th, abs(th - math.pi))
        cur = int(cursor[i])
        if 0 <= cur < min(max(int(n_waypoints[i]), 0), K):
            g = waypoints[i, cur]
            m["goal"] = min(m["goal"], abs(math.hypot(g[0] - new[i, 0], g[1] - new[i, 1]) - goal_radius))
        for q in (agents[i], new[i]):
            sp = math.hypot(q[2], q[3])
            if sp > 0.0:
                m["speed"] = min(m["speed"], sp)
            if od_indexes is not None:
                for c, o in ((q[0], od_origin[0]), (q[1], od_origin[1])):
                    t = (c - o) / float(np.float32(od_resolution))
                    m["edge"] = min(m["edge"], abs(t - round(t)) * float(np.float32(od_resolution)))
    return m


def bound(partners, dt):
    """What the device may differ by in a velocity: one unit of 2^-36 per partner (a flipped rounding), times dt."""
    return partners * QUANTUM * dt


def compare(got_next, got_cursor, want_next, want_cursor, dt, partners, what=""):
    """Positions, velocities and vz * dt (difference wrapped) within crowd_ref.TOL, cursors equal; asserts that this case's
    own bound partners * 2^-36 * dt stays within TOL / 2, and prints the largest differences. Rows that are not finite in
    the checker's result (inert movers) must be equal bit for bit."""
    assert bound(partners, dt) <= TOL / 2, (what, partners, dt)
    g, w = np.asarray(got_next, np.float64), np.asarray(want_next, np.float64)
    assert g.shape == w.shape, what
    fin = np.isfinite(w).all(axis=1) if len(w) else np.zeros(0, bool)
    assert np.array_equal(g[~fin].view(np.uint64), w[~fin].view(np.uint64)), what
    d = np.abs(g[fin, 0:4] - w[fin, 0:4])
    dz = (g[fin, 4] - w[fin, 4]) * dt
    dz = np.abs(np.arctan2(np.sin(dz), np.cos(dz)))
    worst = (float(d.max()) if d.size else 0.0, float(dz.max()) if dz.size else 0.0)
    print(f"{what}: max |d(p, v)| = {worst[0]:.3e}, max |d vz dt| = {worst[1]:.3e}, partners <= {partners}, "
          f"bound {bound(partners, dt):.3e}")
    assert worst[0] <= TOL and worst[1] <= TOL, (what, worst)
    assert np.array_equal(np.asarray(got_cursor), np.asarray(want_cursor)), what
