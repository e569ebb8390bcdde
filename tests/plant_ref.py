"""The sequential yardstick of the robot plant (include/smpc_plant.h states the rule): one robot after the other, numpy
float64 scalars with one operation per line, every substep's two clearances recomputed from scratch over all offsets of the
footprint and all agents. The cosine and sine of the heading are handed in (step 4 of the rule: everything behind them is a
pure function of c and s), so a caller compares bit for bit given the heading a device or a compiled rule obtained, and
holds that heading against numpy's separately (heading_close).

state = (pose [B,3] float64, twist [B,2] float64, queue [B,8,2] float64, tick [B] uint32); a tick is
{"cmd" [B,2], "agents" [B,Np,5], "count" [B] int32}; p is a dict of the call's scalars and the world (see params())."""
import numpy as np

F = np.float64
NONE = 1 << 64                      # above every key
FLAG_WALL, FLAG_AGENT, FLAG_WALL_CONTACT, FLAG_AGENT_CONTACT, FLAG_BAD_COMMAND, FLAG_BAD_STATE = 1, 2, 4, 8, 16, 32
COUNTERS = ("full", "blocked", "partial", "blocked_by_wall", "blocked_by_agent", "blocked_by_both", "wall_contact", "agent_contact",
            "bad_command", "bad_state", "slide", "left_contact", "clamped", "rate_limited")


def params(S=4, L=0, dt=0.1, v_min=0.0, v_max=0.6, w_max=1.4, dv_up=np.inf, dv_down=np.inf, dw=np.inf, contact_dist=0.0, world=None,
           origin=(0.0, 0.0), res=0.05, footprint_d2=-1, wall_min_cost=254, unknown_is_wall=False, outside_is_wall=False):
    world = None if world is None else np.ascontiguousarray(world, np.uint8)
    return dict(S=int(S), L=int(L), dt=F(dt), v_min=F(v_min), v_max=F(v_max), w_max=F(w_max), dv_up=F(dv_up), dv_down=F(dv_down),
                dw=F(dw), contact_dist=F(contact_dist), world=world, origin=(F(origin[0]), F(origin[1])), res=F(res),
                footprint_d2=int(footprint_d2), wall_min_cost=int(wall_min_cost), unknown_is_wall=bool(unknown_is_wall),
                outside_is_wall=bool(outside_is_wall))


def zero_state(B):
    return np.zeros((B, 3)), np.zeros((B, 2)), np.zeros((B, 8, 2)), np.zeros(B, np.uint32)


def clamp(a, lo, hi):
    return lo if a < lo else (hi if a > hi else a)


def bits(d):
    return int(np.array(d, np.float64).view(np.uint64))


def is_wall(p, x, y):
    world = p["world"]
    Hy, Hx = world.shape
    if x < 0 or y < 0 or x >= Hx or y >= Hy:
        return p["outside_is_wall"]
    cost = int(world[y, x])
    return p["unknown_is_wall"] if cost == 255 else cost >= p["wall_min_cost"]


def wall2(p, qx, qy):
    """The least squared offset within the footprint whose cell is a wall, or NONE."""
    if p["world"] is None or p["footprint_d2"] < 0:
        return NONE
    dx = qx - p["origin"][0]
    dy = qy - p["origin"][1]
    fx = np.floor(dx / p["res"])
    fy = np.floor(dy / p["res"])
    if not (abs(fx) <= 2.0 ** 30 and abs(fy) <= 2.0 ** 30):
        return NONE
    cx, cy, d2max = int(fx), int(fy), p["footprint_d2"]
    r = int(np.floor(np.sqrt(d2max)))
    best = NONE
    for jy in range(-r, r + 1):
        for jx in range(-r, r + 1):
            d2 = jx * jx + jy * jy
            if d2 <= d2max and d2 < best and is_wall(p, cx + jx, cy + jy):
                best = d2
    return best


def agent2(p, agents, n, qx, qy):
    """The least key (the bits of d2) over the agents in contact, or NONE."""
    c2 = p["contact_dist"] * p["contact_dist"]
    best = NONE
    for j in range(n):
        px, py = F(agents[j, 0]), F(agents[j, 1])
        if not (np.isfinite(px) and np.isfinite(py)):
            continue
        ax = px - qx
        ay = py - qy
        xx = ax * ax
        yy = ay * ay
        d2 = xx + yy
        if d2 < c2:
            best = min(best, bits(d2))
    return best


def step(state, tick, p, cs):
    """One period of every robot: (new state, contact [B,2] int32, counters {name: [B] int}). cs [B,2]: cosine and sine of
    every heading (rows of robots whose state is not finite are not read)."""
    pose, twist, queue, ticks = (np.array(a) for a in state)
    cmd, agents, count = np.asarray(tick["cmd"], F), np.asarray(tick["agents"], F), np.asarray(tick["count"])
    B, Np = agents.shape[0], agents.shape[1]
    S, L, dt = p["S"], p["L"], p["dt"]
    contact = np.zeros((B, 2), np.int32)
    counters = {k: np.zeros(B, np.int64) for k in COUNTERS}
    with np.errstate(all="ignore"):
        for b in range(B):
            # 1. latency
            if L > 0:
                i = int(ticks[b]) % L
                tv, tw = F(queue[b, i, 0]), F(queue[b, i, 1])
                queue[b, i] = cmd[b]
            else:
                tv, tw = F(cmd[b, 0]), F(cmd[b, 1])
            ticks[b] = np.uint32((int(ticks[b]) + 1) & 0xFFFFFFFF)
            # 2. finite
            x, y, th, v, w = F(pose[b, 0]), F(pose[b, 1]), F(pose[b, 2]), F(twist[b, 0]), F(twist[b, 1])
            if not all(np.isfinite(a) for a in (x, y, th, v, w)):
                twist[b] = 0.0
                contact[b] = (FLAG_BAD_STATE, 0)
                counters["bad_state"][b] += 1
                continue
            flags = 0
            if not (np.isfinite(tv) and np.isfinite(tw)):
                tv, tw = F(0.0), F(0.0)
                flags |= FLAG_BAD_COMMAND
                counters["bad_command"][b] += 1
            # 3. limits
            vt = clamp(tv, p["v_min"], p["v_max"])
            wt = clamp(tw, -p["w_max"], p["w_max"])
            delta = vt - v
            lim = p["dv_up"] if (v >= 0.0 and delta >= 0.0) or (v <= 0.0 and delta <= 0.0) else p["dv_down"]
            dstep = clamp(delta, -lim, lim)
            v1 = v + dstep
            wdelta = wt - w
            wstep = clamp(wdelta, -p["dw"], p["dw"])
            w1 = w + wstep
            counters["clamped"][b] += int(vt != tv or wt != tw)
            counters["rate_limited"][b] += int(dstep != delta or wstep != wdelta)
            # 4. heading, 5. segment
            c, s = F(cs[b, 0]), F(cs[b, 1])
            vc = v1 * c
            vs = v1 * s
            Lx = vc * dt
            Ly = vs * dt
            # 6., 7. clearances and the walk
            n = min(max(int(count[b]), 0), Np)
            qx, qy = x, y
            wk, ak = wall2(p, qx, qy), agent2(p, agents[b], n, qx, qy)
            if wk != NONE:
                flags |= FLAG_WALL_CONTACT
                counters["wall_contact"][b] += 1
            if ak != NONE:
                flags |= FLAG_AGENT_CONTACT
                counters["agent_contact"][b] += 1
            ak0, K = ak, 0
            for k in range(1, S + 1):
                f = F(k) / F(S)
                ex = Lx * f
                ey = Ly * f
                nx = x + ex
                ny = y + ey
                nwk, nak = wall2(p, nx, ny), agent2(p, agents[b], n, nx, ny)
                bw, ba = nwk < wk, nak < ak
                if bw or ba:
                    flags |= (FLAG_WALL if bw else 0) | (FLAG_AGENT if ba else 0)
                    counters["blocked"][b] += 1
                    counters["blocked_by_wall"][b] += int(bw)
                    counters["blocked_by_agent"][b] += int(ba)
                    counters["blocked_by_both"][b] += int(bw and ba)
                    break
                K, qx, qy, wk, ak = k, nx, ny, nwk, nak
            counters["full"][b] += int(K == S)
            counters["partial"][b] += int(0 < K < S)
            counters["slide"][b] += int(K == S and (flags & FLAG_WALL_CONTACT) != 0 and wk != NONE and v1 == vt and v1 != 0.0
                                        and (qx != x or qy != y))
            counters["left_contact"][b] += int(ak0 != NONE and ak > ak0)
            turn = w1 * dt
            pose[b] = (qx, qy, th + turn)
            twist[b] = (v1 if K == S else F(0.0), w1)
            contact[b] = (flags, K)
    return (pose, twist, queue, ticks), contact, counters


def numpy_heading(pose):
    """[B,2] cosine and sine of every heading by numpy (NaN rows for a heading that is not finite)."""
    with np.errstate(all="ignore"):
        th = np.asarray(pose, F)[:, 2]
        return np.stack([np.cos(th), np.sin(th)], axis=1)


# the absolute bound tests/test_math.py (test_sincos) holds sincos_tab to against numpy's sin and cos: 1 ulp of 1
HEADING_ATOL = 2.3e-16


def heading_close(cs, state):
    """Is every (c, s) of a robot whose state (pose and twist) is finite within the bound tests/test_math.py holds sincos_tab
    to? The rows of the other robots are not written and not looked at."""
    pose, twist = np.asarray(state[0], F), np.asarray(state[1], F)
    ok = np.isfinite(pose).all(axis=1) & np.isfinite(twist).all(axis=1)
    return bool((np.abs(np.asarray(cs)[ok] - numpy_heading(pose)[ok]) <= HEADING_ATOL).all())
