"""Sequences for the robot plant (include/smpc_plant.h): hand-made ones with the expected result written out (all in
binary fractions, heading 0 where a position is expected, so every expectation is exact), and seeded ones on a world with
border walls, a block in the middle and a few agents per robot. A sequence is {"p": plant_ref.params(...), "state0": state,
"ticks": [{"cmd", "agents", "count", "want"}]}; the commands are given, the state is fed forward by whoever runs it.
want: None, or {"x", "y", "th", "v", "w", "flags", "K", "tick"}: lists over the robots, None where nothing is expected."""
import numpy as np

import plant_ref as R

INF, NAN = np.inf, np.nan


def no_agents(B, Np=1):
    return np.zeros((B, Np, 5)), np.zeros(B, np.int32)


def state(pose, twist=None):
    pose = np.array(pose, np.float64).reshape(-1, 3)
    B = len(pose)
    _, tw, queue, tick = R.zero_state(B)
    if twist is not None:
        tw = np.array(twist, np.float64).reshape(B, 2)
    return pose, tw, queue, tick


def ticks_of(cmds, agents=None, count=None, wants=None):
    """One tick per entry of cmds ([B,2] each); the same agents every tick unless a list is given."""
    out = []
    for t, cmd in enumerate(cmds):
        cmd = np.array(cmd, np.float64).reshape(-1, 2)
        B = len(cmd)
        a, c = (agents[t], count[t]) if isinstance(agents, list) else (agents, count)
        if a is None:
            a, c = no_agents(B)
        out.append({"cmd": cmd, "agents": np.array(a, np.float64), "count": np.array(c, np.int32),
                    "want": None if wants is None else wants[t]})
    return out


def wall_world(Hx=16, Hy=8, column=10, cost=254):
    w = np.zeros((Hy, Hx), np.uint8)
    w[:, column] = cost
    return w


def hand_sequences():
    H = {}
    # a speed ramp from rest under dv_up, then braking under dv_down; x integrates the executed speed
    p = R.params(S=4, dt=0.25, v_max=1.0, dv_up=0.25, dv_down=0.5, dw=0.5)
    v = [0.25, 0.5, 0.75, 1.0, 1.0, 0.5, 0.0, 0.0]
    x = np.cumsum(np.array(v) * 0.25)
    H["ramp_and_brake"] = dict(p=p, state0=state([0, 0, 0]), ticks=ticks_of(
        [[1.0, 0.0]] * 5 + [[0.0, 0.0]] * 3,
        wants=[dict(x=[x[t]], y=[0.0], th=[0.0], v=[v[t]], w=[0.0], flags=[0], K=[4], tick=[t + 1]) for t in range(8)]))
    # reversals through zero: towards zero the limit is dv_down (and it carries the speed across zero), away from it dv_up;
    # robot 2 turns on the spot: w under dw and w_max, the heading integrates it
    p = R.params(S=2, dt=0.25, v_min=-1.0, v_max=1.0, w_max=1.0, dv_up=0.25, dv_down=0.5, dw=0.5)
    cm = [[[-1, 0], [-1, 0], [0, 2.0]]] * 3 + [[[1, 0], [1, 0], [0, -2.0]]] * 2
    v0, v1 = [0.0, -0.25, -0.5, 0.0, 0.25], [-0.25, -0.5, -0.75, -0.25, 0.25]
    w2 = [0.5, 1.0, 1.0, 0.5, 0.0]
    th2 = np.cumsum(np.array(w2) * 0.25)
    H["reversal"] = dict(p=p, state0=state([[0, 0, 0]] * 3, [[0.5, 0], [0.25, 0], [0, 0]]), ticks=ticks_of(
        cm, wants=[dict(v=[v0[t], v1[t], 0.0], w=[0.0, 0.0, w2[t]], th=[0.0, 0.0, th2[t]], x=[None, None, 0.0], K=[2, 2, 2], flags=[0, 0, 0])
                   for t in range(5)]))
    # latency: the first L ticks execute the zeroed queue's (0, 0)
    for L in (1, 8):
        p = R.params(S=1, L=L, dt=0.25, v_max=1.0)
        n = L + 3
        H[f"latency_{L}"] = dict(p=p, state0=state([0, 0, 0]), ticks=ticks_of(
            [[1.0, 0.0]] * n, wants=[dict(v=[0.0 if t < L else 1.0], w=[0.0], x=[0.25 * max(0, t + 1 - L)], tick=[t + 1], K=[1])
                                     for t in range(n)]))
    # head-on at a wall (column 10, footprint radius 2 cells): the walk ends in cell 7, in front of the first cell with a wall
    # cell within the footprint; v = 0 and flag 1 from then on, the wall is never closer than the footprint; it still turns
    p = R.params(S=4, dt=0.25, v_max=1.0, w_max=1.0, world=wall_world(), res=0.25, footprint_d2=4)
    wants = [dict(x=[1.375], v=[1.0], flags=[0], K=[4]), dict(x=[1.625], v=[1.0], flags=[0], K=[4]), dict(x=[1.875], v=[1.0], flags=[0], K=[4]),
             dict(x=[1.9375], v=[0.0], flags=[1], K=[1]), dict(x=[1.9375], v=[0.0], w=[0.5], th=[0.125], flags=[1], K=[0])]
    wants += [dict(v=[0.0], w=[0.5], flags=[1], th=[0.125 * (t + 2)]) for t in range(5)]
    H["head_on_wall"] = dict(p=p, state0=state([1.125, 1.125, 0]), ticks=ticks_of([[1.0, 0.0]] * 4 + [[1.0, 0.5]] * 6, wants=wants),
                             invariant=lambda st, contact: bool((st[0][:, 0] < 2.0).all() and (contact[:, 0] & 4 == 0).all()))
    # at clearance exactly footprint_d2 (wall row 7, robot in row 5, footprint_d2 4) along the wall: full speed, K = S, flag 4
    world = np.zeros((8, 16), np.uint8)
    world[7, :] = 254
    p = R.params(S=4, dt=0.25, v_max=1.0, world=world, res=0.25, footprint_d2=4)
    H["slide_along_wall"] = dict(p=p, state0=state([0.375, 1.375, 0]), ticks=ticks_of(
        [[1.0, 0.0]] * 6, wants=[dict(x=[0.375 + 0.25 * (t + 1)], y=[1.375], v=[1.0], flags=[4], K=[4]) for t in range(6)]))
    # starts inside a person's contact distance: may not approach, may leave, and may not come back in
    p = R.params(S=4, dt=0.25, v_min=-1.0, v_max=1.0, contact_dist=1.0)
    ag, cnt = np.array([[[0.75, 0, 0, 0, 0]]]), [1]
    H["person_contact"] = dict(p=p, state0=state([0, 0, 0]), ticks=ticks_of(
        [[1.0, 0.0], [-1.0, 0.0], [1.0, 0.0]], ag, cnt,
        wants=[dict(x=[0.0], v=[0.0], flags=[2 | 8], K=[0]), dict(x=[-0.25], v=[-1.0], flags=[8], K=[4]), dict(x=[-0.25], v=[0.0], flags=[2], K=[0])]))
    # a wall and an agent block the same substep
    p = R.params(S=4, dt=0.25, v_max=1.0, world=wall_world(), res=0.25, footprint_d2=4, contact_dist=0.5)
    H["both_blockers"] = dict(p=p, state0=state([1.875, 1.125, 0]), ticks=ticks_of(
        [[1.0, 0.0]], np.array([[[2.46875, 1.125, 0, 0, 0]]]), [1], wants=[dict(x=[1.9375], y=[1.125], v=[0.0], flags=[3], K=[1])]))
    # each not-finite case: the state (pose left bit for bit, twist zeroed, flag 32), and the target command (executed as (0, 0),
    # flag 16) one tick after it was queued
    p = R.params(S=2, L=1, dt=0.25, v_max=1.0, dw=0.25)
    pose0 = [[NAN, 0, 0], [0, INF, 0], [1, 2, -INF], [1, 2, 0.5], [1, 2, 0.5], [3, 0, 0], [3, 0, 0]]
    twist0 = [[0.5, 0.5], [0.5, 0.5], [0.5, 0.5], [NAN, 0.5], [0.5, INF], [1.0, 0.5], [1.0, 0.5]]
    cm = [[1, 0]] * 5 + [[NAN, 0.0], [0.0, -INF]]
    H["not_finite"] = dict(p=p, state0=state(pose0, twist0), ticks=ticks_of(
        [cm, cm], wants=[dict(v=[0.0] * 7, w=[0.0] * 5 + [0.25, 0.25], flags=[32] * 5 + [0, 0], K=[0] * 5 + [2, 2], tick=[1] * 7, x=[None] * 5 + [3.0, 3.0]),
                         dict(v=[0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0], w=[0.0] * 7, flags=[32, 32, 32, 0, 0, 16, 16], K=[0, 0, 0, 2, 2, 2, 2], tick=[2] * 7)]),
                           keeps_pose=[0, 1, 2])
    # footprint_d2 -1 (no walls: straight through), 0 (only the wall cell itself stops: up to its edge), 225 (15 cells)
    for fd2, col, Hx, x_end, K_end, flags_end in ((-1, 10, 16, 2.625, 4, 0), (0, 10, 16, 2.4375, 1, 1), (225, 40, 64, 6.1875, 3, 1)):
        x0 = 2.375 if fd2 <= 0 else 6.0
        p = R.params(S=4, dt=0.25, v_max=1.0, world=wall_world(Hx=Hx, column=col), res=0.25, footprint_d2=fd2)
        H[f"footprint_{fd2}"] = dict(p=p, state0=state([x0, 1.125, 0]), ticks=ticks_of(
            [[1.0, 0.0]], wants=[dict(x=[x_end], K=[K_end], flags=[flags_end])]))
    # the map's edge and beyond it, outside_is_wall both ways: robot 0 drives out over the edge at x = 4, robot 1 is outside
    for outside in (False, True):
        p = R.params(S=4, dt=0.25, v_max=1.0, world=np.zeros((8, 16), np.uint8), res=0.25, footprint_d2=1, outside_is_wall=outside)
        want = dict(x=[3.6875, 6.25], K=[1, 4], flags=[1, 4], v=[0.0, 1.0]) if outside else dict(x=[3.875, 6.25], K=[4, 4], flags=[0, 0])
        H[f"map_edge_outside_{int(outside)}"] = dict(p=p, state0=state([[3.625, 1.125, 0], [6.0, 1.125, 0]]),
                                                     ticks=ticks_of([[[1.0, 0.0], [1.0, 0.0]]], wants=[want]))
    # a cost of 255, unknown_is_wall both ways
    for unknown in (False, True):
        p = R.params(S=4, dt=0.25, v_max=1.0, world=wall_world(cost=255), res=0.25, footprint_d2=0, unknown_is_wall=unknown, wall_min_cost=1)
        want = dict(x=[2.4375], K=[1], flags=[1]) if unknown else dict(x=[2.625], K=[4], flags=[0])
        H[f"unknown_{int(unknown)}"] = dict(p=p, state0=state([2.375, 1.125, 0]), ticks=ticks_of([[1.0, 0.0]], wants=[want]))
    # contact_dist 0: nothing is ever in contact, not even an agent on the robot's own spot
    p = R.params(S=4, dt=0.25, v_max=1.0, contact_dist=0.0)
    H["contact_dist_0"] = dict(p=p, state0=state([0, 0, 0]), ticks=ticks_of(
        [[1.0, 0.0]], np.array([[[0.0, 0.0, 0, 0, 0], [0.125, 0.0, 0, 0, 0]]]), [2], wants=[dict(x=[0.25], K=[4], flags=[0])]))
    # a count above Np reads Np rows (the second one blocks), a negative one none
    p = R.params(S=4, dt=0.25, v_max=1.0, contact_dist=0.5)
    ag = np.array([[[9.0, 9.0, 0, 0, 0], [0.5625, 0.0, 0, 0, 0]]] * 2)
    H["count_clamp"] = dict(p=p, state0=state([[0, 0, 0], [0, 0, 0]]), ticks=ticks_of(
        [[[1.0, 0.0], [1.0, 0.0]]], ag, [5, -3], wants=[dict(x=[0.0625, 0.25], K=[1, 4], flags=[2, 0])]))
    return H


def seeded_world(rng, Hx=64, Hy=48):
    world = np.zeros((Hy, Hx), np.uint8)
    world[rng.random((Hy, Hx)) < 0.02] = 100                 # below every wall_min_cost used
    world[0, :] = world[-1, :] = 254
    world[:, 0] = world[:, -1] = 254
    world[Hy // 2 - 4:Hy // 2 + 4, Hx // 2 - 4:Hx // 2 + 4] = 253
    world[Hy // 2 - 10, Hx // 2 - 12:Hx // 2 - 6] = 255      # a stretch of unknown cells
    return world


def seeded_sequence(seed, B=64, n_ticks=40, Np=4, S=4, L=0, footprint_d2=6, unknown_is_wall=True, outside_is_wall=True, n_agents=4):
    rng = np.random.default_rng(seed)
    res, origin = 0.1, (-1.0, -0.5)
    world = seeded_world(rng)
    Hy, Hx = world.shape
    p = R.params(S=S, L=L, dt=0.1, v_min=0.0, v_max=0.6, w_max=1.4, dv_up=0.05, dv_down=0.1, dw=0.3, contact_dist=0.54, world=world,
                 origin=origin, res=res, footprint_d2=footprint_d2, wall_min_cost=253, unknown_is_wall=unknown_is_wall,
                 outside_is_wall=outside_is_wall)
    pose = np.stack([origin[0] + rng.uniform(0.5, Hx * res - 0.5, B), origin[1] + rng.uniform(0.5, Hy * res - 0.5, B),
                     rng.uniform(-np.pi, np.pi, B)], axis=1)
    twist = np.stack([rng.uniform(0.0, 0.6, B), rng.uniform(-1.0, 1.0, B)], axis=1)
    cmds = np.stack([rng.uniform(-0.1, 0.8, (n_ticks, B)), rng.uniform(-1.6, 1.6, (n_ticks, B))], axis=2)
    steady = rng.random(B) < 0.5                             # half the robots hold a course: they reach the walls
    cmds[:, steady, 0] = 0.6
    cmds[:, steady, 1] *= 0.1
    if B >= 8:                                               # along the lower border at the footprint's reach, heading 0, full speed
        r = int(np.floor(np.sqrt(max(footprint_d2, 0))))
        for b in range(2):
            pose[b] = (origin[0] + 0.6 + 0.3 * b, origin[1] + (1 + r + 0.5) * res, 0.0)
            twist[b] = (0.6, 0.0)
            cmds[:, b] = (0.6, 0.0)
        pose[B - 1, 0] = NAN                                 # a robot whose state is not finite stays where it is
        twist[B - 2, 1] = INF                                # ... one whose twist is not: reset to rest, then it drives
        pose[B - 3, :2] = (origin[0] - 0.35, origin[1] + 1.0)  # one that starts outside the map
    bad = rng.random((n_ticks, B)) < 0.01
    cmds[bad, rng.integers(0, 2, int(bad.sum()))] = rng.choice([NAN, INF, -INF], int(bad.sum()))
    agents = np.zeros((n_ticks, B, Np, 5))
    a0 = pose[:, None, :2] + rng.uniform(-1.2, 1.2, (B, Np, 2))
    a0[~np.isfinite(a0)] = 0.0
    av = rng.uniform(-0.5, 0.5, (B, Np, 2))
    for t in range(n_ticks):
        agents[t, :, :, :2] = a0 + av * (0.1 * t)
        agents[t, :, :, 2:4] = av
    agents[rng.random((n_ticks, B, Np)) < 0.005, 0] = NAN    # a row that is not finite is not an agent
    count = np.full((n_ticks, B), min(n_agents, Np), np.int32)
    count[rng.random((n_ticks, B)) < 0.05] = Np + 3
    count[rng.random((n_ticks, B)) < 0.05] = -1
    st = (pose, twist, np.zeros((B, 8, 2)), rng.integers(0, 2 ** 32, B, dtype=np.uint32) if L else np.zeros(B, np.uint32))
    if L:
        st[3][0] = np.uint32(2 ** 32 - 2)                    # the counter wraps inside the sequence
    return dict(p=p, state0=st, ticks=[{"cmd": cmds[t], "agents": agents[t], "count": count[t], "want": None} for t in range(n_ticks)])


def seeded_sequences():
    """The issue's 64 robots x 40 ticks, and the shapes the GPU test asks for (B 1 / 5 / 257, Np 1 / 8 / 64, S 1 / 4 / 16,
    L 0 / 1 / 8, footprint_d2 0 / 36 / 225), short."""
    return {
        "B64_Np4_S4_L0_fd6": seeded_sequence(11),
        "B1_Np1_S1_L0_fd0": seeded_sequence(12, B=1, n_ticks=12, Np=1, S=1, L=0, footprint_d2=0, n_agents=1),
        "B5_Np64_S16_L8_fd225": seeded_sequence(13, B=5, n_ticks=12, Np=64, S=16, L=8, footprint_d2=225, n_agents=64, unknown_is_wall=False),
        "B257_Np8_S4_L1_fd36": seeded_sequence(14, B=257, n_ticks=5, Np=8, S=4, L=1, footprint_d2=36, n_agents=8, outside_is_wall=False),
    }


# ---- running a sequence ---------------------------------------------------------------------------------------------------
def ref_call(st, tick, p, cs=None):
    """The yardstick as a `call`: (new state, contact, cs); cs None: numpy's cosine and sine of the headings."""
    cs = R.numpy_heading(st[0]) if cs is None else cs
    new, contact, _ = R.step(st, tick, p, cs)
    return new, contact, cs


def run(seq, call):
    """(t, tick, state before, new state, contact, cs) for every tick, the state fed forward from `call`'s own output."""
    st = tuple(np.array(a) for a in seq["state0"])
    for t, tick in enumerate(seq["ticks"]):
        new, contact, cs = call(st, tick, seq["p"])
        yield t, tick, st, new, contact, cs
        st = new


def same(got, want):
    """(state, contact) pairs, bit for bit."""
    return all(np.asarray(g).dtype == np.asarray(w).dtype and np.asarray(g).tobytes() == np.asarray(w).tobytes()
               for g, w in zip(list(got[0]) + [got[1]], list(want[0]) + [want[1]]))


def check_want(seq, before, new, contact, want):
    pose, twist, queue, tick = new
    cols = {"x": pose[:, 0], "y": pose[:, 1], "th": pose[:, 2], "v": twist[:, 0], "w": twist[:, 1], "flags": contact[:, 0], "K": contact[:, 1],
            "tick": tick}
    for k, vals in (want or {}).items():
        for b, v in enumerate(vals):
            assert v is None or cols[k][b] == v, (k, b, cols[k][b], v)
    for b in seq.get("keeps_pose", ()):
        assert pose[b].tobytes() == before[0][b].tobytes(), b
    if "invariant" in seq:
        assert seq["invariant"](new, contact)
