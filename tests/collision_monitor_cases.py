"""Cases of the collision monitor for tests/test_collision_monitor.py and tests/test_gpu_collision_monitor.py: hand-made ones
with the expected result written out, and seeded ones. A case is {"p": collision_monitor_ref.params(...), "pose" [B,3],
"cmd" [B,2], "kind" [B,n] uint8, "cell" [B,n,2] int32}; a hand-made one adds "want": per robot a dict of the outputs it
pins down (cmd_out, ratio, flags, zone, step, points, zone_points).

The hand-made cases use exactly representable numbers: cells of 0.125 m at the origin (0, 0), the robot on the centre of cell
(40, 40) with heading 0, so that the point of offset (i, j) is (0.125 i, 0.125 j) in the robot's frame without rounding."""
import numpy as np

import collision_monitor_ref as R

RES = 0.125
HOME = (40.5 * RES, 40.5 * RES, 0.0)     # the centre of cell (40, 40), heading 0
SQUARE = [(-0.25, -0.25), (0.25, -0.25), (0.25, 0.25), (-0.25, 0.25)]   # a footprint


def case(p, robots):
    """robots: [(pose, cmd, [(kind, (i, j)), ..], want)]; the beams of a robot with fewer than the most are NONE."""
    n = max(1, max(len(r[2]) for r in robots))
    B = len(robots)
    kind, cell = np.zeros((B, n), np.uint8), np.zeros((B, n, 2), np.int32)
    for b, (_, _, beams, _) in enumerate(robots):
        for k, (kd, off) in enumerate(beams):
            kind[b, k], cell[b, k] = kd, off
    return dict(p=p, pose=np.array([r[0] for r in robots], np.float64), cmd=np.array([r[1] for r in robots], np.float64), kind=kind, cell=cell,
                want=[r[3] for r in robots])


def hits(*offsets):
    return [(R.KIND_WORLD, o) for o in offsets]


def hand_cases():
    out = {}
    W, A, CP = R.KIND_WORLD, R.KIND_AGENT, R.KIND_CORNER_PAIR
    nothing = lambda cmd, points, zp: dict(cmd_out=cmd, ratio=1.0, flags=0, zone=-1, step=-1, points=points, zone_points=zp)

    # three points in a STOP circle of four give nothing, a fourth stops; the circle is open: a point at the radius is outside
    stop = R.params([R.circle(R.STOP, 0.5, min_points=4)])
    out["stop_needs_min_points"] = case(stop, [
        (HOME, (0.5, 0.25), hits((1, 0), (2, 0), (0, 1)), nothing((0.5, 0.25), 3, [3])),
        (HOME, (0.5, 0.25), hits((1, 0), (2, 0), (0, 1), (0, -2)), dict(cmd_out=(0.0, 0.0), ratio=0.0, flags=1, zone=0, step=0, points=4, zone_points=[4])),
        (HOME, (0.5, 0.25), hits((1, 0), (2, 0), (0, 1), (4, 0)), nothing((0.5, 0.25), 4, [3])),
        (HOME, (0.5, 0.25), hits((1, 0), (2, 0), (0, 1), (0, -3), (3, 3), (8, 8)), dict(cmd_out=(0.0, 0.0), ratio=0.0, zone_points=[4], points=6)),
    ])

    # a polygon owns its left and lower edges and not its right and upper ones (the crossing rule x < x of the edge)
    box = R.params([R.polygon(R.STOP, [(0.0, 0.0), (0.5, 0.0), (0.5, 0.5), (0.0, 0.5)])])
    inside = lambda off, yes: (HOME, (0.25, 0.0), hits(off), dict(zone_points=[int(yes)], ratio=0.0 if yes else 1.0, zone=0 if yes else -1))
    out["polygon_edges_and_vertices"] = case(box, [
        inside((2, 2), True),                                       # interior
        inside((0, 2), True), inside((2, 0), True),                 # left edge, lower edge
        inside((4, 2), False), inside((2, 4), False),               # right edge, upper edge
        inside((0, 0), True),                                       # the lower left vertex
        inside((4, 0), False), inside((0, 4), False), inside((4, 4), False),
        inside((-1, 2), False), inside((5, 2), False), inside((2, -1), False), inside((2, 5), False),
    ])
    # the same box given clockwise
    box_cw = R.params([R.polygon(R.STOP, [(0.0, 0.5), (0.5, 0.5), (0.5, 0.0), (0.0, 0.0)])])
    out["polygon_clockwise"] = case(box_cw, [inside((2, 2), True), inside((0, 2), True), inside((2, 0), True), inside((4, 2), False),
                                             inside((2, 4), False), inside((0, 0), True), inside((4, 4), False)])

    # a triangle (its slanted edge from (1, 0) to (0, 0.5) is x = 1 - 2 y) and a regular 16-gon of radius 1
    tri = R.params([R.polygon(R.STOP, [(0.0, -0.5), (1.0, 0.0), (0.0, 0.5)])])
    out["triangle"] = case(tri, [inside((2, 0), True), inside((4, 1), True), inside((6, 1), False), inside((7, 1), False), inside((0, 0), True),
                                 inside((4, 2), False), inside((-1, 0), False), inside((4, -1), True), inside((6, -1), False)])
    gon = R.params([R.polygon(R.STOP, [(np.cos(i * np.pi / 8), np.sin(i * np.pi / 8)) for i in range(16)])])
    out["sixteen_gon"] = case(gon, [inside((4, 4), True), inside((6, 6), False), inside((7, 3), True), inside((7, 4), False), inside((-7, -3), True),
                                    inside((0, 0), True), inside((-4, 7), False), inside((0, -7), True), inside((3, -8), False)])

    # SLOWDOWN 0.5, LIMIT 0.25 / 0.5 and APPROACH together, v = 0.5, steps of 0.0625 m, M = 8: a point 0.5 ahead enters the
    # approach circle of 0.3125 at step 4 (0.5 - 0.0625 m < 0.3125), all three yield 0.5 and the lowest index decides; a
    # point 0.375 ahead enters it at step 2, 0.25 decides
    trio = R.params([R.circle(R.SLOWDOWN, 1.0, slowdown_ratio=0.5), R.circle(R.LIMIT, 1.0, linear_limit=0.25, angular_limit=8.0),
                     R.circle(R.APPROACH, 0.3125)], M=8, sim_dt=0.125)
    out["least_ratio_decides"] = case(trio, [
        (HOME, (0.5, 0.0), hits((4, 0)), dict(cmd_out=(0.25, 0.0), ratio=0.5, flags=2, zone=0, step=0, points=1, zone_points=[1, 1, 0])),
        (HOME, (0.5, 0.0), hits((3, 0)), dict(cmd_out=(0.125, 0.0), ratio=0.25, flags=8, zone=2, step=2, points=1, zone_points=[1, 1, 0])),
        (HOME, (0.5, 0.0), hits((2, 0)), dict(cmd_out=(0.0, 0.0), ratio=0.0, flags=8, zone=2, step=0, points=1, zone_points=[1, 1, 1])),
        (HOME, (0.5, 0.0), hits((9, 0)), nothing((0.5, 0.0), 1, [0, 0, 0])),
    ])
    # a LIMIT with only w over its limit
    lim = R.params([R.circle(R.LIMIT, 1.0, linear_limit=0.5, angular_limit=0.5)])
    out["limit_angular_only"] = case(lim, [
        (HOME, (0.25, 1.0), hits((2, 2)), dict(cmd_out=(0.125, 0.5), ratio=0.5, flags=4, zone=0, step=0)),
        (HOME, (0.25, -0.5), hits((2, 2)), nothing((0.25, -0.5), 1, [1])),
        (HOME, (-2.0, 1.0), hits((2, 2)), dict(cmd_out=(-0.5, 0.25), ratio=0.25, flags=4, zone=0)),
    ])

    # a wall 0.625 m straight ahead, the footprint square as APPROACH zone, v = 0.5, sim_dt = 0.125, M = 8: the wall's points
    # enter the square at 0.625 - 0.0625 m < 0.25 (the right edge is not the square's), m = 7: 7 / 8 of the command.
    wall = hits(*[(5, j) for j in range(-4, 5)])
    ahead = R.params([R.polygon(R.APPROACH, SQUARE)], M=8, sim_dt=0.125)
    out["wall_ahead"] = case(ahead, [
        (HOME, (0.5, 0.0), wall, dict(cmd_out=(0.4375, 0.0), ratio=0.875, flags=8, zone=0, step=7, points=9, zone_points=[0])),
        # the same wall and a w that turns the robot clear of it: on an arc of radius 0.125 no corner of the square reaches 0.625
        (HOME, (0.5, 4.0), wall, nothing((0.5, 4.0), 9, [0])),
        # half the speed: 0.625 - 0.03125 m < 0.25 only from m = 13 on
        (HOME, (0.25, 0.0), wall, nothing((0.25, 0.0), 9, [0])),
    ])
    # v < 0 and the wall behind: -0.625 + 0.0625 m >= -0.25 (the left edge is the square's), m = 6
    behind = hits(*[(-5, j) for j in range(-4, 5)])
    out["wall_behind"] = case(ahead, [
        (HOME, (-0.5, 0.0), behind, dict(cmd_out=(-0.375, 0.0), ratio=0.75, flags=8, zone=0, step=6, points=9, zone_points=[0])),
        (HOME, (0.5, 0.0), behind, nothing((0.5, 0.0), 9, [0])),
    ])
    # v = 0, turning in place at 1 rad/s in steps of 0.125 rad: an arm ahead of the robot, 0.125 wide, sweeps onto a point
    # 0.5 m to its left when the angle left, pi / 2 - 0.125 m, is below asin(0.125) = 0.1253: m = 12 of 16
    arm = R.params([R.polygon(R.APPROACH, [(0.0, -0.0625), (0.75, -0.0625), (0.75, 0.0625), (0.0, 0.0625)])], M=16, sim_dt=0.125)
    out["turning_in_place"] = case(arm, [
        (HOME, (0.0, 1.0), hits((0, 4)), dict(cmd_out=(0.0, 0.75), ratio=0.75, flags=8, zone=0, step=12, points=1, zone_points=[0])),
        (HOME, (0.0, -1.0), hits((0, 4)), nothing((0.0, -1.0), 1, [0])),
        (HOME, (-0.0, -1.0), hits((0, -4)), dict(cmd_out=(-0.0, -0.75), ratio=0.75, step=12)),
    ])

    # a ratio of 1 hands cmd through bit for bit; what is not finite; a robot without a cell
    nan, inf = np.nan, np.inf
    bad = dict(cmd_out=(0.0, 0.0), ratio=0.0, flags=16, zone=-1, step=-1, points=0, zone_points=[0])
    out["pass_through_and_bad_input"] = case(stop, [
        (HOME, (-0.0, 0.25), hits((1, 0)), nothing((-0.0, 0.25), 1, [1])),
        (HOME, (0.5, -0.0), [], nothing((0.5, -0.0), 0, [0])),
        ((nan, HOME[1], 0.0), (0.5, 0.0), hits((1, 0)), bad), ((HOME[0], inf, 0.0), (0.5, 0.0), hits((1, 0)), bad),
        ((HOME[0], HOME[1], -inf), (0.5, 0.0), hits((1, 0)), bad), (HOME, (nan, 0.0), hits((1, 0)), bad), (HOME, (0.5, inf), hits((1, 0)), bad),
        ((2.0 ** 40, HOME[1], 0.0), (0.5, 0.25), hits((1, 0), (2, 0), (0, 1), (0, -2)), dict(cmd_out=(0.5, 0.25), ratio=1.0, flags=32, zone=-1, step=-1, points=0, zone_points=[0])),
    ])
    # only WORLD, AGENT and CORNER_PAIR give a point, a pair one; a cell recorded twice is two points
    four = [(1, 0), (2, 0), (0, 1), (0, -2)]
    out["kinds_and_duplicates"] = case(stop, [
        (HOME, (0.5, 0.0), [(R.KIND_NONE, o) for o in four] + [(R.KIND_INVALID, o) for o in four] + [(R.KIND_NO_ROBOT, o) for o in four] + [(6, o) for o in four]
         + [(255, o) for o in four], nothing((0.5, 0.0), 0, [0])),
        (HOME, (0.5, 0.0), [(W, four[0]), (A, four[1]), (CP, four[2])], nothing((0.5, 0.0), 3, [3])),
        (HOME, (0.5, 0.0), [(W, four[0]), (A, four[1]), (CP, four[2]), (CP, four[3])], dict(cmd_out=(0.0, 0.0), ratio=0.0, points=4, zone_points=[4])),
        (HOME, (0.5, 0.0), [(W, four[0]), (W, four[0]), (A, four[0]), (CP, four[0])], dict(cmd_out=(0.0, 0.0), ratio=0.0, points=4, zone_points=[4])),
        (HOME, (0.5, 0.0), [(W, four[0]), (W, four[0]), (A, four[0]), (R.KIND_NONE, four[0])], nothing((0.5, 0.0), 3, [3])),
    ])
    return out


def check_want(c, got):
    """The outputs `got` (collision_monitor_ref.run's keys) against what a hand-made case pins down."""
    for b, want in enumerate(c["want"]):
        for k, v in want.items():
            if k == "cmd_out":
                assert np.array(v, np.float64).tobytes() == np.ascontiguousarray(got["cmd_out"][b]).tobytes(), (b, k, got["cmd_out"][b], v)
            elif k == "ratio":
                assert got["ratio"][b] == v, (b, k, got["ratio"][b], v)
            elif k == "zone_points":
                assert list(got["zone_points"][b]) == list(v), (b, k, got["zone_points"][b], v)
            else:
                col = {"flags": 0, "zone": 1, "step": 2, "points": 3}[k]
                assert got["action"][b, col] == v, (b, k, got["action"][b], v)


# ---- seeded cases ------------------------------------------------------------------------------------------------------------
def regular(n, radius, phase=0.0, centre=(0.0, 0.0)):
    return [(centre[0] + radius * np.cos(phase + 2 * np.pi * i / n), centre[1] + radius * np.sin(phase + 2 * np.pi * i / n)) for i in range(n)]


def zone_set(Z, min_points):
    """Z zones over every action and the three shapes (a circle, a 3-gon, a 16-gon); min_points: one value or one per zone."""
    mp = (lambda i: min_points[i % len(min_points)]) if isinstance(min_points, (list, tuple)) else (lambda i: min_points)
    all8 = [R.circle(R.STOP, 0.27, mp(0)),
            R.polygon(R.APPROACH, regular(16, 0.3, 0.1), mp(1)),
            R.polygon(R.SLOWDOWN, [(-0.3, -0.45), (1.1, 0.0), (-0.3, 0.45)], mp(2), slowdown_ratio=0.625),
            R.circle(R.LIMIT, 0.9, mp(3), linear_limit=0.3, angular_limit=0.7),
            R.polygon(R.APPROACH, [(0.5, 0.0), (-0.25, 0.3), (-0.25, -0.3)], mp(4)),
            R.polygon(R.LIMIT, regular(16, 0.6, 0.0, (0.3, 0.0))[::-1], mp(5), linear_limit=0.55, angular_limit=0.2),
            R.circle(R.APPROACH, 0.2, mp(6)),
            R.polygon(R.SLOWDOWN, regular(5, 0.5, 0.3), mp(7), slowdown_ratio=0.0)]
    return all8[:Z]


def seeded_case(seed, B, n_beams, Z, M, min_points=1, hit_share=0.25, zones=None, sim_dt=0.1):
    """B robots somewhere on a floor of 0.05 m cells, each with walls of hits laid across its path at a distance drawn so that
    the approach zones meet them at every step of the horizon, scattered hits, beams of every other kind, and, in the batches
    large enough, a robot of each odd sort (not finite, without a cell, at rest, backing up)."""
    rng = np.random.default_rng(seed)
    res, origin = 0.05, (-3.2, -2.4)
    p = R.params(zones if zones is not None else zone_set(Z, min_points), M=M, sim_dt=sim_dt, res=res, origin=origin)
    pose = np.stack([rng.uniform(-2.0, 6.0, B), rng.uniform(-2.0, 4.0, B), rng.uniform(-np.pi, np.pi, B)], axis=1)
    cmd = np.stack([rng.uniform(0.1, 0.8, B), np.where(rng.random(B) < 0.5, 0.0, rng.uniform(-1.5, 1.5, B))], axis=1)
    kind = rng.choice(np.array([0, 0, 0, 4, 5, 6, 200], np.uint8), size=(B, n_beams))
    cell = rng.integers(-60, 61, size=(B, n_beams, 2)).astype(np.int32)
    horizon = max(M, 1) * sim_dt
    for b in range(B):
        th = pose[b, 2]
        n_hits = max(1, int(round(hit_share * n_beams))) if n_beams > 1 else int(rng.random() < 0.7)
        ks = rng.permutation(n_beams)[:n_hits]
        # a wall across the path at a distance within reach of the horizon, the rest scattered around the robot
        d = 0.2 + rng.uniform(0.0, 1.1) * (0.3 + cmd[b, 0] * horizon)
        n_wall = (2 * n_hits) // 3
        along = rng.uniform(-0.6, 0.6, n_hits)
        lx = np.where(np.arange(n_hits) < n_wall, d, rng.uniform(-1.5, 1.5, n_hits))
        ly = np.where(np.arange(n_hits) < n_wall, along, rng.uniform(-1.5, 1.5, n_hits))
        if b % 4 == 3:  # a robot in the open: everything it sees lies beyond every zone and every horizon
            far, bearing = rng.uniform(2.2, 3.0, n_hits), rng.uniform(-np.pi, np.pi, n_hits)
            lx, ly = far * np.cos(bearing), far * np.sin(bearing)
        wx, wy = np.cos(th) * lx - np.sin(th) * ly, np.sin(th) * lx + np.cos(th) * ly
        cell[b, ks, 0] = np.round(wx / res).astype(np.int32)
        cell[b, ks, 1] = np.round(wy / res).astype(np.int32)
        kind[b, ks] = rng.choice(np.array([1, 1, 2, 3], np.uint8), size=n_hits)
    if B >= 64:
        # robots 16 .. 16 + M on cell centres with heading 0 drive at 0.8 m/s straight at a wall k cells ahead, 0.08 m per step:
        # the 16-gon of zone_set (0.2956 m ahead of the robot along the rows of cells next to its axis) meets it at step m
        for m in range(M + 1):
            b = 16 + m
            pose[b] = (origin[0] + (40 + b + 0.5) * res, origin[1] + 50.5 * res, 0.0)
            cmd[b] = (0.8, 0.0)
            k = int(np.ceil((0.2956 + 0.08 * (m - 1)) / res)) if m > 0 else 5
            kind[b], cell[b] = 0, 0
            kind[b, :13] = 1
            cell[b, :13, 0], cell[b, :13, 1] = k, np.arange(-6, 7)
    if B >= 16:
        pose[1, 0], pose[2, 2], cmd[3, 0], cmd[4, 1] = np.nan, np.inf, -np.inf, np.nan
        pose[5, 0] = 1e9                       # no cell
        cmd[6] = (0.0, 1.2)                    # turning in place
        cmd[7] = (-0.4, 0.3)                   # backing up
        cmd[8] = (-0.0, 0.0)                   # at rest
        kind[9] = 0                            # sees nothing
        cell[10, :, :] = cell[10, :1, :]       # every beam at one cell
    return dict(p=p, pose=pose, cmd=cmd, kind=kind, cell=cell)


MAIN = "B64_n360_Z8_M12"


def seeded_cases():
    """name -> case: n_beams straddle the lane count (63, 64, 65) and the points a wavefront keeps in registers (512, 513),
    one zone and eight, the three shapes, M of 0, 1, 12 and 32, min_points of 1, 4 and more than n_beams."""
    one = lambda z: [z]
    return {
        MAIN: seeded_case(1, 64, 360, 8, 12, [4, 1, 2, 3, 4, 1, 2, 5]),
        "B16_n1_Z1_M0_circle": seeded_case(2, 16, 1, 1, 0, zones=one(R.circle(R.STOP, 1.2, 1))),
        "B16_n1_Z8_M1": seeded_case(3, 16, 1, 8, 1, 1),
        "B16_n63_Z1_M1_3gon": seeded_case(4, 16, 63, 1, 1, zones=one(R.polygon(R.APPROACH, [(0.5, 0.0), (-0.25, 0.3), (-0.25, -0.3)], 4)), hit_share=0.5),
        "B16_n64_Z8_M32": seeded_case(5, 16, 64, 8, 32, [1, 4], hit_share=0.5, sim_dt=0.05),
        "B16_n65_Z1_M12_16gon": seeded_case(6, 16, 65, 1, 12, zones=one(R.polygon(R.APPROACH, regular(16, 0.3, 0.1), 4)), hit_share=0.5),
        "B16_n360_Z8_M0": seeded_case(7, 16, 360, 8, 0, zones=[z for z in zone_set(8, [1, 4]) if z["action"] != R.APPROACH]
                                      + [R.polygon(R.LIMIT, [(0.8, 0.0), (-0.2, 0.5), (-0.2, -0.5)], 2, linear_limit=0.1, angular_limit=0.0),
                                         R.circle(R.SLOWDOWN, 0.7, 3, slowdown_ratio=1.0), R.circle(R.STOP, 0.4, 361)]),
        "B16_n360_Z1_M12_never": seeded_case(8, 16, 360, 1, 12, zones=one(R.polygon(R.APPROACH, regular(16, 0.3, 0.1), 361)), hit_share=0.1),
        "B8_n512_Z1_M12_circle": seeded_case(9, 8, 512, 1, 12, zones=one(R.circle(R.APPROACH, 0.3, 4)), hit_share=0.2),
        "B8_n513_Z8_M12": seeded_case(10, 8, 513, 8, 12, [4, 1], hit_share=0.15),
        "B4_n4096_Z8_M32": seeded_case(11, 4, 4096, 8, 32, [4, 1, 4097], hit_share=0.03, sim_dt=0.05),
        "B4_n4096_Z1_M1_circle": seeded_case(12, 4, 4096, 1, 1, zones=one(R.circle(R.APPROACH, 0.4, 1)), hit_share=0.03),
    }
