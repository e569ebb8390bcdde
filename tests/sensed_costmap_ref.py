"""The contract of smpc_sensed_costmap_batch (include/smpc_sensed_costmap.h) as plain Python integers and numpy: per robot
the cells, every beam as the sequential walk of the contract's text, the marks, and the inflation as a brute-force search
over the marks. The one yardstick of tests/test_sensed_costmap.py, tests/test_gpu_sensed_costmap.py and
tests/test_gpu_episode_sensed.py; written from the contract, not from csrc/smpc_sensed_costmap_rule.hpp (which takes a
beam column by column in closed form and a row's gaps from bit masks, and is checked against this)."""
import math

import numpy as np

NONE, WORLD, AGENT, CORNER_PAIR, INVALID, NO_ROBOT = range(6)
MAX_REACH = 127
MAX_CELL = float(2 ** 30)


def cell_axis(p, origin, res):
    """floor((p - origin) / res) as a double, every operation rounded on its own (numpy float64 does just that)."""
    with np.errstate(all="ignore"):
        return float(np.floor((np.float64(p) - np.float64(origin)) / np.float64(res)))


def point_cell(x, y, origin, res):
    """The cell of a robot or an agent, or None: x or y not finite, or |q| <= 2^30 fails on an axis."""
    x, y = float(x), float(y)
    qx, qy = cell_axis(x, origin[0], res), cell_axis(y, origin[1], res)
    if not (math.isfinite(x) and math.isfinite(y)) or not (abs(qx) <= MAX_CELL and abs(qy) <= MAX_CELL):
        return None
    return int(qx), int(qy)


def occupied_cells(people, count, origin, res, agent_d2):
    """The set of world cells the agents of one robot occupy."""
    Np = people.shape[0]
    ra = math.isqrt(agent_d2)
    cells = set()
    for j in range(min(max(int(count), 0), Np)):
        q = point_cell(people[j, 0], people[j, 1], origin, res)
        if q is None:
            continue
        for i in range(-ra, ra + 1):
            for k in range(-ra, ra + 1):
                if i * i + k * k <= agent_d2:
                    cells.add((q[0] + i, q[1] + k))
    return cells


def stops(world, occupied, a, c, min_cost=254, unknown=False):
    """What cell c does to a beam of the robot in cell a: 0, WORLD or AGENT."""
    if c == a:
        return 0
    Hy, Hx = world.shape
    if 0 <= c[0] < Hx and 0 <= c[1] < Hy:
        cost = int(world[c[1], c[0]])
        if cost >= min_cost and (cost != 255 or bool(unknown)):
            return WORLD
    return AGENT if c in occupied else 0


def cast(world, occupied, a, off, min_cost=254, unknown=False):
    """One beam from cell a to a + off: (kind, the offset beam_cell reports, the hit cells as offsets)."""
    ex, ey = int(off[0]), int(off[1])
    if abs(ex) > MAX_REACH or abs(ey) > MAX_REACH:
        return INVALID, (ex, ey), []
    dx, dy = abs(ex), abs(ey)
    sx, sy = (1 if ex > 0 else -1), (1 if ey > 0 else -1)
    at = lambda i, j: (sx * i, sy * j)
    test = lambda o: stops(world, occupied, a, (a[0] + o[0], a[1] + o[1]), min_cost, unknown)
    i = j = 0
    while (i, j) != (dx, dy):
        A, Bv = (2 * i + 1) * dy, (2 * j + 1) * dx
        if A < Bv:
            i += 1
        elif A > Bv:
            j += 1
        else:  # a lattice corner: the two cells that touch the segment only there stop the beam as a pair, or not at all
            along_x, along_y = at(i + 1, j), at(i, j + 1)
            if test(along_x) and test(along_y):
                return CORNER_PAIR, along_x, [along_x, along_y]
            i, j = i + 1, j + 1
        kind = test(at(i, j))
        if kind:
            return kind, at(i, j), [at(i, j)]
    return NONE, (ex, ey), []


def inflate(marks, size_x, size_y, table):
    """[size_y,size_x] uint8: table[least d2 to a mark] where that is within the table, else 0. Brute force: every mark
    against every cell that the table can reach from it (a cell farther than isqrt(d2_max) along an axis has d2 > d2_max)."""
    table = np.asarray(table, np.uint8)
    far = np.int64(table.size)                                               # d2_max + 1: beyond the table
    d2 = np.full((size_y, size_x), far, np.int64)
    R = math.isqrt(table.size - 1)
    for mx, my in marks:
        x0, x1, y0, y1 = max(mx - R, 0), min(mx + R, size_x - 1), max(my - R, 0), min(my + R, size_y - 1)
        dx2 = (np.arange(x0, x1 + 1, dtype=np.int64) - mx) ** 2
        dy2 = (np.arange(y0, y1 + 1, dtype=np.int64) - my) ** 2
        np.minimum(d2[y0:y1 + 1, x0:x1 + 1], dy2[:, None] + dx2[None, :], out=d2[y0:y1 + 1, x0:x1 + 1])
    return np.where(d2 < far, table[np.minimum(d2, far - 1)], 0).astype(np.uint8)


def world_cut(world, cell, size_x, size_y, outside_cost):
    """What smpc_local_costmap_batch puts into the window whose cell (0,0) is world cell `cell`."""
    Hy, Hx = world.shape
    out = np.full((size_y, size_x), outside_cost, np.uint8)
    cx, cy = int(cell[0]), int(cell[1])
    x0, x1, y0, y1 = max(0, -cx), min(size_x, Hx - cx), max(0, -cy), min(size_y, Hy - cy)   # the window cells inside the world
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = world[cy + y0:cy + y1, cx + x0:cx + x1]
    return out


def sense_one(world, origin, res, pose_xy, people, count, cell, size_x, size_y, beam_cells, agent_d2, table, base=0, outside_cost=255,
              min_cost=254, unknown=False):
    """One robot: (costmap [size_y,size_x], beam_kind [K], beam_cell [K,2], marks: the set of marked window cells, dropped:
    the number of hit cells outside the window)."""
    K = len(beam_cells)
    kind, hit = np.zeros(K, np.uint8), np.array(beam_cells, np.int32).reshape(K, 2).copy()
    marks, dropped = set(), 0
    a = point_cell(pose_xy[0], pose_xy[1], origin, res)
    if a is None:
        kind[:] = NO_ROBOT
    else:
        occupied = occupied_cells(people, count, origin, res, agent_d2)
        for k in range(K):
            kd, off, hits = cast(world, occupied, a, beam_cells[k], min_cost, unknown)
            kind[k], hit[k] = kd, off
            for o in hits:
                wx, wy = a[0] + o[0] - int(cell[0]), a[1] + o[1] - int(cell[1])
                if 0 <= wx < size_x and 0 <= wy < size_y:
                    marks.add((wx, wy))
                else:
                    dropped += 1
    cost = inflate(marks, size_x, size_y, table)
    if base:
        cost = np.maximum(cost, world_cut(world, cell, size_x, size_y, outside_cost))
    return cost, kind, hit, marks, dropped


def sensed_costmap(world, origin, res, robot_pose, people, count, cell, size_x, size_y, beam_cells, agent_d2, table, base=0,
                   outside_cost=255, min_cost=254, unknown=False, stats=None):
    """The whole call. world [Hy,Hx] with origin [2] (shared) or [B,Hy,Hx] with [B,2]; robot_pose [B,3]; people [B,Np,5]; count
    [B]; cell [B,2]. Returns (costmap [B,size_y,size_x] uint8, beam_kind [B,K] uint8, beam_cell [B,K,2] int32). stats: a dict
    that receives marks [B] (marked cells per robot) and dropped (hit cells outside their window, summed)."""
    world, origin = np.asarray(world, np.uint8), np.asarray(origin, np.float64).reshape(-1, 2)
    people = np.ascontiguousarray(people, np.float64)
    beam_cells = np.asarray(beam_cells, np.int64).reshape(-1, 2)
    B, K = people.shape[0], len(beam_cells)
    shared = world.ndim == 2
    costmap = np.zeros((B, size_y, size_x), np.uint8)
    kind, hit = np.zeros((B, K), np.uint8), np.zeros((B, K, 2), np.int32)
    n_marks, dropped = np.zeros(B, np.int64), 0
    for b in range(B):
        w, o = (world, origin[0]) if shared else (world[b], origin[b])
        costmap[b], kind[b], hit[b], marks, d = sense_one(w, o, res, robot_pose[b, :2], people[b], count[b], cell[b], size_x, size_y,
                                                          beam_cells, agent_d2, table, base, outside_cost, min_cost, unknown)
        n_marks[b], dropped = len(marks), dropped + d
    if stats is not None:
        stats.update(marks=n_marks, dropped=dropped)
    return costmap, kind, hit
