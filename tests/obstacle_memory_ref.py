"""The contract of smpc_obstacle_memory_batch (include/smpc_obstacle_memory.h) as plain Python integers and sets: per robot
the roll of the marked cells, every beam as the sequential walk of the contract's text with the cells it passes, clears,
marks within mark_d2, the footprint, and the window by sensed_costmap_ref's brute-force inflation. The one yardstick of
tests/test_obstacle_memory.py, tests/test_gpu_obstacle_memory.py and tests/test_gpu_episode_obstacle_memory.py; written from
the header's text, not from csrc/smpc_obstacle_memory_rule.hpp (which walks a beam column by column in closed form and rolls
words, and is checked against this).

The state of a call is (memory [B,size_y,W] uint32, memory_cell [B,2] int32), exactly the two arrays of the C call."""
import math

import numpy as np

import sensed_costmap_ref as R


def words(size_x):
    return (int(size_x) + 31) // 32


def zero_state(B, size_x, size_y):
    return np.zeros((B, size_y, words(size_x)), np.uint32), np.zeros((B, 2), np.int32)


def bits_to_cells(bitmap, size_x):
    """The set of window cells (x, y) whose bit is set; bits of columns >= size_x are ignored."""
    cells = set()
    for y, w in zip(*np.nonzero(bitmap)):
        v = int(bitmap[y, w])
        for t in range(32):
            if (v >> t) & 1 and 32 * int(w) + t < size_x:
                cells.add((32 * int(w) + t, int(y)))
    return cells


def cells_to_bits(cells, size_x, size_y):
    out = np.zeros((size_y, words(size_x)), np.uint32)
    for x, y in cells:
        out[y, x >> 5] |= np.uint32(1 << (x & 31))
    return out


def walk(world, occupied, a, off, min_cost=254, unknown=False):
    """One beam from cell a to a + off: (kind, the offset beam_cell reports, the hit cells as offsets, the passed cells as
    offsets). The walk of smpc_sensed_costmap.h rule 3, step by step, with rule 3 of smpc_obstacle_memory.h beside it."""
    ex, ey = int(off[0]), int(off[1])
    if abs(ex) > R.MAX_REACH or abs(ey) > R.MAX_REACH:
        return R.INVALID, (ex, ey), [], []
    dx, dy = abs(ex), abs(ey)
    sx, sy = (1 if ex > 0 else -1), (1 if ey > 0 else -1)
    at = lambda i, j: (sx * i, sy * j)
    test = lambda o: R.stops(world, occupied, a, (a[0] + o[0], a[1] + o[1]), min_cost, unknown)
    passed = [(0, 0)]                                                                     # the robot's own cell
    i = j = 0
    while (i, j) != (dx, dy):
        A, Bv = (2 * i + 1) * dy, (2 * j + 1) * dx
        if A < Bv:
            i += 1
        elif A > Bv:
            j += 1
        else:  # a lattice corner: the pair is tested, never passed
            along_x, along_y = at(i + 1, j), at(i, j + 1)
            if test(along_x) and test(along_y):
                return R.CORNER_PAIR, along_x, [along_x, along_y], passed
            i, j = i + 1, j + 1
        kind = test(at(i, j))
        if kind:
            return kind, at(i, j), [at(i, j)], passed
        passed.append(at(i, j))
    return R.NONE, (ex, ey), [], passed


COUNTERS = ("kept", "cleared", "rolled_out", "beyond_mark", "footprint")


def step_one(bitmap, memory_cell, world, origin, res, pose_xy, people, count, cell, size_x, size_y, beam_cells, agent_d2, table,
             mark_d2, footprint_d2, base=0, outside_cost=255, min_cost=254, unknown=False):
    """One robot: (costmap, beam_kind, beam_cell, new bitmap, counters)."""
    inside = lambda x, y: 0 <= x < size_x and 0 <= y < size_y
    # rule 2: the roll
    sx, sy = int(memory_cell[0]) - int(cell[0]), int(memory_cell[1]) - int(cell[1])
    old = bits_to_cells(bitmap, size_x)
    rolled = {(x + sx, y + sy) for x, y in old if inside(x + sx, y + sy)}
    stats = dict.fromkeys(COUNTERS, 0)
    stats["rolled_out"] = len(old) - len(rolled)
    K = len(beam_cells)
    kind, hit = np.zeros(K, np.uint8), np.array(beam_cells, np.int32).reshape(K, 2).copy()
    marks = set(rolled)
    a = R.point_cell(pose_xy[0], pose_xy[1], origin, res)
    hit_now = set()
    if a is None:
        kind[:] = R.NO_ROBOT
    else:
        occupied = R.occupied_cells(people, count, origin, res, agent_d2)
        win = lambda o: (a[0] + o[0] - int(cell[0]), a[1] + o[1] - int(cell[1]))
        cleared, marked = set(), set()
        for k in range(K):
            kd, off, hits, passed = walk(world, occupied, a, beam_cells[k], min_cost, unknown)
            kind[k], hit[k] = kd, off
            cleared.update(win(o) for o in passed if inside(*win(o)))                     # rule 3
            for o in hits:                                                                # rule 4
                if o[0] * o[0] + o[1] * o[1] <= mark_d2:
                    if inside(*win(o)):
                        marked.add(win(o))
                else:
                    stats["beyond_mark"] += 1
                if inside(*win(o)):
                    hit_now.add(win(o))
        assert not cleared & marked                                                       # what the header promises
        stats["cleared"] = len(marks & cleared)
        marks = (marks - cleared) | marked
        if footprint_d2 >= 0:                                                             # rule 5
            ra = math.isqrt(footprint_d2)
            under = {win((i, j)) for i in range(-ra, ra + 1) for j in range(-ra, ra + 1) if i * i + j * j <= footprint_d2}
            stats["footprint"] = len(marks & under)
            marks -= under
    stats["kept"] = len(marks - hit_now)
    cost = R.inflate(marks, size_x, size_y, table)
    if base:
        cost = np.maximum(cost, R.world_cut(world, cell, size_x, size_y, outside_cost))
    return cost, kind, hit, cells_to_bits(marks, size_x, size_y), stats


def step(state, world, origin, res, robot_pose, people, count, cell, size_x, size_y, beam_cells, agent_d2, table, mark_d2,
         footprint_d2, base=0, outside_cost=255, min_cost=254, unknown=False):
    """The whole call on state = (memory, memory_cell). world [Hy,Hx] with origin [2] (shared) or [B,Hy,Hx] with [B,2].
    Returns (costmap [B,size_y,size_x] uint8, beam_kind [B,K] uint8, beam_cell [B,K,2] int32, the new state, stats: per
    counter of COUNTERS an int64 array [B])."""
    memory, memory_cell = state
    world, origin = np.asarray(world, np.uint8), np.asarray(origin, np.float64).reshape(-1, 2)
    people = np.ascontiguousarray(people, np.float64)
    beam_cells = np.asarray(beam_cells, np.int64).reshape(-1, 2)
    B, K = people.shape[0], len(beam_cells)
    shared = world.ndim == 2
    costmap = np.zeros((B, size_y, size_x), np.uint8)
    kind, hit = np.zeros((B, K), np.uint8), np.zeros((B, K, 2), np.int32)
    new_memory = np.zeros((B, size_y, words(size_x)), np.uint32)
    stats = {name: np.zeros(B, np.int64) for name in COUNTERS}
    for b in range(B):
        w, o = (world, origin[0]) if shared else (world[b], origin[b])
        costmap[b], kind[b], hit[b], new_memory[b], st = step_one(
            np.asarray(memory[b]).view(np.uint32), memory_cell[b], w, o, res, robot_pose[b, :2], people[b], count[b], cell[b], size_x,
            size_y, beam_cells, agent_d2, table, mark_d2, footprint_d2, base, outside_cost, min_cost, unknown)
        for name in COUNTERS:
            stats[name][b] = st[name]
    return costmap, kind, hit, (new_memory, np.asarray(cell, np.int32).copy()), stats
