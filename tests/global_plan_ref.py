"""The contract of smpc_goal_field_batch and smpc_extract_plan_batch (include/smpc_global_plan.h) as plain Python: a heapq
Dijkstra for the field, a plain loop for the walk and the poses. The one yardstick of tests/test_global_plan.py,
tests/test_gpu_global_plan.py and tests/test_gpu_episode_plans.py; written from the contract's text, not from
csrc/smpc_global_plan_rule.hpp, which is checked against it.

All costs are Python / numpy integers; numpy rounds every double operation on its own, which is what the contract asks of
the cell of a point and of a cell's centre."""
import heapq
from dataclasses import dataclass

import numpy as np

UNREACHABLE = 0xFFFFFFFF
NEIGHBOURS = [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1)]   # (dx, dy), the contract's order
OK, START_OUTSIDE, START_BLOCKED, UNREACHABLE_START, TRUNCATED, BAD_GOAL_INDEX, INCONSISTENT_FIELD = range(7)


@dataclass
class Cost:
    neutral_cost: int = 50
    cost_weight: int = 1
    lethal_min_cost: int = 253
    allow_unknown: bool = False


def passable(world, cost: Cost):
    """[Hy,Hx] bool."""
    world = np.asarray(world, np.uint8)
    return (world < cost.lethal_min_cost) | (bool(cost.allow_unknown) & (world == 255))


def weights(world, cost: Cost):
    """[Hy,Hx] int64: w(c) of the passable cells, 0 elsewhere."""
    return np.where(passable(world, cost), cost.neutral_cost + cost.cost_weight * np.asarray(world, np.int64), 0)


def cell_of(point, origin, resolution, cells_x, cells_y):
    """(cx, cy) of a point, or None when it has no cell."""
    q = np.floor((np.asarray(point, np.float64) - np.asarray(origin, np.float64)) / np.float64(resolution))
    if not np.isfinite(np.asarray(point, np.float64)).all():
        return None
    if not (0 <= q[0] < cells_x and 0 <= q[1] < cells_y):
        return None
    return int(q[0]), int(q[1])


def centre_of(cell, origin, resolution):
    """[2] float64: origin + (i + 0.5) * resolution per axis."""
    s = np.asarray(cell, np.int32).astype(np.float64) + 0.5
    m = s * np.float64(resolution)
    return np.asarray(origin, np.float64) + m


def steps_from(w, x, y):
    """The allowed steps out of passable cell (x, y): (k, nx, ny, cost of entering n)."""
    Hy, Hx = w.shape
    for k, (dx, dy) in enumerate(NEIGHBOURS):
        nx, ny = x + dx, y + dy
        if not (0 <= nx < Hx and 0 <= ny < Hy) or w[ny, nx] == 0:
            continue
        if dx != 0 and dy != 0 and (w[y, nx] == 0 or w[ny, x] == 0):
            continue
        yield k, nx, ny, (5 if k < 4 else 7) * int(w[ny, nx])


def goal_field(world, origin, resolution, goal, cost: Cost = Cost()):
    """(field [Hy,Hx] uint32, status) of one goal point."""
    world = np.asarray(world, np.uint8)
    Hy, Hx = world.shape
    field = np.full((Hy, Hx), UNREACHABLE, np.uint32)
    gc = cell_of(goal, origin, resolution, Hx, Hy)
    if gc is None:
        return field, 1
    w = weights(world, cost)
    if w[gc[1], gc[0]] == 0:
        return field, 2
    # field[c] = min over allowed steps c -> n of cost(n) + field[n]: Dijkstra from the goal over the reversed steps; the
    # step n -> c is allowed exactly when c -> n is (the diagonal rule is symmetric), and c -> n costs what entering n costs
    dist = {gc: 0}
    heap = [(0, gc[0], gc[1])]
    done = set()
    while heap:
        d, x, y = heapq.heappop(heap)
        if (x, y) in done:
            continue
        done.add((x, y))
        enter = None
        for k, nx, ny, _ in steps_from(w, x, y):           # predecessors c = (nx, ny) of n = (x, y)
            if (nx, ny) in done:
                continue
            if enter is None:
                enter = int(w[y, x])
            nd = d + (5 if k < 4 else 7) * enter
            if nd < dist.get((nx, ny), UNREACHABLE):
                dist[(nx, ny)] = nd
                heapq.heappush(heap, (nd, nx, ny))
    for (x, y), d in dist.items():
        field[y, x] = d
    return field, 0


def goal_fields(world, origin, resolution, goals, cost: Cost = Cost()):
    """(field [G,Hy,Hx], status [G]) for world [Hy,Hx] + origin [2] (shared) or [G,Hy,Hx] + [G,2]."""
    world, origin = np.asarray(world, np.uint8), np.asarray(origin, np.float64)
    out = [goal_field(world if world.ndim == 2 else world[g], origin if origin.ndim == 1 else origin[g], resolution, goal, cost)
           for g, goal in enumerate(np.asarray(goals, np.float64).reshape(-1, 2))]
    Hy, Hx = world.shape[-2:]
    return (np.stack([f for f, _ in out]) if out else np.zeros((0, Hy, Hx), np.uint32)), np.array([s for _, s in out], np.int32)


def walk(world, field, start_cell, cost: Cost = Cost()):
    """(cells [(x, y)] c0 .. cn, error) down `field` from start_cell by the contract's rule; error 0 or INCONSISTENT_FIELD."""
    w = weights(world, cost)
    x, y = start_cell
    cells = [(x, y)]
    limit = field.size
    while field[y, x] != 0:
        here = int(field[y, x])
        nxt = None
        for k, nx, ny, c in steps_from(w, x, y):
            if field[ny, nx] != UNREACHABLE and int(field[ny, nx]) + c == here:
                nxt = (nx, ny)
                break
        if nxt is None or len(cells) - 1 >= limit:
            return cells, INCONSISTENT_FIELD
        x, y = nxt
        cells.append(nxt)
    return cells, OK


def extract_plan(world, origin, resolution, fields, goals, robot_goal, pose, L, stride=1, cost: Cost = Cost(), plan=None, cells_out=None):
    """(plan [B,L,2], plan_len [B], error [B]) by the contract; `plan`: the rows before the call (default NaN), of which
    those the call does not write stay. world / origin shared or per goal as in goal_fields. cells_out: a list that
    receives every robot's path cells (None for a robot without a walk)."""
    world, origin = np.asarray(world, np.uint8), np.asarray(origin, np.float64)
    fields, goals, pose = np.asarray(fields, np.uint32), np.asarray(goals, np.float64).reshape(-1, 2), np.asarray(pose, np.float64)
    B, G = pose.shape[0], fields.shape[0]
    Hy, Hx = world.shape[-2:]
    plan = np.full((B, L, 2), np.nan) if plan is None else np.array(plan, np.float64)
    plan_len, error = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        path = None
        g = int(robot_goal[b])
        if not 0 <= g < G:
            error[b] = BAD_GOAL_INDEX
        else:
            wm, o = (world if world.ndim == 2 else world[g]), (origin if origin.ndim == 1 else origin[g])
            c0 = cell_of(pose[b, 0:2], o, resolution, Hx, Hy)
            if c0 is None:
                error[b] = START_OUTSIDE
            elif not passable(wm, cost)[c0[1], c0[0]]:
                error[b] = START_BLOCKED
            elif fields[g][c0[1], c0[0]] == UNREACHABLE:
                error[b] = UNREACHABLE_START
            else:
                path, error[b] = walk(wm, fields[g], c0, cost)
                if error[b] == OK:
                    n = len(path) - 1
                    rows = [pose[b, 0:2]] + [centre_of(path[j], o, resolution) for j in range(stride, n, stride)] + [goals[g]]
                    if len(rows) > L:
                        rows, error[b] = rows[:L], TRUNCATED
                    plan[b, :len(rows)] = np.array(rows)
                    plan_len[b] = len(rows)
                else:
                    path = None
        if cells_out is not None:
            cells_out.append(path)
    return plan, plan_len, error


def same_bits(a, b):
    """Equal shapes, dtypes and bytes (doubles as raw 64-bit patterns)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
