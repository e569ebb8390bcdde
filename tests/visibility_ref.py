"""The contract of smpc_visible_people_batch (include/smpc_visibility.h) as plain Python and numpy: per person the cells, the
range gate and the sight line as the sequential walk of the contract's text, then the compaction. The one yardstick of
tests/test_visibility.py, tests/test_gpu_visibility.py and tests/test_gpu_episode_visibility.py; written from the
contract, not from csrc/smpc_visibility_rule.hpp (which takes a ray column by column in closed form and is checked
against this)."""
import math

import numpy as np

HIDDEN, SEEN, OUT_OF_RANGE, NOT_FINITE = 0, 1, 2, 3
MAX_CELL = float(2 ** 30)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cell_axis(p, origin, res):
    """floor((p - origin) / res) as a double, every operation rounded on its own (numpy float64 does just that)."""
    with np.errstate(all="ignore"):
        return float(np.floor((np.float64(p) - np.float64(origin)) / np.float64(res)))


def in_range(rx, ry, px, py, max_range):
    with np.errstate(all="ignore"):
        ddx, ddy = np.float64(px) - np.float64(rx), np.float64(py) - np.float64(ry)
        return bool(ddx * ddx + ddy * ddy <= np.float64(max_range) * np.float64(max_range))


def occludes(world, x, y, min_cost=254, unknown=False):
    """Does cell (x, y) block sight? Cells outside the world never do."""
    Hy, Hx = world.shape
    if not (0 <= x < Hx and 0 <= y < Hy):
        return False
    c = int(world[y, x])
    return c >= min_cost and (c != 255 or bool(unknown))


def hidden(world, a, b, min_cost=254, unknown=False):
    """The sight line between the centres of cells a and b, as the contract's walk."""
    (ax, ay), (bx, by) = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    dx, dy = abs(bx - ax), abs(by - ay)
    sx, sy = (1 if bx > ax else -1), (1 if by > ay else -1)
    occ = lambda i, j: occludes(world, ax + sx * i, ay + sy * j, min_cost, unknown)
    i = j = 0
    while (i, j) != (dx, dy):
        A, Bv = (2 * i + 1) * dy, (2 * j + 1) * dx
        if A < Bv:
            i += 1
        elif A > Bv:
            j += 1
        else:  # exactly through a lattice corner: sight passes unless both cells that touch it there occlude
            if occ(i + 1, j) and occ(i, j + 1):
                return True
            i, j = i + 1, j + 1
        if (i, j) != (dx, dy) and occ(i, j):
            return True
    return False


def walk_cells(a, b):
    """(the cells the walk steps on between a and b, both excluded; the pairs it tests at lattice corners), in walk order."""
    (ax, ay), (bx, by) = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    dx, dy = abs(bx - ax), abs(by - ay)
    sx, sy = (1 if bx > ax else -1), (1 if by > ay else -1)
    at = lambda i, j: (ax + sx * i, ay + sy * j)
    cells, pairs, i, j = [], [], 0, 0
    while (i, j) != (dx, dy):
        A, Bv = (2 * i + 1) * dy, (2 * j + 1) * dx
        if A == Bv:
            pairs.append((at(i + 1, j), at(i, j + 1)))
        i, j = i + (A <= Bv), j + (A >= Bv)
        if (i, j) != (dx, dy):
            cells.append(at(i, j))
    return cells, pairs


def classify(world, origin, res, robot_xy, person_xy, max_range=10.0, min_cost=254, unknown=False):
    """The code of one person as seen from one robot."""
    rx, ry = float(robot_xy[0]), float(robot_xy[1])
    qrx, qry = cell_axis(rx, origin[0], res), cell_axis(ry, origin[1], res)
    if not (math.isfinite(rx) and math.isfinite(ry)) or not (abs(qrx) <= MAX_CELL and abs(qry) <= MAX_CELL):
        return NOT_FINITE
    px, py = float(person_xy[0]), float(person_xy[1])
    if not (math.isfinite(px) and math.isfinite(py)):
        return NOT_FINITE
    if not in_range(rx, ry, px, py, max_range):
        return OUT_OF_RANGE
    a = (int(qrx), int(qry))
    b = (int(cell_axis(px, origin[0], res)), int(cell_axis(py, origin[1], res)))
    return HIDDEN if hidden(world, a, b, min_cost, unknown) else SEEN


def visible_people(world, origin, res, robot_pose, people, count, max_range=10.0, min_cost=254, unknown=False, visible=None,
                   seen=None):
    """The whole call. world [Hy,Hx] with origin [2] (shared) or [B,Hy,Hx] with [B,2]; robot_pose [B,3]; people [B,Np,5]; count
    [B]. visible / seen: the arrays before the call (default NaN / 0xEE): rows from visible_count[b] on and flags from
    count[b] on are left as they are. Returns (visible [B,Np,5], visible_count [B] int32, seen [B,Np] uint8)."""
    world, origin = np.asarray(world, np.uint8), np.asarray(origin, np.float64)
    people = np.ascontiguousarray(people, np.float64)
    B, Np = people.shape[:2]
    shared = world.ndim == 2
    origin = origin.reshape(-1, 2)
    visible = np.full((B, Np, 5), np.nan) if visible is None else np.array(visible, np.float64)
    seen = np.full((B, Np), 0xEE, np.uint8) if seen is None else np.array(seen, np.uint8)
    n = np.zeros(B, np.int32)
    for b in range(B):
        w, o = (world, origin[0]) if shared else (world[b], origin[b])
        for j in range(min(max(int(count[b]), 0), Np)):
            code = classify(w, o, res, robot_pose[b, :2], people[b, j, :2], max_range, min_cost, unknown)
            seen[b, j] = code
            if code == SEEN:
                visible[b, n[b]] = people[b, j]
                n[b] += 1
    return visible, n, seen
