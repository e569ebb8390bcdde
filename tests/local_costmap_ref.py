"""The contract of smpc_local_costmap_batch (include/smpc_local_costmap.h) as plain numpy: the cell rule and the crop. The
one yardstick of tests/test_local_costmap.py, tests/test_gpu_local_costmap.py and tests/test_gpu_episode_world.py; written
on its own, not from the package's scenes.window_cells / scenes.crop_windows, which are checked against it.

numpy rounds every double operation on its own (it never fuses a product into a sum), which is what the contract asks."""
import numpy as np

LIMIT = 2.0 ** 30


def origin_of(w0, cell, res):
    """w0 + cell * res per axis: the product, then the sum. w0 [B,2] or [2], cell [B,2]."""
    prod = np.asarray(cell, np.int32).astype(np.float64) * np.float64(res)
    return np.asarray(w0, np.float64) + prod


def roll_axis(w0, cell, res, size, pose):
    """One axis of B robots with finite poses: the cell after the update, as float64 (an integer within +-2^30)."""
    o = origin_of(w0, cell, res)
    half = ((np.float64(size) - 1.0 + 0.5) * np.float64(res)) / 2.0
    want = np.asarray(pose, np.float64) - half
    with np.errstate(over="ignore"):
        d = np.trunc((want - o) / np.float64(res))
        return np.minimum(np.maximum(np.asarray(cell, np.int32).astype(np.float64) + d, -LIMIT), LIMIT)


def roll(world_origin, res, cell, pose, size_x, size_y, force=False):
    """(cell' [B,2] int32, costmap_origin [B,2], moved [B] int32, written [B] bool) for world_origin [2] or [B,2],
    cell [B,2] int32 and pose [B,>=2]. `force`: the stored cells count as (0,0) and every robot is written."""
    pose = np.asarray(pose, np.float64)
    B = pose.shape[0]
    w0 = np.broadcast_to(np.asarray(world_origin, np.float64).reshape(-1, 2), (B, 2))
    cell = np.zeros((B, 2), np.int32) if force else np.asarray(cell, np.int32).copy()
    finite = np.isfinite(pose[:, 0]) & np.isfinite(pose[:, 1])
    safe = np.where(finite[:, None], pose[:, 0:2], 0.0)
    new = cell.copy()
    for axis, size in ((0, size_x), (1, size_y)):
        c = roll_axis(w0[:, axis], cell[:, axis], res, size, safe[:, axis])
        new[:, axis] = np.where(finite, c, cell[:, axis]).astype(np.int32)
    changed = (new[:, 0] != cell[:, 0]) | (new[:, 1] != cell[:, 1])
    written = changed | bool(force)
    moved = np.where(finite, written.astype(np.int32), 2).astype(np.int32)
    return new, origin_of(w0, new, res), moved, written


def crop(world, cell, size_x, size_y, outside_cost):
    """[B,size_y,size_x] uint8: the overlap of every window with its world as one slice copy, outside_cost elsewhere.
    world [Hy,Hx] (one for all robots) or [B,Hy,Hx]."""
    world = np.asarray(world, np.uint8)
    B = len(cell)
    out = np.full((B, size_y, size_x), outside_cost, np.uint8)
    for b in range(B):
        w = world if world.ndim == 2 else world[b]
        Hy, Hx = w.shape
        cx, cy = int(cell[b][0]), int(cell[b][1])
        x0, x1, y0, y1 = max(cx, 0), min(cx + size_x, Hx), max(cy, 0), min(cy + size_y, Hy)
        if x0 < x1 and y0 < y1:
            out[b, y0 - cy:y1 - cy, x0 - cx:x1 - cx] = w[y0:y1, x0:x1]
    return out


def call(world, world_origin, res, pose, cell, costmap, costmap_origin, outside_cost, force=False):
    """One call of smpc_local_costmap_batch: (cell', costmap', costmap_origin', moved). The robots that are not written
    keep their rows of `costmap` and `costmap_origin` bit for bit (whatever those hold)."""
    costmap = np.asarray(costmap, np.uint8)
    B, size_y, size_x = costmap.shape
    new, origin, moved, written = roll(world_origin, res, cell, pose, size_x, size_y, force)
    window = crop(world, new, size_x, size_y, outside_cost)
    out_map = np.where(written[:, None, None], window, costmap)
    out_origin = np.asarray(costmap_origin, np.float64).copy()
    out_origin[written] = origin[written]
    return new, out_map, out_origin, moved


def same_bits(a, b):
    """Equal shapes, dtypes and bytes (doubles as raw 64-bit patterns)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
