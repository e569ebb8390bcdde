"""The nearest-agent gather of a shared world (include/smpc_nearest.h) as brute force in numpy: all pairs, then a stable
sort on (d2, c). The yardstick of tests/test_nearest.py, tests/test_gpu_nearest.py and tests/test_gpu_episode_shared.py.
numpy rounds every operation on its own, which is the contract. The bins do not occur here: they must not show."""
import numpy as np

MARGIN = 1.0 + 2.0 ** -20


def d2_matrix(agents, robot_pose):
    """d2 [B,A] = ddx * ddx + ddy * ddy, ddx = ax - rx (NaN / inf where a coordinate is not finite or a product overflows)."""
    agents = np.asarray(agents, np.float64).reshape(-1, 5)
    pose = np.asarray(robot_pose, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ddx = agents[None, :, 0] - pose[:, None, 0]
        ddy = agents[None, :, 1] - pose[:, None, 1]
        xx, yy = ddx * ddx, ddy * ddy
        return xx + yy


def qualifying(agents, robot_pose, max_range, self_row=None):
    """(ok [B,A] bool, d2 [B,A]): rule 2 for every pair; a robot without a finite x and y has no qualifying agent."""
    agents = np.asarray(agents, np.float64).reshape(-1, 5)
    pose = np.asarray(robot_pose, np.float64)
    B, A = pose.shape[0], agents.shape[0]
    d2 = d2_matrix(agents, pose)
    r2 = np.float64(max_range) * np.float64(max_range)
    with np.errstate(invalid="ignore"):
        ok = d2 <= r2
    ok &= np.isfinite(agents[:, 0:2]).all(axis=1)[None, :]
    ok &= np.isfinite(pose[:, 0:2]).all(axis=1)[:, None]
    if self_row is not None:
        ok &= np.arange(A)[None, :] != np.asarray(self_row, np.int64).reshape(B, 1)
    return ok, d2


def nearest_people(agents, robot_pose, Np, max_range, self_row=None, people=None, source=None):
    """(people [B,Np,5], count [B] int32, source [B,Np] int32). people / source: the arrays before the call (default NaN /
    -1); only the first count rows of each robot are written."""
    agents = np.asarray(agents, np.float64).reshape(-1, 5)
    pose = np.asarray(robot_pose, np.float64)
    B = pose.shape[0]
    people = np.full((B, Np, 5), np.nan) if people is None else np.array(people, np.float64)
    source = np.full((B, Np), -1, np.int32) if source is None else np.array(source, np.int32)
    count = np.zeros(B, np.int32)
    ok, d2 = qualifying(agents, pose, max_range, self_row)
    for b in range(B):
        rows = np.flatnonzero(ok[b])                                  # ascending c
        rows = rows[np.argsort(d2[b, rows], kind="stable")][:Np]      # stable: equal d2 keep ascending c
        count[b] = len(rows)
        people[b, :len(rows)] = agents[rows]
        source[b, :len(rows)] = rows
    return people, count, source


def bin_axis(p, origin, bin_size, n):
    """clamp(floor((p - origin) / bin_size), 0, n - 1), clamped as a double; a NaN goes to bin 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor((np.asarray(p, np.float64) - np.float64(origin)) / np.float64(bin_size))
    q = np.where(q > 0.0, q, 0.0)                                    # NaN, negative and -0.0 -> 0
    return np.where(q >= n - 1, n - 1, q).astype(np.int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
