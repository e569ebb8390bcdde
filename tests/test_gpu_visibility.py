"""smpc_visible_people_batch on the GPU against tests/visibility_ref.py, bit for bit: batches from 1 x 1 to 130 x 8 on worlds
from one cell to 256 x 192, every ordered pair of cells of a 9 x 7 map, rays across the 64-column stride of the kernel's
lanes with the one occluding cell in every column in turn, the octants and corner slopes, robots and persons off the world
and not finite, every clamp of `count`, shared and per-robot worlds, host and device pointers, poisoned rows and flags
beyond the counts, and the refusals."""
import itertools

import numpy as np
import pytest

import visibility_ref as V
from nav2_social_mpc_controller_amd import _abi_visibility as VA
from nav2_social_mpc_controller_amd.params import OptimizerParams, VisibilityParams

pytestmark = pytest.mark.gpu
POISON_ROW, POISON_FLAG = -3.25, 0xEE


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


def check(solver, world, origin, res, pose, people, count, vp=VisibilityParams()):
    """One host-pointer call on poisoned outputs against the reference on the same poison. Returns the device's outputs."""
    B, Np = people.shape[:2]
    poison_v, poison_s = np.full((B, Np, 5), POISON_ROW), np.full((B, Np), POISON_FLAG, np.uint8)
    vis, n, seen = solver.visible_people(vp, world, origin, res, pose, people, count, visible=poison_v, seen=poison_s)
    want_vis, want_n, want_seen = V.visible_people(world, origin, res, pose, people, count, vp.max_range, vp.occlusion_min_cost,
                                                   vp.unknown_occludes, visible=poison_v, seen=poison_s)
    assert n.dtype == np.int32 and seen.dtype == np.uint8
    assert np.array_equal(seen, want_seen), np.argwhere(seen != want_seen)[:5]
    assert np.array_equal(n, want_n) and V.same_bits(vis, want_vis)
    return vis, n, seen


def centres(cells, origin=(0.0, 0.0), res=1.0):
    """People rows [.., 5] at the centres of `cells` [.., 2], with distinct payloads in the other three columns."""
    cells = np.asarray(cells, np.float64)
    rows = np.zeros(cells.shape[:-1] + (5,))
    rows[..., :2] = np.asarray(origin) + (cells + 0.5) * res
    rows[..., 2:] = np.arange(rows[..., 2:].size).reshape(rows[..., 2:].shape) * 0.5 - 7.0
    return rows


def pose_at(cells, origin=(0.0, 0.0), res=1.0):
    cells = np.asarray(cells, np.float64)
    return np.concatenate([np.asarray(origin) + (cells + 0.5) * res, np.full(cells.shape[:-1] + (1,), 0.3)], axis=-1)


# ---- shapes and worlds ---------------------------------------------------------------------------------------------------
def floor(Hx, Hy):
    from nav2_social_mpc_controller_amd.scenes import make_world
    if (Hx, Hy) == (1, 1):
        return np.full((1, 1), 254, np.uint8), np.array([0.3, -0.2]), 0.5
    if (Hx, Hy) == (9, 7):
        g = np.random.default_rng(97)
        return g.choice(np.array([0, 0, 0, 100, 254, 254, 255], np.uint8), (7, 9)), np.array([-1.0, 2.0]), 0.25
    w = make_world(Hx, Hy, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15))
    return w.map, w.origin, w.resolution


@pytest.mark.parametrize("B,Np,Hx,Hy", [(1, 1, 1, 1), (3, 64, 9, 7), (65, 33, 61, 47), (130, 8, 256, 192)])
def test_batches_on_worlds_from_one_cell_to_256_x_192(solver, B, Np, Hx, Hy):
    world, origin, res = floor(Hx, Hy)
    g = np.random.default_rng(B * 1000 + Np)
    size = np.array([Hx, Hy]) * res
    pose = np.concatenate([origin + g.uniform(-0.1, 1.1, (B, 2)) * size, g.uniform(-3, 3, (B, 1))], axis=1)
    people = g.uniform(-5.0, 5.0, (B, Np, 5))
    people[:, :, :2] = origin + g.uniform(-0.15, 1.15, (B, Np, 2)) * size                     # on and around the floor
    count = g.integers(0, Np + 1, B).astype(np.int32)
    count[0] = Np
    for vp in (VisibilityParams(), VisibilityParams(max_range=0.4 * float(size.max()) + 0.1, occlusion_min_cost=100, unknown_occludes=True)):
        vis, n, seen = check(solver, world, origin, res, pose, people, count, vp)
    valid = np.arange(Np)[None, :] < count[:, None]
    if B > 1:
        assert {V.HIDDEN, V.SEEN, V.OUT_OF_RANGE} <= set(seen[valid])
    if B == 130:                                                                              # a robot's row is its B = 1 call
        for b in (0, 64, 129):
            one = solver.visible_people(vp, world, origin, res, pose[b:b + 1], people[b:b + 1], count[b:b + 1],
                                        visible=np.full((1, Np, 5), POISON_ROW), seen=np.full((1, Np), POISON_FLAG, np.uint8))
            assert V.same_bits(one[0][0], vis[b]) and one[1][0] == n[b] and np.array_equal(one[2][0], seen[b])


def test_every_ordered_pair_of_cells_of_a_9_x_7_map_and_symmetry_from_the_device_flags(solver):
    world, _, _ = floor(9, 7)
    cells = np.array(list(itertools.product(range(9), range(7))))
    people = np.broadcast_to(centres(cells)[None], (63, 63, 5)).copy()
    for vp in (VisibilityParams(max_range=100.0), VisibilityParams(max_range=100.0, unknown_occludes=True),
               VisibilityParams(max_range=100.0, occlusion_min_cost=100)):
        _, n, seen = check(solver, world, [0.0, 0.0], 1.0, pose_at(cells), people, np.full(63, 63, np.int32), vp)
        assert np.array_equal(seen, seen.T) and (np.diag(seen) == V.SEEN).all()               # robot at cell b, person at cell j
        assert 0.1 < (seen == V.HIDDEN).mean() < 0.9
    # the same with a range that cuts: symmetric too
    _, _, seen = check(solver, world, [0.0, 0.0], 1.0, pose_at(cells), people, np.full(63, 63, np.int32), VisibilityParams(max_range=4.0))
    assert np.array_equal(seen, seen.T) and (seen == V.OUT_OF_RANGE).any()


# ---- the lanes' 64-column stride --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,m,sx,sy,swap", [(63, 20, 1, 1, False), (64, 64, -1, 1, True), (65, 0, 1, -1, False), (129, 43, -1, -1, True),
                                            (200, 67, 1, 1, True), (64, 21, -1, -1, False)])
def test_long_rays_with_the_one_occluding_cell_in_every_column_in_turn(solver, M, m, sx, sy, swap):
    """Robot k of M + 1 has a world of its own whose only occluding cell lies on the ray in major column k (columns 0 and M
    hold the robot's and the person's own cells, which never occlude); a second person stands one cell short of it."""
    ex, ey = (m, M) if swap else (M, m)
    Hx, Hy = ex + 1, ey + 1
    a = np.array([0 if sx > 0 else ex, 0 if sy > 0 else ey])
    b = a + np.array([sx * ex, sy * ey])
    worlds = np.zeros((M + 1, Hy, Hx), np.uint8)
    short = np.zeros((M + 1, 2), np.int64)
    for k in range(M + 1):
        r = (2 * k * m + M) // (2 * M)                    # the row of the ray at the centre of column k
        cx, cy = (a[0] + sx * r, a[1] + sy * k) if swap else (a[0] + sx * k, a[1] + sy * r)
        worlds[k, cy, cx] = 254
        kk = max(k - 1, 0)
        rr = (2 * kk * m + M) // (2 * M)
        short[k] = (a[0] + sx * rr, a[1] + sy * kk) if swap else (a[0] + sx * kk, a[1] + sy * rr)
    people = np.stack([np.broadcast_to(centres(b), (M + 1, 5)), centres(short)], axis=1)
    origins = np.zeros((M + 1, 2))
    _, n, seen = check(solver, worlds, origins, 1.0, np.broadcast_to(pose_at(a), (M + 1, 3)).copy(), people,
                       np.full(M + 1, 2, np.int32), VisibilityParams(max_range=300.0))
    assert seen[:, 0].tolist() == [V.SEEN] + [V.HIDDEN] * (M - 1) + [V.SEEN]
    assert (seen[:, 1] == V.SEEN).all()


def test_the_eight_octants_and_the_corner_slopes(solver):
    a = (12, 12)
    worlds, persons = [], []
    for p, q in ((3, 1), (5, 3), (9, 3), (4, 4), (6, 0), (7, 2)):
        for ex, ey in ((p, q), (q, p)):
            for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
                b = (a[0] + sx * ex, a[1] + sy * ey)
                cells, pairs = V.walk_cells(a, b)
                for c0, c1 in pairs:                       # one corner cell, the other, both
                    for occluding in ([c0], [c1], [c0, c1]):
                        worlds.append(occluding)
                        persons.append(b)
                for c in cells[:: max(1, len(cells) // 3)]:
                    worlds.append([c])
                    persons.append(b)
                worlds.append([a, b])                      # the end cells never occlude
                persons.append(b)
    B = len(worlds)
    maps = np.zeros((B, 25, 25), np.uint8)
    for k, occluding in enumerate(worlds):
        for c in occluding:
            maps[k, c[1], c[0]] = 254
    people = centres(np.array(persons))[:, None, :]
    _, _, seen = check(solver, maps, np.zeros((B, 2)), 1.0, np.broadcast_to(pose_at(a), (B, 3)).copy(), people, np.ones(B, np.int32),
                       VisibilityParams(max_range=50.0))
    want = [V.HIDDEN if (len(o) == 2 and a not in o) or (len(o) == 1 and o[0] in V.walk_cells(a, p)[0]) else V.SEEN for o, p in zip(worlds, persons)]
    assert seen[:, 0].tolist() == want and want.count(V.HIDDEN) > 50 and want.count(V.SEEN) > 50


# ---- off the world, not finite, count -------------------------------------------------------------------------------------------
def test_robots_and_persons_off_the_world_and_not_finite(solver):
    world = np.zeros((7, 9), np.uint8)
    world[3, 4] = 254
    world[1, 1] = 255
    origin, res = np.array([0.0, 0.0]), 1.0
    nan, inf = np.nan, np.inf
    spots = [[-3.5, 3.5], [12.5, 3.5], [4.5, -6.5], [4.5, 11.5], [-2.5, -2.5], [20.5, 20.5], [0.5, 3.5], [8.5, 3.5], [4.5, 3.5], [1.5, 1.5],
             [nan, 3.5], [4.5, nan], [inf, 3.5], [4.5, -inf], [1e300, 3.5], [-1e300, -1e300], [1e12, 3.5], [2.0 ** 30 + 1.5, 0.5],
             [2.0 ** 30 + 0.5, 0.5], [-2.0 ** 30 + 0.5, 0.5], [-2.0 ** 30 - 0.5, 0.5], [2.0 ** 30 + 0.5, 2.5]]
    B = Np = len(spots)
    pose = np.concatenate([np.array(spots), np.zeros((B, 1))], axis=1)
    people = np.zeros((B, Np, 5))
    people[:, :, :2] = np.array(spots)[None]
    people[:, :, 2:] = np.arange(B * Np * 3).reshape(B, Np, 3)
    people[:, 3, 2] = nan                                    # a payload that is not a number is copied as it is
    for vp in (VisibilityParams(max_range=40.0), VisibilityParams(max_range=40.0, unknown_occludes=True), VisibilityParams(max_range=5.0)):
        _, n, seen = check(solver, world, origin, res, pose, people, np.full(B, Np, np.int32), vp)
        bad_robot = [10, 11, 12, 13, 17, 20]                 # not finite, or |q| > 2^30 (1e300 and 1e12 too)
        assert (seen[bad_robot] == V.NOT_FINITE).all() and (seen[[14, 15, 16]] == V.NOT_FINITE).all() and (n[bad_robot] == 0).all()
        assert (seen[:10, 10:14] == V.NOT_FINITE).all() and (seen[:10, 14:17] == V.OUT_OF_RANGE).all()
    assert seen[18, 21] == V.SEEN and seen[18, 18] == V.SEEN and seen[19, 19] == V.SEEN      # at the 2^30 bound, off the world
    _, _, seen = check(solver, world, origin, res, pose, people, np.full(B, Np, np.int32), VisibilityParams(max_range=40.0))
    assert seen[0, 1] == V.HIDDEN and seen[2, 3] == V.HIDDEN and seen[6, 7] == V.HIDDEN and seen[0, 4] == V.SEEN


def test_count_of_zero_np_negative_and_above_np(solver):
    world, origin, res = floor(61, 47)
    g = np.random.default_rng(5)
    B, Np = 9, 6
    pose = np.concatenate([origin + g.uniform(0.2, 0.8, (B, 2)) * np.array([61, 47]) * res, np.zeros((B, 1))], axis=1)
    people = g.uniform(-1.0, 1.0, (B, Np, 5))
    people[:, :, :2] = pose[:, None, :2] + g.uniform(-1.0, 1.0, (B, Np, 2))
    count = np.array([0, Np, -1, -2 ** 31, Np + 1, 2 ** 31 - 1, 1, Np - 1, 3], np.int32)
    vis, n, seen = check(solver, world, origin, res, pose, people, count)
    assert (n[[0, 2, 3]] == 0).all() and (seen[[0, 2, 3]] == POISON_FLAG).all() and (vis[[0, 2, 3]] == POISON_ROW).all()
    assert (seen[[1, 4, 5]] != POISON_FLAG).all() and n.sum() > 10


# ---- worlds per robot, pointers, NULL seen ------------------------------------------------------------------------------------
def test_per_robot_worlds_are_the_shared_world_calls_robot_by_robot(solver):
    g = np.random.default_rng(11)
    B, Np = 5, 7
    worlds = (g.random((B, 13, 17)) < 0.15).astype(np.uint8) * 254
    origins = g.uniform(-2.0, 2.0, (B, 2))
    pose = np.concatenate([origins + g.uniform(0.0, 1.0, (B, 2)) * np.array([17, 13]) * 0.5, np.zeros((B, 1))], axis=1)
    people = g.uniform(-1.0, 1.0, (B, Np, 5))
    people[:, :, :2] = origins[:, None] + g.uniform(0.0, 1.0, (B, Np, 2)) * np.array([17, 13]) * 0.5
    count = np.full(B, Np, np.int32)
    vis, n, seen = check(solver, worlds, origins, 0.5, pose, people, count)
    assert len({w.tobytes() for w in worlds}) == B and (seen == V.HIDDEN).any() and (seen == V.SEEN).any()
    for b in range(B):
        one = check(solver, worlds[b], origins[b], 0.5, pose[b:b + 1], people[b:b + 1], count[b:b + 1])
        assert V.same_bits(one[0][0], vis[b]) and one[1][0] == n[b] and np.array_equal(one[2][0], seen[b])


def test_device_pointers_give_the_host_pointers_outputs_and_seen_may_be_null(solver):
    import torch
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point
    world, origin, res = floor(61, 47)
    g = np.random.default_rng(13)
    B, Np, vp = 67, 5, VisibilityParams(max_range=2.0)
    pose = np.concatenate([origin + g.uniform(0.0, 1.0, (B, 2)) * np.array([61, 47]) * res, np.zeros((B, 1))], axis=1)
    people = g.uniform(-1.0, 1.0, (B, Np, 5))
    people[:, :, :2] = origin + g.uniform(0.0, 1.0, (B, Np, 2)) * np.array([61, 47]) * res
    count = g.integers(-1, Np + 2, B).astype(np.int32)
    vis, n, seen = check(solver, world, origin, res, pose, people, count, vp)
    dev = "cuda:0"
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(world=world, world_origin=origin.reshape(1, 2), robot_pose=pose, people=people, count=count).items()}
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    vi = point(BatchSolver.visibility_c(vp, B, Np, 61, 47, True, res, 1), t)
    outs = []
    for with_seen in (True, False):
        d_vis = torch.full((B, Np, 5), POISON_ROW, dtype=torch.float64, device=dev)
        d_n = torch.full((B,), -7, dtype=torch.int32, device=dev)
        d_seen = torch.full((B, Np), POISON_FLAG, dtype=torch.uint8, device=dev)
        solver.visible_people_device(vi, d_vis.data_ptr(), d_n.data_ptr(), d_seen.data_ptr() if with_seen else 0)
        outs.append((d_vis, d_n, d_seen))
    torch.cuda.synchronize()
    solver.set_stream(0)
    for (d_vis, d_n, d_seen), with_seen in zip(outs, (True, False)):
        assert V.same_bits(d_vis.cpu().numpy(), vis) and np.array_equal(d_n.cpu().numpy(), n)
        assert np.array_equal(d_seen.cpu().numpy(), seen) if with_seen else (d_seen.cpu().numpy() == POISON_FLAG).all()
    # host pointers with seen = NULL
    hv, hn = np.full((B, Np, 5), POISON_ROW), np.zeros(B, np.int32)
    from nav2_social_mpc_controller_amd.solver import _ptr
    hi = point(BatchSolver.visibility_c(vp, B, Np, 61, 47, True, res, 0),
               dict(world=world, world_origin=origin.reshape(1, 2), robot_pose=pose, people=people, count=count))
    solver._call("smpc_visible_people_batch", hi, _ptr(hv), _ptr(hn), None)
    assert V.same_bits(hv, vis) and np.array_equal(hn, n)


# ---- a person walks past a pillar --------------------------------------------------------------------------------------------
def test_a_person_walked_past_a_pillar_is_seen_then_hidden_then_seen(solver):
    world = np.zeros((60, 80), np.uint8)
    world[28:33, 38:43] = 254                                # a pillar of 5 x 5 cells = 0.25 m, 2 m in front of the robot
    origin, res = np.array([-1.0, -1.5]), 0.05
    steps = 40
    pose = np.tile([[-0.5, 0.0, 0.0]], (steps, 1))            # cell (10, 30); the pillar's centre is cell (40, 30)
    people = np.zeros((steps, 1, 5))
    people[:, 0, 0] = 2.6                                    # walking along x = 2.6 m, from y = -1.2 to y = 1.2
    people[:, 0, 1] = -1.2 + 2.4 * np.arange(steps) / (steps - 1)
    people[:, 0, 2:] = [0.0, 1.2, 0.0]
    _, n, seen = check(solver, world, origin, res, pose, people, np.ones(steps, np.int32))
    want = [V.classify(world, origin, res, pose[k, :2], people[k, 0, :2]) for k in range(steps)]
    assert seen[:, 0].tolist() == want
    hidden = np.flatnonzero(np.array(want) == V.HIDDEN)
    assert len(hidden) >= 5 and hidden[0] > 5 and hidden[-1] < steps - 6 and np.array_equal(hidden, np.arange(hidden[0], hidden[-1] + 1))
    assert all(c == V.SEEN for k, c in enumerate(want) if k < hidden[0] or k > hidden[-1]) and np.array_equal(n, (np.array(want) == V.SEEN))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_poisoned_outputs_alone(solver):
    import re

    from nav2_social_mpc_controller_amd.solver import SmpcError, _ptr
    world, origin = np.zeros((5, 7), np.uint8), np.zeros((1, 2))
    pose, people, count = np.array([[3.5, 3.5, 0.0]]), np.full((1, 2, 5), 2.5), np.full(1, 2, np.int32)
    vis, n, seen = np.full((1, 2, 5), POISON_ROW), np.full(1, -77, np.int32), np.full((1, 2), POISON_FLAG, np.uint8)

    def vis_in(**kw):
        st = VA.SmpcVisibilityIn(B=1, Np=2, on_device=0, world_x=7, world_y=5, world_shared=1, occlusion_min_cost=254, resolution=1.0,
                                 max_range=10.0, world=_ptr(world), world_origin=_ptr(origin), robot_pose=_ptr(pose), people=_ptr(people),
                                 count=_ptr(count))
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    INVALID, UNSUPPORTED = "(-1)", "(-2)"
    nan, inf = float("nan"), float("inf")
    cases = [(dict(B=-1), INVALID), (dict(Np=0), INVALID), (dict(Np=-4), INVALID), (dict(world_x=0), INVALID), (dict(world_y=-1), INVALID),
             (dict(resolution=0.0), INVALID), (dict(resolution=-1.0), INVALID), (dict(resolution=nan), INVALID), (dict(resolution=inf), INVALID),
             (dict(max_range=0.0), INVALID), (dict(max_range=-2.0), INVALID), (dict(max_range=nan), INVALID), (dict(max_range=inf), INVALID),
             (dict(world=None), INVALID), (dict(world_origin=None), INVALID), (dict(robot_pose=None), INVALID), (dict(people=None), INVALID),
             (dict(count=None), INVALID), (dict(max_range=float(np.nextafter(32768.0, inf))), UNSUPPORTED),
             (dict(max_range=10.0, resolution=1e-4), UNSUPPORTED), (dict(world_x=2 ** 16, world_y=2 ** 15), UNSUPPORTED)]
    for kw, code in cases:
        with pytest.raises(SmpcError, match=re.escape(code)):
            solver._call("smpc_visible_people_batch", vis_in(**kw), _ptr(vis), _ptr(n), _ptr(seen))
    for args in ((None, _ptr(n), _ptr(seen)), (_ptr(vis), None, _ptr(seen))):
        with pytest.raises(SmpcError, match=re.escape(INVALID)):
            solver._call("smpc_visible_people_batch", vis_in(), *args)
    assert solver.lib.smpc_visible_people_batch(None, vis_in(), _ptr(vis), _ptr(n), _ptr(seen)) == -1        # NULL handle
    assert solver.lib.smpc_visible_people_batch(solver._h, None, _ptr(vis), _ptr(n), _ptr(seen)) == -1       # NULL struct
    assert (vis == POISON_ROW).all() and n[0] == -77 and (seen == POISON_FLAG).all()
    # the library's bound is the package's, and the accepted side of it runs; an empty batch is no refusal
    assert VisibilityParams(max_range=32768.0).supported(1.0) and not VisibilityParams(max_range=10.0).supported(1e-4)
    solver._call("smpc_visible_people_batch", vis_in(max_range=32768.0), _ptr(vis), _ptr(n), _ptr(seen))
    assert n[0] == 2 and seen.tolist() == [[V.SEEN, V.SEEN]] and V.same_bits(vis, people)
    solver._call("smpc_visible_people_batch", vis_in(B=0), _ptr(vis), _ptr(n), _ptr(seen))
