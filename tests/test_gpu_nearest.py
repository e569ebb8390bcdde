"""smpc_nearest_people_batch on the GPU against tests/nearest_ref.py, bit for bit: the smallest tables and grids, robots and
agents in the border bins and outside the grid, the selection at the chunk and merge boundaries of the query's 64 lanes,
ties, the gate at the range, pairs across bin edges and corners, the three forms of `self`, rows that are not finite, and the
invariances the contract states: poison beyond the counts, host against device pointers, a robot alone against its batch,
the same call twice, the same table under two grids. Then the refusals and the workspace query."""
import ctypes as C

import numpy as np
import pytest

import nearest_ref as R
from nav2_social_mpc_controller_amd import _abi
from nav2_social_mpc_controller_amd.params import OptimizerParams

pytestmark = pytest.mark.gpu
POISON_ROW, POISON_SRC = -3.25, -77
UP, DOWN = np.inf, -np.inf


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


def table(xy, seed=0):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    rows = np.zeros((len(xy), 5))
    rows[:, 0:2] = xy
    rows[:, 2:5] = np.arange(3 * len(xy)).reshape(-1, 3) * 0.5 - 7.0 + seed
    return rows


def poses(xy):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    return np.concatenate([xy, np.full((len(xy), 1), 0.3)], axis=1)


def grid_for(max_range, origin=(0.0, 0.0), gx=1, gy=1, factor=1.0):
    return dict(grid_x=gx, grid_y=gy, grid_origin=np.asarray(origin, np.float64),
                bin_size=float(np.float64(max_range) * np.float64(R.MARGIN)) * factor, max_range=float(max_range))


def check(solver, agents, pose, Np, grid, self_row=None):
    """One host-pointer call on poisoned outputs against the reference on the same poison. Returns the device's outputs."""
    B = len(pose)
    poison_p, poison_s = np.full((B, Np, 5), POISON_ROW), np.full((B, Np), POISON_SRC, np.int32)
    people, count, source = solver.nearest_people(agents, pose, Np, self_row=self_row, people=poison_p, source=poison_s, **grid)
    want = R.nearest_people(agents, pose, Np, grid["max_range"], self_row, people=poison_p, source=poison_s)
    assert count.dtype == np.int32 and source.dtype == np.int32
    assert np.array_equal(count, want[1]), (count, want[1])
    assert np.array_equal(source, want[2]), np.argwhere(source != want[2])[:5]
    assert R.same_bits(people, want[0])
    return people, count, source


# ---- the smallest shapes ---------------------------------------------------------------------------------------------------
def test_no_agents_one_agent_that_is_the_robot_and_one_robot(solver):
    g = grid_for(2.0, gx=3, gy=2)
    _, count, _ = check(solver, np.zeros((0, 5)), poses([[1.0, 1.0], [50.0, -3.0]]), 4, g)
    assert count.tolist() == [0, 0]
    one = table([[1.0, 1.0]])
    _, count, _ = check(solver, one, poses([[1.0, 1.0]]), 4, g, np.array([0], np.int32))
    assert count.tolist() == [0]
    _, count, source = check(solver, one, poses([[1.0, 1.0]]), 4, g, np.array([-1], np.int32))
    assert count.tolist() == [1] and source[0, 0] == 0
    _, count, _ = check(solver, one, poses([[1.0, 1.0]]), 1, g)
    assert count.tolist() == [1]
    assert solver.nearest_people(one, np.zeros((0, 3)), 4, **g)[1].shape == (0,)                # B == 0 succeeds


@pytest.mark.parametrize("gx,gy", [(1, 1), (1, 7), (7, 1), (5, 4)])
def test_border_bins_corners_and_points_outside_the_grid(solver, gx, gy):
    rng = np.random.default_rng(gx * 10 + gy)
    g = grid_for(1.5, origin=(-2.0, 3.0), gx=gx, gy=gy)
    s = g["bin_size"]
    lo, hi = np.array([-2.0, 3.0]), np.array([-2.0, 3.0]) + np.array([gx, gy]) * s
    # agents all over the floor and around it (they land in the border bins), some far outside
    xy = lo + rng.uniform(-0.6, 1.6, (700, 2)) * (hi - lo)
    xy[:8] = [[1e12, 4.0], [-1e12, 4.0], [0.0, 1e12], [0.0, -1e12], [1e12, 1e12], [-1e12, -1e12], [1e12 + 1.0, 4.0], [0.0, 1e12 + 1.0]]
    agents = table(xy)
    # robots: in each corner bin, on each border, outside on all four sides, beside the far agents
    cx, cy = [lo[0] + 0.3, (lo[0] + hi[0]) / 2, hi[0] - 0.3], [lo[1] + 0.3, (lo[1] + hi[1]) / 2, hi[1] - 0.3]
    robots = [[x, y] for x in cx for y in cy]
    robots += [[lo[0] - 1.0, cy[1]], [hi[0] + 1.0, cy[1]], [cx[1], lo[1] - 1.0], [cx[1], hi[1] + 1.0], [lo[0] - 1.2, lo[1] - 1.2],
               [hi[0] + 1.2, hi[1] + 1.2], [lo[0], lo[1]], [hi[0], hi[1]], [1e12, 4.5], [0.5, -1e12], [1e12, 1e12], [-1e12, 4.0]]
    _, count, _ = check(solver, agents, poses(robots), 8, g)
    assert count[:9].min() >= 1 and count[-4:].tolist() == [2, 1, 1, 1]


# ---- the selection ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [63, 64, 65, 129, 200])
@pytest.mark.parametrize("Np", [1, 8, 64])
def test_chunk_and_merge_boundaries_in_one_neighbourhood(solver, Q, Np):
    """Q qualifying agents around one robot among agents out of range, in the table in an order that is not the distance's;
    a second robot sees exactly Np and a third Np + 1 of them."""
    rng = np.random.default_rng(Q * 100 + Np)
    max_range = 3.0
    ang, rad = rng.uniform(0, 2 * np.pi, Q), np.round(rng.uniform(0.05, 2.95, Q), 2)           # two decimals: ties happen
    near = np.stack([10.0 + rad * np.cos(ang), 10.0 + rad * np.sin(ang)], axis=1)
    ang = rng.uniform(0, 2 * np.pi, 150)
    beyond = np.stack([10.0 + rng.uniform(3.05, 6.0, 150) * np.cos(ang), 10.0 + rng.uniform(3.05, 6.0, 150) * np.sin(ang)], axis=1)
    ring = np.stack([40.0 + 0.04 * np.arange(Np + 1), np.full(Np + 1, 10.0)], axis=1)           # Np + 1 in a row from (40, 10)
    xy = np.concatenate([near, beyond, ring])
    agents = table(xy[rng.permutation(len(xy))])
    exactly = [40.0 + 0.04 * Np - 3.02, 10.0]                                                  # the last of the row is 3.02 away
    robots = poses([[10.0, 10.0], exactly, [40.0 + 0.02 * Np, 10.0]])
    for g in (grid_for(max_range, gx=20, gy=8), grid_for(max_range, gx=1, gy=1), grid_for(max_range, origin=(1.0, 1.0), gx=5, gy=3, factor=3.0)):
        _, count, _ = check(solver, agents, robots, Np, g)
        assert count.tolist() == [min(Np, Q), Np, Np]
    ok, _ = R.qualifying(agents, robots, max_range)
    assert ok.sum(axis=1).tolist() == [Q, Np, Np + 1]


def test_ties_the_gate_at_the_range_and_pairs_across_bin_edges_and_corners(solver):
    four = table([[0.0, 1.0], [1.0, 0.0], [0.0, -1.0], [-1.0, 0.0]])
    for Np in (1, 2, 3, 4, 5):
        _, count, source = check(solver, four, poses([[0.0, 0.0]]), Np, grid_for(2.0, origin=(-0.5, -0.5), gx=2, gy=2))
        assert source[0, :count[0]].tolist() == [0, 1, 2, 3][:Np]
    dup = table([[2.0, 2.0]] * 5 + [[0.5, 0.0]] + [[2.0, 2.0]] * 2)
    _, _, source = check(solver, dup, poses([[0.0, 0.0]]), 4, grid_for(5.0))
    assert source[0].tolist() == [5, 0, 1, 2]
    cut = table([[3.0, 0.0], [0.0, 2.0], [0.1, 0.0], [2.0, 0.0], [0.0, -2.0]])
    _, _, source = check(solver, cut, poses([[0.0, 0.0]]), 3, grid_for(5.0, origin=(-1.0, -1.0), gx=2, gy=2))
    assert source[0].tolist() == [2, 1, 3]
    # the 3-4-5 triangle at exactly the range and one ulp beyond
    tri = table([[4.0, 6.0], [4.0, np.nextafter(6.0, UP)], [np.nextafter(4.0, UP), 6.0], [-2.0, -2.0], [-2.0, np.nextafter(np.nextafter(-2.0, DOWN), DOWN)]])
    _, count, source = check(solver, tri, poses([[1.0, 2.0]]), 5, grid_for(5.0, origin=(0.0, 0.0), gx=3, gy=3))
    assert sorted(source[0, :2].tolist()) == [0, 3] and count[0] == 2
    assert check(solver, tri, poses([[1.0, 2.0]]), 5, grid_for(np.nextafter(5.0, 0.0), gx=3, gy=3))[1].tolist() == [0]
    # robots on, and one ulp beside, bin edges and corners; agents at the range along the axes and the 3-4-5 diagonals
    for origin in ((0.0, 0.0), (0.1, -3.3)):
        g = grid_for(5.0, origin=origin, gx=6, gy=5)
        e = np.asarray(origin) + np.array([2, 3]) * g["bin_size"]
        spots = [e, np.nextafter(e, UP), np.nextafter(e, DOWN), [e[0], e[1] + 1.0], [np.nextafter(e[0], DOWN), e[1] - 2.0]]
        xy = []
        for s in spots:
            for dx, dy in ((5.0, 0.0), (-5.0, 0.0), (0.0, 5.0), (0.0, -5.0), (3.0, 4.0), (-3.0, 4.0), (3.0, -4.0), (-4.0, -3.0)):
                p = np.array([s[0] + dx, s[1] + dy])
                xy += [p, np.nextafter(p, UP), np.nextafter(p, DOWN)]
        _, count, _ = check(solver, table(xy), poses(spots), 64, g)
        assert count.min() >= 8


def test_self_in_three_forms(solver):
    agents = table([[1.0, 1.0], [2.0, 1.0], [1.0, 1.0], [1.0, 1.0]])
    pose = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.5]])
    g = grid_for(3.0, origin=(0.0, 0.0), gx=2, gy=2)
    assert check(solver, agents, pose, 4, g)[2].tolist() == [[0, 2, 3, 1], [0, 2, 3, 1]]                          # NULL
    assert check(solver, agents, pose, 4, g, np.array([-1, -7], np.int32))[2].tolist() == [[0, 2, 3, 1], [0, 2, 3, 1]]
    _, count, source = check(solver, agents, pose, 4, g, np.array([2, 3], np.int32))
    assert source.tolist() == [[0, 3, 1, POISON_SRC], [0, 2, 1, POISON_SRC]] and count.tolist() == [3, 3]


def test_rows_that_are_not_finite_and_more_rows_per_robot_than_agents(solver):
    agents = table([[np.nan, 0.0], [0.0, np.inf], [1e300, 0.0], [0.5, 0.0], [-np.inf, np.nan], [0.0, -1e300], [1e300, 1.0]])
    agents[3, 2:] = [np.nan, -0.0, np.inf]                                                    # velocities are copied, never examined
    pose = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1e300, 0.0, 0.0], [0.2, 0.1, np.nan]])
    people, count, source = check(solver, agents, pose, 64, grid_for(10.0, origin=(-5.0, -5.0), gx=3, gy=3))
    assert count.tolist() == [1, 0, 0, 2, 1] and source[3, :2].tolist() == [2, 6]
    assert (people[1] == POISON_ROW).all() and (people[2] == POISON_ROW).all()                # a robot that is nowhere writes only its count


# ---- the invariances --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def floor():
    """4096 agents and 256 robots on a 256 x 192-cell floor (12.8 m x 9.6 m), and the reference's answer."""
    rng = np.random.default_rng(404)
    size = np.array([12.8, 9.6])
    origin = np.array([-3.2, 1.15])
    agents = rng.uniform(-2.0, 2.0, (4096, 5))
    agents[:, :2] = origin + rng.uniform(-0.05, 1.05, (4096, 2)) * size
    agents[:256, :2] = origin + rng.uniform(0.0, 1.0, (256, 2)) * size                       # the robots' own rows
    pose = np.concatenate([agents[:256, :2], rng.uniform(-3, 3, (256, 1))], axis=1)
    self_row = np.arange(256, dtype=np.int32)
    self_row[::7] = -1
    max_range, Np = 0.3, 8
    g = dict(grid_x=43, grid_y=32, grid_origin=origin, bin_size=float(np.float64(max_range) * np.float64(R.MARGIN)), max_range=max_range)
    want = R.nearest_people(agents, pose, Np, max_range, self_row, people=np.full((256, Np, 5), POISON_ROW),
                            source=np.full((256, Np), POISON_SRC, np.int32))
    return agents, pose, self_row, Np, g, want


def test_random_table_of_4096_agents_and_256_robots(solver, floor):
    agents, pose, self_row, Np, g, want = floor
    people, count, source = check(solver, agents, pose, Np, g, self_row)
    assert count.max() == Np and count.min() < Np                                             # both sides of the cut occur
    again = check(solver, agents, pose, Np, g, self_row)                                       # the same call twice: bitwise equal
    assert R.same_bits(people, again[0]) and np.array_equal(source, again[2])
    wide = dict(g, grid_x=15, grid_y=11, bin_size=3.0 * g["bin_size"])                           # the same table under another grid
    other = check(solver, agents, pose, Np, wide, self_row)
    assert R.same_bits(people, other[0]) and np.array_equal(source, other[2]) and np.array_equal(count, other[1])


def test_a_row_of_130_robots_equals_each_robots_call_alone(solver, floor):
    agents, pose, self_row, Np, g, want = floor
    for b in (0, 1, 63, 64, 129):
        one = solver.nearest_people(agents, pose[b:b + 1], Np, self_row=self_row[b:b + 1], people=np.full((1, Np, 5), POISON_ROW),
                                    source=np.full((1, Np), POISON_SRC, np.int32), **g)
        assert R.same_bits(one[0][0], want[0][b]) and one[1][0] == want[1][b] and np.array_equal(one[2][0], want[2][b])
    part = solver.nearest_people(agents, pose[:130], Np, self_row=self_row[:130], people=np.full((130, Np, 5), POISON_ROW),
                                 source=np.full((130, Np), POISON_SRC, np.int32), **g)
    assert R.same_bits(part[0], want[0][:130]) and np.array_equal(part[1], want[1][:130]) and np.array_equal(part[2], want[2][:130])


def test_device_pointers_equal_host_pointers_with_and_without_source(solver, floor):
    import torch
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point
    agents, pose, self_row, Np, g, want = floor
    B, A = len(pose), len(agents)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d_agents, d_pose, d_self = dev(agents), dev(pose), dev(self_row)
    nbytes = solver.nearest_workspace_bytes(A, g["grid_x"], g["grid_y"])
    assert nbytes == (4 * (2 * 43 * 32 + 1 + A) + 255) // 256 * 256
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")                       # its contents before do not matter
    ni = point(BatchSolver.nearest_c(B, Np, A, g["grid_x"], g["grid_y"], g["grid_origin"], g["bin_size"], g["max_range"], 1),
               {"agents": d_agents, "robot_pose": d_pose, "self": d_self, "workspace": ws})
    ni.workspace_bytes = nbytes
    for with_source in (True, False):
        people, count = dev(np.full((B, Np, 5), POISON_ROW)), dev(np.full(B, -5, np.int32))
        source = dev(np.full((B, Np), POISON_SRC, np.int32))
        solver.nearest_people_device(ni, people.data_ptr(), count.data_ptr(), source.data_ptr() if with_source else 0)
        torch.cuda.synchronize()
        assert R.same_bits(people.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1])
        assert np.array_equal(source.cpu().numpy(), want[2] if with_source else np.full((B, Np), POISON_SRC, np.int32))
    assert solver.last_kernel_ms() > 0.0
    # the workspace after the call: the exclusive prefix sums of the bins' populations, and every finite row once
    words = ws.cpu().numpy().view(np.int32)
    G = g["grid_x"] * g["grid_y"]
    bins = R.bin_axis(agents[:, 1], g["grid_origin"][1], g["bin_size"], g["grid_y"]) * g["grid_x"] \
        + R.bin_axis(agents[:, 0], g["grid_origin"][0], g["bin_size"], g["grid_x"])
    offsets = np.concatenate([[0], np.cumsum(np.bincount(bins, minlength=G))])
    assert np.array_equal(words[:G + 1], offsets) and np.array_equal(words[G + 1:2 * G + 1], offsets[1:])
    rows = words[2 * G + 1:2 * G + 1 + A]
    assert np.array_equal(np.sort(rows), np.arange(A)) and np.array_equal(bins[rows], np.sort(bins))
    # a too-small workspace and a NULL one are refused, nothing is written
    people = dev(np.full((B, Np, 5), POISON_ROW))
    count = dev(np.full(B, -5, np.int32))
    for bad in (nbytes - 1, 0):
        ni.workspace_bytes = bad
        assert solver.lib.smpc_nearest_people_batch(solver._h, C.byref(ni), people.data_ptr(), count.data_ptr(), None) == -1
    ni.workspace_bytes, ni.workspace = nbytes, None
    assert solver.lib.smpc_nearest_people_batch(solver._h, C.byref(ni), people.data_ptr(), count.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (people.cpu().numpy() == POISON_ROW).all() and (count.cpu().numpy() == -5).all()


# ---- the refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_poisoned_buffers_alone_and_the_workspace_query(solver):
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point
    agents, pose = table([[1.0, 1.0], [2.0, 2.0]]), poses([[1.0, 1.5]])
    people, count, source = np.full((1, 4, 5), POISON_ROW), np.full(1, -5, np.int32), np.full((1, 4), POISON_SRC, np.int32)
    self_row = np.array([-1], np.int32)

    def call(handle=True, struct=True, out=(True, True), **change):
        f = dict(B=1, Np=4, A=2, grid_x=2, grid_y=2, origin=[0.0, 0.0], bin_size=3.0, max_range=2.0, agents=agents, robot_pose=pose)
        f.update(change)
        ni = point(BatchSolver.nearest_c(f["B"], f["Np"], f["A"], f["grid_x"], f["grid_y"], f["origin"], f["bin_size"], f["max_range"], 0),
                   {"agents": f["agents"], "robot_pose": f["robot_pose"], "self": self_row})
        return solver.lib.smpc_nearest_people_batch(solver._h if handle else None, C.byref(ni) if struct else None,
                                                    people.ctypes.data if out[0] else None, count.ctypes.data if out[1] else None,
                                                    source.ctypes.data)

    INVALID, UNSUPPORTED = -1, -2
    assert call() == 0 and count[0] == 2 and source[0].tolist() == [0, 1, POISON_SRC, POISON_SRC]
    people[:], count[:], source[:] = POISON_ROW, -5, POISON_SRC
    nan, inf = np.nan, np.inf
    invalid = [dict(handle=False), dict(struct=False), dict(out=(False, True)), dict(out=(True, False)), dict(robot_pose=None),
               dict(agents=None), dict(B=-1), dict(A=-1), dict(Np=0), dict(Np=-3), dict(grid_x=0), dict(grid_y=0), dict(grid_y=-2),
               dict(origin=[nan, 0.0]), dict(origin=[0.0, inf]), dict(origin=[-inf, 0.0]),
               dict(bin_size=nan), dict(bin_size=inf), dict(bin_size=0.0), dict(bin_size=-3.0),
               dict(max_range=nan), dict(max_range=inf), dict(max_range=0.0), dict(max_range=-2.0),
               dict(bin_size=2.0), dict(bin_size=np.nextafter(2.0 * R.MARGIN, 0.0))]
    for change in invalid:
        assert call(**change) == INVALID, change
    unsupported = [dict(Np=_abi.SMPC_MAX_AGENTS + 1), dict(grid_x=257, grid_y=256), dict(grid_x=65537, grid_y=1), dict(A=2 ** 24 + 1)]
    for change in unsupported:
        assert call(**change) == UNSUPPORTED, change
    assert (people == POISON_ROW).all() and (count == -5).all() and (source == POISON_SRC).all()
    assert call(bin_size=2.0 * R.MARGIN) == 0 and call(agents=None, A=0) == 0 and call(grid_x=256, grid_y=256, bin_size=2.5) == 0
    assert call(B=0) == 0 and call(Np=_abi.SMPC_MAX_AGENTS, out=(True, True), B=0) == 0
    # the workspace query: 4 * (2 G + 1 + A) rounded up to 256; 0 for what the call refuses
    assert solver.nearest_workspace_bytes(0, 1, 1) == 256 and solver.nearest_workspace_bytes(70000, 40, 40) == (4 * (3201 + 70000) + 255) // 256 * 256
    assert solver.nearest_workspace_bytes(2 ** 24, 256, 256) == (4 * (2 * 65536 + 1 + 2 ** 24) + 255) // 256 * 256
    for bad in ((-1, 1, 1), (1, 0, 1), (1, 1, 0), (1, 257, 256), (2 ** 24 + 1, 1, 1)):
        assert solver.nearest_workspace_bytes(*bad) == 0
