"""smpc_goal_field_batch and smpc_extract_plan_batch on the GPU against tests/global_plan_ref.py, bit for bit: fields on
worlds from one cell to 256 x 192, a serpentine whose longest path has some 1,400 cells, pockets and bad goals, shared
and per-goal worlds, host and device pointers, refusals that leave poisoned outputs alone, and plans of every stride,
length and error code. The reference fields are computed once per module and shared."""
import numpy as np
import pytest

import global_plan_ref as R
from nav2_social_mpc_controller_amd import _abi_global_plan as GA
from nav2_social_mpc_controller_amd.params import GlobalPlanParams, OptimizerParams

pytestmark = pytest.mark.gpu
U = R.UNREACHABLE


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


def cost_of(gp):
    return R.Cost(gp.neutral_cost, gp.cost_weight, gp.lethal_min_cost, gp.allow_unknown)


def check_fields(solver, gp, world, origin, res, goals):
    field, status = solver.goal_field(gp, world, origin, res, goals)
    want, want_status = R.goal_fields(world, origin, res, goals, cost_of(gp))
    assert field.dtype == np.uint32 and np.array_equal(status, want_status), (status, want_status)
    assert R.same_bits(field, want), np.argwhere(field != want)[:5]
    return field, status


# ---- fields ----------------------------------------------------------------------------------------------------------------
PARAMS = [GlobalPlanParams(), GlobalPlanParams(allow_unknown=True), GlobalPlanParams(cost_weight=0), GlobalPlanParams(7, 3, 200, True)]


@pytest.mark.parametrize("Hx,Hy", [(1, 1), (1, 9), (9, 1), (7, 5), (33, 34)])
def test_small_worlds_every_cell_as_goal_region(solver, Hx, Hy):
    g = np.random.default_rng(Hx * 100 + Hy)
    origin, res = np.array([-0.3, 1.7]), 0.25
    for gp in PARAMS:
        world = g.choice(np.array([0, 0, 0, 0, 30, 120, 252, 253, 254, 255], np.uint8), (Hy, Hx))
        world[g.integers(Hy), g.integers(Hx)] = 0
        # goals anywhere on and around the world: free cells, lethal cells, off the world, not finite
        goals = np.concatenate([origin + g.uniform(-0.3, 1.0, (12, 2)) * np.array([Hx, Hy]) * res + 0.01, [[np.nan, 2.0], [0.0, np.inf]]])
        _, status = check_fields(solver, gp, world, origin, res, goals)
        assert (status[-2:] == 1).all()
    free = np.zeros((Hy, Hx), np.uint8)
    _, status = check_fields(solver, GlobalPlanParams(), free, origin, res, [R.centre_of((Hx - 1, Hy - 1), origin, res), origin - 1.0])
    assert list(status) == [0, 1]


@pytest.fixture(scope="module")
def floor61():
    from nav2_social_mpc_controller_amd.scenes import make_world
    return make_world(61, 47, 0.05, seed=0x5EED0004, origin=(0.4, -0.7))


@pytest.fixture(scope="module")
def floor256():
    """The 256 x 192 floor with 6 goals and their reference fields (0.43 s each): shared by the field and the plan tests."""
    from nav2_social_mpc_controller_amd.scenes import make_world, world_goals
    w = make_world(256, 192, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15))
    goals = world_goals(w, np.tile(w.origin + 0.5, (6, 1)), min_dist=0.0)
    fields, status = R.goal_fields(w.map, w.origin, w.resolution, goals)
    assert (status == 0).all() and len(np.unique(goals, axis=0)) == 6
    return dict(world=w, goals=goals, fields=fields)


def test_floor_61_x_47_with_67_goals_on_one_shared_world(solver, floor61):
    w = floor61
    g = np.random.default_rng(61)
    goals = w.origin + g.uniform(-0.1, 1.1, (67, 2)) * np.array([61, 47]) * w.resolution
    _, status = check_fields(solver, GlobalPlanParams(), w.map, w.origin, w.resolution, goals)
    assert set(status) == {0, 1, 2}      # free goals, goals off the world and goals on lethal cells are all among them


def test_floor_256_x_192_with_6_goals(solver, floor256):
    w = floor256["world"]
    field, status = solver.goal_field(GlobalPlanParams(), w.map, w.origin, w.resolution, floor256["goals"])
    assert not status.any() and R.same_bits(field, floor256["fields"])
    assert ((field != U) == R.passable(w.map, R.Cost())[None]).all()      # the floor is connected: every passable cell is reached


def serpentine():
    """64 x 48: every odd row is lethal except a one-cell gap that alternates between x = 62 and x = 1, inside a lethal
    border; the even rows 2 .. 46 are 23 corridors of 62 cells joined end to end."""
    world = np.zeros((48, 64), np.uint8)
    for k, y in enumerate(range(1, 48, 2)):
        world[y, :] = 254
        world[y, 62 if k % 2 == 0 else 1] = 0
    world[0, :] = world[-1, :] = 254
    world[:, 0] = world[:, -1] = 254
    return world


def test_serpentine_relaxes_to_the_end_of_a_1400_cell_path(solver):
    world = serpentine()
    origin, res = np.array([0.0, 0.0]), 0.1
    goal = R.centre_of((30, 46), origin, res)                 # the last corridor
    field, status = check_fields(solver, GlobalPlanParams(), world, origin, res, [goal])
    assert status[0] == 0
    start = (62, 2)                                           # the far end of the first corridor (row 3 opens at x = 1)
    cells, err = R.walk(world, field[0], start)
    assert err == 0 and len(cells) > 1300                     # far more than the world has tiles
    assert ((field[0] != U) == (world == 0)).all()


def test_pockets_and_bad_goals_leave_the_marker(solver):
    world = np.zeros((40, 70), np.uint8)
    world[10:20, 30:40] = 254
    world[12:18, 32:38] = 0                                   # a pocket that spans a tile edge (x = 32)
    origin, res = np.array([1.0, 2.0]), 0.5
    goals = [R.centre_of((2, 2), origin, res), R.centre_of((34, 14), origin, res), R.centre_of((31, 11), origin, res), [0.0, 0.0], [1e12, 3.0]]
    field, status = check_fields(solver, GlobalPlanParams(), world, origin, res, goals)
    assert list(status) == [0, 0, 2, 1, 1]
    assert (field[0, 12:18, 32:38] == U).all() and (field[1] != U).sum() == 36 and (field[2:] == U).all()


def test_three_goals_with_a_world_each(solver):
    g = np.random.default_rng(3)
    worlds = g.choice(np.array([0, 0, 0, 0, 0, 60, 200, 254, 255], np.uint8), (3, 37, 45))
    origins = np.array([[0.0, 0.0], [-5.5, 2.25], [1e3, -1e3]])
    goals = origins + np.array([[3.3, 4.4], [8.1, 2.2], [5.05, 9.0]])
    for gp in (GlobalPlanParams(), GlobalPlanParams(allow_unknown=True)):
        _, status = check_fields(solver, gp, worlds, origins, 0.25, goals)
    assert len({w.tobytes() for w in worlds}) == 3


def test_device_pointers_give_the_host_pointers_fields_and_plans(solver, floor61):
    import torch
    from nav2_social_mpc_controller_amd.solver import BatchSolver, point
    w, gp = floor61, GlobalPlanParams(max_poses=64, stride=2)
    g = np.random.default_rng(7)
    goals = w.origin + g.uniform(0.1, 0.9, (5, 2)) * np.array([61, 47]) * w.resolution
    pose = np.concatenate([w.origin + g.uniform(0.0, 1.0, (40, 2)) * np.array([61, 47]) * w.resolution, np.zeros((40, 1))], axis=1)
    rg = g.integers(0, 5, 40).astype(np.int32)
    field, status = solver.goal_field(gp, w.map, w.origin, w.resolution, goals)
    plan, plan_len, error = solver.extract_plan(gp, w.map, w.origin, w.resolution, field, goals, rg, pose)
    dev = "cuda:0"
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(world=w.map, world_origin=w.origin.reshape(1, 2), goal=goals, robot_goal=rg, pose=pose).items()}
    d_field = torch.full((5, 47, 61), -7, dtype=torch.int32, device=dev)
    d_status = torch.full((5,), -7, dtype=torch.int32, device=dev)
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    gf = point(BatchSolver.goal_field_c(gp, 5, 61, 47, True, w.resolution, 1), {k: t[k] for k in ("world", "world_origin", "goal")})
    solver.goal_field_device(gf, d_field.data_ptr(), d_status.data_ptr())
    d_plan = torch.full((40, 64, 2), float("nan"), dtype=torch.float64, device=dev)
    d_len = torch.full((40,), -7, dtype=torch.int32, device=dev)
    d_err = torch.full((40,), -7, dtype=torch.int32, device=dev)
    ep = point(BatchSolver.extract_plan_c(gp, 40, 5, 61, 47, True, w.resolution, 1), dict(t, field=d_field))
    solver.extract_plan_device(ep, d_plan.data_ptr(), d_len.data_ptr(), d_err.data_ptr())
    torch.cuda.synchronize()
    solver.set_stream(0)
    assert R.same_bits(d_field.cpu().numpy().view(np.uint32), field) and np.array_equal(d_status.cpu().numpy(), status)
    assert R.same_bits(d_plan.cpu().numpy(), plan) and np.array_equal(d_len.cpu().numpy(), plan_len) and np.array_equal(d_err.cpu().numpy(), error)
    assert (error == 0).any() and (plan_len > 2).any()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_poisoned_outputs_alone(solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError, _ptr
    world = np.zeros((5, 7), np.uint8)
    origin, goal = np.zeros((1, 2)), np.array([[0.5, 0.5]])
    field = np.full((1, 5, 7), 0xDEADBEEF, np.uint32)
    status = np.full(1, -77, np.int32)
    pose, rg = np.array([[3.5, 3.5, 0.0]]), np.zeros(1, np.int32)
    plan, plan_len, error = np.full((1, 8, 2), -3.25), np.full(1, -77, np.int32), np.full(1, -77, np.int32)
    good_field = np.zeros((1, 5, 7), np.uint32)

    def field_in(**kw):
        st = GA.SmpcGoalFieldIn(G=1, on_device=0, world_x=7, world_y=5, world_shared=1, resolution=1.0, world=_ptr(world),
                                world_origin=_ptr(origin), goal=_ptr(goal))
        st.cost.neutral_cost, st.cost.cost_weight, st.cost.lethal_min_cost = 50, 1, 253
        for k, v in kw.items():
            setattr(st.cost if hasattr(st.cost, k) else st, k, v)
        return st

    def plan_in(**kw):
        st = GA.SmpcExtractPlanIn(B=1, G=1, L=8, stride=1, on_device=0, world_x=7, world_y=5, world_shared=1, resolution=1.0,
                                  world=_ptr(world), world_origin=_ptr(origin), field=_ptr(good_field), goal=_ptr(goal),
                                  robot_goal=_ptr(rg), pose=_ptr(pose))
        st.cost.neutral_cost, st.cost.cost_weight, st.cost.lethal_min_cost = 50, 1, 253
        for k, v in kw.items():
            setattr(st.cost if hasattr(st.cost, k) else st, k, v)
        return st

    INVALID, UNSUPPORTED = "(-1)", "(-2)"
    common = [(dict(world_x=0), INVALID), (dict(world_y=-1), INVALID), (dict(resolution=0.0), INVALID), (dict(resolution=float("nan")), INVALID),
              (dict(resolution=float("inf")), INVALID), (dict(neutral_cost=0), INVALID), (dict(cost_weight=-1), INVALID),
              (dict(neutral_cost=2, cost_weight=257), INVALID), (dict(world=None), INVALID), (dict(world_origin=None), INVALID),
              (dict(goal=None), INVALID), (dict(world_x=2 ** 16, world_y=2 ** 15), UNSUPPORTED),
              (dict(world_x=1419, world_y=1419), UNSUPPORTED), (dict(world_x=2011695, world_y=1), UNSUPPORTED)]
    for kw, code in common + [(dict(G=-1), INVALID)]:
        with pytest.raises(SmpcError, match=re_escape(code)):
            solver._call("smpc_goal_field_batch", field_in(**kw), _ptr(field), _ptr(status))
    with pytest.raises(SmpcError, match=re_escape(INVALID)):
        solver._call("smpc_goal_field_batch", field_in(), None, _ptr(status))
    for kw, code in common + [(dict(B=-1), INVALID), (dict(G=-1), INVALID), (dict(L=1), INVALID), (dict(stride=0), INVALID),
                              (dict(field=None), INVALID), (dict(robot_goal=None), INVALID), (dict(pose=None), INVALID)]:
        with pytest.raises(SmpcError, match=re_escape(code)):
            solver._call("smpc_extract_plan_batch", plan_in(**kw), _ptr(plan), _ptr(plan_len), _ptr(error))
    for args in ((None, _ptr(plan_len), _ptr(error)), (_ptr(plan), None, _ptr(error))):
        with pytest.raises(SmpcError, match=re_escape(INVALID)):
            solver._call("smpc_extract_plan_batch", plan_in(), *args)
    assert (field == 0xDEADBEEF).all() and status[0] == -77 and (plan == -3.25).all() and plan_len[0] == -77 and error[0] == -77
    # the library's bound is the package's, and the accepted side of it runs: NULL status and NULL error are legal
    gp = GlobalPlanParams()
    assert gp.world_supported(1418, 1418) and not gp.world_supported(1419, 1419) and gp.world_supported(1024, 1024)
    solver._call("smpc_goal_field_batch", field_in(), _ptr(field), None)
    assert R.same_bits(field, R.goal_fields(world, origin[0], 1.0, goal)[0]) and status[0] == -77
    solver._call("smpc_extract_plan_batch", plan_in(field=_ptr(field)), _ptr(plan), _ptr(plan_len), None)
    assert plan_len[0] == 4 and error[0] == -77 and (plan[0, 4:] == -3.25).all()   # three diagonal steps: pose, c1, c2, goal
    # empty batches are no refusal
    solver._call("smpc_goal_field_batch", field_in(G=0), _ptr(field), _ptr(status))
    solver._call("smpc_extract_plan_batch", plan_in(B=0), _ptr(plan), _ptr(plan_len), _ptr(error))


def re_escape(code):
    import re
    return re.escape(code)


def test_1024_x_1024_is_accepted_at_the_defaults(solver):
    """The size the overflow bound is computed for (tests/test_global_plan.py): an empty floor, whose field is known in
    closed form: max(dx, dy) steps of which min(dx, dy) are diagonal."""
    world = np.zeros((1024, 1024), np.uint8)
    origin = np.array([0.0, 0.0])
    field, status = solver.goal_field(GlobalPlanParams(), world, origin, 1.0, [[700.5, 300.5]])
    yy, xx = np.mgrid[0:1024, 0:1024]
    dx, dy = np.abs(xx - 700), np.abs(yy - 300)
    want = (7 * 50 * np.minimum(dx, dy) + 5 * 50 * (np.maximum(dx, dy) - np.minimum(dx, dy))).astype(np.uint32)
    assert status[0] == 0 and R.same_bits(field[0], want)


def test_a_world_of_more_tiles_than_dirty_flags(solver):
    """One row of 600,000 cells is 18,750 tiles of 32 x 32, more than the kernel's 16,384 dirty flags: two tiles share a
    flag. Weight 1 everywhere (the overflow bound admits 600,000 cells only with small weights), one lethal cell: 5 per
    step up to it, the marker from it on."""
    world = np.zeros((1, 600000), np.uint8)
    world[0, 500000] = 254
    gp = GlobalPlanParams(neutral_cost=1, cost_weight=0)
    assert gp.world_supported(600000, 1) and not GlobalPlanParams().world_supported(600000, 4)
    field, status = solver.goal_field(gp, world, [0.0, 0.0], 1.0, [[100.5, 0.5]])
    want = (5 * np.abs(np.arange(600000, dtype=np.int64) - 100)).astype(np.uint32)
    want[500000:] = U
    assert status[0] == 0 and R.same_bits(field[0, 0], want)


# ---- plans -----------------------------------------------------------------------------------------------------------------
def plan_properties(world, origin, res, field, goal, pose_xy, rows, cost=R.Cost()):
    """From a complete stride-1 plan alone: its cells are a chain of allowed steps whose costs add up to field[start]."""
    Hy, Hx = world.shape
    cells = [R.cell_of(p, origin, res, Hx, Hy) for p in rows]
    assert None not in cells and R.same_bits(rows[0], pose_xy) and R.same_bits(rows[-1], goal)
    w = R.weights(world, cost)
    total = 0
    if len(rows) == 2:                       # [pose, goal]: the same cell, or one step
        chain = cells if cells[0] != cells[1] else cells[:1]
    else:
        chain = cells
        for c, row in zip(cells[1:-1], rows[1:-1]):
            assert R.same_bits(row, R.centre_of(c, origin, res))
    for (x, y), (nx, ny) in zip(chain[:-1], chain[1:]):
        dx, dy = nx - x, ny - y
        assert max(abs(dx), abs(dy)) == 1 and w[ny, nx] != 0 and w[y, x] != 0, ((x, y), (nx, ny))
        if dx and dy:
            assert w[y, nx] != 0 and w[ny, x] != 0, ((x, y), (nx, ny))
        total += (7 if dx and dy else 5) * int(w[ny, nx])
    assert total == int(field[cells[0][1], cells[0][0]])
    return len(chain)


def poses_on(w, n, seed):
    g = np.random.default_rng(seed)
    xy = w.origin + g.uniform(0.02, 0.98, (n, 2)) * np.array([w.cells_x, w.cells_y]) * w.resolution
    return np.concatenate([xy, g.uniform(-3, 3, (n, 1))], axis=1)


@pytest.mark.parametrize("stride", [1, 3, 50])
def test_67_robots_over_6_fields(solver, floor256, stride):
    w, goals, fields = floor256["world"], floor256["goals"], floor256["fields"]
    pose = poses_on(w, 67, 67)
    rg = (np.arange(67) % 6).astype(np.int32)
    gp = GlobalPlanParams(max_poses=400 if stride == 1 else 120, stride=stride)
    poison = np.random.default_rng(1).uniform(-9, 9, (67, gp.max_poses, 2))
    cells = []
    want = R.extract_plan(w.map, w.origin, w.resolution, fields, goals, rg, pose, gp.max_poses, stride, plan=poison, cells_out=cells)
    got = solver.extract_plan(gp, w.map, w.origin, w.resolution, fields, goals, rg, pose, plan=poison)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1])
    assert R.same_bits(got[0], want[0])                       # the rows beyond plan_len are the poison, bit for bit
    assert (want[2] == R.OK).sum() > 30 and want[1].max() > (150 if stride == 1 else 5)
    if stride == 1:
        for b in np.flatnonzero(want[2] == R.OK):
            n = plan_properties(w.map, w.origin, w.resolution, fields[rg[b]], goals[rg[b]], pose[b, :2], got[0][b, :got[1][b]])
            assert n == len(cells[b])


def test_truncation_at_below_and_far_below_a_plans_length(solver, floor256):
    w, goals, fields = floor256["world"], floor256["goals"], floor256["fields"]
    pose = poses_on(w, 67, 67)
    full = R.extract_plan(w.map, w.origin, w.resolution, fields[:1], goals[:1], np.zeros(67, np.int32), pose, 400)
    b = int(np.argmax(np.where(full[2] == R.OK, full[1], 0)))
    n = int(full[1][b])
    assert n > 40
    for L, err in ((n, R.OK), (n - 1, R.TRUNCATED), (2, R.TRUNCATED), (n + 1, R.OK)):
        gp = GlobalPlanParams(max_poses=L)
        poison = np.full((1, L, 2), 1234.5)
        plan, plan_len, error = solver.extract_plan(gp, w.map, w.origin, w.resolution, fields[:1], goals[:1], [0], pose[b:b + 1], plan=poison)
        want = R.extract_plan(w.map, w.origin, w.resolution, fields[:1], goals[:1], [0], pose[b:b + 1], L, plan=poison)
        assert error[0] == err == want[2][0] and plan_len[0] == min(n, L) == want[1][0] and R.same_bits(plan, want[0])
        if err == R.TRUNCATED:
            assert R.same_bits(plan[0], full[0][b, :L])       # the first L rows of the whole plan: the goal point is not among them


def test_every_error_code_and_a_start_on_the_goal_cell(solver, floor61):
    w = floor61
    cost = R.Cost()
    free = np.argwhere(w.map == 0)
    lethal = np.argwhere(w.map >= 253)
    goal = R.centre_of(free[len(free) // 2][::-1], w.origin, w.resolution)
    world = w.map.copy()
    py, px = free[5]
    world[max(py - 2, 0):py + 3, max(px - 2, 0):px + 3] = 254
    world[py, px] = 0                                         # a pocket around free[5]
    fields, status = R.goal_fields(world, w.origin, w.resolution, [goal, [np.nan, 0.0]])
    assert list(status) == [0, 1]
    far = np.argwhere(fields[0] == fields[0][fields[0] != U].max())[0]
    start = (int(far[1]), int(far[0]))                        # the reachable cell farthest from the goal
    path, _ = R.walk(world, fields[0], start)
    assert len(path) > 12
    # A host-built field with raised cells: every cell of a band of potentials wider than the dearest step (7 * 305) is one
    # too high, so whatever way the walk from `start` takes, after a few good steps it stands above the band and no
    # neighbour satisfies the equality.
    lo = int(fields[0][path[-4][1], path[-4][0]])
    band = (fields[0] >= lo) & (fields[0] < lo + 2200)
    assert int(fields[0][start[1], start[0]]) > lo + 2200 + 1000
    raised = np.where(band, fields[0] + 1, fields[0]).astype(np.uint32)
    fields = np.stack([fields[0], fields[1], raised])
    goals = np.array([goal, [np.nan, 0.0], goal])
    c = lambda cell: R.centre_of(cell, w.origin, w.resolution)
    pose = np.array([c(start), c(start), c((px, py)), c(lethal[0][::-1]), w.origin - 0.01, [np.inf, 0.0], c(start), c(start), c(start),
                     goal + 0.01, c(start)])
    rg = np.array([0, 1, 0, 0, 0, 0, 6, -1, 2, 0, 0], np.int32)
    pose = np.concatenate([pose, np.zeros((len(pose), 1))], axis=1)
    L = len(path) - 3
    gp = GlobalPlanParams(max_poses=L)
    poison = np.full((len(pose), L, 2), -8.125)
    want = R.extract_plan(world, w.origin, w.resolution, fields, goals, rg, pose, L, plan=poison)
    got = solver.extract_plan(gp, world, w.origin, w.resolution, fields, goals, rg, pose, plan=poison)
    assert list(want[2]) == [R.TRUNCATED, R.UNREACHABLE_START, R.UNREACHABLE_START, R.START_BLOCKED, R.START_OUTSIDE, R.START_OUTSIDE,
                             R.BAD_GOAL_INDEX, R.BAD_GOAL_INDEX, R.INCONSISTENT_FIELD, R.OK, R.TRUNCATED]
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]) and R.same_bits(got[0], want[0])
    assert list(got[1]) == [L, 0, 0, 0, 0, 0, 0, 0, 0, 2, L]
    assert (got[0][[1, 2, 3, 4, 5, 6, 7, 8]] == -8.125).all()  # an error other than TRUNCATED: no row of the robot is written
    assert R.same_bits(got[0][9, :2], np.array([goal + 0.01, goal]))


def test_130_robots_over_3_worlds_and_each_row_alone(solver):
    g = np.random.default_rng(130)
    worlds = g.choice(np.array([0, 0, 0, 0, 0, 0, 60, 200, 254, 255], np.uint8), (3, 47, 61))
    origins = np.array([[0.0, 0.0], [-5.5, 2.25], [40.0, -30.0]])
    goals = origins + np.array([[3.3, 4.4], [8.1, 2.2], [5.05, 9.0]])
    gp = GlobalPlanParams(allow_unknown=True, max_poses=90, stride=3)
    fields, status = solver.goal_field(gp, worlds, origins, 0.25, goals)
    assert R.same_bits(fields, R.goal_fields(worlds, origins, 0.25, goals, cost_of(gp))[0]) and not status.any()
    rg = g.integers(0, 3, 130).astype(np.int32)
    pose = np.concatenate([origins[rg] + g.uniform(-0.2, 1.0, (130, 2)) * np.array([61, 47]) * 0.25, np.zeros((130, 1))], axis=1)
    poison = g.uniform(-9, 9, (130, 90, 2))
    want = R.extract_plan(worlds, origins, 0.25, fields, goals, rg, pose, 90, 3, cost_of(gp), plan=poison)
    got = solver.extract_plan(gp, worlds, origins, 0.25, fields, goals, rg, pose, plan=poison)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]) and R.same_bits(got[0], want[0])
    assert {R.OK, R.START_OUTSIDE, R.START_BLOCKED} <= set(want[2])
    for b in (0, 7, 64, 129):                                # a robot's outputs do not depend on the batch around it
        one = solver.extract_plan(gp, worlds, origins, 0.25, fields, goals, rg[b:b + 1], pose[b:b + 1], plan=poison[b:b + 1])
        assert R.same_bits(one[0][0], got[0][b]) and one[1][0] == got[1][b] and one[2][0] == got[2][b]


def test_one_robot_one_goal(solver):
    world = np.zeros((1, 12), np.uint8)
    goal = np.array([[11.25, 0.75]])
    field, _ = solver.goal_field(GlobalPlanParams(), world, [0.0, 0.0], 1.0, goal)
    for stride, L in ((1, 16), (5, 16), (11, 16), (1, 12), (1, 11), (1, 2)):
        gp = GlobalPlanParams(max_poses=L, stride=stride)
        got = solver.extract_plan(gp, world, [0.0, 0.0], 1.0, field, goal, [0], [[0.25, 0.5, 1.0]])
        want = R.extract_plan(world, [0.0, 0.0], 1.0, field, goal, [0], [[0.25, 0.5, 1.0]], L, stride)
        assert R.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (stride, L)
