"""smpc_crowd_pool_step_batch on the GPU against tests/crowd_pool_ref.py within crowd_ref.TOL (every case asserts that its
own bound, partners * 2^-36 * dt, is at most TOL / 2): the smallest tables, standing and coincident pairs, inert rows, a
static partner, the gate at the range, bin edges and corners, small grids and points outside them, the population edges of
the candidate chunks, the tiles and the whole table in one bin, waypoints, the obstacle grid, a dense floor and twelve
chained steps; then what the contract promises bit for bit (grids, permutations, repetition, bins_ready, memory spaces, a
mover alone), the private crowd kernel as a cross-check, and the refusals. The seeded inputs are tests/crowd_pool_cases.py's,
which tests/test_crowd_pool.py shows to stay clear of every decision the rules take."""
import ctypes as C

import numpy as np
import pytest

import crowd_pool_cases as PC
import crowd_pool_ref as P
import crowd_ref as R
from nav2_social_mpc_controller_amd.params import CrowdParams, OptimizerParams, PoolCrowdParams

pytestmark = pytest.mark.gpu
POISON = -3.25


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def call(solver, c, agents=None, cursor=None, M=None, grid=None, rows=None, next=None):
    """One host-pointer call of a case (optionally another table / cursors / fewer movers / another grid / the movers `rows`
    of the per-mover arrays) on a poisoned `next`."""
    agents = c["agents"] if agents is None else agents
    M = c["M"] if M is None else M
    rows = np.arange(M) if rows is None else np.asarray(rows)
    pick = lambda a: None if a is None else np.ascontiguousarray(a[rows])
    kw = {}
    if c["od"] is not None:
        kw = dict(od_indexes=c["od"][0], od_origin=c["od"][1], od_resolution=c["od"][2])
    return solver.crowd_pool_step(PoolCrowdParams(interaction_range=c["range"], **c["params"]), c["dt"], agents, M,
                                  pick(c["cursor"]) if cursor is None else cursor, pick(c["waypoints"]), pick(c["n_waypoints"]),
                                  desired_speeds=pick(c["speeds"]), next=np.full((M, 5), POISON) if next is None else next,
                                  **(grid or c["grid"]), **kw)


def custom(agents, M, rng=5.0, grid=None, dt=0.1, waypoints=None, n_waypoints=None, cursor=None, speeds=None, od=None, **params):
    """a hand-made case: no waypoints unless given"""
    agents = np.ascontiguousarray(agents, np.float64).reshape(-1, 5)
    return dict(agents=agents, M=M, cursor=np.zeros(M, np.int32) if cursor is None else np.asarray(cursor, np.int32),
                waypoints=np.zeros((M, 1, 2)) if waypoints is None else np.asarray(waypoints, np.float64),
                n_waypoints=np.zeros(M, np.int32) if n_waypoints is None else np.asarray(n_waypoints, np.int32), speeds=speeds, dt=dt,
                range=float(rng), params={**PC.PARAMS, **params}, od=od, grid=grid or PC.grid_for(rng, (-20.0, -20.0), 9, 9))


def check(solver, c, what, grid=None):
    """the device on a poisoned `next` against the checker on the same poison; returns the device's (next, cursor)"""
    counts = []
    want, want_cur = PC.ref_step(c, next=np.full((c["M"], 5), POISON), counts=counts)
    got, got_cur = call(solver, c, grid=grid)
    assert got_cur.dtype == np.int32 and got.shape == (c["M"], 5)
    P.compare(got, got_cur, want, want_cur, c["dt"], max(counts, default=0), what)
    return got, got_cur


# ---- the seeded cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in PC.CASES if n != "chain"])
def test_seeded_case_against_the_checker(solver, name):
    c = PC.case(name)
    want, want_cur, partners = PC.reference(name, POISON)
    got, got_cur = call(solver, c)
    P.compare(got, got_cur, want, want_cur, c["dt"], partners, name)
    if name.startswith("waypoints"):
        moved = got_cur != c["cursor"]
        assert moved.sum() >= 3 and (got_cur[moved] == 0).any() == bool(c["params"]["cyclic"])   # arrivals, and wraps when cyclic


def test_twelve_chained_steps_from_the_devices_own_states(solver):
    c = PC.case("chain")
    agents, cursor = c["agents"].copy(), c["cursor"].copy()
    for k in range(12):
        counts = []
        want, want_cur = PC.ref_step(c, agents, cursor, counts=counts)
        got, got_cur = call(solver, c, agents=agents, cursor=cursor)
        P.compare(got, got_cur, want, want_cur, c["dt"], max(counts), f"chain step {k}")
        agents[:c["M"]], cursor = got, got_cur


# ---- the smallest tables and the hand-made ones ------------------------------------------------------------------------------
def test_no_movers_and_one_mover_alone(solver):
    robots = np.array([[0.0, 0.0, 0.3, 0.0, 0.0], [1.0, 1.0, 0.0, 0.2, 0.0], [2.0, 0.0, 0.0, 0.0, 0.1]])
    nxt, cur = call(solver, custom(robots, 0))
    assert nxt.shape == (0, 5) and cur.shape == (0,)
    alone = custom([[0.5, -0.5, 0.4, 0.1, 0.0]], 1, waypoints=[[[3.0, 1.0]]], n_waypoints=[1])
    got, _ = check(solver, alone, "alone")
    assert got[0, 0] > 0.5                                                # it walks towards its waypoint


def test_a_standing_pair_is_pushed_apart_by_exact_negatives(solver):
    got, _ = check(solver, custom([[0.0, 0.0, 0.0, 0.0, 0.0], [0.6, 0.8, 0.0, 0.0, 0.0]], 2), "standing pair")
    assert same_bits(got[0, 2:4], -got[1, 2:4]) and got[0, 2] < 0.0 and got[0, 3] < 0.0


def test_a_coincident_pair_takes_the_same_diff_on_both_sides(solver):
    pair = custom([[1.0, 1.0, 0.3, 0.1, 0.0], [1.0, 1.0, -0.2, 0.25, 0.0], [1.0 + 5e-7, 1.0, 0.1, -0.3, 0.0]], 3)
    m = PC.case_margins(pair)
    assert m["theta"] >= 1e-9
    check(solver, pair, "coincident pair")


def test_inert_rows_are_copied_keep_their_cursor_and_are_nobodys_partner(solver):
    rows = [[0.0, 0.0, 0.3, 0.0, 0.5], [np.nan, 0.1, 0.1, 0.0, 7.0], [0.2, np.inf, 0.0, 0.1, 8.0], [0.3, 0.1, -np.inf, 0.0, 9.0],
            [0.1, 0.3, 0.0, np.nan, np.nan], [0.4, 0.4, 0.0, 0.2, 0.0], [1e300, 0.0, 0.0, 0.0, 0.0], [0.0, -1e300, 0.0, 0.0, 1.0],
            [0.2, 0.2, np.nan, 0.0, 0.0], [-np.inf, np.nan, np.nan, np.inf, -0.0]]                # the last two do not move
    c = custom(rows, 8, cursor=[0, 5, 6, 7, 8, 0, 0, 0])
    got, cur = check(solver, c, "inert rows")
    assert same_bits(got[1:5], c["agents"][1:5]) and cur[1:5].tolist() == [5, 6, 7, 8]
    only = custom(np.asarray(rows)[[0, 5, 6, 7]], 4)                      # the same live rows without the others
    alone, _ = call(solver, only)
    assert same_bits(alone, got[[0, 5, 6, 7]])
    assert same_bits(got[6], [1e300, 0.0, 0.0, 0.0, 0.0]) and same_bits(got[7, 0:4], [0.0, -1e300, 0.0, 0.0])


def test_a_person_gives_way_to_a_static_row(solver):
    # a person walks along +x towards its waypoint, a robot stands 1.5 m ahead, 0.1 m to the left: the person swerves right
    table = [[0.0, 0.0, 0.6, 0.0, 0.0], [1.5, 0.1, 0.0, 0.0, 0.0]]
    c = custom(table, 1, waypoints=[[[6.0, 0.0]]], n_waypoints=[1])
    got, _ = check(solver, c, "static partner")
    free, _ = call(solver, custom(table[:1], 1, waypoints=[[[6.0, 0.0]]], n_waypoints=[1]))
    assert got[0, 3] < -1e-3 and free[0, 3] == 0.0 and got[0, 2] < free[0, 2]
    assert same_bits(c["agents"], np.asarray(table))                      # the table is left alone


def test_the_gate_on_a_3_4_5_triangle_and_one_ulp_beyond(solver):
    inside = custom([[1.0, 2.0, 0.0, 0.0, 0.0], [4.0, 6.0, 0.0, 0.0, 0.0]], 2, rng=5.0)
    got, _ = check(solver, inside, "3-4-5 at the range")
    assert got[0, 2] < 0.0 and got[1, 2] > 0.0
    for c in (custom(inside["agents"], 2, rng=np.nextafter(5.0, 0.0), grid=inside["grid"]),
              custom([[1.0, 2.0, 0.0, 0.0, 0.0], [4.0, np.nextafter(6.0, np.inf), 0.0, 0.0, 0.0]], 2, rng=5.0)):
        got, _ = check(solver, c, "3-4-5 one ulp beyond")
        assert same_bits(got[:, 2:4], np.zeros((2, 2)))


def test_the_obstacle_grid_on_off_and_cell_off_the_grid(solver):
    c = PC.case("small_with_grid")
    on, _ = call(solver, c)
    off, _ = call(solver, {**c, "od": None})
    idx, origin, res = c["od"]
    x, y = (c["agents"][:c["M"], 0] - origin[0]) / res, (c["agents"][:c["M"], 1] - origin[1]) / res
    off_grid = (x < 0) | (y < 0) | (x >= idx.shape[1]) | (y >= idx.shape[0])
    assert 0 < off_grid.sum() < c["M"]
    assert same_bits(on[off_grid], off[off_grid])                         # no force off the grid ...
    assert (np.abs(on[~off_grid, 2:4] - off[~off_grid, 2:4]).max(axis=1) > 0).sum() >= (~off_grid).sum() - 1   # ... (but one entry is no cell)
    want, want_cur, partners = PC.reference("small_with_grid")
    P.compare(off, call(solver, {**c, "od": None})[1], *PC.ref_step({**c, "od": None}), c["dt"], partners, "grid off")


# ---- bit for bit -----------------------------------------------------------------------------------------------------------
def test_the_same_table_under_three_grids_permuted_and_twice(solver):
    c = PC.case("small_with_grid")
    base, base_cur = call(solver, c)
    again, again_cur = call(solver, c)
    assert same_bits(base, again) and np.array_equal(base_cur, again_cur)
    for grid in (PC.grid_for(c["range"]), PC.grid_for(c["range"], (-7.3, -2.1), 3, 11, factor=1.7), PC.covering_grid(-3.0, 3.0, c["range"], 1.01)):
        got, cur = call(solver, c, grid=grid)
        assert same_bits(base, got) and np.array_equal(base_cur, cur)
    g = np.random.default_rng(3)
    M, A = c["M"], len(c["agents"])
    pm, ps = g.permutation(M), M + g.permutation(A - M)
    shuffled = {**c, "agents": c["agents"][np.concatenate([pm, ps])], "cursor": c["cursor"][pm], "waypoints": c["waypoints"][pm],
                "n_waypoints": c["n_waypoints"][pm], "speeds": c["speeds"][pm]}
    got, cur = call(solver, shuffled)
    assert same_bits(base[pm], got) and np.array_equal(base_cur[pm], cur)


def test_a_batch_of_movers_against_each_mover_alone_among_static_rows(solver):
    c = PC.case("small_with_grid")
    base, base_cur = call(solver, c)
    for i in (0, 1, 17, c["M"] - 1):
        order = np.arange(len(c["agents"]))
        order[[0, i]] = order[[i, 0]]                                     # mover i into row 0, everybody else static
        got, cur = call(solver, c, agents=c["agents"][order], M=1, rows=[i])
        assert same_bits(got[0], base[i]) and cur[0] == base_cur[i]


def test_device_pointers_bins_ready_after_a_gather_and_host_pointers_agree(solver):
    import torch
    c = PC.case("small_with_grid")
    host, host_cur = call(solver, c)
    dev = "cuda:0"
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    M, A, grid = c["M"], len(c["agents"]), c["grid"]
    t = dict(agents=up(c["agents"], np.float64), waypoints=up(c["waypoints"], np.float64), n_waypoints=up(c["n_waypoints"], np.int32),
             desired_speeds=up(c["speeds"], np.float64), od_indexes=up(c["od"][0].view(np.int32), np.int32), od_origin=up(c["od"][1], np.float64))
    nbytes = solver.nearest_workspace_bytes(A, grid["grid_x"], grid["grid_y"])
    t["workspace"] = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    from nav2_social_mpc_controller_amd.solver import point
    results = []
    for ready in (0, 1):
        ci = point(solver.crowd_pool_c(PoolCrowdParams(interaction_range=c["range"], **c["params"]), M, A, PC.KMAX, c["dt"], grid["grid_x"],
                                       grid["grid_y"], grid["grid_origin"], grid["bin_size"], 1, bins_ready=ready), t)
        ci.workspace_bytes = nbytes
        ci.od_height, ci.od_width, ci.od_resolution = c["od"][0].shape[0], c["od"][0].shape[1], c["od"][2]
        if ready:  # the bins of a gather on this very table and grid (its range may be smaller than the bins allow)
            t["workspace"].zero_()
            pose = up(np.zeros((2, 3)), np.float64)
            ni = point(solver.nearest_c(2, 4, A, grid["grid_x"], grid["grid_y"], grid["grid_origin"], grid["bin_size"], c["range"], 1),
                       {"agents": t["agents"], "robot_pose": pose, "workspace": t["workspace"]})
            ni.workspace_bytes = nbytes
            people, count = torch.zeros(2, 4, 5, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            solver.nearest_people_device(ni, people.data_ptr(), count.data_ptr())
        nxt = torch.full((M, 5), POISON, dtype=torch.float64, device=dev)
        cur = up(c["cursor"], np.int32)
        torch.cuda.synchronize()
        solver.crowd_pool_step_device(ci, nxt.data_ptr(), cur.data_ptr())
        torch.cuda.synchronize()
        results.append((nxt.cpu().numpy(), cur.cpu().numpy()))
        assert same_bits(t["agents"].cpu().numpy(), c["agents"])
    for nxt, cur in results:
        assert same_bits(nxt, host) and np.array_equal(cur, host_cur)


# ---- the private crowd kernel as a cross-check ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 33])
def test_cross_check_with_the_private_crowd_step(solver, n):
    g = np.random.default_rng(70 + n)
    c = PC.build(PC.walkers(g, n, -2.0, 2.0), n, g, 100.0, PC.grid_for(100.0, (-50.0, -50.0)), speeds=True, lo=-3.0, hi=3.0)
    assert PC.case_margins(c)["theta"] >= 1e-9
    got, got_cur = call(solver, c)
    cp = CrowdParams(robot_visible=False, **c["params"])
    people, cursor = solver.crowd_step(cp, c["dt"], c["agents"][None], c["cursor"][None], np.zeros((1, 3)), np.zeros((1, 2)),
                                       np.array([n], np.int32), c["waypoints"][None], c["n_waypoints"][None], desired_speeds=c["speeds"][None])
    # rule 4 rounds each term once: the velocities (and so the positions) of the two kernels differ by at most n * 2^-36 * dt
    # plus their own 1e-12. A heading is known as well as the velocity it is taken from, relative to its length: vz * dt may
    # differ by that bound over the new speed. (Measured at n = 33: p, v differ by 2.4e-12 against a bound of 2.5e-11; vz * dt
    # alone by up to 4.8e-11, and by up to 2.3e-12 once multiplied by the mover's new speed.)
    bound = n * P.QUANTUM * c["dt"] + 1e-12
    err = np.abs(got[:, 0:4] - people[0, :, 0:4]).max()
    dz = (got[:, 4] - people[0, :, 4]) * c["dt"]
    dz = np.abs(np.arctan2(np.sin(dz), np.cos(dz)))
    speed = np.hypot(people[0, :, 2], people[0, :, 3])
    assert speed.min() > 0.01
    print(f"n = {n}: pool step against the private step: |d(p, v)| {err:.3e} (bound {bound:.3e}), |d vz dt| * speed {(dz * speed).max():.3e}")
    assert err <= bound and (dz * speed <= bound).all() and np.array_equal(got_cur, cursor[0])


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_next_and_cursor_untouched(solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError, point
    agents = np.ascontiguousarray(PC.case("small_no_grid_no_speeds")["agents"][:6])
    M, A, K = 4, 6, 2
    wp, n_wp = np.zeros((M, K, 2)), np.zeros(M, np.int32)
    od, od_origin = np.zeros((4, 4), np.uint32), np.zeros(2)

    def attempt(code, cp=None, next_null=False, cursor_null=False, next_in_table=False, **fields):
        ci = point(solver.crowd_pool_c(cp or PoolCrowdParams(), M, A, K, 0.1, 2, 2, [-4.0, -4.0], 5.0 * PC.MARGIN, 0),
                   {"agents": agents, "waypoints": wp, "n_waypoints": n_wp})
        for k, v in fields.items():
            if k == "grid_origin":
                ci.grid_origin[0] = v
            elif isinstance(v, np.ndarray) or v is None:
                point(ci, {k: v})
            else:
                setattr(ci, k, v)
        nxt, cur = np.full((M, 5), POISON), np.full(M, 77, np.int32)
        target = agents[2:] if next_in_table else nxt
        rc = solver.lib.smpc_crowd_pool_step_batch(solver._h, C.byref(ci), None if next_null else target.ctypes.data,
                                                   None if cursor_null else cur.ctypes.data)
        assert rc == code, (fields, rc, solver.lib.smpc_last_error().decode())
        assert (nxt == POISON).all() and (cur == 77).all()

    before = agents.copy()
    bad, unsupported = -1, -2                                             # SMPC_ERR_INVALID_ARG, SMPC_ERR_UNSUPPORTED
    for fields in (dict(M=-1), dict(M=A + 1), dict(A=-1), dict(K=0), dict(grid_x=0), dict(grid_y=0), dict(dt=0.0), dict(dt=-0.1), dict(dt=np.nan),
                   dict(dt=np.inf), dict(goal_radius=-0.1), dict(person_radius=-0.1), dict(person_radius=np.nan), dict(desired_speed=0.0),
                   dict(interaction_range=0.0), dict(interaction_range=np.inf), dict(interaction_range=np.nan), dict(bin_size=5.0),
                   dict(bin_size=np.nan), dict(bin_size=np.inf), dict(grid_origin=np.nan), dict(grid_origin=np.inf), dict(agents=None),
                   dict(waypoints=None), dict(n_waypoints=None), dict(next_null=True), dict(cursor_null=True), dict(next_in_table=True),
                   dict(od_indexes=od, od_origin=None, od_width=4, od_height=4, od_resolution=0.25),
                   dict(od_indexes=od, od_origin=od_origin, od_width=0, od_height=4, od_resolution=0.25),
                   dict(od_indexes=od, od_origin=od_origin, od_width=4, od_height=4, od_resolution=0.0),
                   dict(on_device=1, workspace=None), dict(on_device=1, workspace=agents, workspace_bytes=8)):
        attempt(bad, **fields)
    for fields in (dict(K=9), dict(grid_x=257, grid_y=256), dict(A=2 ** 24 + 1)):
        attempt(unsupported, **fields)
    assert solver.lib.smpc_crowd_pool_step_batch(None, None, None, None) == bad
    assert same_bits(agents, before)
    with pytest.raises(SmpcError, match="bin_size"):
        solver.crowd_pool_step(PoolCrowdParams(), 0.1, agents, M, np.zeros(M, np.int32), wp, n_wp, 2, 2, [-4.0, -4.0], 4.0)
