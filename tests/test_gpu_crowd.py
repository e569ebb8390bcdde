"""smpc_crowd_step_batch on the device against the CPU checker (tests/crowd_ref.py) on the seeded inputs of
tests/crowd_cases.py, whose margins tests/test_crowd.py shows on the CPU. Shapes B x Np: one robot per wave (Np = 64 and,
rounded up to 64 lanes, Np = 33), eight robots per wave (Np = 8), sixty-four (Np = 1), a partly filled last wave."""
import ctypes as C
import math

import numpy as np
import pytest

import crowd_cases as G
import crowd_ref as R
from nav2_social_mpc_controller_amd.params import CrowdParams, OptimizerParams

pytestmark = pytest.mark.gpu
DT = G.DT


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme())
    yield s
    s.close()


def call(s, pos, kw):
    """BatchSolver.crowd_step with the arguments of R.step_batch (crowd_cases.arguments)"""
    dt, people, cursor, pose, twist, count, waypoints, n_wp = pos
    cp = CrowdParams(goal_radius=kw["goal_radius"], person_radius=kw["person_radius"], desired_speed=kw["desired_speed"],
                     cyclic=kw["cyclic"], robot_visible=kw["robot_visible"])
    return s.crowd_step(cp, dt, people, cursor, pose, twist, count, waypoints, n_wp, desired_speeds=kw["desired_speeds"],
                        od_indexes=kw.get("od_indexes"), od_origin=kw.get("od_origin"), od_resolution=kw.get("od_resolution"))


def untouched_beyond_count(got_people, got_cursor, people, cursor, count):
    dead = np.arange(people.shape[1])[None, :] >= np.asarray(count)[:, None]
    assert got_people[dead].tobytes() == np.asarray(people, np.float64)[dead].tobytes()
    assert got_cursor[dead].tobytes() == np.asarray(cursor, np.int32)[dead].tobytes()


@pytest.mark.parametrize("ci", range(len(G.CONFIGS)), ids=lambda i: f"cfg{i}")
@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: f"B{s[0]}_Np{s[1]}")
def test_one_step_matches_the_checker(solver, shape, ci):
    d = G.case(shape)
    pos, kw = G.arguments(d, G.CONFIGS[ci])
    want_people, want_cursor, _ = G.reference(shape, ci)
    got_people, got_cursor = call(solver, pos, kw)
    R.compare(got_people, got_cursor, want_people, want_cursor, DT, d["count"], f"B={shape[0]} Np={shape[1]} {G.CONFIGS[ci]}")
    untouched_beyond_count(got_people, got_cursor, pos[1], pos[2], d["count"])
    if shape[0] >= 2:
        assert (d["count"] == 0).any() and (d["count"] == shape[1]).any()
    if shape[0] >= 3:
        assert (got_cursor != pos[2]).any()


def step_both(s, people, cursor, n_wp=None, wp=None, count=None, **flags):
    people = np.asarray(people, np.float64)
    B, Np, _ = people.shape
    pos = (DT, people, np.asarray(cursor, np.int32).reshape(B, Np), np.zeros((B, 3)), np.zeros((B, 2)),
           np.full(B, Np, np.int32) if count is None else np.asarray(count, np.int32),
           np.zeros((B, Np, 1, 2)) if wp is None else wp, np.zeros((B, Np), np.int32) if n_wp is None else n_wp)
    kw = dict(cyclic=True, robot_visible=False, desired_speeds=None, **G.PARAMS)
    kw.update(flags)
    return pos, call(s, pos, kw), R.step_batch(*pos, **kw)


def test_binary_exact_cases(solver):
    # a standing pair and a pair walking side by side with equal velocities: theta := 0, the terms lie on the line between them
    people = [[[0.25, 0.5, 0.0, 0.0, 0.0], [1.0, -0.75, 0.0, 0.0, 0.0]],
              [[0.0, 0.0, 0.25, 0.125, 0.0], [0.5, 1.0, 0.25, 0.125, 0.0]]]
    pos, (gp, gc), (wp_, wc) = step_both(solver, people, np.zeros((2, 2)))
    R.compare(gp, gc, wp_, wc, DT, pos[5], "equal velocities")
    assert gp[0, 0, 2] == -gp[0, 1, 2] and gp[0, 0, 3] == -gp[0, 1, 3]           # one evaluation per pair: exact negatives
    assert abs(gp[0, 1, 2] * -1.25 - gp[0, 1, 3] * 0.75) <= 1e-15 and math.hypot(*gp[0, 1, 2:4]) > 1e-3
    # a coincident pair (moving apart, and standing): each takes diff = (1e-6, 0)
    people = [[[1.0, 2.0, 0.25, 0.0, 0.0], [1.0, 2.0, -0.125, 0.25, 0.0], [1.0 + 2.0 ** -21, 2.0, 0.0, 0.0, 0.0]],
              [[-1.0, 0.5, 0.0, 0.0, 0.0], [-1.0, 0.5, 0.0, 0.0, 0.0], [3.0, 3.0, 0.0, 0.0, 0.0]]]
    pos, (gp, gc), (wp_, wc) = step_both(solver, people, np.zeros((2, 3)))
    R.compare(gp, gc, wp_, wc, DT, pos[5], "coincident pairs")
    assert gp[1, 0].tobytes() == gp[1, 1].tobytes() and gp[1, 0, 2] < 0.0        # both pushed the same way: away from +x
    # count = 0: nothing is written; n_waypoints = 0: no goal, the cursor stays (cyclic: 0 stays 0; not cyclic: as given)
    sentinel = np.arange(2 * 3 * 5, dtype=np.float64).reshape(2, 3, 5) + 0.5
    pos, (gp, gc), _ = step_both(solver, sentinel, [[3, 4, 5], [6, 7, 8]], count=[0, 0])
    assert gp.tobytes() == sentinel.tobytes() and gc.tolist() == [[3, 4, 5], [6, 7, 8]]
    lone = [[[1.0, 2.0, 0.25, -0.5, 0.75]]]
    for cyclic, start, want in ((True, 0, 0), (False, 0, 0), (False, 2, 2), (True, 2, 0)):
        pos, (gp, gc), (wp_, wc) = step_both(solver, lone, [[start]], cyclic=cyclic)
        R.compare(gp, gc, wp_, wc, DT, pos[5], "n_waypoints = 0")
        assert gc[0, 0] == want
        assert gp[0, 0, 2] == 0.25 - (0.25 / 0.5) * DT and gp[0, 0, 3] == -0.5 - (-0.5 / 0.5) * DT and abs(gp[0, 0, 4]) <= 1e-12


def test_twelve_chained_steps_follow_the_checker_from_the_devices_own_states(solver):
    shape = (65, 33)
    d = G.case(shape)
    cfg = G.CONFIGS[0]
    pos, kw = G.arguments(d, cfg)
    people, cursor = pos[1], pos[2]
    events = {}
    for k in range(12):
        pos, kw = G.arguments(d, cfg, people=people, cursor=cursor)
        got = call(solver, pos, kw)
        want = R.step_batch(*pos, events=events, **kw)
        R.compare(got[0], got[1], want[0], want[1], DT, d["count"], f"step {k + 1}")
        untouched_beyond_count(got[0], got[1], people, cursor, d["count"])
        people, cursor = got
    print("events over 12 steps:", events)
    assert events.get("arrived", 0) > 0 and events.get("wrapped", 0) > 0


def test_rows_do_not_depend_on_the_batch_the_memory_space_or_the_grids_sharing(solver):
    import torch

    shape = (130, 8)
    d = G.case(shape)
    B, Np = shape
    cfg = G.CONFIGS[0]
    pos, kw = G.arguments(d, cfg)
    full = call(solver, pos, kw)
    for b in range(B):
        p1, k1 = G.arguments(d, cfg, rows=slice(b, b + 1))
        alone = call(solver, p1, k1)
        assert alone[0].tobytes() == full[0][b:b + 1].tobytes() and alone[1].tobytes() == full[1][b:b + 1].tobytes(), b
    # device pointers
    dev = "cuda:0"
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(
        people=pos[1], cursor=pos[2], pose=pos[3], twist=pos[4], count=pos[5], wp=pos[6], n_wp=pos[7], speeds=kw["desired_speeds"],
        grids=kw["od_indexes"].view(np.int32), origin=kw["od_origin"]).items()}
    cb = solver.crowd_c(CrowdParams(cyclic=cfg["cyclic"], robot_visible=cfg["robot_visible"], **G.PARAMS), B, Np, cfg["K"], DT, 1)
    cb.robot_pose, cb.robot_twist, cb.count = t["pose"].data_ptr(), t["twist"].data_ptr(), t["count"].data_ptr()
    cb.waypoints, cb.n_waypoints, cb.desired_speeds = t["wp"].data_ptr(), t["n_wp"].data_ptr(), t["speeds"].data_ptr()
    cb.od_indexes, cb.od_origin = t["grids"].data_ptr(), t["origin"].data_ptr()
    cb.od_shared, cb.od_width, cb.od_height, cb.od_resolution = 0, G.CELLS, G.CELLS, G.RES
    solver.crowd_step_device(cb, t["people"].data_ptr(), t["cursor"].data_ptr())
    torch.cuda.synchronize()
    solver.set_stream(0)
    assert t["people"].cpu().numpy().tobytes() == full[0].tobytes() and t["cursor"].cpu().numpy().tobytes() == full[1].tobytes()
    # a shared grid against per-robot copies of it
    pos, kw = G.arguments(d, G.CONFIGS[2])
    assert np.ndim(kw["od_indexes"]) == 2
    a = call(solver, pos, kw)
    kw.update(od_indexes=np.repeat(kw["od_indexes"][None], B, axis=0), od_origin=np.repeat(kw["od_origin"][None], B, axis=0))
    b = call(solver, pos, kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_refusals_leave_people_and_cursor_untouched(solver):
    d = G.case((3, 64))
    B, Np = 3, 64
    lib, h = solver.lib, solver._h
    pos, kw = G.arguments(d, G.CONFIGS[0])
    arrays = dict(pose=pos[3], twist=pos[4], count=pos[5].copy(), wp=pos[6], n_wp=pos[7], grids=kw["od_indexes"], origin=kw["od_origin"])
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    people0, cursor0 = np.ascontiguousarray(pos[1]), np.ascontiguousarray(pos[2], np.int32)

    def refused(null=(), **change):
        cb = solver.crowd_c(CrowdParams(**G.PARAMS), B, Np, 3, DT, 0)
        cb.robot_pose, cb.robot_twist, cb.count = arrays["pose"].ctypes.data, arrays["twist"].ctypes.data, arrays["count"].ctypes.data
        cb.waypoints, cb.n_waypoints = arrays["wp"].ctypes.data, arrays["n_wp"].ctypes.data
        cb.od_indexes, cb.od_origin = arrays["grids"].ctypes.data, arrays["origin"].ctypes.data
        cb.od_shared, cb.od_width, cb.od_height, cb.od_resolution = 0, G.CELLS, G.CELLS, G.RES
        keep = []
        for k, v in change.items():
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = v.ctypes.data
            setattr(cb, k, v)
        people, cursor = people0.copy(), cursor0.copy()
        rc = lib.smpc_crowd_step_batch(None if "handle" in null else h, None if "input" in null else C.byref(cb),
                                       None if "people" in null else people.ctypes.data,
                                       None if "cursor" in null else cursor.ctypes.data)
        assert people.tobytes() == people0.tobytes() and cursor.tobytes() == cursor0.tobytes(), (null, change)
        return rc

    INVALID, UNSUPPORTED = -1, -2
    assert refused(Np=65) == UNSUPPORTED and refused(K=9) == UNSUPPORTED
    bad = [dict(B=0), dict(B=-1), dict(Np=0), dict(K=0), dict(dt=0.0), dict(dt=-0.05), dict(dt=float("nan")),
           dict(goal_radius=-1e-9), dict(person_radius=-0.1), dict(desired_speed=0.0), dict(desired_speed=-0.6),
           dict(robot_pose=None), dict(robot_twist=None), dict(count=None), dict(waypoints=None), dict(n_waypoints=None),
           dict(od_origin=None), dict(od_width=0), dict(od_height=0), dict(od_height=-3), dict(od_resolution=0.0),
           dict(od_resolution=-0.25)]
    for change in bad:
        assert refused(**change) == INVALID, change
    for null in ("handle", "input", "people", "cursor"):
        assert refused(null=(null,)) == INVALID, null
    for where, value in ((0, -1), (B - 1, Np + 1)):
        c = arrays["count"].copy()
        c[where] = value
        assert refused(count=c) == INVALID, (where, value)


def test_a_person_gives_way_to_a_visible_robot(solver):
    cp = {v: CrowdParams(cyclic=False, robot_visible=v, **G.PARAMS) for v in (True, False)}

    def stepper(people, cursor, d, visible):
        return solver.crowd_step(cp[visible], DT, people, cursor, d["pose"], d["twist"], d["count"], d["waypoints"], d["n_waypoints"])
    seen, unseen = G.closest_approach(stepper, True), G.closest_approach(stepper, False)
    print(f"closest approach: robot visible {seen:.4f} m, invisible {unseen:.4f} m")
    assert unseen <= 0.15 and seen - unseen >= 0.1
