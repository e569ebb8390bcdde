"""smpc_robot_plant_batch on the GPU against tests/plant_ref.py: the state (pose, twist, cmd_queue, plant_tick) and contact
bit for bit given the device's own heading_cs, that heading held against numpy's by the bound tests/test_math.py holds
sincos_tab to, tick by tick with the state fed forward from the device's own output: the hand-made and seeded sequences of
tests/plant_cases.py (B 1 / 5 / 64 / 257, Np 1 / 4 / 8 / 64, S 1 / 4 / 16, L 0 / 1 / 8, footprint_d2 0 / 6 / 36 / 225); host
against device pointers, two runs, a permuted and a shorter batch, heading_cs NULL, world NULL, unaligned agents, and the
refusals."""
import re

import numpy as np
import pytest

import plant_cases as PC
import plant_ref as R
from nav2_social_mpc_controller_amd import _abi_plant as PA
from nav2_social_mpc_controller_amd.params import OptimizerParams

pytestmark = pytest.mark.gpu

HAND = PC.hand_sequences()
SEEDED = PC.seeded_sequences()


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme(), device=0)
    yield s
    s.close()


def plant_in(p, B, Np, on_device, world=True):
    """The yardstick's scalars as the call's struct (no pointers yet)."""
    w = p["world"] if world else None
    Hy, Hx = (0, 0) if w is None else w.shape
    pi = PA.SmpcPlantIn(B=B, Np=Np, S=p["S"], L=p["L"], on_device=on_device, Hx=Hx, Hy=Hy, footprint_d2=p["footprint_d2"],
                        wall_min_cost=p["wall_min_cost"], unknown_is_wall=int(p["unknown_is_wall"]), outside_is_wall=int(p["outside_is_wall"]),
                        dt=float(p["dt"]), v_min=float(p["v_min"]), v_max=float(p["v_max"]), w_max=float(p["w_max"]), dv_up=float(p["dv_up"]),
                        dv_down=float(p["dv_down"]), dw=float(p["dw"]), contact_dist=float(p["contact_dist"]), resolution=float(p["res"]))
    pi.world_origin[0], pi.world_origin[1] = float(p["origin"][0]), float(p["origin"][1])
    return pi


def host_call(solver, state, tick, p, rows=None, with_heading=True, world=True):
    rows = slice(None) if rows is None else rows
    agents = np.asarray(tick["agents"], np.float64)[rows]
    pi = plant_in(p, agents.shape[0], agents.shape[1], 0, world)
    pose, twist, queue, ticks, contact, cs = solver.robot_plant(
        pi, state[0][rows], state[1][rows], state[2][rows], state[3][rows], np.asarray(tick["cmd"])[rows], agents, np.asarray(tick["count"])[rows],
        world=p["world"] if world else None, with_heading=with_heading)
    return (pose, twist, queue, ticks), contact, cs


def device_call(solver, state, tick, p, offset=0, with_heading=True, world=True):
    """The call on device pointers; the agents start `offset` bytes into their allocation."""
    import torch
    from nav2_social_mpc_controller_amd.solver import point
    dev = "cuda:0"
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).copy()).to(dev)
    agents = np.ascontiguousarray(tick["agents"], np.float64)
    B, Np = agents.shape[0], agents.shape[1]
    raw = torch.zeros(agents.nbytes + offset, dtype=torch.uint8, device=dev)
    raw[offset:] = torch.from_numpy(agents.view(np.uint8).reshape(-1).copy()).to(dev)
    t = {"cmd": up(tick["cmd"], np.float64), "count": up(tick["count"], np.int32)}
    if world and p["world"] is not None:
        t["world"] = up(p["world"], np.uint8)
    pi = point(plant_in(p, B, Np, 1, world), t)
    pi.agents = raw.data_ptr() + offset
    pose, twist, queue = up(state[0], np.float64), up(state[1], np.float64), up(state[2], np.float64)
    ticks = up(np.asarray(state[3], np.uint32).view(np.int32), np.int32)
    contact = torch.full((B, 2), -1, dtype=torch.int32, device=dev)
    cs = torch.full((B, 2), float("nan"), dtype=torch.float64, device=dev)
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    solver.robot_plant_device(pi, pose.data_ptr(), twist.data_ptr(), queue.data_ptr(), ticks.data_ptr(), contact.data_ptr(),
                              cs.data_ptr() if with_heading else 0)
    torch.cuda.synchronize()
    solver.set_stream(0)
    return ((pose.cpu().numpy(), twist.cpu().numpy(), queue.cpu().numpy(), ticks.cpu().numpy().view(np.uint32)), contact.cpu().numpy(),
            cs.cpu().numpy())


def where(got, want):
    """The arrays (0 - 3: the state, 4: contact) that differ."""
    return [k for k, (g, w) in enumerate(zip(list(got[0]) + [got[1]], list(want[0]) + [want[1]])) if np.asarray(g).tobytes() != np.asarray(w).tobytes()]


def finite_rows(state):
    return np.isfinite(state[0]).all(axis=1) & np.isfinite(state[1]).all(axis=1)


# ---- against the yardstick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND) + sorted(SEEDED))
def test_state_and_contact_are_the_yardsticks_tick_by_tick_from_the_devices_own_state(solver, name):
    seq = HAND[name] if name in HAND else SEEDED[name]
    p = seq["p"]
    for t, tick, before, new, contact, cs in PC.run(seq, lambda st, tick, p: device_call(solver, st, tick, p)):
        want = PC.ref_call(before, tick, p, cs)                                                   # given the device's heading_cs
        assert PC.same((new, contact), want[:2]), (name, t, where((new, contact), want))
        ok = finite_rows(before)
        assert R.heading_close(cs, before) and np.isfinite(cs[ok]).all() and np.isnan(cs[~ok]).all(), (name, t)   # rows of bad states: not written
        PC.check_want(seq, before, new, contact, tick["want"])
    # the last tick again: from host pointers, and twice from the same state
    got = (new, contact, cs)
    host = host_call(solver, before, tick, p)
    assert PC.same(host[:2], got[:2]) and host[2].tobytes() == cs.tobytes(), (name, where(host, got))
    again = device_call(solver, before, tick, p)
    assert PC.same(again[:2], got[:2]) and again[2].tobytes() == cs.tobytes()
    again = host_call(solver, before, tick, p)
    assert PC.same(again[:2], host[:2]) and again[2].tobytes() == host[2].tobytes()


_last = {}


def last_tick(solver, name):
    """(p, tick, state before, the device's result) of a seeded sequence's last tick, the state walked there once by the
    yardstick with numpy's headings (any state serves: the comparison is between calls) and left unchanged."""
    if name not in _last:
        seq = SEEDED[name]
        for t, tick, before, new, contact, cs in PC.run(seq, PC.ref_call):
            pass
        for a in before:
            a.setflags(write=False)
        _last[name] = (seq["p"], tick, before, device_call(solver, before, tick, seq["p"]))
    return _last[name]


@pytest.mark.parametrize("name", ["B64_Np4_S4_L0_fd6", "B257_Np8_S4_L1_fd36", "B5_Np64_S16_L8_fd225"])
def test_a_robots_rows_do_not_depend_on_the_batch(solver, name):
    p, tick, before, full = last_tick(solver, name)
    B = len(tick["count"])
    take = lambda res, rows: (tuple(a[rows] for a in res[0]), res[1][rows], res[2][rows])
    perm = np.random.default_rng(B).permutation(B)
    for rows in (perm, [B - 1], list(range(0, B, 2))):
        got, want = host_call(solver, before, tick, p, rows), take(full, rows)
        assert PC.same(got[:2], want[:2]) and got[2].tobytes() == want[2].tobytes(), where(got, want)


def test_heading_null_world_null_and_unaligned_agents(solver):
    for name in ("B64_Np4_S4_L0_fd6", "B5_Np64_S16_L8_fd225"):
        p, tick, before, full = last_tick(solver, name)
        for offset in (8, 24):                                                                   # doubles, but no 16- or 32-byte boundary
            got = device_call(solver, before, tick, p, offset=offset)
            assert PC.same(got[:2], full[:2]) and got[2].tobytes() == full[2].tobytes()
        new, contact, cs = device_call(solver, before, tick, p, with_heading=False)
        assert np.isnan(cs).all() and PC.same((new, contact), full[:2])
        new, contact, cs = host_call(solver, before, tick, p, with_heading=False)
        assert cs is None and PC.same((new, contact), full[:2])
        # world NULL: the yardstick without walls, given the same headings
        q = dict(p, world=None)
        for call in (device_call, host_call):
            new, contact, cs = call(solver, before, tick, p, world=False)
            assert PC.same((new, contact), PC.ref_call(before, tick, q, cs)[:2]) and cs.tobytes() == full[2].tobytes()
            assert (contact[:, 0] & 5 == 0).all()
        assert (full[1][:, 0] & 5 != 0).any()                                                     # ... which the walls did change


def test_a_null_queue_serves_without_latency(solver):
    p, tick, before, full = last_tick(solver, "B64_Np4_S4_L0_fd6")
    agents = np.asarray(tick["agents"], np.float64)
    pi = plant_in(p, agents.shape[0], agents.shape[1], 0)
    pose, twist, queue, ticks, contact, cs = solver.robot_plant(pi, before[0], before[1], None, before[3], tick["cmd"], agents, tick["count"],
                                                                world=p["world"])
    assert queue is None and PC.same(((pose, twist, before[2], ticks), contact), full[:2]) and cs.tobytes() == full[2].tobytes()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_every_buffer_alone(solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError, _ptr
    world = np.zeros((4, 6), np.uint8)
    cmd, agents, count = np.array([[1.0, 0.5]]), np.array([[[5.0, 5.0, 0.0, 0.0, 0.0], [6.0, 6.0, 0.0, 0.0, 0.0]]]), np.array([2], np.int32)
    pose, twist, queue, tick = np.full((1, 3), 0.5), np.full((1, 2), 0.25), np.full((1, 8, 2), 7.5), np.full(1, 5, np.uint32)
    contact, cs = np.full((1, 2), -9, np.int32), np.full((1, 2), 3.5)

    def make(**kw):
        pi = PA.SmpcPlantIn(B=1, Np=2, S=4, L=2, on_device=0, Hx=6, Hy=4, footprint_d2=4, wall_min_cost=254, unknown_is_wall=0, outside_is_wall=0,
                            dt=0.25, v_min=0.0, v_max=1.0, w_max=1.0, dv_up=0.25, dv_down=0.5, dw=0.25, contact_dist=0.5, resolution=0.25,
                            world=_ptr(world), cmd=_ptr(cmd), agents=_ptr(agents), count=_ptr(count))
        for k, v in kw.items():
            setattr(pi, k, v)
        return pi

    out = lambda: (_ptr(pose), _ptr(twist), _ptr(queue), _ptr(tick), _ptr(contact), _ptr(cs))
    untouched = lambda: ((pose == 0.5).all() and (twist == 0.25).all() and (queue == 7.5).all() and (tick == 5).all() and (contact == -9).all()
                         and (cs == 3.5).all())
    INVALID, UNSUPPORTED = "(-1)", "(-2)"
    nan, inf = float("nan"), float("inf")
    cases = [(dict(B=-1), INVALID), (dict(Np=0), INVALID), (dict(Np=-2), INVALID), (dict(S=0), INVALID), (dict(L=-1), INVALID),
             (dict(footprint_d2=-2), INVALID), (dict(Hx=0), INVALID), (dict(Hy=0), INVALID), (dict(Hy=-3), INVALID),
             (dict(v_min=1.5), INVALID), (dict(v_min=nan), INVALID), (dict(v_max=inf), INVALID), (dict(v_min=-inf), INVALID),
             (dict(dv_up=-0.1), INVALID), (dict(dv_up=nan), INVALID), (dict(dv_down=-1.0), INVALID), (dict(dv_down=nan), INVALID),
             (dict(dw=-0.5), INVALID), (dict(dw=nan), INVALID), (dict(cmd=None), INVALID), (dict(agents=None), INVALID), (dict(count=None), INVALID),
             (dict(Np=65), UNSUPPORTED), (dict(S=17), UNSUPPORTED), (dict(L=9), UNSUPPORTED), (dict(footprint_d2=226), UNSUPPORTED)]
    for name in ("dt", "w_max", "contact_dist", "resolution"):
        cases += [(dict([(name, v)]), INVALID) for v in (nan, inf, -0.5)]
    cases += [(dict(resolution=0.0), INVALID)]
    for kw, code in cases:
        with pytest.raises(SmpcError, match=re.escape(code)):
            solver._call("smpc_robot_plant_batch", make(**kw), *out())
        assert untouched(), kw
    for hole in (0, 1, 2, 3, 4):                                                                 # NULL pose, twist, cmd_queue (L > 0), plant_tick, contact
        args = list(out())
        args[hole] = None
        with pytest.raises(SmpcError, match=re.escape(INVALID)):
            solver._call("smpc_robot_plant_batch", make(), *args)
        assert untouched(), hole
    assert solver.lib.smpc_robot_plant_batch(None, make(), *out()) == -1                         # NULL handle
    assert solver.lib.smpc_robot_plant_batch(solver._h, None, *out()) == -1                      # NULL struct
    assert untouched()
    solver._call("smpc_robot_plant_batch", make(B=0), *out())                                    # an empty batch is no refusal and writes nothing
    assert untouched()
    # the accepted calls run; infinite limits are allowed, and so is a NULL queue without latency
    solver._call("smpc_robot_plant_batch", make(dv_up=inf, dv_down=inf, dw=inf), *out())
    assert twist.tolist() == [[1.0, 1.0]] and tick.tolist() == [6] and contact.tolist() == [[0, 4]] and solver.last_kernel_ms() > 0.0
    assert queue[0, 1].tolist() == [1.0, 0.5] and (queue[0, [0, 2, 3, 4, 5, 6, 7]] == 7.5).all() and np.isfinite(cs).all()
