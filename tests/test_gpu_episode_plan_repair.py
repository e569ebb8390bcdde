"""Closed-loop episodes whose plans give way to what the scan shows (BatchEpisode(sensor=..., repair=PlanRepairParams(...))):
6 robots on an open 96 x 96 world with 40 x 40 windows, every robot's straight plan running through a person who stands 0.6 m
ahead of it; with the sensed windows and with the scan's memory, with and without a plan window, 8 recorded ticks. Every
tick's repaired plans, lengths, status and info are the yardstick's (tests/plan_repair_ref.py) on that tick's recorded pose,
sensed window, window origin, plan and plan_start; every robot is REPAIRED in at least one tick; the tick after reads the
repaired plan: its plan window and its trajectorized path are the library's own on the recorded repaired rows; graph replay
equals the eager ticks byte for byte, as do two shards; without the keyword nothing is allocated and the episode is the one
before; the keyword is refused without a plan.

No assertion on how well the robots then drive."""
import dataclasses

import numpy as np
import pytest

import global_plan_ref as G
import plan_repair_ref as R
from nav2_social_mpc_controller_amd.params import ObstacleMemoryParams, OptimizerParams, PlanRepairParams, SensorParams, TrajectorizerParams

pytestmark = pytest.mark.gpu

B, N, SIZE, TICKS, FOV, L = 6, 2, 40, 8, 1.2, 200
RP = PlanRepairParams(radius=0.9, rejoin_clearance=0.3, stride=2)
WINDOW = (4.0, 10.0)
KINDS = {"sensed_window": dict(sensor=SensorParams(), plan_window=WINDOW), "sensed": dict(sensor=SensorParams()),
         "memory_window": dict(sensor=SensorParams(), sensor_memory=ObstacleMemoryParams(), plan_window=WINDOW),
         "memory": dict(sensor=SensorParams(), sensor_memory=ObstacleMemoryParams())}
STATE = ("pose", "speed", "persons", "person_count", "cmd_vel", "costmap", "costmap_origin", "costmap_cell", "people", "has_people", "beam_kind", "beam_cell")
REPAIR_STATE = ("plan", "plan_len", "repair_status", "repair_info")
AHEAD = 0.6


def setup():
    """The world, the scenes and the keywords: every robot looks towards the floor's centre, its plan runs straight on, and its
    first person stands AHEAD metres down the plan (the others are put away)."""
    from nav2_social_mpc_controller_amd.episode import arc_plans
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world
    prm = OptimizerParams.readme()
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    world = make_world(96, 96, 0.05, origin=(-1.0, 0.5), discs=0)
    sc = scenes_in_world(prm, world, B, N, size_x=SIZE, size_y=SIZE, margin=1.3)
    centre = np.asarray(world.origin) + 0.5 * 96 * 0.05
    to_centre = centre - sc.pose0[:, :2]
    # ... along the axis or diagonal nearest to that bearing: the few cells a scan marks of a person then lie on the plan
    sc.pose0[:, 2] = np.round(np.arctan2(to_centre[:, 1], to_centre[:, 0]) / (np.pi / 4)) * (np.pi / 4)
    plan, plan_len = arc_plans(sc.pose0, np.zeros(B), L=L, ds=0.05)
    persons = np.zeros((B, N, 5))
    persons[:, 0, :2] = sc.pose0[:, :2] + AHEAD * np.stack([np.cos(sc.pose0[:, 2]), np.sin(sc.pose0[:, 2])], axis=1)
    kw = dict(plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=FOV, obstacles_from_costmap=True, world=world)
    return prm, world, sc, kw, persons


def place_persons(ep, persons):
    ep.persons.copy_(ep.torch.from_numpy(persons).to(ep.dev))
    ep.person_count.fill_(1)


def build(kind, repair=RP):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, kw, persons = setup()
    ep = BatchEpisode(prm, sc, np.zeros(B), repair=repair, **KINDS[kind], **kw)
    place_persons(ep, persons)
    return ep, world, kw


def state(ep):
    out = {k: getattr(ep, k).cpu().numpy().copy() for k in STATE + (REPAIR_STATE if ep.repair is not None else ())}
    out.update({"res_" + k: v.cpu().numpy().copy() for k, v in ep.res.items()})
    return out


def repair_case(world, r, windowed):
    """One recorded tick's inputs as the yardstick's case."""
    return dict(costmap=r.sensed_costmap, origin=r.costmap_origin, res=world.resolution, pose=r.robot_pose, plan=r.repair_plan_before,
                plan_len=r.repair_plan_len_before, plan_start=r.plan_start if windowed else None, R=RP.radius_cells(world.resolution), stride=RP.stride,
                clearance_d2=RP.clearance_d2, cost=G.Cost(RP.neutral_cost, RP.cost_weight, RP.lethal_min_cost, RP.allow_unknown))


@pytest.fixture(scope="module", params=list(KINDS))
def eager(request):
    kind = request.param
    ep, world, kw = build(kind)
    windowed = "plan_window" in KINDS[kind]
    assert ep.plan_scratch.shape == ep.plan.shape == (B, L, 2) and ep.plan_scratch.data_ptr() != ep.plan.data_ptr()
    assert ep.repair_status.shape == (B,) and ep.repair_info.shape == (B, 4) and ep.repair_status.dtype == ep.repair_info.dtype == ep.torch.int32
    ri = ep._c.repair
    assert (ri.B, ri.L, ri.on_device, ri.size_x, ri.size_y, ri.costmap_shared, ri.radius, ri.stride) == (B, L, 1, SIZE, SIZE, 0, 18, 2)
    assert (ri.resolution, ri.clearance_d2) == (world.resolution, RP.clearance_d2)
    assert (ri.costmap, ri.costmap_origin, ri.robot_pose) == (ep.costmap.data_ptr(), ep.costmap_origin.data_ptr(), ep.pose.data_ptr())
    assert ri.plan_start == (ep.plan_start.data_ptr() if windowed else None)
    addresses = [getattr(ep, k).data_ptr() for k in REPAIR_STATE]
    recs, states = [], []
    for _ in range(TICKS):
        timing = {}
        recs.append(ep.tick(record=True, timing=timing))
        ep.synchronize()
        assert timing["repair_ms"] > 0.0
        states.append(state(ep))
    assert addresses == [getattr(ep, k).data_ptr() for k in REPAIR_STATE]
    return dict(kind=kind, ep=ep, recs=recs, states=states, world=world, windowed=windowed, tp=kw["traj_params"])


def test_every_ticks_repair_is_the_yardsticks_on_the_recorded_inputs(eager):
    repaired = np.zeros(B, int)
    info = np.full((B, 4), -1, np.int32)                                     # every row is written every tick
    for k, (r, st) in enumerate(zip(eager["recs"], eager["states"])):
        assert r.repair_costmap is None                                      # the sensing stage recorded the windows
        want = R.run(repair_case(eager["world"], r, eager["windowed"]), info=info, field=False)
        got = dict(plan=r.repair_plan_after, plan_len=r.repair_plan_len_after, status=r.repair_status, info=r.repair_info, field=None)
        assert R.same(got, want), (k, [n for n in got if got[n] is not None and got[n].tobytes() != want[n].tobytes()], r.repair_status, want["status"])
        for name, key in zip(REPAIR_STATE, ("plan", "plan_len", "status", "info")):
            assert G.same_bits(st[name], want[key]), (k, name)
        info = want["info"]
        repaired += want["status"] == R.REPAIRED
        if k + 1 < TICKS:                                                    # nothing else touches the plans between two ticks
            nxt = eager["recs"][k + 1]
            assert G.same_bits(nxt.repair_plan_before, r.repair_plan_after) and G.same_bits(nxt.repair_plan_len_before, r.repair_plan_len_after)
    print(eager["kind"], "REPAIRED ticks per robot:", repaired.tolist(), "status of the last tick:", eager["recs"][-1].repair_status.tolist())
    assert (repaired >= 1).all(), repaired                                   # by the yardstick alone: a person stands on every plan


def test_the_tick_after_a_repair_trajectorizes_the_repaired_plan(eager):
    s, tp = eager["ep"].solver, eager["tp"]
    checked = 0
    for k in range(TICKS - 1):
        r, nxt = eager["recs"][k], eager["recs"][k + 1]
        if not (r.repair_status == R.REPAIRED).any():
            continue
        plan, plan_len = r.repair_plan_after, r.repair_plan_len_after
        assert not G.same_bits(plan, r.repair_plan_before)
        if eager["windowed"]:
            start = r.plan_start.copy()
            w = s.transform_global_plan(plan, plan_len, start, nxt.robot_pose, *WINDOW)
            assert G.same_bits(w["window_len"], nxt.window_len) and G.same_bits(start, nxt.plan_start)
            assert all(G.same_bits(w["window"][b, :n], nxt.window[b, :n]) for b, n in enumerate(nxt.window_len)), k    # the rows below the length
            plan, plan_len = w["window"], w["window_len"]
        out = s.trajectorize(tp, plan, plan_len, nxt.robot_pose)
        assert G.same_bits(out["path"], nxt.plan_path) and G.same_bits(out["n_poses"], nxt.traj_n_poses), k
        before = s.trajectorize(tp, r.repair_plan_before, r.repair_plan_len_before, nxt.robot_pose) if not eager["windowed"] else None
        if before is not None:                                               # ... and not the plan from before the repair
            rows = np.flatnonzero(r.repair_status == R.REPAIRED)
            assert any(before["path"][b].tobytes() != nxt.plan_path[b].tobytes() for b in rows), k
        checked += 1
    assert checked >= 1


def test_graph_replay_equals_the_eager_ticks(eager):
    g, _, _ = build(eager["kind"])
    before = g.plan.cpu().numpy().copy()
    g.capture_graph()
    assert G.same_bits(g.plan.cpu().numpy(), before)                         # the warm-up tick's repair is taken back
    for _ in range(TICKS):
        g.replay()
    g.synchronize()
    want = eager["states"][-1]
    for k, v in state(g).items():
        assert G.same_bits(v, want[k]), k


def test_two_shards_give_every_robot_the_same_plans(eager):
    from nav2_social_mpc_controller_amd.episode import ShardedEpisode
    prm, world, sc, kw, persons = setup()
    sh = ShardedEpisode(prm, sc, np.zeros(B), None, None, None, shards=2, repair=RP, **KINDS[eager["kind"]], **kw)
    assert len(sh.parts) == 2 and all(p.repair is RP for p in sh.parts)
    for part, sl in zip(sh.parts, sh.slices):
        with part.torch.cuda.stream(part.gstream):
            part.persons.copy_(part.torch.from_numpy(persons[sl]).to(part.dev))
            part.person_count.fill_(1)
    for _ in range(TICKS):
        sh.tick()
    want = eager["states"][-1]
    for name in ("pose", "cmd_vel") + REPAIR_STATE:
        assert G.same_bits(sh.gather(name).cpu().numpy(), want[name]), name


def test_without_the_keyword_nothing_is_allocated_and_the_episode_is_the_one_before():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, kw, persons = setup()
    more = KINDS["memory_window"]
    plain, none = BatchEpisode(prm, sc, np.zeros(B), **more, **kw), BatchEpisode(prm, sc, np.zeros(B), repair=None, **more, **kw)
    for ep in (plain, none):
        place_persons(ep, persons)
        assert ep.repair is None and not hasattr(ep._c, "repair")
        for name in ("plan_scratch", "repair_status", "repair_info"):
            assert not hasattr(ep, name), name
    plan0 = plain.plan.cpu().numpy().copy()
    for k in range(3):
        timing = {}
        a, b = plain.tick(record=True, timing=timing), none.tick(record=True)
        assert "repair_ms" not in timing
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            assert not f.name.startswith("repair_") or (x is None and y is None), f.name
            if isinstance(x, dict):
                assert all(G.same_bits(x[n], y[n]) for n in x), (k, f.name)
            elif x is not None:
                assert G.same_bits(x, y), (k, f.name)
        for name, v in state(plain).items():
            assert G.same_bits(state(none)[name], v), (k, name)
    assert G.same_bits(plain.plan.cpu().numpy(), plan0)
    stand_in = {k: v for k, v in kw.items() if k not in ("plan", "plan_len", "traj_params")}
    with pytest.raises(ValueError, match=r"repair needs plan= or planner=: there is no plan to repair"):
        BatchEpisode(prm, setup()[2], np.zeros(B), repair=RP, sensor=SensorParams(), **stand_in)
    with pytest.raises(ValueError):
        BatchEpisode(prm, sc, np.zeros(B), repair=dict(radius=0.9), **more, **kw)
    with pytest.raises(ValueError):
        BatchEpisode(prm, sc, np.zeros(B), repair=PlanRepairParams(radius=4.0), **more, **kw)
