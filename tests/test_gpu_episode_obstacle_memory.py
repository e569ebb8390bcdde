"""Closed-loop episodes on sensed local costmaps with memory (BatchEpisode(sensor=..., sensor_memory=ObstacleMemoryParams())):
test_gpu_episode_sensed.py's 12 robots, 80 x 80 windows, arc plans and private persons, 6 recorded ticks. Every tick's
windows, beams and mark bitmaps are the yardstick's (tests/obstacle_memory_ref.py) on that tick's recorded pose, persons,
window cells and state; graph replay equals the eager ticks; without `sensor_memory` the episode is the sensed one. And two
constructed scenes with a standing robot: a pedestrian who walks from sight to behind a pillar, and one whom another hides.

No assertion on how well the robots then drive."""
import dataclasses

import numpy as np
import pytest

import obstacle_memory_ref as M
import sensed_costmap_ref as R
import visibility_ref as V
from nav2_social_mpc_controller_amd.params import ObstacleMemoryParams, OptimizerParams, SensorParams, TrajectorizerParams
from test_gpu_episode_sensed import B, SIZE, setup, spot_in_front
from test_gpu_episode_sensed import state as sensed_state

pytestmark = pytest.mark.gpu

TICKS = 6
SENSOR, MEMORY = SensorParams(), ObstacleMemoryParams()
WORDS = (SIZE + 31) // 32


def build(memory=MEMORY):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup("private")
    ep = BatchEpisode(prm, sc, w_ref, sensor=SENSOR, sensor_memory=memory, **kw)
    spot = spot_in_front(world, sc.pose0[0])                                # a pedestrian stands 1 m from robot 0
    ep.persons[0, 0] = ep.torch.tensor([spot[0], spot[1], 0.0, 0.0, 0.0], dtype=ep.torch.float64, device=ep.dev)
    ep.person_count[0] = max(int(ep.person_count[0]), 1)
    return ep, world


def state(ep):
    out = sensed_state(ep)
    if ep.sensor_memory is not None:
        out.update({k: getattr(ep, k).cpu().numpy().copy() for k in ("obstacle_memory", "obstacle_memory_cell")})
    return out


def reference(world, r, before, sp=SENSOR, mp=MEMORY):
    """The yardstick's call on a tick's record, from the state `before`."""
    res = world.resolution
    table, _ = sp.inflation_table(res)
    return M.step(before, world.map, world.origin, res, r.robot_pose, r.persons, r.person_count, r.costmap_cell, SIZE, SIZE,
                  mp.beam_cells(sp, res), sp.agent_d2(res), table, mp.mark_d2(sp, res), mp.footprint_d2(res), sp.BASES.index(sp.base), 255,
                  sp.occlusion_min_cost, sp.unknown_occludes)


@pytest.fixture(scope="module")
def eager():
    ep, world = build()
    assert ep.obstacle_memory.shape == (B, SIZE, WORDS) and ep.obstacle_memory_cell.shape == (B, 2) and not ep.obstacle_memory.any()
    assert ep._c.sensor_memory.scan.cell == ep.costmap_cell.data_ptr() and ep._c.sensor_memory.mark_d2 == 2500 and ep._c.sensor_memory.footprint_d2 == 23
    assert int(np.abs(ep.sensor_beams.cpu().numpy()).max()) == 60            # the beams clear out to 3.0 m
    recs, states = [], []
    for _ in range(TICKS):
        timing = {}
        recs.append(ep.tick(record=True, timing=timing))
        ep.synchronize()
        assert timing["obstacle_memory_ms"] > 0.0 and "sensed_costmap_ms" not in timing
        states.append(state(ep))
    return dict(ep=ep, recs=recs, states=states, world=world)


def test_every_ticks_windows_beams_and_memory_are_the_yardsticks(eager):
    world = eager["world"]
    kept = 0
    carried = (np.zeros((B, SIZE, WORDS), np.uint32), np.zeros((B, 2), np.int32))
    for k, (r, st) in enumerate(zip(eager["recs"], eager["states"])):
        before = (r.obstacle_memory_before.view(np.uint32), r.obstacle_memory_cell_before)
        assert np.array_equal(before[0], carried[0]) and (k == 0 or np.array_equal(before[1], carried[1])), k   # the state is fed forward
        cm, kind, hit, (memory, cell), stats = reference(world, r, before)
        assert r.sensed_costmap.dtype == np.uint8 and np.array_equal(r.sensed_costmap, cm), k
        assert np.array_equal(r.beam_kind, kind) and np.array_equal(r.beam_cell, hit), k
        assert r.obstacle_memory_after.dtype == np.int32 and np.array_equal(r.obstacle_memory_after.view(np.uint32), memory), k
        assert np.array_equal(st["obstacle_memory_cell"], cell) and np.array_equal(cell, r.costmap_cell), k
        assert np.array_equal(st["costmap"], cm) and np.array_equal(st["obstacle_memory"].view(np.uint32), memory), k
        carried = (memory, cell)
        kept += int((stats["kept"] >= 1).sum())
    print("robot-ticks that keep a mark from memory alone:", kept)
    assert kept >= 1


def test_graph_replay_equals_the_eager_ticks(eager):
    g, _ = build()
    g.capture_graph()
    assert not g.obstacle_memory.any() and not g.obstacle_memory_cell.any()    # the warm-up tick's marks are taken back
    for _ in range(TICKS):
        g.replay()
    g.synchronize()
    want = eager["states"][-1]
    for k, v in state(g).items():
        assert V.same_bits(v, want[k]), k


def test_without_sensor_memory_the_episode_is_the_sensed_one():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode
    prm, world, sc, w_ref, kw = setup("private")
    plain, none = BatchEpisode(prm, sc, w_ref, sensor=SENSOR, **kw), BatchEpisode(prm, sc, w_ref, sensor=SENSOR, sensor_memory=None, **kw)
    for ep in (plain, none):
        assert ep.sensor_memory is None and not hasattr(ep._c, "sensor_memory")
        assert not hasattr(ep, "obstacle_memory") and not hasattr(ep, "obstacle_memory_cell")
        assert int(np.abs(ep.sensor_beams.cpu().numpy()).max()) == 50
    for k in range(3):
        timing = {}
        a, b = plain.tick(record=True), none.tick(record=True, timing=timing)
        assert "obstacle_memory_ms" not in timing and timing["sensed_costmap_ms"] > 0.0
        assert a.obstacle_memory_before is None and a.obstacle_memory_cell_before is None and a.obstacle_memory_after is None
        cm, kind, hit = R.sensed_costmap(world.map, world.origin, world.resolution, a.robot_pose, a.persons, a.person_count, a.costmap_cell, SIZE,
                                         SIZE, SENSOR.beam_cells(world.resolution), SENSOR.agent_d2(world.resolution),
                                         SENSOR.inflation_table(world.resolution)[0])
        assert np.array_equal(a.sensed_costmap, cm) and np.array_equal(a.beam_kind, kind) and np.array_equal(a.beam_cell, hit)
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, dict):
                assert all(V.same_bits(x[n], y[n]) for n in x), (k, f.name)
            elif x is not None:
                assert V.same_bits(x, y), (k, f.name)
    with pytest.raises(ValueError):                                         # the memory is the scan's
        BatchEpisode(prm, sc, w_ref, sensor_memory=MEMORY, **kw)
    with pytest.raises(ValueError):                                         # clears less far than the sensor marks
        BatchEpisode(prm, sc, w_ref, sensor=SENSOR, sensor_memory=ObstacleMemoryParams(raytrace_range=2.0), **kw)
    with pytest.raises(ValueError):                                         # beyond 127 cells
        BatchEpisode(prm, sc, w_ref, sensor=SENSOR, sensor_memory=ObstacleMemoryParams(raytrace_range=6.5), **kw)


# ---- a pedestrian steps out of sight -----------------------------------------------------------------------------------------
# Robot 0 stands on an empty floor. "pillar": a pillar of 5 x 5 cells 0.5 m in front (+x) of it; a pedestrian 1.75 m in front
# (inside the 4 m window) starts 0.9 m to the side (+y), in sight, and walks along -y to end in the pillar's shadow, which is
# wider there than the pedestrian's disc (0.3 m). "person": no pillar; one pedestrian stands 1.85 m in front, a second one
# walks the same 0.9 m across at 0.45 m and ends between the two. In both the inflation (0.7 m) of what hides ends short of the
# hidden disc, so whatever the window holds there is the hidden pedestrian's.
# A robot that stands behind a pillar that stands casts the same beams every tick: a cell it once hit is reached again by the
# same beam and cleared, unless that beam is now stopped earlier or the cell was one of a corner pair, which no beam passes.
# So, by the header's rule, the pillar hides no last-seen cell at all (the set the yardstick gives is empty, and the test says
# so: what it then checks of this scene is that every cell the pedestrian left is free again and that nothing lethal is
# left in the shadow), while another person, who stops beams that ran on before, hides whole last-seen arcs.
SCENE_TICKS, STEP = 7, 0.15             # the walker moves 0.15 m per tick, 0.9 m in all
MIN_HIDDEN = {"pillar": 0, "person": 3}


def scene(kind):
    """(world, scenes, rows of robot 0's persons [n,5], the hidden pedestrian's row)."""
    from nav2_social_mpc_controller_amd.scenes import make_world, scenes_in_world
    prm = OptimizerParams.readme()
    world = make_world(256, 192, 0.05, seed=0x5EED0004, origin=(-3.2, 1.15), discs=0)
    sc = scenes_in_world(prm, world, B, 4, size_x=SIZE, size_y=SIZE)
    robot = sc.pose0[0, :2].copy()
    v = -STEP / prm.dt
    if kind == "pillar":
        c = np.floor((robot + [0.5, 0.0] - world.origin) / world.resolution).astype(int)
        world.map[c[1] - 2:c[1] + 3, c[0] - 2:c[0] + 3] = 254
        rows = [[robot[0] + 1.75, robot[1] + 0.9, 0.0, v, 0.0]]
    else:
        rows = [[robot[0] + 1.85, robot[1], 0.0, 0.0, 0.0], [robot[0] + 0.45, robot[1] + 0.9, 0.0, v, 0.0]]
    return prm, world, sc, np.array(rows), 0


def run_scene(kind, memory):
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, arc_plans
    prm, world, sc, rows, _ = scene(kind)
    tp = TrajectorizerParams(desired_linear_vel=0.6, lookahead_dist=0.4, max_angular_vel=1.0, time_step=0.05, max_time=1.5)
    plan, plan_len = arc_plans(sc.pose0, np.zeros(B))
    ep = BatchEpisode(prm, sc, np.zeros(B), sensor=SENSOR, sensor_memory=memory, plan=plan, plan_len=plan_len, traj_params=tp, fov_angle=1.2,
                      plan_window=(4.0, 10.0), obstacles_from_costmap=True, world=world)
    torch = ep.torch
    pose0, speed0 = ep.pose.clone(), ep.speed.clone()
    ep.persons[0, :len(rows)] = torch.tensor(rows, dtype=torch.float64, device=ep.dev)
    ep.person_count[0] = len(rows)
    recs = []
    for _ in range(SCENE_TICKS):
        ep.pose.copy_(pose0)                                                 # the robots stand
        ep.speed.copy_(speed0)
        recs.append(ep.tick(record=True))
    ep.synchronize()
    return world, recs


def hit_cells(world, r, sp=SENSOR, mp=MEMORY):
    """The window cells of robot 0 that a beam of this tick hits (both cells of a pair), at any range: what the yardstick
    marks from an empty memory with an unlimited marking range and no footprint."""
    res = world.resolution
    zero = (np.zeros((1, SIZE, WORDS), np.uint32), np.zeros((1, 2), np.int32))
    out = M.step(zero, world.map, world.origin, res, r.robot_pose[:1], r.persons[:1], r.person_count[:1], r.costmap_cell[:1], SIZE, SIZE,
                 mp.beam_cells(sp, res), sp.agent_d2(res), sp.inflation_table(res)[0], 2 * 127 * 127, -1)
    return M.bits_to_cells(out[3][0][0], SIZE)


def out_of_sight(world, recs, who):
    """By the yardstick alone, for robot 0 over the recorded ticks: (hidden: marked after the last tick, hit by no beam of it,
    and on the disc `who` stood on when last seen; left: hit in an earlier tick, unmarked after the last; the yardstick's
    last window)."""
    state = (np.zeros((B, SIZE, WORDS), np.uint32), np.zeros((B, 2), np.int32))
    marks, hits = [], []
    for r in recs:
        assert np.array_equal(r.robot_pose, recs[0].robot_pose) and np.array_equal(r.costmap_cell, recs[0].costmap_cell)
        cm, kind, hit, state, _ = reference(world, r, state)
        marks.append(M.bits_to_cells(state[0][0], SIZE))
        hits.append(hit_cells(world, r))
    q = np.array(R.point_cell(*recs[-1].persons[0, who, :2], world.origin, world.resolution)) - recs[-1].costmap_cell[0]
    on_disc = lambda c: (c[0] - q[0]) ** 2 + (c[1] - q[1]) ** 2 <= (6 + STEP / world.resolution) ** 2   # the disc, or where it was a tick ago
    hidden = {c for c in marks[-1] - hits[-1] if on_disc(c)}
    left = set().union(*hits[:-1]) - marks[-1]
    return hidden, left, cm[0]


@pytest.mark.parametrize("kind", ["pillar", "person"])
def test_a_pedestrian_who_steps_out_of_sight_stays_in_the_window_where_last_seen(kind):
    world, recs = run_scene(kind, MEMORY)
    _, plain = run_scene(kind, None)
    hidden, left, want = out_of_sight(world, recs, scene(kind)[4])
    print(kind, "scene: hidden", len(hidden), "freed", len(left))
    assert len(hidden) >= MIN_HIDDEN[kind] and len(left) >= 3
    assert kind != "pillar" or not hidden                                   # see above: a standing robot's pillar hides nothing
    last, last_plain = recs[-1].sensed_costmap[0], plain[-1].sensed_costmap[0]
    assert np.array_equal(last, want)
    assert all(last[y, x] == 254 for x, y in hidden)                        # the memory keeps them lethal
    assert all(last_plain[y, x] == 0 for x, y in hidden)                    # the memoryless scan has forgotten them
    assert all(last[y, x] != 254 for x, y in left)                          # and what was seen to be left is free again
    for a, b in zip(recs, plain):                                           # the two episodes saw the same world
        assert np.array_equal(a.persons, b.persons) and np.array_equal(a.robot_pose, b.robot_pose)
