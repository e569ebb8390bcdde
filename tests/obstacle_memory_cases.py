"""The sequences tests/test_obstacle_memory.py (the yardstick alone, the compiled rule) and tests/test_gpu_obstacle_memory.py
(the kernel) share. A sequence is a dict: `initial` (None: zeroed state, or (marked window cells per robot, memory_cell
[B,2])) and `ticks`, a list of (kw, mark_d2, footprint_d2, want): kw the keyword arguments of sensed_costmap_ref
(sensed_costmap_cases.case), want None or per robot the set of marked window cells after the tick, written out by hand from
the contract."""
import numpy as np

import obstacle_memory_ref as M
import sensed_costmap_cases as K

BIG = 2 * 127 * 127          # a mark_d2 that every valid hit is within
NAN = float("nan")


def initial_state(seq, kw):
    B, sx, sy = kw["people"].shape[0], kw["size_x"], kw["size_y"]
    if seq["initial"] is None:
        return M.zero_state(B, sx, sy)
    cells, memory_cell = seq["initial"]
    return np.stack([M.cells_to_bits(c, sx, sy) for c in cells]), np.array(memory_cell, np.int32).reshape(B, 2)


def tick(mark_d2=BIG, footprint_d2=-1, want=None, **kw):
    return K.case(**kw)[0], mark_d2, footprint_d2, want


ROLL_CELLS = [(0, 0), (1, 1), (31, 5), (32, 5), (33, 6), (69, 69), (35, 40), (64, 0), (0, 69), (69, 0), (38, 31), (37, 33)]
ROLL_SHIFTS = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (31, 0), (32, 0), (33, 0), (-31, 0), (-32, 0), (-33, 0), (0, 31), (0, 32), (0, 33),
               (0, -31), (0, -32), (0, -33), (69, 0), (70, 0), (-70, 0), (0, 70), (0, -70), (5000, 3), (3, -5000), (-33, 32), (2 ** 31 - 1, 0)]


def hand_sequences():
    seqs = {}
    # one cell seen (a wall), then occluded by an agent in front of it (and gone from the world: only the memory holds it),
    # then nothing in the way: the beam passes both cells
    seqs["seen_occluded_seen_through"] = dict(initial=None, ticks=[
        tick(walls=[(14, 10)], beams=[(6, 0)], want=[{(14, 10)}]),
        tick(agents=[[(12, 10)]], agent_d2=0, beams=[(6, 0)], want=[{(14, 10), (12, 10)}]),
        tick(beams=[(3, 0)], want=[{(14, 10)}]),                                          # a short beam clears only what it passes
        tick(beams=[(6, 0)], want=[set()])])
    # a corner pair marks both cells; the diagonal beam never passes either of them, a straight beam does
    seqs["corner_pair"] = dict(initial=None, ticks=[
        tick(walls=[(11, 10), (10, 11)], beams=[(4, 4)], want=[{(11, 10), (10, 11)}]),
        tick(walls=[(11, 10)], beams=[(4, 4)], want=[{(11, 10), (10, 11)}]),
        tick(walls=[(11, 10)], beams=[(4, 4), (0, 4)], want=[{(11, 10)}]),
        tick(beams=[(4, 4), (2, 0)], want=[set()])])
    # a pair whose cells lie on either side of mark_d2 = 4: (2, 0) is within, (1, 1) is too; with mark_d2 = 3 only (1, 1)
    seqs["corner_pair_each_on_its_own_offset"] = dict(initial=None, ticks=[
        tick(walls=[(12, 10), (11, 11)], beams=[(3, 1)], mark_d2=3, want=[{(11, 11)}]),
        tick(walls=[(12, 10), (11, 11)], beams=[(3, 1)], mark_d2=4, want=[{(11, 11), (12, 10)}])])
    # hits at d2 = 9 and d2 = 16: marked exactly at mark_d2, not beyond; a hit beyond leaves a mark that is there alone
    seqs["mark_range"] = dict(initial=None, ticks=[
        tick(walls=[(13, 10), (10, 14)], beams=[(6, 0), (0, 6)], mark_d2=9, want=[{(13, 10)}]),
        tick(walls=[(13, 10), (10, 14)], beams=[(6, 0), (0, 6)], mark_d2=8, want=[{(13, 10)}]),
        tick(walls=[(13, 10), (10, 14)], beams=[(6, 0), (0, 6)], mark_d2=16, want=[{(13, 10), (10, 14)}]),
        tick(walls=[(13, 10), (10, 14)], beams=[(6, 0), (0, 6)], mark_d2=0, want=[{(13, 10), (10, 14)}]),
        tick(walls=[(10, 14)], beams=[(6, 0), (0, 6)], mark_d2=0, want=[{(10, 14)}])])
    # the footprint clears after marking: the hit next to the robot never shows, the one at d2 = 4 does
    seqs["footprint"] = dict(initial=None, ticks=[
        tick(walls=[(11, 10), (10, 12)], beams=[(3, 0), (0, 3)], footprint_d2=-1, want=[{(11, 10), (10, 12)}]),
        tick(walls=[(11, 10), (10, 12)], beams=[(3, 0), (0, 3)], footprint_d2=1, want=[{(10, 12)}]),
        tick(walls=[(11, 10), (10, 12)], beams=[(3, 0), (0, 3)], footprint_d2=0, want=[{(11, 10), (10, 12)}]),
        tick(walls=[(11, 10), (10, 12)], beams=[(3, 0), (0, 3)], footprint_d2=4, want=[set()]),
        # a robot without a cell has no footprint, and one far outside its window clears nothing in it
        tick(walls=[(11, 10), (10, 12)], beams=[(3, 0), (0, 3)], footprint_d2=-1, want=[{(11, 10), (10, 12)}]),
        tick(robots=[(NAN, 0.0)], beams=[(3, 0)], footprint_d2=2 ** 31 - 1, want=[{(11, 10), (10, 12)}]),
        # a robot outside its window: the disc still reaches in, 12 * 12 + 2 * 2 <= 168 < 13 * 13
        tick(robots=[(23, 12)], beams=[(1, 0)], footprint_d2=168, want=[{(10, 12)}])])
    # the roll alone: robots without a cell, one per shift, all from the same marks on a 70 x 70 window
    B = len(ROLL_SHIFTS)
    moved = [{(x + sx, y + sy) for x, y in ROLL_CELLS if 0 <= x + sx < 70 and 0 <= y + sy < 70} for sx, sy in ROLL_SHIFTS]
    assert moved[0] == set(ROLL_CELLS) and moved[5] == {(31, 0), (32, 1), (62, 5), (63, 5), (64, 6), (66, 40), (31, 69), (69, 31), (68, 33)}
    assert moved[9] == {(0, 5), (1, 6), (37, 69), (3, 40), (32, 0), (37, 0), (6, 31), (5, 33)} and moved[16] == {(35, 7), (69, 36), (0, 36), (37, 0)}
    assert moved[17] == {(69, 0), (69, 69)} and not any(moved[k] for k in (18, 19, 20, 21, 22, 23, 25)) and moved[24] == {(0, 38), (31, 32), (36, 32), (5, 63), (4, 65)}
    seqs["roll"] = dict(initial=([set(ROLL_CELLS)] * B, [(7, -3)] * B), ticks=[
        tick(robots=[(NAN, 0.0)] * B, cell=[(7 - sx if sx < 2 ** 31 - 1 else -2 ** 31 + 8, -3 - sy) for sx, sy in ROLL_SHIFTS], size=(70, 70),
             world_size=(80, 80), beams=[(1, 0)], want=moved)])
    # window widths around the word size: a wall above the robot and one in the last column, then a roll by one cell
    for sx in (1, 31, 32, 33, 256):
        rx = max(0, sx - 4)
        walls, beams = [(rx, 0)], [(0, -1)]
        if sx > 1:
            walls, beams = walls + [(sx - 1, 1)], beams + [(sx - 1 - rx, 0)]
        seen = {(w[0], w[1]) for w in walls}
        seqs[f"width_{sx}"] = dict(initial=None, ticks=[
            tick(walls=walls, robots=[(rx, 1)], beams=beams, size=(sx, 3), world_size=(260, 5), want=[seen]),
            tick(walls=walls, robots=[(NAN, 0.0)], beams=beams, size=(sx, 3), cell=(-1, 0), world_size=(260, 5),
                 want=[{(x + 1, y) for x, y in seen if x + 1 < sx}]),
            tick(walls=walls, robots=[(NAN, 0.0)], beams=beams, size=(sx, 3), cell=(0, 1), world_size=(260, 5),
                 want=[{(x, y - 1) for x, y in seen if x + 1 < sx and y >= 1}])])
    return seqs


def seeded_sequence(seed, size, reach, ticks=6, B=8, Np=3, r=3, base=0, footprint_d2=8, mark_fraction=0.8, n_beams=None, near_fraction=0.5,
                    **world):
    """`ticks` calls on one make_world(96, 80) floor: sensed_costmap_cases.random_case's robots and agents, each walking on
    with a velocity of its own (robots up to 2 cells per tick, agents up to 3), windows centred on the robots every tick,
    beams out to `reach` cells and marks out to mark_fraction of that. world: random_case's world_size, discs, agent_d2."""
    from nav2_social_mpc_controller_amd.scenes import window_cells
    kw = K.random_case(seed=seed, reach=reach, size=size, r=r, base=base, B=B, Np=Np, n_beams=n_beams or (96 if reach > 20 else 48), **world)
    g = np.random.default_rng(1000 + seed)
    res = kw["res"]
    vel = g.uniform(-2.0, 2.0, (B, 2)) * res
    pvel = g.uniform(-3.0, 3.0, (B, Np, 2)) * res
    # near_fraction of the agents start close to their robot and walk across it: marks under the footprint, marks left behind
    near = g.random((B, Np)) < near_fraction
    people = kw["people"].copy()
    people[near, :2] = (kw["robot_pose"][:, None, :2] + g.uniform(-6.0, 6.0, (B, Np, 2)) * res)[near]
    pose = kw["robot_pose"].copy()
    mark_d2 = int((mark_fraction * reach) ** 2)
    out = []
    for _ in range(ticks):
        cell, _, _ = window_cells(kw["origin"], res, None, pose[:, :2], size[0], size[1], force=True)
        out.append((dict(kw, robot_pose=pose.copy(), people=people.copy(), cell=np.asarray(cell, np.int32).copy()), mark_d2, footprint_d2, None))
        pose[:, :2] += vel
        people[:, :, :2] += pvel
    return dict(initial=None, ticks=out)


SEEDED = [(1, (24, 20), 10), (2, (24, 20), 30), (3, (40, 33), 10), (4, (40, 33), 30)]   # (seed, window, reach)


def seeded_sequences():
    return {f"seed{seed}_{size[0]}x{size[1]}_reach{reach}": seeded_sequence(seed, size, reach) for seed, size, reach in SEEDED}


def run(seq, call):
    """Feeds a sequence through call(state, kw, mark_d2, footprint_d2) -> (costmap, kind, hit, new_state[, ...]), the state
    fed forward from the call's own output. Yields (tick index, kw, the state before, what call returned, want)."""
    state = initial_state(seq, seq["ticks"][0][0])
    for t, (kw, mark_d2, footprint_d2, want) in enumerate(seq["ticks"]):
        before = (state[0].copy(), state[1].copy())
        got = call(before, kw, mark_d2, footprint_d2)
        state = got[3]
        yield t, kw, before, got, want


def ref_call(state, kw, mark_d2, footprint_d2):
    return M.step(state, mark_d2=mark_d2, footprint_d2=footprint_d2, **kw)
