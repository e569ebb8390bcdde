"""Cases of the scan-based people detector (include/smpc_scan_people.h), shared by tests/test_scan_people.py and
tests/test_gpu_scan_people.py: hand-made ones with the expected rows written out, and seeded ones whose hit offsets are made
directly (random runs of foreground and background beams with random jumps; the scan is not called)."""
import numpy as np

import scan_people_ref as R

RES = 0.125                      # the hand-made cases: cells of 1/8 m at origin (0, 0), so every position is exact
HOME = (5.0625, 5.0625, 0.0)     # the centre of cell (40, 40)
FAR = (30, 0)                    # where a beam that hit nothing ends: beyond every range used here


def hand(n, beams, want, Nd=4, pose=HOME, **kw):
    """One robot of n beams: `beams` maps k -> (kind, (ox, oy)); every other beam is NONE at FAR. want: det_count, the
    det_segment rows, seg_stats, and where given the positions."""
    p = R.params(**{**dict(link_d2=2, min_points=2, width_d2_min=0, width_d2_max=100, range_d2=400, subtract_map=1, body_offset=0.0,
                           res=RES, origin=(0.0, 0.0)), **kw})
    kind = np.zeros((1, n), np.uint8)
    cell = np.tile(np.array(FAR, np.int32), (1, n, 1))
    for k, (kd, o) in beams.items():
        kind[0, k], cell[0, k] = kd, o
    return dict(p=p, Nd=Nd, pose=np.array([pose], np.float64), kind=kind, cell=cell, want=want)


A, W, CP = R.KIND_AGENT, R.KIND_WORLD, R.KIND_CORNER_PAIR
RING = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
SPREAD = [(6, 0), (4, 4), (0, 6), (-4, 4), (-6, 0), (-4, -4), (0, -6), (4, -4)]


def hand_cases():
    c = {}
    c["one_arc"] = hand(16, {3: (A, (8, 0)), 4: (A, (8, 1)), 5: (A, (8, 2))},
                        dict(count=1, segs=[(3, 3, 24, 3)], stats=(1, 0, 0, 1), xy=[(6.0625, 5.1875)]))
    c["offset_pushes_back"] = hand(16, {3: (A, (8, -1)), 4: (A, (8, 0)), 5: (A, (8, 1))}, body_offset=0.25,
                                   want=dict(count=1, segs=[(3, 3, 24, 0)], stats=(1, 0, 0, 1), xy=[(6.3125, 5.0625)]))   # d = 1, k = 0.25
    c["arc_wraps"] = hand(16, {14: (A, (8, -2)), 15: (A, (8, -1)), 0: (A, (8, 0)), 1: (A, (8, 1))},
                          dict(count=1, segs=[(14, 4, 32, -2)], stats=(1, 0, 0, 1), xy=[(6.0625, 5.0)]))
    c["arc_wraps_behind_another"] = hand(16, {15: (A, (8, -1)), 0: (A, (8, 0)), 6: (A, (-8, 0)), 7: (A, (-8, -1))},
                                         dict(count=2, segs=[(6, 2, -16, -1), (15, 2, 16, -1)], stats=(2, 0, 0, 2)))
    c["arc_over_beams_60_to_70"] = hand(128, {k: (A, (10, k - 65)) for k in range(60, 71)},
                                        dict(count=1, segs=[(60, 11, 110, 0)], stats=(1, 0, 0, 1), xy=[(6.3125, 5.0625)]))
    c["too_wide"] = hand(128, {k: (A, (10, k - 65)) for k in range(59, 71)}, dict(count=0, segs=[], stats=(1, 0, 1, 0)))   # chord 121
    c["too_narrow"] = hand(16, {3: (A, (8, 0)), 4: (A, (8, 1))}, width_d2_min=2, want=dict(count=0, segs=[], stats=(1, 0, 1, 0)))
    c["too_few_points"] = hand(16, {3: (A, (8, 0)), 4: (A, (8, 1))}, min_points=3, want=dict(count=0, segs=[], stats=(1, 1, 0, 0)))
    c["every_beam_linked"] = hand(8, {k: (A, o) for k, o in enumerate(RING)},
                                  dict(count=1, segs=[(0, 8, 0, 0)], stats=(1, 0, 0, 1), xy=[(5.0625, 5.0625)], d_zero=1))   # chord |o_0 - o_7|^2 = 1
    c["none_linked_more_than_Nd"] = hand(8, {k: (A, o) for k, o in enumerate(SPREAD)}, min_points=1,
                                         want=dict(count=4, segs=[(k, 1) + SPREAD[k] for k in range(4)], stats=(8, 0, 0, 8)))
    c["one_beam"] = hand(1, {0: (A, (3, 0))}, min_points=1, want=dict(count=1, segs=[(0, 1, 3, 0)], stats=(1, 0, 0, 1), xy=[(5.4375, 5.0625)]))
    c["one_beam_background"] = hand(1, {}, min_points=1, want=dict(count=0, segs=[], stats=(0, 0, 0, 0)))
    c["two_beams_linked_to_each_other"] = hand(2, {0: (A, (3, 0)), 1: (A, (3, 1))}, dict(count=1, segs=[(0, 2, 6, 1)], stats=(1, 0, 0, 1)))
    c["two_beams_apart"] = hand(2, {0: (A, (3, 0)), 1: (A, (-3, 0))}, min_points=1,
                                want=dict(count=2, segs=[(0, 1, 3, 0), (1, 1, -3, 0)], stats=(2, 0, 0, 2)))
    wall = {k: (W, (8, k - 3)) for k in range(2, 6)}
    c["world_run_map_subtracted"] = hand(16, wall, subtract_map=1, want=dict(count=0, segs=[], stats=(0, 0, 0, 0)))
    c["world_run_map_kept"] = hand(16, wall, subtract_map=0, want=dict(count=1, segs=[(2, 4, 32, 2)], stats=(1, 0, 0, 1)))
    c["world_beam_splits_a_person"] = hand(16, {2: (A, (8, 0)), 3: (A, (8, 1)), 4: (W, (8, 2)), 5: (A, (8, 3)), 6: (A, (8, 4))},
                                           dict(count=2, segs=[(2, 2, 16, 1), (5, 2, 16, 7)], stats=(2, 0, 0, 2)))
    c["corner_pair_is_foreground"] = hand(16, {2: (A, (8, 0)), 3: (CP, (8, 1)), 4: (A, (8, 2))}, dict(count=1, segs=[(2, 3, 24, 3)], stats=(1, 0, 0, 1)))
    c["kinds_4_5_200_are_background"] = hand(16, {2: (A, (8, 0)), 3: (4, (8, 1)), 4: (A, (8, 2)), 5: (5, (8, 3)), 6: (A, (8, 4)), 7: (200, (8, 5)),
                                                  8: (A, (8, 6))}, min_points=1,
                                             want=dict(count=4, segs=[(2, 1, 8, 0), (4, 1, 8, 2), (6, 1, 8, 4), (8, 1, 8, 6)], stats=(4, 0, 0, 4)))
    c["hit_beyond_range_splits"] = hand(16, {2: (A, (19, 4)), 3: (A, (19, 5)), 4: (A, (20, 5)), 5: (A, (19, 6)), 6: (A, (18, 6))},   # 20^2 + 5^2 = 425 > 400
                                        dict(count=2, segs=[(2, 2, 38, 9), (5, 2, 37, 12)], stats=(2, 0, 0, 2)))
    c["hit_at_the_range"] = hand(16, {2: (A, (20, 0)), 3: (A, (20, 1)), 4: (A, (20, -1))}, min_points=1,   # 400 is within, 401 is not
                                 want=dict(count=1, segs=[(2, 1, 20, 0)], stats=(1, 0, 0, 1)))
    c["centroid_on_the_robot"] = hand(16, {2: (A, (-1, 0)), 3: (A, (0, 0)), 4: (A, (1, 0))}, body_offset=0.25,
                                      want=dict(count=1, segs=[(2, 3, 0, 0)], stats=(1, 0, 0, 1), xy=[(5.0625, 5.0625)], d_zero=1))
    arc = {3: (A, (8, 0)), 4: (A, (8, 1)), 5: (A, (8, 2))}
    c["robot_without_a_cell"] = hand(16, arc, pose=(1e12, 5.0, 0.0), want=dict(count=0, segs=[], stats=(0, 0, 0, 0)))
    c["pose_not_a_number"] = hand(16, arc, pose=(5.0, np.nan, 0.0), want=dict(count=0, segs=[], stats=(0, 0, 0, 0)))
    c["pose_infinite"] = hand(16, arc, pose=(-np.inf, 5.0, 0.0), want=dict(count=0, segs=[], stats=(0, 0, 0, 0)))
    c["duplicate_cell_at_near_range"] = hand(16, {2: (A, (2, 0)), 3: (A, (2, 0)), 4: (A, (2, 1)), 5: (A, (2, 1))},
                                             dict(count=1, segs=[(2, 4, 8, 2)], stats=(1, 0, 0, 1), xy=[(5.3125, 5.125)]))
    return c


def check_want(c, got):
    """`got` (the call's four outputs over NaN / -99 prefill) against the case's written expectation."""
    w, Nd = c["want"], c["Nd"]
    assert got["det_count"].tolist() == [w["count"]]
    assert got["seg_stats"].tolist() == [list(w["stats"])]
    assert got["det_segment"][0, :w["count"]].tolist() == [list(s) for s in w["segs"]]
    assert (got["det_segment"][0, w["count"]:] == -99).all() and np.isnan(got["detections"][0, w["count"]:]).all()
    rows = got["detections"][0, :w["count"]]
    assert (rows[:, 2:] == 0.0).all() and not np.signbit(rows[:, 2:]).any() and np.isfinite(rows).all()
    if "xy" in w:
        assert rows[:, :2].tolist() == [list(xy) for xy in w["xy"]]
    assert w["count"] <= Nd


SHAPES = [(67, 63, 4), (67, 64, 8), (67, 65, 8), (33, 360, 16), (5, 4096, 64), (9, 130, 1)]
SEEDED_RES, SEEDED_ORIGIN = 0.05, (-3.0, 2.0)


def seeded_name(B, n, Nd):
    return f"B{B}_n{n}_Nd{Nd}"


def _centre(a):
    return tuple(np.float64(o) + ((np.float64(q) + np.float64(0.0)) + np.float64(0.5)) * np.float64(SEEDED_RES) for q, o in zip(a, SEEDED_ORIGIN))


def seeded_case(B, n, Nd, seed):
    """Robot 1 and every fourth: the beams rolled, so runs wrap. Robot 2: every beam linked. Robot 3: a two-beam segment whose
    centroid is the robot's own cell centre, where the robot stands (d == 0). Robot 4: no foreground. Robot 6: no cell.
    Robot 7: NaN."""
    rng = np.random.default_rng(seed)
    p = R.params(link_d2=5, min_points=2, width_d2_min=1, width_d2_max=40, range_d2=900, subtract_map=seed % 2, body_offset=0.2,
                 res=SEEDED_RES, origin=SEEDED_ORIGIN)
    kind, cell = np.zeros((B, n), np.uint8), np.zeros((B, n, 2), np.int32)
    pose = np.stack([rng.uniform(-2.0, 4.0, B), rng.uniform(3.0, 9.0, B), rng.uniform(-3.0, 3.0, B)], axis=1)
    for b in range(B):
        k = 0
        while k < n:
            run = min(n - k, int(rng.integers(1, 14)))
            if rng.random() < 0.45:
                kind[b, k:k + run] = rng.choice([0, 0, 0, 1, 4, 5, 200], run)
                cell[b, k:k + run] = rng.integers(-40, 41, (run, 2))
            else:
                t, rad = rng.uniform(0, 2 * np.pi), rng.uniform(3, 32)                     # some runs lie beyond the range of 30 cells
                o = np.rint([rad * np.cos(t), rad * np.sin(t)]).astype(np.int64)
                for i in range(run):
                    kind[b, k + i] = rng.choice([2, 2, 2, 2, 2, 3, 1]) if rng.random() < 0.3 else 2
                    cell[b, k + i] = o
                    o = o + (rng.integers(-1, 2, 2) if rng.random() < 0.9 else np.array([3, 0]))   # a step of 3 cells is no link
            k += run
        if b % 4 == 1:
            shift = int(rng.integers(1, n)) if n > 1 else 0
            kind[b], cell[b] = np.roll(kind[b], shift), np.roll(cell[b], shift, axis=0)
        if b == 2:
            kind[b] = 2
            cell[b, :, 0], cell[b, :, 1] = 10, np.arange(n) % 2
        if b == 3 and n >= 4:
            a = (int(rng.integers(20, 120)), int(rng.integers(20, 120)))
            pose[b, :2] = _centre(a)
            assert R.robot_cell(pose[b, 0], pose[b, 1], SEEDED_ORIGIN, SEEDED_RES) == a
            kind[b, :4], cell[b, :4] = [0, 2, 2, 0], [(30, 0), (1, 0), (-1, 0), (30, 0)]
        if b == 4:
            kind[b] = rng.choice([0, 4, 5, 200], n)
        if b == 6:
            pose[b, 0] = 1e12
        if b == 7:
            pose[b, 1] = np.nan
    return dict(p=p, Nd=Nd, pose=pose, kind=kind, cell=cell)


def seeded_cases():
    return {seeded_name(B, n, Nd): seeded_case(B, n, Nd, 100 + i) for i, (B, n, Nd) in enumerate(SHAPES)}
