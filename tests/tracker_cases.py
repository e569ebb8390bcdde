"""Cases of the people tracker, shared by tests/test_tracker.py (CPU) and the GPU tests: hand-made sequences with the
expected state written out, seeded sequences of persons at constant velocity behind a per-tick visibility mask, and the
runner that feeds a sequence through a `call` with the state fed forward from the call's own output.

A sequence is dict(p=tracker_ref.params(...), Nd, state0=(tracks, track_meta, next_id), ticks=[dict(det [B,Nd,5], count [B],
pose [B,3], want=None or dict(meta=[B][Nt][4], count=[B], optionally tracks=[B][Nt][4], next_id=[B], source=[B][count][2],
people=[B][count][5]))]). The hand-made ones use alpha = 0.5, beta = 0.25 and dt = 0.125 (gain = 2) on coordinates that
are small multiples of a power of two, so that every expected number is exact and can be checked by hand."""
import numpy as np

import tracker_ref as R

NAN, INF = float("nan"), float("inf")
HAND_P = dict(alpha=0.5, beta=0.25, dt=0.125, gate=0.5)


def _rows(points, Nd, fill=7.25):
    """[Nd,5] detection rows: x, y of `points`, then columns the tracker must not examine (a NaN among them)."""
    rows = np.full((Nd, 5), fill)
    rows[:, 3] = NAN
    for j, (x, y) in enumerate(points):
        rows[j, 0], rows[j, 1] = x, y
    return rows


def _tick(robots, Nd, want=None, counts=None, poses=None):
    """robots: per robot the list of detection points."""
    B = len(robots)
    return dict(det=np.stack([_rows(pts, Nd) for pts in robots]),
                count=np.array([len(pts) for pts in robots] if counts is None else counts, np.int32),
                pose=np.array([(0.0, 0.0, 0.0)] * B if poses is None else poses, np.float64), want=want)


def _seq(ticks, Nd, slots, Np=None, state0=None, **kw):
    p = R.params(**{**HAND_P, **kw}, slots=slots, Np=Np)
    B = ticks[0]["det"].shape[0]
    return dict(p=p, Nd=Nd, state0=R.zero_state(B, slots) if state0 is None else state0, ticks=ticks)


def hand_sequences():
    S = {}
    Z = [0, 0, 0, 0]
    # a lone walker at 2 m/s along x: tentative, tentative, confirmed on its third hit and handed on only then
    S["lone_walker"] = _seq([
        _tick([[(0.0, 1.0)]], 2, dict(meta=[[[1, 1, 0, 0], Z]], tracks=[[[0.0, 1.0, 0.0, 0.0], Z]], count=[0], next_id=[1])),
        _tick([[(0.25, 1.0)]], 2, dict(meta=[[[1, 2, 0, 0], Z]], tracks=[[[0.125, 1.0, 0.5, 0.0], Z]], count=[0], next_id=[1])),
        _tick([[(0.5, 1.0)]], 2, dict(meta=[[[2, 3, 0, 0], Z]], tracks=[[[0.34375, 1.0, 1.125, 0.0], Z]], count=[1], next_id=[1],
                                      source=[[[0, 0]]], people=[[[0.34375, 1.0, 1.125, 0.0, 0.0]]])),
    ], Nd=2, slots=2, confirm_hits=3)
    # a tentative track that misses once is freed; the next detection starts over with a new id
    S["tentative_miss"] = _seq([
        _tick([[(0.0, 0.0)]], 1, dict(meta=[[[1, 1, 0, 0], Z]], count=[0], next_id=[1])),
        _tick([[]], 1, dict(meta=[[Z, Z]], tracks=[[Z, Z]], count=[0], next_id=[1])),
        _tick([[(0.0, 0.0)]], 1, dict(meta=[[[1, 1, 0, 1], Z]], count=[0], next_id=[2])),
    ], Nd=1, slots=2, confirm_hits=2)
    # max_missed = 2: two misses are survived, the third frees the slot
    S["max_missed"] = _seq([
        _tick([[(1.0, 1.0)]], 1, dict(meta=[[[2, 1, 0, 0]]], count=[1], source=[[[0, 0]]])),
        _tick([[]], 1, dict(meta=[[[2, 1, 1, 0]]], tracks=[[[1.0, 1.0, 0.0, 0.0]]], count=[1])),
        _tick([[]], 1, dict(meta=[[[2, 1, 2, 0]]], count=[1], people=[[[1.0, 1.0, 0.0, 0.0, 0.0]]])),
        _tick([[]], 1, dict(meta=[[Z]], tracks=[[Z]], count=[0], next_id=[1])),
    ], Nd=1, slots=1, confirm_hits=1, max_missed=2)
    # the gate: 3/16, 4/16 against gate 5/16 has d2 == gate * gate exactly in binary (robot 0: matched); one ulp more in y
    # is outside (robot 1: the track coasts and the detection is born beside it)
    up = float(np.nextafter(0.25, 1.0))
    S["gate_exact_and_one_ulp"] = _seq([
        _tick([[(0.0, 0.0)], [(0.0, 0.0)]], 1, dict(meta=[[[2, 1, 0, 0], Z], [[2, 1, 0, 0], Z]], count=[1, 1])),
        _tick([[(0.1875, 0.25)], [(0.1875, up)]], 1,
              dict(meta=[[[2, 2, 0, 0], Z], [[2, 1, 1, 0], [2, 1, 0, 1]]], count=[1, 2], next_id=[1, 2],
                   tracks=[[[0.09375, 0.125, 0.375, 0.5], Z], [[0.0, 0.0, 0.0, 0.0], [0.1875, up, 0.0, 0.0]]],
                   source=[[[0, 0]], [[0, 0], [1, 1]]])),
    ], Nd=1, slots=2, confirm_hits=1, gate=0.3125)
    # two slots equidistant from one detection: (d2, i, j) gives it to the lower slot
    S["tie_two_slots"] = _seq([
        _tick([[(-0.25, 0.0), (0.25, 0.0)]], 2, dict(meta=[[[2, 1, 0, 0], [2, 1, 0, 1]]], count=[2])),
        _tick([[(0.0, 0.0)]], 2, dict(meta=[[[2, 2, 0, 0], [2, 1, 1, 1]]], count=[2],
                                      tracks=[[[-0.125, 0.0, 0.5, 0.0], [0.25, 0.0, 0.0, 0.0]]], source=[[[0, 0], [1, 1]]])),
    ], Nd=2, slots=2, confirm_hits=1)
    # two detections equidistant from one slot: the lower detection is taken, the other is born
    S["tie_two_detections"] = _seq([
        _tick([[(0.0, 0.0)]], 2, dict(meta=[[[2, 1, 0, 0], Z]], count=[1])),
        _tick([[(0.25, 0.0), (-0.25, 0.0)]], 2, dict(meta=[[[2, 2, 0, 0], [2, 1, 0, 1]]], count=[2],
                                                     tracks=[[[0.125, 0.0, 0.5, 0.0], [-0.25, 0.0, 0.0, 0.0]]],
                                                     source=[[[0, 0], [1, 1]]])),
    ], Nd=2, slots=2, confirm_hits=1)
    # greedy order decides: slot 1 takes detection 0 (0.375 away) before slot 0 (0.625 away) can, although the assignment
    # (slot 0, detection 0), (slot 1, detection 1) would have matched both; slot 0 coasts and detection 1 is born
    S["crossing_greedy"] = _seq([
        _tick([[(0.0, 0.0), (1.0, 0.0)]], 2, dict(meta=[[[2, 1, 0, 0], [2, 1, 0, 1], Z]], count=[2])),
        _tick([[(0.625, 0.0), (1.875, 0.0)]], 2,
              dict(meta=[[[2, 1, 1, 0], [2, 2, 0, 1], [2, 1, 0, 2]]], count=[3], next_id=[3],
                   tracks=[[[0.0, 0.0, 0.0, 0.0], [0.8125, 0.0, -0.75, 0.0], [1.875, 0.0, 0.0, 0.0]]],
                   source=[[[0, 0], [1, 1], [2, 2]]])),
    ], Nd=2, slots=3, confirm_hits=1, gate=1.0)
    # all slots full with one more detection: it is dropped and takes no id, tick after tick
    S["slots_full"] = _seq([
        _tick([[(0.0, 1.0), (0.0, 2.0), (0.0, 3.0)]], 3, dict(meta=[[[2, 1, 0, 0], [2, 1, 0, 1]]], count=[2], next_id=[2])),
        _tick([[(0.0, 1.0), (0.0, 2.0), (0.0, 3.0)]], 3, dict(meta=[[[2, 2, 0, 0], [2, 2, 0, 1]]], count=[2], next_id=[2])),
    ], Nd=3, slots=2, confirm_hits=1)
    # confirm_hits = 1: handed on at the first sight
    S["confirm_at_once"] = _seq([
        _tick([[(0.5, -0.5)]], 1, dict(meta=[[[2, 1, 0, 0]]], count=[1], source=[[[0, 0]]], people=[[[0.5, -0.5, 0.0, 0.0, 0.0]]])),
    ], Nd=1, slots=1, confirm_hits=1)
    # det_count below 0 and above Nd
    S["count_clamped"] = _seq([
        _tick([[(0.0, 1.0), (0.0, 2.0)], [(0.0, 1.0), (0.0, 2.0)]], 2, counts=[-3, 7],
              want=dict(meta=[[Z, Z, Z], [[2, 1, 0, 0], [2, 1, 0, 1], Z]], count=[0, 2], next_id=[0, 2])),
    ], Nd=2, slots=3, confirm_hits=1)
    # detections without a finite x and y are not used (and take no id)
    S["nan_detection"] = _seq([
        _tick([[(NAN, 0.0), (0.0, INF), (1.0, 1.0), (-INF, NAN)]], 4,
              dict(meta=[[[2, 1, 0, 0], Z]], tracks=[[[1.0, 1.0, 0.0, 0.0], Z]], count=[1], next_id=[1])),
    ], Nd=4, slots=2, confirm_hits=1)
    # a robot without a finite position hands nothing on, but its tracks live on
    S["nan_robot_pose"] = _seq([
        _tick([[(1.0, 1.0)], [(1.0, 1.0)]], 1, poses=[(NAN, 0.0, 0.0), (0.0, INF, 0.0)],
              want=dict(meta=[[[2, 1, 0, 0]], [[2, 1, 0, 0]]], count=[0, 0], next_id=[1, 1])),
        _tick([[(1.0, 1.0)], [(1.0, 1.0)]], 1, poses=[(0.0, 0.0, 0.0), (0.0, 0.0, NAN)],
              want=dict(meta=[[[2, 2, 0, 0]], [[2, 2, 0, 0]]], count=[1, 1])),
    ], Nd=1, slots=1, confirm_hits=1)
    # garbage in the state: states that do not exist and numbers that are not finite are freed, whole slot, before anything
    # else; the one sound slot (2) coasts, and the detection is born into the lowest freed slot
    tracks0 = np.array([[[1.0, 2.0, 3.0, 4.0], [NAN, 0.0, 0.0, 0.0], [4.0, 4.0, 0.0, 0.0], [0.0, 0.0, INF, 0.0], [0.0, 0.0, 0.0, -INF],
                         [5.0, 5.0, 0.0, 0.0]]])
    meta0 = np.array([[[7, 1, 1, 1], [2, 5, 0, 2], [2, 9, 0, 3], [1, 1, 0, 4], [2, 2, 2, 5], [-1, 3, 3, 6]]], np.int32)
    S["garbage_state"] = _seq([
        _tick([[(0.0, 0.0)]], 1, dict(meta=[[[2, 1, 0, 40], Z, [2, 9, 1, 3], Z, Z, Z]], next_id=[41], count=[2],
                                      tracks=[[[0.0, 0.0, 0.0, 0.0], Z, [4.0, 4.0, 0.0, 0.0], Z, Z, Z]], source=[[[0, 40], [2, 3]]])),
    ], Nd=1, slots=6, confirm_hits=1, state0=(tracks0, meta0, np.array([40], np.int32)))
    # more confirmed tracks than output rows: the nearest Np, nearest first
    S["np_below_confirmed"] = _seq([
        _tick([[(3.0, 0.0), (0.0, 1.0), (-2.0, 0.0)]], 3,
              dict(meta=[[[2, 1, 0, 0], [2, 1, 0, 1], [2, 1, 0, 2], Z]], count=[2], source=[[[1, 1], [2, 2]]],
                   people=[[[0.0, 1.0, 0.0, 0.0, 0.0], [-2.0, 0.0, 0.0, 0.0, 0.0]]])),
    ], Nd=3, slots=4, Np=2, confirm_hits=1)
    return S


SEEDED_SHAPES = {  # name -> (Nt, Nd, Np, B, persons, side of the floor in metres, seed)
    "1x1x1_B5": (1, 1, 1, 5, 2, 2.0, 101),
    "3x8x2_B67": (3, 8, 2, 67, 6, 4.0, 102),
    "16x8x8_B67": (16, 8, 8, 67, 8, 4.0, 103),
    "16x8x8_B1": (16, 8, 8, 1, 8, 4.0, 104),
    "64x64x64_B5": (64, 64, 64, 5, 40, 8.0, 105),
}


def seeded_sequence(Nt, Nd, Np, B, P, side, seed, ticks=12):
    """P persons per robot at constant velocity on a floor of side x side metres; every tick each is seen with probability
    0.7 (hidden ones stay hidden a while: the mask is a two-state chain), the seen ones arrive in a fresh random order with
    garbage in the columns the tracker must not read. Some robots start from garbage state, some have no finite position,
    and every fourth robot (from 3 slots on) carries a gadget that makes two standing tracks compete for one detection at
    exactly the same distance."""
    g = np.random.default_rng(seed)
    p = R.params(alpha=0.5, beta=0.2, gate=0.6, confirm_hits=2, max_missed=2, slots=Nt, dt=0.1, Np=Np)
    pos = g.uniform(0.0, side, (B, P, 2))
    vel = g.uniform(-1.5, 1.5, (B, P, 2))
    seen = g.random((B, P)) < 0.7
    pose = np.concatenate([g.uniform(0.0, side, (B, 2)), g.uniform(-3.0, 3.0, (B, 1))], axis=1)
    pose[g.random(B) < 0.1, 0] = NAN
    gadget = [b for b in range(B) if Nt >= 3 and Nd >= 2 and P >= 3 and b % 4 == 0]
    tracks0, meta0, next0 = R.zero_state(B, Nt)
    for b in range(0, B, 3):                                                              # garbage state to be sanitised
        tracks0[b] = g.uniform(-1.0, 1.0, (Nt, 4))
        meta0[b] = g.integers(-2, 5, (Nt, 4))
        tracks0[b, g.random(Nt) < 0.3, g.integers(0, 4)] = NAN
        next0[b] = g.integers(-5, 5)
    out = []
    for t in range(ticks):
        det, count = np.full((B, Nd, 5), 1e300), np.zeros(B, np.int32)
        det[:, :, 2:] = g.uniform(-9.0, 9.0, (B, Nd, 3))
        det[:, :, 4] = NAN
        for b in range(B):
            here, vis = pos[b] + vel[b] * (0.1 * t), seen[b].copy()
            if b in gadget:   # persons 0, 1 stand 0.5 m apart and are seen at tick 0 only; person 2 shows up once, in the middle
                here[0], here[1], here[2] = (side + 1.0, 1.0), (side + 1.5, 1.0), (side + 1.25, 1.125)
                vis[0] = vis[1] = t == 0
                vis[2] = t == 1
            rows = here[vis][g.permutation(int(vis.sum()))][:Nd]
            det[b, :len(rows), :2], count[b] = rows, len(rows)
        out.append(dict(det=det, count=count, pose=pose.copy(), want=None))
        flip = g.random((B, P))
        seen = np.where(seen, flip < 0.8, flip < 0.4)
    return dict(p=p, Nd=Nd, state0=(tracks0, meta0, next0), ticks=out)


def seeded_sequences():
    return {name: seeded_sequence(*shape) for name, shape in SEEDED_SHAPES.items()}


def dense_limit_sequence(B=3, ticks=3):
    """The (64, 64, 64) limit with all 64 detections inside every gate: 64 persons inside a square of 0.5 m against a gate
    of 2 m, so every slot qualifies with every detection and the association takes its 64 rounds."""
    g = np.random.default_rng(106)
    p = R.params(alpha=0.5, beta=0.2, gate=2.0, confirm_hits=1, max_missed=3, slots=64, dt=0.1, Np=64)
    pos = g.uniform(0.0, 0.5, (B, 64, 2))
    vel = g.uniform(-0.5, 0.5, (B, 64, 2))
    out = []
    for t in range(ticks):
        det = np.zeros((B, 64, 5))
        for b in range(B):
            det[b, :, :2] = (pos[b] + vel[b] * (0.1 * t))[g.permutation(64)]
        out.append(dict(det=det, count=np.full(B, 64, np.int32), pose=np.tile([0.25, 0.25, 0.0], (B, 1)), want=None))
    return dict(p=p, Nd=64, state0=R.zero_state(B, 64), ticks=out)


def ref_call(state, tick, p, people=None, source=None):
    new, outs, _ = R.step(state, tick["det"], tick["count"], tick["pose"], p, people, source)
    return new, outs


def run(seq, call):
    """Feeds the sequence through `call(state, tick, p) -> (new state, (people, count, source))`, the state fed forward from
    the call's own output. Yields (t, tick, state before, new state, outputs)."""
    state = tuple(np.array(a) for a in seq["state0"])
    for t, tick in enumerate(seq["ticks"]):
        new, outs = call(state, tick, seq["p"])
        yield t, tick, state, new, outs
        state = new


def same(got, want):
    """(state, outputs) pairs: every array bit for bit (NaN rows included) and of the same dtype."""
    for g, w in zip(list(got[0]) + list(got[1]), list(want[0]) + list(want[1])):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
            return False
    return True


def check_want(new, outs, want):
    """The expected state and outputs a hand-made tick writes out."""
    tracks, meta, next_id = new
    people, count, source = outs
    assert meta.tolist() == want["meta"], (meta.tolist(), want["meta"])
    assert count.tolist() == want["count"], (count.tolist(), want["count"])
    if "tracks" in want:
        assert tracks.tobytes() == np.array(want["tracks"], np.float64).tobytes(), tracks.tolist()
    if "next_id" in want:
        assert next_id.tolist() == want["next_id"], next_id.tolist()
    for b, rows in enumerate(want.get("source", [])):
        assert source[b, :len(rows)].tolist() == rows and len(rows) == count[b], source[b].tolist()
    for b, rows in enumerate(want.get("people", [])):
        assert people[b, :len(rows)].tobytes() == np.array(rows, np.float64).tobytes() and len(rows) == count[b], people[b].tolist()
    # freed slots are all +0.0, and rows from count on keep what was there before
    assert all(tracks[b, i].tobytes() == bytes(32) for b in range(meta.shape[0]) for i in range(meta.shape[1]) if meta[b, i, 0] == 0)
