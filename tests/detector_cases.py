"""Inputs of the people-detector tests, shared by the CPU and the GPU files: hand-made single ticks on dyadic numbers with
the expected outputs written out, and seeded 10-tick sequences with the draw state fed forward. A case is a dict
{p: detector_ref.params(...), state0 [B,2] uint32, ticks: [{people [B,Np,5], count [B] int32, pose [B,3], want}]}; `want` (hand-
made only) maps "state" / "count" / "source" / "outcome" / "rows" to what the contract gives, robot by robot."""
import numpy as np

import detector_ref as R

NAN = float("nan")
ALL = 2 ** 32 - 1
QUIET = dict(p_miss=0.0, sigma=0.0, sigma_growth=0.0, clutter_candidates=0, p_clutter=0.0)   # nothing but the geometry


def person(x, y, vx=0.5, vy=-0.25, extra=0.0):
    return [x, y, vx, vy, extra]


def one(people, count=None, pose=(0.0, 0.0, 0.0), state=(0, 0), want=None, **pkw):
    """A single tick of one robot."""
    people = np.array([people], np.float64)
    pkw.setdefault("Nd", people.shape[1])
    return dict(p=R.params(**pkw), state0=np.array([state], np.uint32),
                ticks=[dict(people=people, count=np.array([people.shape[1] if count is None else count], np.int32),
                            pose=np.array([pose], np.float64), want=want)])


def hand_cases():
    D, O, M, N = R.DETECTED, R.BODY_OCCLUDED, R.MISSED, R.NOT_FINITE
    up = float(np.nextafter(0.25, 1.0))
    front, rear = person(1.0, 0.0), person(2.0, 0.0)
    cases = {
        # the rear person d = (2, 0): dd = 4, R2 * dd = 0.25; the front one at (1, 0.25) has cr = -0.5, cr * cr == 0.25: hidden
        "behind_at_the_radius_exactly": one([person(1.0, 0.25), rear], **QUIET,
                                            want=dict(outcome=[[D, O]], count=[1], source=[[0]], rows=[[person(1.0, 0.25)]], state=[[0, 1]])),
        # one ulp further from the line: cr * cr > 0.25
        "behind_one_ulp_beyond_the_radius": one([person(1.0, up), rear], **QUIET, want=dict(outcome=[[D, D]], count=[2], source=[[0, 1]])),
        "in_file": one([rear, front], **QUIET, want=dict(outcome=[[O, D]], count=[1], source=[[1]], rows=[[front]])),
        "in_file_body_radius_zero": one([rear, front], **dict(QUIET, body_radius=0.0), want=dict(outcome=[[D, D]], count=[2], source=[[0, 1]])),
        # tk == dd: (2, 0.125) projects onto the end of the sight line to (2, 0) and hides nothing there; seen from the other
        # side, (2, 0) projects strictly inside the line to (2, 0.125) and lies 0.125 from it: the rule hides that one
        "tk_equals_dd": one([rear, person(2.0, 0.125)], **QUIET, want=dict(outcome=[[D, O]], count=[1], source=[[0]])),
        "tk_equals_zero": one([rear, person(0.0, 0.125)], **QUIET, want=dict(outcome=[[D, D]], count=[2], source=[[0, 1]])),
        "behind_the_robot": one([rear, person(-1.0, 0.0)], **QUIET, want=dict(outcome=[[D, D]], count=[2], source=[[0, 1]])),
        "two_at_the_same_point": one([person(1.0, 1.0), person(1.0, 1.0, 9.0)], **QUIET,
                                     want=dict(outcome=[[D, D]], count=[2], source=[[0, 1]], rows=[[person(1.0, 1.0), person(1.0, 1.0, 9.0)]])),
        "robot_off_the_origin": one([person(5.0, -3.0), person(4.0, -3.0)], pose=(3.0, -3.0, 1.0), **QUIET,
                                    want=dict(outcome=[[O, D]], count=[1], source=[[1]])),
        "miss_threshold_zero": one([front, person(0.0, 3.0)], **QUIET, miss_threshold=0, want=dict(outcome=[[D, D]], count=[2], source=[[0, 1]])),
        "miss_threshold_all": one([front, person(0.0, 3.0)], **QUIET, miss_threshold=ALL, want=dict(outcome=[[M, M]], count=[0], state=[[0, 1]])),
        # scale == 0: the row is the person's bit for bit, a -0.0 coordinate and a NaN velocity included
        "bit_copy_at_scale_zero": one([[-0.0, 1.0, NAN, -0.0, 3.5]], **QUIET, want=dict(outcome=[[D]], count=[1], source=[[0]],
                                                                                   rows=[[[-0.0, 1.0, NAN, -0.0, 3.5]]])),
        "nd_below_the_detected_persons": one([person(1.0, 0.0), person(0.0, 1.0), person(-1.0, 0.0)], **QUIET, Nd=2,
                                             want=dict(outcome=[[D, D, D]], count=[2], source=[[0, 1]], rows=[[person(1.0, 0.0), person(0.0, 1.0)]])),
        "nd_cuts_through_the_clutter": one([front], **dict(QUIET, clutter_candidates=3), clutter_threshold=ALL, Nd=3,
                                           want=dict(outcome=[[D]], count=[3], source=[[0, -1, -2]])),
        "clutter_alone": one([front], count=0, **dict(QUIET, clutter_candidates=2), clutter_threshold=ALL, Nd=4, state=(7, 5),
                             want=dict(outcome=[[255]], count=[2], source=[[-1, -2]], state=[[7, 6]])),
        "no_clutter_candidates": one([front], **QUIET, clutter_threshold=ALL, want=dict(outcome=[[D]], count=[1], source=[[0]])),
        "count_below_zero": one([front, rear], count=-3, **QUIET, want=dict(outcome=[[255, 255]], count=[0], state=[[0, 1]])),
        "count_above_np": one([front, person(0.0, 1.0)], count=99, **QUIET, want=dict(outcome=[[D, D]], count=[2], source=[[0, 1]])),
        # a NaN person is not reported and hides nobody
        "nan_person": one([person(NAN, 0.0), front, rear, person(0.0, float("inf"))], **QUIET,
                          want=dict(outcome=[[N, D, O, N]], count=[1], source=[[1]])),
        "nan_pose": one([front, rear, person(0.0, 1.0)], count=2, pose=(NAN, 0.0, 0.0), state=(3, 41), **QUIET,
                        want=dict(outcome=[[N, N, 255]], count=[0], state=[[3, 42]])),
        "counter_wraps": one([front], state=(ALL, ALL), **QUIET, want=dict(outcome=[[D]], count=[1], source=[[0]], state=[[ALL, 0]])),
        # an overflowed product is a NaN or an infinity in a comparison: nobody is hidden
        "overflow_hides_nobody": one([person(1e200, 0.0), person(2e200, 0.0)], **QUIET, want=dict(outcome=[[D, D]], count=[2], source=[[0, 1]])),
    }
    return cases


def check_want(new_state, outs, want):
    det, det_count, source, outcome = outs
    if "state" in want:
        assert np.asarray(new_state).tolist() == want["state"]
    assert det_count.tolist() == want["count"]
    assert np.asarray(outcome).tolist() == want["outcome"]
    for b, n in enumerate(det_count):
        if "source" in want:
            assert source[b, :n].tolist() == want["source"][b]
        if "rows" in want:
            assert det[b, :n].tobytes() == np.array(want["rows"][b], np.float64).reshape(n, 5).tobytes()
        assert np.isnan(det[b, n:]).all() and (source[b, n:] == -99).all()                # rows from det_count on: not written


SHAPES = ((1, 1, 0), (3, 4, 2), (8, 8, 4), (40, 64, 24), (64, 64, 64), (8, 4, 2))         # the last: Nd below the detected persons
BATCHES = (1, 5, 67)
TICKS = 10


def seeded_case(Np, Nd, Kc, B, seed):
    """Persons on a few bearings per robot (so that bodies line up), at 0.5 to 8 m, drifting from tick to tick; counts from
    -1 to Np + 1; a few NaN persons; one robot whose pose is NaN for a tick; the counters wrap inside the sequence."""
    rng = np.random.default_rng(seed)
    p = R.params(body_radius=0.25, p_miss=0.2, sigma=0.03, sigma_growth=0.002, clutter_candidates=Kc, p_clutter=0.3, clutter_range=5.0,
                 seed=0x123456789ABCDEF0, Nd=Nd)
    state0 = np.stack([100 + np.arange(B), np.full(B, 2 ** 32 - 4)], axis=1).astype(np.uint32)
    pose = np.concatenate([rng.uniform(-2.0, 2.0, (B, 2)), rng.uniform(-3.0, 3.0, (B, 1))], axis=1)
    lanes = rng.uniform(-np.pi, np.pi, (B, 1 + Np // 3))
    bearing = np.take_along_axis(lanes, rng.integers(0, lanes.shape[1], (B, Np)), axis=1) + rng.normal(0.0, 0.02, (B, Np))
    rng_m = rng.uniform(0.5, 8.0, (B, Np))
    ticks = []
    for t in range(TICKS):
        rng_m = np.clip(rng_m + rng.normal(0.0, 0.1, (B, Np)), 0.3, 9.0)
        bearing = bearing + rng.normal(0.0, 0.01, (B, Np))
        people = np.zeros((B, Np, 5))
        people[:, :, 0] = pose[:, None, 0] + rng_m * np.cos(bearing)
        people[:, :, 1] = pose[:, None, 1] + rng_m * np.sin(bearing)
        people[:, :, 2:4] = rng.normal(0.0, 0.5, (B, Np, 2))
        people[:, :, 4] = rng.integers(0, 3, (B, Np))
        bad = rng.random((B, Np)) < 0.03
        people[bad, rng.integers(0, 2, int(bad.sum()))] = np.where(rng.random(int(bad.sum())) < 0.5, np.nan, np.inf)
        tick_pose = pose.copy()
        if t == 4:
            tick_pose[B // 2, 1] = np.nan
        ticks.append(dict(people=people, count=rng.integers(-1, Np + 2, B).astype(np.int32), pose=tick_pose, want=None))
        pose[:, :2] += rng.normal(0.0, 0.05, (B, 2))
    return dict(p=p, state0=state0, ticks=ticks)


def seeded_cases():
    return {f"{Np}x{Nd}x{Kc}_B{B}": seeded_case(Np, Nd, Kc, B, 1000 * k + B) for k, (Np, Nd, Kc) in enumerate(SHAPES) for B in BATCHES}


def ref_call(state, tick, p, det=None, source=None, outcome=None):
    new, outs, _ = R.step(state, tick["people"], tick["count"], tick["pose"], p, det, source, outcome)
    return new, outs


def run(case, call):
    """[(t, tick, state before, new state, outputs)] of `call(state, tick, p) -> (new state, outputs)` fed its own state."""
    state, out = np.array(case["state0"], np.uint32), []
    for t, tick in enumerate(case["ticks"]):
        new, outs = call(state, tick, case["p"])
        out.append((t, tick, state, new, outs))
        state = new
    return out


def same(a, b):
    """Bit equality of (new state, (det, det_count, source, outcome)); a None output (a NULL pointer) matches anything."""
    (sa, oa), (sb, ob) = a, b
    pairs = [(sa, sb)] + [(x, y) for x, y in zip(oa, ob) if x is not None and y is not None]
    return all(np.asarray(x).dtype == np.asarray(y).dtype and np.asarray(x).shape == np.asarray(y).shape
               and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in pairs)


_reference = {}


def reference(name, case):
    """The yardstick's ticks of a case, computed once per process and frozen: [(tick, state before, new state, outputs, counters)]."""
    if name not in _reference:
        state, ticks = np.array(case["state0"], np.uint32), []
        for tick in case["ticks"]:
            new, outs, counters = R.step(state, tick["people"], tick["count"], tick["pose"], case["p"])
            for a in [state, new, *outs, tick["people"], tick["count"], tick["pose"]]:
                a.setflags(write=False)
            ticks.append((tick, state, new, outs, counters))
            state = new
        _reference[name] = ticks
    return _reference[name]
