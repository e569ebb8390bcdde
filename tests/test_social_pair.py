"""The near-axis pairs of tests/social_pair_cases.py on the CPU: every generated pair meets its conditions by the mpmath
statement alone, the checkers of the three kernels (tests/crowd_ref.py, oracle/pyref_sfm.py, the host C++ mirror) agree with
that statement on them, and the scenes that tests/test_gpu_social_pair.py runs keep the margins of the existing case files
everywhere except at the designed pair."""
import math

import mpmath as mp
import numpy as np
import pytest

import crowd_cases as G
import crowd_pool_cases as PC
import crowd_ref as R
import social_pair_cases as S
from test_projection import host_project, hostlib, pyref_project  # noqa: F401  (hostlib is a fixture)


def _factor_two(dist, target):
    return abs(target) / 2 <= dist <= 2 * abs(target)


def test_every_generated_pair_meets_its_conditions():
    least_jump, n = math.inf, 0
    for near_pi, target, k, me, pa in S.all_pairs():
        signs = []
        for a, b in ((me, pa), (pa, me)):
            dist, sign, jump = S.conditions_mp(*S.ordered(a, b), near_pi)
            assert _factor_two(dist, target), (near_pi, target, k, dist)
            assert jump >= S.MIN_JUMP, (near_pi, target, k, jump)
            signs.append(sign)
            least_jump = min(least_jump, jump)
            n += 1
        assert signs[0] == signs[1] == (1 if target > 0 else -1)      # (near pi: theta = sign(target) pi - target)
    print(f"{n} ordered pairs, none rejected; smallest 2 F |fa| dt = {least_jump:.3e}")
    assert n == 2 * len(S.FAMILIES) * len(S.TARGETS) * S.PER_TARGET


def test_crowd_ref_agrees_with_the_40_digit_term():
    """Measured: max |df| = 5.1e-16 over the 2880 ordered pairs and the exact rows. The bound 1e-14 is about 20 times that:
    the term is below 4.2 in magnitude and goes through a few dozen roundings."""
    worst = 0.0
    rows = [(a, b) for _, _, _, a, b in S.all_pairs()] + [(r["me"], r["partner"]) for r in S.EXACT_ROWS]
    for me, pa in rows:
        for a, b in ((me, pa), (pa, me)):
            args = S.ordered(a, b)
            fx, fy = R.social_term(*args)
            mx, my, _ = S.social_term_mp(*args)
            worst = max(worst, abs(float(fx - mx)), abs(float(fy - my)))
    print(f"crowd_ref.social_term against the {S.DIGITS}-digit term: max |df| = {worst:.3e}")
    assert worst <= 1e-14


def test_exact_rows_are_exact_in_the_checker_and_at_40_digits():
    for r in S.EXACT_ROWS:
        me, pa, ax = r["me"], r["partner"], r["axis"]
        terms = []
        for a, b in ((me, pa), (pa, me)):
            args = S.ordered(a, b)
            theta = R.pair_theta(*args)[0]
            f = R.social_term(*args)
            m = S.social_term_mp(*args)
            if r["kind"] == "head_on":
                assert theta == 0.0 and m[2] == 0, r["name"]
                assert f[1 - ax] == 0.0 and m[1 - ax] == 0 and abs(f[ax]) > 1e-3, r["name"]     # no lateral force: fa = 0
            else:
                with mp.workdps(S.DIGITS):
                    assert theta == math.pi and m[2] == +mp.pi, r["name"]
                assert abs(f[1 - ax]) * 2 * S.DT >= S.MIN_JUMP, r["name"]
            terms.append(f)
        assert terms[0][0] == -terms[1][0] and terms[0][1] == -terms[1][1], r["name"]          # exact negatives
    assert sum("negzero" in r["name"] for r in S.EXACT_ROWS) == 8
    r = next(r for r in S.EXACT_ROWS if r["name"] == "head_on_x+_negzero")
    assert math.copysign(1.0, S.ordered(r["me"], r["partner"])[1]) == -1.0


# ---- the projection's checker and the host mirror, through one-step scenes ------------------------------------------------
def _one_step_scenes():
    return [(f, t, S.projection_case(S.pairs(f, t)[k], "pr", 1, (0,), 1, 100 + k)) for f in S.FAMILIES for t in S.TARGETS
            for k in (0, 1)]


def _step_mp(c):
    """The person's position and velocity after the one step of a `pr` scene with N = 1, T = 1 at DIGITS digits: desired +
    social (social_term_mp) + obstacle force, then updatePosition. The velocities start from the doubles that
    oracle/pyref_sfm.py forms from yaw and speed; the obstacle is the grid's entry 0, at its origin."""
    with mp.workdps(S.DIGITS):
        f = lambda v: mp.mpf(float(v))
        me, rob = (S.as_walked(*s) for s in c["designed"])
        dt, maxtime = f(np.float32(c["dt"])), f(np.float32(c["max_time"]))
        px, py, vx, vy = (f(v) for v in me)
        gx, gy = px + maxtime * vx, py + maxtime * vy
        gd = mp.sqrt((gx - px) ** 2 + (gy - py) ** 2)
        if gd > mp.mpf("0.25"):
            fx, fy = 2 * ((gx - px) / gd * mp.mpf("0.5") - vx) / mp.mpf("0.5"), 2 * ((gy - py) / gd * mp.mpf("0.5") - vy) / mp.mpf("0.5")
        else:
            fx, fy = -vx / mp.mpf("0.5"), -vy / mp.mpf("0.5")
        sx, sy, _ = S.social_term_mp(*S.ordered(me, rob))
        # computeObstacle stores agent - obstacle and the force uses agent - that: the obstacle's own position, here the origin
        ox, oy = f(c["origin"][0]), f(c["origin"][1])
        on = mp.sqrt(ox * ox + oy * oy)
        e = 20 * mp.exp(-(on - mp.mpf("0.5")) / mp.mpf("0.2"))
        fx, fy = fx + sx + e * ox / on, fy + sy + e * oy / on
        vx, vy = vx + fx * dt, vy + fy * dt
        sp = mp.sqrt(vx * vx + vy * vy)
        if sp > mp.mpf("0.5"):
            vx, vy = vx / sp * mp.mpf("0.5"), vy / sp * mp.mpf("0.5")
        return px + vx * dt, py + vy * dt, vx, vy


def test_pyref_sfm_agrees_with_the_40_digit_step():
    """Measured: max |d position| = 5.4e-17, max |d velocity| = 1.5e-16 over 72 one-step scenes (the velocity rebuilt from the
    checker's speed and yaw). The bound 5e-15 is about 30 times the larger of them, the margin crowd_ref's term has: a
    velocity below 3 and a force below about 10 times dt = 0.05, through a few dozen roundings. A wrong sign would move
    the velocity by at least MIN_JUMP = 1e-6."""
    worst_p = worst_v = 0.0
    for near_pi, target, c in _one_step_scenes():
        for (dist, sign) in S.projection_conditions(c, near_pi):
            assert _factor_two(dist, target) and sign == (1 if target > 0 else -1), (near_pi, target, dist)
        want = _step_mp(c)
        got = pyref_project(c, convention=True)[1, 0]                # x, y, yaw, t, lv, av after the step
        gv = (got[4] * math.cos(got[2]), got[4] * math.sin(got[2]))
        worst_p = max(worst_p, abs(float(got[0] - want[0])), abs(float(got[1] - want[1])))
        worst_v = max(worst_v, abs(float(gv[0] - want[2])), abs(float(gv[1] - want[3])))
    print(f"pyref_sfm.project_people against the {S.DIGITS}-digit step: max |dp| = {worst_p:.3e}, max |dv| = {worst_v:.3e}")
    assert worst_p <= 5e-15 and worst_v <= 5e-15


def test_host_cpp_mirror_agrees_with_pyref_sfm_on_the_one_step_scenes(hostlib):
    worst = 0.0
    for near_pi, target, c in _one_step_scenes():
        rc, got, _ = host_project(hostlib, c)
        assert rc == 0
        worst = max(worst, float(np.max(np.abs(got - pyref_project(c)))))
    print(f"host C++ mirror against pyref_sfm: max |d| = {worst:.3e}")
    assert worst < 1e-11


# ---- the scenes of tests/test_gpu_social_pair.py ---------------------------------------------------------------------------
def _designed_conditions(me, pa, near_pi, target, what):
    for a, b in ((me, pa), (pa, me)):
        dist, sign, jump = S.conditions_mp(*S.ordered(a, b), near_pi)
        assert _factor_two(dist, target) and jump >= S.MIN_JUMP and sign == (1 if target > 0 else -1), (what, dist, jump)


@pytest.mark.parametrize("name", sorted(S.CROWD_SCENES))
def test_crowd_scenes_keep_the_margins_except_at_the_designed_pair(name):
    d, tags = S.crowd_scene(name)
    m = S.crowd_margins(d)
    print(name, m)
    for k, v in G.CONDITIONS.items():
        assert m[k] >= v, (name, k, m[k])
    assert len(tags) == len(d["designed"]) > 0
    for (b, i, j), (near_pi, target) in zip(d["designed"], tags):
        me = d["people"][b, i, 0:4]
        pa = d["people"][b, j, 0:4] if j >= 0 else S.robot_state(d, b)
        if target is not None:
            _designed_conditions(me, pa, near_pi, target, (name, b))
        if j < 0 and target is not None:                             # the robot: its velocity from the (yaw, v) passed
            for dist, sign in S.robot_conditions(d, b, near_pi):
                assert _factor_two(dist, target) and sign == (1 if target > 0 else -1), (name, b, dist)


def test_pool_scene_keeps_the_margins_except_at_the_designed_pairs():
    c, tags = S.pool_scene()
    m = S.pool_margins(c)
    print(m)
    assert m["theta"] >= G.CONDITIONS["theta"] and m["pair"] >= G.CONDITIONS["pair"] and m["partners"] == 1 + S.POOL_GENERIC
    for k, v in PC.CONDITIONS.items():
        assert m[k] >= v, (k, m[k])
    for (i, j), (near_pi, target) in zip(c["designed"], tags):
        a = c["agents"]
        assert math.hypot(a[i, 0] - a[j, 0], a[i, 1] - a[j, 1]) < c["range"]
        if target is not None:
            _designed_conditions(a[i, 0:4], a[j, 0:4], near_pi, target, (i, j))


@pytest.mark.parametrize("name", sorted(S.PROJECTION_SCENES))
def test_projection_scenes_keep_the_margins_except_at_the_designed_pair(name):
    for near_pi, target, c in S.projection_scene(name):
        assert S.projection_margin(c) >= S.GENERIC / 2, name          # (G.CONDITIONS["theta"])
        if target is not None:
            for dist, sign in S.projection_conditions(c, near_pi):
                assert _factor_two(dist, target) and sign == (1 if target > 0 else -1), (name, near_pi, target, dist)
        else:                                                        # an exact row: near_pi holds its name
            a, b = (S.as_walked(*q) for q in c["designed"])
            for p, q in ((a, b), (b, a)):
                assert R.pair_theta(*S.ordered(p, q))[0] == (0.0 if near_pi.startswith("head_on") else math.pi), near_pi
