"""The checkers on the inputs of tests/obstacle_edge_cases.py, without a device: before tests/test_gpu_obstacle_edges.py
holds the kernels to the oracle on these maps, the oracle's interpolation is held to a second statement of it and to a
statement of the clamp that shares no line with it, and the table is shown to reach what it is there for.

  oracle against pyref   the oracle's rows (residuals and Jacobian) against oracle/pyref.py on two scenes of every case. The
                         scenes are taken without their people: the obstacle rows do not read them, and pyref's agent loops
                         take seconds per scene.
  pad against crop       the oracle on a case (clamped taps) against the oracle on the same map edge-replicated by p cells
                         with origin - p * resolution (no tap clamped): ceres::Grid2D's clamp, stated on the data. The two
                         differ only by the rounding of (front - origin) / resolution.
                         Measured (x86-64, glibc 2.39): worst relative discrepancy 2.2e-11 over the table, against the bound
                         JAC_RTOL / 10 = 1e-10; the test prints the figure of the run.
  coverage               from the numpy rollout alone: every pair of (row band, column band) is hit on a noise map, on the
                         maps of the dword paths and on the maps of the byte path; the edge-in and edge-out cases have
                         exactly the lanes inside and outside that they claim; the table has the sizes, resolutions,
                         shapes and origins it is meant to have.
  builder check          one byte changed in a tap of a step's patch changes the oracle's row of that step.
  solve inputs           the smooth-map cases that go through the solve: the shares of well-conditioned and firm scenes of
                         the pool meet parity_checks.check_population's 0.97 and 0.9, and the obstacle term is live (with
                         the map zeroed the oracle's commands move by more than 1e-3 on at least half of the scenes).
                         Checked for the README weights with the seeds of the table (obstacle_edge_cases.SOLVE_CASES)."""
import numpy as np
import pytest

import obstacle_edge_cases as E
from conftest import cmd_err, well_conditioned

JAC_RTOL = 1e-9          # the project's K1 bound (test_gpu_instantiations.JAC_RTOL), relative to max(1, |value|)
ALL = list(E.CASES)


def rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(a))


def int_cells(name, x=None):
    prm, sc = E.make_case(name)
    return np.floor(E.cell_coordinates(prm, sc, sc.init_params if x is None else x)).astype(np.int64)


def test_smooth_maps_are_nowhere_constant():
    smooth = [n for n in ALL if E.CASES[n].kind == "smooth"]
    assert len(smooth) >= 7
    for name in smooth:
        sc = E.make_case(name)[1]
        assert E.constant_windows(sc.costmap) == 0, name
        assert sc.costmap.max() <= 253


@pytest.mark.parametrize("name", ALL)
def test_oracle_matches_pyref(oracle, name):
    from oracle import pyref
    prm, sc = E.make_case(name)
    pick = np.unique([(3 * len(name)) % sc.B, (3 * len(name) + 1 + 2 * (sc.B // 3)) % sc.B])
    sub = sc.select(pick)
    sub.has_people[:] = 0
    x = E.perturbed(sc)[pick]
    ev = oracle.evaluate(prm, sub, x)
    ref_rows, _ = E.obstacle_rows(prm, sc.T, False)
    for k in range(sub.B):
        r, J = pyref.evaluate(prm, sub, k, x[k])
        m = len(r)      # the oracle's arrays have the rows of a scene with people; a scene without leaves the rest zero
        assert m == prm.dims(sc.T, False)[4] and not ev["residuals"][k, m:].any() and not ev["jacobian"][k, m:].any()
        er, ej = rel(r, ev["residuals"][k, :m]), rel(J, ev["jacobian"][k, :m])
        assert er.max() < 1e-9 and ej.max() < 1e-9, (name, int(pick[k]), float(er.max()), float(ej.max()),
                                                      "obstacle" if er.argmax() in ref_rows else "other")
        assert np.abs(r[ref_rows]).max() > 0 or sc.costmap.min() == 0   # the rows compared are not all zero


def test_pad_against_crop(oracle):
    worst, where, n = 0.0, None, 0
    for name in ALL:
        prm, sc = E.make_case(name)
        p = E.pad_cells(prm, sc)
        if p is None:
            continue
        n += 1
        big = E.padded(sc, p)
        for x in (sc.init_params, E.perturbed(sc)):
            cc = np.floor(E.cell_coordinates(prm, big, x)).astype(np.int64)
            assert E.interior(cc[..., 0], cc[..., 1], big.size_x, big.size_y).all(), name   # no tap of the twin is clamped
            a, b = oracle.evaluate(prm, sc, x), oracle.evaluate(prm, big, x)
            for key in ("residuals", "jacobian"):
                e = float(rel(a[key], b[key]).max())
                assert e < JAC_RTOL / 10, (name, key, e)
                if e > worst:
                    worst, where = e, (name, key)
    assert n >= len(ALL) - 2    # only the cases a million cells away have no twin
    print(f"\n[pad against crop, oracle] worst relative discrepancy {worst:.2e} at {where} over {n} cases")


def test_coverage():
    hit = {"wide": set(), "narrow": set()}
    for name in ALL:
        c = E.CASES[name]
        if c.kind != "noise":
            continue
        cc = int_cells(name)
        cells = {(int(r), int(q)) for q, r in cc.reshape(-1, 2)}
        for r, q in cells:
            for rb in E.bands(r, c.size_y):
                for cb in E.bands(q, c.size_x):
                    hit["wide" if c.size_x >= 4 else "narrow"].add((rb, cb))
    # the dword paths: some case has both sizes >= 6, so every pair of the ten bands can exist
    assert hit["wide"] == {(rb, cb) for rb in E.BANDS for cb in E.BANDS}, set(E.BANDS) - hit["wide"]
    # the byte path (size_x <= 3: no column band 2 .. size-4; size_y = 9 has every row band)
    assert hit["narrow"] == {(rb, cb) for rb in E.BANDS for cb in E.possible_bands(3)}


@pytest.mark.parametrize("name", [n for n in ALL if E.CASES[n].claim])
def test_edge_cases_have_the_lanes_they_claim(name):
    c = E.CASES[name]
    _, axis, which, inside = c.claim
    cc = int_cells(name)
    col, row = cc[..., 0], cc[..., 1]
    inn = E.interior(col, row, c.size_x, c.size_y)
    along, size = (col, c.size_x) if axis == "x" else (row, c.size_y)
    last_in, first_out = (1, 0) if which == "min" else (size - 3, size - 2)
    if inside:   # every lane interior, at least one of every scene on the last interior cell
        assert inn.all()
        assert ((along == last_in).sum(axis=1) >= 1).all()
    else:        # exactly one lane of every scene is out, by one cell on the named axis alone; all others are interior
        assert ((~inn).sum(axis=1) == 1).all()
        assert ((along == first_out).sum(axis=1) == 1).all()
        assert ((along == last_in).sum(axis=1) >= 1).all() or c.shape == "t1"


def test_the_table_has_what_it_names():
    C = E.CASES
    sizes = {(c.size_x, c.size_y) for c in C.values()}
    assert sizes >= {(sx, sy) for sx in (1, 2, 3) for sy in (1, 3, 9)}
    assert sizes >= {(sx, sy) for sx in (4, 5) for sy in (1, 2, 3, 4, 7)}
    assert sizes >= {(37, 9), (9, 37), (64, 40), (40, 64)}
    assert {c.resolution for c in C.values()} == {0.025, 0.05, 0.1, 0.3}
    assert {c.shape for c in C.values()} == set(E.SHAPES)
    assert any(c.B % 2 for c in C.values()) and all(c.B <= 64 for c in C.values())
    assert any(c.shared for c in C.values()) and any(not c.shared for c in C.values())
    assert any(c.no_people for c in C.values())
    for sx, sy in ((64, 40), (40, 64)):
        claims = {c.claim for c in C.values() if c.claim and (c.size_x, c.size_y) == (sx, sy)}
        assert claims == {("edge", a, w, i) for a in "xy" for w in ("min", "max") for i in (True, False)}
    origins = np.concatenate([E.make_case(n)[1].costmap_origin for n in C])
    assert (origins < 0).any() and (np.abs(origins) > 900).any()
    frac = np.abs(origins / 0.05 - np.round(origins / 0.05))
    assert (frac > 1e-3).any()       # origins that are no multiple of the resolution
    # far-off placements: 3, 10 and 1e6 cells, on every side and corner
    for cells in (3, 10, 10 ** 6):
        names = [n for n in C if n.startswith(f"far_{cells}_")]
        assert names
        sides = set()
        for n in names:
            c, cc = C[n], int_cells(n)
            lo_, hi_ = cc.min(axis=1), cc.max(axis=1)      # [B, 2]
            for b in range(cc.shape[0]):
                sx = -1 if hi_[b, 0] < -cells else 1 if lo_[b, 0] >= c.size_x + cells else 0
                sy = -1 if hi_[b, 1] < -cells else 1 if lo_[b, 1] >= c.size_y + cells else 0
                sides.add((sx, sy))
        assert sides >= set(E.DIRECTIONS), (cells, sides)
    # mixed waves: even scenes interior and odd scenes off the map, the reverse, and border-crossing scenes
    for name, inner in (("mixed_even_in", 0), ("mixed_odd_in", 1)):
        c, cc = C[name], int_cells(name)
        inn = E.interior(cc[..., 0], cc[..., 1], c.size_x, c.size_y)
        assert inn[inner::2].all() and not inn[1 - inner::2].any()
    for name in ("crossing", "crossing_helpers", "solve_crossing"):
        c, cc = C[name], int_cells(name)
        on = (cc[..., 0] >= 0) & (cc[..., 0] < c.size_x) & (cc[..., 1] >= 0) & (cc[..., 1] < c.size_y)
        assert (on.any(axis=1) & (~on).any(axis=1)).all(), name


@pytest.mark.parametrize("name", ALL)
def test_a_changed_byte_changes_the_row(oracle, name):
    """Guards the builder against placing trajectories where nothing is read: for a few (scene, step) of every case, each of
    the 16 taps of the step's patch (clamped into the map) is changed in turn and the oracle's obstacle residual of that
    step must change. On an axis where the step lies within 0.01 of a cell boundary only the tap on that boundary is taken
    (the other three taps of a Catmull-Rom spline have weight zero there)."""
    prm, sc = E.make_case(name)
    c = E.CASES[name]
    coords = E.cell_coordinates(prm, sc, sc.init_params)
    for b in sorted({0, sc.B // 2, sc.B - 1}):
        i = sc.T // 2
        one = sc.select([b])
        hp = bool(one.has_people[0])
        row = E.obstacle_rows(prm, sc.T, hp)[0][i]
        base = oracle.evaluate(prm, one, one.init_params, jacobian=False)["residuals"][0, row]
        q, r = np.floor(coords[b, i]).astype(np.int64)
        fq, fr = coords[b, i] - np.floor(coords[b, i])
        near = lambda f: (1,) if f < 0.01 else (2,) if f > 0.99 else range(4)
        taps = {(min(max(r - 1 + di, 0), c.size_y - 1), min(max(q - 1 + dj, 0), c.size_x - 1))
                for di in near(fr) for dj in near(fq)}
        for rr, qq in sorted(taps):
            mod = one.select([0])
            mod.costmap = mod.costmap.copy()
            mod.costmap[0, rr, qq] ^= 0x80
            got = oracle.evaluate(prm, mod, mod.init_params, jacobian=False)["residuals"][0, row]
            assert got != base, (name, b, i, (int(rr), int(qq)))


_solve_pool = {}


def solve_inputs(oracle):
    """per solve case: (oracle result under the device's theta convention, stable, firm, moved by zeroing the map)"""
    if not _solve_pool:
        for name in E.SOLVE_CASES:
            prm, sc = E.make_case(name)
            rz = oracle.solve(prm, sc, nthreads=16, theta_zero_convention=True)
            stable = well_conditioned(oracle, prm, sc, rz, nthreads=16, theta_zero_convention=True, samples=2)
            flat = sc.select(np.arange(sc.B))
            flat.costmap = np.zeros_like(sc.costmap)
            r0 = oracle.solve(prm, flat, nthreads=16, theta_zero_convention=True)
            _solve_pool[name] = (rz, stable, (rz["marginal_decisions"] == 0) & stable, cmd_err(rz["cmds"], r0["cmds"]) > 1e-3)
    return _solve_pool


def test_solve_inputs_are_well_conditioned_and_the_obstacle_term_is_live(oracle):
    pool = solve_inputs(oracle)
    stable = np.concatenate([v[1] for v in pool.values()])
    firm = np.concatenate([v[2] for v in pool.values()])
    live = np.concatenate([v[3] for v in pool.values()])
    print(f"\n[solve inputs] {len(stable)} scenes: stable {stable.mean():.3f}, firm {firm.mean():.3f}, "
          f"moved by zeroing the map {live.mean():.3f}; per case " +
          " ".join(f"{n}={v[2].mean():.2f}/{v[3].mean():.2f}" for n, v in pool.items()))
    assert stable.mean() >= 0.97 and firm.mean() >= 0.9
    assert live.mean() >= 0.5
