"""People projection: Optimizer::project_people + SFM. Three statements of it are compared:
oracle/pyref_sfm.py (numpy, the checker), the C++ host adapter (CPU) and the HIP kernel behind
smpc_project_people_batch (GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nav2_social_mpc_controller_amd", "host")


def make_case(seed, N=3, n_valid=2, T=28, grid=120, valid_rows=None):
    """valid_rows: the rows of init_people that hold the valid agents (default: the first n_valid)"""
    rng = np.random.default_rng(seed)
    init = np.zeros((N, 6))
    init[:, 3] = -1.0
    for a in (range(n_valid) if valid_rows is None else valid_rows):
        r, phi, hd = rng.uniform(0.8, 3.0), rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi, np.pi)
        lv = 0.0 if rng.uniform() < 0.2 else rng.uniform(0.2, 1.2)
        init[a] = [r * np.cos(phi), r * np.sin(phi), hd, 0.0, lv, 0.0]
    dt = float(np.float32(0.05))
    path = np.zeros((T + 1, 6))
    x = y = 0.0
    th, w = rng.uniform(-np.pi, np.pi), rng.uniform(-0.6, 0.6)
    for k in range(T + 1):
        path[k] = [x, y, th, k * dt, 0.6 if k else rng.uniform(0, 0.6), w]
        x, y, th = x + 0.6 * np.cos(th) * dt, y + 0.6 * np.sin(th) * dt, th + w * dt
    # nearest-obstacle grid: a handful of obstacle cells, every cell points at the closest one
    res, origin = np.float32(0.1), np.array([-6.0, -6.0])
    obs = rng.integers(0, grid, size=(5, 2))
    yy, xx = np.mgrid[0:grid, 0:grid]
    d = (xx[None] - obs[:, 0, None, None]) ** 2 + (yy[None] - obs[:, 1, None, None]) ** 2
    near = obs[np.argmin(d, axis=0)]
    idx = (near[..., 0] + near[..., 1] * grid).astype(np.uint32)
    return dict(init=init, path=path, idx=idx, origin=origin, res=float(res), max_time=1.5, dt=0.05, T=T, N=N, grid=grid)


def pyref_project(c, convention=False):
    from oracle import pyref_sfm
    od = dict(width=c["grid"], height=c["grid"], resolution=c["res"], origin_x=c["origin"][0], origin_y=c["origin"][1], indexes=c["idx"])
    return pyref_sfm.project_people(c["init"], c["path"], od, c["max_time"], c["dt"], theta_zero_convention=convention)  # [T+1][N][6]


@pytest.fixture(scope="module")
def hostlib():
    subprocess.check_call(["make", "-C", HOST, "-s"])
    lib = C.CDLL(os.path.join(HOST, "libsmpc_host.so"))
    lib.smpc_host_project_people.restype = C.c_int
    lib.smpc_host_project_people.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                             C.c_double, C.c_double, C.c_float, C.c_float, C.c_void_p, C.c_char_p, C.c_int]
    return lib


def host_project(lib, c):
    out = np.zeros((c["T"] + 1, c["N"], 6))
    err = C.create_string_buffer(256)
    idx = np.ascontiguousarray(c["idx"], np.uint32)
    rc = lib.smpc_host_project_people(np.ascontiguousarray(c["init"]).ctypes.data, c["N"], np.ascontiguousarray(c["path"]).ctypes.data,
                                      c["T"], idx.ctypes.data, c["grid"], c["grid"], c["res"], c["origin"][0], c["origin"][1],
                                      c["max_time"], c["dt"], out.ctypes.data, err, 256)
    return rc, out, err.value.decode()


@pytest.mark.parametrize("seed,n_valid", [(1, 2), (2, 3), (3, 1), (4, 0)])
def test_host_cpp_matches_numpy_restatement(hostlib, seed, n_valid):
    c = make_case(seed, n_valid=n_valid)
    want = pyref_project(c)
    rc, got, _ = host_project(hostlib, c)
    assert rc == 0
    assert np.max(np.abs(got - want)) < 1e-11
    assert np.all(want[1:, n_valid:, 3] == -1.0)                      # padded phantoms after the valid agents


def test_host_cpp_quirks(hostlib):
    c = make_case(5)
    c100 = dict(c, grid=100, idx=np.zeros((100, 100), np.uint32))     # 100 x 100 grid: every person is dropped
    rc, got, _ = host_project(hostlib, c100)
    assert rc == 0 and np.all(got[1:, :, 3] == -1.0) and np.array_equal(got[0], c["init"])
    far = dict(c, init=c["init"].copy())
    far["init"][0, 0] = 1e3                                           # off the distance grid: the reference throws
    rc, _, msg = host_project(hostlib, far)
    assert rc == -1 and "out of bounds" in msg


@pytest.mark.gpu
def test_hip_projection_matches_restatements(hostlib):
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme())
    # N + 1 lanes per scene rounded up to a power of two: 4, 16, 32 and (N = 40, 63) the whole wavefront
    for N, n_valid in ((3, 2), (3, 3), (3, 0), (8, 6), (16, 16), (40, 37), (63, 63)):
        cases = [make_case(100 + 7 * N + i, N=N, n_valid=n_valid) for i in range(6 if N <= 16 else 2)]
        init = np.stack([c["init"] for c in cases])
        path = np.stack([c["path"] for c in cases])
        idx = np.stack([c["idx"] for c in cases])
        origin = np.stack([c["origin"] for c in cases])
        got, err = s.project_people(init, path, idx, origin, cases[0]["res"], cases[0]["max_time"], cases[0]["dt"])
        assert np.all(err == 0)
        for b, c in enumerate(cases):
            # checker under the theta := 0 convention for exactly equal velocities (two standing people at step 0)
            want = pyref_project(c, convention=True)                  # [T+1][N][6]
            assert np.max(np.abs(got[b].transpose(0, 2, 1) - want)) < 1e-9, (N, n_valid, b)
            literal = pyref_project(c)
            if N == 3 and np.max(np.abs(literal - want)) == 0.0:      # no libm-noise decision in this case
                rc, hostres, _ = host_project(hostlib, c)
                assert rc == 0 and np.max(np.abs(got[b].transpose(0, 2, 1) - hostres)) < 1e-9


@pytest.fixture(scope="module")
def projector():
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    s = BatchSolver(OptimizerParams.readme())
    yield s
    s.close()


_want = {}


def want_of(key, c):
    """the checker's projection of a case (theta := 0 for exactly equal velocities), computed once per key"""
    if key not in _want:
        _want[key] = pyref_project(c, convention=True)            # [T+1][N][6]
    return _want[key]


def project_cases(s, cases):
    got, err = s.project_people(np.stack([c["init"] for c in cases]), np.stack([c["path"] for c in cases]),
                                np.stack([c["idx"] for c in cases]), np.stack([c["origin"] for c in cases]), cases[0]["res"],
                                cases[0]["max_time"], cases[0]["dt"])
    assert np.all(err == 0)
    return got                                                    # [B][T+1][6][N]


def check_cases(got, cases, keys, what):
    worst = 0.0
    for b, (c, key) in enumerate(zip(cases, keys)):
        d = float(np.max(np.abs(got[b].transpose(0, 2, 1) - want_of(key, c))))
        assert d < 1e-9, (what, key, d)
        worst = max(worst, d)
    print(f"{what}: {len(cases)} scenes, max difference {worst:.3e}")


# The pair rounds of the kernel: lane g takes partner (g + k) mod n_act, n_act = n_valid + 1; with H copies of a scene in
# the wavefront (H = 2 while N + 1 <= 32 lanes) copy hh takes the rounds 1 + hh, 1 + hh + H, ..., two of them per trip; for
# even n_act the last round k = n_act / 2 is the mutual one. Which copy and which slot of a trip it lands in, and whether a
# trip's second slot is filled, goes with n_act mod 4 (H = 2) or mod 2 (H = 1): every n_valid covers every class.
@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 3, 7, 8, 15, 16, 31, 40, 63])
def test_hip_projection_every_pairing_class(projector, N):
    valid = range(N + 1) if N <= 16 else range(N - 3, N + 1)
    cases = [make_case(3000 + 100 * N + n, N=N, n_valid=n, T=4) for n in valid]
    if 3 <= N <= 16:
        assert {(n + 1) % 4 for n in valid} == {0, 1, 2, 3}
    check_cases(project_cases(projector, cases), cases, [("sweep", N, n) for n in valid], f"N = {N}, n_valid = {list(valid)}")


PHANTOMS = {3: [[1, 2], [0, 2], [1]], 8: [[1, 2, 3, 4, 5, 6, 7], [0, 3, 4, 7], [1, 3, 5, 7], [0, 2, 4, 6], [7]],
            16: [list(range(1, 16)), [0, 1, 14, 15], list(range(0, 16, 2)), list(range(1, 16, 2)), [5, 11, 15]]}


@pytest.mark.gpu
@pytest.mark.parametrize("N", sorted(PHANTOMS))
def test_hip_projection_phantoms_between_valid_agents(projector, N):
    """invalid rows (t = -1) first, in the middle and alternating: step 0 is init_people as given, from step 1 on the valid
    agents stand compacted at the front and phantoms behind them, as in the checker"""
    cases = [make_case(4000 + 100 * N + k, N=N, T=4, valid_rows=rows) for k, rows in enumerate(PHANTOMS[N])]
    got = project_cases(projector, cases)
    check_cases(got, cases, [("phantoms", N, k) for k in range(len(cases))], f"N = {N}, phantoms in the middle")
    for b, (c, rows) in enumerate(zip(cases, PHANTOMS[N])):
        assert np.array_equal(got[b, 0].T, c["init"])
        assert np.all(got[b, 1:, 3, :len(rows)] >= 0.0) and np.all(got[b, 1:, 3, len(rows):] == -1.0)
        assert c["init"][rows[0], 3] == 0.0 and (c["init"][:, 3] == -1.0).sum() == N - len(rows) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("B,N", [(19, 3), (35, 1), (5, 8)])
def test_hip_projection_several_blocks_of_shared_waves(projector, B, N):
    """8, 16 and 2 scenes per wave in 3 blocks, the last one partly filled; every scene is another one and is checked
    against its own checker result; a scene's rows do not depend on the batch"""
    cases = [make_case(5000 + 100 * N + b, N=N, n_valid=N - (b % 2 if N > 1 else 0), T=4) for b in range(B)]
    per_wave = {3: 8, 1: 16, 8: 2}[N]
    assert -(-B // per_wave) == 3 and B % per_wave != 0
    got = project_cases(projector, cases)
    check_cases(got, cases, [("blocks", N, b) for b in range(B)], f"B = {B}, N = {N}")
    for b in (0, per_wave + 1, B - 1):                            # block 0, a later lane group of block 1, the last scene
        alone = project_cases(projector, cases[b:b + 1])
        assert alone[0].tobytes() == got[b].tobytes(), b


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2])
def test_hip_projection_shortest_horizons(projector, T):
    """T = 1: the robot's prefetched row min(i + 1, T - 1) is row 0 again"""
    cases = [make_case(6000 + 10 * T + k, N=3, n_valid=n, T=T) for k, n in enumerate((3, 2, 1, 0))]
    got = project_cases(projector, cases)
    assert got.shape == (4, T + 1, 6, 3)
    check_cases(got, cases, [("horizon", T, k) for k in range(4)], f"T = {T}")


@pytest.mark.gpu
def test_hip_projection_error_flags_and_grid_quirk():
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    from nav2_social_mpc_controller_amd.solver import BatchSolver, SmpcError
    s = BatchSolver(OptimizerParams.readme())
    c = make_case(9)
    bad = c["init"].copy()
    bad[0, 0] = 1e3
    init = np.stack([c["init"], bad])
    path = np.stack([c["path"], c["path"]])
    got, err = s.project_people(init, path, c["idx"][None], c["origin"][None], c["res"], c["max_time"], c["dt"])
    assert err.tolist() == [0, 1]                                     # scene 1: cell out of bounds (reference throws)
    idx100 = np.zeros((1, 100, 100), np.uint32)
    got, err = s.project_people(init[:1], path[:1], idx100, c["origin"][None], c["res"], c["max_time"], c["dt"])
    assert np.all(got[0, 1:, 3, :] == -1.0)                           # "NOT valid" grid: every person dropped
    with pytest.raises(SmpcError):
        s.project_people(init[:1], path[:1], np.zeros((1, 0, 0), np.uint32), c["origin"][None], c["res"], c["max_time"], c["dt"])


@pytest.mark.gpu
def test_projection_feeds_the_solver(oracle):
    """f1 -> hot path on the GPU: project the people with the HIP kernel, solve with the HIP kernel, check against
    the numpy projection + CPU oracle."""
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    from nav2_social_mpc_controller_amd.scenes import make_scenes
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    prm = OptimizerParams.readme()
    sc = make_scenes(prm, 8, 3, n_valid=3, map_cells=80, seed=77, standing_fraction=0.0)
    s = BatchSolver(prm)
    T = sc.T
    grid = 200
    idx = np.full((1, grid, grid), 5 + 7 * grid, np.uint32)
    origin = np.array([[-15.0, -15.0]])
    init = np.ascontiguousarray(sc.people[:, 0].transpose(0, 2, 1))                # [B][N][6]
    th = np.arctan2(np.diff(sc.path_pts[:, :, 1], axis=1), np.diff(sc.path_pts[:, :, 0], axis=1))
    th = np.concatenate([th, th[:, -1:]], axis=1)
    rpath = np.zeros((sc.B, T + 1, 6))
    rpath[:, :, 0:2], rpath[:, :, 2], rpath[:, :, 4] = sc.path_pts, th, 0.6
    proj, err = s.project_people(init, rpath, idx, origin, 0.15, 1.5, 0.05)
    assert np.all(err == 0)
    sc.people = np.ascontiguousarray(proj)
    from oracle import pyref_sfm
    od = dict(width=grid, height=grid, resolution=0.15, origin_x=-15.0, origin_y=-15.0, indexes=idx[0])
    for b in range(sc.B):
        want = pyref_sfm.project_people(init[b], rpath[b], od, 1.5, 0.05, theta_zero_convention=True)
        assert np.max(np.abs(proj[b].transpose(0, 2, 1) - want)) < 1e-9
    ref = oracle.solve(prm, sc, theta_zero_convention=True)
    got = s.solve(sc)
    firm = ref["marginal_decisions"] == 0
    assert firm.any()
    assert np.max(np.abs(got["cmds"][firm] - ref["cmds"][firm])) <= 1e-5


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_gpu_projection_terminates_on_absurd_angles():
    """The reference normalises angles with +-2 pi loops; a caller-supplied yaw of 1e15 / inf / NaN must not spin a
    wave (finite inputs are pre-reduced with fmod, non-finite ones come out as NaN)."""
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    from nav2_social_mpc_controller_amd.solver import BatchSolver
    c = make_case(31, N=3, n_valid=3)
    init = np.repeat(c["init"][None], 4, axis=0)
    init[1, 0, 2] = 1e15
    init[2, 1, 2] = np.inf
    init[3, 2, 2] = np.nan
    path = np.repeat(c["path"][None], 4, axis=0)
    s = BatchSolver(OptimizerParams.readme())
    got, err = s.project_people(init, path, c["idx"][None], c["origin"][None], c["res"], c["max_time"], c["dt"])
    want = pyref_project(c, convention=True)
    assert np.max(np.abs(got[0].transpose(0, 2, 1) - want)) < 1e-9          # the clean scene is unaffected
    assert np.isfinite(got[1][:, :2]).all()                                 # huge yaw: positions stay finite
