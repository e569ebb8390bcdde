"""smpc_local_costmap_batch on the device against tests/local_costmap_ref.py, bit for bit: cell, moved, every byte of
costmap, and costmap_origin as raw 64-bit patterns. Window sizes that take the 16-byte path (16 x 16, 80 x 80, 200 x 200) and
the byte path (5 x 3, 37 x 29, and a 16 x 16 window on a costmap that is not 16-byte aligned), worlds of 61 x 47 and 256 x 192
cells, B = 67 and B = 1, a shared world and a world per robot, host and device pointers."""
import numpy as np
import pytest

import local_costmap_ref as LR

pytestmark = pytest.mark.gpu

SIZES = [(5, 3), (16, 16), (37, 29), (80, 80), (200, 200)]     # (size_x, size_y)
WORLDS = [(61, 47), (256, 192)]                                 # (world_x, world_y)
B, RES = 67, 0.05
W0 = np.array([-2.35, 1.6])


def target_cells(size, world):
    """(67 window cells, their class names): where the case puts its windows, by hand and then seeded."""
    (sx, sy), (Hx, Hy) = size, world
    cells, names = [], []
    fits = sx <= Hx and sy <= Hy
    # sixteen consecutive columns: every source x-residue mod 16; inside the world where the window fits
    for k in range(16):
        cells.append((k + (1 if fits and Hx - sx > 16 else 0), (k % max(Hy - sy, 1)) if fits else -1 - k % 3))
        names.append("inside" if fits and cells[-1][0] + sx <= Hx else "residue")
    left, right, up, down = -3, Hx - sx + 3, -2, Hy - sy + 2      # three / two cells over each side
    mid_x, mid_y = (Hx - sx) // 2, (Hy - sy) // 2
    for name, c in (("left", (left, mid_y)), ("right", (right, mid_y)), ("top", (mid_x, up)), ("bottom", (mid_x, down)),
                    ("top-left", (left, up)), ("top-right", (right, up)), ("bottom-left", (left, down)), ("bottom-right", (right, down)),
                    ("outside", (Hx + 5, mid_y)), ("outside", (-sx - 1, mid_y)), ("outside", (mid_x, Hy)), ("outside", (mid_x, -sy)),
                    ("outside", (-sx, -sy - 7)), ("around", (-(sx - Hx) // 2 if sx > Hx else 0, -(sy - Hy) // 2 if sy > Hy else 0))):
        cells.append(c)
        names.append(name)
    g = np.random.default_rng(sx * 1000 + Hx)
    while len(cells) < B:
        cells.append((int(g.integers(-sx - 2, Hx + 3)), int(g.integers(-sy - 2, Hy + 3))))
        names.append("seeded")
    return np.array(cells, np.int32), names


def overlap_class(cell, size, world):
    """What a window at `cell` does with the world, from the geometry alone."""
    (cx, cy), (sx, sy), (Hx, Hy) = cell, size, world
    if cx >= Hx or cx + sx <= 0 or cy >= Hy or cy + sy <= 0:
        return "outside"
    over = (cx < 0, cx + sx > Hx, cy < 0, cy + sy > Hy)
    if all(over):
        return "around"
    return {(0, 0, 0, 0): "inside", (1, 0, 0, 0): "left", (0, 1, 0, 0): "right", (0, 0, 1, 0): "top", (0, 0, 0, 1): "bottom",
            (1, 0, 1, 0): "top-left", (0, 1, 1, 0): "top-right", (1, 0, 0, 1): "bottom-left", (0, 1, 0, 1): "bottom-right"}.get(
                tuple(int(o) for o in over), "other")


def poses_for(cells, size, origin):
    """Poses whose forced roll lands on `cells`: the window's aim half a cell from the cell's corner, on the side the
    truncation toward zero keeps (above it for cells >= 0, below it for negative ones), so no rounding decides."""
    half = (np.array(size, np.float64) - 1 + 0.5) * RES / 2.0
    xy = np.asarray(origin) + (cells + np.where(cells >= 0, 0.5, -0.5)) * RES + half
    return np.ascontiguousarray(np.concatenate([xy, np.zeros((len(cells), 1))], axis=1))


def world_map(world, seed=3):
    Hx, Hy = world
    m = np.random.default_rng(seed).integers(1, 255, (Hy, Hx), dtype=np.uint8)   # never 0 or 255: the fill values show
    return np.ascontiguousarray(m)


def test_the_case_list_is_wide_enough():
    """On the CPU, before any GPU call: the placements hit every source x-residue mod 16 and every destination-row residue
    mod 16, and every way a window can lie on the world."""
    seen, src_res, dst_res = set(), set(), set()
    for size in SIZES:
        dst_res |= {(y * size[0]) % 16 for y in range(size[1])}
        for world in WORLDS:
            cells, _ = target_cells(size, world)
            assert cells.shape == (B, 2)
            got, _, _, _ = LR.roll(W0, RES, None, poses_for(cells, size, W0), size[0], size[1], force=True)
            assert np.array_equal(got, cells)                   # the poses do put the windows there
            classes = [overlap_class(c, size, world) for c in cells]
            seen |= set(classes)
            src_res |= {int(c[0]) % 16 for c, k in zip(cells, classes) if k != "outside"}
            # the 16-byte path sees every residue itself, inside and over the edges
            if size[0] % 8 == 0 and (size[0] * size[1]) % 16 == 0:
                assert {int(c[0]) % 16 for c, k in zip(cells, classes) if k != "outside"} == set(range(16)), (size, world)
    assert src_res == set(range(16)) and dst_res == set(range(16))
    assert seen >= {"inside", "left", "right", "top", "bottom", "top-left", "top-right", "bottom-left", "bottom-right", "outside", "around"}
    assert overlap_class(target_cells((200, 200), (61, 47))[0][29], (200, 200), (61, 47)) == "around"   # the whole world inside a window
    assert {(y * 200) % 16 for y in range(200)} == {0, 8}      # a 16-byte piece of a 200-wide window may straddle two rows


@pytest.fixture(scope="module")
def solver():
    from nav2_social_mpc_controller_amd.params import OptimizerParams
    from nav2_social_mpc_controller_amd.solver import BatchSolver

    return BatchSolver(OptimizerParams.readme())


def check(got, want, what):
    cell, costmap, origin, moved = got
    assert np.array_equal(cell, want[0]) and cell.dtype == np.int32, what
    if moved is not None:
        assert np.array_equal(moved, want[3]) and moved.dtype == np.int32, what
    bad = np.flatnonzero((costmap != want[1]).reshape(len(cell), -1).any(axis=1))
    assert bad.size == 0, (what, "windows differ", bad[:8], want[0][bad[:8]])
    assert LR.same_bits(origin, want[2]), what


def device_call(solver, world, origin, pose, cell, costmap, costmap_origin, outside, force, moved=True, misalign=0):
    """The call on device pointers: (cell, costmap, costmap_origin, moved) back on the host."""
    import torch

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Bn, sy, sx = costmap.shape
    d = {k: up(v) for k, v in dict(world=world, origin=np.asarray(origin).reshape(-1, 2), pose=pose, cell=cell, costmap_origin=costmap_origin).items()}
    raw = torch.zeros(costmap.size + 16, dtype=torch.uint8, device="cuda")
    cm = raw[misalign:misalign + costmap.size]
    cm.copy_(up(costmap).reshape(-1))
    mv = torch.full((Bn,), -7, dtype=torch.int32, device="cuda")
    lc = solver.local_costmap_c(Bn, sx, sy, world.shape[-1], world.shape[-2], world.ndim == 2, RES, 1, outside, force)
    lc.world, lc.world_origin, lc.pose = d["world"].data_ptr(), d["origin"].data_ptr(), d["pose"].data_ptr()
    solver.local_costmap_device(lc, d["cell"].data_ptr(), cm.data_ptr(), d["costmap_origin"].data_ptr(), mv.data_ptr() if moved else 0)
    torch.cuda.synchronize()
    assert raw[:misalign].cpu().numpy().sum() == 0 and raw[misalign + costmap.size:].cpu().numpy().sum() == 0   # nothing beside the windows
    return (d["cell"].cpu().numpy(), cm.cpu().numpy().reshape(costmap.shape), d["costmap_origin"].cpu().numpy(),
            mv.cpu().numpy() if moved else None)


@pytest.mark.parametrize("world", WORLDS, ids=lambda w: f"world{w[0]}x{w[1]}")
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_windows_are_the_reference_crop(solver, size, world):
    sx, sy = size
    cells, _ = target_cells(size, world)
    wm = world_map(world)
    pose = poses_for(cells, size, W0)
    junk_cell = np.full((B, 2), 12345, np.int32)                # `force` takes the stored cells as (0,0)
    junk_map, junk_origin = np.full((B, sy, sx), 0xA5, np.uint8), np.full((B, 2), -1.25)
    # host pointers, shared world, outside 255
    want = LR.call(wm, W0, RES, pose, junk_cell, junk_map, junk_origin, 255, force=True)
    assert np.array_equal(want[0], cells) and (want[3] == 1).all()
    check(solver.local_costmap(wm, W0, RES, pose, junk_cell, junk_map, junk_origin, 255, force=True), want, "host, shared, 255")
    assert solver.last_kernel_ms() > 0.0
    # device pointers, shared world, outside 0
    want0 = LR.call(wm, W0, RES, pose, junk_cell, junk_map, junk_origin, 0, force=True)
    check(device_call(solver, wm, W0, pose, junk_cell, junk_map, junk_origin, 0, True), want0, "device, shared, 0")
    # a world and an origin per robot, host pointers, moved = NULL; then the same on device pointers
    worlds = np.ascontiguousarray(np.stack([np.roll(wm, (b, 2 * b), axis=(0, 1)) for b in range(B)]))
    origins = W0 + np.stack([np.arange(B) * 0.35, -np.arange(B) * 1.05], axis=1)
    pose_b = poses_for(cells, size, origins)
    want_b = LR.call(worlds, origins, RES, pose_b, junk_cell, junk_map, junk_origin, 0, force=True)
    assert np.array_equal(want_b[0], cells)
    check(solver.local_costmap(worlds, origins, RES, pose_b, junk_cell, junk_map, junk_origin, 0, force=True, moved=False), want_b,
          "host, per robot, 0, no moved")
    check(device_call(solver, worlds, origins, pose_b, junk_cell, junk_map, junk_origin, 0, True), want_b, "device, per robot, 0")
    # B = 1: over the bottom-right corner
    one = slice(23, 24)
    assert overlap_class(cells[23], size, world) != "inside"    # (a window larger than the world hangs over more sides)
    want1 = LR.call(wm, W0, RES, pose[one], junk_cell[one], junk_map[one], junk_origin[one], 255, force=True)
    check(solver.local_costmap(wm, W0, RES, pose[one], junk_cell[one], junk_map[one], junk_origin[one], 255, force=True), want1, "host, B = 1")
    check(device_call(solver, wm, W0, pose[one], junk_cell[one], junk_map[one], junk_origin[one], 255, True, moved=False), want1, "device, B = 1")


@pytest.mark.parametrize("misalign", [3, 8])
def test_a_costmap_off_the_16_byte_grid_takes_the_byte_path(solver, misalign):
    size, world = (16, 16), (61, 47)
    cells, _ = target_cells(size, world)
    wm, pose = world_map(world), poses_for(cells, size, W0)
    junk_map, junk_origin = np.full((B, 16, 16), 0xA5, np.uint8), np.zeros((B, 2))
    want = LR.call(wm, W0, RES, pose, cells, junk_map, junk_origin, 255, force=True)
    check(device_call(solver, wm, W0, pose, cells, junk_map, junk_origin, 255, True, misalign=misalign), want, f"costmap + {misalign}")


@pytest.mark.parametrize("size", [(200, 200), (37, 29)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_window_that_did_not_move_is_not_rewritten(solver, size, device):
    sx, sy = size
    world = (256, 192)
    cells, _ = target_cells(size, world)
    wm, pose = world_map(world), poses_for(cells, size, W0)
    run = (lambda *a, **k: device_call(solver, *a, **k)) if device else (lambda w, o, p, c, m, mo, out, force: solver.local_costmap(w, o, RES, p, c, m, mo, out, force=force))
    first = run(wm, W0, pose, np.zeros((B, 2), np.int32), np.zeros((B, sy, sx), np.uint8), np.zeros((B, 2)), 255, True)
    assert np.array_equal(first[0], cells)
    # poison; half of the robots move by 3.2 cells in x (and 1.2 back in y), the others by 0.4. The aim was half a cell
    # from the window's corner (poses_for), so 0.4 more leaves every quotient inside (-1, 1): those stay in their cell
    poison_map, poison_origin = np.full((B, sy, sx), 0xA5, np.uint8), np.frombuffer(b"\xa5" * (B * 16), np.float64).reshape(B, 2).copy()
    far = np.arange(B) % 2 == 0
    pose2 = pose.copy()
    pose2[:, 0] += np.where(far, 3.2, 0.4) * RES
    pose2[:, 1] -= np.where(far, 1.2, 0.4) * RES
    pose2[5, 0], pose2[6, 1] = np.nan, np.inf
    want = LR.call(wm, W0, RES, pose2, first[0], poison_map, poison_origin, 255)
    stays = ~far
    stays[[5, 6]] = True
    assert np.array_equal(want[3], np.where(stays, 0, 1) + 2 * np.isin(np.arange(B), [5, 6])) and far.sum() > 30
    assert (np.abs(want[0][:, 0] - cells[:, 0])[want[3] == 1] >= 2).all()
    got = run(wm, W0, pose2, first[0], poison_map, poison_origin, 255, False)
    check(got, want, "second call")
    assert (got[1][stays] == 0xA5).all() and got[2][stays].tobytes() == poison_origin[stays].tobytes()
    assert np.array_equal(got[0][stays], cells[stays]) and list(got[3][[5, 6]]) == [2, 2]


def test_error_returns(solver):
    from nav2_social_mpc_controller_amd.solver import SmpcError, _ptr

    wm = world_map((61, 47))
    pose, cell, cm, org = np.zeros((2, 3)), np.zeros((2, 2), np.int32), np.full((2, 3, 5), 7, np.uint8), np.ones((2, 2))
    origin = np.zeros((1, 2))

    def call(cell_p=cell, cm_p=cm, org_p=org, **over):
        args = dict(B=2, size_x=5, size_y=3, world_x=61, world_y=47, world_shared=True, resolution=RES, on_device=0)
        fields = {"world": wm, "world_origin": origin, "pose": pose}
        for k, v in over.items():
            (fields if k in fields else args)[k] = v
        lc = solver.local_costmap_c(**args)
        for k, v in fields.items():
            setattr(lc, k, _ptr(v))
        solver._call("smpc_local_costmap_batch", lc, _ptr(cell_p), _ptr(cm_p), _ptr(org_p), None)

    call()                                                      # the arguments are good as they stand
    assert (cm != 7).any() and cell.any()
    cm[:], cell[:], org[:] = 7, 0, 1.0
    for over in (dict(size_x=0), dict(size_y=-1), dict(world_x=0), dict(world_y=0), dict(B=-1), dict(resolution=0.0),
                 dict(resolution=-0.05), dict(resolution=float("nan")), dict(resolution=float("inf")), dict(world=None),
                 dict(world_origin=None), dict(pose=None), dict(cell_p=None), dict(cm_p=None), dict(org_p=None)):
        with pytest.raises(SmpcError, match=r"\(-1\)"):          # SMPC_ERR_INVALID_ARG
            call(**over)
    for over in (dict(world_x=65536, world_y=32768), dict(world_x=2 ** 31 - 1, world_y=2), dict(size_x=65536, size_y=32768)):
        with pytest.raises(SmpcError, match=r"\(-2\)"):          # SMPC_ERR_UNSUPPORTED
            call(**over)
    assert (cm == 7).all() and not cell.any() and (org == 1.0).all()   # the refusals wrote nothing
    with pytest.raises(SmpcError):
        solver.local_costmap_c(1, 1, 1, 1, 1, True, RES, 0, outside_cost=256)
