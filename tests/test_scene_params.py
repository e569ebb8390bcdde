"""Per-scene critic weights and velocity bounds (`smpc_scene_batch.scene_params`), host side: the register budget of the
sp kernels and the Python plumbing (CPU only; the struct layout is in tests/test_abi.py, the device behaviour in
tests/test_gpu_scene_params.py)."""
import os

import numpy as np
import pytest

from nav2_social_mpc_controller_amd import _abi
from nav2_social_mpc_controller_amd.params import OptimizerParams, scene_param_rows
from nav2_social_mpc_controller_amd.scenes import SceneBatch, make_scenes
from test_kernel_budget import CSRC, MAX_VGPRS, usage  # noqa: F401  (usage: the NB = 3 build's resource remarks)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_is_6():
    from nav2_social_mpc_controller_amd import solver as S
    assert _abi.SMPC_ABI_VERSION == 6
    assert S.load_library().smpc_abi_version() == 6


def test_scene_row_follows_the_struct_order():
    p = OptimizerParams.readme().replace(desired_linear_vel=0.55, v_min=0.05, v_max=0.5, w_min=-1.1, w_max=1.2)
    row = p.scene_row()
    c = p.to_c()
    assert [n for n, _ in _abi.SmpcSceneParams._fields_] == list(_abi.SCENE_PARAM_FIELDS)
    assert row.dtype == np.float64 and row.shape == (14,)
    assert list(row) == [getattr(c, f) for f in _abi.SCENE_PARAM_FIELDS]


def test_rows_helper_assigns_and_refuses_structural_differences():
    a, b = OptimizerParams.soc_work_obst_benchmark(), OptimizerParams.obst_only_benchmark()
    rows = scene_param_rows([a, b], [0, 1, 1, 0])
    assert rows.shape == (4, 14) and rows.flags["C_CONTIGUOUS"]
    assert np.array_equal(rows[0], a.scene_row()) and np.array_equal(rows[1], b.scene_row())
    assert np.array_equal(rows[2], b.scene_row()) and np.array_equal(rows[3], a.scene_row())
    assert np.array_equal(scene_param_rows([a], np.zeros(3, int)), np.tile(a.scene_row(), (3, 1)))
    for kw in (dict(control_horizon=12), dict(parameter_block_length=4), dict(fn_tol=1e-6), dict(gradient_tol=1e-9),
               dict(param_tol=1e-8), dict(max_iterations=30), dict(linear_solver_type="DENSE_QR"), dict(time_step=0.1),
               dict(max_time=2.0), dict(fixed_iterations=1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            scene_param_rows([a, b.replace(**kw)], [0, 1])
    with pytest.raises(ValueError):
        scene_param_rows([a, b], [0, 2])


def _batch():
    prm = OptimizerParams.readme()
    sc = make_scenes(prm, 6, 3, map_cells=40, seed=11)
    rows = scene_param_rows([prm, prm.replace(social_weight=7.0, v_max=0.4)], [0, 1, 0, 1, 1, 0])
    return prm, sc, sc.with_scene_params(rows), rows


def test_scene_batch_carries_scene_params():
    prm, plain, sc, rows = _batch()
    assert plain.scene_params is None and plain.to_c().scene_params is None
    assert np.array_equal(sc.scene_params, rows)
    assert sc.to_c().scene_params == sc.scene_params.ctypes.data
    sub = sc.select([4, 1])
    assert np.array_equal(sub.scene_params, rows[[4, 1]])
    cut = sc.cut([5, 2, 3], sc.T - 4, 4)
    assert np.array_equal(cut.scene_params, rows[[5, 2, 3]])
    hz = sc.with_horizons(np.full(sc.B, sc.T - 1))
    assert np.array_equal(hz.scene_params, rows)
    with pytest.raises(AssertionError):
        sc.with_scene_params(rows[:, :13])


def test_save_load_round_trip(tmp_path):
    prm, plain, sc, rows = _batch()
    sc.save(str(tmp_path / "sp.npz"))
    back = SceneBatch.load(str(tmp_path / "sp.npz"))
    assert np.array_equal(back.scene_params, rows) and back.scene_params.dtype == np.float64
    plain.save(str(tmp_path / "plain.npz"))
    assert SceneBatch.load(str(tmp_path / "plain.npz")).scene_params is None
    # the committed fixtures (written before the field existed) load as they did
    g = SceneBatch.load(os.path.join(ROOT, "tests", "golden", "cfg3_n8_scenes.npz"))
    assert g.scene_params is None and g.to_c().scene_params is None


# ---- register budget of the sp kernels (compile time, like tests/test_kernel_budget.py) ----------------------------
SP_KERNELS = {
    "solve_sp<3,32>": "_ZN4smpc17smpc_solve_kernelILi3ELi32ELb1ELb1ELb0EEEvNS_7KParamsE",
    "K1_sp<3,32>": "_ZN4smpc16smpc_eval_kernelILi3ELi32ELb1ELb1EEEvNS_7KParamsE",
}
VT_SOLVE = "_ZN4smpc17smpc_solve_kernelILi3ELi32ELb1ELb0ELb0EEEvNS_7KParamsE"  # the per-scene-horizon kernel the sp path extends


@pytest.mark.parametrize("name", sorted(SP_KERNELS))
def test_sp_kernel_keeps_three_waves(usage, name):
    r = usage.get(SP_KERNELS[name])
    assert r is not None, f"{name}: no resource remark (instantiation missing?)"
    assert r["VGPRs"] <= MAX_VGPRS, f"{name}: {r['VGPRs']} VGPRs > {MAX_VGPRS}"
    assert r["SGPRs Spill"] == 0, f"{name}: {r['SGPRs Spill']} spilled SGPRs"
    assert r["Occupancy [waves/SIMD]"] >= 3, f"{name}: occupancy {r['Occupancy [waves/SIMD]']}"


def test_sp_k1_has_no_spill_and_no_private_segment(usage):
    r = usage[SP_KERNELS["K1_sp<3,32>"]]
    assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, r


def test_sp_solve_spills_no_more_than_the_per_scene_horizon_kernel(usage):
    """The sp solve kernel reads its horizon per scene like smpc_solve_kernel<3,32,true>, whose 12 spilled VGPRs (20 B
    private segment) it shares; the per-scene weights and bounds must not add to them."""
    r, vt = usage[SP_KERNELS["solve_sp<3,32>"]], usage[VT_SOLVE]
    assert r["VGPRs Spill"] <= vt["VGPRs Spill"], (r, vt)
    assert r["ScratchSize [bytes/lane]"] <= vt["ScratchSize [bytes/lane]"], (r, vt)


def test_sp_k1_one_scene_per_wave_spills_no_more_than_recorded(usage):
    """K1 sp <3,64> (outside the issue's <3,32> budget) at the values DESIGN §4 records: 3 waves per SIMD, at most 4
    spilled VGPRs and a 20 B private segment."""
    r = usage["_ZN4smpc16smpc_eval_kernelILi3ELi64ELb1ELb1EEEvNS_7KParamsE"]
    assert r["VGPRs"] <= MAX_VGPRS and r["Occupancy [waves/SIMD]"] >= 3, r
    assert r["VGPRs Spill"] <= 4 and r["ScratchSize [bytes/lane]"] <= 20, r


def test_source_digest_covers_every_file_the_build_reads(tmp_path):
    """buildinfo.csrc_digest() ties committed profiles to the device sources: every file csrc/ includes must be in it,
    the headers that hold the kernel bodies among them."""
    import re
    import shutil

    from nav2_social_mpc_controller_amd.buildinfo import SOURCE_SUFFIXES, csrc_digest

    included = set()
    for name in os.listdir(CSRC):
        if name.endswith((".hip", ".hpp", ".inc")):
            included |= set(re.findall(r'#include "([^"/]+)"', open(os.path.join(CSRC, name)).read()))
    assert {"smpc_solve_kernel.hpp", "smpc_eval_kernel.hpp"} <= included
    for name in included:
        assert name.endswith(SOURCE_SUFFIXES), name
    root = tmp_path / "csrc"
    shutil.copytree(CSRC, root, ignore=shutil.ignore_patterns("*.so", "*.o", "__pycache__"))
    before = csrc_digest(str(root))
    with open(root / "smpc_solve_kernel.hpp", "a") as f:
        f.write("// edit\n")
    assert csrc_digest(str(root)) != before


def test_row_check_uses_the_struct_fields():
    from nav2_social_mpc_controller_amd.params import check_scene_param_rows

    rows = scene_param_rows([OptimizerParams.readme()], np.zeros(3, int))
    assert np.array_equal(check_scene_param_rows(rows, 3), rows)
    col = {f: i for i, f in enumerate(_abi.SCENE_PARAM_FIELDS)}
    for f, v in (("v_min", 0.9), ("w_max", -2.0), ("obstacle_w", np.nan), ("desired_linear_vel", np.inf)):
        bad = rows.copy()
        bad[1, col[f]] = v
        with pytest.raises(ValueError):
            check_scene_param_rows(bad, 3)
    with pytest.raises(ValueError):
        check_scene_param_rows(rows, 4)
