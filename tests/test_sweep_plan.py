"""The launch plan of the sweep kernels (csrc/smpc_plan.hpp) on the CPU: which slot width, variant, fixed-shape kernel,
helper lanes and LDS bytes a solve / K1 launch gets. The plan is a pure host function, so a small program compiled with
the compiler of `csrc/build.sh` answers queries here that otherwise need a handle, and a handle a device
(tests/test_gpu_order.py::test_solve_slot_width_rule, tests/test_gpu_fixed_shape.py). The knobs struct is filled directly;
where the program recomputes a value it uses the functions of smpc_launch.hpp alone."""
import os
import subprocess

import pytest

from test_kernel_budget import CSRC, HIPCC

# one query per line of stdin:  kind B T N CH bl T_scene scene_params num_cu share fixed_shapes no_helpers solve_width
#                               (kind: 0 K1, 1 solve, 2 trace; `stage T N`: the staging pass)
# one answer per line:          W S vt sp trace fixed stages hp_A shmem | helper_owner_agents(T, N, W), layout equal to
#                               make_layout()'s, the recomputed LDS bytes
PROBE = r"""
#include <cstdio>
#include <cstring>
#include "smpc_plan.hpp"
using namespace smpc;
int main() {
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    int T, N;
    if (std::sscanf(line, "stage %d %d", &T, &N) == 2) {
      const StagePlan p = plan_stage(T, N);
      const LdsLayout L = make_layout(T, N, 2, kLayoutStage, slot_width(T, N));
      std::printf("%d %d %zu | %d %zu\n", p.W, p.S, p.shmem, !std::memcmp(&p.L, &L, sizeof L),
                  (size_t)(kWave / slot_width(T, N)) * L.total * sizeof(double));
      continue;
    }
    int kind, B, CH, bl, vt, sp, cu, share, fixed, no_helpers, width;
    if (std::sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %d %d", &kind, &B, &T, &N, &CH, &bl, &vt, &sp, &cu, &share, &fixed,
                    &no_helpers, &width) != 13) return 1;
    Knobs kn;
    kn.no_helpers = no_helpers != 0;
    kn.solve_width = width;
    const int nb = (CH - 1) / bl + 1, P = 2 * nb;
    const SweepPlan p = plan_sweep({(Sweep)kind, B, T, N, CH, bl, nb, vt != 0, sp != 0, cu, share, fixed != 0}, kn);
    const bool eval = kind == 0;
    const LdsLayout L = make_layout(T, N, P, eval ? kLayoutEval : kLayoutSolve, p.W, p.sp);
    const int extra = eval ? eval_extra_doubles(T, P, p.W) : wave_extra_doubles(P, p.W);
    std::printf("%d %d %d %d %d %d %d %d %zu | %d %d %zu\n", p.W, p.S, p.vt, p.sp, p.trace, p.fixed, p.stages, p.hp_A, p.shmem,
                helper_owner_agents(T, N, p.W), !std::memcmp(&p.L, &L, sizeof L),
                ((size_t)atan_tab_offset((kWave / p.W) * L.total, extra) + kAtanTabDoubles) * sizeof(double));
  }
  return 0;
}
"""

K1, SOLVE, TRACE = 0, 1, 2
FIELDS = ("W", "S", "vt", "sp", "trace", "fixed", "stages", "hp_A", "shmem", "helper_owner_agents", "layout_same", "shmem_again")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    tmp = tmp_path_factory.mktemp("sweep_plan")
    src, exe = tmp / "probe.hip", tmp / "probe"
    src.write_text(PROBE)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])

    def ask(queries):
        out = subprocess.run([str(exe)], input="".join(q + "\n" for q in queries), capture_output=True, text=True, check=True)
        rows = [[int(v) for v in line.replace("|", " ").split()] for line in out.stdout.splitlines()]
        assert len(rows) == len(queries)
        return rows

    return ask


def q(kind, B, T, N, CH=18, bl=6, T_scene=0, scene_params=0, cus=256, share=1, fixed_shapes=1, no_helpers=0, width=0):
    return f"{kind} {B} {T} {N} {CH} {bl} {T_scene} {scene_params} {cus} {share} {fixed_shapes} {no_helpers} {width}"


def plans(ask, queries):
    return [dict(zip(FIELDS, row)) for row in ask(queries)]


@pytest.mark.parametrize("cus", [256, 7])
def test_solve_slot_width_rule(ask, cus):
    """Every assertion of tests/test_gpu_order.py::test_solve_slot_width_rule, with the MI355X's 256 CUs and with 7, where
    the integer division by the share shows."""
    def W(B, T, N, share=1):
        return plans(ask, [q(SOLVE, B, T, N, cus=cus, share=share)])[0]["W"]

    assert W(8192, 38, 16) == 64 and W(1, 38, 3) == 64
    assert W(8192, 28, 64) == 64
    assert W(8192, 28, 8) == 32
    assert W(1, 28, 8) == 64 and W(8 * cus, 28, 8) == 64
    assert W(8 * cus + 1, 28, 8) == 32
    assert W(4 * cus, 28, 3) == 64 and W(4 * cus + 1, 28, 3) == 32
    assert W(4 * cus, 28, 0) == 64
    assert W(8 * cus // 3, 28, 8, share=3) == 64 and W(8 * cus // 3 + 1, 28, 8, share=3) == 32


def test_width_knob_overrides_a_shape_that_fits_two_scenes_per_wave_only_and_never_k1(ask):
    got = plans(ask, [q(SOLVE, 1, 28, 8, width=32), q(SOLVE, 8192, 28, 8, width=64),
                      q(SOLVE, 8192, 38, 16, width=32), q(SOLVE, 8192, 28, 64, width=32), q(TRACE, 1, 28, 8, width=32)])
    assert [p["W"] for p in got] == [32, 64, 64, 64, 32]
    # K1 takes slot_width(T, N) whatever the batch size, the share or the knob
    k1 = plans(ask, [q(K1, B, T, N, width=w, share=s) for B in (1, 8192) for w in (0, 32, 64) for s in (1, 3)
                     for T, N in ((28, 8), (31, 32), (32, 8), (28, 33), (38, 16))])
    assert [p["W"] for p in k1] == [32, 32, 64, 64, 64] * 12
    assert all(p["S"] == 64 // p["W"] for p in got + k1)


def test_fixed_shape_rule(ask):
    """Key (T, N, CH, bl) = (28, 8, 18, 6), index 0 of SMPC_FIXED_SHAPES."""
    solve, k1 = plans(ask, [q(SOLVE, 8192, 28, 8), q(K1, 8192, 28, 8)])
    assert (solve["fixed"], solve["stages"], solve["W"]) == (0, 1, 32)
    assert (k1["fixed"], k1["stages"], k1["W"]) == (0, 0, 32)
    none = {
        "T_scene": q(SOLVE, 8192, 28, 8, T_scene=1), "scene_params": q(SOLVE, 8192, 28, 8, scene_params=1),
        "K1 T_scene": q(K1, 8192, 28, 8, T_scene=1), "K1 scene_params": q(K1, 8192, 28, 8, scene_params=1),
        "trace": q(TRACE, 8192, 28, 8),
        "fixed_shapes off": q(SOLVE, 8192, 28, 8, fixed_shapes=0), "K1 fixed_shapes off": q(K1, 8192, 28, 8, fixed_shapes=0),
        "SMPC_NO_HELPERS": q(SOLVE, 8192, 28, 8, no_helpers=1), "K1 SMPC_NO_HELPERS": q(K1, 8192, 28, 8, no_helpers=1),
        "B = 1 (width 64)": q(SOLVE, 1, 28, 8),
        "N = 7": q(SOLVE, 8192, 28, 7), "T = 27": q(SOLVE, 8192, 27, 8),
        "CH = 17": q(SOLVE, 8192, 28, 8, CH=17), "bl = 5": q(SOLVE, 8192, 28, 8, bl=5),
    }
    for (name, _), p in zip(none.items(), plans(ask, list(none.values()))):
        assert (p["fixed"], p["stages"]) == (-1, 0), name
    # the case the GPU tests use: a small batch at the two-scenes-per-wave width
    small = plans(ask, [q(SOLVE, 5, 28, 8, width=32)])[0]
    assert (small["fixed"], small["stages"], small["W"]) == (0, 1, 32)


def test_trace_runs_the_most_general_variant_whatever_the_batch_brings(ask):
    for p in plans(ask, [q(TRACE, B, 28, 8, T_scene=t, scene_params=s) for B in (1, 8192) for t in (0, 1) for s in (0, 1)]):
        assert (p["vt"], p["sp"], p["trace"], p["stages"], p["fixed"]) == (1, 1, 1, 0, -1)
    got = plans(ask, [q(kind, 8192, 28, 8, T_scene=t, scene_params=s) for kind in (K1, SOLVE) for t in (0, 1) for s in (0, 1)])
    assert [(p["vt"], p["sp"], p["trace"]) for p in got] == [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0)] * 2


# (T, N, CH, bl, W) with nb = 3, 3, 5, 3; B = 1 runs a two-slot shape at one scene per wave
SHAPES = [(28, 8, 18, 6, 32), (28, 8, 18, 6, 64), (38, 16, 20, 4, 64), (28, 0, 18, 6, 32)]


def test_helper_lanes_layout_and_lds_bytes_are_the_recomputation(ask):
    queries, want_w = [], []
    for T, N, CH, bl, W in SHAPES:
        for kind in (SOLVE, K1):
            if kind == K1 and (T, W) == (28, 64):
                continue   # K1 of a two-slot shape has no one-scene-per-wave launch
            for sp in (0, 1):
                for no_helpers in (0, 1):
                    queries.append(q(kind, 1 if W == 64 else 8192, T, N, CH=CH, bl=bl, scene_params=sp, no_helpers=no_helpers))
                    want_w.append((W, N if no_helpers else None))
    got = plans(ask, queries)
    for query, p, (W, hp_A) in zip(queries, got, want_w):
        assert p["W"] == W, query
        assert p["hp_A"] == (p["helper_owner_agents"] if hp_A is None else hp_A), query
        assert p["layout_same"] == 1 and p["shmem"] == p["shmem_again"] and 0 < p["shmem"] <= 160 * 1024, query
    # helper lanes are at work in this list: BASELINE configs[4] (T = 38, N = 16) walks 11 agents on the owner lane, the
    # headline shape at one scene per wave 4 of 8
    assert {p["helper_owner_agents"] for p in got} >= {0, 4, 8, 11}
    # sp: 14 doubles more per slot
    by = {qq: p["shmem"] for qq, p in zip(queries, got)}
    assert by[q(SOLVE, 8192, 28, 8, scene_params=1)] > by[q(SOLVE, 8192, 28, 8)]


def test_staging_pass_sizing_is_the_recomputation(ask):
    rows = ask(["stage 28 8", "stage 38 16"])
    assert [r[:2] for r in rows] == [[32, 2], [64, 1]]
    for W, S, shmem, layout_same, again in rows:
        assert layout_same == 1 and shmem == again > 0


def test_the_knobs_are_read_in_the_plan_header_and_nowhere_else():
    plan = open(os.path.join(CSRC, "smpc_plan.hpp")).read()
    for name in ("SMPC_NO_HELPERS", "SMPC_SOLVE_WIDTH", "SMPC_LONE_WAVES_PER_CU", "SMPC_MAX_WAVES_PER_CU", "SMPC_PRIO_STEP",
                 "SMPC_FULL_GRAM", "SMPC_DEBUG_GRID"):
        assert plan.count(f'("{name}")') == 1, name
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".inc")) and name != "smpc_plan.hpp":
            assert "getenv" not in open(os.path.join(CSRC, name)).read(), name
