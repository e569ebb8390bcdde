"""The people detector on the CPU: Philox4x32-10 against the known answers of the Random123 distribution, the yardstick
itself (tests/detector_ref.py) on hand-made ticks with the expected outputs written out, the `__host__ __device__` rule of
csrc/smpc_detector_rule.hpp compiled into a host-only program and composed as the kernel composes it (a mask of usable
persons walked bit by bit, draws skipped where the kernel skips them, output rows by ranks) against the yardstick, the ctypes
mirror against include/smpc_detector.h, DetectorParams, the episode's declarations, the kernel's resource remarks, the
statistics of the rule's constants, and that the seeded sequences exercise what the feature adds."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import detector_cases as DC
import detector_ref as R
from nav2_social_mpc_controller_amd import _abi_detector as DA
from nav2_social_mpc_controller_amd import solver as S
from nav2_social_mpc_controller_amd.params import DetectorParams
from test_kernel_budget import CSRC, HIPCC, parse_resource_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc_detector.h")
KERNEL = "_ZN4smpc25smpc_detect_people_kernelENS_14DetectorParamsE"

HAND = DC.hand_cases()
SEEDED = DC.seeded_cases()

# Random123's kat_vectors for philox4x32 with 10 rounds: (counter, key) -> words
KNOWN_ANSWERS = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
def test_the_yardsticks_philox_gives_the_known_answers():
    for counter, key, words in KNOWN_ANSWERS:
        assert R.philox(counter, key) == words
    p = R.params(seed=0x299f31d0a4093822)
    assert R.draw(p, 0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344) == KNOWN_ANSWERS[2][2]     # draw(t, s, i, purpose), key (seed_lo, seed_hi)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_cases_give_what_the_contract_gives(name):
    for t, tick, before, new, outs in DC.run(HAND[name], DC.ref_call):
        assert tick["want"] is not None
        DC.check_want(new, outs, tick["want"])
        assert new.dtype == np.uint32 and outs[0].dtype == np.float64 and outs[1].dtype == np.int32 and outs[3].dtype == np.uint8
        assert new[:, 0].tolist() == before[:, 0].tolist()                                   # the stream id is never written


def test_the_seeded_sequences_exercise_the_detector():
    """By the yardstick alone, before anything is compared with it: every outcome and both truncations occur, clutter is
    reported, a pose is not finite, and every shape with room for them hides, misses and reports somebody."""
    total = dict.fromkeys(R.COUNTERS, 0)
    for name, case in SEEDED.items():
        mine = dict.fromkeys(R.COUNTERS, 0)
        for _, _, _, _, counters in DC.reference(name, case):
            for k in R.COUNTERS:
                mine[k] += int(counters[k].sum())
        for k in R.COUNTERS:
            total[k] += mine[k]
        if case["ticks"][0]["people"].shape[1] >= 8 and case["ticks"][0]["people"].shape[0] >= 5:
            assert mine["detected"] and mine["body_occluded"] and mine["missed"] and mine["not_finite"], (name, mine)
    assert all(total[k] >= 1 for k in R.COUNTERS), total
    assert total["body_occluded"] >= 0.05 * total["detected"] and total["missed"] >= 0.1 * total["detected"], total


def test_the_rules_constants_give_the_stated_statistics():
    """The yardstick alone, one fixed seed, 65,536 draws each: conditions on the rule's constants (a threshold of p * 2^32, a
    noise sum of standard deviation 2^32 / sqrt(3), a clutter scale of range / 2^31), not device measurements. With key
    (123, 456), stream 7, p_miss = 0.2 and unit sigma: miss fraction 0.2028, mean 0.0034, standard deviation 0.9984, largest
    |value| 3.28: all inside the bounds, so a failure is a bug and not bad luck."""
    n, p_miss = 65536, 0.2
    p = R.params(p_miss=p_miss, sigma=1.0, sigma_growth=0.0, clutter_range=5.0, seed=(456 << 32) | 123)
    assert (p["seed_lo"], p["seed_hi"]) == (123, 456)
    ticks, rows = n // 64, 64
    missed = sum(R.draw(p, t, 7, j, R.PURPOSE_MISS)[0] < p["miss_threshold"] for t in range(ticks) for j in range(rows))
    assert abs(missed / n - p_miss) <= 4.0 * np.sqrt(p_miss * (1.0 - p_miss) / n), missed / n
    z = np.array([float(np.float64(R.noise_sum(R.draw(p, t, 7, j, R.PURPOSE_NOISE_X))) * p["noise_scale"]) for t in range(ticks) for j in range(rows)])
    assert abs(z.mean()) <= 4.0 / np.sqrt(n), z.mean()
    # the standard error of a sample standard deviation: sigma * sqrt((kurtosis - 1) / (4 n)); the sum of four uniforms has
    # kurtosis 3 - 1.2 / 4 = 2.7
    assert abs(z.std() - 1.0) <= 4.0 * np.sqrt((2.7 - 1.0) / (4.0 * n)), z.std()
    assert np.abs(z).max() <= 2.0 * np.sqrt(3.0)                                              # the sum's hard bound: 2 sqrt(3) sigma
    signed = lambda v: v - 2 ** 32 if v >= 2 ** 31 else v
    for t in range(ticks):
        for c in range(rows):
            w = R.draw(p, t, 7, c, R.PURPOSE_CLUTTER)
            x, y = np.float64(signed(w[1])) * p["clutter_scale"], np.float64(signed(w[2])) * p["clutter_scale"]
            assert -5.0 <= x < 5.0 and -5.0 <= y < 5.0


# ---- the compiled rule ------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include "smpc_detector_rule.hpp"

static double dbl(unsigned long long u) { double v; std::memcpy(&v, &u, 8); return v; }
static std::string hex(double v) { char b[40]; uint64_t u; std::memcpy(&u, &v, 8); std::snprintf(b, sizeof b, "%016llx", (unsigned long long)u); return b; }

// "k c0 c1 c2 c3 k0 k1": the words of Philox. "r ...": one robot, composed as the kernel composes the rule: a person per
// "lane", the mask of usable persons walked bit by bit with the early exit, the draws the kernel skips skipped, ranks.
int main() {
  std::string kind;
  while (std::cin >> kind) {
    if (kind == "k") {
      unsigned long long c[6];
      for (auto& v : c) std::cin >> std::hex >> v;
      const smpc::DtWords w = smpc::dt_philox((uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2], (uint32_t)c[3], (uint32_t)c[4], (uint32_t)c[5]);
      std::printf("%08x %08x %08x %08x\n", w.w[0], w.w[1], w.w[2], w.w[3]);
      continue;
    }
    long long Np, Nd, Kc, count;
    unsigned long long s_, t_, k0_, k1_, miss_, clutter_, d[6];
    std::cin >> std::dec >> Np >> Nd >> Kc >> count >> std::hex >> s_ >> t_ >> k0_ >> k1_ >> miss_ >> clutter_;
    for (auto& v : d) std::cin >> std::hex >> v;
    const uint32_t stream = (uint32_t)s_, tick = (uint32_t)t_, k0 = (uint32_t)k0_, k1 = (uint32_t)k1_, miss = (uint32_t)miss_, clutter = (uint32_t)clutter_;
    const double body_radius = dbl(d[0]), noise_scale = dbl(d[1]), noise_growth = dbl(d[2]), clutter_scale = dbl(d[3]), rx = dbl(d[4]), ry = dbl(d[5]);
    std::vector<double> row(Np * 5);
    for (auto& v : row) { unsigned long long u; std::cin >> std::hex >> u; v = dbl(u); }
    if (Np > 64 || Nd > 64 || Kc > 64) std::abort();
    const long long n = count < 0 ? 0 : (count > Np ? Np : count);
    std::string out = std::to_string(tick + 1u) + " ";
    if (!(smpc::dt_finite(rx) && smpc::dt_finite(ry))) {
      std::string oc;
      for (long long j = 0; j < n; ++j) oc += std::to_string((int)smpc::kDetectNotFinite) + ",";
      std::printf("%s0 %s- |\n", out.c_str(), oc.c_str());
      continue;
    }
    std::vector<double> dx(64, 0.0), dy(64, 0.0), dd(64, 0.0);
    std::vector<char> usable(64, 0), hidden(64, 0), detected(64, 0);
    std::vector<int> code(64, 0);
    uint64_t mask = 0;
    for (long long j = 0; j < n; ++j) {
      usable[j] = smpc::dt_finite(row[5 * j]) && smpc::dt_finite(row[5 * j + 1]);
      if (usable[j]) { dx[j] = smpc::dt_offset(row[5 * j], rx); dy[j] = smpc::dt_offset(row[5 * j + 1], ry); mask |= 1ull << j; }
    }
    for (long long j = 0; j < 64; ++j) dd[j] = smpc::dt_dd(dx[j], dy[j]);
    if (body_radius > 0.0) {
      const double r2 = smpc::dt_r2(body_radius);
      for (uint64_t m = mask; m != 0; m &= m - 1) {
        const int k = __builtin_ctzll(m) & 63;
        bool left = false;
        for (long long j = 0; j < 64; ++j) {
          const bool hides = smpc::dt_occludes(dx[j], dy[j], dd[j], dx[k], dy[k], r2);
          hidden[j] = hidden[j] || (k != j && hides);
          left = left || (usable[j] && !hidden[j]);
        }
        if (!left) break;
      }
    }
    std::vector<double> zx(64, 0.0), zy(64, 0.0);
    uint64_t det_mask = 0;
    for (long long j = 0; j < 64; ++j) {
      detected[j] = usable[j] && !hidden[j];
      code[j] = !usable[j] ? smpc::kDetectNotFinite : hidden[j] ? smpc::kDetectBodyOccluded : smpc::kDetectDetected;
      if (detected[j] && miss != 0u && smpc::dt_missed(smpc::dt_philox(tick, stream, (uint32_t)j, smpc::kDrawMiss, k0, k1).w[0], miss)) {
        detected[j] = 0; code[j] = smpc::kDetectMissed;
      }
      if (j < Np) { zx[j] = row[5 * j]; zy[j] = row[5 * j + 1]; }
      const double scale = smpc::dt_scale(noise_scale, noise_growth, dd[j]);
      if (detected[j] && scale != 0.0) {
        zx[j] = smpc::dt_noisy(zx[j], smpc::dt_noise_sum(smpc::dt_philox(tick, stream, (uint32_t)j, smpc::kDrawNoiseX, k0, k1)), scale);
        zy[j] = smpc::dt_noisy(zy[j], smpc::dt_noise_sum(smpc::dt_philox(tick, stream, (uint32_t)j, smpc::kDrawNoiseY, k0, k1)), scale);
      }
      if (detected[j]) det_mask |= 1ull << j;
    }
    std::string oc, rows = "|";
    for (long long j = 0; j < n; ++j) oc += std::to_string(code[j]) + ",";
    const int n_det = __builtin_popcountll(det_mask);
    for (long long j = 0; j < 64; ++j) {
      const int rank = __builtin_popcountll(det_mask & ((1ull << j) - 1ull));
      if (detected[j] && rank < Nd)
        rows += std::to_string(rank) + ":" + std::to_string(j) + ":" + hex(zx[j]) + ":" + hex(zy[j]) + ":" + hex(row[5 * j + 2]) + ":" + hex(row[5 * j + 3]) + ":" + hex(row[5 * j + 4]) + "|";
    }
    uint64_t cmask = 0;
    std::vector<double> cx(64, 0.0), cy(64, 0.0);
    for (long long c = 0; c < Kc && clutter != 0u; ++c) {
      const smpc::DtWords w = smpc::dt_philox(tick, stream, (uint32_t)c, smpc::kDrawClutter, k0, k1);
      if (smpc::dt_clutter_exists(w.w[0], clutter)) cmask |= 1ull << c;
      cx[c] = smpc::dt_clutter_xy(rx, w.w[1], clutter_scale); cy[c] = smpc::dt_clutter_xy(ry, w.w[2], clutter_scale);
    }
    for (long long c = 0; c < 64; ++c) {
      const int rank = n_det + __builtin_popcountll(cmask & ((1ull << c) - 1ull));
      if (((cmask >> c) & 1ull) && rank < Nd)
        rows += std::to_string(rank) + ":" + std::to_string(-1 - c) + ":" + hex(cx[c]) + ":" + hex(cy[c]) + ":" + hex(0.0) + ":" + hex(0.0) + ":" + hex(0.0) + "|";
    }
    const long long total = n_det + __builtin_popcountll(cmask);
    std::printf("%s%lld %s- %s\n", out.c_str(), total < Nd ? total : Nd, oc.c_str(), rows.c_str());
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    tmp = tmp_path_factory.mktemp("detector_rule")
    src, exe = tmp / "probe.hip", tmp / "probe"
    src.write_text(PROBE)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])   # -O3 as build.sh
    bits = lambda v: format(int(np.array(v, np.float64).view(np.uint64)), "x")

    def call(state, tick, p, det=None, source=None, outcome=None):
        people, B = np.asarray(tick["people"], np.float64), len(tick["count"])
        Np, Nd = people.shape[1], p["Nd"]
        lines = []
        for b in range(B):
            head = ["r", Np, Nd, p["Kc"], int(tick["count"][b])] + [format(int(v), "x") for v in (state[b][0], state[b][1], p["seed_lo"], p["seed_hi"],
                                                                                                 p["miss_threshold"], p["clutter_threshold"])]
            scalars = [bits(v) for v in (p["body_radius"], p["noise_scale"], p["noise_growth"], p["clutter_scale"], tick["pose"][b][0], tick["pose"][b][1])]
            lines.append(" ".join(map(str, head + scalars + [format(int(u), "x") for u in people[b].ravel().view(np.uint64)])))
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == B
        det = np.full((B, Nd, 5), np.nan) if det is None else np.array(det, np.float64)
        source = np.full((B, Nd), -99, np.int32) if source is None else np.array(source, np.int32)
        outcome = np.full((B, Np), 255, np.uint8) if outcome is None else np.array(outcome, np.uint8)
        new, det_count = np.array(state, np.uint32), np.zeros(B, np.int32)
        for b, line in enumerate(out):
            t_after, cnt, oc, rows = line.split()
            new[b, 1], det_count[b] = int(t_after), int(cnt)
            codes = [int(v) for v in oc.split(",")[:-1]]
            outcome[b, :len(codes)] = codes
            written = [r.split(":") for r in rows.split("|") if r]
            assert sorted(int(r[0]) for r in written) == list(range(det_count[b]))
            for r in written:
                source[b, int(r[0])] = int(r[1])
                det[b, int(r[0])] = np.array([int(v, 16) for v in r[2:]], np.uint64).view(np.float64)
        return new, (det, det_count, source, outcome)

    call.exe = str(exe)
    return call


def test_the_compiled_philox_gives_the_known_answers(rule):
    lines = "".join("k " + " ".join(format(v, "x") for v in counter + key) + "\n" for counter, key, _ in KNOWN_ANSWERS)
    out = subprocess.run([rule.exe], input=lines, capture_output=True, text=True, check=True).stdout.split()
    assert [int(v, 16) for v in out] == [w for _, _, words in KNOWN_ANSWERS for w in words]


def test_compiled_rule_is_the_yardstick_on_the_hand_made_cases(rule):
    for name, case in HAND.items():
        for t, tick, before, new, outs in DC.run(case, rule):
            assert DC.same((new, outs), DC.ref_call(before, tick, case["p"])), (name, t)
            DC.check_want(new, outs, tick["want"])


def test_compiled_rule_is_the_yardstick_on_the_seeded_sequences(rule):
    for name, case in SEEDED.items():
        for t, (tick, before, new, outs, _) in enumerate(DC.reference(name, case)):
            assert DC.same(rule(before, tick, case["p"]), (new, outs)), (name, t)


def test_the_rule_header_rounds_every_operation_on_its_own():
    text = open(os.path.join(CSRC, "smpc_detector_rule.hpp")).read()
    assert "fma(" not in text and re.findall(r"#include\s*\S+", text) == ["#include <stdint.h>"]
    # every function with two floating-point operations switches contraction off
    for body in re.findall(r"SMPC_DT_HD inline [^{]*\{(.*?)\n\}", text, flags=re.S):
        code = re.sub(r"//.*", "", body)
        ops = len(re.findall(r"\s[*+-]\s", code)) if "double" in code else 0
        assert ops < 2 or "#pragma clang fp contract(off)" in body, body
    assert text.count("#pragma clang fp contract(off)") >= 6
    kernel = open(os.path.join(CSRC, "smpc_detector.hpp")).read()
    assert '#include "smpc_detector_rule.hpp"' in kernel and "fma(" not in kernel


# ---- the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mirror_matches_the_header_and_the_library_exports_the_function(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src))) == sorted(DA.FUNCTIONS) == ["smpc_detect_people_batch"]
    assert re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S) == [st.c_name for st in DA.STRUCTS]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' + "".join(f'printf("%zu\\n", offsetof({st.c_name}, {f[0]}));\n' for f in st._fields_)
                   for st in DA.STRUCTS)
    body += 'printf("%d %d %d %d\\n", SMPC_DETECT_DETECTED, SMPC_DETECT_BODY_OCCLUDED, SMPC_DETECT_MISSED, SMPC_DETECT_NOT_FINITE);\n'
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc_detector.h"\nint main(void){\n' + body + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [v for st in DA.STRUCTS for v in [C.sizeof(st)] + [getattr(st, f[0]).offset for f in st._fields_]]
    assert values == want + [DA.SMPC_DETECT_DETECTED, DA.SMPC_DETECT_BODY_OCCLUDED, DA.SMPC_DETECT_MISSED, DA.SMPC_DETECT_NOT_FINITE]
    assert values[-4:] == [0, 1, 2, 3] == [R.DETECTED, R.BODY_OCCLUDED, R.MISSED, R.NOT_FINITE]
    fields = re.findall(r"\b(\w+)\s*;", re.search(r"typedef struct smpc_detector_in \{(.*?)\}", src, flags=re.S).group(1))
    assert fields == [f[0] for f in DA.SmpcDetectorIn._fields_] and C.sizeof(DA.SmpcDetectorIn) == 96
    exported = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    lib = S.load_library()
    for name, (restype, argtypes) in DA.FUNCTIONS.items():
        assert f" {name}\n" in exported
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes


def test_the_main_abi_is_as_it_was():
    from nav2_social_mpc_controller_amd import _abi
    assert _abi.SMPC_ABI_VERSION == 6 and len(_abi.FUNCTIONS) == 27 and not set(DA.FUNCTIONS) & set(_abi.FUNCTIONS)
    structs = [v for v in vars(_abi).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]
    assert len(structs) == 19 and all(st.c_name != "smpc_detector_in" for st in structs)
    assert "SMPC_ABI_VERSION 6" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "smpc.h")).read())


# ---- the parameters -------------------------------------------------------------------------------------------------------
def test_detector_params():
    dp = DetectorParams()
    assert (dp.body_radius, dp.p_miss, dp.sigma, dp.sigma_growth, dp.clutter_candidates, dp.p_clutter, dp.clutter_range, dp.seed) == \
        (0.25, 0.1, 0.03, 0.002, 2, 0.05, 5.0, 0)
    assert dp.thresholds() == (429496730, 214748365) == R.thresholds(0.1, 0.05)              # round to nearest of p * 2^32
    assert DetectorParams(p_miss=0.0, p_clutter=1.0).thresholds() == (0, 2 ** 32 - 1)         # clamped
    assert DetectorParams(p_miss=0.5, p_clutter=2.0 ** -32).thresholds() == (2 ** 31, 1)
    assert DetectorParams(p_miss=1.5 * 2.0 ** -32).thresholds()[0] == 2                       # a half rounds upwards
    ref = R.params()
    assert dp.scales() == (float(ref["noise_scale"]), float(ref["noise_growth"]), float(ref["clutter_scale"]))
    assert DetectorParams(sigma=0.0, sigma_growth=0.0, clutter_range=4.0).scales() == (0.0, 0.0, 2.0 ** -29)
    assert abs(dp.scales()[0] * np.sqrt((2.0 ** 64 - 1.0) / 3.0) - 0.03) < 1e-15
    assert DetectorParams(seed=(456 << 32) | 123).key() == (123, 456) and DetectorParams(seed=2 ** 64 - 1).key() == (2 ** 32 - 1, 2 ** 32 - 1)
    assert dp.supported() and DetectorParams(clutter_candidates=64).supported() and not DetectorParams(clutter_candidates=65).supported()
    nan, inf = float("nan"), float("inf")
    for bad in (dict(body_radius=-0.1), dict(body_radius=nan), dict(p_miss=-0.1), dict(p_miss=1.1), dict(p_miss=nan), dict(sigma=-1.0),
                dict(sigma=inf), dict(sigma_growth=-1.0), dict(sigma_growth=nan), dict(clutter_candidates=-1), dict(clutter_candidates=1.5),
                dict(p_clutter=2.0), dict(p_clutter=nan), dict(clutter_range=-1.0), dict(clutter_range=inf), dict(seed=-1), dict(seed=2 ** 64),
                dict(seed=0.5)):
        with pytest.raises(ValueError):
            DetectorParams(**bad)
    di = S.BatchSolver.detector_c(DetectorParams(body_radius=0.5, p_miss=0.25, sigma=0.0, sigma_growth=0.0, clutter_candidates=3, p_clutter=0.5,
                                                 clutter_range=8.0, seed=(9 << 32) | 7), 5, 8, 11, 1)
    assert (di.B, di.Np, di.Nd, di.Kc, di.on_device, di.reserved, di.seed_lo, di.seed_hi) == (5, 8, 11, 3, 1, 0, 7, 9)
    assert (di.miss_threshold, di.clutter_threshold, di.body_radius, di.noise_scale, di.noise_growth, di.clutter_scale) == \
        (2 ** 30, 2 ** 31, 0.5, 0.0, 0.0, 2.0 ** -28) and not di.people


def test_the_episode_declares_the_argument():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, ShardedEpisode, TickRecord
    assert "detector" in BatchEpisode.FORWARDED and inspect.signature(BatchEpisode.__init__).parameters["detector"].default is None
    fields = TickRecord.__dataclass_fields__
    names = ("draw_state_before", "draw_state_after", "detected_persons", "detected_count", "detected_source", "person_outcome")
    assert all(fields[name].default is None for name in names)
    from nav2_social_mpc_controller_amd.episode_stages import Core, Detector, Tracker, Visibility
    at = BatchEpisode.STAGES.index                                                            # the launch order: Core begins with people_to_status
    assert at(Visibility) < at(Detector) < at(Tracker)
    assert at(Tracker) < at(Core) and Detector.TIMING == "detector"
    assert Detector.STATE == ("draw_state",)                                                  # saved and restored around the warm-up tick
    # a shard's robots draw by their ids in the whole batch: ShardedEpisode hands every shard its robots' stream ids
    assert callable(BatchEpisode.set_detector_streams) and "set_detector_streams(" in inspect.getsource(ShardedEpisode.__init__)


# ---- the kernel's resources ------------------------------------------------------------------------------------------------
def test_the_kernel_has_no_spills_and_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    r = subprocess.run(["bash", os.path.join(CSRC, "build.sh"), "-DSMPC_ONLY_NB=3", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage"],
                       env={**os.environ, "SMPC_OUT": str(tmp_path / "smpc_nb3.o")}, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    use = parse_resource_remarks(r.stderr).get(KERNEL)
    assert use is not None, "no resource remark for smpc_detect_people_kernel"
    print(use)
    assert use["VGPRs Spill"] == 0 and use["SGPRs Spill"] == 0 and use["ScratchSize [bytes/lane]"] == 0, use
    assert use["LDS Size [bytes/block]"] == 4 * 64 * (8 + 8), use
