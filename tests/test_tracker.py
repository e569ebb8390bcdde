"""The people tracker on the CPU: the yardstick itself (tests/tracker_ref.py: all qualifying pairs sorted and accepted
greedily) on hand-made sequences with the expected state written out, the `__host__ __device__` rule of
csrc/smpc_tracker_rule.hpp compiled into a host-only program and composed as the kernel composes it (rounds of per-slot
best pairs, births and output rows by ranks) against the yardstick, the ctypes mirror against include/smpc_tracker.h,
TrackerParams, the episode's declarations, the kernel's resource remarks, and that the seeded sequences exercise what the
feature adds."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import tracker_cases as TC
import tracker_ref as R
from nav2_social_mpc_controller_amd import _abi_tracker as TA
from nav2_social_mpc_controller_amd import solver as S
from nav2_social_mpc_controller_amd.params import TrackerParams
from test_kernel_budget import CSRC, HIPCC, parse_resource_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smpc_tracker.h")
KERNEL = "_ZN4smpc24smpc_track_people_kernelENS_13TrackerParamsE"

HAND = TC.hand_sequences()
SEEDED = TC.seeded_sequences()


@pytest.fixture(scope="module")
def seeded_ref():
    """name -> the yardstick's ticks of a seeded sequence: [(tick, state before, new state, outputs, counters)]."""
    out = {}
    for name, seq in SEEDED.items():
        state, ticks = tuple(np.array(a) for a in seq["state0"]), []
        for tick in seq["ticks"]:
            new, outs, counters = R.step(state, tick["det"], tick["count"], tick["pose"], seq["p"])
            ticks.append((tick, state, new, outs, counters))
            state = new
        out[name] = ticks
    return out


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_sequences_leave_the_state_the_contract_gives(name):
    seq = HAND[name]
    for t, tick, before, new, outs in TC.run(seq, TC.ref_call):
        assert tick["want"] is not None
        TC.check_want(new, outs, tick["want"])
        people, count, source = outs
        B = len(count)
        assert all(np.isnan(people[b, count[b]:]).all() and (source[b, count[b]:] == -1).all() for b in range(B)), (name, t)
        assert new[0].dtype == np.float64 and new[1].dtype == np.int32 and new[2].dtype == np.int32 and count.dtype == np.int32


def test_the_seeded_sequences_exercise_the_tracker(seeded_ref):
    """By the yardstick alone, before anything is compared with it: every counter fires, at least a tenth of the live
    slot-ticks coast, and an exact tie of d2 is resolved by the indices."""
    total = dict.fromkeys(R.COUNTERS, 0)
    for ticks in seeded_ref.values():
        for _, _, _, _, counters in ticks:
            for k in R.COUNTERS:
                total[k] += int(counters[k].sum())
    assert all(total[k] >= 1 for k in R.COUNTERS), total
    live = total["matched"] + total["coasted"] + total["freed_by_misses"] + total["tentative_freed"]
    assert total["coasted"] >= 0.1 * live, total
    for name, ticks in seeded_ref.items():                                                # and shape by shape something is handed on
        assert sum(int(outs[1].sum()) for _, _, _, outs, _ in ticks) >= 1, name


def test_the_dense_limit_matches_every_slot_every_tick():
    seq = TC.dense_limit_sequence()
    state = seq["state0"]
    for t, tick in enumerate(seq["ticks"]):
        state, outs, counters = R.step(state, tick["det"], tick["count"], tick["pose"], seq["p"])
        assert (counters["born" if t == 0 else "matched"] == 64).all() and (outs[1] == 64).all()


# ---- the compiled rule ------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include "smpc_tracker_rule.hpp"

static double num(const std::string& s) { return std::strtod(s.c_str(), nullptr); }   // hex floats, nan, inf
static std::string hex(double v) { char b[40]; uint64_t u; std::memcpy(&u, &v, 8); std::snprintf(b, sizeof b, "%016llx", (unsigned long long)u); return b; }

// One robot per input line, composed as the kernel composes the rule: a slot per "lane", rounds of per-slot best pairs over
// the detections still available, the least key's lowest slot wins, births and output rows by ranks.
int main() {
  long long Nt, Nd, Np, confirm, max_missed, count, next_id;
  while (std::cin >> Nt >> Nd >> Np >> confirm >> max_missed >> count >> next_id) {
    std::string w;
    double sc[6];
    for (double& v : sc) { std::cin >> w; v = num(w); }
    const double dt = sc[0], alpha = sc[1], gain = sc[2], gate = sc[3], px = sc[4], py = sc[5];
    std::vector<double> x(Nt), y(Nt), vx(Nt), vy(Nt), xp(Nt), yp(Nt), zx(Nd), zy(Nd);
    std::vector<int32_t> state(Nt), hits(Nt), missed(Nt), id(Nt);
    for (long long i = 0; i < Nt; ++i) {
      std::cin >> w; x[i] = num(w); std::cin >> w; y[i] = num(w); std::cin >> w; vx[i] = num(w); std::cin >> w; vy[i] = num(w);
    }
    for (long long i = 0; i < Nt; ++i) { long long a, b, c, d; std::cin >> a >> b >> c >> d; state[i] = (int32_t)a; hits[i] = (int32_t)b; missed[i] = (int32_t)c; id[i] = (int32_t)d; }
    for (long long j = 0; j < Nd; ++j) { std::cin >> w; zx[j] = num(w); std::cin >> w; zy[j] = num(w); }
    if (Nt > 64 || Nd > 64 || Np > 64) std::abort();
    std::vector<char> live(Nt), matched(Nt, 0);
    for (long long i = 0; i < Nt; ++i) {
      live[i] = smpc::tk_live(state[i], x[i], y[i], vx[i], vy[i]);
      if (!live[i]) { x[i] = y[i] = vx[i] = vy[i] = 0.0; state[i] = hits[i] = missed[i] = id[i] = 0; }
      xp[i] = smpc::tk_predict(x[i], vx[i], dt); yp[i] = smpc::tk_predict(y[i], vy[i], dt);
    }
    const long long n = count < 0 ? 0 : (count > Nd ? Nd : count);
    uint64_t avail = 0;
    for (long long j = 0; j < n; ++j) if (smpc::tk_finite(zx[j]) && smpc::tk_finite(zy[j])) avail |= 1ull << j;
    const double gate2 = smpc::tk_gate2(gate);
    std::vector<long long> match_j(Nt, 0);
    const long long rounds = Nt < Nd ? Nt : Nd;
    for (long long r = 0; r < rounds && avail; ++r) {
      uint64_t least = smpc::kTrackNoKey; long long wi = -1, wj = -1;
      for (long long i = 0; i < Nt; ++i) {
        if (!live[i] || matched[i]) continue;
        uint64_t nb = smpc::kTrackNoKey; long long nj = 0;
        for (long long j = 0; j < 64; ++j) {
          if (!((avail >> j) & 1ull)) continue;
          const uint64_t k = smpc::tk_pair_key(zx[j], zy[j], xp[i], yp[i], gate2);
          if (k < nb) { nb = k; nj = j; }
        }
        if (nb < least) { least = nb; wi = i; wj = nj; }
      }
      if (least == smpc::kTrackNoKey) break;
      matched[wi] = 1; match_j[wi] = wj; avail &= ~(1ull << wj);
    }
    for (long long i = 0; i < Nt; ++i) {
      if (!live[i]) continue;
      if (matched[i]) {
        const double rx = zx[match_j[i]] - xp[i], ry = zy[match_j[i]] - yp[i];
        x[i] = smpc::tk_update(xp[i], alpha, rx); y[i] = smpc::tk_update(yp[i], alpha, ry);
        vx[i] = smpc::tk_update(vx[i], gain, rx); vy[i] = smpc::tk_update(vy[i], gain, ry);
        hits[i] = smpc::tk_hit(hits[i]); missed[i] = 0;
        if (state[i] == smpc::kTrackTentative && hits[i] >= confirm) state[i] = smpc::kTrackConfirmed;
      } else {
        x[i] = xp[i]; y[i] = yp[i]; missed[i] = smpc::tk_miss(missed[i]);
        if (!smpc::tk_survives_miss(state[i], missed[i], (int32_t)max_missed)) { x[i] = y[i] = vx[i] = vy[i] = 0.0; state[i] = hits[i] = missed[i] = id[i] = 0; }
      }
    }
    std::vector<long long> born, free_slots;
    for (long long j = 0; j < 64; ++j) if ((avail >> j) & 1ull) born.push_back(j);
    for (long long i = 0; i < Nt; ++i) if (state[i] == smpc::kTrackFree) free_slots.push_back(i);
    const size_t n_born = born.size() < free_slots.size() ? born.size() : free_slots.size();
    const uint32_t first_id = (uint32_t)(int32_t)next_id;
    for (size_t f = 0; f < n_born; ++f) {
      const long long i = free_slots[f], j = born[f];
      x[i] = zx[j]; y[i] = zy[j]; vx[i] = vy[i] = 0.0;
      state[i] = smpc::tk_birth_state((int32_t)confirm); hits[i] = 1; missed[i] = 0; id[i] = (int32_t)(first_id + (uint32_t)f);
    }
    std::string out;
    for (long long i = 0; i < Nt; ++i) out += hex(x[i]) + "," + hex(y[i]) + "," + hex(vx[i]) + "," + hex(vy[i]) + ",";
    out += " ";
    for (long long i = 0; i < Nt; ++i) out += std::to_string(state[i]) + "," + std::to_string(hits[i]) + "," + std::to_string(missed[i]) + "," + std::to_string(id[i]) + ",";
    out += " " + std::to_string((int32_t)(first_id + (uint32_t)n_born)) + " ";
    long long n_out = 0;
    std::string rows = "|";
    if (smpc::tk_finite(px) && smpc::tk_finite(py)) {
      std::vector<uint64_t> key(Nt, smpc::kTrackNoKey);
      long long n_conf = 0;
      for (long long i = 0; i < Nt; ++i) if (state[i] == smpc::kTrackConfirmed) { key[i] = smpc::tk_out_key(x[i], y[i], px, py); ++n_conf; }
      n_out = n_conf < Np ? n_conf : Np;
      for (long long i = 0; i < Nt; ++i) {
        if (state[i] != smpc::kTrackConfirmed) continue;
        long long rank = 0;
        for (long long k = 0; k < Nt; ++k)
          if (state[k] == smpc::kTrackConfirmed && smpc::tk_key_less(key[k], (uint32_t)k, key[i], (uint32_t)i)) ++rank;
        if (rank < Np) rows += std::to_string(rank) + "," + std::to_string(i) + "," + std::to_string(id[i]) + "|";
      }
    }
    std::printf("%s%lld %s\n", out.c_str(), n_out, rows.c_str());
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    tmp = tmp_path_factory.mktemp("tracker_rule")
    src, exe = tmp / "probe.hip", tmp / "probe"
    src.write_text(PROBE)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])   # -O3 as build.sh

    def call(state, tick, p, people=None, source=None):
        tracks, meta, next_id = state
        det, B, Nt, Np = np.asarray(tick["det"], np.float64), len(tick["count"]), p["Nt"], p["Np"]
        Nd = det.shape[1]
        hx = lambda v: float(v).hex() if np.isfinite(v) else repr(float(v))
        lines = []
        for b in range(B):
            lines.append(" ".join(map(str, [Nt, Nd, Np, p["confirm_hits"], p["max_missed"], int(tick["count"][b]), int(next_id[b])]
                                      + [hx(v) for v in (p["dt"], p["alpha"], p["gain"], p["gate"], tick["pose"][b][0], tick["pose"][b][1])]
                                      + [hx(v) for v in np.asarray(tracks[b]).ravel()] + [int(v) for v in np.asarray(meta[b]).ravel()]
                                      + [hx(v) for v in det[b, :, :2].ravel()])))
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == B
        new_t, new_m, new_n = np.zeros((B, Nt, 4)), np.zeros((B, Nt, 4), np.int32), np.zeros(B, np.int32)
        people = np.full((B, Np, 5), np.nan) if people is None else np.array(people, np.float64)
        source = np.full((B, Np, 2), -1, np.int32) if source is None else np.array(source, np.int32)
        count = np.zeros(B, np.int32)
        for b, line in enumerate(out):
            t, m, nid, cnt, rows = line.split()
            new_t[b] = np.array([int(v, 16) for v in t.split(",")[:-1]], np.uint64).view(np.float64).reshape(Nt, 4)
            new_m[b] = np.array([int(v) for v in m.split(",")[:-1]]).reshape(Nt, 4)
            new_n[b], count[b] = int(nid), int(cnt)
            written = [tuple(int(v) for v in r.split(",")) for r in rows.split("|") if r]
            assert sorted(r[0] for r in written) == list(range(count[b]))
            for rank, i, tid in written:
                people[b, rank] = [*new_t[b, i], 0.0]
                source[b, rank] = [i, tid]
        return (new_t, new_m, new_n), (people, count, source)

    return call


def test_compiled_rule_is_the_yardstick_on_the_hand_made_sequences(rule):
    for name, seq in HAND.items():
        for t, tick, before, new, outs in TC.run(seq, rule):
            assert TC.same((new, outs), TC.ref_call(before, tick, seq["p"])), (name, t)
            TC.check_want(new, outs, tick["want"])


def test_compiled_rule_is_the_yardstick_on_the_seeded_sequences(rule, seeded_ref):
    for name, ticks in seeded_ref.items():
        p = SEEDED[name]["p"]
        for t, (tick, before, new, outs, _) in enumerate(ticks):
            assert TC.same(rule(before, tick, p), (new, outs)), (name, t)


def test_compiled_rule_is_the_yardstick_on_the_dense_limit(rule):
    seq = TC.dense_limit_sequence()
    for t, tick, before, new, outs in TC.run(seq, rule):
        assert TC.same((new, outs), TC.ref_call(before, tick, seq["p"])), t


def test_the_rule_header_rounds_every_operation_on_its_own():
    text = open(os.path.join(CSRC, "smpc_tracker_rule.hpp")).read()
    assert text.count("#pragma clang fp contract(off)") >= 6 and "fma(" not in text
    assert '#include "smpc_tracker_rule.hpp"' in open(os.path.join(CSRC, "smpc_tracker.hpp")).read()


# ---- the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mirror_matches_the_header_and_the_library_exports_the_function(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(smpc_[a-z0-9_]+)\s*\(", src))) == sorted(TA.FUNCTIONS) == ["smpc_track_people_batch"]
    assert re.findall(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*(\w+)\s*;", src, flags=re.S) == [st.c_name for st in TA.STRUCTS]
    body = "".join(f'printf("%zu\\n", sizeof({st.c_name}));\n' + "".join(f'printf("%zu\\n", offsetof({st.c_name}, {f[0]}));\n' for f in st._fields_)
                   for st in TA.STRUCTS)
    body += 'printf("%d %d %d\\n", SMPC_TRACK_FREE, SMPC_TRACK_TENTATIVE, SMPC_TRACK_CONFIRMED);\n'
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc_tracker.h"\nint main(void){\n' + body + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    values = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [v for st in TA.STRUCTS for v in [C.sizeof(st)] + [getattr(st, f[0]).offset for f in st._fields_]]
    assert values == want + [TA.SMPC_TRACK_FREE, TA.SMPC_TRACK_TENTATIVE, TA.SMPC_TRACK_CONFIRMED] and values[-3:] == [0, 1, 2]
    fields = re.findall(r"\b(\w+)\s*(?:,|;)", re.search(r"typedef struct smpc_tracker_in \{(.*?)\}", src, flags=re.S).group(1))
    assert fields == [f[0] for f in TA.SmpcTrackerIn._fields_] and C.sizeof(TA.SmpcTrackerIn) == 88
    exported = subprocess.check_output(["nm", "-D", "--defined-only", S.LIB_PATH], text=True)
    lib = S.load_library()
    for name, (restype, argtypes) in TA.FUNCTIONS.items():
        assert f" {name}\n" in exported
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes


def test_the_main_abi_is_as_it_was():
    from nav2_social_mpc_controller_amd import _abi
    assert _abi.SMPC_ABI_VERSION == 6 and len(_abi.FUNCTIONS) == 27 and not set(TA.FUNCTIONS) & set(_abi.FUNCTIONS)
    assert "SMPC_ABI_VERSION 6" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "smpc.h")).read())


# ---- the parameters -------------------------------------------------------------------------------------------------------
def test_tracker_params():
    tp = TrackerParams()
    assert (tp.alpha, tp.beta, tp.gate, tp.confirm_hits, tp.max_missed, tp.slots) == (0.5, 0.2, 0.6, 3, 20, 16)
    assert tp.gain(0.1) == float(np.float64(0.2) / np.float64(0.1)) and TrackerParams(beta=0.25).gain(0.125) == 2.0
    assert tp.supported() and tp.supported(0.1) and TrackerParams(slots=64).supported() and not TrackerParams(slots=65).supported()
    assert not tp.supported(0.0) and not tp.supported(np.nan) and not TrackerParams(beta=1e300).supported(1e-300)
    for bad in (dict(alpha=-0.1), dict(alpha=np.nan), dict(beta=-1.0), dict(beta=np.inf), dict(gate=0.0), dict(gate=np.nan),
                dict(confirm_hits=0), dict(confirm_hits=1.5), dict(max_missed=-1), dict(slots=0)):
        with pytest.raises(ValueError):
            TrackerParams(**bad)
    for dt in (0.0, -0.1, np.nan, np.inf):
        with pytest.raises(ValueError):
            tp.gain(dt)
    ti = S.BatchSolver.tracker_c(TrackerParams(alpha=0.25, beta=0.5, gate=0.75, confirm_hits=2, max_missed=7, slots=12), 5, 8, 6, 0.125, 1)
    assert (ti.B, ti.Nd, ti.Nt, ti.Np, ti.on_device, ti.confirm_hits, ti.max_missed, ti.reserved) == (5, 8, 12, 6, 1, 2, 7, 0)
    assert (ti.dt, ti.alpha, ti.gain, ti.gate) == (0.125, 0.25, 4.0, 0.75) and not ti.detections


def test_the_episode_declares_the_argument():
    from nav2_social_mpc_controller_amd.episode import BatchEpisode, TickRecord
    assert "tracker" in BatchEpisode.FORWARDED and inspect.signature(BatchEpisode.__init__).parameters["tracker"].default is None
    fields = TickRecord.__dataclass_fields__
    names = ("tracks_before", "track_meta_before", "track_next_id_before", "tracks_after", "track_meta_after", "track_next_id_after",
             "tracked_persons", "tracked_count", "tracked_source")
    assert all(fields[name].default is None for name in names)
    from nav2_social_mpc_controller_amd.episode_stages import Core, Tracker, Visibility
    at = BatchEpisode.STAGES.index                                                            # the launch order: Core begins with people_to_status
    assert at(Tracker) < at(Core) and Tracker.TIMING == "tracker"
    assert at(Visibility) < at(Tracker)


# ---- the kernel's resources ------------------------------------------------------------------------------------------------
def test_the_kernel_has_no_spills_no_scratch_and_full_occupancy(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip(f"{HIPCC} (the compiler build.sh invokes) not available")
    r = subprocess.run(["bash", os.path.join(CSRC, "build.sh"), "-DSMPC_ONLY_NB=3", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage"],
                       env={**os.environ, "SMPC_OUT": str(tmp_path / "smpc_nb3.o")}, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    use = parse_resource_remarks(r.stderr).get(KERNEL)
    assert use is not None, "no resource remark for smpc_track_people_kernel"
    assert use["VGPRs Spill"] == 0 and use["SGPRs Spill"] == 0 and use["ScratchSize [bytes/lane]"] == 0, use
    assert use["LDS Size [bytes/block]"] == 4 * 64 * (8 + 8 + 4) and use["Occupancy [waves/SIMD]"] == 8, use
