// smpc_plan_smoother_rule.hpp — the rule of the plan smoothing (include/smpc_plan_smoother.h states the contract): which rows
// may move, one row's candidate of a Jacobi sweep and how far it moved, the cell test of a candidate, and what follows a sweep
// (go on, start a refinement, stop). The cell of a point and the passable test are those of smpc_global_plan_rule.hpp,
// included, not copied. Plain double arithmetic with one rounding per operation, integer arithmetic for the rest; no HIP call,
// no include beyond <stdint.h> and that header: the kernel (smpc_plan_smoother.hpp) and a host-only program
// (tests/test_plan_smoother.py) compile the same functions.
#pragma once
#include <stdint.h>

#include "smpc_global_plan_rule.hpp"

namespace smpc {

constexpr int kSmoothMaxPoses = 1024, kSmoothMaxIts = 100000, kSmoothMaxRefinements = 8;

// enum smpc_smooth_status
constexpr int32_t kSmoothConverged = 0, kSmoothMaxItsReached = 1, kSmoothTooShort = 2, kSmoothBadPlan = 3;

// what follows a sweep
constexpr int kSmSweep = 0, kSmNextRound = 1, kSmStop = 2;

struct SmMap {
  double ox, oy, res;       // the map's origin and resolution
  int32_t sx, sy;           // its size in cells
  uint32_t lethal_min;      // cost >= lethal_min is impassable
  uint32_t allow_unknown;   // ... except 255 when set
};

SMPC_GP_HD inline bool sm_finite(double v) {
  uint64_t u;
  __builtin_memcpy(&u, &v, sizeof(u));
  return (u & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

// rule 1: n, and the movable rows first .. last (r0, r1: the robot's range, or 1 and n - 2 without one). false: TOO_SHORT
SMPC_GP_HD inline int32_t sm_rows(int32_t plan_len, int32_t L) { return plan_len < 0 ? 0 : (plan_len > L ? L : plan_len); }
SMPC_GP_HD inline bool sm_movable(int32_t n, bool has_range, int32_t r0, int32_t r1, int32_t* first, int32_t* last) {
  *first = has_range && r0 > 1 ? r0 : 1;
  *last = has_range && r1 < n - 2 ? r1 : n - 2;
  return n >= 3 && *first <= *last;
}

// rule 3, one axis of one row: p the round's starting row, y the row, ym and yp rows i - 1 and i + 1 of the previous iterate
SMPC_GP_HD inline double sm_candidate(double p, double y, double ym, double yp, double w_data, double w_smooth) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double a = p - y;
  const double b = w_data * a;
  const double s = yp + ym;
  const double d = y + y;
  const double e = s - d;
  const double f = w_smooth * e;
  const double g = b + f;
  return y + g;
}

// |h|, h = c - y
SMPC_GP_HD inline double sm_moved(double c, double y) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double h = c - y;
  return __builtin_fabs(h);
}

// the cell of a candidate as an index into the map, when it has one
SMPC_GP_HD inline bool sm_cell(const SmMap& m, double cx, double cy, int32_t* idx) {
  int32_t ix = 0, iy = 0;
  if (!gp_cell_axis(cx, m.ox, m.res, m.sx, &ix)) return false;
  if (!gp_cell_axis(cy, m.oy, m.res, m.sy, &iy)) return false;
  *idx = iy * m.sx + ix;   // below 2^31 (checked by the host)
  return true;
}

SMPC_GP_HD inline bool sm_passable(const SmMap& m, uint32_t v) {
  const GpCost c = {0, 0, m.lethal_min, m.allow_unknown};
  return gp_passable(c, v);
}

// A row's last verdict, so that a candidate in the same cell need not read the map again: the cell's index and whether it
// is passable in one word; kSmNoVerdict: none yet.
constexpr uint32_t kSmNoVerdict = 0xFFFFFFFFu;
SMPC_GP_HD inline uint32_t sm_verdict(int32_t idx, bool passable) { return ((uint32_t)idx << 1) | (passable ? 1u : 0u); }
SMPC_GP_HD inline bool sm_verdict_is_of(uint32_t verdict, int32_t idx) { return verdict != kSmNoVerdict && (verdict >> 1) == (uint32_t)idx; }
SMPC_GP_HD inline bool sm_verdict_passable(uint32_t verdict) { return (verdict & 1u) != 0u; }

// rule 4: where a robot stands between its sweeps
struct SmProgress {
  int32_t sweeps, rounds, its, refinements;   // all sweeps; rounds ended; sweeps of this round; refinements started
  int32_t status;
};

SMPC_GP_HD inline SmProgress sm_start() { return SmProgress{0, 0, 0, 0, kSmoothConverged}; }

// After a sweep; within: its change was <= tolerance. kSmNextRound: the caller sets p := y and sweeps on.
SMPC_GP_HD inline int sm_after_sweep(SmProgress& s, bool within, int32_t max_its, int32_t refinement_num) {
  ++s.sweeps;
  ++s.its;
  if (within) {
    ++s.rounds;
    s.its = 0;
    if (s.refinements < refinement_num) { ++s.refinements; return kSmNextRound; }
    s.status = kSmoothConverged;
    return kSmStop;
  }
  if (s.its >= max_its) {
    ++s.rounds;
    s.status = kSmoothMaxItsReached;
    return kSmStop;
  }
  return kSmSweep;
}

// the most sweeps a robot can run: the bound of the kernel's only open loop
SMPC_GP_HD inline int64_t sm_sweep_bound(int32_t max_its, int32_t refinement_num) { return (int64_t)max_its * ((int64_t)refinement_num + 1); }

// rule 5: the rejected candidates, saturating
SMPC_GP_HD inline int32_t sm_saturate(uint64_t rejected) { return rejected > 0x7FFFFFFFull ? 0x7FFFFFFF : (int32_t)rejected; }

}  // namespace smpc
