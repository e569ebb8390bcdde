// smpc_solve_body.inc — the body of the solve kernels, included by smpc_solve_kernel.hpp inside each of them:
// smpc_solve_kernel<NB, W, kVT, kSP, kTrace> (Shape = RuntimeShape) and smpc_solve_fixed_kernel<Shape>. The including
// kernel provides NB, W, kVT, kSP, kTrace and Shape. Text, not a device function: see the note in smpc_solve_kernel.hpp.
  static_assert(!kSP || kVT, "a kernel with per-scene weights and bounds reads its horizon per scene as well");
  static_assert(!kTrace || (kVT && kSP), "the trace is compiled for the most general variant only");
  const auto& k = *(KParamsK)__builtin_amdgcn_kernarg_segment_ptr();
  constexpr int P = 2 * NB;
  constexpr int S = kWave / W;
  constexpr bool kLone = lone_trip_kernel(W, kVT, kSP, kTrace);
  extern __shared__ __attribute__((aligned(32))) double lds_all[];
  const int lane = threadIdx.x & 63;
  Ctx c;
  c.kp = &k;
  c.L = make_layout(Shape::T(k), Shape::N(k), P, kLayoutSolve, W, kSP);
  c.ag = k.people_rec;
  {
    double* atab = lds_all + atan_tab_offset(S * c.L.total, wave_extra_doubles(P, W));
    load_atan_nodes(c.kp, atab, lane);
    c.atab = atab;
  }
  const auto& prm = k.prm;
  const int T = Shape::T(k);
  // Everything below is derived from the lane index. It is re-derived at the top of every trip and again behind the
  // sweep from a copy of the lane index the compiler cannot see through (an empty asm): otherwise these ~20 addresses
  // and flags are computed once in the prologue, stay live through the whole kernel — the sweep runs at the VGPR limit —
  // and come back as scratch reloads inside the loop.
  int slot, q, qc;
  bool act;
  double *Hs, *Lw, *gs, *gu, *xc, *xt, *dl, *sc, *bc, *rs, *sv, *scratch;
  int32_t* rw;
  auto bind = [&](int lane_t) {
    slot = lane_t / W;
    c.sl = lane_t - slot * W;
    c.slot = slot;
    c.lds = lds_all + (size_t)slot * c.L.total;
    c.wave_lds = lds_all + (size_t)S * c.L.total;
    Hs = c.lds + c.L.lm;   // [P][P] scaled J^T J at the current point, dense
    gs = Hs + P * P;       // [P] scaled gradient
    gu = gs + P;           // [P] unscaled gradient
    xc = gu + P;           // [P] current point
    xt = xc + P;           // [P] trial point (input of the sweep)
    dl = xt + P;           // [P] delta (unscaled step of this iteration)
    sc = dl + P;           // [P] Jacobi scaling
    sv = sc + P;           // scalars [24]
    rw = reinterpret_cast<int32_t*>(sv + S_COUNT);  // the state machine's integers, parked across the sweep
    // temporaries of the LM algebra: over the sweep's cos / sin block, scans and Gram reduction buffer (all dead here)
    Lw = c.lds + c.L.cs;   // [P][P] rows of the Cholesky factor of the damped system
    bc = Lw + P * P;       // [4][P] hand-over words: pivots, forward / backward solutions, scaled step
    rs = bc + 4 * P;       // [3][P] reduction words (every site uses the same three rows: LDS operations of a wave
                           //        execute in program order, a site's reads are behind it before the next site writes)
    scratch = rs + 3 * P;  // [96] generic line-search interpolation fallback
    q = c.sl;              // the parameter this lane owns in the LM algebra
    act = q < P;
    qc = act ? q : 0;      // in-range index for lanes that only tag along
  };
  bind(lane);
  auto slot_any = [&](bool pred) -> bool {
    const unsigned long long slot_bits = (W == 64) ? ~0ull : (0xffffffffull << (32 * slot));
    return (__ballot(pred) & slot_bits) != 0ull;
  };
  // sums / maximum over the parameters: every active lane leaves its terms in the site's words, then every lane adds
  // them up in index order. One form per need — a sum (row 0), two sums (rows 0 and 1), a sum and a maximum (rows 0 and
  // 2) — so that a site pays for the channels it uses; each channel is the same in every form.
  auto reduce_sum = [&](double a, double& sa) {
    double* w3 = rs;
    if (act) w3[q] = a;
    wave_lds_fence();
    sa = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) sa += w3[i];
  };
  auto reduce_sum2 = [&](double a, double b, double& sa, double& sb) {
    double* w3 = rs;
    if (act) { w3[q] = a; w3[P + q] = b; }
    wave_lds_fence();
    sa = 0.0; sb = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) { sa += w3[i]; sb += w3[P + i]; }
  };
  // The maximum as one v_max_f64 per term: fmax() canonicalises both operands first (13 instructions for six maxima).
  // The terms are fabs() of arithmetic results, never a signalling NaN, and a quiet NaN is dropped by the instruction as
  // fmax() drops it: the maximum of the other terms comes out, as ever.
  auto reduce_sum_max = [&](double a, double m, double& sa, double& sm) {
    double* w3 = rs;
    if (act) { w3[q] = a; w3[2 * P + q] = m; }
    wave_lds_fence();
    sa = 0.0; sm = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      sa += w3[i];
      const double mi = w3[2 * P + i];
      asm("v_max_f64 %0, %1, %2" : "=v"(sm) : "v"(sm), "v"(mi));
    }
  };

  // kTrace: row `row` of the slot's scene, columns in the order of smpc_trace_out (iter is the row index itself)
  auto trace_row = [&](int row, double cost, double cost_change, double gmax, double step_norm, double rho, double radius,
                       int ls_evals, bool accepted) {
    const auto& kt = *c.kp;
    if (row >= kt.trace_rows || c.sl >= kTraceCols) return;
    const int j = c.sl;
    const double v = j == 0 ? (double)row : j == 1 ? cost : j == 2 ? cost_change : j == 3 ? gmax : j == 4 ? step_norm
                   : j == 5 ? rho : j == 6 ? radius : j == 7 ? (double)ls_evals : (accepted ? 1.0 : 0.0);
    kt.o_trace[((size_t)c.scene * kt.trace_rows + row) * kTraceCols + j] = v;
  };

  // The state machine's integers and flags live in LDS across the sweep (behind the scalars of sv[]): only the phase
  // stays in a register there. The sweep is the register-hungry part of a trip; nothing of the LM bookkeeping should
  // take room in it.
  LmRegs R;
  R.phase = PH_FETCH;
  R.iter = R.evals = R.num_invalid = R.ls_iters = R.n_samples = 0;
  R.status = SMPC_NO_CONVERGENCE; R.reason = SMPC_REASON_MAX_ITERATIONS;
  R.flags = 0;
  auto park = [&]() {
    rw[0] = R.iter; rw[1] = R.evals; rw[2] = R.num_invalid; rw[3] = R.ls_iters; rw[4] = R.n_samples; rw[5] = R.status;
    rw[6] = R.reason; rw[7] = R.flags;
  };
  auto unpark = [&]() {
    R.iter = rw[0]; R.evals = rw[1]; R.num_invalid = rw[2]; R.ls_iters = rw[3]; R.n_samples = rw[4]; R.status = rw[5];
    R.reason = rw[6]; R.flags = rw[7];
  };
  bool ever_loaded = false;
  // kLone: this wave's trips, those with one slot idle for good and those helped, 21 bits each in one word of LDS behind
  // the state machine's parked integers (each slot keeps the wave's count; a wave makes far fewer than 2^21 trips)
  // Counted only in a launch that reports the counts (kLoneCount of KParams::lone_trips): a trip of any other launch pays
  // one scalar test for it.
  if constexpr (kLone) *reinterpret_cast<unsigned long long*>(rw + 8) = 0ull;
#ifdef SMPC_STAMPS
  for (int i = 0; i < 8; ++i) c.acc[i] = 0;
  for (int i = 0; i < 4; ++i) c.acc2[i] = 0;
  c.t_last = __builtin_amdgcn_s_memtime();
#endif

  for (;;) {
    SMPC_STAMP(c, 6);  // LM state machine + output stage of the previous trip
    // Like everything derived from the lane index (above), everything derived from the launch parameters is re-derived
    // per trip, behind an opaque copy of the argument pointer: sign extensions of T and N, "N > 1", the LDS layout's
    // offsets, ... computed once in the prologue are ~20 scalar registers live through the whole kernel — more than the
    // file has left; they came back as v_writelane / v_readlane spill traffic (22 spilled SGPRs in <3,32>, 70 in <5,64>;
    // now 4 and 33). A few dozen scalar instructions and cached scalar loads per trip.
    {
      KParamsK kp_t = c.kp;
      asm volatile("" : "+s"(kp_t));
      c.kp = kp_t;
    }
    const auto& k = *c.kp;
    const auto& prm = k.prm;
    const int T = Shape::T(k);
    if constexpr (!Shape::kFixed) c.L = make_layout(Shape::T(k), Shape::N(k), P, kLayoutSolve, W, kSP);  // (literals otherwise)
    {
      int lane_t = lane;
      asm volatile("" : "+v"(lane_t));
      bind(lane_t);
    }
    // ---------------------------------------------------------------- fetch the next scene for idle slots
    if (R.phase == PH_FETCH) {
      int scene = 0;
      if (c.sl == 0) {
        scene = atomicAdd(k.queue, 1);
        if (k.order) {  // the caller's order (longest scenes first); an entry outside the batch is skipped
          while (scene < k.B) {
            const int want = k.order[scene];
            if (want >= 0 && want < k.B) { scene = want; break; }
            scene = atomicAdd(k.queue, 1);
          }
        }
      }
      scene = __shfl(scene, slot * W, 64);
      if (scene < k.B) {
        load_scene<W, kVT, kSP, Shape, Shape::kStageAtFetch>(c, scene);
        ever_loaded = true;
        wave_lds_fence();
        const Horizon hz0 = get_horizon<NB, kVT, Shape>(c);
        double v = 0.0;
        if (act && (q >> 1) <= hz0.blast) {  // a scene with fewer blocks than NB keeps the surplus parameters at zero
          const bool bnd = (q >> 1) < hz0.nbounded;
          const double lo0 = bnd ? ((q & 1) ? SMPC_SCENE_PRM(c, kSP, prm, w_min) : SMPC_SCENE_PRM(c, kSP, prm, v_min)) : -1.7976931348623157e308;
          const double hi0 = bnd ? ((q & 1) ? SMPC_SCENE_PRM(c, kSP, prm, w_max) : SMPC_SCENE_PRM(c, kSP, prm, v_max)) : 1.7976931348623157e308;
          v = clampd(k.init_params[(size_t)scene * P + q] + 0.0, lo0, hi0);  // Plus(x, 0): project the start point (A.4)
        }
        if (act) { xc[q] = v; xt[q] = v; }
        double xn;
        reduce_sum(v * v, xn);
        sv[S_XNORM] = fast_sqrt(xn);
        R.phase = PH_INIT;
        R.iter = 0; R.evals = 0; R.num_invalid = 0;
        R.status = SMPC_NO_CONVERGENCE; R.reason = SMPC_REASON_MAX_ITERATIONS;
        R.set(LF_STEP_SUCCESSFUL, true); R.set(LF_AT_LEAST_ONE, false);
      } else {
        if (!ever_loaded) {  // keep the sweep's memory accesses in bounds for a slot that never got a scene
          load_scene<W, kVT, kSP, Shape, Shape::kStageAtFetch>(c, 0, false);  // (a kernel that stages at the fetch: not here)
          ever_loaded = true;
          if (act) xt[q] = 0.0;
        }
        R.phase = PH_IDLE;
      }
    }
    if (__all(R.phase == PH_IDLE)) break;
    SMPC_STAMP(c, 0);  // fetch + load_scene
    if constexpr (kLone) {
      // A lone trip: one slot is idle — for good, PH_IDLE is final — and the other works on a scene with people and
      // N >= 2. Its agent loop is shared between the halves (sweep(), trip_mode()). Decided for the wave; a paired trip pays two
      // ballots and a scalar branch.
      const bool idle = R.phase == PH_IDLE;
      const unsigned long long ib = __ballot(idle);
      const bool half = ((ib ^ (ib >> 32)) & 1ull) != 0ull;  // (the phase is uniform over a slot)
      const bool lone = half && (k.lone_trips & kLoneHelp) != 0 && Shape::N(k) >= 2 && __ballot(!idle && c.has_people) != 0ull;
      *trip_mode(c) = !lone ? kTripPaired : idle ? kTripHelper : kTripOwner;
      if (k.lone_trips & kLoneCount) *reinterpret_cast<unsigned long long*>(rw + 8) += 1ull + (half ? 1ull << 21 : 0ull) + (lone ? 1ull << 42 : 0ull);
    }
    if (k.prio_step > 0) {
      // Attained-service priority: the launch ends when its longest scene does, and a scene's sweeps are a dependent
      // chain — so the longer a scene has been running, the more of the SIMD's issue slots its wave gets against the
      // younger waves beside it (which, having made few sweeps, most likely hold short scenes: lengths 11..146).
      const int mine = (R.phase == PH_IDLE) ? 0 : R.evals;
      int age = __builtin_amdgcn_readfirstlane(mine);
      if (S == 2) age = max(age, __builtin_amdgcn_readlane(mine, 32));
      const int step = k.prio_step;
      if (age >= 3 * step) __builtin_amdgcn_s_setprio(3);
      else if (age >= 2 * step) __builtin_amdgcn_s_setprio(2);
      else if (age >= step) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }

    // ---------------------------------------------------------------- one sweep for every slot of the wave
    park();
    // What the slot needs of this sweep: the whole Gram where the point can be adopted (the initial point, a sample that
    // passes the Armijo test, a re-evaluation), its last column — cost and gradient — where the sample only feeds the
    // line search's interpolation (the common case: 19 of a solve's 52 sweeps are adopted on the headline workload).
    const int phase_at_sweep = R.phase;
    auto need_rest = [&]() -> bool {
      if (phase_at_sweep != PH_LS) return phase_at_sweep != PH_IDLE;
      if (k.full_gram) return true;
      const double* gt = c.lds + c.L.gram;
      const double* svp = c.lds + c.L.lm + P * P + 6 * P;
      const unsigned long long slot_bits = (W == 64) ? ~0ull : (0xffffffffull << (32 * c.slot));
      // a non-finite residual or Jacobian entry shows in this column too (a product with it is not finite): only then,
      // and then always, the diagonal is formed as well and decides as before
      const bool col_finite = (__ballot(c.sl <= P && !isfinite(gt[min(c.sl, P) * (P + 1) + P])) & slot_bits) == 0ull;
      return !col_finite || armijo_holds(0.5 * gt[P * (P + 1) + P], svp[S_COST], svp[S_GD0], svp[S_CUR_X]);
    };
    sweep<NB, W, false, kVT, kSP, Shape, kLone>(c, xt, nullptr, nullptr, need_rest);  // [J r]^T [J r] of this slot, left in LDS
    {
      int lane_t = lane;
      asm volatile("" : "+v"(lane_t));
      bind(lane_t);
    }
    GramView GH;
    GH.base = c.lds + c.L.gram;
    GH.ld = P + 1;
    unpark();
    const Horizon hz = get_horizon<NB, kVT, Shape>(c);
    // bounds of parameter q (src/optimizer.cpp:373-379: blocks 0..CH/bl-1 are bounded)
    const bool bounded = act && (q >> 1) < hz.nbounded;
    const double lo_q = bounded ? ((q & 1) ? SMPC_SCENE_PRM(c, kSP, prm, w_min) : SMPC_SCENE_PRM(c, kSP, prm, v_min)) : -1.7976931348623157e308;
    const double hi_q = bounded ? ((q & 1) ? SMPC_SCENE_PRM(c, kSP, prm, w_max) : SMPC_SCENE_PRM(c, kSP, prm, v_max)) : 1.7976931348623157e308;
    // usable iff every residual and Jacobian entry was finite: a non-finite one makes its diagonal Gram entry non-finite
    // (a sweep that stopped at the last column had every entry of that column finite, see need_rest)
    const bool gram_full = c.gram_full;
    const bool finite = !gram_full || !slot_any(c.sl <= P && !isfinite(GH.base[min(c.sl, P) * GH.ld + min(c.sl, P)]));
    const double val = 0.5 * GH(P, P);
    bool new_iteration = false;

    // ---------------------------------------------------------------- advance the slot's state machine
    auto adopt_trial_point = [&]() {  // x <- xt, Hs / gs / gu / gmax from G (scaled by the fixed Jacobi scaling)
      double xa = 0.0, gm = 0.0;
      if (act) {
        xa = xt[q];
        xc[q] = xa;
        const double scq = sc[q];
        const double* grow = GH.base + q * GH.ld;
#pragma unroll
        for (int b = 0; b < P; ++b) Hs[q * P + b] = grow[b] * scq * sc[b];  // the Gram is bitwise symmetric
        const double g = grow[P];
        gu[q] = g; gs[q] = g * scq;
        gm = fabs(xa - clampd(xa - g, lo_q, hi_q));
      }
      double xn, gmax;
      reduce_sum_max(xa * xa, gm, xn, gmax);
      sv[S_XNORM] = fast_sqrt(xn);
      sv[S_GMAX] = gmax;
    };
    auto candidate = [&]() {  // A.9 tests on the candidate = current trial point; A.10 strategy update
      const double cost = sv[S_COST];
      const double cand_cost = R.has(LF_CUR_VV) ? sv[S_CUR_V] : 1.7976931348623157e308;
      const double d = act ? xc[q] - xt[q] : 0.0;
      double sn2;
      reduce_sum(d * d, sn2);
      const double step_norm = fast_sqrt(sn2);
      const bool tol_allowed = !prm.fixed_iterations && (!prm.tol_needs_successful_step || R.has(LF_AT_LEAST_ONE));
      if (tol_allowed && step_norm <= prm.param_tol * (sv[S_XNORM] + prm.param_tol)) {
        if constexpr (kTrace) trace_row(R.iter, cost, cost - cand_cost, sv[S_GMAX], step_norm, 0.0, sv[S_RADIUS], R.n_samples, false);
        R.status = SMPC_CONVERGENCE; R.reason = SMPC_REASON_PARAMETER_TOL; R.phase = PH_DONE; return;
      }
      const double cost_change = cost - cand_cost;
      if (tol_allowed && fabs(cost_change) <= prm.fn_tol * cost) {
        if constexpr (kTrace) trace_row(R.iter, cost, cost_change, sv[S_GMAX], step_norm, 0.0, sv[S_RADIUS], R.n_samples, false);
        R.status = SMPC_CONVERGENCE; R.reason = SMPC_REASON_FUNCTION_TOL; R.phase = PH_DONE; return;
      }
      const double rho = (cand_cost >= 1.7976931348623157e308) ? -1.7976931348623157e308 : div_fast(cost_change, sv[S_MCC]);
      if (rho > 1e-3 && !gram_full) {
        // never seen: a candidate that failed the Armijo test cannot be accepted (cost - value < -1e-4 g.delta <
        // 1e-3 model_cost_change). Should rounding ever say otherwise, the point is swept again with its whole Gram.
        R.phase = PH_REEVAL;
        return;
      }
      if (rho > 1e-3) {
        adopt_trial_point();
        sv[S_COST] = cand_cost;
        R.flags |= LF_STEP_SUCCESSFUL | LF_AT_LEAST_ONE;
        const double t = 2.0 * rho - 1.0;
        sv[S_RADIUS] = fmin(1e16, div_fast(sv[S_RADIUS], fmax(1.0 / 3.0, 1.0 - t * t * t)));
        sv[S_DECF] = 2.0;
      } else {
        sv[S_RADIUS] = sv[S_RADIUS] * pow2_reciprocal(sv[S_DECF]);  // S_DECF is 2, 4, 8, ...: the quotient, exactly
        sv[S_DECF] *= 2.0;
      }
      if constexpr (kTrace) {  // cost, gmax and radius behind the update: of the adopted point where the step was accepted
        trace_row(R.iter, sv[S_COST], cost_change, sv[S_GMAX], step_norm, rho, sv[S_RADIUS], R.n_samples, R.has(LF_STEP_SUCCESSFUL));
      }
      new_iteration = true;
    };

    if (R.phase == PH_INIT) {
      ++R.evals;
      sv[S_COST] = val;
      sv[S_INITIAL_COST] = val;
      if (kVT && reinterpret_cast<const int*>(c.lds + c.L.hz)[6] != 0) {
        R.status = SMPC_FAILURE; R.reason = SMPC_REASON_SHORT_PATH; R.phase = PH_DONE;  // "Path has less than 2 points"
      } else if (!finite) {
        R.status = SMPC_FAILURE; R.reason = SMPC_REASON_EVAL_FAILED; R.phase = PH_DONE;
      } else {
        if (act) sc[q] = 1.0 / (1.0 + sqrt(GH.base[q * GH.ld + q]));  // Jacobi scaling (A.5)
        wave_lds_fence();
        adopt_trial_point();
        sv[S_RADIUS] = 1e4; sv[S_DECF] = 2.0;
        if constexpr (kTrace) trace_row(0, val, 0.0, sv[S_GMAX], 0.0, 0.0, 1e4, 0, true);
        new_iteration = true;
      }
    } else if (R.phase == PH_LS) {
      ++R.evals;
      // record the sample just evaluated (LineSearchFunction::Evaluate, A.8)
      const double dq = act ? dl[q] : 0.0;
      double gd;
      reduce_sum(act ? dq * GH.base[q * GH.ld + P] : 0.0, gd);
      const bool cur_vv = finite && isfinite(val), cur_gv = cur_vv && isfinite(gd);
      R.set(LF_CUR_VV, cur_vv); R.set(LF_CUR_GV, cur_gv);
      sv[S_CUR_V] = val; sv[S_CUR_G] = gd;
      const double alpha = sv[S_CUR_X];
      if (R.n_samples == 1) { sv[S_FIRST_V] = val; R.set(LF_FIRST_VV, cur_vv); }  // the full step: candidate if the search fails
      if (cur_vv && armijo_holds(val, sv[S_COST], sv[S_GD0], alpha)) {
        // Armijo satisfied: delta *= alpha; the candidate is this very point
        if (act) dl[q] = dq * alpha;
        candidate();
      } else {
        ++R.ls_iters;
        bool failed = R.ls_iters >= 20;
        double step_size = 0.0;
        if (!failed) {
          Sample lower{0.0, sv[S_COST], sv[S_GD0], true, true};
          Sample previous{sv[S_PREV_X], sv[S_PREV_V], sv[S_PREV_G], R.has(LF_PREV_VV), R.has(LF_PREV_GV)};
          Sample current{alpha, val, gd, cur_vv, cur_gv};
          SMPC_STAMP(c, 6);
          if (!interpolate_step_fast(lower, previous, current, 1e-3 * alpha, 0.6 * alpha, step_size))
          { SMPC_LS_COUNT(7, 1); step_size = interpolate_step(lower, previous, current, 1e-3 * alpha, 0.6 * alpha, scratch); }
          SMPC_STAMP(c, 7);  // line-search interpolation
          failed = step_size * sv[S_DIRMAX] < 1e-9;
        }
        if (!failed) {
          sv[S_PREV_X] = alpha; sv[S_PREV_V] = val; sv[S_PREV_G] = gd; R.set(LF_PREV_VV, cur_vv); R.set(LF_PREV_GV, cur_gv);
          sv[S_CUR_X] = step_size;
          if (act) xt[q] = clampd(xc[q] + step_size * dq, lo_q, hi_q);
          ++R.n_samples;
        } else if (R.n_samples > 1) {
          // Line search failed: delta unchanged, the candidate is the full step again (the first sample). Its cost is
          // known; its Gram is only needed if the step were accepted, which a step that failed the Armijo test at
          // alpha = 1 cannot be (cost - value_1 < -1e-4 g.delta < 1e-3 model_cost_change). Only in that never-seen case
          // the point is swept again (PH_REEVAL) so that the accepted state is built from its own Gram.
          if (act) xt[q] = clampd(xc[q] + dq, lo_q, hi_q);
          const double v1 = R.has(LF_FIRST_VV) ? sv[S_FIRST_V] : 1.7976931348623157e308;
          const bool would_accept = R.has(LF_FIRST_VV) && ((sv[S_COST] - v1) / sv[S_MCC] > 1e-3);
          if (would_accept) {
            R.phase = PH_REEVAL;
          } else {
            R.copy(LF_CUR_VV, LF_FIRST_VV);
            sv[S_CUR_V] = v1;
            wave_lds_fence();
            candidate();
          }
        } else {
          candidate();  // the only sample was the full step itself
        }
      }
    } else if (R.phase == PH_REEVAL) {
      ++R.evals;
      R.set(LF_CUR_VV, finite && isfinite(val));
      sv[S_CUR_V] = val;
      candidate();
    }

    // ---------------------------------------------------------------- start the next LM iteration (A.6, A.7)
    if (new_iteration) {
      for (;;) {
        if (R.iter >= prm.max_iterations) { R.status = SMPC_NO_CONVERGENCE; R.reason = SMPC_REASON_MAX_ITERATIONS; R.phase = PH_DONE; break; }
        if (R.has(LF_STEP_SUCCESSFUL) && sv[S_GMAX] <= prm.gradient_tol && !prm.fixed_iterations) { R.status = SMPC_CONVERGENCE; R.reason = SMPC_REASON_GRADIENT_TOL; R.phase = PH_DONE; break; }
        if (sv[S_RADIUS] <= 1e-32) { R.status = SMPC_CONVERGENCE; R.reason = SMPC_REASON_MIN_RADIUS; R.phase = PH_DONE; break; }
        ++R.iter;
        R.set(LF_STEP_SUCCESSFUL, false);
        // (the column masks "q == j" / "q > j" of this block stay inside it: hoisted out of this retry loop they were two
        // scalar registers each, 4 NB of them, spilled)
        int ql = q;
        asm volatile("" : "+v"(ql));
        const double radius = sv[S_RADIUS];
        const double inv_radius = div_fast(1.0, radius);  // radius stays within [1e-32, 1e16]: no scaling cases
        // row q of Hs + diag(D^2), D^2 = clamp(diag, 1e-6, 1e32) / radius: the LM strategy (A.6)
        double arow[P], Lr[P], invd[P];
#pragma unroll
        for (int j = 0; j < P; ++j) arow[j] = Hs[qc * P + j];
        const double gsq = act ? gs[q] : 0.0;
        const double d2 = clampd(Hs[qc * P + qc], 1e-6, 1e32) * inv_radius;
        // Cholesky, one row per lane, column by column: s = a_ij - sum_k<j L_ik L_jk; lane j's s is the pivot
        bool ok = true;
#pragma unroll
        for (int j = 0; j < P; ++j) {
          double s_ = arow[j] + ((j == ql) ? d2 : 0.0);
#pragma unroll
          for (int kk = 0; kk < j; ++kk) s_ = fma(-Lr[kk], Lw[j * P + kk], s_);
          if (ql == j) bc[j] = s_;
          wave_lds_fence();
          const double dpiv = bc[j];
          ok = ok && (dpiv > 0.0) && isfinite(dpiv);
          const double inv = rsqrt_pos(fmax(dpiv, 1e-300));  // 1 / l_jj (never used when the pivot is not positive)
          invd[j] = inv;
          Lr[j] = s_ * inv;
          if (act && ql > j) Lw[q * P + j] = Lr[j];
          wave_lds_fence();
        }
        // forward substitution L y = gs, backward L^T z = y; the step is -z
        double accf = gsq, yq = 0.0;
#pragma unroll
        for (int kk = 0; kk < P; ++kk) {
          const double yk_own = accf * invd[kk];
          if (ql == kk) { bc[P + kk] = yk_own; yq = yk_own; }
          wave_lds_fence();
          const double yk = bc[P + kk];
          accf = fma((ql > kk) ? -Lr[kk] : 0.0, yk, accf);
        }
        double accb = yq, zq = 0.0;
#pragma unroll
        for (int kk = P - 1; kk >= 0; --kk) {
          const double zk_own = accb * invd[kk];
          if (ql == kk) { bc[2 * P + kk] = zk_own; zq = zk_own; }
          wave_lds_fence();
          const double zk = bc[2 * P + kk];
          accb = fma((act && ql < kk) ? -Lw[kk * P + qc] : 0.0, zk, accb);
        }
        const double stepq = act ? -zq : 0.0;
        bool valid = ok && !slot_any(act && !isfinite(stepq));
        double mcc = 0.0;
        if (valid) {
          if (act) bc[3 * P + q] = stepq;
          wave_lds_fence();
          double rowv = 0.0;
#pragma unroll
          for (int b = 0; b < P; ++b) rowv = fma(arow[b], bc[3 * P + b], rowv);
          double sg, sHs;
          reduce_sum2(stepq * gsq, act ? stepq * rowv : 0.0, sg, sHs);
          mcc = -sg - 0.5 * sHs;
          valid = mcc > 0.0;
        }
        if (!valid) {
          if (++R.num_invalid >= 5) { R.status = SMPC_FAILURE; R.reason = SMPC_REASON_INVALID_STEPS; R.phase = PH_DONE; break; }
          sv[S_RADIUS] = radius * pow2_reciprocal(sv[S_DECF]); sv[S_DECF] *= 2.0;
          wave_lds_fence();
          if constexpr (kTrace) trace_row(R.iter, sv[S_COST], 0.0, sv[S_GMAX], 0.0, 0.0, sv[S_RADIUS], 0, false);
          continue;
        }
        R.num_invalid = 0;
        sv[S_MCC] = mcc;
        double dq = 0.0, gq = 0.0;
        if (act) {
          dq = stepq * sc[q];
          dl[q] = dq;
          gq = gu[q] * dq;
          xt[q] = clampd(xc[q] + 1.0 * dq, lo_q, hi_q);
        }
        double gd0, dirmax;
        reduce_sum_max(gq, fabs(dq), gd0, dirmax);
        sv[S_GD0] = gd0; sv[S_DIRMAX] = dirmax;
        sv[S_CUR_X] = 1.0;
        R.flags &= ~(LF_PREV_VV | LF_PREV_GV);
        R.ls_iters = 0; R.n_samples = 1;
        R.phase = PH_LS;
        break;
      }
    }

    // ---------------------------------------------------------------- finished: outputs, a12 unpack
    if (R.phase == PH_DONE) {
      wave_lds_fence();
      const size_t s = c.scene;
      if (c.sl == 0) {
        if (k.o_status) k.o_status[s] = R.status;
        if (k.o_reason) k.o_reason[s] = R.reason;
        if (k.o_iterations) k.o_iterations[s] = R.iter;
        if (k.o_evaluations) k.o_evaluations[s] = R.evals;
        if (k.o_initial_cost) k.o_initial_cost[s] = sv[S_INITIAL_COST];
        if (k.o_final_cost) k.o_final_cost[s] = sv[S_COST];
        if constexpr (kTrace) {  // rows the solve produced, stored or not: 0 .. iter, less the one an exit without a row leaves out
          const bool none = R.reason == SMPC_REASON_SHORT_PATH || R.reason == SMPC_REASON_EVAL_FAILED;
          if (k.o_trace_n) k.o_trace_n[s] = none ? 0 : R.iter + (R.reason == SMPC_REASON_INVALID_STEPS ? 0 : 1);
        }
      }
      if (k.o_params && c.sl < P) k.o_params[s * P + c.sl] = xc[c.sl];
      // saving_velocities[i], i = 0..T: block i/bl for i < CH, else the last block (src/optimizer.cpp:390-411); a scene
      // with a horizon of its own has Th + 1 entries, the rows behind them are written as zeros
      const int Th = hz.T;
      if (k.o_cmds) {
        for (int i = c.sl; i <= T; i += W) {
          const int b = block_of_step<NB>(i, hz);
          const bool in = i <= Th;
          k.o_cmds[(s * (T + 1) + i) * 2] = in ? xc[2 * b] : 0.0;
          k.o_cmds[(s * (T + 1) + i) * 2 + 1] = in ? xc[2 * b + 1] : 0.0;
        }
      }
      if (k.o_path) {
        // Re-roll (:420-446). The reference round-trips every heading through a quaternion (setRPY / getYaw), which
        // is the identity up to 1e-16 plus a wrap into (-pi, pi]; headings are produced here by the same sequential
        // adds followed by an exact wrap, then lane i integrates... positions need the sequential sums of
        // v cos(yaw_i) dt: lane i computes its own term, the running sum goes lane to lane in index order.
        const double* cst = c.lds + c.L.cst;
        double yaw = wrap_angle(cst[2]);
        double my_yaw_in = yaw, my_yaw_out = yaw;
        for (int i = 0; i <= T; ++i) {
          const int b = block_of_step<NB>(i, hz);
          // The run-time-shape kernels keep the plain expression, which the compiler contracts to one fused multiply-add in
          // their rolled loop (with one parameter block it hoists the product instead and adds). Unrolled over a literal T
          // it left the last step's product and sum apart, one ulp from the <3, 32> kernel the fixed-shape kernel stands in
          // for: there the fused operation is written out.
          double nyaw;
          if constexpr (Shape::kFixed) nyaw = wrap_angle(fma(k.dt, xc[2 * b + 1], yaw));
          else nyaw = wrap_angle(yaw + xc[2 * b + 1] * k.dt);
          if (i == c.sl) { my_yaw_in = yaw; my_yaw_out = nyaw; }
          yaw = nyaw;
        }
        const int bi = block_of_step<NB>(c.sl, hz);
        double sn, cs;
        sincos(my_yaw_in, &sn, &cs);
        const double v = (c.sl <= T) ? xc[2 * bi] : 0.0;
        const double tx = v * cs * k.dt, ty = v * sn * k.dt;
        double px = cst[0], py = cst[1], mx = 0.0, my = 0.0;
        for (int i = 0; i <= T; ++i) {
          px += __shfl(tx, slot * W + i, 64);
          py += __shfl(ty, slot * W + i, 64);
          if (i == c.sl) { mx = px; my = py; }
        }
        if (c.sl <= T) {
          const bool in = c.sl <= Th;
          double* o = k.o_path + (s * (T + 1) + c.sl) * 3;
          o[0] = in ? mx : 0.0; o[1] = in ? my : 0.0; o[2] = in ? my_yaw_out : 0.0;
        }
      }
      R.phase = PH_FETCH;
    }
  }
  if constexpr (kLone) {
    // (through the loop's copy of the argument pointer and with an address of its own: the prologue's pointer or the loop's
    // LDS pointers, live to here, were four scalar registers spilled in the line search)
    const auto& ke = *c.kp;
    const LdsLayout Lx = make_layout(Shape::T(ke), Shape::N(ke), P, kLayoutSolve, W, kSP);
    if ((ke.lone_trips & kLoneCount) != 0 && threadIdx.x == 0) {
      const unsigned long long n = *reinterpret_cast<const unsigned long long*>(lds_all + Lx.lm + P * P + 6 * P + S_COUNT + 4);
      atomicAdd(ke.queue + 1, (int)((n >> 21) & 0x1fffffull));
      atomicAdd(ke.queue + 2, (int)(n & 0x1fffffull));
      atomicAdd(ke.queue + 3, (int)(n >> 42));
    }
  }
#ifdef SMPC_STAMPS
  if (k.stamps && lane == 0) {
    for (int i = 0; i < 8; ++i) k.stamps[(size_t)blockIdx.x * 12 + i] = c.acc[i];
    for (int i = 0; i < 4; ++i) k.stamps[(size_t)blockIdx.x * 12 + 8 + i] = c.acc2[i];
  }
#endif
