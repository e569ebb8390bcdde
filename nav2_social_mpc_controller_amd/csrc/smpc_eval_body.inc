// smpc_eval_body.inc — the body of the K1 kernels, included by smpc_eval_kernel.hpp inside each of them:
// smpc_eval_kernel<NB, W, kVT, kSP> (Shape = RuntimeShape) and smpc_eval_fixed_kernel<Shape>. The including kernel provides
// NB, W, kVT, kSP and Shape. Text, not a device function: see the note in smpc_solve_kernel.hpp.
  static_assert(!kSP || kVT, "a kernel with per-scene weights and bounds reads its horizon per scene as well");
  const auto& k = *(KParamsK)__builtin_amdgcn_kernarg_segment_ptr();
  constexpr int P = 2 * NB;
  constexpr int S = kWave / W;
  extern __shared__ __attribute__((aligned(32))) double lds_all[];
  const int lane = threadIdx.x & 63;
  const int slot = lane / W;
  Ctx c;
  c.kp = &k;
  c.sl = lane - slot * W;
  c.L = make_layout(Shape::T(k), Shape::N(k), P, kLayoutEval, W, kSP);
  c.lds = lds_all + (size_t)slot * c.L.total;
  c.wave_lds = lds_all + (size_t)S * c.L.total;
  c.slot = slot;
  c.ag = k.people_rec;
  {
    double* atab = lds_all + atan_tab_offset(S * c.L.total, eval_extra_doubles(Shape::T(k), P, W));
    load_atan_nodes(c.kp, atab, lane);
    c.atab = atab;
  }
#ifdef SMPC_STAMPS
  for (int i = 0; i < 8; ++i) c.acc[i] = 0;
  for (int i = 0; i < 4; ++i) c.acc2[i] = 0;
  c.t_last = __builtin_amdgcn_s_memtime();
#endif
  const int scene_raw = blockIdx.x * S + slot;
  const bool live = scene_raw < k.B;
  const int scene = live ? scene_raw : k.B - 1;
  load_scene<W, kVT, kSP, Shape>(c, scene);
  wave_lds_fence();
  SMPC_STAMP(c, 0);
  const size_t s = scene;
  double* out_r = (live && k.e_residuals) ? k.e_residuals + s * k.e_M : nullptr;
  double* out_J = (live && k.e_jacobian) ? k.e_jacobian + s * (size_t)k.e_M * P : nullptr;
  const Horizon hz = get_horizon<NB, kVT, Shape>(c);
  if (!c.has_people || kVT) {
    // rows the scene does not have stay zero: the people rows of a scene without people, and — reference row order —
    // everything behind the 8 (or 5) Th + n_feasibility rows of a scene with a horizon of its own (in the critic-major
    // order the sweep itself writes the zero rows of every critic block it visits)
    const int Mb = (c.has_people ? 8 : 5) * (k.e_row_order == 1 ? Shape::T(k) : hz.T) + (k.e_row_order == 1 ? Shape::nfeas(k) : hz.nfeas);
    for (int i = Mb + c.sl; i < k.e_M; i += W) {
      if (out_r) out_r[i] = 0.0;
      if (out_J) for (int q = 0; q < P; ++q) out_J[(size_t)i * P + q] = 0.0;
    }
    if (kVT && k.e_row_order == 1) {  // critic-major: the feasibility rows the scene does not have
      const int base = (c.has_people ? 8 : 5) * Shape::T(k);
      for (int i = hz.nfeas + c.sl; i < Shape::nfeas(k); i += W) {
        if (out_r) out_r[base + i] = 0.0;
        if (out_J) for (int q = 0; q < P; ++q) out_J[(size_t)(base + i) * P + q] = 0.0;
      }
    }
  }
  const GramView G = sweep<NB, W, true, kVT, kSP, Shape>(c, k.e_x + s * P, out_r, out_J);
  if (live && c.sl == 0 && k.e_cost) k.e_cost[s] = 0.5 * G(P, P);
  if (live && k.e_gradient && c.sl < P) k.e_gradient[s * P + c.sl] = G(c.sl, P);
#ifdef SMPC_STAMPS
  SMPC_STAMP(c, 6);
  if (k.stamps && lane == 0) {
    for (int i = 0; i < 8; ++i) k.stamps[(size_t)blockIdx.x * 12 + i] = c.acc[i];
    for (int i = 0; i < 4; ++i) k.stamps[(size_t)blockIdx.x * 12 + 8 + i] = c.acc2[i];
  }
#endif
