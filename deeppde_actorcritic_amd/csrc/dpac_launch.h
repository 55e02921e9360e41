// dpac_launch.h — the launcher for one (T, equation functor, D): run_op turns an OpArgs into
// the kernel instantiation and the launch of its op (one launch_* function per op), and
// Registrar enters run_op into the dispatch table of dpac_abi.hip.
#pragma once
// Included by dpac_kernels.h inside namespace dpac, last (after every kernel header).

// The kernel-side view of a dpac_mlp (column offsets of each layer's saved z).
template <typename T>
NnMlp<T> nn_mlp(const dpac_mlp& h) {
  NnMlp<T> m{};
  m.L = h.n_hidden;
  m.ekn = h.ekn_head;
  int z = 0;
  for (int i = 0; i <= m.L + 1; ++i) {
    m.width[i] = h.width[i];
    m.scale[i] = (const T*)h.bn_scale[i];
    m.shift[i] = (const T*)h.bn_shift[i];
    m.zoff[i] = i == 0 ? 0 : z;
    if (i > 0) z += m.width[i];
  }
  m.ztot = z;
  for (int i = 0; i <= m.L; ++i) {
    m.weight[i] = (const T*)h.weight[i];
    m.wkm[i] = (const T*)h.weight_km[i];
  }
  m.bias = (const T*)h.bias;
  m.status = h.status;
  return m;
}

// Sum of the layer widths, input and output included (the BPTT's LDS plan).
template <typename T>
int width_sum(const NnMlp<T>& m) {
  int wsum = 0;
  for (int i = 0; i <= m.L + 1; ++i) wsum += m.width[i];
  return wsum;
}

// BPTT kernel: 2 = k_rollout_nn_bwd2 (stager + writer wavefronts, default), 1 = k_rollout_nn_bwd.
// DPAC_BPTT=1 / 2 forces one (tests compare the two).
inline int bptt_kernel() {
  const char* e = getenv("DPAC_BPTT");  // read per launch: tests switch it in-process
  return (e && e[0] == '1') ? 1 : 2;
}

// Analytic rollout with dw staged through LDS (k_rollout_staged, default) or read directly
// (k_rollout): DPAC_ROLLOUT_STAGED=0 forces the latter (tests compare the two bit for bit).
inline bool rollout_staged() {
  const char* e = getenv("DPAC_ROLLOUT_STAGED");  // read per launch
  return !(e && e[0] == '0');
}

// Row tile of the fused NN rollout for float: 4 (4x4x1 MFMA blocks) or 16
// (16x16x4 tiles; float64 always uses these); by default 4 for B <= 1024.
// DPAC_NN_TILE=4 / 16 forces one (tests compare the two).
inline int nn_tile_rows() {
  const char* e = getenv("DPAC_NN_TILE");  // read per launch: tests switch it in-process
  const int v = e ? atoi(e) : 0;
  return (v == 4 || v == 16) ? v : 0;     // 0: by batch size
}

// Trajectories per workgroup of the split-fp16 NN kernels (k_rollout_nn_x3, k_rollout_nn_bwd_x3):
// 16 (one MFMA row tile) or 8 (half a tile, twice the workgroups).  DPAC_NX_ROWS=8 / 16 forces one.
inline int nx_rows(int64_t B) {
  const char* e = getenv("DPAC_NX_ROWS");  // read per launch: tests switch it in-process
  const int v = e ? atoi(e) : 0;
  if (v == 8 || v == 16) return v;
  (void)B;
  return 16;
}

inline dim3 grid_for(int64_t B, int P) {
  const int64_t per = 64 / P;
  return dim3((unsigned)((B + per - 1) / per));
}

// Runtime value -> compile-time constant: f is a generic lambda and receives the value as an
// integral_constant.  Each helper names every value of its one argument; a launch function
// whose kernel exists only for some combinations of several says which, with a plain if.
template <class F>
void with_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}
template <class F>
void with_scheme(int scheme, F&& f) {
  if (scheme == DPAC_SCHEME_ADAPTIVE) f(std::integral_constant<int, DPAC_SCHEME_ADAPTIVE>{});
  else f(std::integral_constant<int, DPAC_SCHEME_NAIVE>{});
}
template <class F>
void with_out(int out, F&& f) {  // the rollout's optional outputs
  switch (out) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case kOutCost: f(std::integral_constant<int, kOutCost>{}); break;
    case kOutU: f(std::integral_constant<int, kOutU>{}); break;
    default: f(std::integral_constant<int, kOutCost | kOutU>{}); break;
  }
}

template <class F>
void with_lean(int mode, F&& f) {  // the lean modes of the NN forward kernels (NnMode)
  if (mode == kNnLeanPhilox) f(std::integral_constant<int, kNnLeanPhilox>{});
  else f(std::integral_constant<int, kNnLeanDw>{});
}

// A launch with more dynamic LDS than the default limit.  Returns the attribute call's error
// and does not launch after one.
template <class K, class... A>
hipError_t launch_dyn_lds(K kfn, dim3 grid, dim3 block, uint32_t lds, hipStream_t s, const A&... args) {
  if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
    return e;
  hipLaunchKernelGGL(kfn, grid, block, lds, s, args...);
  return hipSuccess;
}

template <typename T>
constexpr bool kNnFastOk = std::is_same<T, float>::value;  // the NN fast path is float-only

// k_rollout_staged with the loader wavefront (GEN = 0) or with GEN generator wavefronts.
template <typename T, class E, int D, int GEN>
void launch_rollout_staged(const E& eq, const DevConsts<T>& c, const RolloutArgs<T>& r, int scheme, int out,
                           hipStream_t s) {
  constexpr int TPW = StagedPlan<T, D, E::kP>::TPW;
  const dim3 grid((unsigned)((r.B + TPW - 1) / TPW)), block(64 * st_waves<GEN>());
  with_scheme(scheme, [&](auto sch) {
    with_out(out, [&](auto o) {
      hipLaunchKernelGGL((k_rollout_staged<T, E, D, decltype(sch)::value, decltype(o)::value, GEN>), grid, block,
                         0, s, eq, c, r);
    });
  });
}

template <typename T, class E, int D>
int launch_rollout(const OpArgs& a, const E& eq, const DevConsts<T>& c, hipStream_t s) {
  RolloutArgs<T> r;
  r.B = a.B; r.traj_offset = a.traj_offset; r.N = a.N; r.sample_type = a.sample_type;
  r.cost_order = a.cost_order; r.seed = a.seed;
  r.x0 = (const T*)a.x0; r.dw = (const T*)a.dw;
  r.x = (T*)a.x_out; r.dt = (T*)a.dt; r.coef = (T*)a.coef; r.u = (T*)a.u_out;
  r.y = (T*)a.y; r.disc = (T*)a.disc;
  const bool philox = a.dw == nullptr, cost = a.y != nullptr;
  const int out = (cost ? kOutCost : 0) | (a.u_out ? kOutU : 0);
  using SP = StagedPlan<T, D, E::kP>;
  // the Philox variant on the ring (generator wavefronts): float, the paired stream layout
  constexpr bool kGenOk = SP::kOk && std::is_same<T, float>::value && 2 * E::M <= 4;
  if constexpr (kGenOk) {
    if (philox && rollout_staged() && dw_steps_per_block<T>(E::M, a.sample_type) == 2) {
      launch_rollout_staged<T, E, D, kStGen>(eq, c, r, a.scheme, out, s);
      return 0;
    }
  }
  if constexpr (SP::kOk) {
    if (!philox && rollout_staged()) {  // dw through the loader wave's LDS ring
      launch_rollout_staged<T, E, D, 0>(eq, c, r, a.scheme, out, s);
      return 0;
    }
  }
  constexpr int KB = rollout_kb(ring_kb((int)sizeof(DwFrame<T, E::M>), DPAC_RING_VGPRS, DPAC_ROLLOUT_KB_CAP), E::kP);
  const dim3 grid = grid_for(a.B, E::kP), block(64);
  with_scheme(a.scheme, [&](auto sch) {
    with_bool(philox, [&](auto ph) {
      with_out(out, [&](auto o) {
        hipLaunchKernelGGL((k_rollout<T, E, D, decltype(sch)::value, decltype(ph)::value, decltype(o)::value, KB>),
                           grid, block, 0, s, eq, c, r);
      });
    });
  });
  return 0;
}

template <typename T, class E, int D>
int launch_flag_init(const OpArgs& a, const E& eq, const DevConsts<T>& c, hipStream_t s) {
  with_scheme(a.scheme, [&](auto sch) {
    hipLaunchKernelGGL((k_flag_init<T, E, D, decltype(sch)::value>), grid_for(a.B, E::kP), dim3(64), 0, s, eq, c,
                       a.B, (const T*)a.x0, a.flag_out);
  });
  return 0;
}

template <typename T, class E, int D>
int launch_step(const OpArgs& a, const E& eq, const DevConsts<T>& c, hipStream_t s) {
  StepArgs<T> st;
  st.B = a.B; st.cost_order = a.cost_order;
  st.x = (const T*)a.x; st.u = (const T*)a.u; st.dw = (const T*)a.dw;
  st.disc_in = (const T*)a.disc_in; st.y_in = (const T*)a.y_in; st.flag_in = a.flag_in;
  st.x_out = (T*)a.x_out; st.disc_out = (T*)a.disc_out; st.y_out = (T*)a.y_out;
  st.dt = (T*)a.dt; st.coef = (T*)a.coef; st.flag_out = a.flag_out;
  st.g_x_out = (const T*)a.g_x_out; st.g_disc_out = (const T*)a.g_disc_out;
  st.g_y_out = (const T*)a.g_y_out;
  st.g_x = (T*)a.g_x; st.g_u = (T*)a.g_u; st.g_disc = (T*)a.g_disc;
  const dim3 grid = grid_for(a.B, E::kP), block(64);
  with_scheme(a.scheme, [&](auto sch) {
    constexpr int SCH = decltype(sch)::value;
    if (a.op == OP_STEP_FWD) hipLaunchKernelGGL((k_step_fwd<T, E, D, SCH>), grid, block, 0, s, eq, c, st);
    else hipLaunchKernelGGL((k_step_bwd<T, E, D, SCH>), grid, block, 0, s, eq, c, st);
  });
  return 0;
}

template <typename T, class E, int D>
int launch_td(const OpArgs& a, const E& eq, const DevConsts<T>& c, hipStream_t s) {
  TdArgs<T> td;
  td.B = a.B; td.traj_offset = a.traj_offset; td.N = a.N; td.sample_type = a.sample_type;
  td.cost_order = a.cost_order; td.seed = a.seed;
  td.x = (const T*)a.x; td.u = (const T*)a.u; td.dw = (const T*)a.dw;
  td.dt = (const T*)a.dt_in; td.coef = (const T*)a.coef_in; td.G = (const T*)a.G;
  td.g_y = (const T*)a.g_y_out;
  td.y = (T*)a.y; td.disc = (T*)a.disc; td.g_G = (T*)a.g_G;
  td.gd = (const T*)a.G; td.g_gd = (T*)a.g_G;
  const bool philox = a.dw == nullptr, bwd = a.op == OP_TD_BWD;
  const dim3 grid = grid_for(a.B, E::kP), block(64 * kTdChunks);
  // k_td<TD1, PHILOX, BWD, GDOT>: GDOT draws nothing; TD0 has neither increments nor a backward
  if (a.td_type == DPAC_TD1_GDOT) {
    with_bool(bwd, [&](auto bw) {
      hipLaunchKernelGGL((k_td<T, E, D, true, false, decltype(bw)::value, true>), grid, block, 0, s, eq, c, td);
    });
  } else if (bwd || a.td_type == DPAC_TD1) {
    with_bool(philox, [&](auto ph) {
      with_bool(bwd, [&](auto bw) {
        hipLaunchKernelGGL((k_td<T, E, D, true, decltype(ph)::value, decltype(bw)::value>), grid, block, 0, s, eq,
                           c, td);
      });
    });
  } else {
    hipLaunchKernelGGL((k_td<T, E, D, false, false, false>), grid, block, 0, s, eq, c, td);
  }
  return 0;
}

template <typename T, class E, int D>
int launch_eval(const OpArgs& a, const E& eq, const DevConsts<T>& c, hipStream_t s) {
  hipLaunchKernelGGL((k_eval<T, E, D>), grid_for(a.B, E::kP), dim3(64), 0, s, eq, c, a.B, a.what,
                     (const T*)a.x, (const T*)a.u, (T*)a.out);
  return 0;
}

// k_rollout_nn_bwd2 reading the forward's sign-bit mask instead of z (the fast path: float only,
// so only float code may name this function).
template <typename T, class E, int D>
hipError_t launch_bwd2_mask(const E& eq, const DevConsts<T>& c, const NnMlp<T>& m, const NnBackArgs<T>& r,
                            int scheme, uint32_t lds, hipStream_t s) {
  const dim3 grid((unsigned)((r.B + kNnRows - 1) / kNnRows)), block(kNnBwdThreads);
  hipError_t e = hipSuccess;
  with_scheme(scheme, [&](auto sch) {
    e = launch_dyn_lds(k_rollout_nn_bwd2<T, E, D, decltype(sch)::value, false, true, true>, grid, block, lds, s,
                       eq, c, m, r);
  });
  return e;
}

template <typename T, class E, int D>
int launch_rollout_nn_bwd(const OpArgs& a, const E& eq, const DevConsts<T>& c, hipStream_t s) {
  using Plan = BwdPlan<T, D, E::CDIM>;
  NnMlp<T> m = nn_mlp<T>(a.mlp);
  NnBackArgs<T> r{};
  r.B = a.B; r.N = a.N;
  r.x = (const T*)a.x; r.u = (const T*)a.u; r.dw = (const T*)a.dw;
  r.disc_t = (const T*)a.save_disc; r.z = (const T*)a.save_z; r.flag = a.save_flag;
  r.g_xN = (const T*)a.g_x_out; r.g_disc = (const T*)a.g_disc_out; r.g_y = (const T*)a.g_y_out;
  r.G = (T*)a.g_G; r.g_x0 = (T*)a.g_x;
  int go = 0;
  for (int i = 0; i <= m.L + 1; ++i) {
    r.goff[i] = go;
    go += m.width[i];
  }
  r.gtot = go;
  for (int i = 0; i <= m.L; ++i) {
    r.wt[i] = (const T*)a.mlp_wt[i];
    r.wtkm[i] = (const T*)a.mlp.weight_km[i];  // k-major images of wt (dpac.h)
  }
  // the fast path serves k_rollout_nn_bwd2 (the generic k_rollout_nn_bwd ignores it)
  r.fast = nn_fast_host<T>(m.L, m.width, (const void* const*)r.wtkm, m.width[m.L + 1], m.width[0]);
  r.mask = r.fast ? a.mask_in : nullptr;
  r.mb = nn_mask_tile_bytes(m.L);
  const dim3 ngrid((unsigned)((a.B + kNnRows - 1) / kNnRows)), nblock(kNnThreads);
  const int gphase = m.status ? a.mlp.guard_phase : DPAC_GUARD_INLINE;  // dpac.h guard_phase
  hipError_t err = hipSuccess;
  if constexpr (kNnFastOk<T>) {  // split-fp16 chain (dpac_rollout_nn_x3.h): needs the forward's mask
    // (guarded by a status word: only with the f32 fast path's operands for the fallback)
    if (r.mask && bptt_kernel() == 2 && (!m.status || r.fast) &&
        nn_x3_host(m.L, m.width, (const void* const*)a.mlp.weight_t_x3, m.width[m.L + 1], m.width[0])) {
      for (int i = 0; i <= m.L; ++i) r.wtx3[i] = (const _Float16*)a.mlp.weight_t_x3[i];
      r.tr = nx_rows(a.B);
      if (gphase != DPAC_GUARD_FALLBACK_ONLY) {
        with_scheme(a.scheme, [&](auto sch) {
          err = launch_dyn_lds(k_rollout_nn_bwd_x3<E, D, decltype(sch)::value>,
                               dim3((unsigned)((a.B + r.tr - 1) / r.tr)), nblock, NxLds::total, s, eq, c, m, r);
        });
        if (err) return (int)err;
      }
      if (m.status && gphase != DPAC_GUARD_SPLIT_ONLY) {
        // the f32 BPTT, run only once the x3 kernel fell back (dpac.h dpac_mlp.status)
        const Plan pl(width_sum(m), m.ztot, true, r.mb);
        NnBackArgs<T> f = r;
        f.guard = m.status;
        err = launch_bwd2_mask<T, E, D>(eq, c, m, f, a.scheme, pl.total, s);
      }
      return (int)err;
    }
  }
  if (gphase == DPAC_GUARD_FALLBACK_ONLY) return 0;  // phase 1 did the whole work
  if (bptt_kernel() == 2) {
    const Plan pl(width_sum(m), m.ztot, true, r.mask ? r.mb : 0);
    const uint32_t lds = pl.total;
    if constexpr (kNnFastOk<T>) {
      if (r.mask) return (int)launch_bwd2_mask<T, E, D>(eq, c, m, r, a.scheme, lds, s);
    }
    with_scheme(a.scheme, [&](auto sch) {
      with_bool(pl.zst, [&](auto zs) {
        constexpr int SCH = decltype(sch)::value;
        constexpr bool ZS = decltype(zs)::value;
        auto kfn = r.fast ? k_rollout_nn_bwd2<T, E, D, SCH, ZS, kNnFastOk<T>>
                          : k_rollout_nn_bwd2<T, E, D, SCH, ZS, false>;
        err = launch_dyn_lds(kfn, ngrid, dim3(kNnBwdThreads), lds, s, eq, c, m, r);
      });
    });
    return (int)err;
  }
  with_scheme(a.scheme, [&](auto sch) {
    hipLaunchKernelGGL((k_rollout_nn_bwd<T, E, D, decltype(sch)::value>), ngrid, nblock, 0, s, eq, c, m, r);
  });
  return 0;
}

template <typename T, class E, int D>
int launch_rollout_nn(const OpArgs& a, const E& eq, const DevConsts<T>& c, hipStream_t s) {
  NnMlp<T> m = nn_mlp<T>(a.mlp);
  m.fast = nn_fast_host<T>(m.L, m.width, (const void* const*)m.wkm, m.width[0], m.width[m.L + 1]);
  NnRolloutArgs<T> r{};
  r.B = a.B; r.N = a.N; r.cost_order = a.cost_order;
  r.x0 = (const T*)a.x0; r.dw = (const T*)a.dw;
  r.x = (T*)a.x_out; r.dt = (T*)a.dt; r.coef = (T*)a.coef; r.u = (T*)a.u_out;
  r.y = (T*)a.y; r.disc = (T*)a.disc;
  r.save_z = (T*)a.save_z; r.save_disc = (T*)a.save_disc; r.save_flag = a.save_flag;
  r.save_mask = nullptr;
  r.mb = nn_mask_tile_bytes(m.L);
  // dpac_policy_cost: the lean instantiations of the kernel chosen below (always with the cost,
  // never with saves or a mask), dw read (kNnLeanDw) or drawn in-kernel (kNnLeanPhilox)
  const int mode = a.x_end ? (a.dw ? kNnLeanDw : kNnLeanPhilox) : kNnFull;
  r.x_end = (T*)a.x_end; r.tau = (T*)a.tau; r.steps = a.steps;
  r.seed = a.seed; r.traj_offset = a.traj_offset; r.sample_type = a.sample_type;
  const bool cost = a.y != nullptr;
  const int gphase = m.status ? a.mlp.guard_phase : DPAC_GUARD_INLINE;  // dpac.h guard_phase
  if constexpr (std::is_same<T, float>::value) {
    // 4-row MFMA blocks (dpac_rollout_nn4.h) where the 16-row tiles would leave
    // most CUs idle: 4x4x1 costs 4x the cycles per flop of 16x16x4, and measured
    // 11.4 vs 15.4 us per step at B <= 1024, 15.8 vs 15.4 at 2048, 31 vs 15.4 at 4096
    const int tile = nn_tile_rows();
    if (tile == 4 || (tile == 0 && a.B <= 1024)) {
      if (gphase == DPAC_GUARD_FALLBACK_ONLY) return 0;  // no split-fp16 launch here: nothing to redo
      const int rg = a.B <= 1024 ? 1 : 2;
      const dim3 g4((unsigned)((a.B + 4 * rg - 1) / (4 * rg))), b4(kN4Threads);
      with_scheme(a.scheme, [&](auto sch) {
        with_bool(rg == 2, [&](auto two) {
          constexpr int RG = decltype(two)::value ? 2 : 1;
          if (mode != kNnFull) {
            with_lean(mode, [&](auto md) {
              hipLaunchKernelGGL((k_rollout_nn4<T, E, D, decltype(sch)::value, true, RG, decltype(md)::value>), g4,
                                 b4, 0, s, eq, c, m, r);
            });
            return;
          }
          with_bool(cost, [&](auto co) {
            hipLaunchKernelGGL((k_rollout_nn4<T, E, D, decltype(sch)::value, decltype(co)::value, RG>), g4, b4, 0,
                               s, eq, c, m, r);
          });
        });
      });
      return 0;
    }
  }
  const dim3 ngrid((unsigned)((a.B + kNnRows - 1) / kNnRows)), nblock(kNnThreads);
  bool x3 = false;
  if constexpr (kNnFastOk<T>)  // guarded by a status word: only with the f32 fast path's operands for the fallback
    x3 = (!m.status || m.fast) &&
         nn_x3_host(m.L, m.width, (const void* const*)a.mlp.weight_x3, m.width[0], m.width[m.L + 1]);
  if ((m.fast || x3) && a.save_mask && a.save_z) {  // the 16-row fast paths write the sign bits
    r.save_mask = a.save_mask;
    if (a.mask_written) *a.mask_written = 1;
  }
  if constexpr (kNnFastOk<T>) {  // split-fp16 MLP (dpac_rollout_nn_x3.h)
    if (x3) {
      for (int i = 0; i <= m.L; ++i) m.wx3[i] = (const _Float16*)a.mlp.weight_x3[i];
      const bool save = r.save_z != nullptr, mask = r.save_mask != nullptr;
      r.tr = nx_rows(a.B);
      const dim3 xgrid((unsigned)((a.B + r.tr - 1) / r.tr));
      if (gphase != DPAC_GUARD_FALLBACK_ONLY) {
        hipError_t e = hipSuccess;
        with_scheme(a.scheme, [&](auto sch) {
          if (mode != kNnFull) {
            with_lean(mode, [&](auto md) {
              e = launch_dyn_lds(k_rollout_nn_x3<E, D, decltype(sch)::value, true, false, false, decltype(md)::value>,
                                 xgrid, nblock, NxLds::total, s, eq, c, m, r);
            });
            return;
          }
          with_bool(cost, [&](auto co) {
            auto go = [&](auto sv, auto mk) {
              e = launch_dyn_lds(k_rollout_nn_x3<E, D, decltype(sch)::value, decltype(co)::value,
                                                 decltype(sv)::value, decltype(mk)::value>,
                                 xgrid, nblock, NxLds::total, s, eq, c, m, r);
            };
            if (mask) go(std::true_type{}, std::true_type{});  // the mask comes only with the saves
            else if (save) go(std::true_type{}, std::false_type{});
            else go(std::false_type{}, std::false_type{});
          });
        });
        if (e != hipSuccess) return (int)e;
      }
      if (!m.status || gphase == DPAC_GUARD_SPLIT_ONLY) return 0;
      r.guard = m.status;  // then the f32 kernel below, run only once the x3 kernel fell back
    }
  }
  if (gphase == DPAC_GUARD_FALLBACK_ONLY && !r.guard) return 0;  // phase 1 did the whole work
  with_scheme(a.scheme, [&](auto sch) {
    if (mode != kNnFull) {
      with_lean(mode, [&](auto md) {
        constexpr int SCH = decltype(sch)::value, MD = decltype(md)::value;
        if (m.fast)
          hipLaunchKernelGGL((k_rollout_nn<T, E, D, SCH, true, 1, kNnFastOk<T>, false, MD>), ngrid, nblock, 0, s, eq,
                             c, m, r);
        else
          hipLaunchKernelGGL((k_rollout_nn<T, E, D, SCH, true, 1, false, false, MD>), ngrid, nblock, 0, s, eq, c, m,
                             r);
      });
      return;
    }
    with_bool(cost, [&](auto co) {
      constexpr int SCH = decltype(sch)::value;
      constexpr bool CO = decltype(co)::value, FAST = kNnFastOk<T>;
      if (m.fast && r.save_mask)
        hipLaunchKernelGGL((k_rollout_nn<T, E, D, SCH, CO, 1, FAST, FAST>), ngrid, nblock, 0, s, eq, c, m, r);
      else if (m.fast)
        hipLaunchKernelGGL((k_rollout_nn<T, E, D, SCH, CO, 1, FAST>), ngrid, nblock, 0, s, eq, c, m, r);
      else
        hipLaunchKernelGGL((k_rollout_nn<T, E, D, SCH, CO, 1, false>), ngrid, nblock, 0, s, eq, c, m, r);
    });
  });
  return 0;
}

template <typename T, class E, int D>
int run_op(const OpArgs& a) {
  const E eq = E::make(a.eq);
  const DevConsts<T> c = DevConsts<T>::make(host_consts(a));
  hipStream_t s = a.stream;
  int err;
  switch (a.op) {
    case OP_ROLLOUT: err = launch_rollout<T, E, D>(a, eq, c, s); break;
    case OP_FLAG_INIT: err = launch_flag_init<T, E, D>(a, eq, c, s); break;
    case OP_STEP_FWD:
    case OP_STEP_BWD: err = launch_step<T, E, D>(a, eq, c, s); break;
    case OP_TD_FWD:
    case OP_TD_BWD: err = launch_td<T, E, D>(a, eq, c, s); break;
    case OP_EVAL: err = launch_eval<T, E, D>(a, eq, c, s); break;
    case OP_ROLLOUT_NN: err = launch_rollout_nn<T, E, D>(a, eq, c, s); break;
    case OP_ROLLOUT_NN_BWD: err = launch_rollout_nn_bwd<T, E, D>(a, eq, c, s); break;
    default: return DPAC_EINVAL;
  }
  return err ? err : (int)hipGetLastError();
}

// Kernel instantiations register themselves per (equation family, dim, dtype): each
// equation TU is compiled once per dtype and state dimension (Makefile), so the heavy
// template instantiations build in parallel, and dpac_abi.hip finds them in a table.
// EQ<T, D> is the functor with its lane split already chosen.
using DispatchFn = int (*)(const OpArgs&);
void register_dispatch(int eqn, int dim, int f64, DispatchFn fn);
DispatchFn find_dispatch(int eqn, int dim, int f64);
constexpr int kMaxRegDim = 64;  // the dispatch table's dimension range (dpac_abi.hip)

template <template <typename, int> class EQ, typename T, int... Ds>
struct Registrar {
  static_assert(((Ds >= 1 && Ds <= kMaxRegDim) && ...),
                "DPAC_DIMS holds a dimension outside the dispatch table (1..kMaxRegDim)");
  explicit Registrar(int eqn) {
    (register_dispatch(eqn, Ds, std::is_same<T, double>::value ? 1 : 0, &run_op<T, EQ<T, Ds>, Ds>), ...);
  }
};
