// dpac_kernels.h — the equation kernels of libdpac; what every equation TU includes.
//
// Three files, read in this order:
//  * dpac_kernels.h (this one): Op, OpArgs and the constants; the device pieces every kernel
//    shares (pipelined(), LaneCoord, Flags, Transition, ...); the analytic kernels k_rollout,
//    k_flag_init, k_step_fwd / k_step_bwd, k_td and k_eval;
//  * dpac_rollout_staged.h, included after k_rollout: k_rollout_staged, the rollout with dw
//    staged through an LDS ring, with its ring plan, producers, clock trace and DPAC_ST_* knobs;
//  * dpac_launch.h, included last, after the NN rollout headers (dpac_rollout_nn*.h): run_op,
//    which launches every kernel above and theirs, one launch_* function per op, the getenv
//    switches it reads, and the Registrar that enters it into dpac_abi.hip's dispatch table.
//
// Mapping: a trajectory is owned by P = E::kP consecutive lanes of a 64-wide
// wavefront, each lane holding M = d/P state components in registers.
//  * k_rollout: one wavefront per workgroup, the whole time loop in-kernel, so a
//    trajectory's state never leaves registers between steps; HBM traffic is
//    exactly what the reference materialises (x_smp, dt, coef: equation.py:63-70,
//    97-104).  Per-step increments are prefetched 2*KB steps ahead (pipelined()).
//  * k_td: the TD sums have no state dependence, only the discount product is
//    sequential; 4 wavefronts per workgroup split the horizon into 4 chunks and
//    combine (local sum, local discount) pairs in LDS.
//  * k_step_fwd / k_step_bwd / k_flag_init / k_eval: one row per lane group.
// Floating-point contraction is off (-ffp-contract=off); the fused multiply-adds
// are written out, so every kernel variant rounds identically.
#pragma once

#include <cmath>
#include <limits>
#include <type_traits>
#include <utility>

#include "dpac_device.h"

namespace dpac {

enum Op : int {
  OP_ROLLOUT = 0,
  OP_FLAG_INIT,
  OP_STEP_FWD,
  OP_STEP_BWD,
  OP_TD_FWD,
  OP_TD_BWD,
  OP_EVAL,
  OP_ROLLOUT_NN,
  OP_ROLLOUT_NN_BWD,
};

// Bytes per 16-row tile of the sign-bit mask (FwdEpiM): 13 16-column tiles per hidden layer
// (the fast path's 193..208-wide layers), 64 bytes each.
inline int nn_mask_tile_bytes(int n_hidden) { return 13 * 64 * n_hidden; }

// Everything any op may need; unused fields are ignored.
struct OpArgs {
  int op;
  dpac_eqn_params eq;
  int scheme, dtype, td_type, cost_order, sample_type, what;
  int64_t B, traj_offset;
  int N;
  double T;
  uint64_t seed;
  const void *x0, *dw, *x, *u, *dt_in, *coef_in, *G, *disc_in, *y_in;
  const int32_t* flag_in;
  const void *g_x_out, *g_disc_out, *g_y_out;
  void *x_out, *dt, *coef, *u_out, *y, *disc, *disc_out, *y_out;
  int32_t* flag_out;
  void *g_x, *g_u, *g_disc, *g_G, *out;
  dpac_mlp mlp;                  // OP_ROLLOUT_NN: the actor MLP
  void *save_z, *save_disc;      // OP_ROLLOUT_NN: optional backward saves
  int32_t* save_flag;
  uint8_t* save_mask;            // OP_ROLLOUT_NN: optional sign-bit mask (fast path only)
  int32_t* mask_written;         // OP_ROLLOUT_NN: host flag, 1 if the mask was written
  const uint8_t* mask_in;        // OP_ROLLOUT_NN_BWD: the forward's mask, or null
  void *x_end, *tau;             // OP_ROLLOUT_NN: x_end selects the lean modes (dpac_policy_cost;
  int32_t* steps;                //   dw null: in-kernel noise from seed / traj_offset / sample_type)
  const void* mlp_wt[DPAC_MLP_MAX_HIDDEN + 1];  // OP_ROLLOUT_NN_BWD: (W_i diag s_{i+1})^T
  hipStream_t stream;
};

inline HostConsts host_consts(const OpArgs& a) {
  HostConsts h;
  const double d = a.eq.dim;
  h.gamma = a.eq.gamma;
  h.R = a.eq.R;
  h.sigma_up = a.eq.sigma_up;
  h.dt0 = a.T / a.N;                                       // delta_t = T / N (:48, :75)
  h.sqrt_dt0 = std::sqrt(h.dt0);                           // np.sqrt(delta_t) (:49)
  h.dt_min = h.dt0 * 1e-4;                                 // delta_t*1e-4 (:86)
  h.den = 3 * a.eq.dim * (a.eq.sigma_up * a.eq.sigma_up);  // 3*dim*sigma_Up**2 (:85)
  h.c_layer = a.eq.sigma_up * std::sqrt(3 * d * h.dt0);    // sigma_Up*sqrt(3*dim*dt) (:80, :94)
  h.R2 = a.eq.R * a.eq.R;                                  // R**2 (:122)
  return h;
}

template <typename T>
struct DevConsts {
  T gamma, R, dt0, sqrt_dt0, dt_min, inv_den, two_inv_den, c_layer, R2, neg_gamma;
  static DevConsts make(const HostConsts& h) {
    DevConsts c;
    c.gamma = (T)h.gamma; c.R = (T)h.R; c.dt0 = (T)h.dt0; c.sqrt_dt0 = (T)h.sqrt_dt0;
    c.dt_min = (T)h.dt_min; c.inv_den = (T)(1.0 / h.den); c.two_inv_den = (T)(2.0 / h.den);
    c.c_layer = (T)h.c_layer; c.R2 = (T)h.R2; c.neg_gamma = (T)(-h.gamma);
    return c;
  }
};

// Prefetch depth (steps per half ring) of the time loops.  The ring of 2*KB
// frames gets a fixed VGPR budget, so wide per-lane frames (VDP keeps the whole
// state in one lane) get a shallow ring instead of spilling: KB = 8 (f32) /
// 4 (f64) for the canonical d = 20 rollout frame of 2 values.
#ifndef DPAC_RING_VGPRS
#define DPAC_RING_VGPRS 32
#endif
#ifndef DPAC_ROLLOUT_KB_CAP
#define DPAC_ROLLOUT_KB_CAP 8
#endif
// Cache-policy immediates of k_rollout's streamed dw loads and x stores (0 = default,
// 2 = nt).  Measured with 5 rotating buffer sets (HBM, not Infinity-Cache resident):
// nt x stores 39.8 -> 38.0 us at B = 4096, 146 -> 131 us at 16384; nt dw loads no gain.
#ifndef DPAC_ROLLOUT_DW_AUX
#define DPAC_ROLLOUT_DW_AUX 0
#endif
#ifndef DPAC_ROLLOUT_X_AUX
#define DPAC_ROLLOUT_X_AUX 2
#endif
// KB = 0 (a frame larger than half the budget): no ring, each step loads its
// own frame right before computing.
constexpr int ring_kb(int frame_bytes, int budget_vgprs, int cap) {
  const int kb = budget_vgprs * 4 / (2 * frame_bytes);
  return kb > cap ? cap : kb;
}
// k_rollout's ring: its dt/coef flush writes F = min(P, 2*KB) steps at compile-time
// phases of the 2*KB-step period, so F must divide 2*KB and be a power of two (P is).
// Round KB down to the nearest value that keeps that: a multiple of P/2 when 2*KB >= P
// (F = P), else a power of two (F = 2*KB).  E.g. P = 8, M = 3: 5 -> 4; P = 4, M = 5: 3 -> 2.
constexpr int rollout_kb(int kb, int P) {
  if (kb < 1) kb = 1;
  if (2 * kb >= P) return kb - kb % (P / 2 > 0 ? P / 2 : 1);
  int p2 = 1;
  while (p2 * 2 <= kb) p2 *= 2;
  return p2;
}
// Timing-only ablations (never in a shipped build): 1 = skip the per-step
// stores of x/dt/coef, 2 = synthesize dw instead of loading it, 3 = skip the
// dt/coef stores, 4 = skip the x stores.
#ifndef DPAC_ABLATE
#define DPAC_ABLATE 0
#endif


// sqrt: the hardware v_sqrt_f32 for float (1 ulp), correctly rounded for double.
__device__ __forceinline__ float dsqrt(float v) { return __builtin_amdgcn_sqrtf(v); }
__device__ __forceinline__ double dsqrt(double v) { return sqrt(v); }

// ---------------------------------------------------------------------------
// Software-pipelined time loop over [t_begin, t_end): frames for KB steps are
// loaded while the previous KB steps compute.  Frame arrays are indexed only by
// unrolled constants, so they live in VGPRs.  body(t, frame, phase) receives
// phase = (t - t_begin) mod 2*KB as a compile-time constant wherever the
// unrolled position fixes it, and Phase<-1> in the scalar tail loop.
// ---------------------------------------------------------------------------
template <int V>
using Phase = std::integral_constant<int, V>;

// body(t + K, fr[K], Phase<BASE + K>) for K in the sequence; with CHECK,
// bodies with t + K >= t_end are skipped.
template <int BASE, bool CHECK, class F, class BodyF, int... K>
__device__ __forceinline__ void run_bodies(BodyF& body, int t, F* fr, int t_end,
                                           std::integer_sequence<int, K...>) {
  if constexpr (CHECK)
    ((t + K < t_end ? body(t + K, fr[K], Phase<BASE + K>{}) : void()), ...);
  else
    (body(t + K, fr[K], Phase<BASE + K>{}), ...);
}

template <int KB, class F, class LoadF, class BodyF>
__device__ __forceinline__ void pipelined(int t_begin, int t_end, LoadF&& load, BodyF&& body) {
  if (t_end <= t_begin) return;
  if constexpr (KB == 0) {
    for (int t = t_begin; t < t_end; ++t) {
      F f;
      load(t, f);
      body(t, f, Phase<-1>{});
    }
  } else {
    const int last = t_end - 1;
    F A[KB], Bq[KB];
    // Loads are never predicated: a load past the end re-reads the last step (in
    // bounds, unused).  A predicated load would force its wait at the branch join
    // and serialise the prefetch.
#pragma unroll
    for (int k = 0; k < KB; ++k) load(min(t_begin + k, last), A[k]);
    int t0 = t_begin;
    for (; t0 + 2 * KB <= t_end; t0 += 2 * KB) {
#pragma unroll
      for (int k = 0; k < KB; ++k) load(t0 + KB + k, Bq[k]);
      run_bodies<0, false>(body, t0, A, t_end, std::make_integer_sequence<int, KB>{});
#pragma unroll
      for (int k = 0; k < KB; ++k) load(min(t0 + 2 * KB + k, last), A[k]);
      run_bodies<KB, false>(body, t0 + KB, Bq, t_end, std::make_integer_sequence<int, KB>{});
    }
    // remainder (< 2*KB steps): A holds steps [t0, t0+KB)
    run_bodies<0, true>(body, t0, A, t_end, std::make_integer_sequence<int, KB>{});
    for (int t = t0 + KB; t < t_end; ++t) {
      F f;
      load(t, f);
      body(t, f, Phase<-1>{});
    }
  }
}

// |v|^2 of the owned slice (fma chain; every kernel uses this one form so all
// variants round identically).
template <typename T, int M>
__device__ __forceinline__ T sumsq(const T (&v)[M]) {
  T q = v[0] * v[0];
#pragma unroll
  for (int m = 1; m < M; ++m) q = fma(v[m], v[m], q);
  return q;
}

// XCD-aware block order (cdna_hip_programming.md §5.5 T1): the dispatcher deals
// blocks round-robin over the 8 XCDs, so blocks b and b+1 — whose per-step rows
// share cache lines (4 trajectories x 80 B = 2.5 lines) — would be written back
// from two different L2s as partial lines.  Remap so that each XCD owns one
// contiguous run of trajectory blocks (bijective for any grid size).
__device__ __forceinline__ int64_t xcd_block(int64_t b, int64_t nb) {
  const int64_t q = nb / 8, r = nb % 8, x = b % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

// Lane coordinates: trajectory b and lane slot p within its group.  Lane groups
// past the end of the batch compute on a duplicate of the last trajectory and
// store the same values it does (identical bits), so no store needs a guard.
template <int P>
struct LaneCoord {
  int p;
  int64_t b;
  bool live;
  __device__ __forceinline__ LaneCoord(int64_t B, int lane, int64_t group0) {
    p = lane % P;
    b = group0 + lane / P;
    live = b < B;
    if (!live) b = B - 1;
  }
};

// Adaptive-scheme state of a trajectory as two lane masks: alive = flag > 0,
// layer = flag == 1 (equation.py:80-82: flag 2 inner, 1 boundary layer, 0 out).
struct Flags {
  bool alive, layer;
  __device__ __forceinline__ int encode() const { return alive ? (layer ? 1 : 2) : 0; }
  __device__ __forceinline__ static Flags decode(int f) { return Flags{f > 0, f == 1}; }
};

// Region of a point at radius r: 1 + floor((sign(R-r-c) + sign(R-r))/2) is
// 2 if R-r-c > 0, 1 if R-r > 0, else 0 (equation.py:80-82, :94-95).
template <typename T>
__device__ __forceinline__ Flags region(T r, const DevConsts<T>& c) {
  const T b = c.R - r;
  const bool inball = b > T(0);
  const bool inner = b - c.c_layer > T(0);
  return Flags{inball, inball && !inner};
}

// (2f-f^2)(R-r)^2/den + (f^2-2f+1)dt0 (equation.py:85) is (R-r)^2/den for f == 1
// and dt0 for f in {0, 2}; the division is a multiply by 1/den.
template <typename T>
__device__ __forceinline__ T adaptive_dt_raw(bool layer, T r, const DevConsts<T>& c) {
  const T b = c.R - r;
  return layer ? (b * b) * c.inv_den : c.dt0;
}

// One transition of the scheme for the owned slice.  In: x, u, dw (masked),
// flags and r = |x|.  Out: xt = x + dx, coef, next flags, St = |xt|^2, rt = |xt|
// (adaptive or norm-dependent equations), dt and sqrt(dt).
template <typename T, class E, int SCHEME>
struct Transition {
  static constexpr int M = E::M, MC = E::MC, P = E::kP;
  static constexpr bool kRadius = SCHEME == DPAC_SCHEME_ADAPTIVE || E::kNeedsNorm;
  T xt[M], dx[M];
  T dt, sq, St, rt;
  bool coef;
  Flags next;
  __device__ __forceinline__ void run(const E& eq, const DevConsts<T>& c, const T (&x)[M],
                                      const T (&u)[MC], const T (&dw)[M], Flags fl, T r) {
    if constexpr (SCHEME == DPAC_SCHEME_ADAPTIVE) {
      // tf.maximum(dt_i, delta_t*1e-4) (:86): dt0 always exceeds the floor, so
      // only the boundary-layer branch is clamped (same bits, one instruction less)
      const T b = c.R - r;
      dt = fl.layer ? fmax((b * b) * c.inv_den, c.dt_min) : c.dt0;
      sq = dsqrt(dt);
    } else {
      dt = c.dt0;
      sq = c.sqrt_dt0;
    }
    T f[M], s[M];
    eq.drift(x, u, r, f);
    eq.sigma(x, u, s);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      dx[m] = fma(f[m], dt, (s[m] * dw[m]) * sq);  // drift*dt + diffusion*sqrt(dt) (:58, :91)
      xt[m] = x[m] + dx[m];
    }
    St = Lanes<P>::sum(sumsq(xt));
    rt = kRadius ? dsqrt(St) : T(0);
    if constexpr (SCHEME == DPAC_SCHEME_ADAPTIVE) {
      const Flags nf = region(rt, c);
      coef = fl.alive && nf.alive;                 // sign(flag)*sign(new_flag) (:96)
      next = Flags{coef, coef && nf.layer};        // new_flag*sign(flag) (:95)
    } else {
      const bool out = St - c.R2 >= T(0);         // ceil((sign(b(x))+1)/2) == 1 (:60-61)
      coef = fl.alive && !out;                    // flag*(1-Exit) (:62)
      next = Flags{coef, false};                  // flag *= 1 - Exit (:69)
    }
  }
};

template <typename T>
__device__ __forceinline__ T cost_increment(int order, T w, T coef, T dt, T disc) {
  return order == DPAC_COST_ACTOR ? ((coef * w) * dt) * disc   // coef*w*dt*discount (solver.py:218)
                                  : (w * disc) * (coef * dt);  // (w*discount)*(coef*dt) (:170-174)
}

template <typename T>
__device__ __forceinline__ T disc_factor(T dt, T coef, const DevConsts<T>& c) {
  return exp((c.neg_gamma * dt) * coef);  // exp(-gamma*dt*coef) (solver.py:187, :219)
}

// The increments of this lane's components at step t (in-kernel Philox).
template <typename T, class E, int D>
__device__ __forceinline__ void draw_owned(uint64_t seed, uint64_t gtraj, int t, int p,
                                           int sample_type, T (&out)[E::M]) {
  if constexpr (E::kP == 1) {
    draw_all<T, D>(seed, gtraj, t, sample_type, out);
  } else {
    static_assert(lanes_for_dim(D) == E::kP && comps_per_lane(D) == E::M,
                  "RNG slots follow the lane split");
    draw_slot<T, D>(seed, gtraj, t, p, sample_type, out);
  }
}

// ---------------------------------------------------------------------------
// Fused rollout with the analytic control u_true (reference `cheat` path).
// ---------------------------------------------------------------------------
template <typename T>
struct RolloutArgs {
  int64_t B, traj_offset;
  int N, sample_type, cost_order;
  uint64_t seed;
  const T* x0;
  const T* dw;
  T *x, *dt, *coef, *u, *y, *disc;
};

template <typename T, int M>
struct DwFrame {
  T dw[M];
};

// Optional outputs of k_rollout (template bits, so the time loop never tests them).
enum : int { kOutCost = 1, kOutU = 2 };

template <typename T, class E, int D, int SCHEME, bool PHILOX, int OUT, int KB>
__global__ __launch_bounds__(64) void k_rollout(const E eq, const DevConsts<T> c,
                                                 const RolloutArgs<T> a) {
  constexpr int P = E::kP, M = E::M, MC = E::MC;
  constexpr bool COST = (OUT & kOutCost) != 0, WANT_U = (OUT & kOutU) != 0;
  // dt / coef rows are trajectory-major [B][N] (the reference's dt[B,N]): lane
  // group keeps its last F steps in a lane shift register (lane p: step t - p,
  // dt with the sign of coef) and writes the F values of its row at once every
  // F steps (F divides the pipeline period 2*KB, so each unrolled body knows at
  // compile time whether it flushes).
  constexpr int F = P < 2 * KB ? P : 2 * KB;
  static_assert(KB >= 1 && (2 * KB) % F == 0 && (F & (F - 1)) == 0,
                "the dt/coef flush needs F | 2*KB and F a power of two (rollout_kb)");
  using TR = Transition<T, E, SCHEME>;
  const LaneCoord<P> lc(a.B, threadIdx.x, xcd_block(blockIdx.x, gridDim.x) * (64 / P));
  const Own<D, P> own(lc.p);
  const Own<E::CDIM, P> ownu(lc.p);
  const BufSlab<T, D, P> sx(own, lc.b, lc.live);           // x0, dw[t], x[t] rows
  const BufSlab<T, E::CDIM, P> su(ownu, lc.b, lc.live);    // u[t] rows
  // whole-array descriptors (host: every array < 2 GiB); the step goes in soffset
  const uint32_t slab = (uint32_t)(a.B * D * sizeof(T));
  const uint32_t slab_u = (uint32_t)(a.B * E::CDIM * sizeof(T));
  const uint32_t row_bytes = (uint32_t)(a.N * sizeof(T));
  const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(a.x, slab * (uint32_t)(a.N + 1));
  const __amdgpu_buffer_rsrc_t rs_dw = make_rsrc(a.dw, PHILOX ? 0u : slab * (uint32_t)a.N);
  const __amdgpu_buffer_rsrc_t rs_u = make_rsrc(a.u, WANT_U ? slab_u * (uint32_t)a.N : 0u);
  const __amdgpu_buffer_rsrc_t rs_dt = make_rsrc(a.dt, (uint32_t)a.B * row_bytes);
  const __amdgpu_buffer_rsrc_t rs_cf = make_rsrc(a.coef, (uint32_t)a.B * row_bytes);
  T keep = 0;  // coef_t ? dt_t : -dt_t (dt > 0 always) of step t_last - p
  auto flush = [&](int t_last, int count) {  // steps (t_last - count, t_last] of the row
    const uint32_t off = (lc.live && lc.p < count)
                             ? (uint32_t)((lc.b * a.N + t_last - lc.p) * (int64_t)sizeof(T)) : kOOB;
    buf_store_scalar<T>(rs_dt, off, fabs(keep));
    buf_store_scalar<T>(rs_cf, off, keep > T(0) ? T(1) : T(0));
  };

  T x[M];
  sx.load(make_rsrc(a.x0, slab), x);
  sx.store(rs_x, x);
  T r = TR::kRadius ? dsqrt(Lanes<P>::sum(sumsq(x))) : T(0);
  Flags fl = SCHEME == DPAC_SCHEME_ADAPTIVE ? region(r, c) : Flags{true, false};
  T disc = 1, y = 0;
  const uint64_t gtraj = (uint64_t)(a.traj_offset + lc.b);

  // in-kernel Philox, paired layout (dpac_device.h): the even step of a pair draws both steps'
  // increments; the odd step takes the half kept here (loads come in step order: pipelined())
  constexpr bool kPairable = PHILOX && E::kP > 1 && 2 * M <= 4;
  const bool paired = kPairable && dw_steps_per_block<T>(M, a.sample_type) == 2;
  T pend[M];
#pragma unroll
  for (int m = 0; m < M; ++m) pend[m] = T(0);
  auto load = [&](int t, DwFrame<T, M>& fr) {
    if constexpr (PHILOX) {
      if constexpr (kPairable) {
        if (paired) {
          if ((t & 1) == 0) {
            T v[2 * M];
            draw_slot_pair<T, D>(a.seed, gtraj, t >> 1, lc.p, a.sample_type, v);
#pragma unroll
            for (int m = 0; m < M; ++m) {
              fr.dw[m] = v[m];
              pend[m] = v[M + m];
            }
          } else {
#pragma unroll
            for (int m = 0; m < M; ++m) fr.dw[m] = pend[m];
          }
          return;
        }
      }
      draw_owned<T, E, D>(a.seed, gtraj, t, lc.p, a.sample_type, fr.dw);
    } else if constexpr (DPAC_ABLATE == 2 || DPAC_ABLATE == 5) {
#pragma unroll
      for (int m = 0; m < M; ++m) fr.dw[m] = T(((t * 7 + m + lc.p) & 3) - 1.5) * T(0.5);
    } else {
      sx.template load<DPAC_ROLLOUT_DW_AUX>(rs_dw, fr.dw, (uint32_t)t * slab);  // zero past d: no mask
    }
  };
  auto body = [&](int t, DwFrame<T, M>& fr, auto phase) {
    T dwv[M];
#pragma unroll
    for (int m = 0; m < M; ++m) dwv[m] = fr.dw[m];
    if constexpr (PHILOX) own.mask(dwv);
    T u[MC];
    eq.u_true(x, r, u);
    TR tr;
    tr.run(eq, c, x, u, dwv, fl, r);
    const T cf = tr.coef ? T(1) : T(0);
    if constexpr (COST) {
      const T w = eq.w_finish(Lanes<P>::sum(eq.w_part(x, u)));
      y += cost_increment(a.cost_order, w, cf, tr.dt, disc);
      disc = disc * disc_factor(tr.dt, cf, c);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = tr.coef ? tr.xt[m] : x[m];  // x + delta_x*coef (:67, :103)
    if constexpr (TR::kRadius) r = tr.coef ? tr.rt : r;
    fl = tr.next;
    if constexpr (DPAC_ABLATE == 1 || DPAC_ABLATE == 5) {
      if (t + 1 == a.N) sx.store(rs_x, x, (uint32_t)(t + 1) * slab);
      return;
    }
    if constexpr (DPAC_ABLATE != 4) sx.template store<DPAC_ROLLOUT_X_AUX>(rs_x, x, (uint32_t)(t + 1) * slab);
    if constexpr (WANT_U) su.store(rs_u, u, (uint32_t)t * slab_u);
    if constexpr (DPAC_ABLATE != 3) {
      constexpr int PH = decltype(phase)::value;
      keep = group_shift_in<P>(keep, tr.coef ? tr.dt : -tr.dt, lc.p == 0);
      if constexpr (PH >= 0) {
        if constexpr (PH % F == F - 1) flush(t, F);
      } else if ((t & (F - 1)) == F - 1) {
        flush(t, F);
      }
    }
  };
  pipelined<KB, DwFrame<T, M>>(0, a.N, load, body);
  if constexpr (DPAC_ABLATE != 3 && DPAC_ABLATE != 1 && DPAC_ABLATE != 5) {
    const int rem = a.N & (F - 1);
    if (rem) flush(a.N - 1, rem);
  }
  if constexpr (COST) {
    if (lc.live && lc.p == 0) {
      a.y[lc.b] = y;
      a.disc[lc.b] = disc;
    }
  }
}

#include "dpac_rollout_staged.h"

// ---------------------------------------------------------------------------
// Flag initialisation (adaptive: equation.py:78-82; naive: np.ones, :52)
// ---------------------------------------------------------------------------
template <typename T, class E, int D, int SCHEME>
__global__ __launch_bounds__(64) void k_flag_init(const E eq, const DevConsts<T> c, int64_t B,
                                                   const T* x0, int32_t* flag) {
  constexpr int P = E::kP, M = E::M;
  const LaneCoord<P> lc(B, threadIdx.x, xcd_block(blockIdx.x, gridDim.x) * (64 / P));
  const Own<D, P> own(lc.p);
  T xv[M];
  own.load_masked(x0 + lc.b * D, xv);
  const T r = dsqrt(Lanes<P>::sum(sumsq(xv)));
  if (lc.p == 0) flag[lc.b] = SCHEME == DPAC_SCHEME_ADAPTIVE ? region(r, c).encode() : 1;
}

// ---------------------------------------------------------------------------
// One transition with an external control (NN actor), fused cost/discount.
// ---------------------------------------------------------------------------
template <typename T>
struct StepArgs {
  int64_t B;
  int cost_order;
  const T *x, *u, *dw, *disc_in, *y_in;
  const int32_t* flag_in;
  T *x_out, *disc_out, *y_out, *dt, *coef;
  int32_t* flag_out;
  // backward
  const T *g_x_out, *g_disc_out, *g_y_out;
  T *g_x, *g_u, *g_disc;
};

template <typename T, class E, int D, int SCHEME>
__global__ __launch_bounds__(64) void k_step_fwd(const E eq, const DevConsts<T> c,
                                                  const StepArgs<T> a) {
  constexpr int P = E::kP, M = E::M, MC = E::MC;
  using TR = Transition<T, E, SCHEME>;
  const LaneCoord<P> lc(a.B, threadIdx.x, xcd_block(blockIdx.x, gridDim.x) * (64 / P));
  const Own<D, P> own(lc.p);
  const Own<E::CDIM, P> ownu(lc.p);
  T x[M], u[MC], dw[M];
  own.load_masked(a.x + lc.b * D, x);
  own.load_masked(a.dw + lc.b * D, dw);
  ownu.load_masked(a.u + lc.b * E::CDIM, u);
  const T r = TR::kRadius ? dsqrt(Lanes<P>::sum(sumsq(x))) : T(0);
  const Flags fl = Flags::decode(a.flag_in[lc.b]);
  const T disc = a.disc_in ? a.disc_in[lc.b] : T(1);
  TR tr;
  tr.run(eq, c, x, u, dw, fl, r);
  const T cf = tr.coef ? T(1) : T(0);
  const T w = eq.w_finish(Lanes<P>::sum(eq.w_part(x, u)));
  T xn[M];
#pragma unroll
  for (int m = 0; m < M; ++m) xn[m] = tr.coef ? tr.xt[m] : x[m];
  own.store(a.x_out + lc.b * D, xn);
  if (lc.p == 0) {
    const T yin = a.y_in ? a.y_in[lc.b] : T(0);
    if (a.y_out) a.y_out[lc.b] = yin + cost_increment(a.cost_order, w, cf, tr.dt, disc);
    if (a.disc_out) a.disc_out[lc.b] = disc * disc_factor(tr.dt, cf, c);
    if (a.dt) a.dt[lc.b] = tr.dt;
    if (a.coef) a.coef[lc.b] = cf;
    a.flag_out[lc.b] = SCHEME == DPAC_SCHEME_ADAPTIVE ? tr.next.encode() : (tr.coef ? 1 : 0);
  }
}

// VJP of k_step_fwd.  Derivation: with lam = dL/dx', E = exp(-g dt c),
//   dL/ddisc = g_disc'*E + g_y'*c*w*dt
//   dL/ddt   = g_disc'*disc*E*(-g*c) + g_y'*c*w*disc + c*Σ_j lam_j*(f_j + s_j dw_j/(2 sqrt(dt)))
//   dL/du    = c*dt*lam·∂f/∂u + c*sqrt(dt)*(lam⊙dw)·∂s/∂u + g_y'*c*dt*disc*∂w/∂u
//   dL/dx    = lam + (same three terms w.r.t. x) + dL/ddt * ∂dt/∂x
//   ∂dt/∂x   = -2(R-r)x/(r*den) if flag == 1 and dt_raw >= 1e-4 dt0 (TF max tie rule), else 0
// The VJP of one transition for the owned slice (shared by k_step_bwd and the
// fused reverse rollout).  lam = dL/dx', gD1 = dL/ddisc', gy1 = dL/dy'.
template <typename T, class E, int SCHEME>
__device__ __forceinline__ void step_vjp(const E& eq, const DevConsts<T>& c, const T (&x)[E::M],
                                         const T (&u)[E::MC], const T (&dw)[E::M], Flags fl,
                                         T disc, const T (&lam)[E::M], T gD1, T gy1,
                                         T (&gx)[E::M], T (&gu)[E::MC], T& g_disc) {
  constexpr int P = E::kP, M = E::M, MC = E::MC;
  using TR = Transition<T, E, SCHEME>;
  const T r = dsqrt(Lanes<P>::sum(sumsq(x)));
  TR tr;
  tr.run(eq, c, x, u, dw, fl, r);
  const T cf = tr.coef ? T(1) : T(0);
  const T w = eq.w_finish(Lanes<P>::sum(eq.w_part(x, u)));
  const T Ef = disc_factor(tr.dt, cf, c);

  T f[M], s[M];
  eq.drift(x, u, r, f);
  eq.sigma(x, u, s);
  T a_f[M], a_s[M];
  T part = 0;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    gx[m] = lam[m];
    a_f[m] = lam[m] * cf * tr.dt;
    a_s[m] = lam[m] * cf * tr.sq * dw[m];
    part += lam[m] * (f[m] + s[m] * dw[m] / (2 * tr.sq));
  }
#pragma unroll
  for (int m = 0; m < MC; ++m) gu[m] = 0;
  eq.drift_vjp(x, u, r, a_f, gx, gu);
  eq.sigma_vjp(x, u, a_s, gx, gu);
  const T gw = gy1 * cf * tr.dt * disc;
  eq.w_vjp(x, u, gw, gx, gu);
  g_disc = gD1 * Ef + gy1 * cf * w * tr.dt;
  if constexpr (SCHEME == DPAC_SCHEME_ADAPTIVE) {
    const T g_dt = gD1 * disc * Ef * (c.neg_gamma * cf) + gy1 * cf * w * disc + cf * Lanes<P>::sum(part);
    const T raw = adaptive_dt_raw(fl.layer, r, c);
    if (fl.layer && raw >= c.dt_min) {
      const T k = g_dt * (-(c.R - r) * c.two_inv_den) / r;
#pragma unroll
      for (int m = 0; m < M; ++m) gx[m] += k * x[m];
    }
  }
}

template <typename T, class E, int D, int SCHEME>
__global__ __launch_bounds__(64) void k_step_bwd(const E eq, const DevConsts<T> c,
                                                  const StepArgs<T> a) {
  constexpr int P = E::kP, M = E::M, MC = E::MC;
  const LaneCoord<P> lc(a.B, threadIdx.x, xcd_block(blockIdx.x, gridDim.x) * (64 / P));
  const Own<D, P> own(lc.p);
  const Own<E::CDIM, P> ownu(lc.p);
  T x[M], u[MC], dw[M], lam[M];
  own.load_masked(a.x + lc.b * D, x);
  own.load_masked(a.dw + lc.b * D, dw);
  own.load_masked(a.g_x_out + lc.b * D, lam);
  ownu.load_masked(a.u + lc.b * E::CDIM, u);
  const Flags fl = Flags::decode(a.flag_in[lc.b]);
  const T disc = a.disc_in ? a.disc_in[lc.b] : T(1);
  const T gD1 = a.g_disc_out ? a.g_disc_out[lc.b] : T(0);
  const T gy1 = a.g_y_out ? a.g_y_out[lc.b] : T(0);
  T gx[M], gu[MC], g_disc;
  step_vjp<T, E, SCHEME>(eq, c, x, u, dw, fl, disc, lam, gD1, gy1, gx, gu, g_disc);
  own.store(a.g_x + lc.b * D, gx);
  ownu.store(a.g_u + lc.b * E::CDIM, gu);
  if (a.g_disc && lc.p == 0) a.g_disc[lc.b] = g_disc;
}

// ---------------------------------------------------------------------------
// TD target assembly over a finished trajectory (solver.py:166-190) and its
// backward with respect to G.  Workgroup = 4 wavefronts over the same 64/P
// trajectories; wavefront w owns steps [w*Nc, (w+1)*Nc).  Each computes its
// chunk with a local discount starting at 1, then the (sum, product) pairs are
// combined in chunk order through LDS: y = Σ_w D_w L_w, D_{w+1} = D_w E_w.
// ---------------------------------------------------------------------------
constexpr int kTdChunks = 4;

template <typename T>
struct TdArgs {
  int64_t B, traj_offset;
  int N, sample_type, cost_order;
  uint64_t seed;
  const T *x, *u, *dw, *dt, *coef, *G, *g_y;
  T *y, *disc, *g_G;
  const T* gd;  // GDOT forward: [N][B] diffusion dots from dpac_mlp_rows_fwd_td1
  T* g_gd;      // GDOT backward: [N][B] d y / d gdot
};

template <typename T, int M, int MC, bool HAS_DW, bool HAS_G>
struct TdFrame {
  T x[M], u[MC], dw[HAS_DW ? M : 1], G[HAS_G ? M : 1];
  T dt, coef, gd;
};

// GDOT: the TD1 diffusion dot of each trajectory-step comes
// precomputed from the G network's epilogue (dpac_mlp_rows_fwd_td1, bitwise the dot
// below), so the forward reads one scalar instead of G and dw, and the backward writes
// the scalar d y / d gdot instead of d y / d G (the G network's backward forms the
// latter in its prologue, dpac_mlp_rows_bwd_td1) and reads neither x, u nor dw.
template <typename T, class E, int D, bool TD1, bool PHILOX, bool BWD, bool GDOT = false>
__global__ __launch_bounds__(256) void k_td(const E eq, const DevConsts<T> c, const TdArgs<T> a) {
  constexpr int P = E::kP, M = E::M, MC = E::MC, GPW = 64 / P;
  constexpr bool USE_DW = (TD1 || BWD) && !GDOT;
  constexpr bool HAS_G = TD1 && !BWD && !GDOT;
  using F = TdFrame<T, M, MC, USE_DW && !PHILOX, HAS_G>;
  constexpr int KB = ring_kb((int)sizeof(F), 3 * DPAC_RING_VGPRS, sizeof(T) == 4 ? 4 : 2);
  __shared__ T s_sum[kTdChunks][GPW];
  __shared__ T s_prod[kTdChunks][GPW];

  // wave index is wave-uniform: say so, or the chunk loops become divergent branches
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
  const LaneCoord<P> lc(a.B, lane, xcd_block(blockIdx.x, gridDim.x) * GPW);
  const Own<D, P> own(lc.p);
  const Own<E::CDIM, P> ownu(lc.p);
  const BufSlab<T, D, P> sx(own, lc.b, lc.live);         // x[t], dw[t], G[t], g_G[t] rows
  const BufSlab<T, E::CDIM, P> su(ownu, lc.b, lc.live);  // u[t] rows
  const int g = lane / P;
  const int64_t B = a.B, stride = a.B * D, stride_u = a.B * E::CDIM;
  const uint32_t slab = (uint32_t)(stride * sizeof(T)), slab_u = (uint32_t)(stride_u * sizeof(T));
  const uint64_t gtraj = (uint64_t)(a.traj_offset + lc.b);
  const int nc = (a.N + kTdChunks - 1) / kTdChunks;
  const int t_begin = min(a.N, wave * nc), t_end = min(a.N, (wave + 1) * nc);

  // whole-array descriptors (host: every array < 2 GiB); the step goes in soffset
  const uint32_t row_bytes = (uint32_t)(a.N * sizeof(T));
  const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(a.x, slab * (uint32_t)a.N);
  const __amdgpu_buffer_rsrc_t rs_u = make_rsrc(a.u, slab_u * (uint32_t)a.N);
  const __amdgpu_buffer_rsrc_t rs_dw = make_rsrc(a.dw, (USE_DW && !PHILOX) ? slab * (uint32_t)a.N : 0u);
  const __amdgpu_buffer_rsrc_t rs_G = make_rsrc(a.G, HAS_G ? slab * (uint32_t)a.N : 0u);
  const __amdgpu_buffer_rsrc_t rs_gG = make_rsrc(a.g_G, (BWD && !GDOT) ? slab * (uint32_t)a.N : 0u);
  const uint32_t gd_bytes = (uint32_t)(B * a.N * (int64_t)sizeof(T));
  const __amdgpu_buffer_rsrc_t rs_gd = make_rsrc(GDOT ? (BWD ? (const T*)a.g_gd : a.gd) : nullptr,
                                                 GDOT ? gd_bytes : 0u);
  const uint32_t off_gd = (uint32_t)(lc.b * (int64_t)sizeof(T));  // gdot rows are [N][B]
  const __amdgpu_buffer_rsrc_t rs_dt = make_rsrc(a.dt, (uint32_t)a.B * row_bytes);
  const __amdgpu_buffer_rsrc_t rs_cf = make_rsrc(a.coef, (uint32_t)a.B * row_bytes);
  const uint32_t off_row = (uint32_t)(lc.b * row_bytes);  // dt / coef rows are [B][N]
  auto load_scalar = [&](__amdgpu_buffer_rsrc_t r, int t) {
    uint32_t w[sizeof(T) / 4];
    buf_load_dwords<sizeof(T) / 4>(r, off_row, w, (uint32_t)t * (uint32_t)sizeof(T));
    T v;
    __builtin_memcpy(&v, &w[0], sizeof(T));
    return v;
  };
  auto load = [&](int t, F& fr) {
    if constexpr (!(GDOT && BWD)) {
      sx.load(rs_x, fr.x, (uint32_t)t * slab);
      su.load(rs_u, fr.u, (uint32_t)t * slab_u);
    }
    if constexpr (USE_DW && !PHILOX) sx.load(rs_dw, fr.dw, (uint32_t)t * slab);
    if constexpr (HAS_G) sx.load(rs_G, fr.G, (uint32_t)t * slab);
    if constexpr (GDOT && !BWD) {
      uint32_t w[sizeof(T) / 4];
      buf_load_dwords<sizeof(T) / 4>(rs_gd, off_gd, w, (uint32_t)t * (uint32_t)(B * sizeof(T)));
      __builtin_memcpy(&fr.gd, &w[0], sizeof(T));
    }
    fr.dt = load_scalar(rs_dt, t);
    fr.coef = load_scalar(rs_cf, t);
  };
  auto increments = [&](int t, F& fr, T (&dwv)[M]) {
    if constexpr (PHILOX) {
      draw_owned<T, E, D>(a.seed, gtraj, t, lc.p, a.sample_type, dwv);
      own.mask(dwv);
    } else {
#pragma unroll
      for (int m = 0; m < M; ++m) dwv[m] = fr.dw[m];
    }
  };

  T disc = 1;
  if constexpr (!BWD) {
    T y = 0;
    auto body = [&](int t, F& fr, auto) {
      const T w = eq.w_finish(Lanes<P>::sum(eq.w_part(fr.x, fr.u)));
      y += cost_increment(a.cost_order, w, fr.coef, fr.dt, disc);
      if constexpr (GDOT) {
        y -= (fr.gd * disc) * (fr.coef * dsqrt(fr.dt));  // solver.py:180-184, dot precomputed
      } else if constexpr (TD1) {
        T s[M], dwv[M];
        eq.sigma(fr.x, fr.u, s);
        increments(t, fr, dwv);
        T acc = (s[0] * dwv[0]) * fr.G[0];
#pragma unroll
        for (int m = 1; m < M; ++m) acc = fma(s[m] * dwv[m], fr.G[m], acc);
        const T dot = Lanes<P>::sum(acc);
        y -= (dot * disc) * (fr.coef * dsqrt(fr.dt));  // solver.py:180-184
      }
      disc = disc * disc_factor(fr.dt, fr.coef, c);
    };
    pipelined<KB, F>(t_begin, t_end, load, body);
    if (lc.p == 0) {
      s_sum[wave][g] = y;
      s_prod[wave][g] = disc;
    }
    __syncthreads();
    if (wave == 0 && lc.p == 0 && lc.live) {
      T Dw = 1, tot = 0;
#pragma unroll
      for (int w = 0; w < kTdChunks; ++w) {
        tot += Dw * s_sum[w][g];
        Dw *= s_prod[w][g];
      }
      a.y[lc.b] = tot;
      a.disc[lc.b] = Dw;
    }
  } else {
    // pass A: the chunk's discount product from (dt, coef) only
    for (int t = t_begin; t < t_end; ++t) {
      const int64_t so = lc.b * a.N + t;
      disc = disc * disc_factor(a.dt[so], a.coef[so], c);
    }
    if (lc.p == 0) s_prod[wave][g] = disc;
    __syncthreads();
    T Dw = 1;
    for (int w = 0; w < wave; ++w) Dw *= s_prod[w][g];
    disc = Dw;
    const T gy = a.g_y[lc.b];
    auto body = [&](int t, F& fr, auto) {
      // d y / d G_j = -disc_t*coef_t*sqrt(dt_t)*diff_j
      const T k = -gy * (disc * (fr.coef * dsqrt(fr.dt)));
      if constexpr (GDOT) {
        const uint32_t off = (lc.live && lc.p == 0) ? off_gd : kOOB;
        buf_store_scalar<T>(rs_gd, off, k, (uint32_t)t * (uint32_t)(B * sizeof(T)));
      } else {
        T s[M], dwv[M], out[M];
        eq.sigma(fr.x, fr.u, s);
        increments(t, fr, dwv);
#pragma unroll
        for (int m = 0; m < M; ++m) out[m] = k * (s[m] * dwv[m]);
        sx.store(rs_gG, out, (uint32_t)t * slab);
      }
      disc = disc * disc_factor(fr.dt, fr.coef, c);
    };
    pipelined<KB, F>(t_begin, t_end, load, body);
  }
}

// ---------------------------------------------------------------------------
// Row-wise evaluation of one Equation method (parity tests, metrics).
// ---------------------------------------------------------------------------
template <typename T, class E, int D>
__global__ __launch_bounds__(64) void k_eval(const E eq, const DevConsts<T> c, int64_t B,
                                              int what, const T* x, const T* u, T* out) {
  constexpr int P = E::kP, M = E::M, MC = E::MC;
  const LaneCoord<P> lc(B, threadIdx.x, xcd_block(blockIdx.x, gridDim.x) * (64 / P));
  const Own<D, P> own(lc.p);
  const Own<E::CDIM, P> ownu(lc.p);
  T xv[M], uv[MC];
  own.load_masked(x + lc.b * D, xv);
  if (u) {
    ownu.load_masked(u + lc.b * E::CDIM, uv);
  } else {
#pragma unroll
    for (int m = 0; m < MC; ++m) uv[m] = 0;
  }
  const T S = Lanes<P>::sum(sumsq(xv));
  const T r = dsqrt(S);
  T v[M];
  T scalar = 0;
  bool vec = false, ctl = false;
  switch (what) {
    case DPAC_EVAL_DRIFT: eq.drift(xv, uv, r, v); vec = true; break;
    case DPAC_EVAL_SIGMA: eq.sigma(xv, uv, v); vec = true; break;
    case DPAC_EVAL_W: scalar = eq.w_finish(Lanes<P>::sum(eq.w_part(xv, uv))); break;
    case DPAC_EVAL_Z: scalar = eq.Z(xv, S, r); break;
    case DPAC_EVAL_V_TRUE: scalar = eq.V_true(xv, S, r); break;
    case DPAC_EVAL_U_TRUE: {
      T uu[MC];
      eq.u_true(xv, r, uu);
      ownu.store(out + lc.b * E::CDIM, uu);
      ctl = true;
      break;
    }
    case DPAC_EVAL_V_GRAD: eq.V_grad(xv, S, r, v); vec = true; break;
    case DPAC_EVAL_B: scalar = S - c.R2; break;
    default: break;
  }
  if (ctl) return;
  if (vec) {
    own.store(out + lc.b * D, v);
  } else if (lc.p == 0) {
    out[lc.b] = scalar;
  }
}

#include "dpac_rollout_nn.h"
#include "dpac_rollout_nn_bwd.h"
#include "dpac_rollout_nn4.h"
#include "dpac_rollout_nn_x3.h"

#include "dpac_launch.h"

}  // namespace dpac
