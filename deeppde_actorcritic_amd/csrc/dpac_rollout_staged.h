// dpac_rollout_staged.h — k_rollout with the increments staged through LDS by a loader
// wavefront (or drawn into LDS by generator wavefronts): the ring plan, the producers, the
// clock trace and the build knobs DPAC_ST_*.
//
// Why: gfx950 counts a wave's vector loads and stores in ONE in-order vmcnt, so in
// k_rollout the wait for step t's dw also waits for every x / dt / coef store issued
// before that load.  With HBM-cold data (measured, 5 rotating sets, B = 4096): loads
// alone 24.9 us, stores alone 26.8 us, both 38.5 us — the coupling, not bandwidth,
// costs the difference (profiles/r02_rollout_cold_ablations.txt).
// Here a workgroup is CW = 4 compute wavefronts (16 trajectories at P = 16) plus one
// LOADER wavefront that copies the workgroup's dw rows of each step (one contiguous
// row block in the step-major layout) into an RS-step LDS ring with global_load_lds,
// CH steps ahead of use; the compute wavefronts read dw from LDS and only store.  The
// loader's vmcnt holds only its DMA; the compute waves' holds only stores, which no
// one waits for.  Hand-off through LDS counters: `ready` (steps landed, loader) and
// `done[w]` (steps consumed, per compute wave), polled with s_sleep; the loader stays
// at most RS steps ahead.  Arithmetic per step is k_rollout's (bitwise the same).
#pragma once
// Included by dpac_kernels.h inside namespace dpac, after k_rollout.

#ifndef DPAC_ST_CHUNKS
#define DPAC_ST_CHUNKS 4  // hand-off chunks in the LDS ring
#endif
#ifndef DPAC_ST_TIGHT
#define DPAC_ST_TIGHT 0  // timing knob: 16-byte-aligned slots for every plan
#endif
#ifndef DPAC_ST_TIGHT_CHUNKS
#define DPAC_ST_TIGHT_CHUNKS 3  // hand-off chunks of a ring of 16-byte-aligned slots
#endif
#ifndef DPAC_ST_CHEAP_CHUNKS
// chunks, from the horizon's start, that the loader issues through its cheap path (st_issue_chunk);
// 2 is what the first hand-off needs (chunk 0 is published once chunk 1 is issued); a large value
// (timing knob) issues every whole chunk that way
#define DPAC_ST_CHEAP_CHUNKS 2
#endif
#ifndef DPAC_ST_PREFETCH
// compute waves: 1 a whole chunk's dw read into registers at the chunk's top and an unrolled
// remainder, where the instantiation takes it (kChunkRegs, below); 0 (timing knob) every
// instantiation reads one step ahead of use and runs a rolled remainder loop
#define DPAC_ST_PREFETCH 1
#endif
constexpr int kStCW = 4;   // compute wavefronts per workgroup
constexpr int kStCH = 16;  // steps per hand-off chunk
constexpr int kStCheapChunks = DPAC_ST_CHEAP_CHUNKS < 4096 ? DPAC_ST_CHEAP_CHUNKS : 4096;
static_assert(kStCheapChunks >= 0, "DPAC_ST_CHEAP_CHUNKS counts chunks");
constexpr int kStPrefetch = DPAC_ST_PREFETCH;
static_assert(kStPrefetch == 0 || kStPrefetch == 1, "DPAC_ST_PREFETCH is 0 or 1");
template <typename T, int D, int P>
struct StagedPlan {
  static constexpr int TPW = kStCW * (64 / P);                                   // trajectories per workgroup
  static constexpr int SLOT = TPW * D * (int)sizeof(T);                          // bytes of one step's rows
  static constexpr int PIECES = (SLOT + 1023) / 1024;                            // 1 KB DMA instructions per step
  // ring depth (steps): the loader publishes a chunk once the next one is issued, so it
  // needs >= 2 chunks; 4 keep it far enough ahead that the compute waves never wait
  // (measured at B = 4096, cold: 4 chunks 29.3 us, 2 chunks 41.6, k_rollout 38.3).  Slots
  // are 1 KB-aligned when 4 chunks of them fit in 128 KB; otherwise (float64 at d = 20:
  // 2560-byte slots) 3 chunks of 16-byte-aligned slots (121 KB) — every DMA piece still
  // starts inside its slot and the lane-0 filler write (at k*1024 < SLOT) never reaches
  // the pad.  Plans that fit neither way run k_rollout.
  static constexpr int kLdsCap = 128 * 1024;
  static constexpr int SLOT_1K = (SLOT + 16 + 1023) / 1024 * 1024;
  static constexpr int SLOT_16 = (SLOT + 16 + 15) / 16 * 16;
  static constexpr bool kWide = !DPAC_ST_TIGHT && DPAC_ST_CHUNKS * kStCH * SLOT_1K <= kLdsCap;
  static constexpr int CHUNKS = kWide ? DPAC_ST_CHUNKS : DPAC_ST_TIGHT_CHUNKS;
  static constexpr int SLOT_LDS = kWide ? SLOT_1K : SLOT_16;  // + a zero pad no DMA writes
  static constexpr int PADOFF = SLOT_LDS - 16;                 // where empty lanes read 0
  static constexpr int RS = CHUNKS * kStCH;
  static_assert(P < 4 || (SLOT % 16 == 0 && (PIECES - 1) * 1024 + 16 <= SLOT), "DMA pieces stay inside the slot");
  // the loader's cheap issue path: a step's pieces before the last are whole (64 lanes x 16
  // bytes), the last has kLastLanes lanes, and a piece is addressed by the instruction's
  // immediate offset (12 bits unsigned at least, for the global and the LDS address alike)
  static constexpr int kLastLanes = (SLOT - (PIECES - 1) * 1024) / 16;
  static_assert(P < 4 || SLOT % 16 == 0, "a step's rows are whole 16-byte lane pieces");
  static_assert(P < 4 || (kLastLanes >= 1 && kLastLanes <= 64), "the last piece has 1 .. 64 lanes");
  static_assert(P < 4 || ((PIECES - 1) * 1024 + kLastLanes * 16 == SLOT), "the pieces cover the slot exactly");
  static constexpr bool kOk = P >= 4 && RS * SLOT_LDS <= kLdsCap && kStCH * PIECES <= 62;
  static_assert(!kOk || (PIECES - 1) * 1024 < (1 << 12), "a piece's offset fits the immediate field");
};

template <class Fn, int... S>
__device__ __forceinline__ void unroll_phases(Fn& fn, std::integer_sequence<int, S...>) {
  (fn(Phase<S>{}), ...);
}

__device__ __forceinline__ int lds_load_relaxed(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_store_relaxed(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// GEN > 0 (round 6): the in-kernel Philox rollout on the same ring.  GEN
// generator wavefronts (one per SIMD) take the loader's place and draw the workgroup's increments
// into the ring, one counter block per lane and pass (the paired stream layout of dpac_device.h:
// a block is one lane slot's two components at two steps), so all 64 lanes of a generator do
// useful Philox and Box-Muller work, beside the compute wavefronts' latency-bound time loop,
// instead of each compute lane drawing its own (6 of 16 lanes idle at d = 20).  Values and
// arithmetic are k_rollout's Philox path's: bitwise its results.
template <int GEN>
constexpr int st_waves() { return kStCW + (GEN > 0 ? GEN : 1); }
#ifndef DPAC_ST_GEN
#define DPAC_ST_GEN 12  // generator wavefronts of the Philox variant (three per SIMD; round 6: 2 / 4 / 8 / 12 measured)
#endif
constexpr int kStGen = DPAC_ST_GEN;
static_assert(64 * st_waves<kStGen>() <= 1024, "DPAC_ST_GEN: a workgroup holds at most 1024 threads");

// The hand-off polls.  Producers wait until every compute wave has consumed the steps before
// `need` (the slots they are about to overwrite); compute waves wait until every producer has
// published the steps before `want`.
__device__ __forceinline__ void st_wait_consumed(const int* s_done, int need) {
  for (;;) {
    int mn = lds_load_relaxed(&s_done[0]);
#pragma unroll
    for (int w = 1; w < kStCW; ++w) mn = min(mn, lds_load_relaxed(&s_done[w]));
    if (mn >= need) break;
    __builtin_amdgcn_s_sleep(2);
  }
}
template <int NREADY>
__device__ __forceinline__ void st_wait_published(const int* s_ready, int want) {
  for (;;) {
    int mn = lds_load_relaxed(&s_ready[0]);
#pragma unroll
    for (int w = 1; w < NREADY; ++w) mn = min(mn, lds_load_relaxed(&s_ready[w]));
    if (mn >= want) break;
    __builtin_amdgcn_s_sleep(1);
  }
}

// The loader's cheap issue of one chunk: NL 1 KB DMA pieces of each of the chunk's kStCH steps,
// at byte offsets OFF0 + j * 1024 of the step's rows and of its slot (the instruction's immediate
// offset applies to the global and to the LDS address alike).  g is the lane's source address in
// the chunk's first step, slot the LDS address of the chunk's first slot (a chunk's slots are
// contiguous: RS is a multiple of kStCH).  The loader is a lone wavefront and issue-bound, about
// 4.5 cycles per instruction, so a piece costs what its address arithmetic costs: here a step is
// one add on m0, one 64-bit add on the address and its loads, in ONE statement, which saves and
// restores m0 once (the compiler reserves m0 and knows nothing of the loads: it inserts no vmcnt
// wait for them, which the counted publish relies on).  The VALU add between the write of m0 and
// the load that reads it is the wait state that pair needs; the first step has an s_nop.
// Every lane the caller leaves enabled reads 16 bytes per piece: the caller bounds them.
#define DPAC_ST_LD1 "global_load_lds_dwordx4 %1, off offset:%5\n\t"
#define DPAC_ST_LD2 DPAC_ST_LD1 "global_load_lds_dwordx4 %1, off offset:%6\n\t"
#define DPAC_ST_ADV "s_add_u32 m0, m0, %4\n\tv_lshl_add_u64 %1, %1, 0, %3\n\t"
#define DPAC_ST_X15(a) a a a a a a a a a a a a a a a
#define DPAC_ST_CHUNK_ASM(LD)                                                                        \
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t" LD DPAC_ST_X15(DPAC_ST_ADV LD) \
               "s_mov_b32 m0, %0"                                                                    \
               : "=&s"(keep), "+v"(g)                                                                \
               : "s"(slot), "s"(step_bytes), "n"(SLOT_LDS), "n"(OFF0), "n"(OFF0 + 1024)              \
               : "memory", "scc")
template <int NL, int OFF0, int SLOT_LDS>
__device__ __forceinline__ void st_issue_chunk(uint64_t g, uint32_t slot, int64_t step_bytes) {
  static_assert(kStCH == 16, "the statement is one step and 15 advances");
  static_assert(NL >= 0 && NL <= 2 && OFF0 + (NL - 1) * 1024 < (1 << 12), "immediate offsets");
  [[maybe_unused]] int keep;
  if constexpr (NL == 1) DPAC_ST_CHUNK_ASM(DPAC_ST_LD1);
  if constexpr (NL == 2) DPAC_ST_CHUNK_ASM(DPAC_ST_LD2);
}
#undef DPAC_ST_CHUNK_ASM
#undef DPAC_ST_X15
#undef DPAC_ST_ADV
#undef DPAC_ST_LD2
#undef DPAC_ST_LD1

// Timing-only builds (-DDPAC_ST_TRACE=1, like DPAC_NN_TRACE): lane 0 of every wavefront of the
// first and the last workgroup stores the shader clock (low 32 bits) at fixed points of
// k_rollout_staged into a per-TU device table, read back by dpac_debug_staged_trace
// (tools/probe_staged_trace.py).  Row layout, kStTraceRow words per (workgroup, wavefront):
//   0 entry, 1 after the barrier, 2 x0 loaded, 3 first chunk seen ready, 4 the last store issued
//   (loader: after its last publish), 7 every store acknowledged, 5 / 6 the 100 MHz real-time
//   clock at entry / at the end;
//   16 + c  chunk c: compute waves start it (ready seen); loader starts issuing it
//   48 + c  chunk c: compute waves finish it; loader has issued it
//   80 + c  chunk c: cycles the compute waves polled `ready`; loader: when it published in pass c
#ifndef DPAC_ST_TRACE
#define DPAC_ST_TRACE 0
#endif
#if DPAC_ST_TRACE
constexpr int kStTraceRow = 128, kStTraceWaves = 16, kStTraceChunks = 32;
static __device__ uint32_t g_st_trace[2 * kStTraceWaves * kStTraceRow];  // [first | last workgroup][wave][point]
__device__ __forceinline__ uint32_t st_clock() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return (uint32_t)t;
}
__device__ __forceinline__ uint32_t st_realtime() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return (uint32_t)t;
}
#define ST_PUT(pt, v)                \
  do {                               \
    const uint32_t st_v_ = (v);      \
    if (st_on) st_row[(pt)] = st_v_; \
  } while (0)
#define ST_MARK(pt) ST_PUT(pt, st_clock())
#define ST_CHUNK(base, c0) ((base) + ((c0) / kStCH < kStTraceChunks ? (c0) / kStCH : kStTraceChunks - 1))
#else
#define ST_PUT(pt, v) \
  do {                \
  } while (0)
#define ST_MARK(pt) \
  do {              \
  } while (0)
#endif

template <typename T, class E, int D, int SCHEME, int OUT, int GEN = 0>
__global__ __launch_bounds__(64 * st_waves<GEN>()) void k_rollout_staged(const E eq, const DevConsts<T> c,
                                                                          const RolloutArgs<T> a) {
  constexpr int P = E::kP, M = E::M, MC = E::MC;
  using PL = StagedPlan<T, D, P>;
  constexpr int TPW = PL::TPW, RS = PL::RS, PIECES = PL::PIECES, SLOT_LDS = PL::SLOT_LDS;
  constexpr bool COST = (OUT & kOutCost) != 0, WANT_U = (OUT & kOutU) != 0;
  constexpr int F = P < kStCH ? P : kStCH;
  constexpr int NREADY = GEN > 0 ? GEN : 1;  // producers: the loader, or the generators
  static_assert(kStCH % F == 0 && (F & (F - 1)) == 0, "flush phase fixed per unrolled body");
  static_assert(GEN == 0 || (2 * M <= 4 && kStCH % 2 == 0), "generators draw the paired layout");
  using TR = Transition<T, E, SCHEME>;
  __shared__ __attribute__((aligned(16))) unsigned char s_ring[RS * SLOT_LDS];
  __shared__ int s_ready[NREADY], s_done[kStCW];
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / 64), lane = (int)threadIdx.x % 64;
  const int64_t row0 = xcd_block(blockIdx.x, gridDim.x) * TPW;
  const int N = a.N;
#if DPAC_ST_TRACE
  const bool st_on = lane == 0 && wave < kStTraceWaves && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1);
  uint32_t* const st_row = g_st_trace + ((blockIdx.x == 0 ? 0 : kStTraceWaves) + (wave < kStTraceWaves ? wave : 0)) * kStTraceRow;
  ST_MARK(0);
  ST_PUT(5, st_realtime());
#endif
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < NREADY; ++w) s_ready[w] = 0;
#pragma unroll
    for (int w = 0; w < kStCW; ++w) s_done[w] = 0;
  }
  if (threadIdx.x < RS * 4)  // the zero pads (lanes that own no component read them)
    reinterpret_cast<uint32_t*>(s_ring + (threadIdx.x / 4) * SLOT_LDS + PL::PADOFF)[threadIdx.x % 4] = 0u;
  __syncthreads();
  ST_MARK(1);

  if constexpr (GEN > 0) {
    if (wave >= kStCW) {  // ---- generator g: its share of each chunk's counter blocks -> the ring ----
      const int g = wave - kStCW;
      const int64_t rows_live = (a.B - row0) < TPW ? (a.B - row0) : TPW;
      constexpr int PLS = (D + M - 1) / M;                // lane slots that own components
      constexpr int NBLK = (kStCH / 2) * TPW * PLS;       // blocks per chunk (d = 20: 8 x 16 x 10)
      constexpr int PASSES = (NBLK + 64 * GEN - 1) / (64 * GEN);
      constexpr int SLOT_T = SLOT_LDS / (int)sizeof(T);
      T* const ringw = reinterpret_cast<T*>(s_ring);
      for (int c0 = 0; c0 < N; c0 += kStCH) {
        const int need = c0 + kStCH - RS;  // the chunk's slots were last read at steps < need
        if (need > 0) st_wait_consumed(s_done, need);
        asm volatile("" ::: "memory");
#pragma unroll 1
        for (int k = 0; k < PASSES; ++k) {
          const int e = (k * GEN + g) * 64 + lane;
          const int u = e / (TPW * PLS), rem = e - u * (TPW * PLS);
          const int i = rem / PLS, p = rem - i * PLS;
          const int t0 = c0 + 2 * u;
          if (e < NBLK && t0 < N && i < rows_live) {
            T v[4];
            dw_block_values<T>(a.seed, (uint64_t)(a.traj_offset + row0 + i), (uint64_t)(t0 >> 1) * P + p,
                               a.sample_type, v);
            T* d0 = ringw + (t0 % RS) * SLOT_T + i * D + p * M;
            T* d1 = ringw + ((t0 + 1) % RS) * SLOT_T + i * D + p * M;
#pragma unroll
            for (int m = 0; m < M; ++m) {
              if (p * M + m < D) {
                d0[m] = v[m];
                if (t0 + 1 < N) d1[m] = v[M + m];
              }
            }
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) lds_store_relaxed(&s_ready[g], c0 + kStCH < N ? c0 + kStCH : N);
      }
      return;
    }
  } else if (wave == kStCW) {  // ---- loader: dw rows of steps t -> ring slot t % RS ----
    const int64_t rows_live = (a.B - row0) < TPW ? (a.B - row0) : TPW;
    const uint32_t bytes = (uint32_t)(rows_live * D * (int64_t)sizeof(T));
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)s_ring;
    const char* base = (const char*)(a.dw + row0 * D);
    const int64_t step_bytes = a.B * D * (int64_t)sizeof(T);
    // A whole chunk of a full workgroup goes through st_issue_chunk: no bounds predicate, source
    // and slot addresses advanced by step_bytes and SLOT_LDS per step.  Every step reads exactly
    // the SLOT bytes of its rows: all lanes in the pieces before the last, kLastLanes lanes in
    // the last, and the chunk's last pieces are issued together under one exec change (the
    // counted wait counts instructions, in any order).  A partial workgroup and the horizon's
    // last, clamped chunk take the predicated path below, which also issues PIECES instructions
    // per step.
    // Only the first kStCheapChunks chunks go that way: they are what the compute waves wait for
    // at start-up.  From then on the loader is chunks ahead, and issuing a chunk in a burst (a
    // third of the cycles) made the compute waves' steady state slower by more than the start-up
    // gained, so later chunks keep the slower, evenly spaced issue.
    const bool cheap = rows_live == TPW;
    const int64_t chunk_bytes = step_bytes * kStCH;
    uint64_t csrc = (uint64_t)(uintptr_t)base + (uint32_t)lane * 16u;  // this lane's 16 bytes of the chunk's first step
    uint32_t cslot = lds0;                                             // the chunk's first slot: lds0 + (c0 % RS) * SLOT_LDS
    for (int c0 = 0; c0 < N; c0 += kStCH) {
      // the slots of this chunk were last read at steps c0 + s - RS: wait for every consumer
      const int need = c0 + kStCH - RS;
      if (need > 0) st_wait_consumed(s_done, need);
      asm volatile("" ::: "memory");
#if DPAC_ST_TRACE
      ST_MARK(ST_CHUNK(16, c0));
#endif
      if (cheap && c0 < kStCheapChunks * kStCH && c0 + kStCH <= N) {
        st_issue_chunk<PIECES - 1, 0, SLOT_LDS>(csrc, cslot, step_bytes);
        if (lane < PL::kLastLanes) st_issue_chunk<1, (PIECES - 1) * 1024, SLOT_LDS>(csrc, cslot, step_bytes);
        csrc += chunk_bytes;
        cslot = cslot + kStCH * SLOT_LDS == lds0 + RS * SLOT_LDS ? lds0 : cslot + kStCH * SLOT_LDS;
      } else {
#pragma unroll
        for (int s = 0; s < kStCH; ++s) {
          const int t = c0 + s < N ? c0 + s : N - 1;  // past the end: re-copy the last step (unused)
          const char* src = base + t * step_bytes;
          const uint32_t slot = lds0 + (uint32_t)((t % RS) * SLOT_LDS);
#pragma unroll
          for (int k = 0; k < PIECES; ++k) {
            const uint32_t off = (uint32_t)((k * 64 + lane) * 16);
            const char* gp = src + (off < bytes ? off : 0u);  // lane 0 past the rows re-reads row 0
            const uint32_t m0 = __builtin_amdgcn_readfirstlane(slot + (uint32_t)(k * 1024));
            // lanes past the rows write nothing (the zero pad stays zero); lane 0 always issues,
            // so every instruction counts in vmcnt (it lands at k*1024, never on the pad)
            if (off < bytes || lane == 0) {
              int keep;
              asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                           : "=&s"(keep) : "v"(gp), "s"(m0) : "memory");
            }
          }
        }
      }
#if DPAC_ST_TRACE
      ST_MARK(ST_CHUNK(48, c0));
#endif
      // the previous chunk has landed once only this chunk's copies are outstanding
      if (c0 > 0) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kStCH * PIECES) : "memory");
        if (lane == 0) lds_store_relaxed(&s_ready[0], c0);
#if DPAC_ST_TRACE
        ST_MARK(ST_CHUNK(80, c0));
#endif
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) lds_store_relaxed(&s_ready[0], N);
    ST_MARK(4);
    ST_PUT(6, st_realtime());
    return;
  }

  // ---- compute wavefronts: k_rollout's time loop with dw from the ring ----
  const LaneCoord<P> lc(a.B, lane, row0 + wave * (64 / P));
  const int gl = wave * (64 / P) + lane / P;  // trajectory within the workgroup
  const Own<D, P> own(lc.p);
  const Own<E::CDIM, P> ownu(lc.p);
  const BufSlab<T, D, P> sx(own, lc.b, lc.live);
  const BufSlab<T, E::CDIM, P> su(ownu, lc.b, lc.live);
  const uint32_t slab = (uint32_t)(a.B * D * sizeof(T));
  const uint32_t slab_u = (uint32_t)(a.B * E::CDIM * sizeof(T));
  const uint32_t row_bytes = (uint32_t)(N * sizeof(T));
  const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(a.x, slab * (uint32_t)(N + 1));
  const __amdgpu_buffer_rsrc_t rs_u = make_rsrc(a.u, WANT_U ? slab_u * (uint32_t)N : 0u);
  const __amdgpu_buffer_rsrc_t rs_dt = make_rsrc(a.dt, (uint32_t)a.B * row_bytes);
  const __amdgpu_buffer_rsrc_t rs_cf = make_rsrc(a.coef, (uint32_t)a.B * row_bytes);
  const T* ring = reinterpret_cast<const T*>(s_ring);
  const int lds_e = gl * D + lc.p * M;  // element offset of this lane's components in a slot
  // full-or-empty lanes: one vector LDS read per step, empty lanes aimed at the zero pad
  constexpr bool kVecRead = Own<D, P>::kFull && (M * sizeof(T) == 8 || M * sizeof(T) == 16);
  const uint32_t lane_off = own.active() ? (uint32_t)(lds_e * (int)sizeof(T)) : (uint32_t)PL::PADOFF;
  T keep = 0;
  auto flush = [&](int t_last, int count) {
    const uint32_t off = (lc.live && lc.p < count)
                             ? (uint32_t)((lc.b * N + t_last - lc.p) * (int64_t)sizeof(T)) : kOOB;
    buf_store_scalar<T>(rs_dt, off, fabs(keep));
    buf_store_scalar<T>(rs_cf, off, keep > T(0) ? T(1) : T(0));
  };
  T x[M];
  sx.load(make_rsrc(a.x0, slab), x);
  sx.store(rs_x, x);
  T r = TR::kRadius ? dsqrt(Lanes<P>::sum(sumsq(x))) : T(0);
  Flags fl = SCHEME == DPAC_SCHEME_ADAPTIVE ? region(r, c) : Flags{true, false};
  T disc = 1, y = 0;
  // the own step's state (see `step` below): the candidate chain xc / rc, the radius Ra the
  // chain measures against (R while the trajectory runs, -inf once it is dead), whether it runs
  // (naive scheme), the step's dt and sqrt(dt), and sqrt(dt0) as the hardware computes it
  T xc[M], rc = r;
#pragma unroll
  for (int m = 0; m < M; ++m) xc[m] = x[m];
  T Ra = fl.alive ? c.R : -std::numeric_limits<T>::infinity();
  bool alive = fl.alive;
  const T sq0 = SCHEME == DPAC_SCHEME_ADAPTIVE ? dsqrt(c.dt0) : c.sqrt_dt0;
  T dt = c.dt0, sq = sq0;
  if constexpr (SCHEME == DPAC_SCHEME_ADAPTIVE) {
    dt = adaptive_dt_raw(fl.layer, r, c);
    dt = fl.layer ? fmax(dt, c.dt_min) : dt;
    sq = dsqrt(dt);
  }
  ST_MARK(2);  // the clock read waits for nothing of x0; r's DPP sum above did
  // slot_bytes: (t % RS) * SLOT_LDS, formed once per chunk plus a compile-time step offset
  auto read_dw_at = [&](int t, uint32_t slot_bytes, T (&dwv)[M]) {  // components past d read 0
    if constexpr (kVecRead) {
      typedef T vec __attribute__((ext_vector_type(M)));
      const vec v = *reinterpret_cast<const vec*>(s_ring + slot_bytes + lane_off);
#pragma unroll
      for (int m = 0; m < M; ++m) dwv[m] = v[m];
    } else {
      const T* slot = ring + (t % RS) * (SLOT_LDS / (int)sizeof(T)) + lds_e;
#pragma unroll
      for (int m = 0; m < M; ++m) dwv[m] = own.valid(m) ? slot[m] : T(0);
    }
  };
  auto read_dw = [&](int t, T (&dwv)[M]) { read_dw_at(t, (uint32_t)((t % RS) * SLOT_LDS), dwv); };
  // The staged kernel's own step: Transition's arithmetic, bit for bit, laid out
  // for a lone wavefront, whose time per step is the length of its dependent chain (the clock
  // trace, DESIGN section 4: 233 cycles for 36 instructions).  What the chain keeps is
  //   sum -> sqrt -> R - rt -> (b b) / den -> max -> sqrt -> select -> (sigma dw) sqrt(dt) -> fma -> add -> sumsq;
  //  * the candidate state is the chain's state: xc = xt, unselected.  While the trajectory runs,
  //    x == xc bit for bit; once a step is rejected the trajectory is dead for good, Ra = -inf
  //    makes every later b = Ra - rt fail both compares, and whatever xc drifts to (inf and NaN
  //    included) reaches no output: x, r, u and the cost are taken from the selected state, dt and
  //    coef from the compares;
  //  * the next step's dt comes from the candidate radius: dt' = layer' ? max((b b) / den, dt_min)
  //    : dt0 with b = R - rt.  layer' implies coef, so whenever the boundary-layer value is used
  //    r' == rt and b is the b of Transition's second subtraction; a dead trajectory steps with dt0;
  //  * sqrt(dt') is selected from sqrt(boundary-layer dt) and sqrt(dt0), both the hardware square
  //    root of the value Transition would take it of, so the root leaves the compare's shadow.
  // The selects of x and r, the stores and the dt / coef shift register hang off the chain.
  auto step = [&](int t, const T (&dwv)[M], auto phase) {
    T uc[MC], f[M], s[M], xt[M];
    eq.u_true(xc, rc, uc);
    eq.drift(xc, uc, rc, f);
    eq.sigma(xc, uc, s);
#pragma unroll
    for (int m = 0; m < M; ++m) xt[m] = xc[m] + fma(f[m], dt, (s[m] * dwv[m]) * sq);  // as Transition
    const T St = Lanes<P>::sum(sumsq(xt));
    T u[MC];  // the control at the selected state (frozen once dead): an output and the cost's input
    if constexpr (COST || WANT_U) eq.u_true(x, r, u);
    bool coef;
    T rt = T(0), dtn = dt, sqn = sq;
    if constexpr (SCHEME == DPAC_SCHEME_ADAPTIVE) {
      rt = dsqrt(St);
      const T b = Ra - rt;  // R - rt while the trajectory runs: region(rt) and adaptive_dt_raw(rt) share it
      const bool inner = b - c.c_layer > T(0);
      coef = b > T(0);
      const T dtb = fmax((b * b) * c.inv_den, c.dt_min);
      const T sqb = dsqrt(dtb);
      const bool layer = coef && !inner;
      dtn = layer ? dtb : c.dt0;
      sqn = layer ? sqb : sq0;
      Ra = coef ? Ra : -std::numeric_limits<T>::infinity();
    } else {
      if constexpr (E::kNeedsNorm) rt = dsqrt(St);
      coef = alive && !(St - c.R2 >= T(0));
      alive = coef;
    }
    if constexpr (COST) {
      const T cf = coef ? T(1) : T(0);
      const T w = eq.w_finish(Lanes<P>::sum(eq.w_part(x, u)));
      y += cost_increment(a.cost_order, w, cf, dt, disc);
      disc = disc * disc_factor(dt, cf, c);
    }
    const T kv = coef ? dt : -dt;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      x[m] = coef ? xt[m] : x[m];
      xc[m] = xt[m];
    }
    if constexpr (E::kNeedsNorm) {
      r = coef ? rt : r;
      rc = rt;
    }
    dt = dtn;
    sq = sqn;
    sx.template store<DPAC_ROLLOUT_X_AUX>(rs_x, x, (uint32_t)(t + 1) * slab);
    if constexpr (WANT_U) su.store(rs_u, u, (uint32_t)t * slab_u);
    constexpr int PH = decltype(phase)::value;
    keep = group_shift_in<P>(keep, kv, lc.p == 0);
    if constexpr (PH >= 0) {
      if constexpr (PH % F == F - 1) flush(t, F);
    } else if ((t & (F - 1)) == F - 1) {
      flush(t, F);
    }
  };
  // A chunk's dw in registers (kChunkRegs): all kStCH steps' ring reads are issued together at
  // the chunk's top and the compiler places counted lgkmcnt waits in front of the steps that use
  // them, so a step waits for LDS only where its own read has not returned; the last N % kStCH
  // steps run as unrolled pieces.  A chunk is kStCH M dwords per lane in float, twice that in
  // double.  Which instantiations read this way is decided by the compiler's resource remarks
  // (profiles/staged_prefetch_resources_*.txt) and by measurement:
  //  * not with the cost outputs: given a chunk in registers the scheduler fills the register
  //    budget of these larger bodies and spills (float generator variant: 25 VGPRs; double: 5 to 30);
  //  * not the generator variant: its compute wave shares the SIMD with three generator
  //    wavefronts, which hide the LDS latency already (128 VGPRs, 16 wavefronts per workgroup);
  //  * the others (dw from memory, one compute wavefront per SIMD, 256 VGPRs) do.
  // The rest read each step's dw one step ahead of its use and run a rolled remainder loop.
  constexpr bool kChunkRegs = kStPrefetch != 0 && !COST && GEN == 0;
  for (int c0 = 0; c0 < N; c0 += kStCH) {
    const int want = c0 + kStCH < N ? c0 + kStCH : N;
#if DPAC_ST_TRACE
    const uint32_t st_poll0 = st_clock();
#endif
    st_wait_published<NREADY>(s_ready, want);  // every producer has published the chunk
    asm volatile("" ::: "memory");
#if DPAC_ST_TRACE
    {
      const uint32_t st_now = st_clock();
      ST_PUT(ST_CHUNK(16, c0), st_now);
      ST_PUT(ST_CHUNK(80, c0), st_now - st_poll0);
      if (c0 == 0) ST_PUT(3, st_now);
    }
#endif
    if constexpr (kChunkRegs) {
      // steps t0 .. t0 + count - 1 (count <= kStCH, inside one chunk, whose slots are contiguous
      // in the ring: RS is a multiple of kStCH): all reads, then the steps at compile-time phases
      auto steps = [&](int t0, auto count) {
        constexpr int CNT = decltype(count)::value;
        const uint32_t cb = (uint32_t)__builtin_amdgcn_readfirstlane((t0 % RS) * SLOT_LDS);
        T dwv[CNT][M];
#pragma unroll
        for (int q = 0; q < CNT; ++q) read_dw_at(t0 + q, cb + (uint32_t)(q * SLOT_LDS), dwv[q]);
        auto one = [&](auto sidx) {
          constexpr int S = decltype(sidx)::value;
          step(t0 + S, dwv[S], Phase<S>{});
        };
        unroll_phases(one, std::make_integer_sequence<int, CNT>{});
      };
      if (c0 + kStCH <= N) {
        steps(c0, Phase<kStCH>{});
      } else {
        // The remainder as unrolled pieces of 8, 4, 2 and 1 steps.  A piece of L steps starts at
        // a multiple of 2 L past c0 and the flush period F is a power of two: for F <= 2 L the
        // flush phase of step s of the piece is s % F, and for F > 2 L no step of the piece
        // flushes and s < F - 1, so Phase<s> is right either way.
        static_assert(kStCH == 16, "remainder pieces of 8, 4, 2 and 1 steps");
        int t0 = c0;
        auto piece = [&](auto len) {
          if ((N - c0) & decltype(len)::value) {
            steps(t0, len);
            t0 += decltype(len)::value;
          }
        };
        piece(Phase<8>{});
        piece(Phase<4>{});
        piece(Phase<2>{});
        piece(Phase<1>{});
      }
    } else if (c0 + kStCH <= N) {
      // RS is a multiple of kStCH: the chunk's slots are contiguous from cb
      const uint32_t cb = (uint32_t)__builtin_amdgcn_readfirstlane((c0 % RS) * SLOT_LDS);
      constexpr int PD = 1;  // steps of dw in registers ahead of use
      T nxt[PD][M];
#pragma unroll
      for (int q = 0; q < PD; ++q) read_dw_at(c0 + q, cb + (uint32_t)(q * SLOT_LDS), nxt[q]);
      auto one = [&](auto sidx) {
        constexpr int S = decltype(sidx)::value;
        T cur[M];
#pragma unroll
        for (int m = 0; m < M; ++m) cur[m] = nxt[S % PD][m];
        if constexpr (S + PD < kStCH) read_dw_at(c0 + S + PD, cb + (uint32_t)((S + PD) * SLOT_LDS), nxt[S % PD]);
        step(c0 + S, cur, Phase<S>{});
      };
      unroll_phases(one, std::make_integer_sequence<int, kStCH>{});
    } else {
      for (int t = c0; t < N; ++t) {
        T cur[M];
        read_dw(t, cur);
        step(t, cur, Phase<-1>{});
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) lds_store_relaxed(&s_done[wave], want);
#if DPAC_ST_TRACE
    ST_MARK(ST_CHUNK(48, c0));
#endif
  }
  const int rem = N & (F - 1);
  if (rem) flush(N - 1, rem);
#if DPAC_ST_TRACE
  ST_MARK(4);  // every store issued (not yet acknowledged)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ST_MARK(7);  // every store acknowledged
  ST_PUT(6, st_realtime());
#endif
  if constexpr (COST) {
    if (lc.live && lc.p == 0) {
      a.y[lc.b] = y;
      a.disc[lc.b] = disc;
    }
  }
}
