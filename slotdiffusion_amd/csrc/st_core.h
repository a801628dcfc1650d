// Tile toolkit of the fused token-row blocks -- st_fused.hip (SpatialTransformer block, bf16 inference), st_train.hip (its
// training forward / backward twins), rollout_layer.hip (SlotFormer rollout layer): a workgroup owns 64 / 32 token rows,
// eight symmetric waves, per-wave weight rings over LDS-DMA.  See st_fused.hip for the layout description.  One copy of
//   geometry (StGeom), the ring (StRing, st_ring_setup / _prime / _init), the lane constants (st_frag_addrs),
//   one K tile of the weights-as-A GEMM (st_gemm_step) with the LayerNorm-fold statistics (st_ln_stats), the hand-off
//   barrier (ST_BARRIER) and the counted wait (ST_WAIT_UNITS),
//   the row copies into the swizzled operand buffer (st_rows_to_y, st_load_rows_to_y) and out (st_store_rows),
//   the residual prefetch and its epilogue (st_load_residual, st_add_bias_residual),
//   the self-attention stage of the phase-B kernels (st_self_attention, st_attn_out_to_y).
// Everything is __forceinline__ template code selected by compile-time parameters only, and the header is compiled per
// translation unit: each file keeps its own code generation (csrc/build.py: -fno-slp-vectorize on two of the three).
// What differs in substance stays with its kernel: the feed-forward chunk loops, the folded / explicit cross-attention,
// the GroupNorm prologues.  st_fused.hip's phase A (st_block_a_kernel) keeps its own copy of the set-up, the proj_in
// epilogue and the q | k | v passes: that file is built WITH the SLP vectoriser, and the instruction schedule the shared
// forms gave its q | k | v epilogue hit the packed-fp32 hazard of st_train.hip's build note.
#pragma once
#include "common.h"
#include <type_traits>

namespace {

typedef __attribute__((address_space(3))) char lds_char;
typedef short st_s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef short st_s16x8 __attribute__((ext_vector_type(8)));
#define ST_LDS_V4(p) ((__attribute__((address_space(3))) st_s16x4*)(p))

constexpr int ST_UNIT = 2048;          // 16 weight rows x 64 k x 2 B
constexpr int ST_KP = 80, ST_VP = 64;  // attention staging: K row pitch (64 B + pad), V row pitch

__device__ __forceinline__ unsigned st_pack2(float lo, float hi) { return f32x2_to_bf16x2(lo, hi); }

// Epilogue vectors (biases, LayerNorm-fold column sums): lane group lg's four of the 16 floats of a slice.
__device__ __forceinline__ f32x4 st_vec4(const float* base16, int lg) {
  return *reinterpret_cast<const f32x4*>(base16 + 4 * lg);
}

__device__ __forceinline__ int st_xcd_id(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

template <int C, int TT>
struct StGeom {
  static constexpr int ROWS = 16 * TT;          // token rows of a workgroup (TT 16-row tiles: 64, or 32 for small grids)
  static constexpr int NSL = C / 128;          // 16-column slices per wave of an N = C GEMM
  static constexpr int KT = C / 64;            // 64-wide K tiles of a K = C GEMM
  static constexpr int HEADS = C / 32;
  static constexpr int R = HEADS * 8;          // head-expanded slot rows of the folded cross-attention
  static constexpr int RP = 128;               // ... padded (N of the score GEMM, K of the output GEMM)
  static constexpr int NHC = C / 32;           // hidden chunks of 128 (4C hidden units)
  static constexpr int PITCH = C * 2;          // row pitch of the activation operand buffer
  static constexpr int Y_BYTES = ROWS * PITCH;
  static constexpr int G_BYTES = ROWS * 256;   // one GEGLU chunk / the cross-attention probabilities
  static constexpr int FREE2 = 160 * 1024 - Y_BYTES - 2 * G_BYTES;     // what two chunk buffers leave for the rings
  // ring depth in units per wave: as deep as the LDS allows next to two chunk buffers (8 at most), 6 otherwise
  static constexpr int D = FREE2 >= 8 * 8 * ST_UNIT ? 8 : (FREE2 >= 8 * 7 * ST_UNIT ? 7 : 6);
  static constexpr int GBUF = (Y_BYTES + 2 * G_BYTES + 8 * D * ST_UNIT <= 160 * 1024) ? 2 : 1;
  static constexpr int Y_OFF = 0;
  static constexpr int RING_OFF = Y_BYTES + GBUF * G_BYTES;
  static constexpr int SMEM_GEMM = Y_BYTES + GBUF * G_BYTES + 8 * D * ST_UNIT;
  // units per wave
  static constexpr int UA = KT * NSL + 3 * KT * NSL;                       // phase A: proj_in, q, k, v
  static constexpr int UB1 = KT * NSL;                                     // phase B shared, part 1: to_out
  static constexpr int UIMG = KT * 1 + 2 * NSL;                            // per image: scores, cross output
  static constexpr int UB2 = KT * NSL + NHC * (KT * 2 + 2 * NSL);          // part 2: x2 @ Wpo, FF chunks
};

// ---------------------------------------------------------------------------------------------------------
// per-wave weight stream + ring (all state wave-uniform)
// ---------------------------------------------------------------------------------------------------------
template <int D>
struct StRing {
  __amdgpu_buffer_rsrc_t rs_sh, rs_img;
  int g_iss;            // next unit to fetch
  int n1, n_img, total; // shared part 1 | per-image | shared part 2 (unit counts)
  int pos_iss;          // ring position of unit g_iss
  int pos_con;          // ring position of the next unit to consume
  lds_char* ring;       // this wave's ring
  int voff;             // lane * 16
  int jump_at = 1 << 30, jump = 0;   // shared-stream units from `jump_at` on lie `jump` units further (a workgroup that skips
                                     // part of the stream: the feed-forward split of st_fused.hip's phase B)

  __device__ __forceinline__ void issue_one() {
    int g = g_iss < total ? g_iss : total - 1;          // (steps past the end re-fetch the last unit: static vmcnt)
    lds_char* dst = ring + pos_iss * ST_UNIT;
    if (g >= n1 && g < n1 + n_img) {
      const int so = (g - n1) * ST_UNIT;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_img, (lds_void*)dst, 16, voff, so, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_img, (lds_void*)(dst + 1024), 16, voff, so + 1024, 0, 0);
    } else {
      int gs = g >= n1 ? g - n_img : g;
      if (gs >= jump_at) gs += jump;
      const int so = gs * ST_UNIT;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_sh, (lds_void*)dst, 16, voff, so, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_sh, (lds_void*)(dst + 1024), 16, voff, so + 1024, 0, 0);
    }
    ++g_iss;
    if (++pos_iss == D) pos_iss = 0;
  }
};

// EXTRA = global stores of the epilogue in front of this step: they are younger than every DMA in flight and
// vmcnt retires in issue order, so they simply stay outstanding on top of the D - n units (a vmcnt(0) here waited
// for the stores' round trip: ~2 k cycles per q / k / v pass of phase A).  -DST_DRAIN: vmcnt(0) everywhere (experiment).
#if defined(ST_DRAIN)
#define ST_WAIT_UNITS(D_, n_, extra_) asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define ST_WAIT_UNITS(D_, n_, extra_) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * ((D_) - (n_)) + (extra_)) : "memory")
#endif
// Workgroup barrier that leaves the DMA queue alone: `__syncthreads()` carries a fence that waits vmcnt(0) while
// LDS-DMA is in flight (it is a pending LDS write); LDS stores / reads of this wave are retired explicitly.
#ifdef ST_TIMELINE      // experiment: s_memtime of wave 0 at the phase boundaries of phase B -> p.gn_gamma[wg][8] (u64)
#define ST_STAMP(i) do { if (threadIdx.x == 0) ((unsigned long long*)p.gn_gamma)[blockIdx.x * 16 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define ST_STAMP(i)
#endif
#ifdef ST_TIMELINE
#define ST_TL_DECL unsigned long long tl_t = 0, tl_a[4] = {0, 0, 0, 0};
#define ST_TL_BEGIN tl_t = __builtin_amdgcn_s_memtime();
#define ST_TL_LAP(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); tl_a[i] += n_ - tl_t; tl_t = n_; } while (0)
#define ST_TL_FLUSH do { if (threadIdx.x == 0) for (int i_ = 0; i_ < 4; ++i_) ((unsigned long long*)p.gn_gamma)[blockIdx.x * 16 + 12 + i_] = tl_a[i_]; } while (0)
#else
#define ST_TL_DECL
#define ST_TL_BEGIN
#define ST_TL_LAP(i)
#define ST_TL_FLUSH
#endif
#ifdef ST_TIMELINE
#define STA_STAMP(i) do { if (threadIdx.x == 0) ((unsigned long long*)p.vec_img)[blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define STA_STAMP(i)
#endif
#define ST_BARRIER()                                         \
  do {                                                       \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       \
    __builtin_amdgcn_s_barrier();                            \
    asm volatile("" ::: "memory");                           \
  } while (0)

// One K tile (64 k = two MFMA k-steps) of a GEMM whose wave block is NU 16-column slices x 64 rows:
// acc[s][tt] += W_unit(s) . act[rows 16 tt ..][k tile kt].  STATS: LayerNorm-fold row sums from the
// activation fragments (lane: row lane & 15 of tile tt, its 8 k of each 32).
template <int D, int NU, bool STATS, int EXTRA = 0, int TT = 4>
__device__ __forceinline__ void st_gemm_step(StRing<D>& rg, const lds_char* act, const int (&yaddr)[4], int kt,
                                             int tt_stride, const int (&woff)[2], f32x4 (&acc)[NU][TT],
                                             float (&sx)[TT], float (&sxx)[TT]) {
#ifdef ST_STEP_BARRIER       // experiment: the eight waves in lock step (the default lets them run free)
  __builtin_amdgcn_s_barrier();
#endif
  ST_WAIT_UNITS(D, NU, EXTRA);
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int kk = kt * 2 + ks;
    bf16x8 b[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
      b[tt] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const __attribute__((address_space(3))) u32x4*>(
                                             act + yaddr[kk & 3] + tt * tt_stride + (kk >> 2) * 256));
    if constexpr (STATS) {
      const sdmi_bf16x2 ones = __builtin_bit_cast(sdmi_bf16x2, 0x3F803F80u);
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const sdmi_bf16x2 v0 = {b[tt][0], b[tt][1]}, v1 = {b[tt][2], b[tt][3]}, v2 = {b[tt][4], b[tt][5]},
                          v3 = {b[tt][6], b[tt][7]};
        sx[tt] = __builtin_amdgcn_fdot2_f32_bf16(v0, ones, sx[tt], false);
        sxx[tt] = __builtin_amdgcn_fdot2_f32_bf16(v0, v0, sxx[tt], false);
        sx[tt] = __builtin_amdgcn_fdot2_f32_bf16(v1, ones, sx[tt], false);
        sxx[tt] = __builtin_amdgcn_fdot2_f32_bf16(v1, v1, sxx[tt], false);
        sx[tt] = __builtin_amdgcn_fdot2_f32_bf16(v2, ones, sx[tt], false);
        sxx[tt] = __builtin_amdgcn_fdot2_f32_bf16(v2, v2, sxx[tt], false);
        sx[tt] = __builtin_amdgcn_fdot2_f32_bf16(v3, ones, sx[tt], false);
        sxx[tt] = __builtin_amdgcn_fdot2_f32_bf16(v3, v3, sxx[tt], false);
      }
    }
#pragma unroll
    for (int s = 0; s < NU; ++s) {
      int pos = rg.pos_con + s;
      if (pos >= D) pos -= D;
      const bf16x8 a = __builtin_bit_cast(
          bf16x8, *reinterpret_cast<const __attribute__((address_space(3))) u32x4*>(rg.ring + pos * ST_UNIT + woff[ks]));
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) acc[s][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[tt], acc[s][tt], 0, 0, 0);
    }
  }
  // The units just multiplied are free: refill their ring positions -- but only once this step's fragment reads have
  // RETURNED.  To the instruction scheduler a `buffer_load ... lds` is a load, not an LDS store: without the wait and
  // the scheduling barrier it moves the refill in front of the ds_reads of the very slot it overwrites, and when the
  // stream hits in L2 the DMA wins the race now and then: with free-running waves 2 - 6 % of the 16-column output
  // slices were wrong (exactly one 1 KB piece of one K tile each; tools/exp/st_forensic.py, st_stress.py), in lock step
  // still ~1e-3.  Neither vmcnt(0) per step, a barrier behind the wait, nor waiting a step ahead cured it; this does:
  // 0 / 102400 slices over 40 runs, bitwise repeatable.
#ifndef ST_UNSAFE_REFILL
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
#endif
  rg.pos_con += NU;
  if (rg.pos_con >= D) rg.pos_con -= D;
#pragma unroll
  for (int s = 0; s < NU; ++s) rg.issue_one();
}

// row statistics of the LayerNorm fold: after all K tiles, fold the four 8-k lane groups of a row
template <int TT>
__device__ __forceinline__ void st_ln_stats(float (&sx)[TT], float (&sxx)[TT], float inv_k, float eps, float (&mean)[TT],
                                            float (&rstd)[TT]) {
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) {
    float a = sx[tt], b = sxx[tt];
    a += __shfl_xor(a, 16, 64);
    b += __shfl_xor(b, 16, 64);
    a += __shfl_xor(a, 32, 64);
    b += __shfl_xor(b, 32, 64);
    mean[tt] = a * inv_k;
    rstd[tt] = rsqrtf(fmaxf(b * inv_k - mean[tt] * mean[tt], 0.f) + eps);
  }
}

// ---------------------------------------------------------------------------------------------------------
// ring set-up, lane constants
// ---------------------------------------------------------------------------------------------------------
// One stream of `units` units per wave, nothing in flight yet: a kernel with a per-image stream or a workgroup that
// skips part of the stream adjusts rs_img / n1 / n_img / total / jump_at / jump before st_ring_prime.
template <int D>
__device__ __forceinline__ void st_ring_setup(StRing<D>& rg, const void* stream, int units, lds_char* ring, int lane, int w) {
  rg.rs_sh = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)stream + (long long)w * units * ST_UNIT), 0,
                                               units * ST_UNIT, 0x00020000);
  rg.rs_img = rg.rs_sh;
  rg.g_iss = 0; rg.n1 = units; rg.n_img = 0; rg.total = units; rg.pos_iss = 0; rg.pos_con = 0;
  rg.ring = ring + w * D * ST_UNIT;
  rg.voff = lane * 16;
}
template <int D>
__device__ __forceinline__ void st_ring_prime(StRing<D>& rg) {
#pragma unroll
  for (int i = 0; i < D; ++i) rg.issue_one();
}
template <int D>
__device__ __forceinline__ void st_ring_init(StRing<D>& rg, const void* stream, int units, lds_char* ring, int lane, int w) {
  st_ring_setup<D>(rg, stream, units, ring, lane, w);
  st_ring_prime<D>(rg);
}

// Lane constants of the GEMM core: fragment offsets into the operand buffer Y (row pitch PITCH), into a 256-byte-pitch
// chunk buffer, and into a weight unit.
template <int PITCH>
__device__ __forceinline__ void st_frag_addrs(int l15, int lg, int (&yaddr)[4], int (&gaddr)[4], int (&woff)[2]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int sw = (((4 * j + lg) ^ l15) & 15) * 16;
    yaddr[j] = l15 * PITCH + sw;
    gaddr[j] = l15 * 256 + sw;
  }
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) woff[ks] = l15 * 128 + (((4 * ks + lg) ^ ((l15 >> 1) & 7)) * 16);
}
template <int PITCH>
__device__ __forceinline__ void st_frag_addrs(int l15, int lg, int (&yaddr)[4], int (&woff)[2]) {
  int gaddr[4];
  st_frag_addrs<PITCH>(l15, lg, yaddr, gaddr, woff);
}

// ---------------------------------------------------------------------------------------------------------
// rows <-> operand buffer Y (XOR-swizzled 16-byte chunks: chunk c of row r lies at (c & ~15) | ((c ^ r) & 15))
// ---------------------------------------------------------------------------------------------------------
// fp32 rows held across the workgroup (lane: row 16 tt + l15, columns (w NSL + s) 16 + 4 lg + j) -> bf16 in Y (+ optional
// global copy).  MASKED (rollout layer): rows lrow0 + r >= L are pad rows.  A pad row's values may be anything (inf, NaN):
// its copy is zero, so the LayerNorm statistics and the hidden chunk of that row stay finite.
template <int C, int TT, int NSL, bool GLOBAL, bool MASKED = false>
__device__ __forceinline__ void st_rows_to_y(const f32x4 (&x)[NSL][TT], lds_char* Y, bf16_t* gout, int w, int l15, int lg,
                                             int lrow0 = 0, int L = 0) {
  constexpr int PITCH = C * 2;
#pragma unroll
  for (int s = 0; s < NSL; ++s) {
    const int n0 = (w * NSL + s) * 16 + 4 * lg;
    const int c = n0 >> 3;
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const int r = tt * 16 + l15;
      const int phys = (c & ~15) | ((c ^ r) & 15);
      uint2 o;
      if constexpr (MASKED) {
        const bool real = lrow0 + r < L;
        o.x = real ? st_pack2(x[s][tt][0], x[s][tt][1]) : 0u;
        o.y = real ? st_pack2(x[s][tt][2], x[s][tt][3]) : 0u;
      } else {
        o.x = st_pack2(x[s][tt][0], x[s][tt][1]);
        o.y = st_pack2(x[s][tt][2], x[s][tt][3]);
      }
      *reinterpret_cast<__attribute__((address_space(3))) u32x2*>(Y + r * PITCH + phys * 16 + (lg & 1) * 8) = u32x2{o.x, o.y};
      if constexpr (GLOBAL) *reinterpret_cast<uint2*>(gout + (long long)r * C + n0) = o;
    }
  }
}

template <int C, int TT, int NSL>
__device__ __forceinline__ void st_store_rows(const f32x4 (&x)[NSL][TT], bf16_t* gout, int ld, int w, int l15, int lg) {
#pragma unroll
  for (int s = 0; s < NSL; ++s) {
    const int n0 = (w * NSL + s) * 16 + 4 * lg;
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      uint2 o;
      o.x = st_pack2(x[s][tt][0], x[s][tt][1]);
      o.y = st_pack2(x[s][tt][2], x[s][tt][3]);
      *reinterpret_cast<uint2*>(gout + (long long)(tt * 16 + l15) * ld + n0) = o;
    }
  }
}

// ROWS x C bf16 rows from global memory (row stride ld) into Y: all 512 threads, 16-byte vectors, the loads of all
// passes in flight before the first LDS store
template <int C, int ROWS>
__device__ __forceinline__ void st_load_rows_to_y(const bf16_t* src, int ld, lds_char* Y, int tid) {
  constexpr int VPR = C / 8, PITCH = 2 * C;     // vectors per row
  static_assert((ROWS * VPR) % 512 == 0, "whole passes");
  u32x4 v[ROWS * VPR / 512];
#pragma unroll
  for (int it = 0; it < ROWS * VPR / 512; ++it) {
    const int i = tid + it * 512, r = i / VPR, vc = i - r * VPR;
    v[it] = *reinterpret_cast<const u32x4*>(src + (long long)r * ld + vc * 8);
  }
#pragma unroll
  for (int it = 0; it < ROWS * VPR / 512; ++it) {
    const int i = tid + it * 512, r = i / VPR, vc = i - r * VPR;
    const int phys = (vc & ~15) | ((vc ^ r) & 15);
    *reinterpret_cast<__attribute__((address_space(3))) u32x4*>(Y + r * PITCH + phys * 16) = v[it];
  }
}

// bf16 residual of an epilogue (this lane's columns of the workgroup's rows at `rows`).  An ordinary vector load issued
// behind weight DMAs makes its consumer wait for every DMA in front of it (vmcnt retires in order): the residual is
// fetched where no DMA is in flight -- WAIT: and RETIRED before the caller issues the first one.
template <int C, int TT, int NSL, bool WAIT>
__device__ __forceinline__ void st_load_residual(uint2 (&rsd)[NSL][TT], const bf16_t* rows, int w, int l15, int lg) {
#pragma unroll
  for (int s = 0; s < NSL; ++s)
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
      rsd[s][tt] = *reinterpret_cast<const uint2*>(rows + (long long)(tt * 16 + l15) * C + (w * NSL + s) * 16 + 4 * lg);
  if constexpr (WAIT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// out = acc + bias + residual (fp32; out may be acc)
template <int TT, int NSL>
__device__ __forceinline__ void st_add_bias_residual(f32x4 (&out)[NSL][TT], const f32x4 (&acc)[NSL][TT],
                                                     const f32x4 (&bias)[NSL], const uint2 (&rsd)[NSL][TT]) {
#pragma unroll
  for (int s = 0; s < NSL; ++s) {
    const f32x4 bi = bias[s];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const uint2 t2 = rsd[s][tt];
      out[s][tt][0] = acc[s][tt][0] + bi[0] + __uint_as_float(t2.x << 16);
      out[s][tt][1] = acc[s][tt][1] + bi[1] + __uint_as_float(t2.x & 0xffff0000u);
      out[s][tt][2] = acc[s][tt][2] + bi[2] + __uint_as_float(t2.y << 16);
      out[s][tt][3] = acc[s][tt][3] + bi[3] + __uint_as_float(t2.y & 0xffff0000u);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// self-attention stage of a phase-B kernel: 16 TT queries x HEADS heads over the S keys of the image / sequence
// ---------------------------------------------------------------------------------------------------------
struct StNoHook {
  __device__ __forceinline__ void operator()(int) const {}
};

// attention.hip's transposed matrix-core formulation (v_mfma_f32_32x32x16_bf16, V read through ds_read_tr16_b64): a wave
// owns 32 queries of one head, four heads per round.  64 rows: two 32-query halves x four heads per round; 32 rows:
// waves 0-3 take the four heads, waves 4-7 only stage and keep the barriers.  qkv [.][S][3C] of image / sequence `b`,
// queries lrow0 .. lrow0 + 16 TT of it; the whole dynamic LDS is the K / V staging region, and the trailing barrier
// hands it back (it becomes operand buffers + rings).  -> opack[round][8]: this lane's bf16 output of query row
// qh * 32 + ql, channels h * 32 + 8 j + 4 hh .. + 4 (st_attn_out_to_y writes them out).
// MASKED: only keys < L are real, the others leave every softmax (key 0 is real, so every 32-key block kb < nkb holds a
// finite score for every query).  LSE: the log-sum-exp of every (head, query) -> lse1 [.][HEADS][S] (training).
// hook(0) runs behind the first staging pass, hook(1) in front of the trailing barrier (timeline stamps of an
// experiment build; nothing by default).
template <int C, int TT, bool MASKED, bool LSE, class Hook = StNoHook>
__device__ __forceinline__ void st_self_attention(unsigned (&opack)[C / 128][8], const bf16_t* qkv, int b, int lrow0, int S,
                                                  int L, float attn_scale, float* lse1, lds_char* smem, int tid, int lane,
                                                  int w, Hook hook = Hook()) {
  constexpr int HEADS = C / 32;
  const long long row0 = (long long)b * S + lrow0;
  const int hs = TT == 4 ? (w >> 1) : (w & 3), qh = TT == 4 ? (w & 1) : 0;
  const bool att_active = TT == 4 || w < 4;
  const int ql = lane & 31, hh = lane >> 5;
  const bf16_t* qkv_img = qkv + (long long)b * S * 3 * C;
  const int head_bytes = S * (ST_KP + ST_VP);
  const float sc2 = attn_scale * 1.4426950408889634f;
  const int g4 = lane >> 4, t16 = lane & 15;
  // K / V of `hb` heads are staged at a time: all of them when they fit (S = 64: one staging pass for the block),
  // four otherwise; the loads of a pass are in flight together (a load per iteration behind its own wait cost a
  // memory latency each: 27 of st_block_b_kernel's 72 us at S = 256).
  const bool all_heads = HEADS * head_bytes <= 160 * 1024;
  const int hb = all_heads ? HEADS : 4;
  int nkb;                                                 // 32-key blocks that hold a real key
  if constexpr (MASKED) nkb = (L + 31) >> 5;
  else nkb = S / 32;
  bf16x8 bq[HEADS / 4][2];
#pragma unroll
  for (int ri = 0; ri < HEADS / 4; ++ri) {
    const bf16_t* qp = qkv + (row0 + qh * 32 + ql) * 3 * C + (ri * 4 + hs) * 32 + hh * 8;
    bq[ri][0] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(qp));
    bq[ri][1] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(qp + 16));
  }
  auto stage = [&](int h0, auto nb_) __attribute__((always_inline)) {
    constexpr int NB = decltype(nb_)::value;
    const int ppr = hb * 8;                              // 16-byte pieces per key row: [K of hb heads | V of hb heads]
    for (int i0 = tid; i0 < S * ppr; i0 += NB * 512) {
      u32x4 v[NB];
      int dsto[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int i = i0 + j * 512, row = i / ppr, rem = i - row * ppr;
        const int isv = rem >= hb * 4, r2 = rem - isv * hb * 4, hl = r2 >> 2, c = r2 & 3;
        v[j] = *reinterpret_cast<const u32x4*>(qkv_img + (long long)row * 3 * C + (1 + isv) * C + (h0 + hl) * 32 + c * 8);
        dsto[j] = hl * head_bytes + (isv ? S * ST_KP + row * ST_VP : row * ST_KP) + c * 16;
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) *reinterpret_cast<__attribute__((address_space(3))) u32x4*>(smem + dsto[j]) = v[j];
    }
  };
#pragma unroll
  for (int ri = 0; ri < HEADS / 4; ++ri) {
    if (ri == 0 || !all_heads) {
      if (ri) __syncthreads();
      const int per_thread = S * hb / 64;                // pieces per thread of this pass (S in {64, 128, 192, 256})
      if (per_thread % 16 == 0) stage(ri * 4, std::integral_constant<int, 16>());
      else if (per_thread % 12 == 0) stage(ri * 4, std::integral_constant<int, 12>());
      else stage(ri * 4, std::integral_constant<int, 4>());
      __syncthreads();
      if (ri == 0) hook(0);
    }
    const int hl = (all_heads ? ri * 4 : 0) + hs;
    const lds_char* Ks = smem + hl * head_bytes;
    const lds_char* Vs = Ks + S * ST_KP;
    const lds_char* kfrag = Ks + ql * ST_KP + hh * 16;
    const lds_char* vfrag = Vs + (4 * hh + (t16 >> 2)) * ST_VP + ((g4 & 1) * 16 + (t16 & 3) * 4) * 2;
    if (!att_active) continue;
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    float m = -INFINITY, lsum = 0.f;
    for (int kb = 0; kb < nkb; ++kb) {
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const u32x4 a = *reinterpret_cast<const __attribute__((address_space(3))) u32x4*>(kfrag + kb * 32 * ST_KP + ks * 32);
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), bq[ri][ks], s, 0, 0, 0);
      }
      float bmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if constexpr (MASKED) {   // accumulator r of this lane is key kb * 32 + 8 (r / 4) + 4 hh + r % 4 (query ql)
          const int key = kb * 32 + (r >> 2) * 8 + hh * 4 + (r & 3);
          s[r] = key < L ? s[r] * sc2 : -INFINITY;
        } else {
          s[r] *= sc2;
        }
        bmax = fmaxf(bmax, s[r]);
      }
      bmax = fmaxf(bmax, __shfl_xor(bmax, 32, 64));
      const float m_new = fmaxf(m, bmax);
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = __builtin_amdgcn_exp2f(s[r] - m_new);
        psum += s[r];
      }
      psum += __shfl_xor(psum, 32, 64);
      if (__builtin_amdgcn_ballot_w64(m_new > m) != 0) {
        const float alpha = __builtin_amdgcn_exp2f(m - m_new);
        lsum = lsum * alpha + psum;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= alpha;
      } else {
        lsum += psum;
      }
      m = m_new;
#pragma unroll
      for (int mm = 0; mm < 2; ++mm) {
        const u32x4 pb = {st_pack2(s[8 * mm + 0], s[8 * mm + 1]), st_pack2(s[8 * mm + 2], s[8 * mm + 3]),
                          st_pack2(s[8 * mm + 4], s[8 * mm + 5]), st_pack2(s[8 * mm + 6], s[8 * mm + 7])};
        const lds_char* vp = vfrag + (kb * 32 + 16 * mm) * ST_VP;
        const st_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(ST_LDS_V4(vp));
        const st_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(ST_LDS_V4(vp + 8 * ST_VP));
        const st_s16x8 av = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, pb), o, 0, 0, 0);
      }
    }
    const float inv = 1.f / lsum;
#pragma unroll
    for (int j = 0; j < 4; ++j) {       // d = 8 j + 4 hh + (0..3)
      opack[ri][2 * j] = st_pack2(o[4 * j] * inv, o[4 * j + 1] * inv);
      opack[ri][2 * j + 1] = st_pack2(o[4 * j + 2] * inv, o[4 * j + 3] * inv);
    }
    if constexpr (LSE) {
      if (hh == 0)
        lse1[((long long)b * HEADS + (ri * 4 + hs)) * S + lrow0 + qh * 32 + ql] = m * 0.6931471805599453f + __logf(lsum);
    }
  }
  hook(1);
  __syncthreads();                      // the staging region becomes operand buffers + rings
}

// attention output -> operand buffer Y: row qh * 32 + ql, channels h * 32 + 8 j + 4 hh .. + 4.  GLOBAL: also the bf16
// copy the training pass stores (gout: the tensor, row0: this workgroup's first row in it).
template <int C, int TT, bool GLOBAL>
__device__ __forceinline__ void st_attn_out_to_y(const unsigned (&opack)[C / 128][8], lds_char* Y, bf16_t* gout,
                                                 long long row0, int w, int lane) {
  constexpr int HEADS = C / 32, PITCH = C * 2;
  const int hs = TT == 4 ? (w >> 1) : (w & 3), qh = TT == 4 ? (w & 1) : 0;
  const int ql = lane & 31, hh = lane >> 5;
  const int r = qh * 32 + ql;
  bf16_t* grow = nullptr;
  if constexpr (GLOBAL) grow = gout + (row0 + r) * C;
  if (TT == 4 || w < 4)
#pragma unroll
    for (int rd = 0; rd < HEADS / 4; ++rd) {
      const int h = rd * 4 + hs;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = h * 4 + j;
        const int phys = (c & ~15) | ((c ^ r) & 15);
        uint2 v;
        v.x = opack[rd][2 * j];
        v.y = opack[rd][2 * j + 1];
        *reinterpret_cast<__attribute__((address_space(3))) u32x2*>(Y + r * PITCH + phys * 16 + hh * 8) = u32x2{v.x, v.y};
        if constexpr (GLOBAL) *reinterpret_cast<uint2*>(grow + h * 32 + 8 * j + 4 * hh) = v;
      }
    }
}

}  // namespace
