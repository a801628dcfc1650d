// Sequence-resident fused SlotFormer rollout layer (bf16 inference; sdmi.h: sdmi_rollout_layer).
//
// Reference: vp_vqa/models/slotformer.py:70-78 -- nn.TransformerEncoderLayer(norm_first=True, activation=relu,
// batch_first=True):  x += out_proj(MHA(LN1(x)));  x += linear2(relu(linear1(LN2(x)))).
//
// The layer is st_fused.hip's SpatialTransformer block without GroupNorm, proj_in, the folded cross-attention, GEGLU
// and proj_out; it has a biased q | k | v and a ReLU feed-forward.  Same two launches, same GEMM core (st_core.h:
// weights as the A operand of v_mfma_f32_16x16x32_bf16, per-wave weight rings over LDS-DMA with counted vmcnt,
// LayerNorm folded into the epilogue), same operand layouts:
//   phase A  x rows -> LDS;  LayerNorm-fold -> q | k | v (+ bias)                                   [B][Lp][3C]
//   phase B  self-attention of the 64 rows over the sequence's L keys -> out_proj + x -> LayerNorm-fold ->
//            linear1 + ReLU, hidden chunk (128) by hidden chunk, accumulated straight into linear2 -> + x1
// A sequence has L = history_len x num_slots real tokens in Lp rows (a multiple of the 64-row tile).  Keys >= L are
// excluded from every softmax; phase A writes zeros into the q | k | v rows >= L and phase B zeros into the output
// rows >= L, so whatever the pad rows held on entry (anything, NaN included) never reaches a real row and never
// survives a layer.
#include "st_core.h"

namespace {

constexpr int RL_C = 256;

// units per wave of the two streams (python: kern.rollout_index_a / rollout_index_b)
template <int TT>
struct RlGeom : StGeom<RL_C, TT> {
  typedef StGeom<RL_C, TT> G;
  static constexpr int UA = 3 * G::KT * G::NSL;                         // q, k, v
  static constexpr int UB0 = G::KT * G::NSL;                            // out_proj
  static constexpr int UCH = G::KT + 2 * G::NSL;                        // one hidden chunk: linear1 rows, linear2 k-chunk
};

// ---------------------------------------------------------------------------------------------------------
// phase A: LayerNorm-fold -> q | k | v
// ---------------------------------------------------------------------------------------------------------
template <int TT>
__global__ __launch_bounds__(512) void rollout_qkv_kernel(SdmiRolloutLayerArgs p) {
  typedef RlGeom<TT> G;
  constexpr int C = RL_C, ROWS = G::ROWS, NSL = G::NSL, KT = G::KT, D = G::D, PITCH = G::PITCH;
  extern __shared__ __attribute__((aligned(16))) char smem_[];
  lds_char* const smem = (lds_char*)smem_;
  lds_char* const Y = smem + G::Y_OFF;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wgs_per_seq = p.Lp / ROWS;
  const int vid = (int)blockIdx.x;
  const int b = vid / wgs_per_seq, rb = vid - b * wgs_per_seq;
  const long long row0 = (long long)b * p.Lp + rb * ROWS;      // first token row of this workgroup
  const int lrow0 = rb * ROWS;                                   // ... within its sequence

  StRing<D> rg;
  rg.rs_sh = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.wstream_a + (long long)w * G::UA * ST_UNIT), 0,
                                               G::UA * ST_UNIT, 0x00020000);
  rg.rs_img = rg.rs_sh;
  rg.g_iss = 0; rg.n1 = G::UA; rg.n_img = 0; rg.total = G::UA; rg.pos_iss = 0; rg.pos_con = 0;
  rg.ring = smem + G::RING_OFF + w * D * ST_UNIT;
  rg.voff = lane * 16;
#pragma unroll
  for (int i = 0; i < D; ++i) rg.issue_one();               // weights in flight under the activation load

  // ---- this workgroup's 64 rows into the operand buffer (XOR-swizzled 16-byte chunks, st_fused.hip's layout)
  {
    constexpr int VPR = C / 8;                    // vectors per row
    const bf16_t* xr = (const bf16_t*)p.x + row0 * C;
    static_assert((ROWS * VPR) % 512 == 0, "whole passes");
    u32x4 v[ROWS * VPR / 512];
#pragma unroll
    for (int it = 0; it < ROWS * VPR / 512; ++it) {
      const int i = tid + it * 512;
      const int r = i / VPR, vc = i - r * VPR;
      v[it] = *reinterpret_cast<const u32x4*>(xr + (long long)r * C + vc * 8);
    }
#pragma unroll
    for (int it = 0; it < ROWS * VPR / 512; ++it) {
      const int i = tid + it * 512;
      const int r = i / VPR, vc = i - r * VPR;
      const int phys = (vc & ~15) | ((vc ^ r) & 15);
      *reinterpret_cast<__attribute__((address_space(3))) u32x4*>(Y + r * PITCH + phys * 16) = v[it];
    }
  }
  ST_BARRIER();

  int yaddr[4], woff[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) yaddr[j] = l15 * PITCH + ((((4 * j + lg) ^ l15) & 15) * 16);
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) woff[ks] = l15 * 128 + (((4 * ks + lg) ^ ((l15 >> 1) & 7)) * 16);
  float sx[TT], sxx[TT], mean[TT], rstd[TT];
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) sx[tt] = sxx[tt] = 0.f;

  // (epilogue operands are fetched BEFORE the GEMM they follow: st_fused.hip's note on vmcnt order)
  f32x4 acc[NSL][TT], ev0[NSL], ev1[NSL];
#pragma unroll 1
  for (int pass = 0; pass < 3; ++pass) {
    const float* colsum = p.vec_a + pass * C;
    const float* bias = p.vec_a + 3 * C + pass * C;
#pragma unroll
    for (int s = 0; s < NSL; ++s) {
      ev0[s] = st_vec4(colsum + (w * NSL + s) * 16, lg);
      ev1[s] = st_vec4(bias + (w * NSL + s) * 16, lg);
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) acc[s][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (pass == 0) {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) st_gemm_step<D, NSL, true, 0, TT>(rg, Y, yaddr, kt, 16 * PITCH, woff, acc, sx, sxx);
      st_ln_stats<TT>(sx, sxx, 1.f / (float)C, p.ln_eps, mean, rstd);
    } else {
      // (the NSL * TT row stores of the epilogue before this pass are younger than every DMA in flight)
      st_gemm_step<D, NSL, false, NSL * TT, TT>(rg, Y, yaddr, 0, 16 * PITCH, woff, acc, sx, sxx);
#pragma unroll
      for (int kt = 1; kt < KT; ++kt) st_gemm_step<D, NSL, false, 0, TT>(rg, Y, yaddr, kt, 16 * PITCH, woff, acc, sx, sxx);
    }
    bf16_t* qkv = (bf16_t*)p.qkv + row0 * 3 * C + pass * C;
#pragma unroll
    for (int s = 0; s < NSL; ++s) {
      const int n0 = (w * NSL + s) * 16 + 4 * lg;
      const f32x4 cs = ev0[s];
      const f32x4 bi = ev1[s];
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const int r = tt * 16 + l15;
        const bool real = lrow0 + r < p.L;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = real ? rstd[tt] * (acc[s][tt][j] - mean[tt] * cs[j]) + bi[j] : 0.f;
        uint2 o;
        o.x = st_pack2(v[0], v[1]);
        o.y = st_pack2(v[2], v[3]);
        *reinterpret_cast<uint2*>(qkv + (long long)r * 3 * C + n0) = o;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no DMA may outlive the workgroup's LDS
}

// ---------------------------------------------------------------------------------------------------------
// phase B: attention -> out_proj + x -> LayerNorm-fold -> ReLU feed-forward -> + x1
// ---------------------------------------------------------------------------------------------------------
template <int TT>
__global__ __launch_bounds__(512) void rollout_tail_kernel(SdmiRolloutLayerArgs p) {
  typedef RlGeom<TT> G;
  static_assert(TT == 4, "the attention stage maps eight waves to 2 query halves x 4 heads");
  constexpr int C = RL_C, ROWS = G::ROWS, NSL = G::NSL, KT = G::KT, D = G::D, PITCH = G::PITCH, HEADS = G::HEADS;
  extern __shared__ __attribute__((aligned(16))) char smem_[];
  lds_char* const smem = (lds_char*)smem_;
  lds_char* const Y = smem + G::Y_OFF;
  lds_char* const Gb = smem + G::Y_OFF + G::Y_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int S = p.Lp, L = p.L;
  const int wgs_per_seq = S / ROWS;
  const int vid = (int)blockIdx.x;
  const int b = vid / wgs_per_seq, rb = vid - b * wgs_per_seq;
  const long long row0 = (long long)b * S + rb * ROWS;
  const int lrow0 = rb * ROWS;
  const int NHC = p.ffn_dim / 128;
  const int ub = G::UB0 + NHC * G::UCH;                     // units per wave of the stream

  // =========================== self-attention: 64 queries x 8 heads over the L real keys ===========================
  // (st_fused.hip's stage: a wave owns 32 queries of one head, four heads per round; keys >= L masked out)
  unsigned opack[HEADS / 4][8];
  {
    const int hs = w >> 1, qh = w & 1;
    const int ql = lane & 31, hh = lane >> 5;
    const bf16_t* qkv_seq = (const bf16_t*)p.qkv + (long long)b * S * 3 * C;
    const int head_bytes = S * (ST_KP + ST_VP);
    const float sc2 = p.attn_scale * 1.4426950408889634f;
    const int g4 = lane >> 4, t16 = lane & 15;
    const bool all_heads = HEADS * head_bytes <= 160 * 1024;
    const int hb = all_heads ? HEADS : 4;
    const int nkb = (L + 31) >> 5;                          // 32-key blocks that hold a real key
    bf16x8 bq[HEADS / 4][2];
#pragma unroll
    for (int ri = 0; ri < HEADS / 4; ++ri) {
      const bf16_t* qp = (const bf16_t*)p.qkv + (row0 + qh * 32 + ql) * 3 * C + (ri * 4 + hs) * 32 + hh * 8;
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
          v[j] = *reinterpret_cast<const u32x4*>(qkv_seq + (long long)row * 3 * C + (1 + isv) * C + (h0 + hl) * 32 + c * 8);
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
      }
      const int hl = (all_heads ? ri * 4 : 0) + hs;
      const lds_char* Ks = smem + hl * head_bytes;
      const lds_char* Vs = Ks + S * ST_KP;
      const lds_char* kfrag = Ks + ql * ST_KP + hh * 16;
      const lds_char* vfrag = Vs + (4 * hh + (t16 >> 2)) * ST_VP + ((g4 & 1) * 16 + (t16 & 3) * 4) * 2;
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
        // accumulator r of this lane is key kb * 32 + 8 (r / 4) + 4 hh + r % 4 (query ql): pad keys leave the softmax.
        // (key 0 is real, so every block kb < nkb holds a finite score for every query)
        float bmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kb * 32 + (r >> 2) * 8 + hh * 4 + (r & 3);
          s[r] = key < L ? s[r] * sc2 : -INFINITY;
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
    }
    __syncthreads();                      // the staging region becomes operand buffers + rings
  }

  // the layer input (residual of the first epilogue): fetched and RETIRED before any weight DMA is issued
  uint2 rsd[NSL][TT];
  {
    const bf16_t* xr = (const bf16_t*)p.x + row0 * C;
#pragma unroll
    for (int s = 0; s < NSL; ++s)
#pragma unroll
      for (int tt = 0; tt < TT; ++tt)
        rsd[s][tt] = *reinterpret_cast<const uint2*>(xr + (long long)(tt * 16 + l15) * C + (w * NSL + s) * 16 + 4 * lg);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  // ================================ weight stream + ring of this wave ================================
  StRing<D> rg;
  rg.rs_sh = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.wstream_b + (long long)w * ub * ST_UNIT), 0,
                                               ub * ST_UNIT, 0x00020000);
  rg.rs_img = rg.rs_sh;
  rg.g_iss = 0; rg.n1 = ub; rg.n_img = 0; rg.total = ub; rg.pos_iss = 0; rg.pos_con = 0;
  rg.ring = smem + G::RING_OFF + w * D * ST_UNIT;
  rg.voff = lane * 16;
#pragma unroll
  for (int i = 0; i < D; ++i) rg.issue_one();
  {
    const int hs = w >> 1, qh = w & 1;
    const int ql = lane & 31, hh = lane >> 5;
    // attention output -> operand buffer: row qh * 32 + ql, channels h * 32 + 8 j + 4 hh .. + 4
    const int r = qh * 32 + ql;
#pragma unroll
    for (int rd = 0; rd < HEADS / 4; ++rd) {
      const int h = rd * 4 + hs;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = h * 4 + j;
        const int phys = (c & ~15) | ((c ^ r) & 15);
        *reinterpret_cast<__attribute__((address_space(3))) u32x2*>(Y + r * PITCH + phys * 16 + hh * 8) =
            u32x2{opack[rd][2 * j], opack[rd][2 * j + 1]};
      }
    }
  }
  ST_BARRIER();                           // attention output complete in Y

  int yaddr[4], gaddr[4], woff[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int sw = (((4 * j + lg) ^ l15) & 15) * 16;
    yaddr[j] = l15 * PITCH + sw;
    gaddr[j] = l15 * 256 + sw;
  }
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) woff[ks] = l15 * 128 + (((4 * ks + lg) ^ ((l15 >> 1) & 7)) * 16);
  float sx[TT], sxx[TT], mean[TT], rstd[TT];
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) sx[tt] = sxx[tt] = mean[tt] = rstd[tt] = 0.f;
  const float* vb = p.vec_b;              // [out_proj bias (C) | colsum of linear1 (F) | folded bias of linear1 (F) | linear2 bias (C)]

  // residual stream of this wave's columns, fp32: res[s][tt][j] = row 16 tt + l15, column (w NSL + s) 16 + 4 lg + j
  f32x4 res[NSL][TT], acc[NSL][TT];
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < NSL; ++s)
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) acc[s][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
  };

  // ---- out_proj + x -> x1
  f32x4 ev0[NSL];
#pragma unroll
  for (int s = 0; s < NSL; ++s) ev0[s] = st_vec4(vb + (w * NSL + s) * 16, lg);
  zero_acc();
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) st_gemm_step<D, NSL, false, 0, TT>(rg, Y, yaddr, kt, 16 * PITCH, woff, acc, sx, sxx);
#pragma unroll
  for (int s = 0; s < NSL; ++s) {
    const f32x4 bi = ev0[s];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const uint2 t2 = rsd[s][tt];
      res[s][tt][0] = acc[s][tt][0] + bi[0] + __uint_as_float(t2.x << 16);
      res[s][tt][1] = acc[s][tt][1] + bi[1] + __uint_as_float(t2.x & 0xffff0000u);
      res[s][tt][2] = acc[s][tt][2] + bi[2] + __uint_as_float(t2.y << 16);
      res[s][tt][3] = acc[s][tt][3] + bi[3] + __uint_as_float(t2.y & 0xffff0000u);
    }
  }
  ST_BARRIER();                           // every wave is done reading the attention output
  // bf16 copy of the residual stream = the feed-forward's operand.  A pad row's input may be anything (inf, NaN): its
  // copy is zero, so the LayerNorm statistics and the hidden chunk of that row stay finite.
#pragma unroll
  for (int s = 0; s < NSL; ++s) {
    const int c = ((w * NSL + s) * 16 + 4 * lg) >> 3;
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const int r = tt * 16 + l15;
      const bool real = lrow0 + r < L;
      const int phys = (c & ~15) | ((c ^ r) & 15);
      uint2 o;
      o.x = real ? st_pack2(res[s][tt][0], res[s][tt][1]) : 0u;
      o.y = real ? st_pack2(res[s][tt][2], res[s][tt][3]) : 0u;
      *reinterpret_cast<__attribute__((address_space(3))) u32x2*>(Y + r * PITCH + phys * 16 + (lg & 1) * 8) = u32x2{o.x, o.y};
    }
  }
  ST_BARRIER();

  // ---- feed-forward: per hidden chunk of 128, h = relu(LN-fold(x1) W1'^T + b1') -> LDS -> acc += h W2[:, chunk]^T.
  //      The first chunk's GEMM also yields the LayerNorm-fold row statistics of x1.
  const float* cs_ff = vb + C;
  const float* bi_ff = vb + C + p.ffn_dim;
  zero_acc();
  auto chunk = [&](int hc, auto first_) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(first_)::value;
    f32x4 hq[1][TT];
    const f32x4 cs1 = st_vec4(cs_ff + hc * 128 + w * 16, lg);
    const f32x4 bi1 = st_vec4(bi_ff + hc * 128 + w * 16, lg);
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) hq[0][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) st_gemm_step<D, 1, FIRST, 0, TT>(rg, Y, yaddr, kt, 16 * PITCH, woff, hq, sx, sxx);
    if constexpr (FIRST) st_ln_stats<TT>(sx, sxx, 1.f / (float)C, p.ln_eps, mean, rstd);
    lds_char* gb = Gb + (G::GBUF == 2 ? (hc & 1) * G::G_BYTES : 0);
    if (G::GBUF == 1) ST_BARRIER();                     // the previous chunk's readers are done
    {
      const int c = (w * 16 + 4 * lg) >> 3;
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = fmaxf(rstd[tt] * (hq[0][tt][j] - mean[tt] * cs1[j]) + bi1[j], 0.f);
        const int r = tt * 16 + l15;
        const int phys = (c & ~15) | ((c ^ r) & 15);
        *reinterpret_cast<__attribute__((address_space(3))) u32x2*>(gb + r * 256 + phys * 16 + (lg & 1) * 8) =
            u32x2{st_pack2(y[0], y[1]), st_pack2(y[2], y[3])};
      }
    }
    ST_BARRIER();
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) st_gemm_step<D, NSL, false, 0, TT>(rg, gb, gaddr, kt, 16 * 256, woff, acc, sx, sxx);
  };
  chunk(0, std::true_type());
#pragma unroll 1
  for (int hc = 1; hc < NHC; ++hc) chunk(hc, std::false_type());

  // ---- + linear2 bias + x1 -> out   (only dummy re-fetches are in flight now: drain them, then ordinary loads are safe)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int s = 0; s < NSL; ++s) ev0[s] = st_vec4(vb + C + 2 * p.ffn_dim + (w * NSL + s) * 16, lg);
  {
    bf16_t* outp = (bf16_t*)p.out + row0 * C;
#pragma unroll
    for (int s = 0; s < NSL; ++s) {
      const int n0 = (w * NSL + s) * 16 + 4 * lg;
      const f32x4 bi = ev0[s];
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const int r = tt * 16 + l15;
        const bool real = lrow0 + r < L;
        uint2 o;
        o.x = real ? st_pack2(acc[s][tt][0] + bi[0] + res[s][tt][0], acc[s][tt][1] + bi[1] + res[s][tt][1]) : 0u;
        o.y = real ? st_pack2(acc[s][tt][2] + bi[2] + res[s][tt][2], acc[s][tt][3] + bi[3] + res[s][tt][3]) : 0u;
        *reinterpret_cast<uint2*>(outp + (long long)r * C + n0) = o;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

int rollout_launch(const SdmiRolloutLayerArgs& a, hipStream_t st) {
  typedef RlGeom<4> G;
  const int heads_bytes = a.Lp * (ST_KP + ST_VP);
  const int att = (G::HEADS * heads_bytes <= 160 * 1024 ? G::HEADS : 4) * heads_bytes;
  const int smem_b = att > G::SMEM_GEMM ? att : G::SMEM_GEMM;
  const int grid = a.B * (a.Lp / G::ROWS);
  if (a.phase == 0 || a.phase == 1) {
    SDMI_OPTIN_LDS((rollout_qkv_kernel<4>), G::SMEM_GEMM, "rollout_layer (phase A)");
    hipLaunchKernelGGL((rollout_qkv_kernel<4>), dim3(grid), dim3(512), G::SMEM_GEMM, st, a);
    const int rc = sdmi_check_launch("rollout_layer (phase A)");
    if (rc) return rc;
  }
  if (a.phase == 0 || a.phase == 2) {
    SDMI_OPTIN_LDS((rollout_tail_kernel<4>), 160 * 1024, "rollout_layer (phase B)");
    hipLaunchKernelGGL((rollout_tail_kernel<4>), dim3(grid), dim3(512), smem_b, st, a);
    return sdmi_check_launch("rollout_layer (phase B)");
  }
  return SDMI_OK;
}

}  // namespace

extern "C" int sdmi_rollout_layer(const SdmiRolloutLayerArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->x && a->qkv && a->out, "null pointer");
  SDMI_REQUIRE(a->wstream_a && a->vec_a && a->wstream_b && a->vec_b, "null stream");
  SDMI_REQUIRE(a->C == 256 && a->heads == 8, "C must be 256 with 8 heads of 32");
  SDMI_REQUIRE(a->B >= 1, "empty batch");
  SDMI_REQUIRE(a->Lp >= 64 && a->Lp <= 256 && a->Lp % 64 == 0, "Lp must be a multiple of the 64-row tile, at most 256");
  SDMI_REQUIRE(a->L >= 1 && a->L <= a->Lp, "1 <= L <= Lp");
  SDMI_REQUIRE(a->ffn_dim >= 128 && a->ffn_dim <= 4 * a->C && a->ffn_dim % 128 == 0, "ffn_dim must be a multiple of 128, at most 4C");
  SDMI_REQUIRE(a->phase >= 0 && a->phase <= 2, "phase: 0 = both, 1 = A, 2 = B");
  SDMI_REQUIRE((const char*)a->out != (const char*)a->x, "out must not be x");
  return rollout_launch(*a, (hipStream_t)stream);
}
