// Sequence-resident fused SlotFormer rollout layer (bf16 inference; sdmi.h: sdmi_rollout_layer).
//
// Reference: vp_vqa/models/slotformer.py:70-78 -- nn.TransformerEncoderLayer(norm_first=True, activation=relu,
// batch_first=True):  x += out_proj(MHA(LN1(x)));  x += linear2(relu(linear1(LN2(x)))).
//
// The layer is st_fused.hip's SpatialTransformer block without GroupNorm, proj_in, the folded cross-attention, GEGLU
// and proj_out; it has a biased q | k | v and a ReLU feed-forward.  Same two launches, built from the same pieces
// (st_core.h: weights as the A operand of v_mfma_f32_16x16x32_bf16, per-wave weight rings over LDS-DMA with counted
// vmcnt, LayerNorm folded into the epilogue, the self-attention stage, the row <-> operand buffer copies), same operand
// layouts:
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
  st_ring_init<D>(rg, p.wstream_a, G::UA, smem + G::RING_OFF, lane, w);      // weights in flight under the activation load
  // ---- this workgroup's 64 rows into the operand buffer
  st_load_rows_to_y<C, ROWS>((const bf16_t*)p.x + row0 * C, C, Y, tid);
  ST_BARRIER();

  int yaddr[4], woff[2];
  st_frag_addrs<PITCH>(l15, lg, yaddr, woff);
  float sx[TT], sxx[TT], mean[TT], rstd[TT];
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) sx[tt] = sxx[tt] = 0.f;

  // ---- q | k | v = LayerNorm1(x) W^T + b through the fold; pad rows are written as zeros
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
  unsigned opack[HEADS / 4][8];
  st_self_attention<C, TT, true, false>(opack, (const bf16_t*)p.qkv, b, lrow0, S, L, p.attn_scale, nullptr, smem, tid, lane, w);

  // the layer input (residual of the first epilogue): fetched and RETIRED before any weight DMA is issued
  uint2 rsd[NSL][TT];
  st_load_residual<C, TT, NSL, true>(rsd, (const bf16_t*)p.x + row0 * C, w, l15, lg);
  // ================================ weight stream + ring of this wave ================================
  StRing<D> rg;
  st_ring_init<D>(rg, p.wstream_b, ub, smem + G::RING_OFF, lane, w);
  st_attn_out_to_y<C, TT, false>(opack, Y, nullptr, row0, w, lane);
  ST_BARRIER();                           // attention output complete in Y

  int yaddr[4], gaddr[4], woff[2];
  st_frag_addrs<PITCH>(l15, lg, yaddr, gaddr, woff);
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
  st_add_bias_residual<TT, NSL>(res, acc, ev0, rsd);
  ST_BARRIER();                           // every wave is done reading the attention output
  // bf16 copy of the residual stream = the feed-forward's operand (pad rows: zeros)
  st_rows_to_y<C, TT, NSL, false, true>(res, Y, nullptr, w, l15, lg, lrow0, L);
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
