// Image-resident fused SpatialTransformer block (bf16 inference; sdmi.h: sdmi_st_block).
//
// Reference: video_based/models/unet/attention.py:297-308 (SpatialTransformer: GroupNorm -> proj_in ->
// BasicTransformerBlock -> proj_out + x) and 247-251 (BasicTransformerBlock: self-attention, slot
// cross-attention, GEGLU feed-forward, each behind a LayerNorm and with a residual add).
//
// Everything in the block is local to a token row or to an image, so a workgroup that owns 64 token rows of
// one image needs no other workgroup -- except for the keys / values of its image's self-attention.  The
// block is therefore TWO launches instead of 10-13:
//   phase A  GroupNorm (statistics of the whole image recomputed by each of its S/64 workgroups: the image
//            is 32-128 KB and L2 resident) -> proj_in -> tok;  LayerNorm-fold -> q | k | v
//   phase B  self-attention of the 64 rows over the image's S keys -> to_out + tok -> LayerNorm-fold ->
//            folded slot cross-attention (per-image weights, softmax over each head's 7 slots) -> + ->
//            LayerNorm-fold -> GEGLU feed-forward, hidden chunk by hidden chunk, accumulated straight into
//            the merged (ff.net.2 ; proj_out) output -> + x
// Activations of the 64 rows stay in LDS (bf16, as the next GEMM's operand) and registers (fp32 residual
// stream); only tok, q|k|v and the block output touch HBM.
//
// GEMM core: out^T[n][m] = W[n][:] . act[m][:] on v_mfma_f32_16x16x32_bf16 with W as the A operand, so a lane's
// four accumulator values are FOUR CONSECUTIVE OUTPUT COLUMNS of ONE token row (lane & 15): residual adds,
// LayerNorm-fold terms, GEGLU and the 8-wide slot softmax are lane-local, and the result goes back to LDS as
// one ds_write_b64 in the next GEMM's operand layout.  The eight waves of the workgroup are the same program
// (no loader waves): wave w owns output columns [w*C/8, (w+1)*C/8) -- NSL = C/128 slices of 16 -- for ALL 64
// rows, and streams exactly the weight rows it multiplies through a PRIVATE ring of 2 KB units
// (`buffer_load_dwordx4 ... lds`, counted `s_waitcnt vmcnt`): no barrier orders weight traffic -- the waves run
// free inside a GEMM phase --, barriers exist only where an LDS activation buffer changes hands (~2 per phase).  The weights are pre-packed
// on the host (kern.WeightBank.st_fused_weights) into per-wave streams of units in consumption order, each unit
// the exact XOR-swizzled LDS image of 16 weight rows x 64 k, so the fetch side is `base + g * 2048`.
#include "st_core.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// phase A: GroupNorm -> proj_in -> tok ; LayerNorm-fold -> q | k | v
// ---------------------------------------------------------------------------------------------------------
template <int C, int TT>
__global__ __launch_bounds__(512, 2) void st_block_a_kernel(SdmiStBlockArgs p) {
  typedef StGeom<C, TT> G;
  constexpr int ROWS = G::ROWS;
  constexpr int NSL = G::NSL, KT = G::KT, D = G::D, PITCH = G::PITCH;
  extern __shared__ __attribute__((aligned(16))) char smem_[];
  lds_char* const smem = (lds_char*)smem_;
  lds_char* const Y = smem + G::Y_OFF;
  float* const red = (float*)(smem_ + G::Y_OFF + G::Y_BYTES);          // GroupNorm partials (the chunk buffer's region)
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wgs_per_img = p.S / ROWS;
  // block b runs on XCD b % 8 (observed placement; speed only): every XCD gets a contiguous range of workgroup
  // ids, so the S / ROWS workgroups of an image share one L2 (they all read the image's x / K / V)
  // ff_split = 2: a PAIR of workgroups per ROWS token rows -- both run the GroupNorm and proj_in (tok is written twice with
  // the same bytes), the first takes the q pass, the second k and v: 2 C^2 / 3 C^2 of weights per workgroup instead of 4 C^2
  const int vid0 = st_xcd_id((int)blockIdx.x, (int)gridDim.x);
  const int ffs = p.ff_split == 2 ? 2 : 1;
  const int half = ffs == 2 ? (vid0 & 1) : 0;
  const int vid = ffs == 2 ? (vid0 >> 1) : vid0;
  const int b = vid / wgs_per_img, rb = vid - b * wgs_per_img;
  const long long row0 = (long long)b * p.S + rb * ROWS;     // first token row of this workgroup
  const int pass0 = half ? 1 : 0, pass1 = (ffs == 2 && !half) ? 1 : 3;

  StRing<D> rg;
  rg.rs_sh = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.wstream_a + (long long)w * G::UA * ST_UNIT), 0,
                                               G::UA * ST_UNIT, 0x00020000);
  rg.rs_img = rg.rs_sh;
  rg.g_iss = 0; rg.n1 = G::UA; rg.n_img = 0; rg.total = G::UA; rg.pos_iss = 0; rg.pos_con = 0;
  if (ffs == 2) {
    rg.total = half ? 3 * KT * NSL : 2 * KT * NSL;
    if (half) { rg.jump_at = KT * NSL; rg.jump = KT * NSL; }      // (skips the q units)
  }
  rg.ring = smem + G::RING_OFF + w * D * ST_UNIT;
  rg.voff = lane * 16;
#pragma unroll
  for (int i = 0; i < D; ++i) rg.issue_one();               // weights in flight under the GroupNorm
  STA_STAMP(0);

  // ---- GroupNorm statistics of the image (32 groups): thread -> (row slot, 16-byte vector column)
  constexpr int VPR = C / 8;                    // vectors per row
  constexpr int RPP = 512 / VPR;                // rows per pass
  constexpr int GS4 = C / 32 / 4;               // half-vectors (4 channels) per group
  {
    const bf16_t* xi = (const bf16_t*)p.x + (long long)b * p.S * C;
    float s0 = 0.f, s1 = 0.f, q0 = 0.f, q1 = 0.f;
    const int vr = tid / VPR, vc = tid - vr * VPR;
    if (vr < RPP) {
      // (eight rows in flight: one load per iteration behind its own wait cost a memory latency per row)
      for (int r0 = vr; r0 < p.S; r0 += 8 * RPP) {
        uint4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int r = r0 + j * RPP;
          v[j] = r < p.S ? *reinterpret_cast<const uint4*>(xi + (long long)r * C + vc * 8) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f[8];
          unpack16<bf16_t>(v[j], f);
          s0 += (f[0] + f[1]) + (f[2] + f[3]);
          s1 += (f[4] + f[5]) + (f[6] + f[7]);
          q0 += f[0] * f[0] + f[1] * f[1] + f[2] * f[2] + f[3] * f[3];
          q1 += f[4] * f[4] + f[5] * f[5] + f[6] * f[6] + f[7] * f[7];
        }
      }
      f32x4 v = {s0, q0, s1, q1};
      *reinterpret_cast<f32x4*>(red + (vr * VPR + vc) * 4) = v;      // [row slot][vector][{s, q} x 2 halves]
    }
    ST_BARRIER();
    if (tid < 32) {
      float s = 0.f, q = 0.f;
      for (int r = 0; r < RPP; ++r)
        for (int h = 0; h < GS4; ++h) {
          const int hv = tid * GS4 + h;           // half-vector index along C
          const float* e = red + ((r * VPR + (hv >> 1)) * 4 + (hv & 1) * 2);
          s += e[0];
          q += e[1];
        }
      const float n = (float)(p.S * (C / 32));
      const float mean = s / n;
      const float var = fmaxf(q / n - mean * mean, 0.f);
      red[512 * 4 + tid * 2] = mean;
      red[512 * 4 + tid * 2 + 1] = rsqrtf(var + p.gn_eps);
    }
    ST_BARRIER();
  STA_STAMP(1);
  }
  // ---- normalise this workgroup's 64 rows into the operand buffer
  {
    const float* st = red + 512 * 4;
    const bf16_t* xr = (const bf16_t*)p.x + row0 * C;
    static_assert((ROWS * VPR) % 512 == 0, "whole passes");
#pragma unroll
    for (int it = 0; it < ROWS * VPR / 512; ++it) {
      const int i = tid + it * 512;
      const int r = i / VPR, vc = i - r * VPR;
      float f[8], gm[8], bt[8];
      unpack16<bf16_t>(*reinterpret_cast<const uint4*>(xr + (long long)r * C + vc * 8), f);
      *reinterpret_cast<f32x4*>(gm) = *reinterpret_cast<const f32x4*>(p.gn_gamma + vc * 8);
      *reinterpret_cast<f32x4*>(gm + 4) = *reinterpret_cast<const f32x4*>(p.gn_gamma + vc * 8 + 4);
      *reinterpret_cast<f32x4*>(bt) = *reinterpret_cast<const f32x4*>(p.gn_beta + vc * 8);
      *reinterpret_cast<f32x4*>(bt + 4) = *reinterpret_cast<const f32x4*>(p.gn_beta + vc * 8 + 4);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int g = (vc * 8 + h * 4) / (C / 32);
        const float mean = st[g * 2], rstd = st[g * 2 + 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) f[h * 4 + j] = (f[h * 4 + j] - mean) * rstd * gm[h * 4 + j] + bt[h * 4 + j];
      }
      const int phys = (vc & ~15) | ((vc ^ r) & 15);
      { const uint4 pk = pack16<bf16_t>(f);
        *reinterpret_cast<__attribute__((address_space(3))) u32x4*>(Y + r * PITCH + phys * 16) = u32x4{pk.x, pk.y, pk.z, pk.w}; }
    }
  }
  ST_BARRIER();
  STA_STAMP(2);

  // lane constants of the GEMM core
  int yaddr[4], woff[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) yaddr[j] = l15 * PITCH + ((((4 * j + lg) ^ l15) & 15) * 16);
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) woff[ks] = l15 * 128 + (((4 * ks + lg) ^ ((l15 >> 1) & 7)) * 16);
  float sx[TT], sxx[TT];
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) sx[tt] = sxx[tt] = 0.f;

  // Epilogue operands are fetched BEFORE the GEMM they follow: a vector load issued behind the weight DMAs
  // would make its consumer wait for every DMA in front of it (vmcnt retires in order) -- a ring drain.
  // ---- proj_in: tok = gn(x) Win^T + bin
  f32x4 acc[NSL][TT], ev0[NSL], ev1[NSL];
#pragma unroll
  for (int s = 0; s < NSL; ++s) {
    ev0[s] = st_vec4(p.vec_a + (w * NSL + s) * 16, lg);
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) acc[s][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) st_gemm_step<D, NSL, false, 0, TT>(rg, Y, yaddr, kt, 16 * PITCH, woff, acc, sx, sxx);
  ST_BARRIER();                                      // every wave is done reading gn(x)
  STA_STAMP(3);
  {
    bf16_t* tok = (bf16_t*)p.tok + row0 * C;
#pragma unroll
    for (int s = 0; s < NSL; ++s) {
      const int n0 = (w * NSL + s) * 16 + 4 * lg;
      const f32x4 bi = ev0[s];
      const int c = n0 >> 3;
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const int r = tt * 16 + l15;
        uint2 o;
        o.x = st_pack2(acc[s][tt][0] + bi[0], acc[s][tt][1] + bi[1]);
        o.y = st_pack2(acc[s][tt][2] + bi[2], acc[s][tt][3] + bi[3]);
        *reinterpret_cast<uint2*>(tok + (long long)r * C + n0) = o;
        const int phys = (c & ~15) | ((c ^ r) & 15);
        *reinterpret_cast<__attribute__((address_space(3))) u32x2*>(Y + r * PITCH + phys * 16 + (lg & 1) * 8) = u32x2{o.x, o.y};
      }
    }
  }
  ST_BARRIER();
  STA_STAMP(4);

  // ---- q | k | v = LayerNorm(tok) W^T through the fold: three passes of N = C over the same operand
  float mean[TT], rstd[TT];
#pragma unroll 1
  for (int pass = pass0; pass < pass1; ++pass) {
    const float* colsum = p.vec_a + C + pass * C;
    const float* bias = p.vec_a + 4 * C + pass * C;
#pragma unroll
    for (int s = 0; s < NSL; ++s) {
      ev0[s] = st_vec4(colsum + (w * NSL + s) * 16, lg);
      ev1[s] = st_vec4(bias + (w * NSL + s) * 16, lg);
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) acc[s][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // (the NSL * 4 row stores of the epilogue before this pass are younger than every DMA in flight)
    if (pass == pass0) {
      st_gemm_step<D, NSL, true, NSL * TT, TT>(rg, Y, yaddr, 0, 16 * PITCH, woff, acc, sx, sxx);
#pragma unroll
      for (int kt = 1; kt < KT; ++kt) st_gemm_step<D, NSL, true, 0, TT>(rg, Y, yaddr, kt, 16 * PITCH, woff, acc, sx, sxx);
      st_ln_stats<TT>(sx, sxx, 1.f / (float)C, p.ln_eps, mean, rstd);
    } else {
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
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = rstd[tt] * (acc[s][tt][j] - mean[tt] * cs[j]) + bi[j];
        uint2 o;
        o.x = st_pack2(v[0], v[1]);
        o.y = st_pack2(v[2], v[3]);
        *reinterpret_cast<uint2*>(qkv + (long long)r * 3 * C + n0) = o;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no DMA may outlive the workgroup's LDS
  STA_STAMP(5);
}

// ---------------------------------------------------------------------------------------------------------
// phase B
// ---------------------------------------------------------------------------------------------------------
template <int C, int TT>
__global__ __launch_bounds__(512, 2) void st_block_b_kernel(SdmiStBlockArgs p) {
  typedef StGeom<C, TT> G;
  constexpr int ROWS = G::ROWS;
  constexpr int NSL = G::NSL, KT = G::KT, D = G::D, PITCH = G::PITCH, HEADS = G::HEADS, R = G::R;
  extern __shared__ __attribute__((aligned(16))) char smem_[];
  lds_char* const smem = (lds_char*)smem_;
  lds_char* const Y = smem + G::Y_OFF;
  lds_char* const Gb = smem + G::Y_OFF + G::Y_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wgs_per_img = p.S / ROWS;
  // block b runs on XCD b % 8 (observed placement; speed only): every XCD gets a contiguous range of workgroup
  // ids, so the S / ROWS workgroups of an image share one L2 (they all read the image's x / K / V)
  const int vid0 = st_xcd_id((int)blockIdx.x, (int)gridDim.x);
  const int ffs = p.ff_split == 2 ? 2 : 1;
  const int half = ffs == 2 ? (vid0 & 1) : 0;            // (the two workgroups of a pair: neighbours on one XCD)
  const int vid = ffs == 2 ? (vid0 >> 1) : vid0;
  const int b = vid / wgs_per_img, rb = vid - b * wgs_per_img;
  const long long row0 = (long long)b * p.S + rb * ROWS;
  const int S = p.S;
  ST_STAMP(0);

  // =========================== self-attention: 64 queries x HEADS heads over S keys ===========================
  unsigned opack[HEADS / 4][8];
  st_self_attention<C, TT, false, false>(opack, (const bf16_t*)p.qkv, b, rb * ROWS, S, S, p.attn_scale, nullptr, smem, tid, lane, w,
                                         [&](int i) __attribute__((always_inline)) { ST_STAMP(8 + i); });
  ST_STAMP(10);

  // the token residual of the first epilogue: fetched and RETIRED before any weight DMA is issued
  uint2 rsd[NSL][TT];
  st_load_residual<C, TT, NSL, true>(rsd, (const bf16_t*)p.tok + row0 * C, w, l15, lg);
  ST_STAMP(11);
  // the second-dispatched half of the workgroup loses issue arbitration to the first on every SIMD and arrives last
  // at each hand-off barrier (the FF loop's wave 0 spent 22 % of its time waiting there): static priority for it
  if (w >= 4) __builtin_amdgcn_s_setprio(1);
  // ================================ weight stream + ring of this wave ================================
  StRing<D> rg;
  st_ring_setup<D>(rg, p.wstream_b, G::UB1 + G::UB2, smem + G::RING_OFF, lane, w);
  rg.rs_img = __builtin_amdgcn_make_buffer_rsrc(
      (void*)((const char*)p.wstream_img + ((long long)b * 8 + w) * G::UIMG * ST_UNIT), 0, G::UIMG * ST_UNIT, 0x00020000);
  rg.n1 = G::UB1; rg.n_img = G::UIMG; rg.total = G::UB1 + G::UIMG + G::UB2;
  constexpr int UCH = KT * 2 + 2 * NSL;                 // units of one hidden chunk
  if (ffs == 2) {                                        // this workgroup's half of the hidden chunks
    rg.total -= (G::NHC / 2) * UCH;
    if (half) { rg.jump_at = G::UB1 + KT * NSL; rg.jump = (G::NHC / 2) * UCH; }
  }
  st_ring_prime<D>(rg);
  st_attn_out_to_y<C, TT, false>(opack, Y, nullptr, row0, w, lane);
  ST_BARRIER();                           // attention output complete in Y
  ST_STAMP(1);

  int yaddr[4], gaddr[4], woff[2];
  st_frag_addrs<PITCH>(l15, lg, yaddr, gaddr, woff);
  float sx[TT], sxx[TT], mean[TT], rstd[TT];
  const float* vb = p.vec_b;              // [bo | bo2 | colsum_ff (8C) | bias_ff (8C) | bias_out]  fp32
  const float* vi = p.vec_img + (long long)b * 256;   // per image: [colsum_q (128) | bias_q (128)]

  // residual stream of this wave's columns, fp32: res[s][tt][j] = row 16 tt + l15, column (w NSL + s) 16 + 4 lg + j
  f32x4 res[NSL][TT], acc[NSL][TT];
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < NSL; ++s)
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) acc[s][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
  };

  // (epilogue operands are fetched BEFORE the GEMM they follow -- see phase A)
  ST_STAMP(2);
  // ---- attn1.to_out + tok  -> x1
  f32x4 ev0[NSL];
#pragma unroll
  for (int s = 0; s < NSL; ++s) ev0[s] = st_vec4(vb + (w * NSL + s) * 16, lg);
  zero_acc();
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) st_gemm_step<D, NSL, false, 0, TT>(rg, Y, yaddr, kt, 16 * PITCH, woff, acc, sx, sxx);
  st_add_bias_residual<TT, NSL>(res, acc, ev0, rsd);
  ST_BARRIER();
  st_rows_to_y<C, TT, NSL, false>(res, Y, nullptr, w, l15, lg);     // bf16 copy of the residual stream = next GEMM's operand
  ST_BARRIER();

  ST_STAMP(3);
  // ---- folded slot cross-attention: P = softmax8(LN-fold(x1) Wq[b]^T) ; x2 = P W2[b]^T + bo2 + x1
  {
    f32x4 sc[1][TT];
    const int n0 = w * 16 + 4 * lg;                   // column of the padded score matrix
    const f32x4 cs = st_vec4(vi + w * 16, lg);
    const f32x4 bi = st_vec4(vi + 128 + w * 16, lg);
#pragma unroll
    for (int s = 0; s < NSL; ++s) ev0[s] = st_vec4(vb + C + (w * NSL + s) * 16, lg);
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      sc[0][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
      sx[tt] = sxx[tt] = 0.f;
    }
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) st_gemm_step<D, 1, true, 0, TT>(rg, Y, yaddr, kt, 16 * PITCH, woff, sc, sx, sxx);
    st_ln_stats<TT>(sx, sxx, 1.f / (float)C, p.ln_eps, mean, rstd);
    const int c = n0 >> 3;
    // score groups: 8 columns per head (two lane groups of four, lg ^ 1) up to 8 slots; from 9 slots (C = 256: 8 heads
    // x 16 = the 128 padded columns, a wave's 16-column slice is ONE head) 16 columns = all four lane groups of a row
    const bool wide = p.slots > 8;
    const int Rr = wide ? HEADS * 16 : R;
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      float v[4];
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = n0 < Rr && (4 * (wide ? lg : (lg & 1)) + j) < p.slots;
        v[j] = ok ? rstd[tt] * (sc[0][tt][j] - mean[tt] * cs[j]) + bi[j] : -INFINITY;
        mx = fmaxf(mx, v[j]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));          // the group's other four columns: lane ^ 16
      if (wide) mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      float sm = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = n0 < Rr ? __expf(v[j] - mx) : 0.f;
        sm += v[j];
      }
      sm += __shfl_xor(sm, 16, 64);
      if (wide) sm += __shfl_xor(sm, 32, 64);
      const float inv = n0 < Rr ? 1.f / sm : 0.f;
      const int r = tt * 16 + l15;
      const int phys = (c & ~15) | ((c ^ r) & 15);
      uint2 o;
      o.x = st_pack2(v[0] * inv, v[1] * inv);
      o.y = st_pack2(v[2] * inv, v[3] * inv);
      *reinterpret_cast<__attribute__((address_space(3))) u32x2*>(Gb + r * 256 + phys * 16 + (lg & 1) * 8) = u32x2{o.x, o.y};
    }
  }
  ST_BARRIER();
  zero_acc();
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) st_gemm_step<D, NSL, false, 0, TT>(rg, Gb, gaddr, kt, 16 * 256, woff, acc, sx, sxx);
#pragma unroll
  for (int s = 0; s < NSL; ++s) {
    const f32x4 bi = ev0[s];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
#pragma unroll
      for (int j = 0; j < 4; ++j) res[s][tt][j] += acc[s][tt][j] + bi[j];
  }
  ST_BARRIER();                                         // (Y readers of the score GEMM are long done; Gb readers too)
  st_rows_to_y<C, TT, NSL, false>(res, Y, nullptr, w, l15, lg);
  ST_BARRIER();

  ST_STAMP(4);
  // ---- merged (ff.net.2 ; proj_out): out = [g | x2] [Wpo Wff | Wpo]^T + b' + x.  First the x2 part (also
  //      yields the LayerNorm-fold statistics of x2 for the feed-forward), then the hidden chunks.
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) sx[tt] = sxx[tt] = 0.f;
  zero_acc();
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) st_gemm_step<D, NSL, true, 0, TT>(rg, Y, yaddr, kt, 16 * PITCH, woff, acc, sx, sxx);
  st_ln_stats<TT>(sx, sxx, 1.f / (float)C, p.ln_eps, mean, rstd);
  if (half) zero_acc();                                  // (the x2 Wpo^T term belongs to the first workgroup of the pair)
  const float* cs_ff = vb + 2 * C;
  const float* bi_ff = vb + 10 * C;
  ST_TL_DECL
  ST_TL_BEGIN
  const int hc0 = half * (G::NHC / 2), hc1 = ffs == 2 ? hc0 + G::NHC / 2 : G::NHC;
#pragma unroll 1
  for (int hc = hc0; hc < hc1; ++hc) {
    f32x4 vg[2][TT];                                     // [value | gate] columns hc * 128 + w * 16 + 4 lg ..
    const f32x4 csv = st_vec4(cs_ff + hc * 128 + w * 16, lg);
    const f32x4 csg = st_vec4(cs_ff + 4 * C + hc * 128 + w * 16, lg);
    const f32x4 biv = st_vec4(bi_ff + hc * 128 + w * 16, lg);
    const f32x4 big = st_vec4(bi_ff + 4 * C + hc * 128 + w * 16, lg);
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) vg[0][tt] = vg[1][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
    ST_TL_LAP(3);
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) st_gemm_step<D, 2, false, 0, TT>(rg, Y, yaddr, kt, 16 * PITCH, woff, vg, sx, sxx);
    ST_TL_LAP(0);
    lds_char* gb = Gb + (G::GBUF == 2 ? (hc & 1) * G::G_BYTES : 0);
    if (G::GBUF == 1) ST_BARRIER();                     // the previous chunk's readers are done
    {
      const int c = (w * 16 + 4 * lg) >> 3;
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = rstd[tt] * (vg[0][tt][j] - mean[tt] * csv[j]) + biv[j];
          const float g = rstd[tt] * (vg[1][tt][j] - mean[tt] * csg[j]) + big[j];
          y[j] = v * act_apply<true>(g, SDMI_ACT_GELU);
        }
        const int r = tt * 16 + l15;
        const int phys = (c & ~15) | ((c ^ r) & 15);
        uint2 o;
        o.x = st_pack2(y[0], y[1]);
        o.y = st_pack2(y[2], y[3]);
        *reinterpret_cast<__attribute__((address_space(3))) u32x2*>(gb + r * 256 + phys * 16 + (lg & 1) * 8) = u32x2{o.x, o.y};
      }
    }
    ST_TL_LAP(1);
    ST_BARRIER();
    ST_TL_LAP(2);
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) st_gemm_step<D, NSL, false, 0, TT>(rg, gb, gaddr, kt, 16 * 256, woff, acc, sx, sxx);
  }
  ST_STAMP(5);
  ST_TL_FLUSH;
  // ---- + b' + x  -> out   (only dummy re-fetches are in flight now: drain them, then ordinary loads are safe)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (ffs == 2) {          // this workgroup's fp32 partial; the pair is summed (+ b' + x) by the kernel behind
    float* pp = p.part + ((long long)half * p.B * p.S + row0) * C;
#pragma unroll
    for (int s = 0; s < NSL; ++s)
#pragma unroll
      for (int tt = 0; tt < TT; ++tt)
        *reinterpret_cast<f32x4*>(pp + (long long)(tt * 16 + l15) * C + (w * NSL + s) * 16 + 4 * lg) = acc[s][tt];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return;
  }
#pragma unroll
  for (int s = 0; s < NSL; ++s) ev0[s] = st_vec4(vb + 18 * C + (w * NSL + s) * 16, lg);
  st_load_residual<C, TT, NSL, false>(rsd, (const bf16_t*)p.x + row0 * C, w, l15, lg);
  st_add_bias_residual<TT, NSL>(acc, acc, ev0, rsd);
  st_store_rows<C, TT, NSL>(acc, (bf16_t*)p.out + row0 * C, C, w, l15, lg);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ST_STAMP(6);
}

template <int C, int TT>
int st_launch(const SdmiStBlockArgs& a, hipStream_t st) {
  typedef StGeom<C, TT> G;
  const int heads_bytes = a.S * (ST_KP + ST_VP);
  const int att = (G::HEADS * heads_bytes <= 160 * 1024 ? G::HEADS : 4) * heads_bytes;
  const int smem_b = att > G::SMEM_GEMM ? att : G::SMEM_GEMM;
  const int grid = a.B * (a.S / G::ROWS);
  if (a.phase == 0 || a.phase == 1) {
    SDMI_OPTIN_LDS((st_block_a_kernel<C, TT>), G::SMEM_GEMM, "st_block (phase A)");
    hipLaunchKernelGGL((st_block_a_kernel<C, TT>), dim3(grid * (a.ff_split == 2 ? 2 : 1)), dim3(512), G::SMEM_GEMM, st, a);
    const int rc = sdmi_check_launch("st_block (phase A)");
    if (rc) return rc;
  }
  if (a.phase == 0 || a.phase == 2) {
    SDMI_OPTIN_LDS((st_block_b_kernel<C, TT>), 160 * 1024, "st_block (phase B)");
    hipLaunchKernelGGL((st_block_b_kernel<C, TT>), dim3(grid * (a.ff_split == 2 ? 2 : 1)), dim3(512), smem_b, st, a);
    return sdmi_check_launch("st_block (phase B)");
  }
  return SDMI_OK;
}

}  // namespace

extern "C" int sdmi_st_block(const SdmiStBlockArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->x && a->tok && a->qkv && a->out, "null pointer");
  SDMI_REQUIRE(a->wstream_a && a->vec_a && a->wstream_b && a->wstream_img && a->vec_b && a->vec_img, "null stream");
  SDMI_REQUIRE(a->C == 256 || a->C == 384, "C must be 256 or 384");
  SDMI_REQUIRE(a->rows == 0 || a->rows == 64 || a->rows == 32, "rows per workgroup: 64 (0) or 32");
  const int rows = a->rows ? a->rows : 64;
  SDMI_REQUIRE(a->S >= rows && a->S % rows == 0 && a->S % 32 == 0 && 4 * a->S * (ST_KP + ST_VP) <= 160 * 1024,
               "S must be a multiple of the rows per workgroup and at most 256 tokens per image");
  SDMI_REQUIRE(a->slots >= 1 && (a->slots <= 8 || (a->slots <= 16 && a->C == 256)),
               "1..8 slots (C = 256: up to 16, in 16-column score groups)");
  SDMI_REQUIRE(a->phase >= 0 && a->phase <= 2, "phase: 0 = both, 1 = A, 2 = B");
  SDMI_REQUIRE(a->ff_split == 0 || a->ff_split == 1 || (a->ff_split == 2 && a->part), "ff_split: 0 / 1, or 2 with a partials buffer");
  hipStream_t st = (hipStream_t)stream;
  if (rows == 64) return a->C == 256 ? st_launch<256, 4>(*a, st) : st_launch<384, 4>(*a, st);
  return a->C == 256 ? st_launch<256, 2>(*a, st) : st_launch<384, 2>(*a, st);
}
