// Physion VQA readout (sdmi.h: sdmi_readout_fwd / sdmi_readout_bwd; the reference's vp_vqa/models/readout.py:56-87).
//
// forward, launch 1 (readout_frames_kernel): a workgroup owns R = 32 RB slot rows = R / N whole frames (rows past the
//   last whole frame are zero) staged in LDS in the operand dtype; wave w owns features [32 w, 32 w + 32) and computes
//   the 32 x 32 tiles U = S W_a^T and V = S W_b^T of every row block with W1 streamed from L2 in MFMA B-fragment order.
//   In the 32 x 32 accumulator layout a feature's 32 rows sit in lanes l and l + 32: one exchange gives every lane its
//   feature's whole column, and the pair aggregate is a walk down that column in registers (prefix max of U for max,
//   fixed weights for sum / mean).  (m + b1) w2 is summed over the 32 features of the wave by shuffles and over the
//   waves through LDS, in a fixed order (in fp64, rounded to fp32 once).  With fp32 operands U, V (8-k MFMA chunks) and
//   the aggregate are carried in fp64 as well; with bf16 operands they are fp32.
// forward, launch 2 (readout_finish_kernel): one workgroup; a wave per sample takes the max over time (lowest t on
//   ties), lane 0 the loss terms; the loss is summed in a fixed order.
// backward (readout_bwd_kernel): one wave per feature walks the samples in order (see sdmi.h).
#include <limits.h>
#include <type_traits>
#include "common.h"

namespace {

constexpr int RO_FIN_THREADS = 256;

__device__ __forceinline__ float ro_round(float v, bool op_bf16) {
  return op_bf16 ? bf16_to_f32(f32_to_bf16(v)) : v;
}

// four consecutive elements of a slot row (idx a multiple of 4), as floats
__device__ __forceinline__ void ro_load4(const void* base, long long idx, bool x_bf16, float* f) {
  if (x_bf16) {
    const uint2 v = *reinterpret_cast<const uint2*>((const bf16_t*)base + idx);
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  } else {
    const float4 v = *reinterpret_cast<const float4*>((const float*)base + idx);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  }
}
__device__ __forceinline__ float ro_load1(const void* base, long long idx, bool x_bf16) {
  return x_bf16 ? bf16_to_f32(((const bf16_t*)base)[idx]) : ((const float*)base)[idx];
}

// ------------------------------------------------------------------------------------------
// forward, launch 1
// ------------------------------------------------------------------------------------------
template <bool BF16, int RB>
__global__ __launch_bounds__(512) void readout_frames_kernel(SdmiReadoutFwdArgs p) {
  typedef typename std::conditional<BF16, bf16_t, float>::type OpT;
  constexpr int R = 32 * RB;
  constexpr int PADE = BF16 ? 8 : 4;                 // 16 bytes: consecutive rows start on different banks
  extern __shared__ __attribute__((aligned(16))) unsigned char ro_smem[];
  const int C = p.C, N = p.N, F = p.F;
  const int lda = C + PADE;
  OpT* As = reinterpret_cast<OpT*>(ro_smem);
  double* part = reinterpret_cast<double*>(ro_smem + (size_t)R * lda * sizeof(OpT));    // [waves][R / 2]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x;
  const int fpt = R / N;                              // whole frames per tile
  const int rows_used = fpt * N;
  const long long frames = (long long)p.B * p.T;
  const long long frame0 = (long long)blockIdx.x * fpt;
  const long long row0 = frame0 * N, rows_total = frames * N;
  const bool x_bf16 = p.x_dtype == SDMI_BF16;

  // ---- stage the tile's slot rows (operand dtype), zeros past the last real row
  const int c4n = C >> 2;
  for (int idx = tid; idx < R * c4n; idx += nthr) {
    const int r = idx / c4n, c = (idx - r * c4n) << 2;
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < rows_used && row0 + r < rows_total) ro_load4(p.slots, (row0 + r) * C + c, x_bf16, f);
    if constexpr (BF16) {
      *reinterpret_cast<uint2*>(As + r * lda + c) = make_uint2(f32x2_to_bf16x2(f[0], f[1]), f32x2_to_bf16x2(f[2], f[3]));
    } else {
      *reinterpret_cast<float4*>(As + r * lda + c) = make_float4(f[0], f[1], f[2], f[3]);
    }
  }
  __syncthreads();

  // ---- U | V tiles of this wave's 32 features.  bf16 operands: fp32 accumulators.  fp32 operands (the parity
  // configuration): the MFMA sums 8 k at a time in fp32 and the chunks are carried in fp64, as is the aggregate below --
  // a 256-term fp32 dot product alone is 3e-7 of the logit's magnitude off (3e-5 at the sum aggregate of 16 slots)
  typedef typename std::conditional<BF16, float, double>::type AggT;
  const int l31 = lane & 31, half = lane >> 5;
  AggT accU[RB][16], accV[RB][16];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) { accU[rb][i] = 0; accV[rb][i] = 0; }
  if constexpr (BF16) {
    const int KS = C >> 4;
    const uint4* wp = reinterpret_cast<const uint4*>(p.w1p) + (size_t)wave * KS * 128 + lane;
    f32x16 cu[RB], cv[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int i = 0; i < 16; ++i) { cu[rb][i] = 0.f; cv[rb][i] = 0.f; }
    for (int ks = 0; ks < KS; ++ks) {
      const uint4 bu = wp[(size_t)ks * 128], bv = wp[(size_t)ks * 128 + 64];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const uint4 a = *reinterpret_cast<const uint4*>(As + (rb * 32 + l31) * lda + ks * 16 + half * 8);
        cu[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bu),
                                                         cu[rb], 0, 0, 0);
        cv[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bv),
                                                         cv[rb], 0, 0, 0);
      }
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int i = 0; i < 16; ++i) { accU[rb][i] = cu[rb][i]; accV[rb][i] = cv[rb][i]; }
  } else {
    const int KG = C >> 3;
    const float4* wp = reinterpret_cast<const float4*>(p.w1p) + (size_t)wave * KG * 128 + lane;
    for (int kg = 0; kg < KG; ++kg) {
      const float4 bu = wp[(size_t)kg * 128], bv = wp[(size_t)kg * 128 + 64];
      const float bua[4] = {bu.x, bu.y, bu.z, bu.w}, bva[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const float4 a = *reinterpret_cast<const float4*>(As + (rb * 32 + l31) * lda + kg * 8 + half * 4);
        const float aa[4] = {a.x, a.y, a.z, a.w};
        f32x16 cu, cv;
#pragma unroll
        for (int i = 0; i < 16; ++i) { cu[i] = 0.f; cv[i] = 0.f; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          cu = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[j], bua[j], cu, 0, 0, 0);
          cv = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[j], bva[j], cv, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) { accU[rb][i] += (double)cu[i]; accV[rb][i] += (double)cv[i]; }
      }
    }
  }

  // ---- every lane gets its feature's whole column: register i of lane half h is row 8 (i / 4) + 4 h + i % 4
  AggT U[R], V[R];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const AggT ou = accU[rb][4 * g + w], ov = accV[rb][4 * g + w];
        const AggT xu = __shfl_xor(ou, 32, 64), xv = __shfl_xor(ov, 32, 64);
        U[rb * 32 + 8 * g + w] = half ? xu : ou;
        U[rb * 32 + 8 * g + 4 + w] = half ? ou : xu;
        V[rb * 32 + 8 * g + w] = half ? xv : ov;
        V[rb * 32 + 8 * g + 4 + w] = half ? ov : xv;
      }

  // ---- pair aggregate down the column, linear2 partial of the wave's 32 features
  const int f = wave * 32 + l31;
  const int P = N * (N - 1) / 2;
  const AggT w2f = p.w2[f];
  const AggT b1f = (AggT)p.b1[f] * (p.agg == SDMI_AGG_SUM ? (AggT)P : (AggT)1);
  AggT pm = 0, best = 0, s = 0;
  int i = 0, fl = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r < rows_used) {                              // (wave-uniform: r is a constant, N a kernel argument)
      if (i == 0) {
        pm = U[r];
        best = -INFINITY;
        s = (AggT)(N - 1) * U[r];
      } else {
        best = fmax(best, pm + V[r]);
        pm = fmax(pm, U[r]);
        s += (AggT)(N - 1 - i) * U[r] + (AggT)i * V[r];
      }
      if (++i == N) {
        const AggT m = p.agg == SDMI_AGG_MAX ? best : (p.agg == SDMI_AGG_MEAN ? s / (AggT)P : s);
        // linear2: the F-term sum of the products is carried in fp64 and rounded once (the products cancel: a chain
        // of fp32 additions alone moves a sum-aggregate logit by 1e-5)
        double v = (double)((m + b1f) * w2f);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) part[wave * (R / 2) + fl] = v;
        ++fl;
        i = 0;
      }
    }
  }
  __syncthreads();
  if (tid < fpt && frame0 + tid < frames) {
    const int nw = F >> 5;
    double v = part[tid];
    for (int w = 1; w < nw; ++w) v += part[w * (R / 2) + tid];
    p.frame_logits[frame0 + tid] = (float)(v + (double)p.b2[0]);
  }
}

// ------------------------------------------------------------------------------------------
// forward, launch 2: max over time, t_star, BCE-with-logits and its gradient
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RO_FIN_THREADS) void readout_finish_kernel(SdmiReadoutFwdArgs p) {
  __shared__ float wsum[RO_FIN_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int NW = RO_FIN_THREADS / 64;
  const int B = p.B, T = p.T;
  float lsum = 0.f;                                   // lane 0: loss terms of this wave's samples, in b order
  for (int b = wave; b < B; b += NW) {
    const float* fr = p.frame_logits + (long long)b * T;
    float v = -INFINITY;
    int t = INT_MAX;
    for (int tt = lane; tt < T; tt += 64) {
      const float x = fr[tt];
      if (x > v || t == INT_MAX) { v = x; t = tt; }   // strict: the lowest t of a lane's equal values stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int ot = __shfl_xor(t, o, 64);
      if (ot != INT_MAX && (t == INT_MAX || ov > v || (ov == v && ot < t))) { v = ov; t = ot; }
    }
    if (lane == 0) {
      t = t == INT_MAX ? 0 : t;
      p.logits[b] = v;
      p.t_star[b] = t;
      if (p.label) {
        const float y = p.label[b];
        lsum += fmaxf(v, 0.f) - v * y + log1pf(expf(-fabsf(v)));
        p.dlogit[b] = p.loss_weight * (1.f / (1.f + expf(-v)) - y) / (float)B;
      }
    }
  }
  if (p.label) {
    if (lane == 0) wsum[wave] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) {
      float tot = 0.f;
      for (int w = 0; w < NW; ++w) tot += wsum[w];
      p.loss[0] = p.loss_weight * tot / (float)B;
    }
  }
}

// ------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------
// pair p of itertools.combinations(range(N), 2) -> (i, j)
__device__ __forceinline__ void ro_pair(int pidx, int N, int& i, int& j) {
  i = 0;
  int rem = pidx;
  while (i < N - 2 && rem >= N - 1 - i) { rem -= N - 1 - i; ++i; }
  j = i + 1 + rem;
  j = j < N ? j : N - 1;
}

// element (f, col) of W1 [F][2C] inside the packed operand (sdmi.h)
__device__ __forceinline__ float ro_w1(const void* w1p, int f, int col, int C, bool op_bf16) {
  const int h = col >= C, k = col - h * C, fc = f >> 5, fr = f & 31;
  if (op_bf16) {
    const size_t idx = ((((size_t)fc * (C >> 4) + (k >> 4)) * 2 + h) * 64 + fr + 32 * ((k >> 3) & 1)) * 8 + (k & 7);
    return bf16_to_f32(((const bf16_t*)w1p)[idx]);
  }
  const size_t idx = ((((size_t)fc * (C >> 3) + (k >> 3)) * 2 + h) * 64 + fr + 32 * ((k >> 2) & 1)) * 4 + (k & 3);
  return ((const float*)w1p)[idx];
}

__global__ __launch_bounds__(256) void readout_bwd_kernel(SdmiReadoutBwdArgs p) {
  __shared__ float wsh[4][512];                       // per wave: W_a[f][0 .. C) | W_b[f][0 .. C)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = p.C, N = p.N, B = p.B, T = p.T;
  const int f = blockIdx.x * 4 + wave;                // F is a multiple of 32: every wave has a feature
  const bool x_bf16 = p.x_dtype == SDMI_BF16, op_bf16 = p.op_dtype == SDMI_BF16;
  float* wa = wsh[wave];
  float* wb = wa + C;
  for (int c = lane; c < 2 * C; c += 64) wa[c] = ro_w1(p.w1p, f, c, C, op_bf16);
  __syncthreads();
  const int P = N * (N - 1) / 2;
  const int r = lane & 15, seg = lane >> 4, sl = C >> 2;          // slot row, quarter of the C range
  const float w2f = p.w2[f], b1f = p.b1[f];
  const float gs = p.gscale ? p.gscale[0] : 1.f;
  int pi[2], pj[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) ro_pair(min(lane + 64 * q, P - 1), N, pi[q], pj[q]);
  const float scale = p.agg == SDMI_AGG_MEAN ? 1.f / (float)P : 1.f;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  float db1 = 0.f, dw2 = 0.f, db2 = 0.f;
#pragma unroll 1
  for (int b = 0; b < B; ++b) {
    int t = p.t_star[b];
    t = t < 0 ? 0 : (t >= T ? T - 1 : t);             // (a t_star from elsewhere never reads outside the sample)
    const float g = p.dlogit[b] * gs;
    const long long base = ((long long)b * T + t) * N * C;
    // ---- U_r, V_r of this feature: four lanes per slot row
    float pu = 0.f, pv = 0.f;
    if (r < N) {
      const long long ro = base + (long long)r * C + seg * sl;
      for (int k = 0; k < sl; k += 4) {
        float x[4];
        ro_load4(p.slots, ro + k, x_bf16, x);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xv = ro_round(x[e], op_bf16);
          pu = fmaf(wa[seg * sl + k + e], xv, pu);
          pv = fmaf(wb[seg * sl + k + e], xv, pv);
        }
      }
    }
    pu += __shfl_xor(pu, 16, 64); pu += __shfl_xor(pu, 32, 64);
    pv += __shfl_xor(pv, 16, 64); pv += __shfl_xor(pv, 32, 64);
    const float gf = g * w2f;
    float m;
    if (p.agg == SDMI_AGG_MAX) {
      // ---- the winning pair: two pairs per lane, ties to the lower pair index
      float v = -INFINITY;
      int pb = INT_MAX;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float cand = __shfl(pu, pi[q], 64) + __shfl(pv, pj[q], 64);
        const int pidx = lane + 64 * q;
        if (pidx < P && (pb == INT_MAX || cand > v)) { v = cand; pb = pidx; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int ob = __shfl_xor(pb, o, 64);
        if (ob != INT_MAX && (pb == INT_MAX || ov > v || (ov == v && ob < pb))) { v = ov; pb = ob; }
      }
      pb = __builtin_amdgcn_readfirstlane(pb);
      v = __shfl(v, 0, 64);
      pb = pb < 0 ? 0 : (pb > P - 1 ? P - 1 : pb);
      int is, js;
      ro_pair(pb, N, is, js);
      m = v + b1f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c2 = lane + 64 * k;
        if (c2 < 2 * C) {
          const long long src = c2 < C ? base + (long long)is * C + c2 : base + (long long)js * C + (c2 - C);
          acc[k] = fmaf(gf, ro_round(ro_load1(p.slots, src, x_bf16), op_bf16), acc[k]);
        }
      }
      db1 += gf;
    } else {
      // ---- sum / mean: fixed weights (N-1-i) on U_i, j on V_j
      float c = (seg == 0 && r < N) ? (float)(N - 1 - r) * pu + (float)r * pv : 0.f;
      c = wave_sum(c);
      m = c * scale + b1f * (p.agg == SDMI_AGG_SUM ? (float)P : 1.f);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c2 = lane + 64 * k;
        if (c2 < 2 * C) {
          const bool first = c2 < C;
          const int cc = first ? c2 : c2 - C;
          float sx = 0.f;
          for (int i = 0; i < N; ++i)
            sx = fmaf((float)(first ? N - 1 - i : i),
                      ro_round(ro_load1(p.slots, base + (long long)i * C + cc, x_bf16), op_bf16), sx);
          acc[k] = fmaf(gf * scale, sx, acc[k]);
        }
      }
      db1 += gf * (p.agg == SDMI_AGG_SUM ? (float)P : 1.f);
    }
    dw2 = fmaf(g, m, dw2);
    db2 += g;
  }
  const bool add = p.accumulate != 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c2 = lane + 64 * k;
    if (c2 < 2 * C) {
      float* d = p.dw1 + (size_t)f * 2 * C + c2;
      *d = add ? *d + acc[k] : acc[k];
    }
  }
  if (lane == 0) {
    p.db1[f] = add ? p.db1[f] + db1 : db1;
    p.dw2[f] = add ? p.dw2[f] + dw2 : dw2;
    if (f == 0) p.db2[0] = add ? p.db2[0] + db2 : db2;
  }
}

template <bool BF16, int RB>
int readout_frames_launch(const SdmiReadoutFwdArgs& a, hipStream_t st) {
  constexpr int R = 32 * RB;
  const int lda = a.C + (BF16 ? 8 : 4);
  const int smem = R * lda * (BF16 ? 2 : 4) + (a.F / 32) * (R / 2) * 8;
  const int fpt = R / a.N;
  const long long tiles = ((long long)a.B * a.T + fpt - 1) / fpt;
  if (tiles > INT_MAX) {
    sdmi_set_error("sdmi_readout_fwd: B T too large for one grid");
    return SDMI_EINVAL;
  }
  hipLaunchKernelGGL((readout_frames_kernel<BF16, RB>), dim3((unsigned)tiles), dim3(64 * (a.F / 32)), smem, st, a);
  return sdmi_check_launch("sdmi_readout_fwd (frames)");
}

bool ro_dtype_ok(int d) { return d == SDMI_F32 || d == SDMI_BF16; }

}  // namespace

#define RO_GEOMETRY(a)                                                                                          \
  SDMI_REQUIRE((a)->B >= 1 && (a)->T >= 1, "empty batch or no frames");                                         \
  SDMI_REQUIRE((a)->N >= 2 && (a)->N <= 16, "2 <= N <= 16");                                                    \
  SDMI_REQUIRE((a)->C >= 32 && (a)->C <= 256 && (a)->C % 32 == 0, "C must be a multiple of 32, at most 256");   \
  SDMI_REQUIRE((a)->F >= 32 && (a)->F <= 256 && (a)->F % 32 == 0, "F must be a multiple of 32, at most 256");   \
  SDMI_REQUIRE((a)->agg >= SDMI_AGG_SUM && (a)->agg <= SDMI_AGG_MAX, "agg: 0 sum, 1 mean, 2 max");              \
  SDMI_REQUIRE(ro_dtype_ok((a)->x_dtype) && ro_dtype_ok((a)->op_dtype), "x_dtype / op_dtype: fp32 or bf16");    \
  SDMI_REQUIRE(((uintptr_t)(a)->slots & 15) == 0 && ((uintptr_t)(a)->w1p & 15) == 0, "slots / w1p must be 16-byte aligned")

extern "C" int sdmi_readout_fwd(const SdmiReadoutFwdArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->slots && a->w1p && a->b1 && a->w2 && a->b2, "null input pointer");
  SDMI_REQUIRE(a->frame_logits && a->logits && a->t_star, "null output pointer");
  SDMI_REQUIRE(!a->label || (a->loss && a->dlogit), "label given without loss / dlogit");
  RO_GEOMETRY(a);
  SDMI_REQUIRE(a->phase >= 0 && a->phase <= 2, "phase: 0 = both, 1 = frame logits, 2 = finisher");
  hipStream_t st = (hipStream_t)stream;
  if (a->phase == 0 || a->phase == 1) {
    const int rc = a->op_dtype == SDMI_BF16 ? readout_frames_launch<true, 2>(*a, st) : readout_frames_launch<false, 1>(*a, st);
    if (rc) return rc;
  }
  if (a->phase == 0 || a->phase == 2) {
    hipLaunchKernelGGL(readout_finish_kernel, dim3(1), dim3(RO_FIN_THREADS), 0, st, *a);
    return sdmi_check_launch("sdmi_readout_fwd (finisher)");
  }
  return SDMI_OK;
}

extern "C" int sdmi_readout_bwd(const SdmiReadoutBwdArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->slots && a->w1p && a->b1 && a->w2, "null input pointer");
  SDMI_REQUIRE(a->t_star && a->dlogit, "null t_star / dlogit");
  SDMI_REQUIRE(a->dw1 && a->db1 && a->dw2 && a->db2, "null gradient pointer");
  RO_GEOMETRY(a);
  hipLaunchKernelGGL(readout_bwd_kernel, dim3(a->F / 4), dim3(256), 0, (hipStream_t)stream, *a);
  return sdmi_check_launch("sdmi_readout_bwd");
}
