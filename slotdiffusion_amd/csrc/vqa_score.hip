// Physion VQA test stage (sdmi.h: sdmi_vqa_score; the reference's vp_vqa/test_physion_vqa.py): a bank of W readout
// checkpoints and K thresholds scored on a batch of videos in ONE launch.
//
// A workgroup owns one (video b, checkpoint w): grid (B, W), so neighbouring workgroups share a checkpoint's W1 in L2
// and a video's slots are re-read per checkpoint from L2.  It walks the video's T N slot rows through LDS in chunks of
// R = 32 RB rows = R / N whole frames (rows past the last whole frame, and past the video's end, are zero); per chunk
// it is readout_frames_kernel (readout.hip) statement for statement -- wave v owns features [32 v, 32 v + 32), W1 is
// streamed from L2 in MFMA B-fragment order, one lane exchange gives every lane its feature's column, the pair
// aggregate walks down it in registers, linear2 is summed over the 32 features by shuffles and over the waves through
// LDS in fp64 -- so a frame's logit has the bits sdmi_readout_fwd gives it (a frame's logit there does not depend on
// the tile it landed in).  Thread i < R / N keeps the running time max of frames i, i + R / N, .. (lowest t on equal
// values, as readout_finish_kernel), wave 0 reduces them by that same rule, and K lanes do the strict compares against
// the cuts and one integer atomic each into correct[w][k][task[b]].  No floating-point atomics, no workspace, no
// cross-workgroup combination: logits and table do not depend on execution order.
//
// W1's fragments are re-streamed from L2 per chunk rather than held: at C = 256 they alone are 128 VGPRs per lane, on
// top of the U[R] | V[R] columns and the accumulators the walk needs (see the counts below), and the per-chunk stream
// is what readout_frames_kernel pays per tile as well.
//
// Compiler resource report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   vqa_score_kernel<true, 2>  (bf16 operands, 64-row chunks): 166 VGPRs, 0 AGPRs, scratch 0, 3 waves / SIMD
//   vqa_score_kernel<false, 1> (fp32 operands, 32-row chunks): 176 VGPRs, 0 AGPRs, scratch 0, 2 waves / SIMD
// LDS is dynamic: R (C + pad) operand elements + (F / 32) (R / 2) doubles, 35840 bytes (bf16) / 34304 bytes (fp32) at
// C = F = 256.
#include <limits.h>
#include <type_traits>
#include "common.h"

namespace {

// four consecutive elements of a slot row (idx a multiple of 4), as floats
__device__ __forceinline__ void vq_load4(const void* base, long long idx, bool x_bf16, float* f) {
  if (x_bf16) {
    const uint2 v = *reinterpret_cast<const uint2*>((const bf16_t*)base + idx);
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  } else {
    const float4 v = *reinterpret_cast<const float4*>((const float*)base + idx);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  }
}

template <bool BF16, int RB>
__global__ __launch_bounds__(512) void vqa_score_kernel(SdmiVqaScoreArgs p) {
  typedef typename std::conditional<BF16, bf16_t, float>::type OpT;
  constexpr int R = 32 * RB;
  constexpr int PADE = BF16 ? 8 : 4;                 // 16 bytes: consecutive rows start on different banks
  extern __shared__ __attribute__((aligned(16))) unsigned char vq_smem[];
  const int C = p.C, N = p.N, F = p.F, T = p.T;
  const int lda = C + PADE;
  OpT* As = reinterpret_cast<OpT*>(vq_smem);
  double* part = reinterpret_cast<double*>(vq_smem + (size_t)R * lda * sizeof(OpT));    // [waves][R / 2]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x;
  const int b = blockIdx.x, ck = blockIdx.y;
  const int fpt = R / N;                              // whole frames per chunk
  const int rows_used = fpt * N;
  const int rows_video = T * N;
  const bool x_bf16 = p.x_dtype == SDMI_BF16;
  const long long vbase = (long long)b * rows_video * C;              // first element of this video's slots
  const OpT* w1p = reinterpret_cast<const OpT*>(p.w1p) + (size_t)ck * F * 2 * C;
  const float* b1 = p.b1 + (size_t)ck * F;
  const float* w2 = p.w2 + (size_t)ck * F;
  const double b2 = (double)p.b2[ck];

  typedef typename std::conditional<BF16, float, double>::type AggT;
  const int l31 = lane & 31, half = lane >> 5;
  const int f = wave * 32 + l31;
  const int P = N * (N - 1) / 2;
  const AggT w2f = w2[f];
  const AggT b1f = (AggT)b1[f] * (p.agg == SDMI_AGG_SUM ? (AggT)P : (AggT)1);
  const int nw = F >> 5;
  const int c4n = C >> 2;

  float tv = -INFINITY;                               // thread i < fpt: time max of frames i, i + fpt, ..
  int tt = INT_MAX;

#pragma unroll 1
  for (int frame0 = 0; frame0 < T; frame0 += fpt) {
    const int row0 = frame0 * N;
    // ---- stage the chunk's slot rows (operand dtype), zeros past the last real row
    for (int idx = tid; idx < R * c4n; idx += nthr) {
      const int r = idx / c4n, c = (idx - r * c4n) << 2;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (r < rows_used && row0 + r < rows_video) vq_load4(p.slots, vbase + (long long)(row0 + r) * C + c, x_bf16, v);
      if constexpr (BF16) {
        *reinterpret_cast<uint2*>(As + r * lda + c) = make_uint2(f32x2_to_bf16x2(v[0], v[1]), f32x2_to_bf16x2(v[2], v[3]));
      } else {
        *reinterpret_cast<float4*>(As + r * lda + c) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    __syncthreads();

    // ---- U | V tiles of this wave's 32 features: bf16 operands in fp32 accumulators; fp32 operands in 8-k MFMA chunks
    // carried in fp64 (readout.hip)
    AggT accU[RB][16], accV[RB][16];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int i = 0; i < 16; ++i) { accU[rb][i] = 0; accV[rb][i] = 0; }
    if constexpr (BF16) {
      const int KS = C >> 4;
      const uint4* wp = reinterpret_cast<const uint4*>(w1p) + (size_t)wave * KS * 128 + lane;
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
      const float4* wp = reinterpret_cast<const float4*>(w1p) + (size_t)wave * KG * 128 + lane;
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
    // ---- the chunk's frame logits, folded into the running time max (strict: the lowest t of equal values stays)
    if (tid < fpt && frame0 + tid < T) {
      double v = part[tid];
      for (int w = 1; w < nw; ++w) v += part[w * (R / 2) + tid];
      const float x = (float)(v + b2);
      if (x > tv || tt == INT_MAX) { tv = x; tt = frame0 + tid; }
    }
    // (the next chunk's writes to `part` come after its staging barrier, which these reads precede)
  }

  // ---- max over time (fpt <= 32: all candidates sit in wave 0), then K lanes score the thresholds
  if (wave == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(tv, o, 64);
      const int ot = __shfl_xor(tt, o, 64);
      if (ot != INT_MAX && (tt == INT_MAX || ov > tv || (ov == tv && ot < tt))) { tv = ov; tt = ot; }
    }
    if (lane == 0) p.logits[(long long)ck * p.B + b] = tv;
    const int task = p.task[b];
    if (lane < p.K && task >= 0 && task < p.J) {        // (a task outside [0, J) is counted nowhere)
      const bool yes = tv > p.cut[lane];
      if (yes == (p.label[b] != 0.f)) atomicAdd(p.correct + ((long long)ck * p.K + lane) * p.J + task, 1);
    }
  }
}

template <bool BF16, int RB>
int vqa_score_launch(const SdmiVqaScoreArgs& a, hipStream_t st) {
  constexpr int R = 32 * RB;
  const int lda = a.C + (BF16 ? 8 : 4);
  const int smem = R * lda * (BF16 ? 2 : 4) + (a.F / 32) * (R / 2) * 8;
  hipLaunchKernelGGL((vqa_score_kernel<BF16, RB>), dim3((unsigned)a.B, (unsigned)a.W), dim3(64 * (a.F / 32)), smem, st, a);
  return sdmi_check_launch("sdmi_vqa_score");
}

bool vq_dtype_ok(int d) { return d == SDMI_F32 || d == SDMI_BF16; }

}  // namespace

extern "C" int sdmi_vqa_score(const SdmiVqaScoreArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->slots && a->w1p && a->b1 && a->w2 && a->b2, "null input pointer");
  SDMI_REQUIRE(a->label && a->task && a->cut, "null label / task / cut");
  SDMI_REQUIRE(a->logits && a->correct, "null output pointer");
  SDMI_REQUIRE(a->B >= 1 && a->T >= 1, "empty batch or no frames");
  SDMI_REQUIRE(a->N >= 2 && a->N <= 16, "2 <= N <= 16");
  SDMI_REQUIRE(a->C >= 32 && a->C <= 256 && a->C % 32 == 0, "C must be a multiple of 32, at most 256");
  SDMI_REQUIRE(a->F >= 32 && a->F <= 256 && a->F % 32 == 0, "F must be a multiple of 32, at most 256");
  SDMI_REQUIRE(a->agg >= SDMI_AGG_SUM && a->agg <= SDMI_AGG_MAX, "agg: 0 sum, 1 mean, 2 max");
  SDMI_REQUIRE(vq_dtype_ok(a->x_dtype) && vq_dtype_ok(a->op_dtype), "x_dtype / op_dtype: fp32 or bf16");
  SDMI_REQUIRE(((uintptr_t)a->slots & 15) == 0 && ((uintptr_t)a->w1p & 15) == 0, "slots / w1p must be 16-byte aligned");
  SDMI_REQUIRE(a->W >= 1 && a->W <= 65535, "1 <= W <= 65535 checkpoints");
  SDMI_REQUIRE(a->K >= 1 && a->K <= 32, "1 <= K <= 32 thresholds");
  SDMI_REQUIRE(a->J >= 1 && a->J <= 64, "1 <= J <= 64 tasks");
  SDMI_REQUIRE((long long)a->T * a->N < (1LL << 24), "T N too large");
  hipStream_t st = (hipStream_t)stream;
  return a->op_dtype == SDMI_BF16 ? vqa_score_launch<true, 2>(*a, st) : vqa_score_launch<false, 1>(*a, st);
}
