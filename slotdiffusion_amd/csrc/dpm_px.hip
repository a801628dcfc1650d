// The image-space tail of one function evaluation (include/sdmi.h: sdmi_dpm_step_px, sdmi_unipc_step_px): data
// prediction, correction of x0 (none / clamp / dynamic thresholding), m0, solver update -- one launch.
//
// Dynamic thresholding needs, per sample, the p-quantile of |x0| over n = 3 * rows_per_sample values.  torch.quantile
// sorts; two order statistics are enough, and a most-significant-digit radix select over the bit patterns of |x0|
// (non-negative floats: unsigned order = value order) finds them exactly.  One workgroup of 1024 threads owns a sample
// and keeps its prediction in registers from the load to the last store (NR rows of 3 values per thread: 48 values at
// 128 x 128), so every input row is read once, every output row written once, and |x0| never goes to memory.
//
// Counting: four passes of 8-bit digits into ONE 256-bin LDS histogram.  The top byte of a float is mostly exponent, so
// in the first pass nearly every key of a wave falls into one or two bins (and a constant or coarsely quantised sample
// does the same in every pass); 64 lanes adding 1 to one LDS word serialise.  So each wave pre-aggregates: the digit of
// the first active lane is broadcast, its holders are counted with one ballot and added by one lane, twice; only what
// is left after the two heaviest digits goes through per-lane atomics.  From the second pass on only the keys that
// share the prefix found so far take part, which is a small fraction.  After each pass wave 0 scans the histogram
// (4 bins per lane, one wave prefix sum) for the bin that holds rank k.  The second order statistic needs no further
// select: it is the found key again when more than k + 1 keys are <= it, otherwise the smallest larger key (one
// count + min reduction over the registers).
//
// Compiled with -ffp-contract=off like vq.hip / elementwise.hip: every expression rounds like the launch chain's.
#include "common.h"
#include "dpm_tail.h"

namespace {

constexpr int PX_T = 1024;                               // threads per sample (16 waves: <= 128 VGPRs)
static_assert(16 * PX_T == SDMI_PX_MAX_ROWS, "register-resident limit: 16 rows per thread");

__device__ __forceinline__ void px_update_row(const SdmiDpmStepPxArgs& p, long long ro, const f32x4& m) {
  dpm_update_row(p, ro, m);
}
__device__ __forceinline__ void px_update_row(const SdmiUnipcStepPxArgs& p, long long ro, const f32x4& m) {
  unipc_update_row(p, ro, m);
}

// The front half's first step, shared by every kernel here: sdmi_dpm_step's data prediction of one row.
template <typename P>
__device__ __forceinline__ void px_predict_row(const P& p, long long ro, float (&v)[3]) {
  const f32x4 xv = *reinterpret_cast<const f32x4*>(p.x + ro);
  const float* o = p.out + ro;                           // (the pad channel of the network output is never read)
  v[0] = dpm_x0(p.target, p.sigma, p.alpha, xv[0], o[0]);
  v[1] = dpm_x0(p.target, p.sigma, p.alpha, xv[1], o[1]);
  v[2] = dpm_x0(p.target, p.sigma, p.alpha, xv[2], o[2]);
}

__device__ __forceinline__ float px_clamp(float v, float lo, float hi) {   // torch.clamp: a NaN stays a NaN
  return v < lo ? lo : (v > hi ? hi : v);
}

// NONE / CLAMP need nothing from the rest of the sample: one row per thread, any number of rows.
template <typename P>
__global__ __launch_bounds__(256) void px_rows_kernel(P p) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= p.R) return;
  const long long ro = r * 4;
  float v[3];
  px_predict_row(p, ro, v);
  if (p.correct == SDMI_X0_CLAMP) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = px_clamp(v[c], -1.0f, 1.0f);
  }
  const f32x4 m = {v[0], v[1], v[2], 0.f};
  *reinterpret_cast<f32x4*>(p.m0 + ro) = m;
  px_update_row(p, ro, m);
}

// hist[digit] += 1 for every lane with act, the wave's two most likely heavy digits through one add each
__device__ __forceinline__ void px_hist_add(unsigned* hist, unsigned digit, bool act, int lane) {
  unsigned long long todo = __ballot(act);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (todo == 0) break;                                // wave-uniform
    const int lead = __ffsll((long long)todo) - 1;
    const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)digit, lead);
    const unsigned long long same = __ballot(act && digit == d0);
    if (lane == lead) atomicAdd(&hist[d0], (unsigned)__popcll(same));
    act = act && digit != d0;
    todo &= ~same;
  }
  if (act) atomicAdd(&hist[digit], 1u);
}

template <int NR, typename P>
__global__ __launch_bounds__(PX_T) void px_dynamic_kernel(P p) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sel[2];                            // the key prefix found so far, the rank inside it
  __shared__ unsigned red_cnt[PX_T / 64], red_min[PX_T / 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rps = p.rows_per_sample;
  const long long row0 = (long long)blockIdx.x * rps;

  // ---- data prediction, kept in registers ----
  float v[NR][3];
  int bad = 0;
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int lr = tid + j * PX_T;
    v[j][0] = v[j][1] = v[j][2] = 0.f;
    if (lr < rps) {
      px_predict_row(p, (row0 + lr) * 4, v[j]);
#pragma unroll
      for (int c = 0; c < 3; ++c) bad |= (__float_as_uint(v[j][c]) & 0x7fffffffu) > 0x7f800000u;
    }
  }
  const bool any_nan = __syncthreads_or(bad) != 0;

  // ---- s = quantile(|x0|, p): radix select of rank q_k over the keys, most significant byte first ----
  float s = __uint_as_float(0x7fc00000u);
  if (!any_nan) {                                        // workgroup-uniform
    unsigned prefix = 0, k = (unsigned)p.q_k;
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const bool valid = tid + j * PX_T < rps;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const unsigned key = __float_as_uint(v[j][c]) & 0x7fffffffu;
          const bool act = valid && (pass == 0 || (key >> (shift + 8)) == prefix);
          px_hist_add(hist, (key >> shift) & 255u, act, lane);
        }
      }
      __syncthreads();
      if (wave == 0) {                                   // bins 4 * lane .. 4 * lane + 3
        const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
        const unsigned own = h0 + h1 + h2 + h3;
        unsigned incl = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const unsigned up = (unsigned)__shfl_up((int)incl, d);
          if (lane >= d) incl += up;
        }
        unsigned below = incl - own;
        if (k >= below && k < incl) {                    // exactly one lane: the keys counted are more than k
          unsigned bin = 4 * lane;
          if (k >= below + h0) { below += h0; ++bin;
            if (k >= below + h1) { below += h1; ++bin;
              if (k >= below + h2) { below += h2; ++bin; } } }
          sel[0] = (prefix << 8) | bin;
          sel[1] = k - below;
        }
      }
      __syncthreads();
      prefix = sel[0];
      k = sel[1];
    }
    const unsigned klo = prefix;                         // the bits of a_(q_k)
    unsigned khi = klo;
    if (p.q_w != 0.f) {                                  // a_(q_k + 1): klo again, or the next larger key
      unsigned cnt = 0, mn = 0xffffffffu;
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const bool valid = tid + j * PX_T < rps;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const unsigned key = __float_as_uint(v[j][c]) & 0x7fffffffu;
          if (valid) {
            if (key <= klo) ++cnt;
            else mn = min(mn, key);
          }
        }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        cnt += (unsigned)__shfl_xor((int)cnt, d);
        mn = min(mn, (unsigned)__shfl_xor((int)mn, d));
      }
      if (lane == 0) { red_cnt[wave] = cnt; red_min[wave] = mn; }
      __syncthreads();
      cnt = 0; mn = 0xffffffffu;
#pragma unroll
      for (int w = 0; w < PX_T / 64; ++w) { cnt += red_cnt[w]; mn = min(mn, red_min[w]); }
      if (cnt <= (unsigned)p.q_k + 1u) khi = mn;
    }
    const float lo = __uint_as_float(klo), hi = __uint_as_float(khi);
    const float d = hi - lo;
    // ATen's lerp, one rounding (sdmi.h)
    s = p.q_w < 0.5f ? __builtin_fmaf(p.q_w, d, lo) : __builtin_fmaf(-d, 1.0f - p.q_w, hi);
    if (s == s) s = s < p.max_val ? p.max_val : s;       // torch.maximum: a NaN stays
  }

  // ---- correction, m0, update ----
  const bool s_nan = !(s == s);
  const float ns = -s;
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int lr = tid + j * PX_T;
    if (lr < rps) {
      const long long ro = (row0 + lr) * 4;
      f32x4 m = {s, s, s, 0.f};
      if (!s_nan) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = px_clamp(v[j][c], ns, s) / s;
      }
      *reinterpret_cast<f32x4*>(p.m0 + ro) = m;
      px_update_row(p, ro, m);
    }
  }
}

template <typename P>
int px_check_common(const P* a) {
  SDMI_REQUIRE(a && a->x && a->out && a->m0, "null pointer");
  SDMI_REQUIRE(a->R >= 1 && a->rows_per_sample >= 1 && a->R % a->rows_per_sample == 0,
               "rows_per_sample must be positive and divide R");
  SDMI_REQUIRE(a->target >= SDMI_DPM_EPS && a->target <= SDMI_DPM_V, "unknown prediction target");
  SDMI_REQUIRE(a->correct >= SDMI_X0_NONE && a->correct <= SDMI_X0_DYNAMIC, "unknown correction of x0");
  SDMI_REQUIRE(a->alpha != 0.f && (a->target != SDMI_DPM_X0 || a->sigma != 0.f), "zero divisor");
  if (a->correct == SDMI_X0_DYNAMIC) {
    const long long n = 3LL * a->rows_per_sample;
    SDMI_REQUIRE(a->q_k >= 0 && a->q_k <= n - 1, "quantile rank outside the sample");
    SDMI_REQUIRE(a->q_w >= 0.f && a->q_w < 1.f && (a->q_w == 0.f || a->q_k < n - 1), "quantile weight outside [0, 1)");
    SDMI_REQUIRE(a->max_val > 0.f, "thresholding_max_val must be positive");
  }
  return SDMI_OK;
}

int px_check_alias(long long R, const void* const* ins, int n_in, const void* const* outs, int n_out) {
  const long long row = R * 16;
  for (int o = 0; o < n_out; ++o) {
    for (int i = 0; i < n_in; ++i)
      SDMI_REQUIRE(!spans_overlap(outs[o], row, ins[i], row), "an output aliases an input");
    for (int j = o + 1; j < n_out; ++j)
      SDMI_REQUIRE(!spans_overlap(outs[o], row, outs[j], row), "two outputs alias");
  }
  return SDMI_OK;
}

template <typename P>
int px_launch(const P& a, hipStream_t st, const char* what) {
  if (a.correct != SDMI_X0_DYNAMIC) {
    hipLaunchKernelGGL(px_rows_kernel<P>, dim3((a.R + 255) / 256), dim3(256), 0, st, a);
    return sdmi_check_launch(what);
  }
  const dim3 grid(a.R / a.rows_per_sample);
  if (a.rows_per_sample <= PX_T) hipLaunchKernelGGL((px_dynamic_kernel<1, P>), grid, dim3(PX_T), 0, st, a);
  else if (a.rows_per_sample <= 4 * PX_T) hipLaunchKernelGGL((px_dynamic_kernel<4, P>), grid, dim3(PX_T), 0, st, a);
  else hipLaunchKernelGGL((px_dynamic_kernel<16, P>), grid, dim3(PX_T), 0, st, a);
  return sdmi_check_launch(what);
}

// DYNAMIC past the register-resident sample size: nothing is launched, the caller runs the chain
#define PX_REFUSE_LARGE(a)                                                                         \
  do {                                                                                             \
    if ((a)->correct == SDMI_X0_DYNAMIC && (a)->rows_per_sample > SDMI_PX_MAX_ROWS) {              \
      sdmi_set_error("%s: dynamic thresholding serves samples of up to %d rows", __func__, (int)SDMI_PX_MAX_ROWS); \
      return SDMI_EUNSUPPORTED;                                                                    \
    }                                                                                              \
  } while (0)

}  // namespace

extern "C" int sdmi_dpm_step_px(const SdmiDpmStepPxArgs* a, void* stream) {
  if (const int rc = px_check_common(a)) return rc;
  SDMI_REQUIRE(a->mode >= SDMI_DPM_UPD_NONE && a->mode <= SDMI_DPM_UPD_MULTI3, "unknown update form");
  SDMI_REQUIRE(a->mode == SDMI_DPM_UPD_NONE || (a->base && a->y), "update without base / destination");
  SDMI_REQUIRE(a->mode < SDMI_DPM_UPD_SINGLE || a->h1, "update form needs the previous prediction");
  SDMI_REQUIRE(a->mode != SDMI_DPM_UPD_MULTI3 || a->h2, "third-order update needs two previous predictions");
  const bool upd = a->mode != SDMI_DPM_UPD_NONE;
  const void* ins[5] = {a->x, a->out, upd ? a->base : nullptr, a->mode >= SDMI_DPM_UPD_SINGLE ? a->h1 : nullptr,
                        a->mode == SDMI_DPM_UPD_MULTI3 ? a->h2 : nullptr};
  const void* outs[2] = {a->m0, upd ? a->y : nullptr};
  if (const int rc = px_check_alias(a->R, ins, 5, outs, 2)) return rc;
  PX_REFUSE_LARGE(a);
  return px_launch(*a, (hipStream_t)stream, "dpm_step_px");
}

extern "C" int sdmi_unipc_step_px(const SdmiUnipcStepPxArgs* a, void* stream) {
  if (const int rc = px_check_common(a)) return rc;
  SDMI_REQUIRE(a->corr_order >= 0 && a->corr_order <= 3 && a->pred_order >= 0 && a->pred_order <= 3,
               "corrector / predictor order outside 0..3");
  const int need = a->corr_order > a->pred_order - 1 ? a->corr_order : a->pred_order - 1;
  SDMI_REQUIRE((a->corr_order == 0 && a->pred_order == 0) || a->base, "update without base state");
  SDMI_REQUIRE(a->corr_order == 0 || a->xc, "corrector without destination");
  SDMI_REQUIRE(a->pred_order == 0 || a->y, "predictor without destination");
  SDMI_REQUIRE((need < 1 || a->h1) && (need < 2 || a->h2) && (a->corr_order < 3 || a->h3),
               "orders need more earlier predictions than given");
  const void* ins[6] = {a->x, a->out, a->base, a->h1, a->h2, a->h3};
  const void* outs[3] = {a->m0, a->corr_order ? a->xc : nullptr, a->pred_order ? a->y : nullptr};
  if (const int rc = px_check_alias(a->R, ins, 6, outs, 3)) return rc;
  PX_REFUSE_LARGE(a);
  return px_launch(*a, (hipStream_t)stream, "unipc_step_px");
}
