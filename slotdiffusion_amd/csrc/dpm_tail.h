// Row-level device code of the sampler tail kernels (include/sdmi.h: sdmi_dpm_step, sdmi_unipc_step and their image-space
// twins sdmi_dpm_step_px, sdmi_unipc_step_px): the data prediction and the solver updates of ONE [4]-float row.  Every
// expression is spelled op by op like the chain of sdmi_lincomb launches it replaces; the files that include this are
// compiled with -ffp-contract=off, so the bits are the chain's.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float dpm_x0(int target, float sigma, float alpha, float x, float o) {
  float eps = o;                                         // SDMI_DPM_EPS: the network predicts the noise
  if (target == SDMI_DPM_X0) {                           // model_wrapper 358-361: (x - alpha * out) / sigma
    const float t0 = 1.0f * x, t1 = (-alpha) * o;
    eps = (t0 + t1) / sigma;
  } else if (target == SDMI_DPM_V) {                     // 362-365: alpha * out + sigma * x
    const float t0 = alpha * o, t1 = sigma * x;
    eps = t0 + t1;
  }
  const float t0 = 1.0f * x, t1 = (-sigma) * eps;        // data_prediction_fn 529: (x - sigma * eps) / alpha
  return (t0 + t1) / alpha;
}

template <typename P>
__device__ __forceinline__ float dpm_update(const P& p, float x, float m0, float h1, float h2) {
  if (p.mode == SDMI_DPM_UPD_FIRST) {                    // c0 * x + c1 * m0
    const float t0 = p.c0 * x, t1 = p.c1 * m0;
    return t0 + t1;
  }
  if (p.mode == SDMI_DPM_UPD_SINGLE) {                   // (c0 * x + c1 * h1) + c2 * (m0 - h1)
    const float t0 = p.c0 * x, t1 = p.c1 * h1;
    const float d = m0 - h1, t2 = p.c2 * d;
    return (t0 + t1) + t2;
  }
  const float d0 = m0 - h1;
  const float D1_0 = p.k0 * d0;                          // D1_0 = (1 / r0) * (m0 - h1)
  const float t0 = p.c0 * x, t1 = p.c1 * m0;
  if (p.mode == SDMI_DPM_UPD_MULTI2) {                   // (c0 * x + c1 * m0) + c2 * D1_0
    const float t2 = p.c2 * D1_0;
    return (t0 + t1) + t2;
  }
  const float d1 = h1 - h2;
  const float D1_1 = p.k1 * d1;                          // D1_1 = (1 / r1) * (h1 - h2)
  const float dd = D1_0 - D1_1;
  const float gd = p.g * dd;
  const float D1 = 1.0f * D1_0 + gd;                     // D1 = D1_0 + r0 / (r0 + r1) * (D1_0 - D1_1)
  const float D2 = p.k2 * dd;                            // D2 = 1 / (r0 + r1) * (D1_0 - D1_1)
  const float t2 = p.c2 * D1, t3 = p.c3 * D2;
  const float y1 = (t0 + t1) + t2;
  const float u0 = 1.0f * y1;
  return u0 + t3;                                        // ((c0 * x + c1 * m0) + c2 * D1) + c3 * D2
}

// The back half of one row of the DPM-Solver++ tail (P: SdmiDpmStepArgs or SdmiDpmStepPxArgs, the same field names):
// the update from the base state, the prediction m of this evaluation and the earlier predictions, one 16-byte store.
template <typename P>
__device__ __forceinline__ void dpm_update_row(const P& p, long long ro, const f32x4& m) {
  if (p.mode == SDMI_DPM_UPD_NONE) return;
  const f32x4 bv = *reinterpret_cast<const f32x4*>(p.base + ro);
  f32x4 h1 = {0.f, 0.f, 0.f, 0.f}, h2 = {0.f, 0.f, 0.f, 0.f};
  if (p.mode >= SDMI_DPM_UPD_SINGLE) h1 = *reinterpret_cast<const f32x4*>(p.h1 + ro);
  if (p.mode == SDMI_DPM_UPD_MULTI3) h2 = *reinterpret_cast<const f32x4*>(p.h2 + ro);
  const f32x4 y = {dpm_update(p, bv[0], m[0], h1[0], h2[0]), dpm_update(p, bv[1], m[1], h1[1], h2[1]),
                   dpm_update(p, bv[2], m[2], h1[2], h2[2]), 0.f};
  *reinterpret_cast<f32x4*>(p.y + ro) = y;
}

template <typename P>
__device__ __forceinline__ float unipc_corr(const P& p, float b, float m0, float h1, float h2, float h3) {
  const float t0 = p.c0 * b, t1 = p.c1 * h1;
  float v = t0 + t1;                                     // c0 * base + c1 * h1
  if (p.corr_order >= 2) { const float d = h2 - h1, t = p.w1 * d; v = v + t; }
  if (p.corr_order == 3) { const float d = h3 - h1, t = p.w2 * d; v = v + t; }
  const float d = m0 - h1, t = p.wn * d;
  return v + t;
}

template <typename P>
__device__ __forceinline__ float unipc_pred(const P& p, float b, float m0, float h1, float h2) {
  const float t0 = p.p0 * b, t1 = p.p1 * m0;
  float v = t0 + t1;                                     // p0 * state + p1 * m0
  if (p.pred_order >= 2) { const float d = h1 - m0, t = p.q1 * d; v = v + t; }
  if (p.pred_order == 3) { const float d = h2 - m0, t = p.q2 * d; v = v + t; }
  return v;
}

// The back half of one row of the UniPC tail (P: SdmiUnipcStepArgs or SdmiUnipcStepPxArgs): corrector, then predictor
// from the corrected state, which goes from one to the other in registers.
template <typename P>
__device__ __forceinline__ void unipc_update_row(const P& p, long long ro, const f32x4& m) {
  if (p.corr_order == 0 && p.pred_order == 0) return;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f32x4 st = *reinterpret_cast<const f32x4*>(p.base + ro);
  const int need = max(p.corr_order, p.pred_order - 1);  // how many earlier predictions the two updates read
  const f32x4 h1 = need >= 1 ? *reinterpret_cast<const f32x4*>(p.h1 + ro) : z;
  const f32x4 h2 = need >= 2 ? *reinterpret_cast<const f32x4*>(p.h2 + ro) : z;
  const f32x4 h3 = p.corr_order == 3 ? *reinterpret_cast<const f32x4*>(p.h3 + ro) : z;
  if (p.corr_order > 0) {
    st = f32x4{unipc_corr(p, st[0], m[0], h1[0], h2[0], h3[0]), unipc_corr(p, st[1], m[1], h1[1], h2[1], h3[1]),
               unipc_corr(p, st[2], m[2], h1[2], h2[2], h3[2]), 0.f};
    *reinterpret_cast<f32x4*>(p.xc + ro) = st;
  }
  if (p.pred_order > 0) {
    const f32x4 y = {unipc_pred(p, st[0], m[0], h1[0], h2[0]), unipc_pred(p, st[1], m[1], h1[1], h2[1]),
                     unipc_pred(p, st[2], m[2], h1[2], h2[2]), 0.f};
    *reinterpret_cast<f32x4*>(p.y + ro) = y;
  }
}

// byte ranges [a, a + na) and [b, b + nb) intersect (a null pointer has no range)
static bool spans_overlap(const void* a, long long na, const void* b, long long nb) {
  const char *x = (const char*)a, *y = (const char*)b;
  return a && b && x < y + nb && y < x + na;
}

}  // namespace
