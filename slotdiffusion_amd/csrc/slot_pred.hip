// SAVi slot transition (sdmi.h: sdmi_lstm_cell / sdmi_lstm_cell_bwd / sdmi_pred_step / sdmi_pred_tf; the reference's
// video_based/models/predictor.py:20-44 TransformerPredictor, 47-73 ResidualMLPPredictor and 76-135
// RNNPredictorWrapper), and at the end of the file sdmi_rollout_feed, the per-step glue of the SlotFormer rollout on the
// same ps_dot products -- described at rollout_feed_kernel.
//
// sdmi_pred_tf: the transformer transition, all layers in one launch -- described at pred_tf_kernel below.  Attention
//   uses the 16-deep bf16 MFMA (hipcc --offload-arch=gfx950 accepts __builtin_amdgcn_mfma_f32_16x16x16bf16_1k), so a
//   head dim of 48 is three k steps and nothing is zero-padded in LDS.
//
// sdmi_lstm_cell / _bwd: one thread per (row, hidden unit) -- the gate arithmetic around the GEMM that sdmi_igemm does.
//
// sdmi_pred_step: a workgroup of 16 waves owns 16 slot rows; every stage is a [16 x K] x [K x 16 n] product on
//   mfma_f32_16x16x32_bf16 with the A operand (the activations, bf16) in LDS and the B operand (the weights) streamed
//   from L2 straight into registers in fragment order, 16 bytes per lane -- a workgroup reads every weight once, so
//   staging them in LDS would only add a pass.  In the 16 x 16 accumulator a lane holds rows 4 (lane / 16) .. + 3 of
//   column lane % 16: the wave that owns hidden units [16 c, 16 c + 16) computes their i, f, g, o columns into four
//   accumulators and the cell update happens on those registers, with no exchange.
//     stage 0  LayerNorm of the rows (a wave per row, fp32, two-pass variance) -> xn (bf16, LDS), res (fp32, LDS);
//              h_prev -> bf16 into the [u | h_prev] operand
//     stage 1  hidden = relu(W1 xn + b1)                 -> bf16, LDS
//     stage 2  u = W2 hidden + b2 + res                  -> bf16 into [u | h_prev] (or y, without the wrapper)
//     stage 3  z = Wg [u | h_prev] + bg, cell update     -> h, c (fp32, global), h (bf16, LDS)
//     stage 4  y = Wo h + bo
//   Rows past R are computed on zeros and never stored.  h / c may alias h_prev / c_prev: a workgroup has read its rows
//   of h_prev before its first barrier, and a c_prev element is read by the thread that overwrites it.
#include "common.h"

namespace {

__device__ __forceinline__ float lc_sigm(float x) { return 1.f / (1.f + __expf(-x)); }

__global__ __launch_bounds__(256) void lstm_cell_kernel(SdmiLstmCellArgs p) {
  const long long n = (long long)p.R * p.H;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / p.H;
    const int c = (int)(i - r * p.H);
    const float* z = p.z + r * p.ldz;
    const float ig = lc_sigm(z[c]), fg = lc_sigm(z[p.H + c]), gg = tanhf(z[2 * p.H + c]), og = lc_sigm(z[3 * p.H + c]);
    const float cp = p.c_prev ? p.c_prev[r * p.ldcp + c] : 0.f;
    const float cn = fmaf(fg, cp, ig * gg);
    p.c[i] = cn;
    p.h[i] = og * tanhf(cn);
    if (p.gates) {
      float* g = p.gates + r * 4 * p.H;
      g[c] = ig; g[p.H + c] = fg; g[2 * p.H + c] = gg; g[3 * p.H + c] = og;
    }
  }
}

__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(SdmiLstmCellBwdArgs p) {
  const long long n = (long long)p.R * p.H;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / p.H;
    const int c = (int)(i - r * p.H);
    const float* g = p.gates + r * 4 * p.H;
    const float ig = g[c], fg = g[p.H + c], gg = g[2 * p.H + c], og = g[3 * p.H + c];
    const float cp = p.c_prev ? p.c_prev[r * p.ldcp + c] : 0.f;
    const float tc = tanhf(p.c[i]);
    const float dh = p.dh[i];
    const float dc = fmaf(dh * og, 1.f - tc * tc, p.dc_next ? p.dc_next[i] : 0.f);
    float* dz = p.dz + r * 4 * p.H;
    dz[c] = dc * gg * ig * (1.f - ig);
    dz[p.H + c] = dc * cp * fg * (1.f - fg);
    dz[2 * p.H + c] = dc * ig * (1.f - gg * gg);
    dz[3 * p.H + c] = dh * tc * og * (1.f - og);
    p.dc_prev[i] = dc * fg;
  }
}

// ------------------------------------------------------------------------------------------
// fused transition
// ------------------------------------------------------------------------------------------
constexpr int PS_ROWS = 16, PS_WAVES = 16, PS_PAD = 8;      // pad: 16 bytes, consecutive rows start 4 banks apart
constexpr int PS_INFLIGHT = 16;                             // weight fragments (16 bytes per lane) a wave keeps in flight

// U k steps of NB fragments each: all U NB loads are issued before the first MFMA waits for one -- a workgroup is
// alone on its compute unit and every weight comes from L2 exactly once, so the loads in flight, not the MFMAs, set the
// time of a stage
template <int NB, int U>
__device__ __forceinline__ void ps_batch(const bf16_t* ap, const uint4* wp, int s, f32x4* acc) {
  uint4 b[U][NB];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int g = 0; g < NB; ++g) b[u][g] = wp[((size_t)(s + u) * NB + g) * 64];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint4 a = *reinterpret_cast<const uint4*>(ap + (s + u) * 32);
#pragma unroll
    for (int g = 0; g < NB; ++g)
      acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b[u][g]),
                                                       acc[g], 0, 0, 0);
  }
}

// acc[g] += A[16 x 32 ks] (LDS, `lda` elements per row) x the packed fragments wp[(s NB + g) 64 + lane], s < ks, g < NB
template <int NB, int INFLIGHT = PS_INFLIGHT>
__device__ __forceinline__ void ps_dot(const bf16_t* A, int lda, const uint4* wp, int ks, int lane, f32x4* acc) {
  const bf16_t* ap = A + (lane & 15) * lda + 8 * (lane >> 4);
  wp += lane;
  constexpr int U = INFLIGHT / NB;
  int s = 0;
  for (; s + U <= ks; s += U) ps_batch<NB, U>(ap, wp, s, acc);
  if constexpr (U >= 8) if (s + 8 <= ks) { ps_batch<NB, 8>(ap, wp, s, acc); s += 8; }
  if constexpr (U >= 4) if (s + 4 <= ks) { ps_batch<NB, 4>(ap, wp, s, acc); s += 4; }
  if (s + 2 <= ks) { ps_batch<NB, 2>(ap, wp, s, acc); s += 2; }
  if (s < ks) ps_batch<NB, 1>(ap, wp, s, acc);
}

__global__ __launch_bounds__(64 * PS_WAVES) void pred_step_kernel(SdmiPredStepArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ps_smem[];
  const int D = p.D, H = p.H;
  const bool mlp = p.mode & SDMI_PRED_MLP, rnn = p.mode & SDMI_PRED_RNN;
  const int ld0 = D + PS_PAD, ld1 = (2 * D > H ? 2 * D : H) + PS_PAD, ldc = D + H + PS_PAD;
  float* resf = reinterpret_cast<float*>(ps_smem);                       // [16][D]
  bf16_t* A0 = reinterpret_cast<bf16_t*>(resf + PS_ROWS * D);            // [16][ld0]  xn
  bf16_t* A1 = A0 + PS_ROWS * ld0;                                       // [16][ld1]  hidden, later h
  bf16_t* Ac = A1 + PS_ROWS * ld1;                                       // [16][ldc]  [u | h_prev]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long row0 = (long long)blockIdx.x * PS_ROWS;
  const int col = lane & 15, rq = 4 * (lane >> 4);                        // accumulator: column, first of 4 rows

  // ---- stage 0
  {
    const int r = wave;                                                   // a wave per row
    const bool live = row0 + r < p.R;
    const float* xr = p.x + (row0 + r) * p.ldx;
    float v[4];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + 64 * k;
      v[k] = (live && c < D) ? xr[c] : 0.f;
      s += v[k];
    }
    if (mlp) {
      const float mean = wave_sum(s) / (float)D;
      float q = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = (lane + 64 * k < D) ? v[k] - mean : 0.f;
        q = fmaf(d, d, q);
      }
      const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + p.eps);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c < D) {
          const float xn = fmaf((v[k] - mean) * rstd, p.ln_g[c], p.ln_b[c]);
          resf[r * D + c] = p.norm_first ? xn : v[k];
          A0[r * ld0 + c] = f32_to_bf16(xn);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c < D) Ac[r * ldc + c] = f32_to_bf16(v[k]);
      }
    }
  }
  if (rnn) {
    for (int idx = tid; idx < PS_ROWS * H; idx += 64 * PS_WAVES) {
      const int r = idx / H, c = idx - r * H;
      const float hv = (p.h_prev && row0 + r < p.R) ? p.h_prev[(row0 + r) * p.ldh + c] : 0.f;
      Ac[r * ldc + D + c] = f32_to_bf16(hv);
    }
  }
  __syncthreads();

  if (mlp) {
    // ---- stage 1
    const int ks1 = D >> 5;
    for (int n = wave; n < (2 * D) >> 4; n += PS_WAVES) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      ps_dot<1>(A0, ld0, reinterpret_cast<const uint4*>(p.w1p) + (size_t)n * ks1 * 64, ks1, lane, &acc);
      const float b = p.b1[16 * n + col];
#pragma unroll
      for (int j = 0; j < 4; ++j) A1[(rq + j) * ld1 + 16 * n + col] = f32_to_bf16(fmaxf(acc[j] + b, 0.f));
    }
    __syncthreads();
    // ---- stage 2
    const int ks2 = (2 * D) >> 5;
    for (int n = wave; n < D >> 4; n += PS_WAVES) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      ps_dot<1>(A1, ld1, reinterpret_cast<const uint4*>(p.w2p) + (size_t)n * ks2 * 64, ks2, lane, &acc);
      const int c = 16 * n + col;
      const float b = p.b2[c];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float u = acc[j] + b + resf[(rq + j) * D + c];
        if (rnn) Ac[(rq + j) * ldc + c] = f32_to_bf16(u);
        else if (row0 + rq + j < p.R) p.y[(row0 + rq + j) * D + c] = u;
      }
    }
    __syncthreads();
  }
  if (!rnn) return;

  // ---- stage 3
  const int ksg = (D + H) >> 5;
  for (int n = wave; n < H >> 4; n += PS_WAVES) {
    const uint4* wp = reinterpret_cast<const uint4*>(p.wgp) + (size_t)n * ksg * 256;
    f32x4 z[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) z[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    ps_dot<4>(Ac, ldc, wp, ksg, lane, z);
    const int c = 16 * n + col;
    const float bi = p.bg[c], bf = p.bg[H + c], bgg = p.bg[2 * H + c], bo = p.bg[3 * H + c];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long r = row0 + rq + j;
      const bool live = r < p.R;
      const float ig = lc_sigm(z[0][j] + bi), fg = lc_sigm(z[1][j] + bf), gg = tanhf(z[2][j] + bgg), og = lc_sigm(z[3][j] + bo);
      const float cp = (p.c_prev && live) ? p.c_prev[r * p.ldh + c] : 0.f;
      const float cn = fmaf(fg, cp, ig * gg);
      const float hn = og * tanhf(cn);
      if (live) {
        p.c[r * H + c] = cn;
        p.h[r * H + c] = hn;
      }
      A1[(rq + j) * ld1 + c] = f32_to_bf16(hn);
    }
  }
  __syncthreads();

  // ---- stage 4
  const int kso = H >> 5;
  for (int n = wave; n < D >> 4; n += PS_WAVES) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    ps_dot<1>(A1, ld1, reinterpret_cast<const uint4*>(p.wop) + (size_t)n * kso * 64, kso, lane, &acc);
    const int c = 16 * n + col;
    const float b = p.bo[c];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (row0 + rq + j < p.R) p.y[(row0 + rq + j) * D + c] = acc[j] + b;
  }
}

// ------------------------------------------------------------------------------------------
// fused transformer transition
// ------------------------------------------------------------------------------------------
typedef short tf_bf16x4 __attribute__((ext_vector_type(4)));
constexpr int TF_LDP = 24;      // row pitch of the 16-key tiles (P, V^T): 48 bytes, 8-byte fragments stay aligned
constexpr int TF_INFLIGHT = 8;  // weight fragments in flight: with 16 the kernel spills at the 128 VGPRs of a 16-wave workgroup

// LayerNorm of slot row `wave` (fp32, two-pass; the arithmetic of pred_step_kernel's stage 0) -> A0 (bf16).  first: the
// row comes from global memory (zeros past row N) and is copied into the residual stream
__device__ __forceinline__ void tf_layer_norm(const float* xg, float* xres, bf16_t* A0, int ld0, int D, int N, bool first,
                                              const float* g, const float* b, float eps, int wave, int lane) {
  const int r = wave;
  float v[4];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + 64 * k;
    v[k] = 0.f;
    if (c < D) {
      if (first) {
        v[k] = r < N ? xg[(size_t)r * D + c] : 0.f;
        xres[r * D + c] = v[k];
      } else {
        v[k] = xres[r * D + c];
      }
    }
    s += v[k];
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float d = (lane + 64 * k < D) ? v[k] - mean : 0.f;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + 64 * k;
    if (c < D) A0[r * ld0 + c] = f32_to_bf16(fmaf((v[k] - mean) * rstd, g[c], b[c]));
  }
}

// sdmi_pred_tf: a workgroup of 16 waves owns ONE sample (its N <= 16 slot rows are one MFMA tile; rows past N are zeros
// on the way in and never stored).  The residual stream stays in LDS in fp32 across the layers.  Per layer:
//     stage 0  LN1 (a wave per row)                            -> A0 (bf16)
//     stage 1  q | k | v = Wqkv A0 + bqkv                      -> QK [16][2D] and V transposed, Vt [D][16 keys] (bf16)
//     stage 2  wave h < heads: S = scale Q_h K_h^T on the 16-deep bf16 MFMA (head_dim / 16 k steps: 48 needs no pad),
//              keys past N masked, row softmax inside the accumulator (a row's 16 keys = the 16 lanes of a lane group)
//                                                              -> P_h (bf16)
//     stage 3  column chunk n of O = P V (one 16-deep MFMA)    -> A0 (bf16)
//     stage 4  x += Wo A0 + bo                                 (fp32, LDS)
//     stage 5  LN2                                             -> A0
//     stage 6  hidden = relu(W1 A0 + b1)                       -> Hd (bf16; over QK / Vt / P, dead by now)
//     stage 7  x += W2 hidden + b2                             (the last layer stores rows < N to y instead)
//   The projections are ps_dot on the packed operands of pred_step_kernel, the layers' operands one behind the other.
__global__ __launch_bounds__(64 * PS_WAVES) void pred_tf_kernel(SdmiPredTfArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tf_smem[];
  const int D = p.D, F = p.F, N = p.N, heads = p.heads, hd = D / heads;
  const int ld0 = D + PS_PAD, ldq = 2 * D + PS_PAD, ldh = F + PS_PAD;
  float* xres = reinterpret_cast<float*>(tf_smem);                       // [16][D]
  bf16_t* A0 = reinterpret_cast<bf16_t*>(xres + PS_ROWS * D);            // [16][ld0]
  bf16_t* QK = A0 + PS_ROWS * ld0;                                       // [16][ldq]
  bf16_t* Vt = QK + PS_ROWS * ldq;                                       // [D][TF_LDP]
  bf16_t* Pb = Vt + D * TF_LDP;                                          // [heads][16][TF_LDP]
  bf16_t* Hd = QK;                                                       // [16][ldh]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, rq = 4 * (lane >> 4);
  const float* xg = p.x + (size_t)blockIdx.x * N * D;
  float* yg = p.y + (size_t)blockIdx.x * N * D;
  const float scale = 1.f / sqrtf((float)hd);
  const int ksd = D >> 5, ksf = F >> 5;

  for (int l = 0; l < p.layers; ++l) {
    // ---- stage 0
    tf_layer_norm(xg, xres, A0, ld0, D, N, l == 0, p.ln1_g + l * D, p.ln1_b + l * D, p.eps, wave, lane);
    __syncthreads();
    // ---- stage 1
    {
      const uint4* w = reinterpret_cast<const uint4*>(p.wqkv) + (size_t)l * 3 * D * D / 8;
      const float* bias = p.bqkv + l * 3 * D;
      for (int n = wave; n < (3 * D) >> 4; n += PS_WAVES) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        ps_dot<1, TF_INFLIGHT>(A0, ld0, w + (size_t)n * ksd * 64, ksd, lane, &acc);
        const int c = 16 * n + col;
        const float b = bias[c];
        if (c < 2 * D) {
#pragma unroll
          for (int j = 0; j < 4; ++j) QK[(rq + j) * ldq + c] = f32_to_bf16(acc[j] + b);
        } else {
          uint2 v;
          v.x = f32x2_to_bf16x2(acc[0] + b, acc[1] + b);
          v.y = f32x2_to_bf16x2(acc[2] + b, acc[3] + b);
          *reinterpret_cast<uint2*>(Vt + (c - 2 * D) * TF_LDP + rq) = v;
        }
      }
    }
    __syncthreads();
    // ---- stage 2
    if (wave < heads) {
      const bf16_t* qp = QK + col * ldq + wave * hd + rq;
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < hd; k += 16) {
        const tf_bf16x4 a = *reinterpret_cast<const tf_bf16x4*>(qp + k);
        const tf_bf16x4 b = *reinterpret_cast<const tf_bf16x4*>(qp + D + k);
        s = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, s, 0, 0, 0);
      }
      bf16_t* pw = Pb + wave * PS_ROWS * TF_LDP;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = col < N ? s[j] * scale : -INFINITY;
        float m = v;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        const float e = __expf(v - m);
        float t = e;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        pw[(rq + j) * TF_LDP + col] = f32_to_bf16(e / t);
      }
    }
    __syncthreads();
    // ---- stage 3
    for (int n = wave; n < D >> 4; n += PS_WAVES) {
      const int h = (16 * n) / hd;
      const tf_bf16x4 a = *reinterpret_cast<const tf_bf16x4*>(Pb + (h * PS_ROWS + col) * TF_LDP + rq);
      const tf_bf16x4 b = *reinterpret_cast<const tf_bf16x4*>(Vt + (16 * n + col) * TF_LDP + rq);
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      o = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, o, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) A0[(rq + j) * ld0 + 16 * n + col] = f32_to_bf16(o[j]);
    }
    __syncthreads();
    // ---- stage 4
    {
      const uint4* w = reinterpret_cast<const uint4*>(p.wo) + (size_t)l * D * D / 8;
      for (int n = wave; n < D >> 4; n += PS_WAVES) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        ps_dot<1, TF_INFLIGHT>(A0, ld0, w + (size_t)n * ksd * 64, ksd, lane, &acc);
        const int c = 16 * n + col;
        const float b = p.bo[l * D + c];
#pragma unroll
        for (int j = 0; j < 4; ++j) xres[(rq + j) * D + c] = acc[j] + b + xres[(rq + j) * D + c];
      }
    }
    __syncthreads();
    // ---- stage 5
    tf_layer_norm(xg, xres, A0, ld0, D, N, false, p.ln2_g + l * D, p.ln2_b + l * D, p.eps, wave, lane);
    __syncthreads();
    // ---- stage 6
    {
      const uint4* w = reinterpret_cast<const uint4*>(p.w1) + (size_t)l * F * D / 8;
      for (int n = wave; n < F >> 4; n += PS_WAVES) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        ps_dot<1, TF_INFLIGHT>(A0, ld0, w + (size_t)n * ksd * 64, ksd, lane, &acc);
        const float b = p.b1[l * F + 16 * n + col];
#pragma unroll
        for (int j = 0; j < 4; ++j) Hd[(rq + j) * ldh + 16 * n + col] = f32_to_bf16(fmaxf(acc[j] + b, 0.f));
      }
    }
    __syncthreads();
    // ---- stage 7
    {
      const uint4* w = reinterpret_cast<const uint4*>(p.w2) + (size_t)l * D * F / 8;
      const bool last = l + 1 == p.layers;
      for (int n = wave; n < D >> 4; n += PS_WAVES) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        ps_dot<1, TF_INFLIGHT>(Hd, ldh, w + (size_t)n * ksf * 64, ksf, lane, &acc);
        const int c = 16 * n + col;
        const float b = p.b2[l * D + c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float o = acc[j] + b + xres[(rq + j) * D + c];
          if (!last) xres[(rq + j) * D + c] = o;
          else if (rq + j < N) yg[(size_t)(rq + j) * D + c] = o;
        }
      }
    }
    __syncthreads();
  }
}

int tf_smem_bytes(int D, int F, int heads) {
  const int attn = (PS_ROWS * (2 * D + PS_PAD) + D * TF_LDP + heads * PS_ROWS * TF_LDP) * 2;
  const int ffn = PS_ROWS * (F + PS_PAD) * 2;
  return PS_ROWS * D * 4 + PS_ROWS * (D + PS_PAD) * 2 + (attn > ffn ? attn : ffn);
}

int lc_blocks(long long n) {
  const long long b = (n + 255) / 256;
  return (int)(b > 2048 ? 2048 : b);
}

}  // namespace

extern "C" int sdmi_lstm_cell(const SdmiLstmCellArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->z && a->h && a->c, "null pointer");
  SDMI_REQUIRE(a->R >= 1 && a->H >= 1, "empty problem");
  SDMI_REQUIRE(a->ldz >= 4 * a->H && (!a->c_prev || a->ldcp >= a->H), "row pitch shorter than the row");
  hipLaunchKernelGGL(lstm_cell_kernel, dim3(lc_blocks((long long)a->R * a->H)), dim3(256), 0, (hipStream_t)stream, *a);
  return sdmi_check_launch("sdmi_lstm_cell");
}

extern "C" int sdmi_lstm_cell_bwd(const SdmiLstmCellBwdArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->dh && a->gates && a->c && a->dz && a->dc_prev, "null pointer");
  SDMI_REQUIRE(a->R >= 1 && a->H >= 1, "empty problem");
  SDMI_REQUIRE(!a->c_prev || a->ldcp >= a->H, "row pitch shorter than the row");
  hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(lc_blocks((long long)a->R * a->H)), dim3(256), 0, (hipStream_t)stream, *a);
  return sdmi_check_launch("sdmi_lstm_cell_bwd");
}

extern "C" int sdmi_pred_step(const SdmiPredStepArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->x && a->y, "null x / y");
  SDMI_REQUIRE(a->mode >= 1 && a->mode <= 3, "mode: SDMI_PRED_MLP | SDMI_PRED_RNN");
  SDMI_REQUIRE(a->R >= 1 && (long long)a->R + PS_ROWS - 1 <= 2147483647LL, "1 <= R < 2^31 - 16");
  SDMI_REQUIRE(a->D >= 32 && a->D <= 256 && a->D % 32 == 0, "D must be a multiple of 32, at most 256");
  SDMI_REQUIRE(a->ldx >= a->D, "ldx shorter than the row");
  const bool mlp = a->mode & SDMI_PRED_MLP, rnn = a->mode & SDMI_PRED_RNN;
  if (mlp) {
    SDMI_REQUIRE(a->ln_g && a->ln_b && a->w1p && a->b1 && a->w2p && a->b2, "null MLP operand");
    SDMI_REQUIRE((((uintptr_t)a->w1p | (uintptr_t)a->w2p) & 15) == 0, "w1p / w2p must be 16-byte aligned");
  }
  const int H = rnn ? a->H : 0;
  if (rnn) {
    SDMI_REQUIRE(a->H >= 32 && a->H <= 512 && a->H % 32 == 0, "H must be a multiple of 32, at most 512");
    SDMI_REQUIRE(a->h && a->c && a->wgp && a->bg && a->wop && a->bo, "null LSTM operand");
    SDMI_REQUIRE((((uintptr_t)a->wgp | (uintptr_t)a->wop) & 15) == 0, "wgp / wop must be 16-byte aligned");
    SDMI_REQUIRE(!(a->h_prev || a->c_prev) || a->ldh >= a->H, "ldh shorter than the row");
  }
  SdmiPredStepArgs k = *a;
  k.H = H;
  const int D = a->D;
  const int smem = PS_ROWS * (D * 4 + (D + PS_PAD) * 2 + ((2 * D > H ? 2 * D : H) + PS_PAD) * 2 + (D + H + PS_PAD) * 2);
  SDMI_OPTIN_LDS(pred_step_kernel, 96 * 1024, "sdmi_pred_step");
  const int tiles = (a->R + PS_ROWS - 1) / PS_ROWS;
  hipLaunchKernelGGL(pred_step_kernel, dim3(tiles), dim3(64 * PS_WAVES), smem, (hipStream_t)stream, k);
  return sdmi_check_launch("sdmi_pred_step");
}

extern "C" int sdmi_pred_tf(const SdmiPredTfArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->x && a->y, "null x / y");
  SDMI_REQUIRE(a->B >= 1, "empty batch");
  SDMI_REQUIRE(a->N >= 1 && a->N <= PS_ROWS, "1 <= N <= 16");
  SDMI_REQUIRE(a->D >= 32 && a->D <= 256 && a->D % 32 == 0, "D must be a multiple of 32, at most 256");
  SDMI_REQUIRE(a->heads >= 1 && a->D % a->heads == 0 && (a->D / a->heads) % 16 == 0 && a->D / a->heads <= 64,
               "head_dim = D / heads must be a multiple of 16, at most 64");
  SDMI_REQUIRE(a->F >= 32 && a->F <= 1024 && a->F % 32 == 0, "F must be a multiple of 32, at most 1024");
  SDMI_REQUIRE(a->layers >= 1 && a->layers <= 4, "1 <= layers <= 4");
  SDMI_REQUIRE(a->wqkv && a->wo && a->w1 && a->w2 && a->ln1_g && a->ln1_b && a->bqkv && a->bo && a->ln2_g && a->ln2_b &&
               a->b1 && a->b2, "null operand");
  SDMI_REQUIRE((((uintptr_t)a->wqkv | (uintptr_t)a->wo | (uintptr_t)a->w1 | (uintptr_t)a->w2) & 15) == 0,
               "packed weights must be 16-byte aligned");
  {
    const uintptr_t x0 = (uintptr_t)a->x, y0 = (uintptr_t)a->y;
    const unsigned long long n = (unsigned long long)a->B * a->N * a->D * 4;
    SDMI_REQUIRE(x0 + n <= y0 || y0 + n <= x0, "y must not overlap x");
  }
  SDMI_OPTIN_LDS(pred_tf_kernel, 96 * 1024, "sdmi_pred_tf");
  hipLaunchKernelGGL(pred_tf_kernel, dim3(a->B), dim3(64 * PS_WAVES), tf_smem_bytes(a->D, a->F, a->heads),
                     (hipStream_t)stream, *a);
  return sdmi_check_launch("sdmi_pred_tf");
}

// ------------------------------------------------------------------------------------------
// SlotFormer rollout: everything between the last layer of step s and the first layer of step s + 1
// (vp_vqa/models/slotformer.py:112-124)
// ------------------------------------------------------------------------------------------
namespace {

constexpr int RF_MAXD = 256;                                // largest C / Ds

// sdmi_rollout_feed: a workgroup of 16 waves owns ONE sequence; its N <= 16 newest token rows are one MFMA tile (rows
// past N are zeros on the way in and never stored).
//     stage a  rows [L - N, L) of x                                   -> A0 (bf16, LDS)
//     stage b  pred = Wout A0 + bout    (a wave per 16-column chunk)  -> pred (fp32, global), bf16(pred) -> A1 (LDS)
//     stage c  tok = bf16(Win A1 + bin)                               -> A0 (LDS; its stage-a rows are dead by now)
//     stage d  win_next = [win rows [N, L) | tok], x_next = bf16(win_next + pos), x_next rows [L, Lp) = 0: 16-byte
//              accesses, all waves
//   win == NULL (the last step) ends after stage b.  The products are ps_dot on operands packed as for pred_step_kernel.
__global__ __launch_bounds__(64 * PS_WAVES) void rollout_feed_kernel(SdmiRolloutFeedArgs p) {
  __shared__ __attribute__((aligned(16))) bf16_t A0[PS_ROWS * (RF_MAXD + PS_PAD)];
  __shared__ __attribute__((aligned(16))) bf16_t A1[PS_ROWS * (RF_MAXD + PS_PAD)];
  const int C = p.C, Ds = p.Ds, N = p.N, L = p.L;
  const int ld0 = C + PS_PAD, ld1 = Ds + PS_PAD, cv = C >> 3;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, rq = 4 * (lane >> 4);
  const size_t seq = (size_t)blockIdx.x * p.Lp * C;          // first element of this sequence's window

  // ---- stage a
  if (tid < PS_ROWS * cv) {
    const int r = tid / cv, ch = tid - r * cv;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (r < N) v = *reinterpret_cast<const uint4*>((const bf16_t*)p.x + seq + (size_t)(L - N + r) * C + 8 * ch);
    *reinterpret_cast<uint4*>(A0 + r * ld0 + 8 * ch) = v;
  }
  __syncthreads();
  // ---- stage b
  {
    const int ks = C >> 5;
    float* pg = p.pred + (long long)blockIdx.x * p.ld_pred;
    for (int n = wave; n < Ds >> 4; n += PS_WAVES) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      ps_dot<1>(A0, ld0, reinterpret_cast<const uint4*>(p.wout) + (size_t)n * ks * 64, ks, lane, &acc);
      const int c = 16 * n + col;
      const float b = p.bout[c];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = acc[j] + b;
        if (rq + j < N) pg[(rq + j) * Ds + c] = v;
        A1[(rq + j) * ld1 + c] = f32_to_bf16(v);
      }
    }
  }
  if (!p.win) return;
  __syncthreads();
  // ---- stage c
  {
    const int ks = Ds >> 5;
    for (int n = wave; n < C >> 4; n += PS_WAVES) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      ps_dot<1>(A1, ld1, reinterpret_cast<const uint4*>(p.win_w) + (size_t)n * ks * 64, ks, lane, &acc);
      const int c = 16 * n + col;
      const float b = p.bin[c];
#pragma unroll
      for (int j = 0; j < 4; ++j) A0[(rq + j) * ld0 + c] = f32_to_bf16(acc[j] + b);
    }
  }
  __syncthreads();
  // ---- stage d
  {
    const bf16_t* wg = (const bf16_t*)p.win + seq;
    bf16_t* wn = (bf16_t*)p.win_next + seq;
    bf16_t* xn = (bf16_t*)p.x_next + seq;
    const int keep = L - N;
    for (int i = tid; i < L * cv; i += 64 * PS_WAVES) {
      const int r = i / cv, ch = i - r * cv;
      const size_t o = (size_t)r * C + 8 * ch;
      uint4 v;
      if (r < keep) v = *reinterpret_cast<const uint4*>(wg + o + (size_t)N * C);
      else v = *reinterpret_cast<const uint4*>(A0 + (r - keep) * ld0 + 8 * ch);
      *reinterpret_cast<uint4*>(wn + o) = v;
      float f[8];
      unpack16<bf16_t>(v, f);
      const float4 p0 = *reinterpret_cast<const float4*>(p.pos + o);
      const float4 p1 = *reinterpret_cast<const float4*>(p.pos + o + 4);
      f[0] += p0.x; f[1] += p0.y; f[2] += p0.z; f[3] += p0.w;
      f[4] += p1.x; f[5] += p1.y; f[6] += p1.z; f[7] += p1.w;
      *reinterpret_cast<uint4*>(xn + o) = pack16<bf16_t>(f);
    }
    for (int i = L * cv + tid; i < p.Lp * cv; i += 64 * PS_WAVES)
      *reinterpret_cast<uint4*>(xn + (size_t)i * 8) = make_uint4(0u, 0u, 0u, 0u);
  }
}

bool rf_disjoint(const void* a, const void* b, unsigned long long n) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 + n <= b0 || b0 + n <= a0;
}

}  // namespace

extern "C" int sdmi_rollout_feed(const SdmiRolloutFeedArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->x && a->pred && a->wout && a->bout, "null x / pred / wout / bout");
  SDMI_REQUIRE(a->B >= 1, "empty batch");
  SDMI_REQUIRE(a->N >= 1 && a->N <= PS_ROWS, "1 <= N <= 16");
  SDMI_REQUIRE(a->L >= a->N && a->L % a->N == 0 && a->L <= a->Lp, "L must be a multiple of N with N <= L <= Lp");
  SDMI_REQUIRE(a->C >= 32 && a->C <= RF_MAXD && a->C % 32 == 0, "C must be a multiple of 32, at most 256");
  SDMI_REQUIRE(a->Ds >= 32 && a->Ds <= RF_MAXD && a->Ds % 32 == 0, "Ds must be a multiple of 32, at most 256");
  SDMI_REQUIRE(a->ld_pred >= (long long)a->N * a->Ds, "ld_pred shorter than a sample's [N][Ds]");
  SDMI_REQUIRE((((uintptr_t)a->x | (uintptr_t)a->wout) & 15) == 0, "x / wout must be 16-byte aligned");
  if (a->win) {
    SDMI_REQUIRE(a->win_next && a->x_next && a->pos && a->win_w && a->bin, "null win_next / x_next / pos / win_w / bin");
    SDMI_REQUIRE((((uintptr_t)a->win | (uintptr_t)a->win_next | (uintptr_t)a->x_next | (uintptr_t)a->pos |
                   (uintptr_t)a->win_w) & 15) == 0, "win / win_next / x_next / pos / win_w must be 16-byte aligned");
    const unsigned long long n = (unsigned long long)a->B * a->Lp * a->C * 2;
    SDMI_REQUIRE(rf_disjoint(a->x_next, a->x, n) && rf_disjoint(a->x_next, a->win, n) &&
                 rf_disjoint(a->win_next, a->x, n) && rf_disjoint(a->win_next, a->win, n) &&
                 rf_disjoint(a->win_next, a->x_next, n), "x_next / win_next must not overlap x, win or each other");
  }
  hipLaunchKernelGGL(rollout_feed_kernel, dim3(a->B), dim3(64 * PS_WAVES), 0, (hipStream_t)stream, *a);
  return sdmi_check_launch("sdmi_rollout_feed");
}
