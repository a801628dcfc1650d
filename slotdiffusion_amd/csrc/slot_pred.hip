// SAVi slot transition (sdmi.h: sdmi_lstm_cell / sdmi_lstm_cell_bwd / sdmi_pred_step; the reference's
// video_based/models/predictor.py:47-73 ResidualMLPPredictor and 76-135 RNNPredictorWrapper).
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
template <int NB>
__device__ __forceinline__ void ps_dot(const bf16_t* A, int lda, const uint4* wp, int ks, int lane, f32x4* acc) {
  const bf16_t* ap = A + (lane & 15) * lda + 8 * (lane >> 4);
  wp += lane;
  constexpr int U = PS_INFLIGHT / NB;
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
