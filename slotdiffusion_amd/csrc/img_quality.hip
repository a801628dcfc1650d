// Image-quality scoring tail in one launch (include/sdmi.h: sdmi_img_quality): to_rgb of both images, the squared error,
// the 8-bit frames and SSIM from one staged copy of each source row band.
//
// grid (F * nbands): a workgroup owns one frame's band of R = S * 8 SSIM output rows.  Per channel it stages the band's
// R + 10 source rows of both images in LDS as to_rgb(x) * 255 (fp32, 16-byte loads where the layout allows, 16-byte LDS
// writes); the same pass adds the band's own pixels to the squared error and writes their bytes.  Then thread
// (column, sub-band) walks the 18 source rows of its 8 output rows: the 11-tap row filter of the five moments from LDS
// (fp64), each row's result added to the (up to 8) column-filter accumulators it belongs to -- 22 taps per pixel and
// moment, all in registers, no scratch.  Per-workgroup fp64 partials, fixed reduction tree, no floating-point atomics.
// Compiled without FMA contraction: x * 0.5f + 0.5f and a * 255.f are the two-rounding forms of the composed path.
#include "common.h"

namespace {

constexpr int IQ_THREADS = 256;
constexpr int IQ_SR = 8;                  // output rows per thread
constexpr int IQ_ROWS = IQ_SR + 10;       // source rows a thread walks
constexpr int IQ_MAXSUB = 8;              // sub-bands per workgroup at most

struct IqGeom { int S, CW, R, nb, Wp, nrows; };

// S sub-bands of 8 output rows side by side in the 256 threads (CW threads each, one per output column)
static IqGeom iq_geom(int H, int W) {
  IqGeom g;
  const int h = H - 10, w = W - 10;
  g.CW = (w + 31) / 32 * 32;
  g.S = IQ_THREADS / g.CW;
  if (g.S > IQ_MAXSUB) g.S = IQ_MAXSUB;
  const int need = (h + IQ_SR - 1) / IQ_SR;
  if (g.S > need) g.S = need;
  g.R = g.S * IQ_SR;
  g.nb = (h + g.R - 1) / g.R;
  g.Wp = (W + 3) / 4 * 4;
  g.nrows = g.R + 10;
  return g;
}

struct IqWin { double g[11]; };

enum { IQ_NCHW = 0, IQ_NCHW_V4 = 1, IQ_NHWC4 = 2 };

// four consecutive pixels (x0 .. x0 + 3, x0 a multiple of 4) of channel c, row y of frame f; 0 beyond W
__device__ __forceinline__ f32x4 iq_load4(const float* __restrict__ img, int mode, int f, int c, int y, int x0, int H, int W) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (mode == IQ_NHWC4) {
    const f32x4* p = reinterpret_cast<const f32x4*>(img) + ((long long)f * H + y) * W + x0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x0 + i < W) {
        const f32x4 px = p[i];
        v[i] = c == 0 ? px.x : (c == 1 ? px.y : px.z);
      }
  } else {
    const float* p = img + (((long long)f * 3 + c) * H + y) * W + x0;
    if (mode == IQ_NCHW_V4) {
      v = *reinterpret_cast<const f32x4*>(p);                      // W % 4 == 0: the whole quad is inside the row
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (x0 + i < W) v[i] = p[i];
    }
  }
  return v;
}

// to_rgb_from_tensor (utils.py:47-49)
__device__ __forceinline__ float iq_rgb(float x) { return fminf(fmaxf(x * 0.5f + 0.5f, 0.f), 1.f); }

__global__ __launch_bounds__(IQ_THREADS, 2) void img_quality_kernel(SdmiImgQualityArgs p, IqGeom G, IqWin win, int pmode,
                                                                    int gmode) {
  extern __shared__ __align__(16) float iq_lds[];
  const int tid = threadIdx.x;
  const int f = blockIdx.x / G.nb, band = blockIdx.x % G.nb;
  const int H = p.H, W = p.W, h = H - 10, w = W - 10;
  const int y0 = band * G.R;                                        // first source row staged = first output row
  // the rows whose pixels this band adds to se / writes as bytes: a partition of [0, H) over the bands
  const int own_lo = band == 0 ? 0 : y0 + 5;
  const int own_hi = band == G.nb - 1 ? H : y0 + G.R + 5;
  float* la = iq_lds;
  float* lb = iq_lds + G.nrows * G.Wp;
  const int qpr = G.Wp / 4, nq = G.nrows * qpr;
  unsigned char* pu8 = (unsigned char*)p.pred_u8;
  unsigned char* gu8 = (unsigned char*)p.gt_u8;
  const int col = tid % G.CW, sub = tid / G.CW;
  const bool works = col < w && sub < G.S;
  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  double se = 0.0, ss = 0.0;

#pragma unroll 1
  for (int c = 0; c < 3; ++c) {
    for (int i = tid; i < nq; i += IQ_THREADS) {
      const int r = i / qpr, x0 = (i - r * qpr) * 4, y = y0 + r;
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
      if (y < H) {
        const f32x4 xa = iq_load4(p.pred, pmode, f, c, y, x0, H, W);
        const f32x4 xb = iq_load4(p.gt, gmode, f, c, y, x0, H, W);
        const bool own = y >= own_lo && y < own_hi;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (x0 + k < W) {
            const float ra = iq_rgb(xa[k]), rb = iq_rgb(xb[k]);
            a[k] = ra * 255.f;
            b[k] = rb * 255.f;
            if (own) {
              const double d = (double)ra - (double)rb;
              se += d * d;
              const long long o = (((long long)f * H + y) * W + x0 + k) * 3 + c;
              if (pu8) pu8[o] = (unsigned char)(int)rintf(a[k]);
              if (gu8) gu8[o] = (unsigned char)(int)rintf(b[k]);
            }
          }
        }
      }
      *reinterpret_cast<f32x4*>(la + r * G.Wp + x0) = a;
      *reinterpret_cast<f32x4*>(lb + r * G.Wp + x0) = b;
    }
    __syncthreads();
    if (works) {
      double acc[IQ_SR][5];
#pragma unroll
      for (int o = 0; o < IQ_SR; ++o)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[o][m] = 0.0;
      int off = (sub * IQ_SR) * G.Wp + col;                         // this thread's window in the current source row
#pragma unroll
      for (int r = 0; r < IQ_ROWS; ++r) {
        double rx = 0, ry = 0, rxx = 0, ryy = 0, rxy = 0;          // rows first, like sdmi_ssim
#pragma unroll
        for (int k = 0; k < 11; ++k) {
          const double A = (double)la[off + k], B = (double)lb[off + k], g = win.g[k];
          rx += g * A; ry += g * B; rxx += g * A * A; ryy += g * B * B; rxy += g * A * B;
        }
#pragma unroll
        for (int o = 0; o < IQ_SR; ++o) {
          if (r - o >= 0 && r - o < 11) {                           // (compile-time after unrolling)
            const double g = win.g[r - o];
            acc[o][0] += g * rx; acc[o][1] += g * ry; acc[o][2] += g * rxx; acc[o][3] += g * ryy; acc[o][4] += g * rxy;
            // One source row at a time.  Left free, the compiler computes the row moments of all 18 unrolled rows before
            // the first accumulator update and spills them: the empty statement makes the next row's LDS offset depend
            // on this row's updates.  It emits no instruction.
            asm volatile("" : "+v"(off), "+v"(acc[o][0]), "+v"(acc[o][1]), "+v"(acc[o][2]), "+v"(acc[o][3]), "+v"(acc[o][4]));
          }
        }
        off += G.Wp;
      }
#pragma unroll
      for (int o = 0; o < IQ_SR; ++o) {
        if (y0 + sub * IQ_SR + o < h) {
          const double ux = acc[o][0], uy = acc[o][1];
          const double vx = acc[o][2] - ux * ux, vy = acc[o][3] - uy * uy, vxy = acc[o][4] - ux * uy;
          ss += ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
        }
      }
    }
    __syncthreads();
  }

  double* red = reinterpret_cast<double*>(iq_lds);                  // (the staged rows are dead: barrier above)
  red[tid] = se;
  red[IQ_THREADS + tid] = ss;
  __syncthreads();
  for (int s = IQ_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      red[IQ_THREADS + tid] += red[IQ_THREADS + tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* out = p.partial + ((long long)f * G.nb + band) * 2;
    out[0] = red[0];
    out[1] = red[IQ_THREADS] / (3.0 * (double)h * (double)w);
  }
}

}  // namespace

extern "C" int sdmi_img_quality(const SdmiImgQualityArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->pred && a->gt && a->partial, "null pointer");
  SDMI_REQUIRE(a->F >= 1, "F >= 1");
  SDMI_REQUIRE(a->H >= 11 && a->W >= 11 && a->W <= 256, "the gate: H >= 11, 11 <= W <= 256");
  SDMI_REQUIRE((a->pred_nhwc4 == 0 || a->pred_nhwc4 == 1) && (a->gt_nhwc4 == 0 || a->gt_nhwc4 == 1),
               "layout flags are 0 (NCHW) or 1 (NHWC-4)");
  SDMI_REQUIRE(((uintptr_t)a->pred & 3) == 0 && ((uintptr_t)a->gt & 3) == 0 && ((uintptr_t)a->partial & 7) == 0,
               "misaligned pointer");
  SDMI_REQUIRE((!a->pred_nhwc4 || ((uintptr_t)a->pred & 15) == 0) && (!a->gt_nhwc4 || ((uintptr_t)a->gt & 15) == 0),
               "NHWC-4 rows must be 16-byte aligned");
  const IqGeom G = iq_geom(a->H, a->W);
  SDMI_REQUIRE(a->nbands == G.nb, "nbands must be the band count of (H, W): metrics.img_quality_bands");
  const long long grid = (long long)a->F * G.nb;
  SDMI_REQUIRE(grid < (1LL << 31) && (long long)a->F * a->H < (1LL << 31), "too many workgroups");
  IqWin win;
  double s = 0.0;
  for (int i = 0; i < 11; ++i) { win.g[i] = exp(-0.5 * (double)((i - 5) * (i - 5)) / (1.5 * 1.5)); s += win.g[i]; }
  for (int i = 0; i < 11; ++i) win.g[i] /= s;
  const int pmode = a->pred_nhwc4 ? IQ_NHWC4 : ((a->W % 4 == 0 && ((uintptr_t)a->pred & 15) == 0) ? IQ_NCHW_V4 : IQ_NCHW);
  const int gmode = a->gt_nhwc4 ? IQ_NHWC4 : ((a->W % 4 == 0 && ((uintptr_t)a->gt & 15) == 0) ? IQ_NCHW_V4 : IQ_NCHW);
  size_t lds = (size_t)2 * G.nrows * G.Wp * sizeof(float);
  if (lds < 2 * IQ_THREADS * sizeof(double)) lds = 2 * IQ_THREADS * sizeof(double);
  SDMI_REQUIRE(lds <= 64 * 1024, "LDS budget");
  hipLaunchKernelGGL(img_quality_kernel, dim3((unsigned)grid), dim3(IQ_THREADS), lds, (hipStream_t)stream, *a, G, win, pmode,
                     gmode);
  return sdmi_check_launch("img_quality");
}
