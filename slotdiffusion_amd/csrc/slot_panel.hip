// Slot-decomposition panel kernel (include/sdmi.h: sdmi_slot_panel): Slot Attention's low-resolution attention map (or
// planar alpha masks, or a ground-truth id map) plus the frames -> the 8-bit make_grid panel of the validation pass, in
// one launch.  A workgroup owns one (frame, band of output rows): the source rows of the attention map the band needs
// are staged into LDS with coalesced 16-byte loads (seg_eval.hip's scheme), every thread computes its pixels' bytes of
// ALL tiles into an LDS copy of the band's panel rows, and the workgroup then stores those rows with aligned 32-bit
// stores.  Neither the upsampled masks, nor the id map, nor a float tile reach memory.
//
// Stores: a panel row is GW = K (W + 2) + 2 bytes and starts wherever the strides put it, so rows are not
// dword-aligned (GW = 2342 at the MOVi-E shape).  The LDS copy of a row is therefore laid out with the SAME
// misalignment as its destination (its first byte sits at offset `address & 3` of a 4-byte aligned LDS row): an aligned
// dword of the destination is then an aligned dword of LDS, consecutive lanes store consecutive dwords (256 contiguous
// bytes per wave), and only the at most two edge dwords of a row fall back to byte stores, so that nothing outside the
// rectangle is written.
//
// Compiled with -ffp-contract=off (csrc/build.py), as elementwise.hip and seg_eval.hip are: the interpolation below is
// mask_up_kernel's, expression for expression, and every product and sum of a tile value is rounded on its own, as the
// composed torch path rounds them.
#include "common.h"

namespace {

constexpr int PNL_THREADS = 256;
constexpr int PNL_LDS_BUDGET = 160 * 1024;
enum { PNL_IMG = 0, PNL_RECON = 1, PNL_COLOR = 2, PNL_OVERLAY = 3, PNL_GTCOLOR = 4 };

// first / second source row of output row y (torch's area_pixel source index, align_corners=False)
__host__ __device__ __forceinline__ int pnl_src_lo(float scale, int y) {
  float f = scale * ((float)y + 0.5f) - 0.5f;
  if (f < 0.f) f = 0.f;
  return (int)f;
}
__host__ __device__ __forceinline__ int pnl_src_hi(float scale, int y, int n) {
  const int lo = pnl_src_lo(scale, y);
  return lo + (lo < n - 1 ? 1 : 0);
}

// [-1, 1] -> byte: to_rgb_from_tensor, * 255, astype(uint8) (a truncation)
__device__ __forceinline__ unsigned char pnl_byte(float t) {
  float a = t * 0.5f + 0.5f;
  a = fminf(fmaxf(a, 0.f), 1.f);
  return (unsigned char)(a * 255.f);
}

__device__ __forceinline__ float pnl_px(const float* img, int nhwc4, long long f, int c, int y, int x, int H, int W) {
  return nhwc4 ? img[((f * H + y) * W + x) * 4 + c] : img[((f * 3 + c) * H + y) * W + x];
}

// Store `rows` rows of GW bytes: row r goes to dst + r * dst_pitch and comes from LDS row lds + r * pitch (whose first
// byte is at that row's `address & 3`), or is zero when lds is NULL.  Aligned dwords inside the row are 32-bit stores.
__device__ __forceinline__ void pnl_store_rows(unsigned char* dst, long long dst_pitch, const unsigned char* lds,
                                               int pitch, int rows, int GW, int tid) {
  const int ndw = pitch >> 2;
  for (int i = tid; i < rows * ndw; i += PNL_THREADS) {
    const int r = i / ndw, lo = (i % ndw) * 4;
    unsigned char* g = dst + (long long)r * dst_pitch;
    const int mis = (int)((uintptr_t)g & 3);
    if (lo >= mis + GW) continue;
    unsigned char* ga = g - mis;                         // the aligned window of this row; only [mis, mis + GW) is ours
    const unsigned char* l = lds ? lds + (long long)r * pitch : nullptr;
    if (lo >= mis && lo + 4 <= mis + GW) {
      *reinterpret_cast<unsigned*>(ga + lo) = l ? *reinterpret_cast<const unsigned*>(l + lo) : 0u;
    } else {
      for (int b = 0; b < 4; ++b) {
        const int q = lo + b;
        if (q >= mis && q < mis + GW) ga[q] = l ? l[q] : (unsigned char)0;
      }
    }
  }
}

// grid (F * nbands): workgroup = (frame, band of `band` output rows).  LDS: stage_floats floats of source rows (layout 0
// only; 16-byte aligned, the first `lead` of them alignment slack), band * W ints of predicted ids, then
// 3 * band rows of `pitch` panel bytes.
__global__ __launch_bounds__(PNL_THREADS) void slot_panel_kernel(SdmiSlotPanelArgs p, int band, int nbands, int srows,
                                                                 int stage_floats, int pitch) {
  extern __shared__ __attribute__((aligned(16))) char pnl_smem[];
  float* stage = reinterpret_cast<float*>(pnl_smem);
  int* amap = reinterpret_cast<int*>(pnl_smem + (size_t)stage_floats * sizeof(float));
  unsigned char* rowsb = reinterpret_cast<unsigned char*>(amap + band * p.W);
  const int tid = threadIdx.x;
  const long long f = blockIdx.x / nbands;
  const int bidx = blockIdx.x % nbands;
  const int r0 = bidx * band;
  const int r1 = r0 + band < p.H ? r0 + band : p.H;
  const int nr = r1 - r0;
  const int K = p.nprefix + p.N;
  const int GW = K * (p.W + 2) + 2;
  const int H = p.H, W = p.W, N = p.N;

  const float sy = (float)p.h / (float)p.H, sx = (float)p.w / (float)p.W;
  const int ylo = pnl_src_lo(sy, r0);
  int lead = 0;
  if (p.seg && !p.seg_planar) {
    int nrows = pnl_src_hi(sy, r1 - 1, p.h) - ylo + 1;
    if (nrows > srows) nrows = srows;           // (the host sized srows from these same expressions)
    // stage rows ylo .. ylo + nrows - 1 of frame f: one contiguous run of the source, read as aligned 16-byte vectors
    const long long total = (long long)p.F * p.h * p.w * N;
    const long long e0 = (f * p.h + ylo) * p.w * N;
    const long long e1 = e0 + (long long)nrows * p.w * N;
    const long long a0 = e0 & ~3LL;
    lead = (int)(e0 - a0);
    const int ngroups = (int)((e1 - a0 + 3) >> 2);
    for (int g = tid; g < ngroups; g += PNL_THREADS) {
      const long long e = a0 + 4LL * g;
      if (e + 4 <= total) {
        *reinterpret_cast<float4*>(stage + 4 * g) = *reinterpret_cast<const float4*>(p.seg + e);
      } else {
        for (int j = 0; j < 4; ++j)
          if (e + j < total) stage[4 * g + j] = p.seg[e + j];
      }
    }
  }
  __syncthreads();

  const long long im = f / p.G;
  const int grow = (int)(f % p.G);
  const long long prow0 = (long long)grow * (H + 2) + 2 + r0;      // panel row of the band's first row
  const float ov_a = 0.7f, ov_b = (float)(1.0 - 0.7);             // torch_draw_rgb_mask's alpha and 1 - alpha
  const float* s = stage + lead;
  const float* planar = p.seg_planar ? p.seg + f * N * (long long)p.h * p.w : nullptr;
  const long long kstride = p.seg_planar ? (long long)p.h * p.w : 1;

  for (int pass = 0; pass < (p.hard ? 2 : 1); ++pass) {
    unsigned char* out = reinterpret_cast<unsigned char*>(pass ? p.hard : p.soft) + im * p.img_stride;
    // the band's panel rows start every pass as padding (byte 0 = pad_value -1) and pixels overwrite their own bytes
    // only.  Zeroed per pass: a row sits at ITS destination's `address & 3`, which soft and hard need not share, so
    // the first pass's pixel bytes could otherwise show through the second pass's padding columns.
    for (int i = tid; i < (3 * band * pitch) >> 2; i += PNL_THREADS) reinterpret_cast<unsigned*>(rowsb)[i] = 0u;
    __syncthreads();
    for (int i = tid; i < nr * W; i += PNL_THREADS) {
      const int ry = i / W, x = i % W, y = r0 + ry;
      int lo[3];                                 // LDS offset of the row's first byte, per channel
      for (int c = 0; c < 3; ++c) {
        const unsigned char* g = out + c * p.ch_stride + (prow0 + ry) * p.row_stride;
        lo[c] = (c * band + ry) * pitch + (int)((uintptr_t)g & 3);
      }
      float v[3];
      for (int c = 0; c < 3; ++c) v[c] = pnl_px(p.img, p.img_nhwc4, f, c, y, x, H, W);

      // the mask taps of this pixel (mask_up_kernel's expressions)
      float fy = sy * ((float)y + 0.5f) - 0.5f;
      float fx = sx * ((float)x + 0.5f) - 0.5f;
      if (fy < 0.f) fy = 0.f;
      if (fx < 0.f) fx = 0.f;
      const int y0 = (int)fy, x0 = (int)fx;
      const int y1 = y0 + (y0 < p.h - 1 ? 1 : 0), x1 = x0 + (x0 < p.w - 1 ? 1 : 0);
      const float ly1 = fy - (float)y0, ly0 = 1.f - ly1;
      const float lx1 = fx - (float)x0, lx0 = 1.f - lx1;
      const float *s00 = nullptr, *s01 = nullptr, *s10 = nullptr, *s11 = nullptr;
      if (planar) {
        s00 = planar + (long long)y0 * p.w + x0;
        s01 = planar + (long long)y0 * p.w + x1;
        s10 = planar + (long long)y1 * p.w + x0;
        s11 = planar + (long long)y1 * p.w + x1;
      } else if (p.seg) {
        int ry0 = y0 - ylo, ry1 = y1 - ylo;
        if (ry0 > srows - 1) ry0 = srows - 1;     // never read past the staged rows
        if (ry1 > srows - 1) ry1 = srows - 1;
        s00 = s + (ry0 * p.w + x0) * N;
        s01 = s + (ry0 * p.w + x1) * N;
        s10 = s + (ry1 * p.w + x0) * N;
        s11 = s + (ry1 * p.w + x1) * N;
      }

      int a;                                      // predicted id; -1: an id outside [0, N)
      if (pass) {
        a = amap[i];
      } else {
        if (p.ids) {
          a = p.ids[(f * H + y) * W + x];
          if ((unsigned)a >= (unsigned)N) a = -1;
        } else {
          float best = -INFINITY;
          a = 0;
          for (int k = 0; k < N; ++k) {
            const long long o = k * kstride;
            const float m = ly0 * (lx0 * s00[o] + lx1 * s01[o]) + ly1 * (lx0 * s10[o] + lx1 * s11[o]);
            if (m > best) { best = m; a = k; }
          }
        }
        amap[i] = a;
      }

      for (int j = 0; j < p.nprefix; ++j) {
        const int code = (int)((p.tiles >> (4 * j)) & 15u);
        const int col = 2 + j * (W + 2) + x;
        int cid = a;
        if (code == PNL_GTCOLOR) {
          cid = p.gt[(f * H + y) * W + x];
          if ((unsigned)cid >= (unsigned)p.P) cid = -1;
        }
        for (int c = 0; c < 3; ++c) {
          float t = 0.f;
          bool zero = false;
          if (code == PNL_IMG) {
            t = v[c];
          } else if (code == PNL_RECON) {
            t = pnl_px(p.recon, p.recon_nhwc4, f, c, y, x, H, W);
          } else if (cid < 0) {
            zero = true;
          } else if (code == PNL_OVERLAY) {
            t = v[c] * ov_a + p.palette[cid * 3 + c] * ov_b;
          } else {
            t = p.palette[cid * 3 + c];
          }
          rowsb[lo[c] + col] = zero ? (unsigned char)0 : pnl_byte(t);
        }
      }

      for (int k = 0; k < N; ++k) {
        float m;
        if (pass || p.ids) {
          m = (k == a) ? 1.f : 0.f;               // make_one_hot / F.one_hot
        } else {
          const long long o = k * kstride;
          m = ly0 * (lx0 * s00[o] + lx1 * s01[o]) + ly1 * (lx0 * s10[o] + lx1 * s11[o]);
        }
        const float bg = 1.f - m;
        const int col = 2 + (p.nprefix + k) * (W + 2) + x;
        for (int c = 0; c < 3; ++c) {
          const float sc = p.slot_img ? p.slot_img[(((f * N + k) * 3 + c) * H + y) * W + x] : v[c];
          rowsb[lo[c] + col] = pnl_byte(sc * m + bg);
        }
      }
    }
    __syncthreads();

    for (int c = 0; c < 3; ++c) {
      unsigned char* oc = out + c * p.ch_stride;
      pnl_store_rows(oc + prow0 * p.row_stride, p.row_stride, rowsb + (long long)c * band * pitch, pitch, nr, GW, tid);
      // the padding rows: the two above a frame's tiles (its first band), the two that close the picture (the last
      // band of the last tile row)
      if (bidx == 0)
        pnl_store_rows(oc + (prow0 - 2) * p.row_stride, p.row_stride, nullptr, pitch, 2, GW, tid);
      if (bidx == nbands - 1 && grow == p.G - 1)
        pnl_store_rows(oc + (prow0 + nr) * p.row_stride, p.row_stride, nullptr, pitch, 2, GW, tid);
    }
    __syncthreads();
  }
}

// the most source rows any band of `band` output rows touches (the kernel's own expressions, on the host)
int pnl_band_rows(int band, int h, int H) {
  const float sy = (float)h / (float)H;
  int most = 1;
  for (int r0 = 0; r0 < H; r0 += band) {
    const int r1 = r0 + band < H ? r0 + band : H;
    const int n = pnl_src_hi(sy, r1 - 1, h) - pnl_src_lo(sy, r0) + 1;
    if (n > most) most = n;
  }
  return most;
}

// band height for a shape: the largest of 8, 4, 2, 1 (at most H) whose LDS need fits the budget; 0 when none does
int pnl_plan(const SdmiSlotPanelArgs* a, int* srows, long long* stage_floats, int* pitch, long long* lds) {
  const long long GW = ((long long)a->nprefix + a->N) * (a->W + 2) + 2;
  *pitch = (int)((GW + 3 + 3) / 4 * 4);
  int band = 8;
  while (band > a->H) band /= 2;
  for (; band >= 1; band /= 2) {
    *srows = 0;
    *stage_floats = 0;
    if (a->seg && !a->seg_planar) {
      *srows = pnl_band_rows(band, a->h, a->H);
      *stage_floats = ((long long)*srows * a->w * a->N + 8 + 3) / 4 * 4;
    }
    *lds = *stage_floats * 4 + (long long)band * a->W * 4 + 3LL * band * *pitch;
    if (*lds <= PNL_LDS_BUDGET) return band;
  }
  return 0;
}

}  // namespace

extern "C" int sdmi_slot_panel(const SdmiSlotPanelArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->img && a->soft, "null pointer (img, soft)");
  SDMI_REQUIRE((a->seg != nullptr) != (a->ids != nullptr), "exactly one mask source: seg or ids");
  SDMI_REQUIRE(a->N >= 1, "N >= 1");
  SDMI_REQUIRE(a->h >= 1 && a->w >= 1 && a->H >= 1 && a->W >= 1, "h, w, H, W >= 1");
  SDMI_REQUIRE(a->F >= 1 && a->G >= 1 && a->F % a->G == 0, "F >= 1, G >= 1, F a multiple of G");
  SDMI_REQUIRE(a->nprefix >= 0 && a->nprefix <= 8, "nprefix in [0, 8]");
  SDMI_REQUIRE((a->img_nhwc4 | 1) == 1 && (a->recon_nhwc4 | 1) == 1 && (a->seg_planar | 1) == 1,
               "layout flags are 0 or 1");
  bool colour = false, pal = false;
  for (int j = 0; j < a->nprefix; ++j) {
    const unsigned code = (a->tiles >> (4 * j)) & 15u;
    SDMI_REQUIRE(code <= (unsigned)PNL_GTCOLOR, "unknown tile code");
    SDMI_REQUIRE(code != (unsigned)PNL_RECON || a->recon, "a RECON tile needs recon");
    SDMI_REQUIRE(code != (unsigned)PNL_GTCOLOR || a->gt, "a GTCOLOR tile needs gt");
    colour = colour || code == (unsigned)PNL_COLOR || code == (unsigned)PNL_OVERLAY;
    pal = pal || code >= (unsigned)PNL_COLOR;
  }
  SDMI_REQUIRE(!pal || (a->palette && a->P >= 1), "colour tiles need a palette, P >= 1");
  SDMI_REQUIRE(!colour || a->N <= a->P, "COLOR / OVERLAY tiles need N <= P");
  SDMI_REQUIRE(a->seg == nullptr || a->seg_planar || ((uintptr_t)a->seg & 15) == 0, "seg must be 16-byte aligned");
  const long long GW = ((long long)a->nprefix + a->N) * ((long long)a->W + 2) + 2;
  const long long GH = (long long)a->G * ((long long)a->H + 2) + 2;
  SDMI_REQUIRE(GW < (1LL << 24) && (long long)a->H * a->W < (1LL << 31) && (long long)a->h * a->w * a->N < (1LL << 31) &&
                   a->F < (1 << 20), "frame too large");
  SDMI_REQUIRE(a->row_stride >= GW && a->ch_stride >= 0 && a->img_stride >= 0, "strides: row_stride >= GW, none negative");
  const long long plane = (GH - 1) * a->row_stride + GW;          // bytes from a plane's first byte to its last
  SDMI_REQUIRE(a->ch_stride >= plane, "ch_stride: the three channel planes overlap");
  SDMI_REQUIRE(a->F == a->G || a->img_stride >= 2 * a->ch_stride + plane, "img_stride: the pictures overlap");
  int srows = 0, pitch = 0;
  long long stage_floats = 0, lds = 0;
  const int band = pnl_plan(a, &srows, &stage_floats, &pitch, &lds);
  if (band == 0) {
    sdmi_set_error("%s: LDS budget: one band row of %lld panel bytes x 3 and its source rows exceed %d", __func__, GW,
                   PNL_LDS_BUDGET);
    return SDMI_EUNSUPPORTED;
  }
  const int nbands = (a->H + band - 1) / band;
  const long long grid = (long long)a->F * nbands;
  SDMI_REQUIRE(grid < (1LL << 31), "too many workgroups");
  SDMI_OPTIN_LDS(slot_panel_kernel, PNL_LDS_BUDGET, "slot_panel");
  hipLaunchKernelGGL(slot_panel_kernel, dim3((unsigned)grid), dim3(PNL_THREADS), (size_t)lds, (hipStream_t)stream, *a,
                     band, nbands, srows, (int)stage_floats, pitch);
  return sdmi_check_launch("slot_panel");
}
