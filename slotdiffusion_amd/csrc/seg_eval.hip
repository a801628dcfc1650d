// Segmentation evaluation kernel (include/sdmi.h: sdmi_seg_tables): Slot Attention's low-resolution attention map
// -> bilinear upsample -> argmax over slots -> (gt id, predicted id) contingency tables, in one pass.  HBM-bound
// integer work: the source rows a band of output rows needs are staged into LDS with coalesced 16-byte loads, every
// thread computes its pixels from LDS, the counts go through LDS integer atomics into a per-workgroup copy of the
// tables, and one global integer atomic per non-empty cell adds that copy to the sample's tables.  Neither the
// upsampled masks nor (unless asked for) the id map reach memory.
//
// Compiled with -ffp-contract=off (csrc/build.py), as elementwise.hip is: the interpolation below is mask_up_kernel's,
// expression for expression, so the two argmaxes agree bit for bit.
#include "common.h"

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_LDS_BUDGET = 160 * 1024;

// first source row of output row y, and the second one (torch's area_pixel source index, align_corners=False)
__host__ __device__ __forceinline__ int seg_src_lo(float scale, int y) {
  float f = scale * ((float)y + 0.5f) - 0.5f;
  if (f < 0.f) f = 0.f;
  return (int)f;
}
__host__ __device__ __forceinline__ int seg_src_hi(float scale, int y, int n) {
  const int lo = seg_src_lo(scale, y);
  return lo + (lo < n - 1 ? 1 : 0);
}

// grid (B * T * nbands): workgroup = (frame, band of `band` output rows).  LDS: stage_floats floats of source rows
// (16-byte aligned, the first `lead` of them alignment slack), then maps * (Kg + 1) * N ints.
__global__ __launch_bounds__(SEG_THREADS) void seg_tables_kernel(SdmiSegTablesArgs p, int band, int nbands, int srows,
                                                                 int stage_floats) {
  extern __shared__ __attribute__((aligned(16))) char seg_smem[];
  float* stage = reinterpret_cast<float*>(seg_smem);
  int* hist = reinterpret_cast<int*>(seg_smem + (size_t)stage_floats * sizeof(float));
  const int tid = threadIdx.x;
  const int f = blockIdx.x / nbands;
  const int r0 = (blockIdx.x % nbands) * band;
  const int r1 = r0 + band < p.H ? r0 + band : p.H;
  int b, t;
  if (p.time_major) { t = f / p.B; b = f % p.B; } else { b = f / p.T; t = f % p.T; }
  const int maps = p.gt2 ? 2 : 1;
  const int cells = (p.Kg + 1) * p.N;
  for (int i = tid; i < maps * cells; i += SEG_THREADS) hist[i] = 0;

  const float sy = (float)p.h / (float)p.H, sx = (float)p.w / (float)p.W;
  const int ylo = seg_src_lo(sy, r0);
  int nrows = seg_src_hi(sy, r1 - 1, p.h) - ylo + 1;
  if (nrows > srows) nrows = srows;             // (the host sized srows from these same expressions)

  // stage rows ylo .. ylo + nrows - 1 of frame f: one contiguous run of the source, read as aligned 16-byte vectors
  const long long total = (long long)p.B * p.T * p.h * p.w * p.N;
  const long long e0 = ((long long)f * p.h + ylo) * p.w * p.N;
  const long long e1 = e0 + (long long)nrows * p.w * p.N;
  const long long a0 = e0 & ~3LL;
  const int lead = (int)(e0 - a0);
  const int ngroups = (int)((e1 - a0 + 3) >> 2);
  for (int g = tid; g < ngroups; g += SEG_THREADS) {
    const long long e = a0 + 4LL * g;
    if (e + 4 <= total) {
      *reinterpret_cast<float4*>(stage + 4 * g) = *reinterpret_cast<const float4*>(p.seg + e);
    } else {
      for (int j = 0; j < 4; ++j)
        if (e + j < total) stage[4 * g + j] = p.seg[e + j];
    }
  }
  __syncthreads();

  const float* s = stage + lead;
  const int npix = (r1 - r0) * p.W;
  const long long mbase = (long long)b * p.map_bstride + (long long)t * p.map_tstride;
  const int ov_cell = p.Kg * p.N;
  int cur0 = -1, n0 = 0, cur1 = -1, n1 = 0;      // run of equal cells per thread: one LDS atomic per run
  for (int i = tid; i < npix; i += SEG_THREADS) {
    const int y = r0 + i / p.W;
    const int x = i % p.W;
    float fy = sy * ((float)y + 0.5f) - 0.5f;
    float fx = sx * ((float)x + 0.5f) - 0.5f;
    if (fy < 0.f) fy = 0.f;
    if (fx < 0.f) fx = 0.f;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < p.h - 1 ? 1 : 0), x1 = x0 + (x0 < p.w - 1 ? 1 : 0);
    const float ly1 = fy - (float)y0, ly0 = 1.f - ly1;
    const float lx1 = fx - (float)x0, lx0 = 1.f - lx1;
    int ry0 = y0 - ylo, ry1 = y1 - ylo;
    if (ry0 > srows - 1) ry0 = srows - 1;         // never read past the staged rows
    if (ry1 > srows - 1) ry1 = srows - 1;
    const float* s00 = s + (ry0 * p.w + x0) * p.N;
    const float* s01 = s + (ry0 * p.w + x1) * p.N;
    const float* s10 = s + (ry1 * p.w + x0) * p.N;
    const float* s11 = s + (ry1 * p.w + x1) * p.N;
    float best = -INFINITY;
    int bi = 0;
    for (int k = 0; k < p.N; ++k) {
      const float v00 = s00[k], v01 = s01[k], v10 = s10[k], v11 = s11[k];
      const float v = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
      if (v > best) { best = v; bi = k; }
    }
    const long long pix = (long long)y * p.W + x;
    if (p.ids) {
      const long long o = (long long)f * p.H * p.W + pix;
      if (p.ids_u8) reinterpret_cast<unsigned char*>(p.ids)[o] = (unsigned char)bi;
      else reinterpret_cast<int*>(p.ids)[o] = bi;
    }
    const bool ov = p.overlap && p.overlap[mbase + pix] != 0;
    const int c0 = p.gt[mbase + pix];
    const int cell0 = ov ? ov_cell + bi : ((unsigned)c0 < (unsigned)p.Kg ? c0 * p.N + bi : -1);
    if (cell0 != cur0) {
      if (cur0 >= 0) atomicAdd(&hist[cur0], n0);
      cur0 = cell0;
      n0 = 0;
    }
    ++n0;
    if (p.gt2) {
      const int c1 = p.gt2[mbase + pix];
      const int cell1 = ov ? ov_cell + bi : ((unsigned)c1 < (unsigned)p.Kg ? c1 * p.N + bi : -1);
      if (cell1 != cur1) {
        if (cur1 >= 0) atomicAdd(&hist[cells + cur1], n1);
        cur1 = cell1;
        n1 = 0;
      }
      ++n1;
    }
  }
  if (cur0 >= 0) atomicAdd(&hist[cur0], n0);
  if (cur1 >= 0) atomicAdd(&hist[cells + cur1], n1);
  __syncthreads();
  int* out = p.counts + (long long)b * maps * cells;
  for (int i = tid; i < maps * cells; i += SEG_THREADS)
    if (hist[i]) atomicAdd(&out[i], hist[i]);
}

// the most source rows any band of `band` output rows touches (the kernel's own expressions, on the host)
int seg_band_rows(int band, int h, int H) {
  const float sy = (float)h / (float)H;
  int most = 1;
  for (int r0 = 0; r0 < H; r0 += band) {
    const int r1 = r0 + band < H ? r0 + band : H;
    const int n = seg_src_hi(sy, r1 - 1, h) - seg_src_lo(sy, r0) + 1;
    if (n > most) most = n;
  }
  return most;
}

}  // namespace

extern "C" int sdmi_seg_tables(const SdmiSegTablesArgs* a, void* stream) {
  SDMI_REQUIRE(a && a->seg && a->gt && a->counts, "null pointer");
  SDMI_REQUIRE(a->N >= 1, "N >= 1");
  SDMI_REQUIRE(a->h >= 1 && a->w >= 1 && a->H >= 1 && a->W >= 1, "h, w, H, W >= 1");
  SDMI_REQUIRE(a->B >= 1 && a->T >= 1 && (a->time_major == 0 || a->time_major == 1), "B, T >= 1, time_major 0 or 1");
  SDMI_REQUIRE(a->Kg >= 1 && ((long long)a->Kg + 1) * a->N <= 8192, "bad table size: (Kg + 1) * N <= 8192");
  SDMI_REQUIRE(a->ids_u8 == 0 || (a->ids_u8 == 1 && a->N <= 256), "ids_u8 is 0 or 1, uint8 ids need N <= 256");
  SDMI_REQUIRE(a->map_bstride >= 0 && a->map_tstride >= 0, "negative map stride");
  SDMI_REQUIRE(((uintptr_t)a->seg & 15) == 0, "seg must be 16-byte aligned");
  SDMI_REQUIRE((long long)a->H * a->W < (1LL << 31) && (long long)a->h * a->w * a->N < (1LL << 31) &&
                   (long long)a->B * a->T < (1LL << 20), "frame too large");
  const int maps = a->gt2 ? 2 : 1;
  const long long table_bytes = (long long)maps * (a->Kg + 1) * a->N * (long long)sizeof(int);
  int band = a->H >= 64 ? 16 : 8;
  if (band > a->H) band = a->H;
  int srows = 0;
  long long stage_floats = 0;
  for (;; band /= 2) {
    srows = seg_band_rows(band, a->h, a->H);
    stage_floats = ((long long)srows * a->w * a->N + 8 + 3) / 4 * 4;
    if (stage_floats * 4 + table_bytes <= SEG_LDS_BUDGET) break;
    if (band == 1) {
      sdmi_set_error("%s: LDS budget: %lld bytes of tables and one source row of %d x %d floats exceed %d", __func__,
                     table_bytes, a->w, a->N, SEG_LDS_BUDGET);
      return SDMI_EUNSUPPORTED;
    }
  }
  const int nbands = (a->H + band - 1) / band;
  const long long grid = (long long)a->B * a->T * nbands;
  SDMI_REQUIRE(grid < (1LL << 31), "too many workgroups");
  SDMI_OPTIN_LDS(seg_tables_kernel, SEG_LDS_BUDGET, "seg_tables");
  hipLaunchKernelGGL(seg_tables_kernel, dim3((unsigned)grid), dim3(SEG_THREADS),
                     (size_t)(stage_floats * 4 + table_bytes), (hipStream_t)stream, *a, band, nbands, srows,
                     (int)stage_floats);
  return sdmi_check_launch("seg_tables");
}
