// Depthwise 3x3 convolution on NHWC fp16 slices: four kernels, bitwise identical to each other.
// Replaces (reference, ultralytics/): nn/modules/conv.py:185-200 DWConv (BN folded by utils/torch_utils.py:237-267)
// and the C2PSA positional-encoding conv (psa.hip calls dwconv3x3).
#include "conv_variant.h"

namespace fce {

// ============================================================================ depthwise 3x3
// HBM-bound (each input pixel read once from HBM, 9x from L2): grid = (row chunks, N*Ho), one
// thread per (output pixel, 8 channels) with 32-bit index math; taps unrolled, weights [9][wcs].
struct DwArgs {
  const _Float16* x;
  int N, H, W, xcs;
  int C, stride;
  int Ho, Wo;
  const float* w;  // [9][wcs] (wcs >= C: a channel slice of a wider packed table)
  int wcs;
  const float* bias;
  _Float16* y;
  int ycs;
  int act;
};

// XCD-aware 2-D block order: block b runs on XCD b % 8; logical block L = (b % 8) * per + b / 8 gives each
// XCD a contiguous run of (x fastest, then y) blocks, so the row bands that share halo rows meet in one L2
__device__ __forceinline__ void xcd_block2(int& bx, int& by) {
  const int gx = int(gridDim.x), total = gx * int(gridDim.y), b = int(blockIdx.y) * gx + int(blockIdx.x);
  const int per = total >> 3, body = per << 3;
  const int L = b < body ? (b & 7) * per + (b >> 3) : b;
  by = L / gx;
  bx = L - by * gx;
}

// One thread = PX adjacent output pixels x 8 channels: the 9 tap weights are loaded once and the
// S*(PX-1)+3 input columns of each row are shared by the PX outputs.
template <int S, int PX>
__global__ __launch_bounds__(256) void dwconv_kernel(DwArgs a) {
  constexpr int NCOL = S * (PX - 1) + 3;
  const int cg8 = a.C >> 3;
  const int Q = (a.Wo + PX - 1) / PX;
  int bx, by;
  xcd_block2(bx, by);  // the rows that share input rows run on one XCD's L2
  const int idx = bx * 256 + threadIdx.x;
  if (idx >= Q * cg8) return;
  const int q = idx / cg8, c0 = (idx - q * cg8) * 8;
  const int row = by, n = row / a.Ho, oy = row - n * a.Ho;
  const int ox0 = q * PX, ix0 = ox0 * S - 1;
  float wk[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const f4 w0 = *reinterpret_cast<const f4*>(a.w + t * a.wcs + c0);
    const f4 w1 = *reinterpret_cast<const f4*>(a.w + t * a.wcs + c0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      wk[t][j] = w0[j];
      wk[t][j + 4] = w1[j];
    }
  }
  float acc[PX][8];
  {
    const f4 b0 = *reinterpret_cast<const f4*>(a.bias + c0);
    const f4 b1 = *reinterpret_cast<const f4*>(a.bias + c0 + 4);
#pragma unroll
    for (int p = 0; p < PX; ++p)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[p][j] = b0[j];
        acc[p][j + 4] = b1[j];
      }
  }
  const _Float16* xn = a.x + int64_t(n) * a.H * a.W * a.xcs + c0;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * S - 1 + ky;
    if (iy < 0 || iy >= a.H) continue;
    const _Float16* xr = xn + int64_t(iy) * a.W * a.xcs;
    h8 v[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      const int ix = ix0 + c;
      v[c] = (ix >= 0 && ix < a.W) ? *reinterpret_cast<const h8*>(xr + int64_t(ix) * a.xcs)
                                   : h8{0, 0, 0, 0, 0, 0, 0, 0};
    }
#pragma unroll
    for (int p = 0; p < PX; ++p)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
        fma8_mix(v[p * S + kx], wk[ky * 3 + kx], acc[p]);
  }
#pragma unroll
  for (int p = 0; p < PX; ++p) {
    if (ox0 + p >= a.Wo) break;
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (_Float16)fpin(a.act ? silu(acc[p][j]) : acc[p][j]);
    *reinterpret_cast<h8*>(a.y + (int64_t(row) * a.Wo + ox0 + p) * a.ycs + c0) = o;
  }
}

// Row-staged variant: one block = (channel slab of CS <= 64 channels, output row).  The 3 input rows
// of the slab are staged in LDS with coalesced 16-byte loads; thread e then owns output
// (pixel e / cg, 8-channel group e % cg), so consecutive lanes store consecutive 16-byte chunks
// (no partial-line writes).  Per pixel the (ky, kx) order and skipped padding taps match dwconv_kernel.
template <int S>
__global__ __launch_bounds__(256) void dwconv_rows_kernel(DwArgs a, int CS) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  int bx, by;
  xcd_block2(bx, by);
  const int c0 = bx * CS;
  const int cs = min(CS, a.C - c0), cg = cs >> 3;
  const int row = by, n = row / a.Ho, oy = row - n * a.Ho;
  float* wl = dsm;              // [9][CS]
  float* bl = wl + 9 * CS;      // [CS]
  h8* rows = reinterpret_cast<h8*>(bl + CS);  // [3][W][CS/8]
  for (int e = threadIdx.x; e < 9 * cs; e += 256) {
    const int t = e / cs, c = e - t * cs;
    wl[t * CS + c] = a.w[t * a.wcs + c0 + c];
  }
  for (int c = threadIdx.x; c < cs; c += 256) bl[c] = a.bias[c0 + c];
  const _Float16* xn = a.x + int64_t(n) * a.H * a.W * a.xcs + c0;
  const int RW = a.W * (CS >> 3);
  for (int r = 0; r < 3; ++r) {
    const int iy = oy * S - 1 + r;
    const bool rin = iy >= 0 && iy < a.H;
    for (int e = threadIdx.x; e < a.W * cg; e += 256) {
      const int xx = e / cg, g = e - xx * cg;
      h8 v = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (rin) v = *reinterpret_cast<const h8*>(xn + (int64_t(iy) * a.W + xx) * a.xcs + 8 * g);
      rows[r * RW + xx * (CS >> 3) + g] = v;
    }
  }
  __syncthreads();
  _Float16* yr = a.y + int64_t(row) * a.Wo * a.ycs + c0;
  for (int e = threadIdx.x; e < a.Wo * cg; e += 256) {
    const int ox = e / cg, g = e - ox * cg;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = bl[8 * g + j];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * S - 1 + ky;
      if (iy < 0 || iy >= a.H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * S - 1 + kx;
        if (ix < 0 || ix >= a.W) continue;
        const h8 v = rows[ky * RW + ix * (CS >> 3) + g];
        const float* wt = wl + (ky * 3 + kx) * CS + 8 * g;
        fma8_mix(v, wt, acc);
      }
    }
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (_Float16)fpin(a.act ? silu(acc[j]) : acc[j]);
    *reinterpret_cast<h8*>(yr + int64_t(ox) * a.ycs + 8 * g) = o;
  }
}

// depthwise 3x3 (pad 1) on NHWC f16 slices; w = [9][wcs] fp32 taps (BN folded), bias fp32 [C]
// Lane-contiguous variant: a block owns one output row; thread t = (pixel slot t / cg, group t % cg)
// with blockDim a multiple of cg, so a thread keeps one channel group (its 9 x 8 weights stay in
// registers) while striding over the row, and every load / store instruction covers consecutive
// 16-byte chunks across lanes.
template <int S>
__global__ __launch_bounds__(256) void dwconv_lanes_kernel(DwArgs a) {
  const int cg = a.C >> 3;
  const int tpx = blockDim.x / cg;  // pixels per sweep
  const int t = threadIdx.x, g = t % cg, px = t / cg;
  const int row = blockIdx.x, n = row / a.Ho, oy = row - n * a.Ho;
  const int c0 = g * 8;
  float wk[9][8], bz[8];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const f4 w0 = *reinterpret_cast<const f4*>(a.w + k * a.wcs + c0);
    const f4 w1 = *reinterpret_cast<const f4*>(a.w + k * a.wcs + c0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      wk[k][j] = w0[j];
      wk[k][j + 4] = w1[j];
    }
  }
  {
    const f4 b0 = *reinterpret_cast<const f4*>(a.bias + c0), b1 = *reinterpret_cast<const f4*>(a.bias + c0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bz[j] = b0[j];
      bz[j + 4] = b1[j];
    }
  }
  const _Float16* xn = a.x + int64_t(n) * a.H * a.W * a.xcs + c0;
  _Float16* yr = a.y + int64_t(row) * a.Wo * a.ycs + c0;
  for (int ox = px; ox < a.Wo; ox += tpx) {
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = bz[j];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * S - 1 + ky;
      if (iy < 0 || iy >= a.H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * S - 1 + kx;
        if (ix < 0 || ix >= a.W) continue;
        const h8 v = *reinterpret_cast<const h8*>(xn + (int64_t(iy) * a.W + ix) * a.xcs);
        fma8_mix(v, wk[ky * 3 + kx], acc);
      }
    }
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (_Float16)fpin(a.act ? silu(acc[j]) : acc[j]);
    *reinterpret_cast<h8*>(yr + int64_t(ox) * a.ycs) = o;
  }
}

// Column-run variant: thread = (output column ox, 8-channel group), consecutive lanes = consecutive
// channel groups then columns, so every load / store instruction covers contiguous pixels (full
// lines); each thread computes PY outputs down its column from (PY-1)*S+3 input rows, every loaded
// row feeding all the outputs that use it.  Out-of-image taps load the zero line and add fmaf(0, w, acc) == acc,
// the value the other variants get by skipping them; each output accumulates its taps in (ky, kx) order with fmaf.
template <int S, int PY>
__global__ __launch_bounds__(256) void dwconv_cols_kernel(DwArgs a) {
  const int cg = a.C >> 3;
  int bx, by;
  xcd_block2(bx, by);
  const int e = bx * 256 + threadIdx.x;
  if (e >= a.Wo * cg) return;
  const int ox = e / cg, g = e - ox * cg, c0 = g * 8;
  const int bands = (a.Ho + PY - 1) / PY;
  const int n = by / bands, oy0 = (by - n * bands) * PY;
  float wk[9][8], acc[PY][8];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const f4 w0 = *reinterpret_cast<const f4*>(a.w + t * a.wcs + c0);
    const f4 w1 = *reinterpret_cast<const f4*>(a.w + t * a.wcs + c0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      wk[t][j] = w0[j];
      wk[t][j + 4] = w1[j];
    }
  }
  {
    const f4 b0 = *reinterpret_cast<const f4*>(a.bias + c0), b1 = *reinterpret_cast<const f4*>(a.bias + c0 + 4);
#pragma unroll
    for (int p = 0; p < PY; ++p)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[p][j] = b0[j];
        acc[p][j + 4] = b1[j];
      }
  }
  const _Float16* xn = a.x + int64_t(n) * a.H * a.W * a.xcs + c0;
  const int iy0 = oy0 * S - 1, ix0 = ox * S - 1;
  bool cok[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) cok[kx] = ix0 + kx >= 0 && ix0 + kx < a.W;
  constexpr int NR = (PY - 1) * S + 3;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int iy = iy0 + r;
    const bool rin = iy >= 0 && iy < a.H;
    h8 v[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const bool ok = rin && cok[kx];
      v[kx] = *(ok ? reinterpret_cast<const h8*>(xn + (int64_t(iy) * a.W + ix0 + kx) * a.xcs)
                   : reinterpret_cast<const h8*>(g_zero_line));
    }
#pragma unroll
    for (int p = 0; p < PY; ++p) {
      const int ky = r - p * S;
      if (ky < 0 || ky > 2) continue;  // compile-time after unrolling
      // an out-of-image tap loaded the zero line: fmaf(0, w, acc) == acc (the skipped tap of the other variants;
      // a select per FMA here was a third of the kernel's VALU work)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const u4 pk = __builtin_bit_cast(u4, v[kx]);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          acc[p][2 * jj] = fma_mix_lo(pk[jj], wk[ky * 3 + kx][2 * jj], acc[p][2 * jj]);
          acc[p][2 * jj + 1] = fma_mix_hi(pk[jj], wk[ky * 3 + kx][2 * jj + 1], acc[p][2 * jj + 1]);
        }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < PY; ++p) {
    if (oy0 + p >= a.Ho) break;
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (_Float16)fpin(a.act ? silu(acc[p][j]) : acc[p][j]);
    *reinterpret_cast<h8*>(a.y + ((int64_t(n) * a.Ho + oy0 + p) * a.Wo + ox) * a.ycs + c0) = o;
  }
}

// Variants (bitwise-identical results; the executor autotunes `variant` per layer, -1 = default).  All
// three accumulate with explicit fmaf in (ky, kx) order and pin the result before the fp16 conversion,
// so hipcc cannot contract them differently.
//   0 pixel-quad (dwconv_kernel<S,4>)   1 row-staged LDS (dwconv_rows_kernel)   2 lane-contiguous
//   3 / 4 column runs of 2 / 4 outputs (dwconv_cols_kernel<S,PY>; runs of 8 measured slower on every n32 op)
int dwconv_variants(int c, int w, int* out, int cap) {
  int n = 0;
  if (n < cap) out[n++] = 0;
  if (n < cap && size_t(10) * 8 * sizeof(float) + size_t(3) * w * 8 * sizeof(_Float16) <= 64 * 1024) out[n++] = 1;
  if (n < cap && c / 8 <= 256) out[n++] = 2;
  if (n < cap) out[n++] = 3;  // column runs of 2
  if (n < cap) out[n++] = 4;  // column runs of 4
  return n;
}

// depthwise 3x3 (pad 1) on NHWC f16 slices; w = [9][wcs] fp32 taps (BN folded), bias fp32 [C]
int dwconv3x3(const fce_tensor& x, int stride, const float* w, int wcs, const float* bias, int act,
              const fce_tensor& y, hipStream_t s, int variant) {
  FCE_CHECK(x.c == y.c && x.c % 8 == 0 && wcs >= x.c && wcs % 4 == 0, "dwconv: channel mismatch");
  FCE_CHECK(x.layout == FCE_NHWC && y.layout == FCE_NHWC && x.dtype == FCE_F16 && y.dtype == FCE_F16,
            "dwconv: NHWC f16 views");
  FCE_CHECK(x.cstride % 8 == 0 && x.coff % 8 == 0 && y.cstride % 8 == 0 && y.coff % 8 == 0,
            "dwconv: slices must be 8-aligned");
  const int Ho = (x.h - 1) / stride + 1, Wo = (x.w - 1) / stride + 1;
  FCE_CHECK(y.n == x.n && y.h == Ho && y.w == Wo, "dwconv: output size mismatch");
  if (int64_t(y.n) * Ho * Wo == 0) return FCE_OK;
  FCE_CHECK(int64_t(y.n) * Ho < 65536 * 1024, "dwconv: too many output rows");
  DwArgs a{static_cast<const _Float16*>(x.data) + x.coff, x.n, x.h, x.w, x.cstride, x.c, stride, Ho, Wo,
           w, wcs, bias, static_cast<_Float16*>(y.data) + y.coff, y.cstride, act};
  if (variant < 0) variant = 0;
  if (variant == 1) {
    for (int CS = std::min(64, x.c); CS >= 8; CS /= 2) {  // row-staged kernel while its LDS fits 64 KiB
      if (CS % 8) continue;
      const size_t lds = size_t(10) * CS * sizeof(float) + size_t(3) * x.w * CS * sizeof(_Float16);
      if (lds > 64 * 1024) continue;
      dim3 g((x.c + CS - 1) / CS, y.n * Ho);
      if (stride == 1)
        FCE_LAUNCH((dwconv_rows_kernel<1>), g, dim3(256), lds, s, a, CS);
      else
        FCE_LAUNCH((dwconv_rows_kernel<2>), g, dim3(256), lds, s, a, CS);
      return launch_status("dwconv_rows_kernel");
    }
  }
  if (variant == 2 && x.c / 8 <= 256) {
    const int cg = x.c / 8;
    const int threads = (256 / cg) * cg;
    if (stride == 1)
      FCE_LAUNCH((dwconv_lanes_kernel<1>), dim3(y.n * Ho), dim3(threads), 0, s, a);
    else
      FCE_LAUNCH((dwconv_lanes_kernel<2>), dim3(y.n * Ho), dim3(threads), 0, s, a);
    return launch_status("dwconv_lanes_kernel");
  }
  if (variant == 3 || variant == 4) {
    const int py = variant == 3 ? 2 : 4;
    const int64_t rows = int64_t(y.n) * ((Ho + py - 1) / py);
    FCE_CHECK(rows < 65536, "dwconv: too many row bands");
    const dim3 g((Wo * (x.c / 8) + 255) / 256, unsigned(rows));
    if (stride == 1 && py == 2)
      FCE_LAUNCH((dwconv_cols_kernel<1, 2>), g, dim3(256), 0, s, a);
    else if (stride == 1)
      FCE_LAUNCH((dwconv_cols_kernel<1, 4>), g, dim3(256), 0, s, a);
    else if (py == 2)
      FCE_LAUNCH((dwconv_cols_kernel<2, 2>), g, dim3(256), 0, s, a);
    else
      FCE_LAUNCH((dwconv_cols_kernel<2, 4>), g, dim3(256), 0, s, a);
    return launch_status("dwconv_cols_kernel");
  }
  constexpr int PX = 4;
  dim3 grid(((Wo + PX - 1) / PX * (x.c / 8) + 255) / 256, y.n * Ho);
  if (stride == 1)
    FCE_LAUNCH((dwconv_kernel<1, PX>), grid, dim3(256), 0, s, a);
  else
    FCE_LAUNCH((dwconv_kernel<2, PX>), grid, dim3(256), 0, s, a);
  return launch_status("dwconv_kernel");
}

// As conv variants the depthwise kernels are coded 100 + variant (any other code: the default kernel)
static int dw_encode(int variant) { return 100 + variant; }
static int dw_decode(int code) { return code >= 100 ? code - 100 : -1; }

int dwconv_candidates(const fce_conv_desc& d, int in_w, int* out, int cap) {
  int v[8];  // every variant dwconv_variants lists (a cap of 4 used to drop the 4-row column runs)
  const int nv = d.k == 3 ? dwconv_variants(d.cin, in_w, v, 8) : 0;
  for (int i = 0; i < nv && i < cap; ++i) out[i] = dw_encode(v[i]);
  return std::min(nv, cap);
}

int dwconv_launch(const fce_conv_desc& d, const fce_tensor& x, const void* w, const float* bias, const fce_tensor& y,
                  hipStream_t s, int code) {
  return dwconv3x3(x, d.stride, static_cast<const float*>(w), d.cin, bias, d.act, y, s, dw_decode(code));
}

}  // namespace fce

