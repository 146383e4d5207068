// The Cin<=4 stem: reads the NCHW network input (f16 / f32 / u8) directly, writes NHWC fp16.
// Replaces (reference, ultralytics/): nn/modules/conv.py:39-89 Conv.forward_fuse of the first layer, with the BN
// folded by utils/torch_utils.py:237-267.
#include <type_traits>

#include "conv_variant.h"

namespace fce {

// ============================================================================ stem (NCHW input, cin <= 4)
struct StemArgs {
  const void* x;
  int dtype;
  int N, C, H, W;
  int stride, k;
  int Ho, Wo, cout;
  const float* w;  // [ci][ky][kx][co]
  const float* bias;
  _Float16* y;
  int ycs;
  int act;
};

template <typename T>
__device__ __forceinline__ float ld_in(const T* p, int64_t i);
template <>
__device__ __forceinline__ float ld_in<_Float16>(const _Float16* p, int64_t i) {
  return (float)p[i];
}
template <>
__device__ __forceinline__ float ld_in<float>(const float* p, int64_t i) {
  return p[i];
}
// uint8 network input: the reference preprocess (predictor.py:151-173) computes `im.half() / 255`, i.e.
// the fp16 rounding of v / 255 — the value the fp16 model sees for every pixel
__device__ __forceinline__ float u8_to_unit(unsigned v) { return (float)(_Float16)((float)v / 255.0f); }
template <>
__device__ __forceinline__ float ld_in<uint8_t>(const uint8_t* p, int64_t i) {
  return u8_to_unit(p[i]);
}

template <int COUT, typename T>
__global__ __launch_bounds__(256) void stem_kernel(StemArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int nw = a.C * a.k * a.k * COUT;
  for (int i = threadIdx.x; i < nw; i += blockDim.x) {
    const int co = i % COUT, r = i / COUT;
    smem[i] = co < a.cout ? a.w[r * a.cout + co] : 0.f;
  }
  __syncthreads();
  const T* x = static_cast<const T*>(a.x);
  const int64_t P = int64_t(a.N) * a.Ho * a.Wo;
  const int pad = a.k / 2;
  for (int64_t pix = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; pix < P; pix += int64_t(gridDim.x) * blockDim.x) {
    const int ox = int(pix % a.Wo);
    const int oy = int((pix / a.Wo) % a.Ho);
    const int n = int(pix / (int64_t(a.Wo) * a.Ho));
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = 0.f;
    for (int ci = 0; ci < a.C; ++ci) {
      const int64_t plane = (int64_t(n) * a.C + ci) * a.H * a.W;
      for (int ky = 0; ky < a.k; ++ky) {
        const int iy = oy * a.stride - pad + ky;
        if (iy < 0 || iy >= a.H) continue;
        for (int kx = 0; kx < a.k; ++kx) {
          const int ix = ox * a.stride - pad + kx;
          if (ix < 0 || ix >= a.W) continue;
          const float v = ld_in<T>(x, plane + int64_t(iy) * a.W + ix);
          const float* wt = smem + ((ci * a.k + ky) * a.k + kx) * COUT;
#pragma unroll
          for (int co = 0; co < COUT; ++co) acc[co] += v * wt[co];
        }
      }
    }
    _Float16* yo = a.y + pix * a.ycs;
#pragma unroll
    for (int co0 = 0; co0 < COUT; co0 += 8) {
      if (co0 >= a.cout) break;
      h8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int co = co0 + j;
        const float t = acc[co] + bias_or0(a.bias, co, a.cout);
        o[j] = (_Float16)(a.act ? silu(t) : t);
      }
      *reinterpret_cast<h8*>(yo + co0) = o;
    }
  }
}

// 3x3 stride-2 stem (the network's first Conv, 640 -> 320): one thread = PX adjacent output pixels
// of one row.  Their receptive columns are the aligned run x[2*PX*q .. 2*PX*q + 2PX-1] plus the
// element before it, so each (ci, ky) costs one vector load + one scalar load instead of 3*PX.
// Weights [ci][ky][kx][co] broadcast from LDS; same per-pixel summation order as stem_kernel.
// NE consecutive input elements held as raw 32-bit words (one aligned vector load)
template <typename T, int NE>
struct RawRun {
  static constexpr int NW = (int(sizeof(T)) * NE + 3) / 4;
  uint32_t w[NW];
  __device__ __forceinline__ void load(const T* p) {
    if constexpr (NW == 8) {
      const uint4 lo = reinterpret_cast<const uint4*>(p)[0], hi = reinterpret_cast<const uint4*>(p)[1];
      w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w; w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
    } else if constexpr (NW == 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else if constexpr (NW == 2) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      w[0] = v.x; w[1] = v.y;
    } else {
      static_assert(NW == 1, "run size");
      w[0] = *reinterpret_cast<const uint32_t*>(p);
    }
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = 0u;
  }
  __device__ __forceinline__ float get(int e) const {
    if constexpr (sizeof(T) == 4) {
      return __uint_as_float(w[e]);
    } else if constexpr (sizeof(T) == 2) {
      const unsigned short h = (unsigned short)(w[e >> 1] >> ((e & 1) * 16));
      return (float)__ushort_as_half(h);
    } else {
      return u8_to_unit((w[e >> 2] >> ((e & 3) * 8)) & 255u);
    }
  }
};

template <int COUT, int PX, typename T>
__global__ __launch_bounds__(256) void stem_s2_kernel(StemArgs a) {
  // RGB input (CIN = 3).  Output: when the view is a dense [pixel][COUT] buffer the block stages its
  // results in LDS and each store instruction writes 64 x 16 contiguous bytes (direct per-thread
  // stores at a 32*PX-byte lane stride reach HBM as partial lines: 2.4x the output bytes measured).
  constexpr int CIN = 3, NE = 2 * PX, CPT = PX * COUT / 8;  // 16-byte chunks per thread
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int nw = CIN * 9 * COUT;
  for (int i = threadIdx.x; i < nw; i += blockDim.x) {
    const int co = i % COUT, r = i / COUT;
    smem[i] = co < a.cout ? a.w[r * a.cout + co] : 0.f;
  }
  __syncthreads();
  const int Q = (a.Wo + PX - 1) / PX;
  const int nthreads = a.N * a.Ho * Q;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const bool valid = idx < nthreads;
  const int row = valid ? idx / Q : 0, q = valid ? idx - row * Q : 0;
  const int n = row / a.Ho, oy = row - n * a.Ho;
  const int ix0 = 2 * PX * q;
  const bool interior = ix0 + NE <= a.W;
  const T* x = static_cast<const T*>(a.x);
  float acc[PX][COUT];
#pragma unroll
  for (int j = 0; j < PX; ++j)
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[j][co] = 0.f;
#pragma unroll 1
  for (int ci = 0; ci < CIN; ++ci) {
    RawRun<T, NE> run[3];
    float pre[3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {  // the three row loads of a channel are issued together
      const int iy = 2 * oy - 1 + ky;
      const bool rin = valid && iy >= 0 && iy < a.H;
      const T* rp = x + ((int64_t(n) * CIN + ci) * a.H + (rin ? iy : 0)) * a.W;
      pre[ky] = (rin && ix0 > 0) ? ld_in<T>(rp, ix0 - 1) : 0.f;
      if (rin && interior)
        run[ky].load(rp + ix0);
      else  // rows outside the image (the dispatcher only launches this kernel for W % 2PX == 0)
        run[ky].zero();
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      float v[NE + 1];
      v[0] = pre[ky];
#pragma unroll
      for (int e = 0; e < NE; ++e) v[1 + e] = run[ky].get(e);
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float* wt = smem + ((ci * 3 + ky) * 3 + kx) * COUT;
#pragma unroll
        for (int co = 0; co < COUT; co += 4) {
          const f4 w4 = *reinterpret_cast<const f4*>(wt + co);
#pragma unroll
          for (int j = 0; j < PX; ++j) {
            const float xv = v[2 * j + kx];
            acc[j][co] += xv * w4[0];
            acc[j][co + 1] += xv * w4[1];
            acc[j][co + 2] += xv * w4[2];
            acc[j][co + 3] += xv * w4[3];
          }
        }
      }
    }
  }
  h8 o[PX][COUT / 8];
#pragma unroll
  for (int j = 0; j < PX; ++j)
#pragma unroll
    for (int c8 = 0; c8 < COUT / 8; ++c8)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int co = c8 * 8 + e;
        const float t = acc[j][co] + bias_or0(a.bias, co, a.cout);
        o[j][c8][e] = (_Float16)(a.act ? silu(t) : t);
      }
  if (a.cout == COUT && a.ycs == COUT) {
    h8* st = reinterpret_cast<h8*>(smem + nw);  // [256][CPT]
#pragma unroll
    for (int j = 0; j < PX; ++j)
#pragma unroll
      for (int c8 = 0; c8 < COUT / 8; ++c8) st[threadIdx.x * CPT + j * (COUT / 8) + c8] = o[j][c8];
    __syncthreads();
    const int lane = threadIdx.x & 63, t0 = threadIdx.x - lane;  // this wave's first thread
    const int idx0 = blockIdx.x * 256 + t0;
    if (idx0 >= nthreads) return;
    const int row0 = idx0 / Q, q0 = idx0 - row0 * Q;
    // consecutive threads own consecutive output pixels (Wo % PX == 0), so the wave's output is one
    // contiguous run of 64 * PX pixels
    _Float16* y0 = a.y + (int64_t(row0) * a.Wo + PX * q0) * COUT;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const int c = k * 64 + lane, tt = c / CPT;
      if (idx0 + tt < nthreads) reinterpret_cast<h8*>(y0)[c] = st[(t0 + tt) * CPT + (c - tt * CPT)];
    }
    return;
  }
  if (!valid) return;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    const int ox = PX * q + j;
    if (ox >= a.Wo) break;
    _Float16* yo = a.y + (int64_t(row) * a.Wo + ox) * a.ycs;
#pragma unroll
    for (int c8 = 0; c8 < COUT / 8; ++c8)
      if (c8 * 8 < a.cout) *reinterpret_cast<h8*>(yo + c8 * 8) = o[j][c8];
  }
}

// 3x3 stride-2 stem on MFMA (3 -> <= 64 channels; k = ci * 9 + tap fits one 32-deep K-step).  A block
// takes SR output rows of one image: the 2 SR + 1 input rows of all channels are staged in LDS as fp16
// (the network's input type; f32 inputs are rounded, u8 inputs become fp16(v / 255) as im.half() / 255
// does) with 16-byte loads and a 16-byte zero pad each side; each wave then builds, per 16-pixel fragment, its B operand by
// gathering the 8 (ci, ky, kx) values of its lane group from LDS and runs RC MFMAs (16 couts each).
// Lane (col, grp) of D holds couts 4 grp .. of pixel col: 8-byte stores, a fragment's 16 pixels x
// RC*16 couts contiguous in NHWC.  fp16 weights, fp32 accumulation, like every other conv here.
template <typename T, int RC, int SR>
__global__ __launch_bounds__(256) void stem_mfma_kernel(StemArgs a, const _Float16* wfr) {
  // SR output rows per block
  constexpr int IR = 2 * SR + 1;        // staged input rows
  extern __shared__ __attribute__((aligned(16))) _Float16 ssm[];  // [C][IR][8 + W + 8]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int rows = (a.Ho + SR - 1) / SR;
  const int n = blockIdx.x / rows, oy0 = (blockIdx.x - n * rows) * SR;
  const int WP = a.W + 16;  // 16-byte zero pads left and right keep every staged chunk aligned
  const int CW = WP / 8;    // 16-byte chunks per staged row
  const T* x = static_cast<const T*>(a.x);
  const int ne = a.C * IR * CW;
  if constexpr (std::is_same<T, _Float16>::value) {
    // fp16 input: up to 12 staging chunks per thread issued back to back (address select onto a zero
    // line, unconditional LDS stores), instead of one dependent load -> store round trip per chunk
    constexpr int NLS = 12;
    if (ne <= NLS * 256) {
      h8 v[NLS];
      int dst[NLS];
      // (staged row, chunk) of e = threadIdx.x + 256 i, stepped without a division per chunk
      const int dq = 256 % CW, dcr = 256 / CW;
      int cr = int(threadIdx.x) / CW, q = int(threadIdx.x) - cr * CW;
#pragma unroll
      for (int i = 0; i < NLS; ++i) {
        const int e = threadIdx.x + 256 * i;
        if (i > 0) {
          q += dq;
          cr += dcr;
          if (q >= CW) {
            q -= CW;
            ++cr;
          }
        }
        const int ci = cr / IR, r = cr - ci * IR;
        const int iy = 2 * oy0 - 1 + r, ix0 = (q - 1) * 8;
        const bool ok = e < ne && iy >= 0 && iy < a.H && q >= 1 && ix0 < a.W;
        dst[i] = e < ne ? cr * WP + q * 8 : a.C * IR * WP;  // one 16-byte dummy slot past the image
        v[i] = *(ok ? reinterpret_cast<const h8*>(x + ((int64_t(n) * a.C + ci) * a.H + iy) * a.W + ix0)
                    : reinterpret_cast<const h8*>(g_zero_line));
      }
#pragma unroll
      for (int i = 0; i < NLS; ++i) *reinterpret_cast<h8*>(ssm + dst[i]) = v[i];
    } else {
      for (int e = threadIdx.x; e < ne; e += 256) {
        const int cr = e / CW, q = e - cr * CW;
        const int ci = cr / IR, r = cr - ci * IR;
        const int iy = 2 * oy0 - 1 + r, ix0 = (q - 1) * 8;
        const bool ok = iy >= 0 && iy < a.H && q >= 1 && ix0 < a.W;
        *reinterpret_cast<h8*>(ssm + cr * WP + q * 8) =
            *(ok ? reinterpret_cast<const h8*>(x + ((int64_t(n) * a.C + ci) * a.H + iy) * a.W + ix0)
                 : reinterpret_cast<const h8*>(g_zero_line));
      }
    }
  } else {
    for (int e = threadIdx.x; e < ne; e += 256) {
      const int cr = e / CW, q = e - cr * CW;
      const int ci = cr / IR, r = cr - ci * IR;
      const int iy = 2 * oy0 - 1 + r, ix0 = (q - 1) * 8;
      h8 v = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (iy >= 0 && iy < a.H && q >= 1 && ix0 < a.W) {
        const T* src = x + ((int64_t(n) * a.C + ci) * a.H + iy) * a.W + ix0;
        RawRun<T, 8> run;
        run.load(src);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (_Float16)run.get(j);
      }
      *reinterpret_cast<h8*>(ssm + cr * WP + q * 8) = v;
    }
  }
  // this lane's 8 k values: (ci, ky, kx) -> LDS offset relative to the pixel's window origin.  k >= cin * 9 (the
  // zero-padded tail of the K-step) reads tap (0, 0, 0) again: its weights are zero and the value finite
  // (that tap is also a real tap of the same output), so the gather needs no per-element select or exec mask
  int koff[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int kq = 8 * grp + j, ci = kq / 9, t = kq - ci * 9;
    koff[j] = kq < a.C * 9 ? (ci * IR + t / 3) * WP + (t % 3) : 0;  // staged col of ix = 2 ox - 1 + kx is 2 ox + 7 + kx
  }
  h8 af[RC];
#pragma unroll
  for (int r = 0; r < RC; ++r) af[r] = reinterpret_cast<const h8*>(wfr)[r * 64 + lane];
  float bz[RC][4];
#pragma unroll
  for (int r = 0; r < RC; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = r * 16 + grp * 4 + j;
      bz[r][j] = bias_or0(a.bias, co, a.cout);
    }
  __syncthreads();
  // the block's outputs: rows oy0 .. oy0 + SR - 1 of image n; 32-bit offsets from the block's first pixel
  _Float16* yb = a.y + (int64_t(n) * a.Ho + oy0) * a.Wo * a.ycs;
  const int fpr = (a.Wo + 15) / 16;  // fragments per output row
#pragma unroll
  for (int rr = 0; rr < SR; ++rr) {
    if (oy0 + rr >= a.Ho) break;
    for (int fx = wave; fx < fpr; fx += 4) {
      const int ox = fx * 16 + col;
      const int base = (2 * rr) * WP + 2 * min(ox, a.Wo - 1) + 7;  // window origin: staged row 2 rr, col 2 ox + 7
      h8 b;
#pragma unroll
      for (int j = 0; j < 8; ++j) b[j] = ssm[base + koff[j]];
      _Float16* yo = yb + (rr * a.Wo + ox) * a.ycs;
#pragma unroll
      for (int r = 0; r < RC; ++r) {
        const f4 d = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[r], b, f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        const int co0 = r * 16 + grp * 4;
        if (ox < a.Wo && co0 < a.cout) {
          h4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float t = d[j] + bz[r][j];
            o[j] = (_Float16)(a.act ? silu(t) : t);
          }
          *reinterpret_cast<h4*>(yo + co0) = o;
        }
      }
    }
  }
}

// Picks among the MFMA stem (3x3 stride 2, cin * 9 <= 32), the stride-2 VALU stem and the general one.
int launch_stem(const fce_conv_desc& d, const fce_tensor& x, const void* w, const float* bias, const fce_tensor* res,
                const fce_tensor& y, int Ho, int Wo, hipStream_t s) {
  FCE_CHECK(x.layout == FCE_NCHW && y.dtype == FCE_F16 && d.up == 0, "stem conv: NCHW input, f16 NHWC output");
  FCE_CHECK(d.epilogue == FCE_EPI_STORE && res == nullptr, "stem conv: plain store only");
  FCE_CHECK(y.cstride % 8 == 0 && y.coff % 8 == 0 && d.cout % 8 == 0, "stem conv: output slice must be 8-aligned");
  StemArgs a{x.data, x.dtype, x.n, x.c, x.h, x.w, d.stride, d.k, Ho, Wo, d.cout, static_cast<const float*>(w),
             bias, static_cast<_Float16*>(y.data) + y.coff, y.cstride, d.act};
  const int64_t P = int64_t(x.n) * Ho * Wo;
  const int blocks = grid_cap((P + 255) / 256);
  int coutT = d.cout <= 16 ? 16 : d.cout <= 32 ? 32 : d.cout <= 64 ? 64 : d.cout <= 96 ? 96 : 0;
  FCE_CHECK(coutT > 0, "stem conv: cout > 96 unsupported");
  const size_t shm = size_t(x.c) * d.k * d.k * coutT * sizeof(float);
  const int PX = coutT <= 32 ? 2 : 1;  // measured: PX 2 beats 4 (occupancy) and 1 (reuse) at cout 16
  const char* sv = getenv("FCE_STEM_VALU");  // diagnostics: the fp32 VALU stem instead of MFMA
  // the staged rows exceed 64 KiB above W = 1168 (imgsz 1280: 70 KiB): gfx950 LDS opt-in up to 160 KiB
  static const int SRE = [] {  // output rows per block (FCE_STEM_SR = 2 / 4 / 8; measured default 4)
    const char* e = getenv("FCE_STEM_SR");
    const int v = e ? atoi(e) : 4;
    return v == 2 || v == 8 ? v : 4;
  }();
  int SR = SRE;
  if (size_t(x.c) * (2 * SR + 1) * (x.w + 16) * 2 + 16 > 160 * 1024) SR = 4;
  if (stem_mfma_ok(d) && d.stride == 2 && x.c == d.cin && d.cout % 16 == 0 && x.w % 8 == 0 &&
      size_t(x.c) * (2 * SR + 1) * (x.w + 16) * 2 + 16 <= 160 * 1024 && !(sv && atoi(sv))) {
    // + the dummy staging slot
    const size_t lds = size_t(x.c) * (2 * SR + 1) * (x.w + 16) * sizeof(_Float16) + 16;
    const int64_t blocks2 = int64_t(x.n) * ((Ho + SR - 1) / SR);
    FCE_CHECK(blocks2 < (int64_t(1) << 31), "stem conv: input too large");
    const _Float16* wfr = reinterpret_cast<const _Float16*>(static_cast<const char*>(w) + stem_fp32_bytes(d));
    const int rc = d.cout / 16;
#define STEMM_SR(T, RC, SRC)                                                                                  \
  do {                                                                                                        \
    static const bool big = hipFuncSetAttribute(reinterpret_cast<const void*>(&stem_mfma_kernel<T, RC, SRC>), \
                                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) ==    \
                            hipSuccess;                                                                       \
    if (!big && lds > 64 * 1024) return fail(FCE_ERR_HIP, "stem conv: cannot opt in to >64 KiB LDS");        \
    FCE_LAUNCH((stem_mfma_kernel<T, RC, SRC>), dim3(unsigned(blocks2)), dim3(256), lds, s, a, wfr);           \
  } while (0)
#define STEMM(T, RC)          \
  do {                        \
    if (SR == 2)              \
      STEMM_SR(T, RC, 2);     \
    else if (SR == 8)         \
      STEMM_SR(T, RC, 8);     \
    else                      \
      STEMM_SR(T, RC, 4);     \
  } while (0)
#define STEMM_T(T)          \
  do {                      \
    if (rc == 1)            \
      STEMM(T, 1);          \
    else if (rc == 2)       \
      STEMM(T, 2);          \
    else if (rc == 3)       \
      STEMM(T, 3);          \
    else                    \
      STEMM(T, 4);          \
  } while (0)
    if (x.dtype == FCE_F16)
      STEMM_T(_Float16);
    else if (x.dtype == FCE_F32)
      STEMM_T(float);
    else
      STEMM_T(uint8_t);
#undef STEMM_T
#undef STEMM
#undef STEMM_SR
    return launch_status("stem_mfma_kernel");
  }
  if (d.k == 3 && d.stride == 2 && x.c == 3 && x.w % (2 * PX) == 0) {
    const int64_t threads = int64_t(x.n) * Ho * ((Wo + PX - 1) / PX);
    FCE_CHECK(threads < (int64_t(1) << 31), "stem conv: input too large");
    const dim3 grid(unsigned((threads + 255) / 256));
#define STEM2_LAUNCH(CT, P, T)                                                                       \
  FCE_LAUNCH((stem_s2_kernel<CT, P, T>), grid, dim3(256), shm + size_t(256) * P * CT * 2, s, a)
#define STEM2_DT(CT, P)                  \
  do {                                   \
    if (x.dtype == FCE_F16)              \
      STEM2_LAUNCH(CT, P, _Float16);     \
    else if (x.dtype == FCE_F32)         \
      STEM2_LAUNCH(CT, P, float);        \
    else                                 \
      STEM2_LAUNCH(CT, P, uint8_t);      \
  } while (0)
    if (coutT == 16)
      STEM2_DT(16, 2);
    else if (coutT == 32)
      STEM2_DT(32, 2);
    else if (coutT == 64)
      STEM2_DT(64, 1);
    else
      STEM2_DT(96, 1);
#undef STEM2_DT
#undef STEM2_LAUNCH
    return launch_status("stem_s2_kernel");
  }
#define STEM_LAUNCH(CT, T) FCE_LAUNCH((stem_kernel<CT, T>), dim3(blocks), dim3(256), shm, s, a)
#define STEM_DT(CT)                      \
  do {                                   \
    if (x.dtype == FCE_F16)              \
      STEM_LAUNCH(CT, _Float16);         \
    else if (x.dtype == FCE_F32)         \
      STEM_LAUNCH(CT, float);            \
    else                                 \
      STEM_LAUNCH(CT, uint8_t);          \
  } while (0)
  if (coutT == 16)
    STEM_DT(16);
  else if (coutT == 32)
    STEM_DT(32);
  else if (coutT == 64)
    STEM_DT(64);
  else
    STEM_DT(96);
#undef STEM_DT
#undef STEM_LAUNCH
  return launch_status("stem_kernel");
}

}  // namespace fce

