// Shared pieces of the device NMS (nms.hip: the one-workgroup kernel; nms_v2.hip: the multi-workgroup path):
// constants, the classes= mask, both workspace layouts, scans and sorts, the reference's box and IoU arithmetic,
// the per-anchor arg-max and the best-class key.
// The box and IoU arithmetic reproduces the reference's fp32 operation order, and a contracted FMA flips
// near-threshold decisions: this header relies on the including unit for `#pragma clang fp contract(off)`,
// placed before the #include.
#pragma once
#include "common.h"

namespace fce {

static constexpr int NMS_THREADS = 1024;  // the one-workgroup kernel
static constexpr int NWAVES = NMS_THREADS / 64;
static constexpr int RADIX_CAP = 8192;  // LDS radix sort capacity (16 waves x 512)
static constexpr int HEAD_CAP = 2048;   // small-set / sorted-prefix sort capacity
static constexpr int REMOVED_CAP = 32768;
static constexpr int KEPT_CAP = 1024;  // kept boxes held in LDS by the tiled greedy
static constexpr int TILE = 64;
static constexpr int WIN = 256;  // frontier extension step (the multi-workgroup path; FCE_NMS_WIN's default)
static constexpr int NMS2_CH = 2048;  // anchors per sort chunk of the multi-workgroup path

// classes= filter (nms.py:128-132) as a bit mask over class ids < 1024; on == 0: every class
struct NmsClassMask {
  uint32_t w[32];
  int on;
  __device__ __forceinline__ bool allows(int j) const { return !on || (j < 1024 && ((w[j >> 5] >> (j & 31)) & 1u)); }
};

__host__ __device__ inline int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

// ---------------------------------------------------------------- workspace layouts: one function per path fills
// the pointer struct from an image's base pointer and returns the bytes used; a null base is the host's size query
struct WsCarver {
  char* base;
  size_t off;
  template <typename T>
  __host__ __device__ T* take(size_t count, bool align16 = true) {
    T* p = reinterpret_cast<T*>(base + off);  // null base (the size query): never dereferenced
    const size_t b = count * sizeof(T);
    off += align16 ? (b + 15) & ~size_t(15) : b;
    return p;
  }
};

// Candidate capacity C: A (best class per anchor), or A * nc with multi_label (one candidate per
// (anchor, class) above conf_thres).
struct NmsWs {
  float* aconf;    // per-anchor best score    [A]   (nms_best_class_kernel)
  int* acls;       // per-anchor best class    [A]
  int* cidx;       // candidate anchor index   [C]
  float* cscore;   // candidate score          [C]
  int* ccls;       // candidate class          [C]
  float* carea;    // candidate area           [C]
  float4* cbox;    // candidate class-offset xyxy [C]
  uint64_t* keys;  // global sort keys         [P2 = next_pow2(C)]  (> RADIX_CAP candidates)
  int* spos;       // sorted -> candidate pos  [M = min(C, max_nms)]   (> RADIX_CAP candidates)
};

__host__ __device__ inline size_t nms_ws_layout(NmsWs& w, char* base, int A, int C, int max_nms) {
  WsCarver c{base, 0};
  w.aconf = c.take<float>(A);
  w.acls = c.take<int>(A);
  w.cidx = c.take<int>(C);
  w.cscore = c.take<float>(C);
  w.ccls = c.take<int>(C);
  w.carea = c.take<float>(C);
  w.cbox = c.take<float4>(C);
  w.keys = c.take<uint64_t>(next_pow2(C > 1 ? C : 1), false);
  w.spos = c.take<int>(C < max_nms ? C : max_nms);
  return c.off;
}

struct Nms2Ws {
  uint64_t* keys;  // [A2] per anchor, then sorted within each chunk (descending)
  int* acls;       // [A] best class per anchor
  int* ccount;     // [NCH] candidates per chunk
  int* flags;      // [4]: [0] = a degenerate box among the first M sorted candidates
  float4* sbox;    // [Mc = min(A, max_nms)] rank-ordered class-offset xyxy boxes
  float* sarea;    // [Mc]
  int* sanc;       // [Mc] anchor
  float* sscore;   // [Mc]
  int* scls;       // [Mc]
};

__host__ __device__ inline int nms2_a2(int A) { return (A + NMS2_CH - 1) / NMS2_CH * NMS2_CH; }

__host__ __device__ inline size_t nms2_ws_layout(Nms2Ws& w, char* base, int A, int Mc) {
  WsCarver c{base, 0};
  w.keys = c.take<uint64_t>(nms2_a2(A), false);
  w.acls = c.take<int>(A);
  w.ccount = c.take<int>(nms2_a2(A) / NMS2_CH);
  w.flags = c.take<int>(4);
  w.sbox = c.take<float4>(Mc);
  w.sarea = c.take<float>(Mc);
  w.sanc = c.take<int>(Mc);
  w.sscore = c.take<float>(Mc);
  w.scls = c.take<int>(Mc);
  return c.off;
}

// per-image workspace stride: either path fits (chosen per call)
inline size_t nms_ws_per_image(int A, int C, int max_nms) {
  NmsWs w1;
  Nms2Ws w2;
  const size_t v1 = nms_ws_layout(w1, nullptr, A, C, max_nms);
  const size_t v2 = nms2_ws_layout(w2, nullptr, A, A < max_nms ? A : max_nms);
  return ((v1 > v2 ? v1 : v2) + 255) & ~size_t(255);
}

// the multi-workgroup path (nms_v2.hip; `per` = nms_ws_per_image) and its greedy workgroup's LDS: candidate flags
// + 24 B per kept box
int nms2(const float* pred, const unsigned long long* best, int n, int nc, int A, float conf, float iou, int max_det,
         int max_nms, float max_wh, char* ws, size_t per, float* dets, int64_t* keep, int32_t* counts, hipStream_t s,
         const NmsClassMask& cm);
inline size_t nms2_greedy_lds(int A, int max_det, int max_nms) {
  return size_t(((A < max_nms ? A : max_nms) + 15) & ~15) + size_t(max_det) * 24;
}

// ---------------------------------------------------------------- scans and sorts
// inclusive sum over the lanes of a wave
__device__ __forceinline__ int wave_scan_incl(int x, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  return x;
}

// block-wide exclusive scan of non-negative counts (1024 threads = 16 waves)
__device__ inline int block_scan_int(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x = wave_scan_incl(v, lane);
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int i = 0; i < NWAVES; ++i) {
      const int t = wsum[i];
      wsum[i] = acc;
      acc += t;
    }
    *total = acc;
  }
  __syncthreads();
  return wsum[wv] + x - v;
}

// One wave: g[0..N) (per-(chunk, wave) counts, in position order) becomes its exclusive prefix sum offset by
// `base`; returns base + the total (valid in lane 63).
template <int N>
__device__ __forceinline__ int wave_scan_counts(int* g, int base, int lane) {
  constexpr int PER = (N + 63) / 64;
  int v[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int idx = lane * PER + k;
    v[k] = idx < N ? g[idx] : 0;
    sum += v[k];
  }
  const int inc = wave_scan_incl(sum, lane);
  int ex = base + inc - sum;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int idx = lane * PER + k;
    if (idx < N) g[idx] = ex;
    ex += v[k];
  }
  return base + inc;
}

__device__ inline void bitonic_desc(uint64_t* k, int n2) {
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < n2 / 2; i += blockDim.x) {
        const int lo = 2 * i - (i & (stride - 1));
        const int hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const uint64_t a = k[lo], b = k[hi];
        if ((a < b) == desc) {
          k[lo] = b;
          k[hi] = a;
        }
      }
      __syncthreads();
    }
  }
}

// Stable LSD radix sort of 1024 * IPL (key, index) pairs by ascending key, in LDS.  Wave w owns
// positions [64 IPL w, 64 IPL (w+1)) in lane-striped order (item j of lane l = 64 IPL w + 64j + l), so the
// ballot-matched running rank of a digit inside the wave is its stable rank; per-(digit, wave)
// counts are then scanned digit-major for the global offsets.
template <int IPL>
__device__ void radix_sort_lds(uint32_t* kA, uint32_t* kB, uint16_t* vA, uint16_t* vB, int* wcnt, int* wsum) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  uint32_t* ks = kA;
  uint32_t* kd = kB;
  uint16_t* vs = vA;
  uint16_t* vd = vB;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    for (int e = threadIdx.x; e < NWAVES * 256; e += NMS_THREADS) wcnt[e] = 0;
    __syncthreads();
    uint32_t k[IPL];
    uint16_t v[IPL];
    int d[IPL], rank[IPL];
#pragma unroll
    for (int j = 0; j < IPL; ++j) {
      const int idx = 64 * IPL * wv + 64 * j + lane;
      k[j] = ks[idx];
      v[j] = vs[idx];
      d[j] = int((k[j] >> shift) & 255u);
    }
    int* wc = wcnt + wv * 256;
#pragma unroll
    for (int j = 0; j < IPL; ++j) {
      uint64_t peer = ~0ull;
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const bool bit = (d[j] >> b) & 1;
        const uint64_t bal = __ballot(bit);
        peer &= bit ? bal : ~bal;
      }
      const int pre = __popcll(peer & lt);
      const int base = wc[d[j]];
      rank[j] = base + pre;
      __builtin_amdgcn_wave_barrier();
      if (pre == 0) wc[d[j]] = base + __popcll(peer);
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // block-wide exclusive scan over e = digit * 16 + wave, four entries per thread
    int c[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = threadIdx.x * 4 + i;
      c[i] = wcnt[(e & 15) * 256 + (e >> 4)];
      s += c[i];
    }
    const int inc = wave_scan_incl(s, lane);
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int excl = inc - s;
    for (int i = 0; i < wv; ++i) excl += wsum[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = threadIdx.x * 4 + i;
      wcnt[(e & 15) * 256 + (e >> 4)] = excl;
      excl += c[i];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < IPL; ++j) {
      const int pos = wc[d[j]] + rank[j];
      kd[pos] = k[j];
      vd[pos] = v[j];
    }
    __syncthreads();
    uint32_t* tk = ks;
    ks = kd;
    kd = tk;
    uint16_t* tv = vs;
    vs = vd;
    vd = tv;
  }
  // 4 passes: the result is back in (kA, vA)
}

// ---------------------------------------------------------------- boxes and IoU
// an anchor's box as the reference forms it (xywh2xyxy, ops.py:224-240): centre and half extents
struct BoxXyhh {
  float cx, cy, hw, hh;
};
__device__ __forceinline__ BoxXyhh load_box(const float* P, int A, int a) {  // P: the image's (4 + nc, A) rows
  return BoxXyhh{P[a], P[int64_t(1) * A + a], P[int64_t(2) * A + a] / 2.0f, P[int64_t(3) * A + a] / 2.0f};
}

// the class-offset xyxy box (cls * max_wh, nms.py:141) the greedy works on, its area, and whether it is
// degenerate (area <= 0, NaN or inf: the tiled greedy is exact only without such boxes)
__device__ __forceinline__ float4 class_box(const BoxXyhh& b, int cls, float max_wh, float* area, int* degenerate) {
  const float off = (float)cls * max_wh;
  const float bx1 = (b.cx - b.hw) + off, by1 = (b.cy - b.hh) + off, bx2 = (b.cx + b.hw) + off, by2 = (b.cy + b.hh) + off;
  const float ar = (bx2 - bx1) * (by2 - by1);
  *area = ar;
  *degenerate |= !(ar > 0.0f) || !isfinite(ar);
  return make_float4(bx1, by1, bx2, by2);
}

// reference IoU (nms.py:276-291) in fp32, same operation order
__device__ __forceinline__ float iou_ref(float4 bi, float ai, float4 bj, float aj, float* inter_out) {
  const float ww = fmaxf(fminf(bi.z, bj.z) - fmaxf(bi.x, bj.x), 0.0f);
  const float hh = fmaxf(fminf(bi.w, bj.w) - fmaxf(bi.y, bj.y), 0.0f);
  const float inter = ww * hh;
  *inter_out = inter;
  return inter / ((ai + aj) - inter);
}

// min / max of finite floats without the NaN-quieting canonicalisation fminf / fmaxf get in IEEE mode (two
// extra v_max per operand, re-done every iteration even for loop-invariant boxes): the same value for every
// finite input, and every box here is finite (degenerate boxes take the literal path)
__device__ __forceinline__ float vmin_(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float vmax_(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// iou_ref(...) > thr for positive areas: a zero intersection gives IoU 0 (thr >= 0), skip the division.  The IEEE
// division (~10 VALU ops) runs only when inter is within 2^-20 of thr * union: p = RN(thr * union) is within 2^-24 of
// the real product, so inter > p (1 + 2^-20) puts the real quotient above thr by far more than the half ulp RN(q)
// could lose (RN(q) > thr, as the reference computes it), and inter < p (1 - 2^-20) puts it below thr.  Exact.
__device__ __forceinline__ bool suppresses(float4 bi, float ai, float4 bj, float aj, float thr) {
  const float ww = vmax_(vmin_(bi.z, bj.z) - vmax_(bi.x, bj.x), 0.0f);
  const float hh = vmax_(vmin_(bi.w, bj.w) - vmax_(bi.y, bj.y), 0.0f);
  const float inter = ww * hh;
  const float uni = (ai + aj) - inter;
  const float p = thr * uni;
  const bool hi = inter > p * 1.00000095367431640625f;  // 1 + 2^-20
  const bool lo = inter < p * 0.99999904632568359375f;  // 1 - 2^-20 (inter == 0 < p: lo, when thr > 0)
  bool r = hi;
  if (!(hi || lo)) r = inter / uni > thr;  // within 2^-20 of thr * union: the reference's quotient
  return r;
}

// ---------------------------------------------------------------- best class per anchor
// first maximum over the nc class rows of anchor column p (torch.max, nms.py:101), 8 loads in flight
__device__ __forceinline__ void first_max_class(const float* p, int nc, int A, float* best_out, int* cls_out) {
  float best = -INFINITY;
  int bj = 0;
  int c = 0;
  for (; c + 8 <= nc; c += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[int64_t(c + j) * A];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (v[j] > best) {
        best = v[j];
        bj = c + j;
      }
  }
  for (; c < nc; ++c) {
    const float v = p[int64_t(c) * A];
    if (v > best) {
      best = v;
      bj = c;
    }
  }
  *best_out = best;
  *cls_out = bj;
}

// the Detect cls epilogue's per-anchor key: score bits << 32 | ~class
__device__ __forceinline__ void unpack_best_key(unsigned long long k, float* best, int* cls) {
  *best = __uint_as_float(uint32_t(k >> 32));
  *cls = int(0xFFFFFFFFu - uint32_t(k));
}

}  // namespace fce
