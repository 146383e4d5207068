// The greedy suppression of the device NMS, written once and instantiated by nms_kernel (nms.hip, 1024 threads,
// sorted position -> candidate through the sort's index array) and nms2_greedy_kernel (nms_v2.hip, 256 threads,
// rank-ordered arrays).  A "sorted view" V maps a sorted position i (score desc, position asc) to a box:
//   int V::id(i)                                  what the kept list and the emission hold for position i
//   float4 V::box(id), float V::area(id)          the class-offset xyxy box and its area
//   int V::anchor(id), float V::score(id), int V::cls(id)    the output row
// Everything here is __forceinline__, so a view is resolved at compile time.
//
// The IoU arithmetic reproduces the reference's fp32 operation order: this header relies on the including unit
// for `#pragma clang fp contract(off)`, placed before the #include.
#pragma once
#include "nms_common.h"

namespace fce {

// where an image's rows go
struct NmsOut {
  const float* P;  // the image's (4 + nc, A) prediction rows
  int A;
  float* dets;    // the image's [max_det][6]
  int64_t* keep;  // the image's [max_det]
};

template <class V>
__device__ __forceinline__ void emit_det(const V& v, const NmsOut& o, int id, int slot) {
  const int a = v.anchor(id);
  const BoxXyhh b = load_box(o.P, o.A, a);
  float* d = o.dets + int64_t(slot) * 6;
  d[0] = b.cx - b.hw;
  d[1] = b.cy - b.hh;
  d[2] = b.cx + b.hw;
  d[3] = b.cy + b.hh;
  d[4] = v.score(id);
  d[5] = (float)v.cls(id);
  o.keep[slot] = a;
}

// The greedy's LDS arrays (carved by the kernel from its pool): one flag per sorted position, and the kept
// list the tiled greedy tests later candidates against.
struct GreedyLds {
  uint8_t* removed;  // [positions covered]
  float4* kbox;      // [max_det] kept boxes
  float* karea;      // [max_det]
  int* kidx;         // [max_det] kept slot -> view id
};

// The tiled greedy's tile and its workgroup-wide scalars; each kernel declares one with FCE_GREEDY_TILE.  The boxes
// are plain floats so the type is 8-aligned without tail padding (a float4 member would round it up by 8 bytes of
// LDS); the macro aligns the variable itself to 16 and the boxes come first, so box() is an aligned 16-byte access.
struct GreedyTile {
  float boxes[TILE][4];
  uint64_t colmask[TILE];  // colmask[u] = {t < u in the tile : IoU(t, u) > thr}
  int idx[TILE];           // sorted positions of the tile's candidates
  float area[TILE];
  int n, need, next, nk, done, kept;
  __device__ __forceinline__ float4& box(int i) { return reinterpret_cast<float4*>(boxes)[i]; }
};
#define FCE_GREEDY_TILE(name) __shared__ __attribute__((aligned(16))) GreedyTile name

// Diagnostics of the one-workgroup kernel (FCE_NMS_STOP, scripts/nms_diag.py): 5 skips the window tests, 6 the
// column masks, 12 fixes the frontier step, 9 clocks the segments [select, colmask, resolve, window test,
// tiles, extensions, extension tests, emit] with s_memtime.  With !ON stop stays 0 and everything folds away.
template <bool ON>
struct GreedyDiag {
  int stop = 0;
  uint64_t tm[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
  __device__ __forceinline__ explicit GreedyDiag(int stop_ = 0) {
    if (ON) stop = stop_;
    if (ON && stop == 9) tprev = __builtin_amdgcn_s_memtime();
  }
  __device__ __forceinline__ void tick(int slot) {
    if (ON && stop == 9) {
      const uint64_t t = __builtin_amdgcn_s_memtime();
      tm[slot] += t - tprev;
      tprev = t;
    }
  }
  __device__ __forceinline__ void count(int slot) { tm[slot] += ON; }
};

// Literal per-box greedy (TorchNMS.nms with its early exit, nms.py:276-296) over sorted positions [0, M): the
// path for degenerate boxes, whose IoU can be NaN.  Emits as it keeps; returns the kept count (every thread).
template <int THREADS, class V>
__device__ __forceinline__ int literal_greedy(const V& v, const NmsOut& o, uint8_t* removed, int M, float iou_thres,
                                              int max_det) {
  for (int i = threadIdx.x; i < M; i += THREADS) removed[i] = 0;
  __syncthreads();
  int kept = 0;
  for (int i = 0; i < M && kept < max_det; ++i) {
    if (removed[i]) continue;
    const int ci = v.id(i);
    if (threadIdx.x == 0) emit_det(v, o, ci, kept);
    ++kept;
    if (kept >= max_det) break;
    const float4 bi = v.box(ci);
    const float ai = v.area(ci);
    int any = 0;
    for (int j = i + 1 + threadIdx.x; j < M; j += THREADS) {
      if (removed[j]) continue;
      const int cj = v.id(j);
      float inter;
      iou_ref(bi, ai, v.box(cj), v.area(cj), &inter);
      any |= inter != 0.0f;
    }
    any = __syncthreads_or(any);
    if (any) {
      for (int j = i + 1 + threadIdx.x; j < M; j += THREADS) {
        if (removed[j]) continue;
        const int cj = v.id(j);
        float inter;
        const float iou = iou_ref(bi, ai, v.box(cj), v.area(cj), &inter);
        if (!(iou <= iou_thres)) removed[j] = 1;
      }
    }
    __syncthreads();
  }
  return kept;
}

// Candidates [jlo, jhi) (sorted positions, not yet removed) against kept boxes [klo, khi): all THREADS
// threads, thread = (candidate, split of the kept list).  Each wave holds 64 consecutive candidates
// and one split, so every lane of a wave reads the same kept boxes (LDS broadcast), 4 per batch of
// loads; a suppressed candidate's flag is set by whichever split finds it (all writers store 1).
template <int THREADS, class V>
__device__ __forceinline__ void test_range(const V& v, const GreedyLds& g, int jlo, int jhi, int klo, int khi,
                                           float iou_thres) {
  const int nj = jhi - jlo, nk = khi - klo;
  if (nj <= 0 || nk <= 0) return;
  const int rj = (nj + 63) & ~63;
  const int S = max(1, min(nk, THREADS / rj));
  for (int idx = threadIdx.x; idx < rj * S; idx += THREADS) {
    const int j = jlo + idx % rj, sp0 = idx / rj;
    if (j >= jhi || g.removed[j]) continue;
    const int c = v.id(j);
    const float4 bj = v.box(c);
    const float aj = v.area(c);
    bool rem = false;
    int k = klo + sp0;
    for (; k + 3 * S < khi && !rem; k += 4 * S) {
      float4 kb[4];
      float ka[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        kb[u] = g.kbox[k + u * S];
        ka[u] = g.karea[k + u * S];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) rem |= suppresses(kb[u], ka[u], bj, aj, iou_thres);
    }
    for (; k < khi && !rem; k += S) rem = suppresses(g.kbox[k], g.karea[k], bj, aj, iou_thres);
    if (rem) g.removed[j] = 1;
  }
}

// Tiled greedy with a lazy frontier over sorted positions [0, M) (exact when every area > 0), by tiles of the
// next 64 surviving candidates: the tile's 64 x 64 suppression bit matrix is built by every wave (one ballot
// per row) and resolved in greedy order with 64-bit mask operations; later candidates are tested lazily, only
// those inside the frontier window [tile end, F) against each tile's kept boxes, and a candidate entering the
// window once against every box kept so far.  The frontier grows by `win` positions; with ADAPTIVE the step
// shrinks near max_det.  Fills g.kbox / karea / kidx [0, t.kept) and leaves the kept count in t.kept (set it
// to 0 before the call); returns whether max_det was reached.  Every return follows a barrier with no LDS
// write after it, so the kept list is visible to the whole workgroup.
template <int THREADS, bool ADAPTIVE, bool DIAG, class V>
__device__ __forceinline__ bool tiled_greedy(const V& v, const GreedyLds& g, GreedyTile& t, int M, float iou_thres,
                                             int max_det, int win, GreedyDiag<DIAG>& dg) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int cursor = 0, F = 0;
  while (true) {
    // select the next <= 64 surviving candidates in [cursor, F), extending F while short
    while (true) {
      if (wv == 0) {
        int cnt = 0;
        for (int c = cursor; cnt < TILE && c < F; c += 64) {
          const int j = c + lane;
          const bool alive = j < F && !g.removed[j];
          const uint64_t bb = __ballot(alive);
          const int take = min(__popcll(bb), TILE - cnt);
          const int rank = __popcll(bb & ((1ull << lane) - 1ull));
          if (alive && rank < take) t.idx[cnt + rank] = j;
          cnt += take;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's t.idx writes have landed
        __builtin_amdgcn_wave_barrier();
        const bool need = cnt < TILE && F < M;
        if (!need && lane < cnt) {
          const int c = v.id(t.idx[lane]);
          t.box(lane) = v.box(c);
          t.area[lane] = v.area(c);
        }
        if (lane == 0) {
          t.n = cnt;
          t.need = need;
          t.next = cnt == TILE ? t.idx[TILE - 1] + 1 : M;
        }
      }
      __syncthreads();
      dg.tick(0);
      if (!t.need) break;
      // candidates entering the window: tested once against every box kept so far.  ADAPTIVE: near max_det the
      // step shrinks to what the survival rate so far (t.kept kept of F) says is still needed, +25 %, in multiples
      // of 64: candidates past the greedy's stop are tested for nothing (any schedule gives the same result)
      int step = win;
      if (ADAPTIVE && t.kept > 0 && dg.stop != 12) {
        const int64_t est = int64_t(max_det - t.kept) * F / t.kept;
        step = min(win, max(64, int(((est * 5) / 4 + 63) & ~int64_t(63))));
      }
      const int Fn = min(M, F + step);
      for (int j = F + threadIdx.x; j < Fn; j += THREADS) g.removed[j] = 0;
      __syncthreads();
      if (dg.stop != 5) test_range<THREADS>(v, g, F, Fn, 0, t.kept, iou_thres);
      F = Fn;
      __syncthreads();
      dg.count(5);
      dg.tick(6);
    }
    dg.count(4);
    const int cnt = t.n;
    if (cnt == 0) return false;
    // column masks of the tile's suppression relation: wave w owns columns u = w, w + THREADS / 64, ..; lane = row
    for (int u = wv; u < TILE && dg.stop != 6; u += THREADS / 64) {
      bool sup = false;
      if (lane < u && u < cnt) sup = suppresses(t.box(lane), t.area[lane], t.box(u), t.area[u], iou_thres);
      const uint64_t bb = __ballot(sup);
      if (lane == 0) t.colmask[u] = bb;
    }
    __syncthreads();
    dg.tick(1);
    if (wv == 0) {
      // greedy over the tile as a fixpoint (lane u = tile candidate u): u is kept once none of its
      // suppressors is kept or undecided, removed once one of them is kept.  Every round decides at
      // least the lowest undecided candidate, and each decision is the sequential greedy's.
      const int kept0 = t.kept;
      const uint64_t C = lane < cnt ? t.colmask[lane] : 0ull;
      uint64_t undecided = cnt == 64 ? ~0ull : ((1ull << cnt) - 1ull), kept = 0;
      while (undecided) {
        const bool me = (undecided >> lane) & 1ull;
        const uint64_t k = __ballot(me && (C & (kept | undecided)) == 0ull);
        const uint64_t r = __ballot(me && (C & kept) != 0ull);
        kept |= k;
        undecided &= ~(k | r);
      }
      // max_det: the greedy stops at the (max_det - kept0)-th kept candidate of the tile
      int nk = __popcll(kept);
      bool done = false;
      if (kept0 + nk >= max_det) {
        const int allow = max_det - kept0;
        uint64_t m = kept;
        for (int i = 0; i < allow - 1; ++i) m &= m - 1ull;  // drop the lowest allow-1 bits
        const uint64_t last = m & (~m + 1ull);               // the allow-th kept candidate
        kept &= (last << 1) - 1ull;
        nk = allow;
        done = true;
      }
      if ((kept >> lane) & 1ull) {
        const int r = __popcll(kept & ((1ull << lane) - 1ull));
        g.kbox[kept0 + r] = t.box(lane);
        g.karea[kept0 + r] = t.area[lane];
        g.kidx[kept0 + r] = v.id(t.idx[lane]);
      }
      if (lane == 0) {
        t.nk = nk;
        t.kept = kept0 + nk;
        t.done = done ? 2 : (t.next >= M ? 1 : 0);
      }
    }
    __syncthreads();
    dg.tick(2);
    if (t.done) return t.done == 2;
    // the rest of the window against the tile's kept boxes
    const int start = t.next;
    if (dg.stop != 5) test_range<THREADS>(v, g, start, F, t.kept - t.nk, t.kept, iou_thres);
    cursor = start;
    __syncthreads();
    dg.tick(3);
  }
}

}  // namespace fce
