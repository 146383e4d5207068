// Non-maximum suppression on the device (reference ultralytics/utils/nms.py:13-166 with the predict
// defaults multi_label=False, agnostic=False, classes=None; TorchNMS.nms :239-296; xywh2xyxy
// utils/ops.py:224-240).  This file: the one-workgroup kernel and the host entry nms() (argument checks, choice
// of path).  nms_common.h: constants, workspace layouts, scans, sorts, box and IoU arithmetic.  nms_greedy.h: the
// greedy suppression shared with the multi-workgroup path (nms_v2.hip, FCE_NMS_V2=1).
//
// nms_best_class_kernel (all CUs; skipped when the forward's Detect cls epilogue already produced the
// per-anchor best-class keys, fce_nms_best) + one 1024-thread workgroup per image:
//   1. candidates: best class per anchor (first maximum), keep conf > conf_thres, compacted in anchor
//      order with a block prefix sum; the class-offset xyxy box (cls * max_wh) and its area are
//      formed here, where the anchor-ordered loads coalesce;
//   2. order by (score desc, anchor asc): stable LDS radix sort (4 x 8-bit digits, ballot-matched
//      ranks) up to 8192 candidates, otherwise a bitonic sort of 64-bit keys in the workspace;
//      truncate to max_nms;
//   3. greedy suppression in sorted order (nms_greedy.h) in the reference's fp32 arithmetic (no FMA contraction
//      in this file), stopping at max_det: tiled when all areas > 0 (no IoU is NaN and the reference's "no overlap
//      -> keep all" early exit changes nothing), else (or max_det > 1024) the literal per-box loop.
#include "common.h"
#include "ops.h"

#pragma clang fp contract(off)

#include "nms_greedy.h"

namespace fce {

// the one-workgroup kernel's frontier step: candidates entering the window are tested against every box kept so
// far, and those past the greedy's stop point are tested for nothing, so a short step wastes fewer tests at the
// price of more extension rounds (FCE_NMS_WIN overrides, a multiple of 64)
static int nms_win() {
  static const int w = [] {
    const int v = getenv("FCE_NMS_WIN") ? atoi(getenv("FCE_NMS_WIN")) : WIN;
    return v >= 64 && v % 64 == 0 ? v : WIN;
  }();
  return w;
}

// ---------------------------------------------------------------- LDS pool of nms_kernel
// One pool, three layouts.  A sort layout is live while its sort runs; afterwards only its `va` region (the sorted
// positions, spos16: sorted rank -> candidate) stays live, beside the greedy layout over the dead key regions.
//   full sort  | keysA 32K | keysB 32K | valsA 16K | valsB 16K | wcnt 16K |
//   head sort  | keysA 8K | keysB 8K | valsA 4K | valsB 4K | wcnt 16K (the select's histograms first) |
//   greedy     | removed 32K | kbox 16K | karea 4K | kidx 4K |  ..  (spos16 of the sort that ran)
struct LdsRegion { int off, bytes; };
struct SortLds { LdsRegion ka, kb, va, vb, wc; };  // keys A / B (uint32), values A / B (uint16), (wave, digit) counts
struct GreedyRegions { LdsRegion removed, kbox, karea, kidx; };
static constexpr int POOL = 112 * 1024;
static constexpr int KiB = 1024;
static constexpr int WCNT_BYTES = NWAVES * 256 * 4;
__host__ __device__ constexpr SortLds sort_lds(bool head) {
  return head ? SortLds{{0, HEAD_CAP * 4}, {8 * KiB, HEAD_CAP * 4}, {16 * KiB, HEAD_CAP * 2}, {20 * KiB, HEAD_CAP * 2},
                        {24 * KiB, WCNT_BYTES}}
              : SortLds{{0, RADIX_CAP * 4}, {32 * KiB, RADIX_CAP * 4}, {64 * KiB, RADIX_CAP * 2},
                        {80 * KiB, RADIX_CAP * 2}, {96 * KiB, WCNT_BYTES}};
}
// `positions`: the sorted positions the greedy can flag in that mode
__host__ __device__ constexpr GreedyRegions greedy_lds(int positions = REMOVED_CAP) {
  return GreedyRegions{{0, positions}, {32 * KiB, KEPT_CAP * 16}, {48 * KiB, KEPT_CAP * 4}, {52 * KiB, KEPT_CAP * 4}};
}
// the radix select's scratch inside the head layout's wcnt: 3 rotating 256-bin histograms, then the
// per-(chunk, wave) counts of the candidates above and at the threshold
static constexpr int SELECT_KPT = RADIX_CAP / NMS_THREADS;
static constexpr int SELECT_BYTES = (3 * 256 + 2 * SELECT_KPT * NWAVES) * 4;

constexpr bool lds_ok(LdsRegion r) { return r.off >= 0 && r.off % 16 == 0 && r.bytes >= 0 && r.off + r.bytes <= POOL; }
constexpr bool lds_disjoint(LdsRegion a, LdsRegion b) { return a.off + a.bytes <= b.off || b.off + b.bytes <= a.off; }
constexpr bool sort_lds_ok(SortLds s) {  // inside the pool, in ascending order without overlap
  return lds_ok(s.ka) && lds_ok(s.kb) && lds_ok(s.va) && lds_ok(s.vb) && lds_ok(s.wc) && s.ka.off + s.ka.bytes <= s.kb.off &&
         s.kb.off + s.kb.bytes <= s.va.off && s.va.off + s.va.bytes <= s.vb.off && s.vb.off + s.vb.bytes <= s.wc.off;
}
// the greedy's regions lie inside the pool, apart from each other and from the sorted positions they must not overwrite
constexpr bool greedy_lds_ok(GreedyRegions g, LdsRegion spos) {
  return lds_ok(g.removed) && lds_ok(g.kbox) && lds_ok(g.karea) && lds_ok(g.kidx) && g.removed.bytes <= g.kbox.off &&
         g.kbox.off + g.kbox.bytes <= g.karea.off && g.karea.off + g.karea.bytes <= g.kidx.off &&
         lds_disjoint(spos, g.removed) && lds_disjoint(spos, g.kbox) && lds_disjoint(spos, g.karea) &&
         lds_disjoint(spos, g.kidx);
}
static_assert(sort_lds_ok(sort_lds(false)) && sort_lds_ok(sort_lds(true)), "a sort region leaves the pool or overlaps");
static_assert(greedy_lds_ok(greedy_lds(REMOVED_CAP), sort_lds(false).va), "full layout: greedy regions / sorted positions");
static_assert(greedy_lds_ok(greedy_lds(HEAD_CAP), sort_lds(true).va), "head layout: greedy regions / sorted positions");
static_assert(SELECT_BYTES <= sort_lds(true).wc.bytes, "the select's histograms and counts leave the wcnt region");
static_assert(sort_lds(false).va.bytes == RADIX_CAP * 2 && sort_lds(true).va.bytes == HEAD_CAP * 2 && RADIX_CAP <= 65536 &&
                  RADIX_CAP == 8 * NMS_THREADS && HEAD_CAP == 2 * NMS_THREADS,
              "uint16 positions for every slot; radix_sort_lds<8> / <2> cover the capacities");

template <typename T>
__device__ __forceinline__ T* lds_at(char* pool, LdsRegion r) { return reinterpret_cast<T*>(pool + r.off); }
// radix_sort_lds over a sort layout: (keysA, valsA) ascending by key, in place
template <int IPL>
__device__ __forceinline__ void sort_in_lds(char* pool, SortLds L, int* wsum) {
  radix_sort_lds<IPL>(lds_at<uint32_t>(pool, L.ka), lds_at<uint32_t>(pool, L.kb), lds_at<uint16_t>(pool, L.va),
                      lds_at<uint16_t>(pool, L.vb), lds_at<int>(pool, L.wc), wsum);
}

static int nms_cap(int A, int nc, int multi) { return multi && nc > 1 ? A * nc : A; }

size_t nms_ws_bytes(int n, int A, int max_nms) { return size_t(n) * nms_ws_per_image(A, A, max_nms); }
size_t nms_ws_bytes_ex(int n, int nc, int A, int max_nms, int multi) {
  return size_t(n) * nms_ws_per_image(A, nms_cap(A, nc, multi), max_nms);
}

// best class per anchor (first maximum, like torch.max): one thread per (image, anchor), all CUs
__global__ __launch_bounds__(256) void nms_best_class_kernel(const float* pred, int nc, int A, int max_nms, char* ws,
                                                             size_t ws_per_image) {
  const int n = blockIdx.y;
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= A) return;
  float best;
  int bj;
  first_max_class(pred + (int64_t(n) * (4 + nc) + 4) * A + a, nc, A, &best, &bj);
  NmsWs w;
  nms_ws_layout(w, ws + size_t(n) * ws_per_image, A, A, max_nms);
  w.aconf[a] = best;
  w.acls[a] = bj;
}

// ---------------------------------------------------------------- phases of nms_kernel
// Each is called by the whole workgroup and ends on a barrier.

// candidate c: anchor, score, class, class-offset box and area into the workspace
__device__ __forceinline__ void put_candidate(const NmsWs& w, int c, int a, float score, int j, const BoxXyhh& b,
                                              float max_wh, int* degenerate) {
  w.cidx[c] = a;
  w.cscore[c] = score;
  w.ccls[c] = j;
  float ar;
  w.cbox[c] = class_box(b, j, max_wh, &ar, degenerate);
  w.carea[c] = ar;
}

// 1m. multi_label candidates (nms.py:116-120): torch.where(cls > conf_thres) in (anchor, class) order, then
// classes=.  LDS: wsum, *total (scan scratch); the pool is untouched.  Returns the candidate count.
__device__ __forceinline__ int collect_multi_label(const float* P, int nc, int A, float conf_thres, float max_wh,
                                                   const NmsClassMask& cm, const NmsWs& w, int* wsum, int* total,
                                                   int* degenerate) {
  int base = 0;
  for (int a0 = 0; a0 < A; a0 += NMS_THREADS) {
    const int a = a0 + threadIdx.x;
    int cnt = 0;
    if (a < A)
      for (int j = 0; j < nc; ++j) cnt += (P[int64_t(4 + j) * A + a] > conf_thres) && cm.allows(j);
    int c = base + block_scan_int(cnt, wsum, total);
    if (cnt) {
      const BoxXyhh b = load_box(P, A, a);
      for (int j = 0; j < nc; ++j) {
        const float v = P[int64_t(4 + j) * A + a];
        if (v > conf_thres && cm.allows(j)) put_candidate(w, c++, a, v, j, b, max_wh, degenerate);
      }
    }
    base += *total;
    __syncthreads();
  }
  return base;
}

// 1b. best-class candidates: groups of CG chunks of 1024 anchors, ONE scan per group (two barriers) over the
// per-(chunk, wave) counts, instead of a block scan (three barriers) per chunk; the candidates' box loads of
// the whole group are issued before any of its workspace writes.  Same positions: anchor order.  bestk: the
// image's Detect-epilogue keys, or null (then w.aconf / w.acls from nms_best_class_kernel).
// LDS: gcnt [CG * NWAVES], *total; the pool is untouched.  Returns the candidate count.
static constexpr int CG = 9;
__device__ __forceinline__ int collect_best_class(const float* P, const unsigned long long* bestk, int A,
                                                  float conf_thres, float max_wh, const NmsClassMask& cm,
                                                  const NmsWs& w, int* gcnt, int* total, int* degenerate) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  int base = 0;
  for (int g0 = 0; g0 < A; g0 += CG * NMS_THREADS) {
    float best[CG];
    int bj[CG];
    uint32_t fl = 0;
#pragma unroll
    for (int c = 0; c < CG; ++c) {
      const int a = g0 + c * NMS_THREADS + int(threadIdx.x);
      best[c] = -INFINITY;
      bj[c] = 0;
      if (a < A) {
        if (bestk) {
          unpack_best_key(bestk[a], &best[c], &bj[c]);
        } else {
          best[c] = w.aconf[a];
          bj[c] = w.acls[a];
        }
      }
      const bool f = a < A && best[c] > conf_thres && cm.allows(bj[c]);
      fl |= uint32_t(f) << c;
      const uint64_t m = __ballot(f);
      if (lane == 0) gcnt[c * NWAVES + wv] = __popcll(m);
    }
    __syncthreads();
    if (wv == 0) {  // exclusive prefix over (chunk, wave) = anchor order, offset by the candidates so far
      const int end = wave_scan_counts<CG * NWAVES>(gcnt, base, lane);
      if (lane == 63) *total = end;
    }
    __syncthreads();
    BoxXyhh b[CG];
#pragma unroll
    for (int c = 0; c < CG; ++c)
      if ((fl >> c) & 1u) b[c] = load_box(P, A, g0 + c * NMS_THREADS + int(threadIdx.x));
#pragma unroll
    for (int c = 0; c < CG; ++c) {
      const bool f = (fl >> c) & 1u;
      const uint64_t m = __ballot(f);
      if (f) put_candidate(w, gcnt[c * NWAVES + wv] + __popcll(m & lt), g0 + c * NMS_THREADS + int(threadIdx.x), best[c],
                           bj[c], b[c], max_wh, degenerate);
    }
    base = *total;
    __syncthreads();  // gcnt / *total are rewritten by the next group
  }
  return base;
}

// 2s. HEAD_CAP < hn <= RADIX_CAP candidates: only the first HEAD_CAP entries of the sorted order (score desc,
// position asc) are sorted.  A radix select (four 8-bit digit passes over the score bits held in registers,
// wave-aggregated LDS atomics, three rotating histograms so each pass has one barrier, every wave finding
// the digit itself) gives the HEAD_CAP-th largest score T and how many of the candidates scoring exactly T
// the prefix takes (`need`: the first ones in position order, as the sort's tie order has it).  One ballot
// scan over (chunk, wave) counts of the candidates above T and at T places the prefix in position order
// and sort_head orders it.  The greedy over the prefix is the full greedy's when max_det is reached
// inside it; otherwise the full sort runs (the retry in the kernel body).
// LDS: writes head ka / va [HEAD_CAP] (the sort's input, left live) and its scratch inside head wc (dead on
// return).
__device__ __forceinline__ void select_prefix(char* pool, const float* cscore, int hn) {
  constexpr int KPT = SELECT_KPT;
  constexpr SortLds L = sort_lds(true);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  int* hist = lds_at<int>(pool, L.wc);  // 3 x 256 bins, rotating over the passes
  int* gsel = hist + 3 * 256;           // [KPT * NWAVES] above T, then [KPT * NWAVES] at T
  uint32_t key[KPT];
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    const int idx = k * NMS_THREADS + int(threadIdx.x);
    key[k] = idx < hn ? __float_as_uint(cscore[idx]) : 0u;  // scores > conf >= 0: valid keys > 0
  }
  if (threadIdx.x < 512) hist[threadIdx.x] = 0;
  __syncthreads();
  uint32_t pre = 0, pmask = 0;
  int need = HEAD_CAP;
#pragma unroll 1
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    int* h = hist + 256 * (pass % 3);
    // the histogram of pass + 1 was last read after the barrier of pass - 2: every wave is past that read
    if (pass > 0 && threadIdx.x < 256) hist[256 * ((pass + 1) % 3) + threadIdx.x] = 0;
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
      // the lanes sharing the first active lane's digit add once (saturated scores put most keys in one
      // bin for the top digits; same-address LDS atomics would serialise)
      const bool in = k * NMS_THREADS + int(threadIdx.x) < hn && (key[k] & pmask) == pre;
      const int d = int(key[k] >> shift) & 255;
      const uint64_t act = __ballot(in);
      if (act) {
        const int first = __builtin_ctzll(act);
        const int d0 = __shfl(d, first);
        const uint64_t same = __ballot(in && d == d0);
        if (lane == first) atomicAdd(&h[d0], __popcll(same));
        if (in && d != d0) atomicAdd(&h[d], 1);
      }
    }
    __syncthreads();
    // every wave: lane l holds digits 4l .. 4l+3; the digit whose bin holds the need-th largest key
    int hv[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hv[i] = h[4 * lane + i];
      s += hv[i];
    }
    int inc = s;  // suffix sum over lanes >= lane
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_down(inc, o);
      if (lane + o < 64) inc += y;
    }
    int above = inc - s, myd = 0, myab = 0;
    bool found = false;
#pragma unroll
    for (int i = 3; i >= 0; --i) {
      if (above < need && need <= above + hv[i]) {
        found = true;
        myd = 4 * lane + i;
        myab = above;
      }
      above += hv[i];
    }
    const int src = __builtin_ctzll(__ballot(found));
    pre |= uint32_t(__shfl(myd, src)) << shift;
    pmask |= 255u << shift;
    need -= __shfl(myab, src);
  }
  // pre = T; the prefix = every candidate above T and the first `need` at T in position order
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    const bool valid = k * NMS_THREADS + int(threadIdx.x) < hn;
    const uint64_t ma = __ballot(valid && key[k] > pre), mt = __ballot(valid && key[k] == pre);
    if (lane == 0) {
      gsel[k * NWAVES + wv] = __popcll(ma);
      gsel[KPT * NWAVES + k * NWAVES + wv] = __popcll(mt);
    }
  }
  __syncthreads();
  if (wv == 0) {  // two exclusive scans in (chunk, wave) = position order
    wave_scan_counts<KPT * NWAVES>(gsel, 0, lane);
    wave_scan_counts<KPT * NWAVES>(gsel + KPT * NWAVES, 0, lane);
  }
  __syncthreads();
  uint32_t* kA = lds_at<uint32_t>(pool, L.ka);
  uint16_t* vA = lds_at<uint16_t>(pool, L.va);
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    const int idx = k * NMS_THREADS + int(threadIdx.x);
    const bool valid = idx < hn, ab = valid && key[k] > pre, at = valid && key[k] == pre;
    const uint64_t ma = __ballot(ab), mt = __ballot(at);
    const int nab = gsel[k * NWAVES + wv] + __popcll(ma & lt);                 // above T before me
    const int nat = gsel[KPT * NWAVES + k * NWAVES + wv] + __popcll(mt & lt);  // at T before me
    if (ab || (at && nat < need)) {
      const int pos = nab + min(nat, need);
      kA[pos] = ~key[k];
      vA[pos] = uint16_t(idx);
    }
  }
  __syncthreads();
}

// sort keys of candidates [0, n) padded to `slots`: ~score bits ascending = score descending (scores > conf
// >= 0, so the bits order like the values), position as the value; the stable sort keeps position order in ties
__device__ __forceinline__ void fill_sort_keys(char* pool, SortLds L, const float* cscore, int n, int slots) {
  uint32_t* kA = lds_at<uint32_t>(pool, L.ka);
  uint16_t* vA = lds_at<uint16_t>(pool, L.va);
  for (int i = threadIdx.x; i < slots; i += NMS_THREADS) {
    kA[i] = i < n ? ~__float_as_uint(cscore[i]) : 0xFFFFFFFFu;
    vA[i] = uint16_t(i);
  }
  __syncthreads();
}

// 2h. the head sort: `slots` (1024 or 2048) keys in head ka / va, filled by select_prefix or fill_sort_keys.
// Small candidate sets (<= HEAD_CAP, the usual case for a trained model) and the selected prefix are sorted
// here instead of in RADIX_CAP slots.
// LDS: writes the head layout and wsum; leaves live: head va = spos16 [slots].
__device__ __forceinline__ void sort_head(char* pool, int slots, int* wsum) {
  if (slots == 1024)
    sort_in_lds<1>(pool, sort_lds(true), wsum);
  else
    sort_in_lds<2>(pool, sort_lds(true), wsum);
  __syncthreads();
}

// 2f. order the full candidate list (score desc, candidate position asc): the LDS radix sort up to RADIX_CAP
// candidates, otherwise a bitonic sort of 64-bit keys in the workspace (w.keys -> w.spos [M]).
// LDS: the radix sort writes the full layout and wsum and leaves live: full va = spos16 [ncand]; the bitonic
// sort touches no LDS.  Returns whether the sorted positions are the ones in LDS.
__device__ __forceinline__ bool sort_full(char* pool, const NmsWs& w, int ncand, int M, int* wsum) {
  const bool lds_sorted = ncand <= RADIX_CAP;
  if (lds_sorted) {
    constexpr SortLds L = sort_lds(false);
    fill_sort_keys(pool, L, w.cscore, ncand, RADIX_CAP);
    sort_in_lds<8>(pool, L, wsum);
  } else {
    const int n2 = next_pow2(ncand);
    for (int i = threadIdx.x; i < n2; i += NMS_THREADS) {
      uint64_t k = 0;
      if (i < ncand) k = (uint64_t(__float_as_uint(w.cscore[i])) << 32) | uint64_t(0xFFFFFFFFu - uint32_t(i));
      w.keys[i] = k;
    }
    __syncthreads();
    bitonic_desc(w.keys, n2);
    for (int i = threadIdx.x; i < M; i += NMS_THREADS)
      w.spos[i] = int(0xFFFFFFFFu - uint32_t(w.keys[i] & 0xFFFFFFFFull));
    __syncthreads();
  }
  __syncthreads();
  return lds_sorted;
}

// the greedy's view of nms_kernel's candidates: sorted position -> candidate through the sort's index array
// (in LDS, or in the workspace after the bitonic sort); the id is the candidate's position
struct CandidateView {
  const uint16_t* spos16;
  bool lds_sorted;
  NmsWs w;
  __device__ __forceinline__ int id(int i) const { return lds_sorted ? int(spos16[i]) : w.spos[i]; }
  __device__ __forceinline__ float4 box(int c) const { return w.cbox[c]; }
  __device__ __forceinline__ float area(int c) const { return w.carea[c]; }
  __device__ __forceinline__ int anchor(int c) const { return w.cidx[c]; }
  __device__ __forceinline__ float score(int c) const { return w.cscore[c]; }
  __device__ __forceinline__ int cls(int c) const { return w.ccls[c]; }
};

// FCE_NMS_STOP (`stop`, diagnostics only, scripts/nms_diag.py): 1 / 2 / 10 end the kernel after the candidates /
// the head sort / the full sort; 3 always takes the full sort; 5, 6, 9, 12: GreedyDiag in nms_greedy.h.
__global__ __launch_bounds__(NMS_THREADS) void nms_kernel(const float* pred, const unsigned long long* bestk, int nc,
                                                          int A, float conf_thres, float iou_thres, int max_det,
                                                          int max_nms, float max_wh, char* ws, size_t ws_per_image,
                                                          float* dets, int64_t* keep, int32_t* counts, int stop,
                                                          int multi, int cap, NmsClassMask cm, int win) {
  __shared__ __attribute__((aligned(16))) char pool[POOL];
  __shared__ int wsum[NWAVES];
  __shared__ int gcnt[CG * NWAVES];
  __shared__ int s_total;
  FCE_GREEDY_TILE(tile);

  const int n = blockIdx.x;
  const float* P = pred + int64_t(n) * (4 + nc) * A;
  NmsWs w;
  nms_ws_layout(w, ws + size_t(n) * ws_per_image, A, cap, max_nms);
  const NmsOut out{P, A, dets + int64_t(n) * max_det * 6, keep + int64_t(n) * max_det};

  // ---- 1. candidates in anchor order (+ their class-offset boxes)
  int degenerate = 0;
  const int ncand =
      multi ? collect_multi_label(P, nc, A, conf_thres, max_wh, cm, w, wsum, &s_total, &degenerate)
            : collect_best_class(P, bestk ? bestk + int64_t(n) * A : nullptr, A, conf_thres, max_wh, cm, w, gcnt,
                                 &s_total, &degenerate);
  degenerate = __syncthreads_or(degenerate);
  if (stop == 1) return;
  const int M = min(ncand, max_nms);
  const bool tiled = !degenerate && max_det <= KEPT_CAP;

  // ---- 2. the head of the order: a small set whole, or the sorted 2048-prefix of a larger one (empty sets take
  // neither; the literal greedy and more than RADIX_CAP candidates go straight to the full sort)
  int hn = 0;
  bool head = false, prefix_only = false;
  if (tiled && stop != 3 && stop != 10) {
    if (ncand > HEAD_CAP && ncand <= RADIX_CAP) {
      select_prefix(pool, w.cscore, ncand);
      hn = HEAD_CAP;
      head = prefix_only = true;
    } else if (ncand > 0 && ncand <= HEAD_CAP) {
      fill_sort_keys(pool, sort_lds(true), w.cscore, ncand, ncand <= 1024 ? 1024 : 2048);
      hn = ncand;
      head = true;
    }
    if (head) sort_head(pool, hn <= 1024 ? 1024 : 2048, wsum);
  }
  if (stop == 2) return;

  for (int attempt = head ? 0 : 1; attempt < 2; ++attempt) {  // the small (or prefix) sort, else the full sort
    const bool H = attempt == 0;
    int Mg = M;  // sorted positions this attempt covers
    bool lds_sorted = true;
    if (H) {
      Mg = min(hn, M);
    } else {
      lds_sorted = sort_full(pool, w, ncand, M, wsum);
      if (stop == 10) return;
    }
    // ---- 3. greedy over the dead sort keys (the sorted positions, spos16, stay live in either layout)
    const CandidateView view{lds_at<const uint16_t>(pool, sort_lds(H).va), lds_sorted, w};
    constexpr GreedyRegions G = greedy_lds();
    const GreedyLds g{lds_at<uint8_t>(pool, G.removed), lds_at<float4>(pool, G.kbox), lds_at<float>(pool, G.karea),
                      lds_at<int>(pool, G.kidx)};
    if (threadIdx.x == 0) tile.kept = 0;
    __syncthreads();
    if (!tiled) {  // degenerate boxes (or max_det > KEPT_CAP): emits as it goes
      const int kept = literal_greedy<NMS_THREADS>(view, out, g.removed, M, iou_thres, max_det);
      if (threadIdx.x == 0) tile.kept = kept;
      break;
    }
    GreedyDiag<true> dg(stop);
    const bool reached = tiled_greedy<NMS_THREADS, true, true>(view, g, tile, Mg, iou_thres, max_det, win, dg);
    __syncthreads();
    // the selected prefix ran out before max_det: its decisions are the full greedy's, but the greedy goes on
    // past it, so start again over the full sort
    if (H && prefix_only && !reached && Mg < M) continue;
    // ---- 4. emit the kept list
    dg.tick(7);
    for (int slot = threadIdx.x; slot < tile.kept; slot += NMS_THREADS) emit_det(view, out, g.kidx[slot], slot);
    __syncthreads();
    dg.tick(7);
    if (stop == 9 && threadIdx.x == 0)  // the segment clocks instead of the first rows
      for (int i = 0; i < 8; ++i) out.dets[i] = float(dg.tm[i]);
    break;
  }
  __syncthreads();
  if (threadIdx.x == 0) counts[n] = tile.kept;
}

int nms(const float* pred, const unsigned long long* best, int n, int nc, int A, float conf, float iou, int max_det,
        int max_nms, float max_wh, void* ws, size_t ws_bytes, float* dets, int64_t* keep, int32_t* counts,
        hipStream_t s, int multi, const int32_t* classes, int nclasses) {
  FCE_CHECK(nc >= 1 && nc <= 65535 && A >= 0 && max_det >= 1 && max_nms >= 1, "nms: bad sizes");
  FCE_CHECK(max_nms <= REMOVED_CAP, "nms: max_nms > 32768 unsupported");
  FCE_CHECK(conf >= 0.f && conf <= 1.f && iou >= 0.f && iou <= 1.f, "nms: thresholds must be in [0, 1]");
  FCE_CHECK(nclasses >= 0 && (nclasses == 0 || classes), "nms: classes list");
  multi = multi && nc > 1;  // nms.py:96 multi_label &= nc > 1
  FCE_CHECK(!multi || int64_t(A) * nc < (int64_t(1) << 30), "nms: multi_label candidate capacity too large");
  NmsClassMask cm{};
  cm.on = classes != nullptr;
  if (classes) {
    FCE_CHECK(nc <= 1024, "nms: classes filter supports nc <= 1024");
    for (int i = 0; i < nclasses; ++i)
      if (classes[i] >= 0 && classes[i] < nc) cm.w[classes[i] >> 5] |= 1u << (classes[i] & 31);
  }
  if (n == 0) return FCE_OK;
  const int cap = nms_cap(A, nc, multi);
  const size_t per = nms_ws_per_image(A, cap, max_nms);
  FCE_CHECK(ws && ws_bytes >= per * n, "nms: workspace too small");
  const int stop = getenv("FCE_NMS_STOP") ? atoi(getenv("FCE_NMS_STOP")) : 0;  // diagnostics (nms_kernel)
  if (multi) best = nullptr;  // candidates come from every class row
  // FCE_NMS_V2=1: the multi-workgroup path (opt-in: measured slower on the bench batch)
  const bool v1 = !(getenv("FCE_NMS_V2") && atoi(getenv("FCE_NMS_V2")) != 0);
  // V2 only where its greedy workgroup's LDS (candidate flags + 24 B per kept box) fits 64 KiB; every other
  // configuration (multi_label, max_det > KEPT_CAP, a large max_det) takes the one-workgroup kernel
  const bool v2_lds = nms2_greedy_lds(A, max_det, max_nms) <= 64 * 1024;
  if (!multi && A > 0 && max_det <= KEPT_CAP && !v1 && stop == 0 && v2_lds)
    return nms2(pred, best, n, nc, A, conf, iou, max_det, max_nms, max_wh, static_cast<char*>(ws), per, dets, keep,
                counts, s, cm);
  if (A > 0 && !best && !multi)  // else the keys came from the Detect cls epilogue (fce_nms_best)
    FCE_LAUNCH(nms_best_class_kernel, dim3((A + 255) / 256, n), dim3(256), 0, s, pred, nc, A, max_nms,
                       static_cast<char*>(ws), per);
  FCE_LAUNCH(nms_kernel, dim3(n), dim3(NMS_THREADS), 0, s, pred, best, nc, A, conf, iou, max_det, max_nms, max_wh,
                     static_cast<char*>(ws), per, dets, keep, counts, stop, multi, cap, cm, nms_win());
  return launch_status("nms_kernel");
}

}  // namespace fce
