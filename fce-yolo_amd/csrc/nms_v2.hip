// Multi-workgroup NMS (opt-in: FCE_NMS_V2=1; nms() in nms.hip chooses the path).
// The one-workgroup kernel (nms.hip) needs a whole CU per image (1024 threads, 112 KB of LDS), so beside the forward
// of other batches it waits for CUs to drain, and its candidate and sort phases are serial over one workgroup.
// Here the same computation is four launches:
//   K1 nms2_keys_kernel   (all CUs, one thread per anchor): best class (the Detect epilogue's key, or the
//                          arg-max over the class rows) and the sort key score bits << 32 | ~anchor (0 for
//                          a non-candidate).  Descending keys = (score desc, anchor asc) = the reference's
//                          order of candidates (they are formed in anchor order, nms.py:101-105, 150-153);
//   K2 nms2_sort_kernel   (one 256-thread workgroup per 2048-anchor chunk): bitonic sort of the chunk's
//                          keys in 16 KB of LDS, candidate count per chunk;
//   K3 nms2_rank_kernel   (one workgroup per chunk): a candidate's global rank = its rank in its chunk +
//                          the number of larger keys in every other chunk (binary searches); ranks <
//                          max_nms scatter the class-offset box, area, anchor, score and class into
//                          rank-ordered arrays (the truncation of nms.py:155-156), and flag degenerate boxes;
//   K4 nms2_greedy_kernel (one 256-thread workgroup per image, LDS = max_nms bytes + max_det kept boxes): the
//                          greedy of nms_greedy.h over the rank-ordered arrays (coalesced), tiled or literal.
// Same fp32 arithmetic (no FMA contraction in this file), same order, same greedy: bitwise nms_kernel's results.
#include "common.h"
#include "ops.h"

#pragma clang fp contract(off)

#include "nms_greedy.h"

namespace fce {

static constexpr int NMS2_SORT_THREADS = 256;
static constexpr int NMS2_G_THREADS = 256;

__global__ __launch_bounds__(256) void nms2_keys_kernel(const float* pred, const unsigned long long* bestk, int nc, int A,
                                                        int Mc, float conf_thres, char* ws, size_t per,
                                                        NmsClassMask cm) {
  const int n = blockIdx.y;
  const int a = blockIdx.x * 256 + threadIdx.x;
  Nms2Ws w;
  nms2_ws_layout(w, ws + size_t(n) * per, A, Mc);
  uint64_t key = 0;
  if (a < A) {
    float best;
    int bj;
    if (bestk)  // fused into the Detect cls epilogue
      unpack_best_key(bestk[int64_t(n) * A + a], &best, &bj);
    else
      first_max_class(pred + (int64_t(n) * (4 + nc) + 4) * A + a, nc, A, &best, &bj);
    if (best > conf_thres && cm.allows(bj))  // a positive score: its bits order like the value
      key = (uint64_t(__float_as_uint(best)) << 32) | uint64_t(0xFFFFFFFFu - uint32_t(a));
    w.acls[a] = bj;
  }
  if (a < nms2_a2(A)) w.keys[a] = key;
}

__global__ __launch_bounds__(NMS2_SORT_THREADS) void nms2_sort_kernel(int A, int Mc, char* ws, size_t per) {
  __shared__ uint64_t sk[NMS2_CH];
  __shared__ int scount;
  const int n = blockIdx.y, chunk = blockIdx.x;
  Nms2Ws w;
  nms2_ws_layout(w, ws + size_t(n) * per, A, Mc);
  uint64_t* g = w.keys + size_t(chunk) * NMS2_CH;
  if (threadIdx.x == 0) scount = 0;
  __syncthreads();
  int cnt = 0;
  for (int i = threadIdx.x; i < NMS2_CH; i += NMS2_SORT_THREADS) {
    const uint64_t k = g[i];
    sk[i] = k;
    cnt += k != 0;
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0) atomicAdd(&scount, cnt);
  __syncthreads();
  if (scount > 0) bitonic_desc(sk, NMS2_CH);  // ends with __syncthreads
  for (int i = threadIdx.x; i < NMS2_CH; i += NMS2_SORT_THREADS) g[i] = sk[i];
  if (threadIdx.x == 0) {
    w.ccount[chunk] = scount;
    if (chunk == 0) w.flags[0] = 0;
  }
}

// number of keys > k in a descending run of `cnt` distinct keys
__device__ __forceinline__ int count_greater(const uint64_t* run, int cnt, uint64_t k) {
  int lo = 0, hi = cnt;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (run[mid] > k)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// the image's candidate count after the max_nms truncation
__device__ __forceinline__ int nms2_sorted_count(const Nms2Ws& w, int A, int max_nms) {
  const int nch = nms2_a2(A) / NMS2_CH;
  int total = 0;
  for (int r = 0; r < nch; ++r) total += w.ccount[r];
  return min(total, max_nms);
}

__global__ __launch_bounds__(256) void nms2_rank_kernel(const float* pred, int nc, int A, int Mc, int max_nms,
                                                        float max_wh, char* ws, size_t per) {
  const int n = blockIdx.y, chunk = blockIdx.x;
  Nms2Ws w;
  nms2_ws_layout(w, ws + size_t(n) * per, A, Mc);
  const int nch = nms2_a2(A) / NMS2_CH;
  const int M = nms2_sorted_count(w, A, max_nms);
  const int mine = w.ccount[chunk];
  const uint64_t* run = w.keys + size_t(chunk) * NMS2_CH;
  const float* P = pred + int64_t(n) * (4 + nc) * A;
  int deg = 0;
  for (int i = threadIdx.x; i < mine; i += 256) {
    const uint64_t k = run[i];
    int rank = i;
    for (int r = 0; r < nch; ++r)
      if (r != chunk) rank += count_greater(w.keys + size_t(r) * NMS2_CH, w.ccount[r], k);
    if (rank >= M) continue;
    const int a = int(0xFFFFFFFFu - uint32_t(k));
    const int j = w.acls[a];
    float ar;
    w.sbox[rank] = class_box(load_box(P, A, a), j, max_wh, &ar, &deg);
    w.sarea[rank] = ar;
    w.sanc[rank] = a;
    w.sscore[rank] = __uint_as_float(uint32_t(k >> 32));
    w.scls[rank] = j;
  }
  if (__any(deg) && (threadIdx.x & 63) == 0) atomicOr(w.flags, 1);
}

// the greedy's view of the rank-ordered arrays: a sorted position is its own id
struct RankedView {
  Nms2Ws w;
  __device__ __forceinline__ int id(int i) const { return i; }
  __device__ __forceinline__ float4 box(int i) const { return w.sbox[i]; }
  __device__ __forceinline__ float area(int i) const { return w.sarea[i]; }
  __device__ __forceinline__ int anchor(int i) const { return w.sanc[i]; }
  __device__ __forceinline__ float score(int i) const { return w.sscore[i]; }
  __device__ __forceinline__ int cls(int i) const { return w.scls[i]; }
};

__global__ __launch_bounds__(NMS2_G_THREADS) void nms2_greedy_kernel(const float* pred, int nc, int A, int Mc,
                                                                     float iou_thres, int max_det, int max_nms,
                                                                     char* ws, size_t per, float* dets,
                                                                     int64_t* keep, int32_t* counts) {
  extern __shared__ __attribute__((aligned(16))) char g2pool[];  // removed [Mc] | kbox | karea | kidx (nms2_greedy_lds)
  FCE_GREEDY_TILE(tile);
  const int n = blockIdx.x;
  RankedView view;
  nms2_ws_layout(view.w, ws + size_t(n) * per, A, Mc);
  const int M = nms2_sorted_count(view.w, A, max_nms);
  const bool degenerate = view.w.flags[0] != 0;
  const NmsOut out{pred + int64_t(n) * (4 + nc) * A, A, dets + int64_t(n) * max_det * 6, keep + int64_t(n) * max_det};
  GreedyLds g;
  g.removed = reinterpret_cast<uint8_t*>(g2pool);
  g.kbox = reinterpret_cast<float4*>(g2pool + ((Mc + 15) & ~15));
  g.karea = reinterpret_cast<float*>(g.kbox + max_det);
  g.kidx = reinterpret_cast<int*>(g.karea + max_det);
  if (threadIdx.x == 0) tile.kept = 0;
  __syncthreads();

  if (degenerate) {
    const int kept = literal_greedy<NMS2_G_THREADS>(view, out, g.removed, M, iou_thres, max_det);
    if (threadIdx.x == 0) counts[n] = kept;
    return;
  }
  GreedyDiag<false> dg;  // no diagnostics on this path
  tiled_greedy<NMS2_G_THREADS, false, false>(view, g, tile, M, iou_thres, max_det, WIN, dg);
  for (int slot = threadIdx.x; slot < tile.kept; slot += NMS2_G_THREADS) emit_det(view, out, g.kidx[slot], slot);
  if (threadIdx.x == 0) counts[n] = tile.kept;
}

int nms2(const float* pred, const unsigned long long* best, int n, int nc, int A, float conf, float iou, int max_det,
         int max_nms, float max_wh, char* ws, size_t per, float* dets, int64_t* keep, int32_t* counts, hipStream_t s,
         const NmsClassMask& cm) {
  const int Mc = std::min(A, max_nms);
  const int A2 = nms2_a2(A), nch = A2 / NMS2_CH;
  const size_t lds = nms2_greedy_lds(A, max_det, max_nms);
  FCE_CHECK(lds <= 64 * 1024, "nms: greedy LDS over 64 KiB");
  FCE_LAUNCH(nms2_keys_kernel, dim3(A2 / 256, n), dim3(256), 0, s, pred, best, nc, A, Mc, conf, ws, per, cm);
  FCE_LAUNCH(nms2_sort_kernel, dim3(nch, n), dim3(NMS2_SORT_THREADS), 0, s, A, Mc, ws, per);
  FCE_LAUNCH(nms2_rank_kernel, dim3(nch, n), dim3(256), 0, s, pred, nc, A, Mc, max_nms, max_wh, ws, per);
  FCE_LAUNCH(nms2_greedy_kernel, dim3(n), dim3(NMS2_G_THREADS), lds, s, pred, nc, A, Mc, iou, max_det, max_nms, ws,
             per, dets, keep, counts);
  return launch_status("nms2_greedy_kernel");
}

}  // namespace fce
