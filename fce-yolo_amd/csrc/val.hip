// Detection validation on the device: the ground-truth matching of the reference's validation loop
// (ultralytics/models/yolo/detect/val.py:274-288 _process_batch -> utils/metrics.py:57-77 box_iou ->
// engine/validator.py:266-306 BaseValidator.match_predictions, the numpy variant), one launch per batch.
//
// Per image the reference forms iou[g, d] = box_iou(gt, det) * (gt_cls[g] == det_cls[d]) and, for every threshold t,
// sorts the pairs with iou >= t by IoU descending, keeps the first pair of every detection, then the first pair of
// every GT in the resulting (detection-ascending) order.  The first step leaves every detection with its best GT,
// whatever t is; the second gives a GT to the lowest-indexed detection that holds it.  So with
//   g*(d) = arg max_g iou[g, d],   m(d) = max_g iou[g, d]
//   tp[d, i] = m(d) >= iouv[i]  and  no d' < d has g*(d') == g*(d) and m(d') >= iouv[i]
// the result is the reference's in every cell ("Validation").  Exactly equal IoUs of one detection with two
// GTs are the one undefined spot of the reference (numpy's unstable sort); here the higher GT index wins, which is
// what numpy does for up to 16 matches.
//
// The IoU is the reference's fp32 arithmetic in the reference's order, every operation rounded on its own (no FMA
// contraction, IEEE division), box 1 = GT, box 2 = detection:
//   inter = max(min(a2x, b2x) - max(a1x, b1x), 0) * max(min(a2y, b2y) - max(a1y, b1y), 0)
//   union = (((a2x - a1x) * (a2y - a1y) + (b2x - b1x) * (b2y - b1y)) - inter) + 1e-7f
//   iou   = inter / union
//
// One workgroup per image.  Phase 1: the image's GT goes through LDS in chunks of VAL_GT_CHUNK (box + class); thread
// t owns detections t, t + 256, ... and carries (m, g*) of each across the chunks.  Phase 2: every detection scans the
// detections before it for an earlier claimant of its GT (at most max_det^2 / 2 broadcast reads per image).  The
// per-detection (m | threshold mask, g*) pairs live in LDS up to VAL_DET_LDS detections per image and in the caller's
// workspace beyond (the same kernel, the other address space).
#include "common.h"
#include "ops.h"

namespace fce {

constexpr int VAL_THREADS = 256;
constexpr int VAL_GT_CHUNK = 256;  // GT boxes staged in LDS at a time (box, area, class: 6 KB)
constexpr int VAL_DET_LDS = 512;   // detections per image whose phase-1 results stay in LDS (4 KB)
constexpr int VAL_MAX_IOU = 16;    // thresholds: one bit each of the uint16 result

struct ValIouv {
  float t[VAL_MAX_IOU];  // travels in the kernel arguments: the launch reads no descriptor from memory
};

// Plain operators under contract(off), as tta.hip: hipcc's __fmul_rn / __fsub_rn are ordinary inline functions whose
// operations stay contractable, and `(area_a + area_b) - w * h` through them became one v_fma_f32 (one rounding
// instead of two): IoUs one float step from a threshold then land on the other side.
__device__ __forceinline__ float val_area(float x1, float y1, float x2, float y2) {
#pragma clang fp contract(off)
  return (x2 - x1) * (y2 - y1);
}
__device__ __forceinline__ float val_iou(float a1x, float a1y, float a2x, float a2y, float area_a, float b1x, float b1y,
                                         float b2x, float b2y, float area_b) {
#pragma clang fp contract(off)
  const float w = fmaxf(fminf(a2x, b2x) - fmaxf(a1x, b1x), 0.f);
  const float h = fmaxf(fminf(a2y, b2y) - fmaxf(a1y, b1y), 0.f);
  const float inter = w * h;
  const float uni = ((area_a + area_b) - inter) + 1e-7f;
  return inter / uni;  // IEEE: hipcc's fp32 division is correctly rounded by default, and the build sets no fast-math
}

// grid (n), block (VAL_THREADS).  WS: the per-detection state is in `ws` (2 * max_det words per image), else in LDS
// (max_det <= VAL_DET_LDS, checked on the host).
template <bool WS>
__global__ __launch_bounds__(VAL_THREADS) void val_match_kernel(const float* __restrict__ dets,
                                                                const int32_t* __restrict__ counts, int max_det,
                                                                const float* __restrict__ gt_boxes,
                                                                const float* __restrict__ gt_cls,
                                                                const int32_t* __restrict__ gt_off, const ValIouv iouv,
                                                                int niou, uint32_t* ws, uint16_t* __restrict__ tp) {
  __shared__ float s_box[VAL_GT_CHUNK * 4];
  __shared__ float s_area[VAL_GT_CHUNK];
  __shared__ float s_cls[VAL_GT_CHUNK];
  __shared__ uint32_t s_m[WS ? 1 : VAL_DET_LDS];
  __shared__ int s_g[WS ? 1 : VAL_DET_LDS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int k = min(max(counts[b], 0), max_det);
  const int g0 = gt_off[b];
  const int M = max(gt_off[b + 1] - g0, 0);
  const float* det = dets + int64_t(b) * max_det * 6;
  uint16_t* out = tp + int64_t(b) * max_det;
  if (k == 0 || M == 0) {  // uniform over the block: nothing can match
    for (int d = tid; d < max_det; d += VAL_THREADS) out[d] = 0;
    return;
  }
  // m(d) as float bits during phase 1, the threshold mask afterwards | g*(d) relative to the image's first GT
  uint32_t* bm = WS ? ws + int64_t(b) * max_det * 2 : s_m;
  int* bg = WS ? reinterpret_cast<int*>(ws + int64_t(b) * max_det * 2 + max_det) : s_g;

  // ---------------------------------------------------------------- phase 1: best GT per detection
  for (int c0 = 0; c0 < M; c0 += VAL_GT_CHUNK) {
    const int cn = min(VAL_GT_CHUNK, M - c0);
    if (c0) __syncthreads();  // the previous chunk has been read
    for (int j = tid; j < cn; j += VAL_THREADS) {
      const float* gb = gt_boxes + int64_t(g0 + c0 + j) * 4;
      const float x1 = gb[0], y1 = gb[1], x2 = gb[2], y2 = gb[3];
      s_box[j * 4 + 0] = x1, s_box[j * 4 + 1] = y1, s_box[j * 4 + 2] = x2, s_box[j * 4 + 3] = y2;
      s_area[j] = val_area(x1, y1, x2, y2);
      s_cls[j] = gt_cls[g0 + c0 + j];
    }
    __syncthreads();
    const bool last = c0 + VAL_GT_CHUNK >= M;
    for (int d = tid; d < k; d += VAL_THREADS) {
      const float* p = det + d * 6;
      const float b1x = p[0], b1y = p[1], b2x = p[2], b2y = p[3], cls = p[5];
      const float area_b = val_area(b1x, b1y, b2x, b2y);
      float m = -1.f;  // every IoU is >= 0: the first GT always enters
      int g = -1;
      if (c0) m = __uint_as_float(bm[d]), g = bg[d];  // this thread's own entries: no barrier needed
      for (int j = 0; j < cn; ++j) {  // every lane reads the same LDS words: broadcasts
        const float iou = val_iou(s_box[j * 4], s_box[j * 4 + 1], s_box[j * 4 + 2], s_box[j * 4 + 3], s_area[j], b1x,
                                  b1y, b2x, b2y, area_b);
        const float v = s_cls[j] == cls ? iou : 0.f;  // iou * correct_class
        if (v >= m) m = v, g = c0 + j;                // >=: of equal IoUs the higher GT index
      }
      if (last) {
        uint32_t mask = 0;
#pragma unroll
        for (int i = 0; i < VAL_MAX_IOU; ++i)
          if (i < niou && m >= iouv.t[i]) mask |= 1u << i;
        bm[d] = mask;
      } else {
        bm[d] = __float_as_uint(m);
      }
      bg[d] = g;
    }
  }
  __syncthreads();  // every detection's (mask, g*) is visible to the block (LDS, or global at workgroup scope)

  // ---------------------------------------------------------------- phase 2: the first claimant of a GT keeps it
  for (int d = tid; d < max_det; d += VAL_THREADS) {
    uint32_t res = 0;
    if (d < k) {
      const uint32_t mine = bm[d];
      if (mine) {
        const int g = bg[d];
        uint32_t claimed = 0;
        for (int e = 0; e < d; ++e)
          if (bg[e] == g) claimed |= bm[e];
        res = mine & ~claimed;
      }
    }
    out[d] = uint16_t(res);
  }
}

size_t val_match_ws_bytes(int n, int max_det, int max_gt_total, int niou) {
  (void)max_gt_total, (void)niou;  // the GT is never copied: it is read in place, chunk by chunk
  if (n <= 0 || max_det <= VAL_DET_LDS) return 0;
  return size_t(n) * size_t(max_det) * 2 * sizeof(uint32_t);
}

int val_match(const float* dets, const int32_t* counts, int n, int max_det, const float* gt_boxes, const float* gt_cls,
              const int32_t* gt_off, const float* iouv, int niou, void* ws, size_t ws_bytes, uint16_t* tp,
              hipStream_t s) {
  FCE_CHECK(niou >= 1 && niou <= VAL_MAX_IOU, "val_match: niou must be 1..16");
  FCE_CHECK(dets && counts && gt_boxes && gt_cls && gt_off && iouv && tp, "val_match: null argument");
  FCE_CHECK(n > 0 && max_det > 0 && int64_t(n) * max_det <= (int64_t(1) << 30), "val_match: bad n / max_det");
  const size_t need = val_match_ws_bytes(n, max_det, 0, niou);
  FCE_CHECK(need == 0 || (ws && ws_bytes >= need), "val_match: workspace too small (fce_val_match_workspace_bytes)");
  FCE_CHECK(need == 0 || reinterpret_cast<uintptr_t>(ws) % 4 == 0, "val_match: workspace must be 4-byte aligned");
  ValIouv t{};
  for (int i = 0; i < niou; ++i) t.t[i] = iouv[i];
  if (need)
    FCE_LAUNCH(val_match_kernel<true>, dim3(n), dim3(VAL_THREADS), 0, s, dets, counts, max_det, gt_boxes, gt_cls,
               gt_off, t, niou, static_cast<uint32_t*>(ws), tp);
  else
    FCE_LAUNCH(val_match_kernel<false>, dim3(n), dim3(VAL_THREADS), 0, s, dets, counts, max_det, gt_boxes, gt_cls,
               gt_off, t, niou, static_cast<uint32_t*>(nullptr), tp);
  return launch_status("val_match_kernel");
}

// ---------------------------------------------------------------------------------------------------------------
// The confusion matrix of the same loop (models/yolo/detect/val.py update_metrics -> utils/metrics.py:441-518
// ConfusionMatrix.process_batch), accumulated over a whole run in one resident int32 table.
//
// Per image, among the detections with conf > conf_thres and with iou = box_iou(gt, det) NOT masked by class, the
// reference sorts the pairs with iou > iou_thres by IoU descending, keeps the first pair of every detection and then,
// sorted again, the first pair of every GT.  So with g*(d), m(d) as above (without the class mask):
//   d claims g*(d) when m(d) > iou_thres;  w(g) = the claimant of g with the largest m;
//   GT g with a winner:  matrix[cls(w(g)), cls(g)] += 1        GT g without:  matrix[nc, cls(g)] += 1  (FN)
//   participating detection d that is no winner:  matrix[cls(d), nc] += 1  (FP), whether or not it claims a GT
// Exactly equal IoUs are the reference's undefined spots (numpy's unstable sort); here the higher GT index and the
// higher detection index win, which is what numpy does for up to 16 candidate pairs.
//
// One workgroup per image, phase 1 as val_match_kernel's (the same val_iou; state (m bits, claimed GT or CF_*) in LDS
// or the workspace).  Phase 2 goes through the GT in chunks again: thread j scans the detections for the winner of
// GT c0 + j (broadcast reads), adds that GT's cell and leaves the winner in LDS; then every detection claiming a GT of
// the chunk looks its GT's winner up and adds its FP cell if it is another.  The cells are int32 global atomics: sums
// of ones, whatever the order.  A class outside 0..nc-1 (the fp32 class truncated, as .int() does) adds nothing to
// the matrix and one to the error word at the head of the workspace.
constexpr int CF_NO_CLAIM = -1;  // takes part (conf), claims no GT
constexpr int CF_OUT = -2;       // conf <= conf_thres: takes no part
constexpr size_t CF_WS_HEAD = 16;  // bytes: word 0 counts the out-of-range classes met

__device__ __forceinline__ int cf_class(float c, int nc) {
  return (c > -1.f && c < float(nc)) ? int(c) : -1;  // -1: out of range (NaN included)
}

template <bool WS>
__global__ __launch_bounds__(VAL_THREADS) void val_confusion_kernel(
    const float* __restrict__ dets, const int32_t* __restrict__ counts, int max_det,
    const float* __restrict__ gt_boxes, const float* __restrict__ gt_cls, const int32_t* __restrict__ gt_off, int nc,
    float conf, float iou_thres, uint32_t* ws, int32_t* err, int32_t* matrix) {
  __shared__ float s_box[VAL_GT_CHUNK * 4];
  __shared__ float s_area[VAL_GT_CHUNK];
  __shared__ int s_win[VAL_GT_CHUNK];
  __shared__ uint32_t s_m[WS ? 1 : VAL_DET_LDS];
  __shared__ int s_g[WS ? 1 : VAL_DET_LDS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int k = min(max(counts[b], 0), max_det);
  const int g0 = gt_off[b];
  const int M = max(gt_off[b + 1] - g0, 0);
  const float* det = dets + int64_t(b) * max_det * 6;
  const int ld = nc + 1;
  uint32_t* bm = WS ? ws + int64_t(b) * max_det * 2 : s_m;
  int* bg = WS ? reinterpret_cast<int*>(ws + int64_t(b) * max_det * 2 + max_det) : s_g;

  // ---------------------------------------------------------------- phase 1: best GT per participating detection
  if (M == 0)
    for (int d = tid; d < k; d += VAL_THREADS) bg[d] = det[d * 6 + 4] > conf ? CF_NO_CLAIM : CF_OUT;
  for (int c0 = 0; c0 < M; c0 += VAL_GT_CHUNK) {
    const int cn = min(VAL_GT_CHUNK, M - c0);
    if (c0) __syncthreads();  // the previous chunk has been read
    for (int j = tid; j < cn; j += VAL_THREADS) {
      const float* gb = gt_boxes + int64_t(g0 + c0 + j) * 4;
      const float x1 = gb[0], y1 = gb[1], x2 = gb[2], y2 = gb[3];
      s_box[j * 4 + 0] = x1, s_box[j * 4 + 1] = y1, s_box[j * 4 + 2] = x2, s_box[j * 4 + 3] = y2;
      s_area[j] = val_area(x1, y1, x2, y2);
    }
    __syncthreads();
    const bool last = c0 + VAL_GT_CHUNK >= M;
    for (int d = tid; d < k; d += VAL_THREADS) {
      const float* p = det + d * 6;
      if (!(p[4] > conf)) {  // strict, as detections["conf"] > conf
        bg[d] = CF_OUT;
        continue;
      }
      const float b1x = p[0], b1y = p[1], b2x = p[2], b2y = p[3];
      const float area_b = val_area(b1x, b1y, b2x, b2y);
      float m = -1.f;
      int g = CF_NO_CLAIM;
      if (c0) m = __uint_as_float(bm[d]), g = bg[d];  // this thread's own entries: no barrier needed
      for (int j = 0; j < cn; ++j) {
        const float iou = val_iou(s_box[j * 4], s_box[j * 4 + 1], s_box[j * 4 + 2], s_box[j * 4 + 3], s_area[j], b1x,
                                  b1y, b2x, b2y, area_b);
        if (iou >= m) m = iou, g = c0 + j;  // >=: of equal IoUs the higher GT index
      }
      bm[d] = __float_as_uint(m);
      bg[d] = (last && !(m > iou_thres)) ? CF_NO_CLAIM : g;  // strict, as iou > iou_thres
    }
  }
  __syncthreads();  // every detection's (m, claim) is visible to the block (LDS, or global at workgroup scope)

  // ---------------------------------------------------------------- phase 2: the best claimant of a GT keeps it
  for (int c0 = 0; c0 < M; c0 += VAL_GT_CHUNK) {
    const int cn = min(VAL_GT_CHUNK, M - c0);
    if (c0) __syncthreads();  // the previous chunk's winners have been read
    for (int j = tid; j < cn; j += VAL_THREADS) {
      const int g = c0 + j;
      float best = -1.f;
      int win = -1;
      for (int e = 0; e < k; ++e)
        if (bg[e] == g) {
          const float v = __uint_as_float(bm[e]);
          if (v >= best) best = v, win = e;  // >=: of equal IoUs the higher detection index
        }
      s_win[j] = win;
      const int gc = cf_class(gt_cls[g0 + g], nc);
      const int row = win < 0 ? nc : cf_class(det[win * 6 + 5], nc);  // no winner: a false negative
      if (gc >= 0 && row >= 0)
        atomicAdd(matrix + row * ld + gc, 1);
      else
        atomicAdd(err, 1);
    }
    __syncthreads();
    for (int d = tid; d < k; d += VAL_THREADS) {
      const int g = bg[d];
      if (g < c0 || g >= c0 + cn || s_win[g - c0] == d) continue;
      const int dc = cf_class(det[d * 6 + 5], nc);  // its GT went to a better detection: a false positive
      if (dc >= 0)
        atomicAdd(matrix + dc * ld + nc, 1);
      else
        atomicAdd(err, 1);
    }
  }
  for (int d = tid; d < k; d += VAL_THREADS) {
    if (bg[d] != CF_NO_CLAIM) continue;
    const int dc = cf_class(det[d * 6 + 5], nc);  // no GT above the threshold: a false positive
    if (dc >= 0)
      atomicAdd(matrix + dc * ld + nc, 1);
    else
      atomicAdd(err, 1);
  }
}

size_t val_confusion_ws_bytes(int n, int max_det) {
  if (n <= 0 || max_det <= 0) return 0;
  return CF_WS_HEAD + (max_det <= VAL_DET_LDS ? 0 : size_t(n) * size_t(max_det) * 2 * sizeof(uint32_t));
}

int val_confusion(const float* dets, const int32_t* counts, int n, int max_det, const float* gt_boxes,
                  const float* gt_cls, const int32_t* gt_off, int nc, float conf, float iou_thres, void* ws,
                  size_t ws_bytes, int32_t* matrix, hipStream_t s) {
  FCE_CHECK(dets && counts && gt_boxes && gt_cls && gt_off && matrix, "val_confusion: null argument");
  FCE_CHECK(n > 0 && max_det > 0 && int64_t(n) * max_det <= (int64_t(1) << 30), "val_confusion: bad n / max_det");
  FCE_CHECK(nc > 0 && nc < (1 << 15), "val_confusion: nc must be 1..32767");
  FCE_CHECK(conf >= 0.f && conf <= 1.f && iou_thres >= 0.f && iou_thres <= 1.f,
            "val_confusion: conf and iou_thres must be in 0..1");
  const size_t need = val_confusion_ws_bytes(n, max_det);
  FCE_CHECK(ws && ws_bytes >= need, "val_confusion: workspace too small (fce_val_confusion_workspace_bytes)");
  FCE_CHECK(reinterpret_cast<uintptr_t>(ws) % 4 == 0, "val_confusion: workspace must be 4-byte aligned");
  int32_t* err = static_cast<int32_t*>(ws);
  uint32_t* state = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + CF_WS_HEAD);
  if (max_det > VAL_DET_LDS)
    FCE_LAUNCH(val_confusion_kernel<true>, dim3(n), dim3(VAL_THREADS), 0, s, dets, counts, max_det, gt_boxes, gt_cls,
               gt_off, nc, conf, iou_thres, state, err, matrix);
  else
    FCE_LAUNCH(val_confusion_kernel<false>, dim3(n), dim3(VAL_THREADS), 0, s, dets, counts, max_det, gt_boxes, gt_cls,
               gt_off, nc, conf, iou_thres, static_cast<uint32_t*>(nullptr), err, matrix);
  return launch_status("val_confusion_kernel");
}

}  // namespace fce
