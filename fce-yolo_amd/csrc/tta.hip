// Test-time augmentation around the detection forward: the two device steps of the reference's three-pass
// DetectionModel._predict_augment (ultralytics/nn/tasks.py:422-484) that are not a forward.
//
// tta_scale_img_kernel replaces utils/torch_utils.py:476-495 scale_img with the `x.flip(fi)` of tasks.py:439 folded
// in: flip, bilinear resize to (h_s, w_s), pad right / bottom with `pad` up to the scaled pass's canvas, written as
// the fp16 NCHW input of that pass's engine.  The resize is ATen's upsample_bilinear2d with align_corners = False and
// an explicit size (F.interpolate(size=s)), restated:
//   scale = (float)in / out;  src = max((dst + 0.5f) * scale - 0.5f, 0);  i0 = (int)src;  i1 = min(i0 + 1, in - 1);
//   l1 = src - i0;  l0 = 1 - l1;   v = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d)
// in fp32 on the fp16-rounded source values (what the fp16 model sees: f32 inputs are rounded, u8 inputs become
// fp16(v / 255) as the stem reads them), every operation rounded on its own (no FMA contraction), then rounded once
// to fp16.  A ratio of 1 gives src = dst, l1 = 0 and v = a: the plain converted copy.
//
// tta_merge_kernel replaces _descale_pred (:446-466), _clip_augmented (:468-484) and the torch.cat of :444 in one
// launch: anchors [first, first + count) of every pass's (B, R, A_i) prediction go to their segment of the merged
// (B, R, sum count) tensor, rows 0..3 divided by the pass's scale (an IEEE fp32 division, as `p[:, :4] /= scale`),
// cx / cy mirrored for a flipped pass; the other rows and the per-anchor best-class keys (score and class only) are
// copied.  The parts travel in the kernel arguments, so the launch reads no descriptor from memory and can be captured.
#include "common.h"
#include "ops.h"

namespace fce {

// ---------------------------------------------------------------- scale_img
template <typename T>
__device__ __forceinline__ float tta_src(const T* p);
template <>
__device__ __forceinline__ float tta_src<_Float16>(const _Float16* p) {
  return (float)*p;
}
template <>
__device__ __forceinline__ float tta_src<float>(const float* p) {
  return (float)(_Float16)*p;
}
template <>
__device__ __forceinline__ float tta_src<uint8_t>(const uint8_t* p) {
  return (float)(_Float16)((float)*p / 255.0f);  // stem.hip u8_to_unit
}

struct TtaAxis {
  int i0, i1;    // source samples (of the flipped image)
  float l0, l1;  // their weights
};

__device__ __forceinline__ TtaAxis tta_axis(int d, int in, float scale) {
#pragma clang fp contract(off)
  float src = (float(d) + 0.5f) * scale - 0.5f;
  src = src < 0.f ? 0.f : src;
  TtaAxis a;
  a.i0 = min(int(src), in - 1);
  a.i1 = min(a.i0 + 1, in - 1);
  a.l1 = src - float(a.i0);
  a.l0 = 1.f - a.l1;
  return a;
}

constexpr int TTA_PX = 4;  // consecutive output columns per thread (one 8-byte store)

// block (64, 4): 64 threads x TTA_PX columns along W, 4 rows; grid (ceil(Wc / 256), ceil(Hc / 4), B * 3 planes)
template <typename T>
__global__ __launch_bounds__(256) void tta_scale_img_kernel(const T* __restrict__ src, _Float16* __restrict__ dst,
                                                            int H, int W, int hs, int ws, int Hc, int Wc, int flip,
                                                            float sh, float sw, float pad) {
#pragma clang fp contract(off)
  const int x0 = (blockIdx.x * 64 + threadIdx.x) * TTA_PX, y = blockIdx.y * 4 + threadIdx.y;
  if (x0 >= Wc || y >= Hc) return;
  const int64_t plane = blockIdx.z;
  const T* s = src + plane * H * W;
  _Float16* o = dst + (plane * Hc + y) * Wc + x0;
  const _Float16 hpad = (_Float16)pad;
  h4 out = {hpad, hpad, hpad, hpad};
  if (y < hs && x0 < ws) {
    const TtaAxis ay = tta_axis(y, H, sh);
    const int r0 = flip == 2 ? H - 1 - ay.i0 : ay.i0, r1 = flip == 2 ? H - 1 - ay.i1 : ay.i1;
    const T* p0 = s + int64_t(r0) * W;
    const T* p1 = s + int64_t(r1) * W;
#pragma unroll
    for (int j = 0; j < TTA_PX; ++j) {
      if (x0 + j < ws) {
        const TtaAxis ax = tta_axis(x0 + j, W, sw);
        const int c0 = flip == 3 ? W - 1 - ax.i0 : ax.i0, c1 = flip == 3 ? W - 1 - ax.i1 : ax.i1;
        const float a = tta_src(p0 + c0), b = tta_src(p0 + c1), c = tta_src(p1 + c0), d = tta_src(p1 + c1);
        const float top = ax.l0 * a + ax.l1 * b, bot = ax.l0 * c + ax.l1 * d;
        out[j] = (_Float16)fpin(ay.l0 * top + ay.l1 * bot);
      }
    }
  }
  if ((Wc & 3) == 0) {  // x0 % 4 == 0: the row start and x0 are 8-byte aligned (dst is checked on the host)
    *reinterpret_cast<h4*>(o) = out;
  } else {
#pragma unroll
    for (int j = 0; j < TTA_PX; ++j)
      if (x0 + j < Wc) o[j] = out[j];
  }
}

int tta_scale_img(const fce_tensor& x, const fce_tensor& y, int flip, int hs, int ws, float pad, hipStream_t s) {
  FCE_CHECK(x.data && y.data, "tta_scale_img: null data pointer");
  FCE_CHECK(x.layout == FCE_NCHW && y.layout == FCE_NCHW, "tta_scale_img: x and y must be NCHW");
  FCE_CHECK(x.dtype == FCE_F16 || x.dtype == FCE_F32 || x.dtype == FCE_U8, "tta_scale_img: x must be f16, f32 or u8");
  FCE_CHECK(y.dtype == FCE_F16, "tta_scale_img: y must be f16");
  FCE_CHECK(flip == 0 || flip == 2 || flip == 3, "tta_scale_img: flip must be 0 (none), 2 (up-down) or 3 (left-right)");
  FCE_CHECK(x.n > 0 && x.c > 0 && x.h > 0 && x.w > 0 && y.n == x.n && y.c == x.c, "tta_scale_img: bad shapes");
  FCE_CHECK(hs > 0 && ws > 0 && hs <= y.h && ws <= y.w, "tta_scale_img: the resized size must fit the canvas");
  FCE_CHECK(reinterpret_cast<uintptr_t>(y.data) % 8 == 0, "tta_scale_img: y must be 8-byte aligned");
  const int64_t planes = int64_t(x.n) * x.c;
  const int gy = (y.h + 3) / 4;
  FCE_CHECK(planes <= 65535 && gy <= 65535, "tta_scale_img: batch * channels / height too large for the grid");
  const float sh = float(x.h) / float(hs), sw = float(x.w) / float(ws);
  const dim3 grid((y.w + 64 * TTA_PX - 1) / (64 * TTA_PX), gy, unsigned(planes)), block(64, 4);
  _Float16* o = static_cast<_Float16*>(y.data);
  if (x.dtype == FCE_F16)
    FCE_LAUNCH(tta_scale_img_kernel<_Float16>, grid, block, 0, s, static_cast<const _Float16*>(x.data), o, x.h, x.w, hs,
               ws, y.h, y.w, flip, sh, sw, pad);
  else if (x.dtype == FCE_F32)
    FCE_LAUNCH(tta_scale_img_kernel<float>, grid, block, 0, s, static_cast<const float*>(x.data), o, x.h, x.w, hs, ws,
               y.h, y.w, flip, sh, sw, pad);
  else
    FCE_LAUNCH(tta_scale_img_kernel<uint8_t>, grid, block, 0, s, static_cast<const uint8_t*>(x.data), o, x.h, x.w, hs,
               ws, y.h, y.w, flip, sh, sw, pad);
  return launch_status("tta_scale_img_kernel");
}

// ---------------------------------------------------------------- merge
constexpr int TTA_MAX_PARTS = 4;
constexpr int TTA_ROWS = 4;  // pred rows per thread (independent loads in flight)

struct TtaMergeArgs {
  fce_tta_part p[TTA_MAX_PARTS];
  int off[TTA_MAX_PARTS + 1];  // segment starts in the merged anchor axis; unused parts and the end: A_total
  int n, rows;
};

// One thread per merged anchor; blockIdx.y < ceil(rows / TTA_ROWS): that group of pred rows, the last blockIdx.y: the
// best-class keys; blockIdx.z: image.  Segment starts are arbitrary, so source and destination are accessed one
// element per lane (a wave reads and writes 256 or 512 contiguous bytes), never as wider vectors.
__global__ __launch_bounds__(256) void tta_merge_kernel(const TtaMergeArgs a, float* __restrict__ pred,
                                                        unsigned long long* __restrict__ best) {
  const int A = a.off[TTA_MAX_PARTS];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= A) return;
  int k = 0;
#pragma unroll
  for (int i = 1; i < TTA_MAX_PARTS; ++i)
    if (j >= a.off[i]) k = i;  // unused parts start at A_total
  // the parts live in the kernel arguments: select fields one by one (no runtime-indexed private copy)
  const float* sp = a.p[0].pred;
  const unsigned long long* sb = a.p[0].best;
  int Ak = a.p[0].anchors, first = a.p[0].first, flip = a.p[0].flip, ih = a.p[0].img_h, iw = a.p[0].img_w;
  int off = a.off[0];
  float scale = a.p[0].scale;
#pragma unroll
  for (int i = 1; i < TTA_MAX_PARTS; ++i)
    if (k == i) {
      sp = a.p[i].pred, sb = a.p[i].best, Ak = a.p[i].anchors, first = a.p[i].first, flip = a.p[i].flip;
      ih = a.p[i].img_h, iw = a.p[i].img_w, off = a.off[i], scale = a.p[i].scale;
    }
  const int64_t b = blockIdx.z;
  const int src_a = first + (j - off);
  const int groups = (a.rows + TTA_ROWS - 1) / TTA_ROWS;
  if (int(blockIdx.y) == groups) {
    if (best) best[b * A + j] = sb[b * Ak + src_a];
    return;
  }
  const int r0 = blockIdx.y * TTA_ROWS;
  const float* s = sp + (b * a.rows + r0) * Ak + src_a;
  float* o = pred + (b * a.rows + r0) * A + j;
  float v[TTA_ROWS];
#pragma unroll
  for (int r = 0; r < TTA_ROWS; ++r) v[r] = r0 + r < a.rows ? s[int64_t(r) * Ak] : 0.f;
  if (r0 == 0) {  // rows 0..3 = cx, cy, w, h (TTA_ROWS == 4; rows >= 4 is checked on the host)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = scale == 1.f ? v[r] : v[r] / scale;  // x / 1 is x: the unscaled pass copies
    if (flip == 3) v[0] = float(iw) - v[0];
    if (flip == 2) v[1] = float(ih) - v[1];
  }
#pragma unroll
  for (int r = 0; r < TTA_ROWS; ++r)
    if (r0 + r < a.rows) o[int64_t(r) * A] = v[r];
}

int tta_merge(const fce_tta_part* parts, int nparts, int batch, int rows, float* pred, unsigned long long* best,
              hipStream_t s) {
  static_assert(TTA_ROWS == 4, "the box rows are one row group");
  FCE_CHECK(nparts >= 1 && nparts <= TTA_MAX_PARTS, "tta_merge: 1..4 parts");
  FCE_CHECK(parts && pred, "tta_merge: null argument");
  FCE_CHECK(batch > 0 && batch <= 65535 && rows >= 4 && rows <= 65535 * TTA_ROWS - TTA_ROWS, "tta_merge: bad batch / rows");
  TtaMergeArgs a{};
  a.n = nparts, a.rows = rows;
  int64_t total = 0;
  for (int i = 0; i < nparts; ++i) {
    const fce_tta_part& p = parts[i];
    FCE_CHECK(p.pred, "tta_merge: a part has no pred");
    FCE_CHECK(!best || p.best, "tta_merge: best-class keys are merged only when every part has them");
    FCE_CHECK(p.anchors > 0 && p.first >= 0 && p.count >= 0 && int64_t(p.first) + p.count <= p.anchors,
              "tta_merge: a part's [first, first + count) is outside its anchors");
    FCE_CHECK(p.flip == 0 || p.flip == 2 || p.flip == 3, "tta_merge: flip must be 0 (none), 2 (up-down) or 3 (left-right)");
    FCE_CHECK(p.scale > 0.f, "tta_merge: scale must be positive");
    a.p[i] = p;
    a.off[i] = int(total);
    total += p.count;
    FCE_CHECK(total <= (int64_t(1) << 30), "tta_merge: too many anchors");
  }
  for (int i = nparts; i <= TTA_MAX_PARTS; ++i) a.off[i] = int(total);
  if (total == 0) return FCE_OK;
  const dim3 grid(unsigned((total + 255) / 256), (rows + TTA_ROWS - 1) / TTA_ROWS + (best ? 1 : 0), batch);
  FCE_LAUNCH(tta_merge_kernel, grid, dim3(256), 0, s, a, pred, best);
  return launch_status("tta_merge_kernel");
}

}  // namespace fce
