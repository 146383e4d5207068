// C-ABI entry points (include/fce_yolo.h) of the standalone ops, and the thread-local error and probe state every
// unit reports through.  The fce_net executor's entry points are in net_build.hip, net_plan.hip and net_run.hip.
#include "ops.h"

namespace fce {

static thread_local std::string g_err;
static thread_local LaunchProbe* g_probe = nullptr;
LaunchProbe*& probe_slot() { return g_probe; }
void set_error(const std::string& m) { g_err = m; }
int fail(int code, const std::string& m) {
  g_err = m;
  return code;
}
int check_nhwc(const fce_tensor* t, const char* name, int dtype) {
  if (!t) return fail(FCE_ERR_INVALID, std::string(name) + ": null tensor");
  if (t->layout != FCE_NHWC || t->dtype != dtype) return fail(FCE_ERR_INVALID, std::string(name) + ": wrong layout/dtype");
  return FCE_OK;
}

}  // namespace fce

using namespace fce;

extern "C" {

const char* fce_last_error(void) { return g_err.c_str(); }
int fce_abi_version(void) { return FCE_ABI_VERSION; }
int fce_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

size_t fce_conv_weight_bytes(const fce_conv_desc* d) { return d ? conv_weight_bytes(*d) : 0; }
int fce_conv_pack_weights(const fce_conv_desc* d, const float* w, void* out) {
  FCE_CHECK(d && w && out, "fce_conv_pack_weights: null argument");
  FCE_GUARD(return conv_pack(*d, w, out);)
}
int fce_conv2d(const fce_conv_desc* d, const fce_tensor* x, const void* w, const float* bias, const fce_tensor* res,
               const fce_tensor* y, void* stream) {
  FCE_CHECK(d && x && w && bias && y, "fce_conv2d: null argument");
  FCE_GUARD(return conv2d(*d, *x, w, bias, res, *y, S(stream));)
}
int fce_conv_variants(const fce_conv_desc* d, int in_w, int* codes, int cap) {
  if (!d || !codes || cap <= 0) return 0;
  return conv_tile_candidates(*d, 0, in_w, codes, cap);
}
int fce_conv2d_variant(const fce_conv_desc* d, const fce_tensor* x, const void* w, const float* bias,
                       const fce_tensor* res, const fce_tensor* y, int variant, void* stream) {
  FCE_CHECK(d && x && w && bias && y, "fce_conv2d_variant: null argument");
  FCE_GUARD(return conv2d(*d, *x, w, bias, res, *y, S(stream), variant);)
}
int fce_conv2d_variant_dup(const fce_conv_desc* d, const fce_tensor* x, const void* w, const float* bias,
                           const fce_tensor* res, const fce_tensor* y, int variant, const fce_tensor* dup, int dup_lo,
                           void* stream) {
  FCE_CHECK(d && x && w && bias && y && dup, "fce_conv2d_variant_dup: null argument");
  FCE_CHECK(d->k == 1 && d->groups == 1 && d->epilogue == FCE_EPI_STORE && dup->dtype == FCE_F16 &&
                dup->layout == FCE_NHWC && dup_lo >= 0 && dup_lo % 8 == 0 && dup->c % 8 == 0 &&
                dup_lo + dup->c <= d->cout && dup->n == y->n && dup->h == y->h && dup->w == y->w,
            "fce_conv2d_variant_dup: the duplicate store needs a plain 1x1 conv and an aligned f16 view of y's size");
  FCE_GUARD(return conv2d(*d, *x, w, bias, res, *y, S(stream), variant, dup, dup_lo);)
}
int fce_c3k2_supported(const fce_c3k2_desc* d) { return d && c3k2_fused_ok(*d) ? 1 : 0; }
int fce_c3k2(const fce_c3k2_desc* d, const fce_tensor* x, const fce_tensor* y, void* stream) {
  FCE_CHECK(d && x && y, "fce_c3k2: null argument");
  FCE_GUARD(return c3k2_fused(*d, *x, *y, S(stream));)
}
int fce_detect_cls_supported(const fce_dcls_desc* d) { return d && detect_cls_fused_ok(*d) ? 1 : 0; }
int fce_detect_cls(const fce_dcls_desc* d, const fce_tensor* x, const fce_detect_epi* e, void* stream) {
  FCE_CHECK(d && x && e, "fce_detect_cls: null argument");
  FCE_GUARD(return detect_cls_fused(*d, *x, *e, S(stream));)
}
int fce_bneck_supported(const fce_bneck_desc* d) { return d && bneck_fused_ok(*d) ? 1 : 0; }
int fce_bneck_fused(const fce_bneck_desc* d, const fce_tensor* x, const fce_tensor* y, void* stream) {
  FCE_CHECK(d && x && y, "fce_bneck_fused: null argument");
  FCE_GUARD(return bneck_fused(*d, *x, *y, S(stream));)
}
int fce_pw2_supported(const fce_pw2_desc* d) { return d && pw2_fused_ok(*d) ? 1 : 0; }
int fce_pw2(const fce_pw2_desc* d, const fce_tensor* x1, const fce_tensor* r1, const fce_tensor* h, int h_store,
            const fce_tensor* x2, const fce_tensor* r2, const fce_tensor* y, const fce_tensor* dup, int dup_lo,
            void* stream) {
  FCE_CHECK(d && x1 && h && x2 && y, "fce_pw2: null argument");
  FCE_GUARD(return pw2_fused(*d, *x1, r1, *h, h_store, *x2, r2, *y, dup, dup_lo, S(stream));)
}
int fce_stem_fused_supported(const fce_stem2_desc* d) { return d && stem_fused_ok(*d) ? 1 : 0; }
int fce_stem_fused(const fce_stem2_desc* d, const fce_tensor* x, const fce_tensor* y, void* stream) {
  FCE_CHECK(d && x && y, "fce_stem_fused: null argument");
  FCE_GUARD(return stem_fused(*d, *x, *y, S(stream));)
}
int fce_conv2d_detect(const fce_conv_desc* d, const fce_tensor* x, const void* w, const float* bias,
                      const fce_detect_epi* e, void* stream) {
  FCE_CHECK(d && x && w && bias && e, "fce_conv2d_detect: null argument");
  FCE_GUARD(return conv2d_detect(*d, *x, w, bias, *e, S(stream));)
}
int fce_maxpool_chain(const fce_tensor* x, const fce_tensor* y1, const fce_tensor* y2, const fce_tensor* y3, int k,
                      void* stream) {
  FCE_CHECK(x && y1 && y2 && y3, "fce_maxpool_chain: null argument");
  FCE_GUARD(return maxpool_chain(*x, *y1, *y2, *y3, k, S(stream));)
}
int fce_weighted_add(const fce_tensor* x, int up, const float* fw, int fn, int fi, int accumulate, const fce_tensor* y,
                     void* stream) {
  FCE_CHECK(x && y, "fce_weighted_add: null argument");
  FCE_GUARD(return weighted_add(*x, up, fw, fn, fi, accumulate, *y, S(stream));)
}
size_t fce_coord_workspace_bytes(const fce_coord_desc* d, int n, int h, int w) {
  return d ? coord_ws_bytes(*d, n, h, w) : 0;
}
int fce_bicoordcrossatt(const fce_coord_desc* d, const fce_tensor* x, const fce_tensor* y, void* ws, size_t wsb,
                        void* stream) {
  FCE_CHECK(d && x && y, "fce_bicoordcrossatt: null argument");
  FCE_GUARD(return bicoordcrossatt(*d, *x, *y, ws, wsb, S(stream));)
}
int fce_coordatt(const fce_coord_desc* d, const fce_tensor* x, const fce_tensor* y, void* ws, size_t wsb,
                 void* stream) {
  FCE_CHECK(d && x && y, "fce_coordatt: null argument");
  FCE_GUARD(return coordatt(*d, *x, *y, ws, wsb, S(stream));)
}
int fce_coordcrossatt(const fce_coord_desc* d, const fce_tensor* x, const fce_tensor* y, void* ws, size_t wsb,
                      void* stream) {
  FCE_CHECK(d && x && y, "fce_coordcrossatt: null argument");
  FCE_GUARD(return coordcrossatt(*d, *x, *y, ws, wsb, S(stream));)
}
int fce_psa_attention(const fce_tensor* qkv, int heads, int kd, int hd, const float* pe_w, const float* pe_b,
                      const fce_tensor* y, void* stream) {
  FCE_CHECK(qkv && y && pe_w && pe_b, "fce_psa_attention: null argument");
  FCE_GUARD(return psa_attention(*qkv, heads, kd, hd, pe_w, pe_b, *y, S(stream));)
}
int fce_detect_decode(const fce_tensor* box, const fce_tensor* cls, int nl, const float* strides, int reg_max,
                      float* out, void* stream) {
  FCE_CHECK(box && cls && strides && out, "fce_detect_decode: null argument");
  FCE_GUARD(return detect_decode(box, cls, nl, strides, reg_max, out, S(stream));)
}
size_t fce_nms_workspace_bytes(int n, int anchors, int max_nms) { return nms_ws_bytes(n, anchors, max_nms); }
int fce_nms(const float* pred, int n, int nc, int A, float conf, float iou, int max_det, int max_nms, float max_wh,
            void* ws, size_t wsb, float* dets, int64_t* keep, int32_t* counts, void* stream) {
  FCE_CHECK(pred && dets && keep && counts, "fce_nms: null argument");
  FCE_GUARD(return nms(pred, nullptr, n, nc, A, conf, iou, max_det, max_nms, max_wh, ws, wsb, dets, keep, counts,
                       S(stream));)
}
int fce_nms_best(const float* pred, const unsigned long long* best, int n, int nc, int A, float conf, float iou,
                 int max_det, int max_nms, float max_wh, void* ws, size_t wsb, float* dets, int64_t* keep,
                 int32_t* counts, void* stream) {
  FCE_CHECK(pred && best && dets && keep && counts, "fce_nms_best: null argument");
  FCE_GUARD(return nms(pred, best, n, nc, A, conf, iou, max_det, max_nms, max_wh, ws, wsb, dets, keep, counts,
                       S(stream));)
}
size_t fce_nms_workspace_bytes_ex(int n, int nc, int anchors, const fce_nms_opts* o) {
  return o ? nms_ws_bytes_ex(n, nc, anchors, o->max_nms, o->multi_label) : 0;
}
int fce_nms_ex(const float* pred, const unsigned long long* best, int n, int nc, int A, const fce_nms_opts* o, void* ws,
               size_t wsb, float* dets, int64_t* keep, int32_t* counts, void* stream) {
  FCE_CHECK(pred && o && dets && keep && counts, "fce_nms_ex: null argument");
  FCE_GUARD(return nms(pred, best, n, nc, A, o->conf_thres, o->iou_thres, o->max_det, o->max_nms,
                       o->agnostic ? 0.f : o->max_wh, ws, wsb, dets, keep, counts, S(stream), o->multi_label,
                       o->classes, o->nclasses);)
}
int fce_letterbox(const fce_letterbox_img* imgs, int n, uint8_t* dst, int H, int W, int pad_value, void* stream) {
  FCE_GUARD(return letterbox(imgs, n, dst, H, W, pad_value, S(stream));)
}
int fce_scale_boxes(float* dets, const int32_t* counts, int n, int max_det, const fce_box_scale* params,
                    void* stream) {
  FCE_GUARD(return scale_boxes(dets, counts, n, max_det, params, S(stream));)
}
int fce_tta_scale_img(const fce_tensor* x, const fce_tensor* y, int flip, int h_s, int w_s, float pad_value,
                      void* stream) {
  FCE_CHECK(x && y, "fce_tta_scale_img: null argument");
  FCE_GUARD(return tta_scale_img(*x, *y, flip, h_s, w_s, pad_value, S(stream));)
}
int fce_tta_merge(const fce_tta_part* parts, int nparts, int batch, int rows, float* pred, unsigned long long* best,
                  void* stream) {
  FCE_GUARD(return tta_merge(parts, nparts, batch, rows, pred, best, S(stream));)
}
size_t fce_val_match_workspace_bytes(int n, int max_det, int max_gt_total, int niou) {
  return val_match_ws_bytes(n, max_det, max_gt_total, niou);
}
int fce_val_match(const float* dets, const int32_t* counts, int n, int max_det, const float* gt_boxes,
                  const float* gt_cls, const int32_t* gt_off, const float* iouv, int niou, void* ws, size_t ws_bytes,
                  uint16_t* tp, void* stream) {
  FCE_GUARD(return val_match(dets, counts, n, max_det, gt_boxes, gt_cls, gt_off, iouv, niou, ws, ws_bytes, tp,
                             S(stream));)
}
size_t fce_val_confusion_workspace_bytes(int n, int max_det) { return val_confusion_ws_bytes(n, max_det); }
int fce_val_confusion(const float* dets, const int32_t* counts, int n, int max_det, const float* gt_boxes,
                      const float* gt_cls, const int32_t* gt_off, int nc, float conf, float iou_thres, void* ws,
                      size_t ws_bytes, int32_t* matrix, void* stream) {
  FCE_GUARD(return val_confusion(dets, counts, n, max_det, gt_boxes, gt_cls, gt_off, nc, conf, iou_thres, ws, ws_bytes,
                                 matrix, S(stream));)
}
int fce_copy(const fce_tensor* src, const fce_tensor* dst, void* stream) {
  FCE_CHECK(src && dst, "fce_copy: null argument");
  FCE_GUARD(return copy(*src, *dst, S(stream));)
}

}  // extern "C"
