// Host entry points of the kernel units: the one declaration site.  The C-ABI wrappers (api.hip) and the fce_net
// executor (net_*.hip) call these; every unit that defines one includes this header, so a definition that drifts
// from its declaration fails to compile instead of leaving an undefined symbol in the library.  Host declarations
// only: nothing here reaches device code.
#pragma once
#include <exception>

#include "common.h"

namespace fce {

// conv.hip
size_t conv_weight_bytes(const fce_conv_desc& d);
int conv_pack(const fce_conv_desc& d, const float* w, void* out);
int conv2d(const fce_conv_desc& d, const fce_tensor& x, const void* w, const float* bias, const fce_tensor* res,
           const fce_tensor& y, hipStream_t s, int tile = -1, const fce_tensor* dup = nullptr, int duplo = 0);
int conv2d_detect(const fce_conv_desc& d, const fce_tensor& x, const void* w, const float* bias,
                  const fce_detect_epi& e, hipStream_t s, int tile = -1);
int conv_tile_candidates(const fce_conv_desc& d, int det_box, int in_w, int* out, int cap);
// pool.hip
int maxpool_chain(const fce_tensor& x, const fce_tensor& y1, const fce_tensor& y2, const fce_tensor& y3, int k,
                  hipStream_t s);
int weighted_add(const fce_tensor& x, int up, const float* fw, int fn, int fi, int accumulate, const fce_tensor& y,
                 hipStream_t s);
int copy(const fce_tensor& src, const fce_tensor& dst, hipStream_t s);
// coord.hip
size_t coord_ws_bytes(const fce_coord_desc& d, int n, int h, int w);
int bicoordcrossatt(const fce_coord_desc& d, const fce_tensor& x, const fce_tensor& y, void* ws, size_t wsb,
                    hipStream_t s);
int coordatt(const fce_coord_desc& d, const fce_tensor& x, const fce_tensor& y, void* ws, size_t wsb, hipStream_t s);
int coordcrossatt(const fce_coord_desc& d, const fce_tensor& x, const fce_tensor& y, void* ws, size_t wsb,
                  hipStream_t s);
// psa.hip, detect.hip
int psa_attention(const fce_tensor& qkv, int heads, int key_dim, int head_dim, const float* pe_w, const float* pe_b,
                  const fce_tensor& y, hipStream_t s);
int detect_decode(const fce_tensor* box, const fce_tensor* cls, int nl, const float* strides, int reg_max,
                  float* out, hipStream_t s);
// nms.hip
size_t nms_ws_bytes(int n, int A, int max_nms);
size_t nms_ws_bytes_ex(int n, int nc, int A, int max_nms, int multi);
int nms(const float* pred, const unsigned long long* best, int n, int nc, int A, float conf, float iou, int max_det,
        int max_nms, float max_wh, void* ws, size_t ws_bytes, float* dets, int64_t* keep, int32_t* counts,
        hipStream_t s, int multi = 0, const int32_t* classes = nullptr, int nclasses = 0);
// fused.hip, detect_cls.hip, stem_fused.hip, bneck.hip, pw2.hip: *_ok = the channel configuration is instantiated,
// *_fits = and the kernel covers this map size
bool c3k2_fused_ok(const fce_c3k2_desc& d);
int c3k2_fused(const fce_c3k2_desc& d, const fce_tensor& x, const fce_tensor& y, hipStream_t s);
bool detect_cls_fused_ok(const fce_dcls_desc& d);
int detect_cls_fused(const fce_dcls_desc& d, const fce_tensor& x, const fce_detect_epi& e, hipStream_t s);
bool stem_fused_ok(const fce_stem2_desc& d);
bool stem_fused_fits(const fce_stem2_desc& d, int h, int w);
int stem_fused(const fce_stem2_desc& d, const fce_tensor& x, const fce_tensor& y, hipStream_t s);
bool bneck_fused_ok(const fce_bneck_desc& d);
bool bneck_fused_fits(const fce_bneck_desc& d, int h, int w);
int bneck_fused(const fce_bneck_desc& d, const fce_tensor& x, const fce_tensor& y, hipStream_t s);
bool pw2_fused_ok(const fce_pw2_desc& d);
int pw2_fused(const fce_pw2_desc& d, const fce_tensor& x1, const fce_tensor* r1, const fce_tensor& h, int h_store,
              const fce_tensor& x2, const fce_tensor* r2, const fce_tensor& y, const fce_tensor* dup, int dup_lo,
              hipStream_t s);
// preprocess.hip
int letterbox(const fce_letterbox_img* imgs, int n, uint8_t* dst, int H, int W, int pad, hipStream_t s);
int scale_boxes(float* dets, const int32_t* counts, int n, int max_det, const fce_box_scale* sc, hipStream_t s);
// tta.hip
int tta_scale_img(const fce_tensor& x, const fce_tensor& y, int flip, int hs, int ws, float pad, hipStream_t s);
int tta_merge(const fce_tta_part* parts, int nparts, int batch, int rows, float* pred, unsigned long long* best,
              hipStream_t s);
// val.hip
size_t val_match_ws_bytes(int n, int max_det, int max_gt_total, int niou);
int val_match(const float* dets, const int32_t* counts, int n, int max_det, const float* gt_boxes, const float* gt_cls,
              const int32_t* gt_off, const float* iouv, int niou, void* ws, size_t ws_bytes, uint16_t* tp,
              hipStream_t s);
size_t val_confusion_ws_bytes(int n, int max_det);
int val_confusion(const float* dets, const int32_t* counts, int n, int max_det, const float* gt_boxes,
                  const float* gt_cls, const int32_t* gt_off, int nc, float conf, float iou_thres, void* ws,
                  size_t ws_bytes, int32_t* matrix, hipStream_t s);

}  // namespace fce

// a C-ABI function's body: no exception crosses the ABI
#define FCE_GUARD(...)                                                          \
  try {                                                                         \
    __VA_ARGS__                                                                 \
  } catch (const std::exception& e) {                                           \
    return ::fce::fail(FCE_ERR_INVALID, std::string("exception: ") + e.what()); \
  } catch (...) {                                                               \
    return ::fce::fail(FCE_ERR_INVALID, "unknown exception");                   \
  }
