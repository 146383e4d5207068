// fce_net, planning: buffer placement per (batch, H, W), which alternatives can run (fit predicates, who else touches
// their buffers), the plan-time autotune of conv variants and alternative forms, and the cost model behind
// fce_net_op_info.
#include <algorithm>

#include "net.h"

using namespace fce;

namespace fce {

// ---- cost model (the cost column of kOpKinds): bytes moved and flops of one op on the planned shapes
static double map_px(const fce_net* net, int id) {  // pixels of one image's map in buffer id
  return double(net->H >> net->bufs[id].shift) * double(net->W >> net->bufs[id].shift);
}
static double in_px(const fce_net* net, const OpDesc& op) { return net->batch * map_px(net, op.in); }
static double wbytes(int cin, int cout, int k, int groups) {  // packed weights of one conv
  fce_conv_desc d{};
  d.cin = cin;
  d.cout = cout;
  d.k = k;
  d.groups = groups;
  return double(conv_weight_bytes(d));
}

const char* cost_conv(const fce_net* net, const OpDesc& op, double* bytes, double* flops) {
  const fce_conv_desc& d = op.conv;
  const double N = net->batch, ohw = map_px(net, op.out);
  const double ihw = op.in >= 0 ? map_px(net, op.in) : double(net->H) * net->W;  // f16 network input in the bench
  const bool dw = d.groups > 1;
  const bool stem = !dw && d.cin <= 4;
  const int osz = net->bufs[op.out].dtype == FCE_F32 ? 4 : 2;
  *bytes = N * ihw * d.cin * 2 + N * ohw * d.cout * osz + double(conv_weight_bytes(d));
  if (op.res >= 0) *bytes += N * ohw * d.cout * 2;
  if (op.dup >= 0) *bytes += N * ohw * op.dup_c * 2;
  if (d.epilogue == FCE_EPI_ACCUM) *bytes += N * ohw * d.cout * 2;
  *flops = 2.0 * N * ohw * d.cout * d.k * d.k * (dw ? 1 : d.cin);
  return stem ? "conv_stem" : dw ? "dwconv3x3" : (d.k == 3 ? "conv3x3_mfma" : "conv1x1_mfma");
}
const char* cost_conv_detect(const fce_net* net, const OpDesc& op, double* bytes, double* flops) {
  const fce_conv_desc& d = op.conv;
  const double px = in_px(net, op);
  *bytes = px * d.cin * 2 + px * (op.part == 0 ? 4 : d.cout) * 4 + double(conv_weight_bytes(d));
  *flops = 2.0 * px * d.cout * d.cin;
  return op.part == 0 ? "conv1x1_detect_box" : "conv1x1_detect_cls";
}
const char* cost_maxpool(const fce_net* net, const OpDesc& op, double* bytes, double*) {
  *bytes = in_px(net, op) * op.in_c * 2 * 4;
  return "maxpool_chain";
}
const char* cost_wadd(const fce_net* net, const OpDesc& op, double* bytes, double*) {
  *bytes = net->batch * map_px(net, op.out) * op.in_c * 2 * (op.accumulate ? 3 : 2) / (op.up ? 1.6 : 1.0);
  return "bifpn_weighted_add";
}
const char* cost_coord(const fce_net* net, const OpDesc& op, double* bytes, double* flops) {
  static const char* const nm[3] = {"bicoordcrossatt", "coordatt", "coordcrossatt"};
  const double px = in_px(net, op);
  *bytes = px * op.coord.inp * 2 * 2 + px * op.coord.oup * 2;  // 2 reads (pool, gate) + 1 write
  const double L = double(net->H >> net->bufs[op.in].shift) + double(net->W >> net->bufs[op.in].shift);
  *flops = 2.0 * net->batch * (3.0 * op.coord.mid * op.coord.inp * L + op.coord.oup * op.coord.mid * L);
  return nm[op.coord_kind];
}
// one read of the f16 input, one write of the second conv's output, both convs' weights
const char* cost_stem2(const fce_net* net, const OpDesc& op, double* bytes, double* flops) {
  const fce_stem2_desc& d = op.stem2;
  const double N = net->batch, ohw = map_px(net, op.out), ihw = double(net->H) * net->W;
  *bytes = N * ihw * 3 * 2 + N * ohw * d.c1 * 2 + wbytes(3, d.c0, 3, 1) + wbytes(d.c0, d.c1, 3, 1);
  *flops = 2.0 * N * (ihw / 4.0 * d.c0 * 27.0 + ohw * d.c1 * 9.0 * d.c0);
  return "stem_fused";
}
// one read of x, one write of the fp32 scores, the five ops' weights
const char* cost_dcls(const fce_net* net, const OpDesc& op, double* bytes, double* flops) {
  const fce_dcls_desc& d = op.dcls;
  const double px = in_px(net, op);
  *bytes = px * d.c0 * 2 + px * d.nc * 4 + wbytes(d.c0, d.c0, 3, d.c0) + wbytes(d.c0, d.c3, 1, 1) +
           wbytes(d.c3, d.c3, 3, d.c3) + wbytes(d.c3, d.c3, 1, 1) + wbytes(d.c3, d.nc, 1, 1);
  *flops = 2.0 * px * (9.0 * d.c0 + double(d.c0) * d.c3 + 9.0 * d.c3 + double(d.c3) * d.c3 + double(d.c3) * d.nc);
  return "detect_cls_fused";
}
// x1, op 2's inputs that are not op 1's output, the residuals, y (+ h when stored), both weights
const char* cost_pw2(const fce_net* net, const OpDesc& op, double* bytes, double* flops) {
  const fce_pw2_desc& d = op.pw2;
  const double px = in_px(net, op);
  const int lo = std::max(op.in2_coff, op.out_coff), hi = std::min(op.in2_coff + d.cin2, op.out_coff + d.cout1);
  const int over = op.in2 == op.out ? std::max(0, hi - lo) : 0;
  *bytes = px * 2 * (d.cin1 + (d.cin2 - over) + d.cout2 + (op.h_store ? d.cout1 : 0) + (op.res >= 0 ? d.cout1 : 0) +
                     (d.epi1 == FCE_EPI_ACCUM ? d.cout1 : 0) +
                     (op.res2 >= 0 ? d.cout2 : 0) + (op.dup >= 0 ? op.dup_c : 0)) +
           wbytes(d.cin1, d.cout1, 1, 1) + wbytes(d.cin2, d.cout2, 1, 1);
  *flops = 2.0 * px * (double(d.cin1) * d.cout1 + double(d.cin2) * d.cout2);
  return "pw2_fused";
}
// one read of x, one write of y, the 2 n convs' weights
const char* cost_bneck(const fce_net* net, const OpDesc& op, double* bytes, double* flops) {
  const fce_bneck_desc& d = op.bneck;
  const double px = in_px(net, op);
  *bytes = px * d.c * 2 * 2 + d.n * (wbytes(d.c, d.c_mid, 3, 1) + wbytes(d.c_mid, d.c, 3, 1));
  *flops = 2.0 * px * d.n * (9.0 * d.c * d.c_mid + 9.0 * d.c_mid * d.c);
  return "bneck_fused";
}
// one read of x, one write of y, the four convs' weights
const char* cost_c3k2(const fce_net* net, const OpDesc& op, double* bytes, double* flops) {
  const fce_c3k2_desc& d = op.c3k2;
  const double px = in_px(net, op);
  *bytes = px * (d.cin + d.cout) * 2 + wbytes(d.cin, 2 * d.c, 1, 1) + wbytes(d.c, d.c_mid, 3, 1) +
           wbytes(d.c_mid, d.c, 3, 1) + wbytes(3 * d.c, d.cout, 1, 1);
  *flops = 2.0 * px * (d.cin * 2.0 * d.c + 9.0 * d.c * d.c_mid + 9.0 * d.c_mid * d.c + 3.0 * d.c * d.cout);
  return "c3k2_fused";
}
const char* cost_psa(const fce_net* net, const OpDesc& op, double* bytes, double* flops) {
  const double N = net->batch, t = map_px(net, op.in);
  *bytes = N * t * op.heads * (2 * op.key_dim + op.head_dim) * 2 + N * t * op.heads * op.head_dim * 2;
  *flops = 2.0 * N * op.heads * t * t * (op.key_dim + op.head_dim);
  return "psa_attention";
}
const char* cost_detect(const fce_net* net, const OpDesc& op, double* bytes, double*) {
  double a = 0;
  for (int i = 0; i < op.nl; ++i) a += map_px(net, op.box[i]);
  *bytes = net->batch * a * (4 * op.reg_max + net->nc) * 4 + net->batch * a * (4 + net->nc) * 4;
  return "detect_decode";
}

// ---- plan-time fit predicates (the fits column of kOpKinds)
bool fits_stem2(const fce_net* net, const OpDesc& op) { return stem_fused_fits(op.stem2, net->H, net->W); }
bool fits_bneck(const fce_net* net, const OpDesc& op) {
  const int sh = net->bufs[op.in].shift;
  return bneck_fused_fits(op.bneck, net->H >> sh, net->W >> sh);
}

}  // namespace fce

namespace {

// FCE_FUSE_<kind>=1: the kind's alternatives stay fused, untimed
bool forced(OpKind kind) {
  const char* var = kOpKinds[kind].fuse_env;
  const char* e = var ? getenv(var) : nullptr;
  return e && strcmp(e, "1") == 0;
}

// the conv ops with kernel variants to choose from (the stem on the network input has one kernel)
bool tunable(const OpDesc& op) { return (op.kind == OP_CONV && op.in >= 0) || op.kind == OP_CONV_DETECT; }
int op_candidates(const fce_net* net, const OpDesc& op, int* out, int cap) {
  if (!tunable(op)) return 0;
  return conv_tile_candidates(op.conv, op.kind == OP_CONV_DETECT && op.part == 0, net->W >> net->bufs[op.in].shift,
                              out, cap);
}

// Does any op other than op i and the ops it replaces touch (reads_only: read) channels [c0, c1) of buffer `buf`?
// The ops of every form count: each is probed with skip cleared.
bool touched_elsewhere(const fce_net* net, int i, int buf, int c0, int c1, bool reads_only) {
  const OpDesc& self = net->ops[i];
  std::vector<Access> acc;
  for (int j = 0; j < int(net->ops.size()); ++j) {
    if (j == i || (j >= self.alt_first && j < self.alt_first + self.alt_n)) continue;
    OpDesc probe = net->ops[j];
    probe.skip = false;
    op_accesses(net, probe, acc);
    for (const Access& x : acc)
      if (!(reads_only && x.write) && x.buf == buf && x.c0 < c1 && c0 < x.c1) return true;
  }
  return false;
}

// Plan-time tile autotuning: every dense conv is timed (on the planned shapes, arena contents) with
// each candidate register tile and keeps the fastest.  Small maps favour fewer, fuller tiles (L2
// traffic) over occupancy in ways a closed-form rule does not capture reliably.
int autotune(fce_net* net) {
  hipStream_t ts = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float* pred = nullptr;
  int st = FCE_OK;
  int nc = 0;
  for (const OpDesc& op : net->ops)
    if (op.kind == OP_CONV_DETECT) nc = std::max(nc, op.nc);
  // a dummy network input (f16 NCHW, zeros) for timing the alternatives that read it (the fused stem pair)
  void* tin = nullptr;
  bool need_in = false;
  for (const OpDesc& op : net->ops) need_in |= op.kind == OP_STEM2 && op.alt_first >= 0 && !op.alt_locked;
  auto cleanup = [&]() {
    if (tin) (void)hipFree(tin);
    if (pred) (void)hipFree(pred);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (ts) (void)hipStreamDestroy(ts);
  };
  if (hipStreamCreateWithFlags(&ts, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
      hipEventCreate(&e1) != hipSuccess ||
      (nc > 0 && hipMalloc(reinterpret_cast<void**>(&pred), size_t(net->batch) * (4 + nc) * std::max(net->anchors, 1) *
                                                                 sizeof(float)) != hipSuccess)) {
    cleanup();
    return fail(FCE_ERR_HIP, "fce_net_plan: autotune setup failed");
  }
  fce_tensor input{};
  if (need_in) {
    const size_t nb = size_t(net->batch) * 3 * net->H * net->W * sizeof(_Float16);
    if (hipMalloc(&tin, nb) != hipSuccess || hipMemset(tin, 0, nb) != hipSuccess) {
      cleanup();
      return fail(FCE_ERR_HIP, "fce_net_plan: autotune input allocation failed");
    }
    input = fce_tensor{tin, FCE_F16, FCE_NCHW, net->batch, 3, net->H, net->W, 3, 0};
  }
  // ms per launch of `launch` (which returns a status): two warm-up launches, then the best of two 3-launch windows
  // (one window alone let clock / co-tenant noise flip close picks)
  auto time_launches = [&](auto&& launch, float* ms) {
    int rc = FCE_OK;
    for (int r = 0; r < 2 && rc == FCE_OK; ++r) rc = launch();
    *ms = 1e30f;
    for (int t = 0; t < 2 && rc == FCE_OK; ++t) {
      (void)hipEventRecord(e0, ts);
      for (int r = 0; r < 3 && rc == FCE_OK; ++r) rc = launch();
      (void)hipEventRecord(e1, ts);
      if (hipEventSynchronize(e1) != hipSuccess) rc = fail(FCE_ERR_HIP, "fce_net_plan: autotune sync failed");
      float w = 0.f;
      (void)hipEventElapsedTime(&w, e0, e1);
      *ms = std::min(*ms, w / 3.f);
    }
    return rc;
  };
  for (size_t i = 0; i < net->ops.size() && st == FCE_OK; ++i) {
    OpDesc& op = net->ops[i];
    int cand[128];
    const int ncand = op_candidates(net, op, cand, 128);
    if (ncand <= 1) continue;
    float best_ms = 1e30f, ms;
    int best = -1;
    for (int c = 0; c < ncand && st == FCE_OK; ++c) {
      op.tile = cand[c];
      st = time_launches([&]() { return run_op_impl(net, op, input, pred, ts); }, &ms);
      if (st) break;
      net->tune_log.push_back({int(i), cand[c], ms});
      if (ms < best_ms) {
        best_ms = ms;
        best = cand[c];
      }
    }
    op.tile = best;
  }
  // alternative forms (fused C3k2 against its four tuned convs, fused Detect cls branch against its five tuned ops):
  // time both on the planned shapes, keep the faster (FCE_FUSE_C3K2=1 / FCE_FUSE_DCLS=1 keep the fused form without
  // timing).  Logged as codes 0xF01 (fused) / 0xF00 (the unfused ops).
  for (size_t i = 0; i < net->ops.size() && st == FCE_OK; ++i) {
    OpDesc& op = net->ops[i];
    if (op.alt_first < 0 || op.alt_locked || forced(op.kind)) continue;
    float t[2] = {1e30f, 1e30f};  // [convs, fused]
    for (int form = 0; form < 2 && st == FCE_OK; ++form) {
      auto run_form = [&]() {
        if (form == 1) return run_op_impl(net, op, input, pred, ts);
        for (int j = op.alt_first; j < op.alt_first + op.alt_n; ++j) {
          const int r = run_op_impl(net, net->ops[j], input, pred, ts);
          if (r) return r;
        }
        return FCE_OK;
      };
      st = time_launches(run_form, &t[form]);
      if (st == FCE_OK) net->tune_log.push_back({int(i), 0xF00 | form, t[form]});
    }
    if (st == FCE_OK) set_alt_form(net, op, t[1] <= t[0]);
  }
  if (hipStreamSynchronize(ts) != hipSuccess && st == FCE_OK) st = fail(FCE_ERR_HIP, "fce_net_plan: autotune failed");
  cleanup();
  return st;
}

}  // namespace

extern "C" {

int fce_net_plan(fce_net* net, int batch, int h, int w) {
  const char* at = getenv("FCE_AUTOTUNE");
  return fce_net_plan_ex(net, batch, h, w, (at && atoi(at) == 0) ? FCE_PLAN_NO_AUTOTUNE : 0);
}

int fce_net_plan_ex(fce_net* net, int batch, int h, int w, int flags) {
  FCE_CHECK(net && batch > 0 && h > 0 && w > 0, "fce_net_plan: bad argument");
  FCE_CHECK((flags & ~FCE_PLAN_NO_AUTOTUNE) == 0, "fce_net_plan_ex: unknown flags");
  FCE_CHECK(h % 32 == 0 && w % 32 == 0, "fce_net_plan: H and W must be multiples of 32 (max stride)");
  FCE_GUARD({
    net->release();
    net->tune_log.clear();
    net->batch = batch;
    net->H = h;
    net->W = w;
    size_t off = 0;
    for (BufDesc& b : net->bufs) {
      b.offset = off;
      b.bytes = size_t(batch) * (h >> b.shift) * (w >> b.shift) * b.c * dtype_size(b.dtype);
      off += (b.bytes + 255) & ~size_t(255);
    }
    net->arena_bytes = off;
    size_t ws = 256;
    int A = 0;
    for (const OpDesc& op : net->ops) {
      if (op.kind == OP_COORD)
        ws = std::max(ws, coord_ws_bytes(op.coord, batch, h >> net->bufs[op.in].shift, w >> net->bufs[op.in].shift));
      if (op.kind == OP_DETECT)
        for (int i = 0; i < op.nl; ++i) A += (h >> net->bufs[op.box[i]].shift) * (w >> net->bufs[op.box[i]].shift);
    }
    // fused Detect levels: anchor blocks in level order (head.py:155 torch.cat over levels)
    int lv_hw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, nlv = 0;
    for (const OpDesc& op : net->ops)
      if (op.kind == OP_CONV_DETECT && op.part == 0) {
        lv_hw[op.level] = (h >> net->bufs[op.in].shift) * (w >> net->bufs[op.in].shift);
        nlv = std::max(nlv, op.level + 1);
      }
    if (nlv) {
      A = 0;
      for (int i = 0; i < nlv; ++i) {
        net->level_off[i] = A;
        A += lv_hw[i];
      }
    }
    net->anchors = A;
    net->ws_bytes = ws;
    for (size_t i = 0; i < net->ops.size(); ++i) {
      OpDesc& op = net->ops[i];
      if (op.alt_first < 0) continue;
      if (op.kind == OP_PW2) {
        // a fused 1x1 pair stores op 1's output only when some other op reads it (the ops of every form count)
        op.h_store = touched_elsewhere(net, int(i), op.out, op.out_coff, op.out_coff + op.out_c, true);
        continue;
      }
      FitsFn* fits = kOpKinds[op.kind].fits;
      if (!fits) continue;
      // a fused stem pair runs only for the input sizes its kernel is built for, a fused Bottleneck chain only where
      // an instantiation covers its map width
      op.alt_locked = !fits(net, op);
      if (op.kind == OP_STEM2 && !op.alt_locked) {
        // it skips writing the stem's output: valid only when nothing but the second conv touches it
        const OpDesc& s0 = net->ops[op.alt_first];
        op.alt_locked = touched_elsewhere(net, int(i), s0.out, s0.out_coff, s0.out_coff + s0.out_c, false);
      }
      if (op.alt_locked) set_alt_form(net, op, false);
      else if (op.kind == OP_BNECK && forced(op.kind)) set_alt_form(net, op, true);
    }
    FCE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&net->arena), std::max<size_t>(off, 256)));
    FCE_HIP_CHECK(hipMalloc(&net->ws, ws));
    FCE_HIP_CHECK(hipMemset(net->arena, 0, std::max<size_t>(off, 256)));
    net->cur_best = nullptr;
    if (!(flags & FCE_PLAN_NO_AUTOTUNE)) return autotune(net);
    return FCE_OK;
  })
}

size_t fce_net_arena_bytes(const fce_net* net) { return net ? net->arena_bytes + net->ws_bytes : 0; }
int fce_net_num_anchors(const fce_net* net) { return net ? net->anchors : 0; }

int fce_net_op_info(const fce_net* net, int i, char* name, int cap, double* bytes, double* flops) {
  FCE_CHECK(net && i >= 0 && i < int(net->ops.size()) && bytes && flops, "fce_net_op_info: bad argument");
  const OpDesc& op = net->ops[i];
  *bytes = *flops = 0;
  const char* nm = kOpKinds[op.kind].cost(net, op, bytes, flops);
  // before fce_net_plan (no sizes yet), or the inactive form of an alternative: the op's name, no work
  if (net->batch <= 0 || op.skip) *bytes = *flops = 0;
  if (name && cap > 0) {
    size_t n = std::min(strlen(nm), size_t(cap - 1));
    memcpy(name, nm, n);
    name[n] = 0;
  }
  return FCE_OK;
}

int fce_net_op_variants(const fce_net* net, int i, int* codes, int cap) {
  if (!net || i < 0 || i >= int(net->ops.size()) || !codes || cap <= 0 || net->batch <= 0) return 0;
  return op_candidates(net, net->ops[i], codes, cap);
}

int fce_net_set_op_variant(fce_net* net, int i, int code) {
  FCE_CHECK(net && i >= 0 && i < int(net->ops.size()) && net->batch > 0, "fce_net_set_op_variant: bad argument");
  OpDesc& op = net->ops[i];
  FCE_CHECK(tunable(op), "fce_net_set_op_variant: not a conv op");
  if (code != -1) {
    int cand[128];
    const int nc = op_candidates(net, op, cand, 128);
    FCE_CHECK(std::find(cand, cand + nc, code) != cand + nc, "fce_net_set_op_variant: not a candidate of this op");
  }
  if (op.tile != code) net->drop_graph();  // captured forwards hold the old variant's launches
  op.tile = code;
  return FCE_OK;
}

int fce_net_tune_record(const fce_net* net, int k, int* op, int* code, float* ms) {
  if (!net || k < 0 || k >= int(net->tune_log.size())) return 0;
  if (op) *op = net->tune_log[k].op;
  if (code) *code = net->tune_log[k].code;
  if (ms) *ms = net->tune_log[k].ms;
  return 1;
}

}  // extern "C"
