// The native whole-graph executor (fce_net): its buffers, its op list and the one table that describes an op kind.
//
// The executor restates BaseModel._predict_once (reference ultralytics/nn/tasks.py:160-188) as a
// flat list of kernel launches over an NHWC fp16 arena whose buffers are planned once per
// (batch, H, W): every layer output, every C2f/C3/SPPF/C2PSA concat buffer and the fp32 Detect
// maps live at fixed offsets, so one forward is a fixed launch sequence that is captured into a
// hipGraph and replayed (AutoBackend.forward / warmup, nn/autobackend.py:667-700, :912-926).
//
// net_build.hip records the ops (fce_net_add_*), net_plan.hip places the buffers, picks the forms and variants and
// holds the cost model, net_run.hip launches the ops (one stream, the op DAG over several, or a captured graph).
#pragma once
#include <vector>

#include "ops.h"

namespace fce {

enum OpKind { OP_CONV, OP_MAXPOOL, OP_WADD, OP_COORD, OP_PSA, OP_DETECT, OP_CONV_DETECT, OP_C3K2, OP_DCLS, OP_STEM2, OP_BNECK, OP_PW2 };

struct BufDesc {
  int c, shift, dtype;
  size_t offset = 0, bytes = 0;
};

// One recorded op (trivially copyable: the plan and the autotuner probe copies).  Every kind reads channels
// [in_coff, +in_c) of buffer `in` (-1: the network input), adds `res` over the output's channels and writes
// [out_coff, +out_c) of `out` (-1: none) and the duplicate store; what a kind touches beyond that is its
// OpKindInfo::extra.
struct OpDesc {
  OpKind kind;
  int in = -1, in_coff = 0, in_c = 0;
  int out = -1, out_coff = 0, out_c = 0;  // these seven first: make_op (net_build.hip) fills them positionally
  int res = -1, res_coff = 0;
  fce_conv_desc conv{};
  fce_coord_desc coord{};
  int coord_kind = 0;
  const void* w = nullptr;
  const float* b = nullptr;
  int k = 0, up = 0, accumulate = 0;
  const float* fw = nullptr;
  int fn = 0, fi = 0;
  int heads = 0, key_dim = 0, head_dim = 0;
  const float* pe_w = nullptr;
  const float* pe_b = nullptr;
  int nl = 0;
  int box[4] = {0, 0, 0, 0}, cls[4] = {0, 0, 0, 0};
  float strides[4] = {0, 0, 0, 0};
  int reg_max = 16;
  int part = 0, level = 0, nc = 0;  // OP_CONV_DETECT, OP_DCLS (part 1)
  fce_c3k2_desc c3k2{};              // OP_C3K2
  fce_dcls_desc dcls{};              // OP_DCLS
  fce_stem2_desc stem2{};            // OP_STEM2
  fce_bneck_desc bneck{};            // OP_BNECK
  fce_pw2_desc pw2{};                // OP_PW2: op 1 = in / res / out (h), op 2 = in2 / res2 / out2 / dup
  int in2 = -1, in2_coff = 0, res2 = -1, res2_coff = 0, out2 = -1, out2_coff = 0, h_store = 1;
  int tile = -1;                     // dense conv register tile (autotuned at plan), -1 = heuristic
  int dup = -1, dup_lo = 0, dup_c = 0;  // duplicate store of the last conv's out channels [dup_lo, +dup_c) into buffer dup
  // alternative forms: a fused op added by fce_net_add_*_alt computes the same output as ops
  // [alt_first, alt_first + alt_n) (the C3k2's four convs, the Detect cls branch's five ops, ...); exactly one form
  // runs, the other's ops are skipped (plan-time choice)
  int alt_first = -1, alt_n = 0;
  bool alt_locked = false;  // the alternative cannot run in this net (fce_net_plan found a reason): the ops it replaces run
  bool skip = false;
};

// ---- what an op touches, for the stream scheduler and the plan's "does anything else use this" questions
// Every op touches buffer channel ranges (reads / writes); two ops conflict when they touch
// overlapping ranges of the same buffer and at least one writes.  The coordinate-attention ops
// share the executor workspace (pseudo buffer WS); Detect tails write disjoint blocks of pred.
struct Access {
  int buf, c0, c1;
  bool write;
};
constexpr int kBufPred = -2, kBufWs = -3, kBufBest = -4;

}  // namespace fce

struct fce_net {
  std::vector<fce::BufDesc> bufs;
  std::vector<fce::OpDesc> ops;
  struct TuneRec {
    int op, code;
    float ms;
  };
  std::vector<TuneRec> tune_log;  // plan-time autotune measurements (fce_net_tune_record)
  int batch = 0, H = 0, W = 0;
  char* arena = nullptr;
  size_t arena_bytes = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  int anchors = 0, nc = 0;
  int level_off[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // captured forwards, one per (input, pred, stream, input dtype / channels): a double-buffered caller
  // (engine.Pipeline alternates two pred buffers) replays its graphs instead of recapturing
  struct Captured {
    hipGraph_t graph;
    hipGraphExec_t exec;
    const void* in;
    float* out;
    unsigned long long* best;
    hipStream_t stream;
    int dtype, c;
    unsigned long long used;
  };
  static constexpr int kMaxGraphs = 4;
  unsigned long long* cur_best = nullptr;  // best-class key output of the current forward (or null)
  // fork point: after op fork_op of a direct-launch forward, mid_ev is recorded on the forward's stream
  // (a side stream can start concurrent work -- the previous batch's NMS -- where the forward leaves
  // CUs idle); with graph replay, multiple streams or fork_op < 0 it is recorded at the end instead
  int fork_op = -1;
  hipEvent_t mid_ev = nullptr;
  std::vector<Captured> graphs;
  unsigned long long graph_clock = 0;
  // multi-stream capture: side streams + one event per op (+ fork), created on first capture
  std::vector<hipStream_t> side;
  std::vector<hipEvent_t> op_ev;
  hipEvent_t fork_ev = nullptr;
  hipStream_t own = nullptr;                   // capture/replay stream when the caller passes the null stream
  hipEvent_t join_ev[2] = {nullptr, nullptr};  // caller -> own, own -> caller

  void drop_streams() {
    for (hipEvent_t e : op_ev) (void)hipEventDestroy(e);
    op_ev.clear();
    if (fork_ev) (void)hipEventDestroy(fork_ev);
    fork_ev = nullptr;
    for (hipStream_t q : side) (void)hipStreamDestroy(q);
    side.clear();
    for (hipEvent_t& e : join_ev) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
    if (own) (void)hipStreamDestroy(own);
    own = nullptr;
  }

  static void destroy(Captured& c) {
    if (c.exec) (void)hipGraphExecDestroy(c.exec);
    if (c.graph) (void)hipGraphDestroy(c.graph);
  }
  void drop_graph() {  // every captured forward (the plan, a buffer or an op variant changed)
    for (Captured& c : graphs) destroy(c);
    graphs.clear();
  }
  void release() {
    drop_graph();
    if (arena) (void)hipFree(arena);
    if (ws) (void)hipFree(ws);
    arena = nullptr;
    ws = nullptr;
    arena_bytes = ws_bytes = 0;
  }
  ~fce_net() {
    release();
    drop_streams();
    if (mid_ev) (void)hipEventDestroy(mid_ev);
  }

  fce_tensor view(int id, int coff, int c) const {
    const fce::BufDesc& b = bufs[id];
    fce_tensor t{};
    t.data = arena + b.offset;
    t.dtype = b.dtype;
    t.layout = FCE_NHWC;
    t.n = batch;
    t.c = c;
    t.h = H >> b.shift;
    t.w = W >> b.shift;
    t.cstride = b.c;
    t.coff = coff;
    return t;
  }
};

namespace fce {

// ---- one row per op kind: everything the executor knows about a kind beyond the OpDesc fields every kind shares
// x / y: the views of the op's input and output ranges (y is empty where out < 0)
typedef int RunFn(fce_net* net, const OpDesc& op, const fce_tensor& x, const fce_tensor& y, float* pred, hipStream_t s);
// the op's profile name; its bytes moved and flops on the planned shapes are added to *bytes / *flops
typedef const char* CostFn(const fce_net* net, const OpDesc& op, double* bytes, double* flops);
typedef void AccessFn(const fce_net* net, const OpDesc& op, std::vector<Access>& a);
typedef bool FitsFn(const fce_net* net, const OpDesc& op);

RunFn run_conv, run_maxpool, run_wadd, run_coord, run_psa, run_detect, run_conv_detect, run_c3k2, run_dcls, run_stem2,
    run_bneck, run_pw2;  // net_run.hip
AccessFn acc_coord, acc_detect, acc_detect_tail, acc_pw2;  // net_run.hip
CostFn cost_conv, cost_maxpool, cost_wadd, cost_coord, cost_psa, cost_detect, cost_conv_detect, cost_c3k2, cost_dcls,
    cost_stem2, cost_bneck, cost_pw2;  // net_plan.hip
FitsFn fits_stem2, fits_bneck;         // net_plan.hip

struct OpKindInfo {
  RunFn* run;
  CostFn* cost;
  AccessFn* extra;       // accesses beyond the shared in / res / out / dup rule, or null
  const char* fuse_env;  // FCE_FUSE_* switch of a kind that is added as an alternative: "0" keeps the lowering from
                         // recording it, "1" keeps it fused without timing it (forced())
  FitsFn* fits;          // plan time: the fused kernel covers the planned shapes (null: always)
};
inline const OpKindInfo kOpKinds[] = {
    /* OP_CONV        */ {run_conv, cost_conv, nullptr, nullptr, nullptr},
    /* OP_MAXPOOL     */ {run_maxpool, cost_maxpool, nullptr, nullptr, nullptr},
    /* OP_WADD        */ {run_wadd, cost_wadd, nullptr, nullptr, nullptr},
    /* OP_COORD       */ {run_coord, cost_coord, acc_coord, nullptr, nullptr},
    /* OP_PSA         */ {run_psa, cost_psa, nullptr, nullptr, nullptr},
    /* OP_DETECT      */ {run_detect, cost_detect, acc_detect, nullptr, nullptr},
    /* OP_CONV_DETECT */ {run_conv_detect, cost_conv_detect, acc_detect_tail, nullptr, nullptr},
    /* OP_C3K2        */ {run_c3k2, cost_c3k2, nullptr, "FCE_FUSE_C3K2", nullptr},
    /* OP_DCLS        */ {run_dcls, cost_dcls, acc_detect_tail, "FCE_FUSE_DCLS", nullptr},
    /* OP_STEM2       */ {run_stem2, cost_stem2, nullptr, "FCE_FUSE_STEM", fits_stem2},
    /* OP_BNECK       */ {run_bneck, cost_bneck, nullptr, "FCE_FUSE_BNECK", fits_bneck},
    /* OP_PW2         */ {run_pw2, cost_pw2, acc_pw2, "FCE_FUSE_PW2", nullptr},
};
static_assert(sizeof(kOpKinds) / sizeof(kOpKinds[0]) == OP_PW2 + 1, "one row per OpKind, in enum order");

// ---- shared between the executor units
void set_alt_form(fce_net* net, OpDesc& op, bool fused);  // net_build.hip: the active form of an alternative
// net_run.hip
int run_op_impl(fce_net* net, const OpDesc& op, const fce_tensor& input, float* pred, hipStream_t s);  // skip ignored
void op_accesses(const fce_net* net, const OpDesc& op, std::vector<Access>& a);  // nothing for a skipped op

}  // namespace fce
