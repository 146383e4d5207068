// fce_net, running: one launch function per op kind, the access lists and the scheduler of the op DAG over several
// streams, the forward (direct launches or a captured hipGraph, cached per caller buffers) and the per-kernel profile.
#include <algorithm>

#include "net.h"

using namespace fce;

namespace fce {

// ---- one launch function per op kind (the run column of kOpKinds)
int run_conv(fce_net* net, const OpDesc& op, const fce_tensor& x, const fce_tensor& y, float*, hipStream_t s) {
  fce_tensor r, dv;
  if (op.res >= 0) r = net->view(op.res, op.res_coff, op.out_c);
  if (op.dup >= 0) dv = net->view(op.dup, 0, op.dup_c);
  return conv2d(op.conv, x, op.w, op.b, op.res >= 0 ? &r : nullptr, y, s, op.tile, op.dup >= 0 ? &dv : nullptr,
                op.dup_lo);
}
int run_maxpool(fce_net* net, const OpDesc& op, const fce_tensor& x, const fce_tensor&, float*, hipStream_t s) {
  const int c = op.in_c;  // the output range is three maps of c channels
  return maxpool_chain(x, net->view(op.out, op.out_coff, c), net->view(op.out, op.out_coff + c, c),
                       net->view(op.out, op.out_coff + 2 * c, c), op.k, s);
}
int run_wadd(fce_net*, const OpDesc& op, const fce_tensor& x, const fce_tensor& y, float*, hipStream_t s) {
  return weighted_add(x, op.up, op.fw, op.fn, op.fi, op.accumulate, y, s);
}
int run_coord(fce_net* net, const OpDesc& op, const fce_tensor& x, const fce_tensor& y, float*, hipStream_t s) {
  if (op.coord_kind == 0) return bicoordcrossatt(op.coord, x, y, net->ws, net->ws_bytes, s);
  if (op.coord_kind == 1) return coordatt(op.coord, x, y, net->ws, net->ws_bytes, s);
  return coordcrossatt(op.coord, x, y, net->ws, net->ws_bytes, s);
}
int run_psa(fce_net*, const OpDesc& op, const fce_tensor& x, const fce_tensor& y, float*, hipStream_t s) {
  return psa_attention(x, op.heads, op.key_dim, op.head_dim, op.pe_w, op.pe_b, y, s);
}
int run_c3k2(fce_net*, const OpDesc& op, const fce_tensor& x, const fce_tensor& y, float*, hipStream_t s) {
  return c3k2_fused(op.c3k2, x, y, s);
}
int run_stem2(fce_net*, const OpDesc& op, const fce_tensor& x, const fce_tensor& y, float*, hipStream_t s) {
  return stem_fused(op.stem2, x, y, s);
}
int run_bneck(fce_net*, const OpDesc& op, const fce_tensor& x, const fce_tensor& y, float*, hipStream_t s) {
  return bneck_fused(op.bneck, x, y, s);
}
int run_pw2(fce_net* net, const OpDesc& op, const fce_tensor& x, const fce_tensor& h, float*, hipStream_t s) {
  const fce_pw2_desc& d = op.pw2;
  const fce_tensor x2 = net->view(op.in2, op.in2_coff, d.cin2);
  const fce_tensor y = net->view(op.out2, op.out2_coff, d.cout2);
  fce_tensor r1{}, r2{}, dv{};
  if (op.res >= 0) r1 = net->view(op.res, op.res_coff, d.cout1);
  if (op.res2 >= 0) r2 = net->view(op.res2, op.res2_coff, d.cout2);
  if (op.dup >= 0) dv = net->view(op.dup, 0, op.dup_c);
  return pw2_fused(d, x, op.res >= 0 ? &r1 : nullptr, h, op.h_store, x2, op.res2 >= 0 ? &r2 : nullptr, y,
                   op.dup >= 0 ? &dv : nullptr, op.dup_lo, s);
}
static fce_detect_epi detect_epi(const fce_net* net, const OpDesc& op, float* pred) {
  return {pred, net->anchors, net->level_off[op.level], op.nc, op.reg_max, op.part, op.strides[0], net->cur_best};
}
int run_conv_detect(fce_net* net, const OpDesc& op, const fce_tensor& x, const fce_tensor&, float* pred, hipStream_t s) {
  return conv2d_detect(op.conv, x, op.w, op.b, detect_epi(net, op, pred), s, op.tile);
}
int run_dcls(fce_net* net, const OpDesc& op, const fce_tensor& x, const fce_tensor&, float* pred, hipStream_t s) {
  return detect_cls_fused(op.dcls, x, detect_epi(net, op, pred), s);
}
int run_detect(fce_net* net, const OpDesc& op, const fce_tensor&, const fce_tensor&, float* pred, hipStream_t s) {
  fce_tensor bx[4], cl[4];
  for (int i = 0; i < op.nl; ++i) {
    const int c = net->bufs[op.box[i]].c;
    bx[i] = net->view(op.box[i], 0, 4 * op.reg_max);
    cl[i] = net->view(op.cls[i], 4 * op.reg_max, c - 4 * op.reg_max);
  }
  return detect_decode(bx, cl, op.nl, op.strides, op.reg_max, pred, s);
}

int run_op_impl(fce_net* net, const OpDesc& op, const fce_tensor& input, float* pred, hipStream_t s) {
  const fce_tensor x = op.in >= 0 ? net->view(op.in, op.in_coff, op.in_c) : input;
  const fce_tensor y = op.out >= 0 ? net->view(op.out, op.out_coff, op.out_c) : fce_tensor{};
  return kOpKinds[op.kind].run(net, op, x, y, pred, s);
}

// ---- what the kinds touch beyond in / res / out / dup (the extra column of kOpKinds)
void acc_coord(const fce_net*, const OpDesc&, std::vector<Access>& a) { a.push_back({kBufWs, 0, 1, true}); }
void acc_detect_tail(const fce_net*, const OpDesc& op, std::vector<Access>& a) {
  a.push_back({kBufPred, 2 * op.level + op.part, 2 * op.level + op.part + 1, true});
  a.push_back({kBufBest, op.level, op.level + 1, true});  // box zeroes, cls maxes: keep them ordered
}
void acc_detect(const fce_net* net, const OpDesc& op, std::vector<Access>& a) {
  for (int i = 0; i < op.nl; ++i) a.push_back({op.box[i], 0, net->bufs[op.box[i]].c, false});
  a.push_back({kBufPred, 0, 1 << 20, true});
}
void acc_pw2(const fce_net*, const OpDesc& op, std::vector<Access>& a) {
  if (op.pw2.epi1 == FCE_EPI_ACCUM) a.push_back({op.out, op.out_coff, op.out_coff + op.out_c, false});
  a.push_back({op.in2, op.in2_coff, op.in2_coff + op.pw2.cin2, false});
  if (op.res2 >= 0) a.push_back({op.res2, op.res2_coff, op.res2_coff + op.pw2.cout2, false});
  a.push_back({op.out2, op.out2_coff, op.out2_coff + op.pw2.cout2, true});
}

void op_accesses(const fce_net* net, const OpDesc& op, std::vector<Access>& a) {
  a.clear();
  if (op.skip) return;
  if (op.in >= 0) a.push_back({op.in, op.in_coff, op.in_coff + op.in_c, false});
  if (op.res >= 0) a.push_back({op.res, op.res_coff, op.res_coff + op.out_c, false});
  if (op.out >= 0) a.push_back({op.out, op.out_coff, op.out_coff + op.out_c, true});
  if (op.dup >= 0) a.push_back({op.dup, 0, op.dup_c, true});
  if (AccessFn* extra = kOpKinds[op.kind].extra) extra(net, op, a);
}

}  // namespace fce

namespace {

// an op of the inactive form of an alternative launches nothing
int run_op(fce_net* net, const OpDesc& op, const fce_tensor& input, float* pred, hipStream_t s) {
  return op.skip ? FCE_OK : run_op_impl(net, op, input, pred, s);
}

int run_all(fce_net* net, const fce_tensor& input, float* pred, hipStream_t s, bool fork = false) {
  for (size_t i = 0; i < net->ops.size(); ++i) {
    int st = run_op(net, net->ops[i], input, pred, s);
    if (st) return st;
    if (fork && int(i) == net->fork_op) FCE_HIP_CHECK(hipEventRecord(net->mid_ev, s));
  }
  return FCE_OK;
}

// ---- the op DAG over several streams: two ops conflict when they touch overlapping ranges of one buffer and at least
// one writes (Access, net.h)
bool conflict(const std::vector<Access>& x, const std::vector<Access>& y) {
  for (const Access& p : x)
    for (const Access& q : y)
      if (p.buf == q.buf && (p.write || q.write) && p.c0 < q.c1 && q.c0 < p.c1) return true;
  return false;
}

// Scheduling of the op DAG onto the net's streams: an op goes to the stream of its most recent
// dependency when that stream has not moved on, otherwise to the stream idle longest, and waits
// (hipStreamWaitEvent) on every dependency recorded on another stream, so independent branches (the
// Detect levels / box and cls chains, the P3 head against the neck's P4/P5 path) run concurrently.
// Launched directly: multi-stream stream capture crashed the ROCm 7 runtime here (4 streams), and a
// captured linear graph replays slower than direct launches (measured).
int run_all_streams(fce_net* net, const fce_tensor& input, float* pred, hipStream_t s, int nstreams) {
  const int nops = int(net->ops.size());
  while (int(net->side.size()) < nstreams) {
    hipStream_t q = nullptr;
    FCE_HIP_CHECK(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
    net->side.push_back(q);
  }
  while (int(net->op_ev.size()) < nops) {
    hipEvent_t e = nullptr;
    FCE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    net->op_ev.push_back(e);
  }
  if (!net->fork_ev) FCE_HIP_CHECK(hipEventCreateWithFlags(&net->fork_ev, hipEventDisableTiming));
  std::vector<hipStream_t> st(net->side.begin(), net->side.begin() + nstreams);
  FCE_HIP_CHECK(hipEventRecord(net->fork_ev, s));
  for (int k = 0; k < nstreams; ++k) FCE_HIP_CHECK(hipStreamWaitEvent(st[k], net->fork_ev, 0));
  std::vector<std::vector<Access>> acc(nops);
  for (int j = 0; j < nops; ++j) op_accesses(net, net->ops[j], acc[j]);
  std::vector<int> stream_of(nops, 0), last_on(nstreams, -1);
  std::vector<int> deps;
  for (int j = 0; j < nops; ++j) {
    deps.clear();
    for (int i = 0; i < j; ++i)
      if (conflict(acc[i], acc[j])) deps.push_back(i);
    int pick = -1;
    for (int t = int(deps.size()) - 1; t >= 0 && pick < 0; --t) {
      const int k = stream_of[deps[t]];
      if (last_on[k] == deps[t]) pick = k;  // continue the chain on its own stream
    }
    if (pick < 0) {  // the stream whose last op is oldest
      pick = 0;
      for (int k = 1; k < nstreams; ++k)
        if (last_on[k] < last_on[pick]) pick = k;
    }
    for (int i : deps)
      if (stream_of[i] != pick || i > last_on[pick]) FCE_HIP_CHECK(hipStreamWaitEvent(st[pick], net->op_ev[i], 0));
    const int rc = run_op(net, net->ops[j], input, pred, st[pick]);
    if (rc) return rc;
    FCE_HIP_CHECK(hipEventRecord(net->op_ev[j], st[pick]));
    stream_of[j] = pick;
    last_on[pick] = j;
  }
  for (int k = 0; k < nstreams; ++k)
    if (last_on[k] >= 0) FCE_HIP_CHECK(hipStreamWaitEvent(s, net->op_ev[last_on[k]], 0));
  return FCE_OK;
}

int check_input(const fce_net* net, const fce_tensor* in) {
  FCE_CHECK(net->arena, "fce_net: call fce_net_plan first");
  FCE_CHECK(in && in->layout == FCE_NCHW && in->n == net->batch && in->h == net->H && in->w == net->W,
            "fce_net: input must be NCHW with the planned batch/size");
  return FCE_OK;
}

int forward_best(fce_net* net, const fce_tensor* input, float* pred, unsigned long long* best, int graph,
                        void* stream) {
  int st = check_input(net, input);
  if (st) return st;
  hipStream_t caller = S(stream);
  FCE_GUARD({
    if (!graph) {
      // direct launches on the caller's stream (measured fastest: 1.865 ms vs 1.944 ms for the
      // captured graph and 2.24-2.30 ms for the DAG over 2-4 streams, n-fce 640 bs32); FCE_STREAMS > 1
      // spreads the op DAG over that many net-owned streams
      const char* ns = getenv("FCE_STREAMS");
      const int nstreams = std::max(1, std::min(8, ns ? atoi(ns) : 1));
      const bool mid = net->mid_ev && net->fork_op >= 0 && nstreams == 1;
      st = nstreams == 1 ? run_all(net, *input, pred, caller, mid) : run_all_streams(net, *input, pred, caller, nstreams);
      if (!st && net->mid_ev && !mid) FCE_HIP_CHECK(hipEventRecord(net->mid_ev, caller));
      return st;
    }
    // hipGraph: one linear capture (the legacy null stream cannot be captured, so the net then
    // captures and replays on a stream of its own, ordered against the caller's with events)
    hipStream_t s = caller;
    if (!net->join_ev[0]) {
      FCE_HIP_CHECK(hipEventCreateWithFlags(&net->join_ev[0], hipEventDisableTiming));
      FCE_HIP_CHECK(hipEventCreateWithFlags(&net->join_ev[1], hipEventDisableTiming));
    }
    if (s == nullptr) {
      if (!net->own) FCE_HIP_CHECK(hipStreamCreateWithFlags(&net->own, hipStreamNonBlocking));
      s = net->own;
      FCE_HIP_CHECK(hipEventRecord(net->join_ev[0], caller));
      FCE_HIP_CHECK(hipStreamWaitEvent(s, net->join_ev[0], 0));
    }
    fce_net::Captured* hit = nullptr;
    for (fce_net::Captured& c : net->graphs)
      if (c.in == input->data && c.out == pred && c.best == best && c.stream == s && c.dtype == input->dtype &&
          c.c == input->c)
        hit = &c;
    if (!hit) {
      if (int(net->graphs.size()) >= fce_net::kMaxGraphs) {  // evict the least recently replayed
        auto lru = std::min_element(net->graphs.begin(), net->graphs.end(),
                                    [](const fce_net::Captured& a, const fce_net::Captured& b) { return a.used < b.used; });
        fce_net::destroy(*lru);
        net->graphs.erase(lru);
      }
      FCE_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      st = run_all(net, *input, pred, s);
      hipGraph_t g = nullptr;
      hipError_t e = hipStreamEndCapture(s, &g);
      if (st) {
        if (g) (void)hipGraphDestroy(g);
        return st;
      }
      FCE_HIP_CHECK(e);
      hipGraphExec_t x = nullptr;
      if (hipGraphInstantiate(&x, g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGraphDestroy(g);
        return fail(FCE_ERR_HIP, "fce_net_forward: hipGraphInstantiate failed");
      }
      net->graphs.push_back({g, x, input->data, pred, best, s, input->dtype, input->c, 0});
      hit = &net->graphs.back();
    }
    hit->used = ++net->graph_clock;
    FCE_HIP_CHECK(hipGraphLaunch(hit->exec, s));
    if (net->mid_ev) FCE_HIP_CHECK(hipEventRecord(net->mid_ev, s));
    if (s != caller) {
      FCE_HIP_CHECK(hipEventRecord(net->join_ev[1], s));
      FCE_HIP_CHECK(hipStreamWaitEvent(caller, net->join_ev[1], 0));
    }
    return FCE_OK;
  })
}

}  // namespace

extern "C" {

int fce_net_fork_hint(const fce_net* net) {
  // the op after which the forward runs at its coarsest resolution (stride 32): from there on the
  // forward's kernels are small and leave most CUs idle
  if (!net) return -1;
  int best = -1, shift = -1;
  for (size_t i = 0; i < net->ops.size(); ++i) {
    const OpDesc& op = net->ops[i];
    if (op.kind == OP_CONV && op.out >= 0 && net->bufs[op.out].shift > shift) {
      shift = net->bufs[op.out].shift;
      best = int(i);
    }
  }
  return best;
}

int fce_net_set_fork(fce_net* net, int op) {
  FCE_CHECK(net && op >= -1 && op < int(net->ops.size()), "fce_net_set_fork: bad op");
  if (!net->mid_ev) FCE_HIP_CHECK(hipEventCreateWithFlags(&net->mid_ev, hipEventDisableTiming));
  net->fork_op = op;
  net->drop_graph();
  return FCE_OK;
}

int fce_net_wait_fork(fce_net* net, void* stream) {
  FCE_CHECK(net && net->mid_ev, "fce_net_wait_fork: call fce_net_set_fork first");
  FCE_HIP_CHECK(hipStreamWaitEvent(S(stream), net->mid_ev, 0));
  return FCE_OK;
}

int fce_net_forward(fce_net* net, const fce_tensor* input, float* pred, int graph, void* stream) {
  return fce_net_forward_best(net, input, pred, nullptr, graph, stream);
}

int fce_net_forward_best(fce_net* net, const fce_tensor* input, float* pred, unsigned long long* best, int graph,
                         void* stream) {
  FCE_CHECK(net && pred, "fce_net_forward: null argument");
  // the Detect epilogues read cur_best while this call enqueues (captured graphs hold it by value); it is
  // cleared afterwards so a later profile / autotune pass can never write into a caller's key buffer
  net->cur_best = best;
  const int st = forward_best(net, input, pred, best, graph, stream);
  net->cur_best = nullptr;
  return st;
}

int fce_net_profile(fce_net* net, const fce_tensor* input, float* pred, float* ms, int* launches, int cap,
                    void* stream) {
  FCE_CHECK(net && pred && ms, "fce_net_profile: null argument");
  net->cur_best = nullptr;  // no best-class keys: the Detect epilogues write pred only
  int st = check_input(net, input);
  if (st) return st;
  hipStream_t s = S(stream);
  FCE_GUARD({
    // every kernel of every op carries its own (start, stop) event pair (hipExtLaunchKernelGGL): an
    // op's time is the sum of its kernels' execution intervals, the quantity rocprofv3 reports
    constexpr int kPerOp = 16;
    const int nops = int(net->ops.size());
    std::vector<hipEvent_t> ev(size_t(nops) * kPerOp * 2, nullptr);
    std::vector<int> used(nops, 0);
    auto destroy = [&]() {
      for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
    };
    for (auto& e : ev) {
      if (hipEventCreate(&e) != hipSuccess) {
        destroy();
        return fail(FCE_ERR_HIP, "fce_net_profile: hipEventCreate failed");
      }
    }
    for (int i = 0; i < nops && !st; ++i) {
      LaunchProbe probe{ev.data() + size_t(i) * kPerOp * 2, kPerOp, 0};
      probe_slot() = &probe;
      st = run_op(net, net->ops[i], *input, pred, s);
      probe_slot() = nullptr;
      used[i] = probe.n;
    }
    if (!st && hipStreamSynchronize(s) != hipSuccess) st = fail(FCE_ERR_HIP, "fce_net_profile: sync failed");
    for (int i = 0; i < nops && i < cap && !st; ++i) {
      float tot = 0.f;
      for (int k = 0; k < used[i]; ++k) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, ev[(size_t(i) * kPerOp + k) * 2], ev[(size_t(i) * kPerOp + k) * 2 + 1]) !=
            hipSuccess) {
          st = fail(FCE_ERR_HIP, "fce_net_profile: hipEventElapsedTime failed");
          break;
        }
        tot += t;
      }
      ms[i] = tot;
      if (launches) launches[i] = used[i];
    }
    destroy();
    return st;
  })
}

int fce_net_buffer(const fce_net* net, int id, fce_tensor* out) {
  FCE_CHECK(net && out && id >= 0 && id < int(net->bufs.size()) && net->arena, "fce_net_buffer: bad argument");
  *out = net->view(id, 0, net->bufs[id].c);
  return FCE_OK;
}

}  // extern "C"
