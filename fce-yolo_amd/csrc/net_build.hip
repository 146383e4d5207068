// fce_net, recording: create / destroy, the buffers, one fce_net_add_* per op kind, the alternatives (a fused op
// recorded after the ops it can replace) and the getters / setters of an op's form.  Nothing here touches the GPU.
#include <algorithm>

#include "net.h"

using namespace fce;

namespace fce {

// the active form of an alternative: the fused op, or the ops it replaces
void set_alt_form(fce_net* net, OpDesc& op, bool fused) {
  if (op.skip != !fused) net->drop_graph();  // captured forwards hold the other form's launches
  op.skip = !fused;
  for (int j = op.alt_first; j < op.alt_first + op.alt_n; ++j) net->ops[j].skip = fused;
}

}  // namespace fce

namespace {

bool valid_buf(const fce_net* net, int id, bool allow_input) {
  return (allow_input && id == -1) || (id >= 0 && id < int(net->bufs.size()));
}

OpDesc make_op(OpKind kind, int in, int in_coff, int in_c, int out, int out_coff, int out_c) {
  return OpDesc{kind, in, in_coff, in_c, out, out_coff, out_c};
}

int push_op(fce_net* net, const OpDesc& op) {
  net->drop_graph();
  net->ops.push_back(op);
  return FCE_OK;
}

// ---- alternatives.  Every fce_net_add_*_alt first checks, with its own messages, that the ops it replaces are the
// last `nops` added (last_ops: only then may it look at them) and plain (plain_ops), then what its pattern needs.
bool last_ops(const fce_net* net, int first_op, int nops) {
  return net && nops >= 1 && first_op >= 0 && first_op + nops == int(net->ops.size());
}
// conv ops (the last one of kind `last`), none skipped, none an alternative itself
bool plain_ops(const fce_net* net, int first_op, int nops, OpKind last = OP_CONV) {
  for (int j = 0; j < nops; ++j) {
    const OpDesc& o = net->ops[first_op + j];
    if (o.kind != (j == nops - 1 ? last : OP_CONV) || o.skip || o.alt_first >= 0) return false;
  }
  return true;
}
// the fused op of ops [first_op, +nops): recorded, and selected until the plan (a fit predicate, the autotune) says
// otherwise
int push_alt(fce_net* net, OpDesc op, int first_op, int nops) {
  op.alt_first = first_op;
  op.alt_n = nops;
  push_op(net, op);
  set_alt_form(net, net->ops.back(), true);
  return FCE_OK;
}

// a fused C3k2, on its own (first_op < 0) or as the alternative of ops [first_op, +nops)
int add_c3k2(fce_net* net, const fce_c3k2_desc* d, int in, int in_coff, int out, int out_coff, int first_op, int nops) {
  FCE_CHECK(net && d && valid_buf(net, in, false) && valid_buf(net, out, false), "fce_net_add_c3k2: bad argument");
  FCE_CHECK(c3k2_fused_ok(*d), "fce_net_add_c3k2: unsupported channel configuration");
  OpDesc op = make_op(OP_C3K2, in, in_coff, d->cin, out, out_coff, d->cout);
  op.c3k2 = *d;
  return first_op < 0 ? push_op(net, op) : push_alt(net, op, first_op, nops);
}

}  // namespace

extern "C" {

fce_net* fce_net_create(void) {
  try {
    return new fce_net();
  } catch (...) {
    set_error("fce_net_create: allocation failed");
    return nullptr;
  }
}
void fce_net_destroy(fce_net* net) { delete net; }

int fce_net_num_ops(const fce_net* net) { return net ? int(net->ops.size()) : 0; }

int fce_net_add_buffer(fce_net* net, int c, int shift, int dtype) {
  FCE_CHECK(net && c > 0 && shift >= 0 && shift <= 8 && (dtype == FCE_F16 || dtype == FCE_F32),
            "fce_net_add_buffer: bad argument");
  net->drop_graph();
  net->bufs.push_back(BufDesc{c, shift, dtype});
  return int(net->bufs.size()) - 1;
}

static int add_conv(fce_net* net, const fce_conv_desc* d, int in, int in_coff, int out, int out_coff, int res,
                    int res_coff, const void* w, const float* b, int dup, int dup_lo, int dup_c) {
  FCE_CHECK(net && d && w && b, "fce_net_add_conv: null argument");
  FCE_CHECK(valid_buf(net, in, true) && valid_buf(net, out, false) && (res == -1 || valid_buf(net, res, false)),
            "fce_net_add_conv: bad buffer id");
  OpDesc op = make_op(OP_CONV, in, in_coff, d->cin, out, out_coff, d->cout);
  op.conv = *d;
  op.res = res;
  op.res_coff = res_coff;
  op.w = w;
  op.b = b;
  op.dup = dup;
  op.dup_lo = dup_lo;
  op.dup_c = dup_c;
  return push_op(net, op);
}

int fce_net_add_conv(fce_net* net, const fce_conv_desc* d, int in, int in_coff, int out, int out_coff, int res,
                     int res_coff, const void* w, const float* b) {
  return add_conv(net, d, in, in_coff, out, out_coff, res, res_coff, w, b, -1, 0, 0);
}

int fce_net_add_conv_dup(fce_net* net, const fce_conv_desc* d, int in, int in_coff, int out, int out_coff, int res,
                         int res_coff, const void* w, const float* b, int dup, int dup_lo, int dup_c) {
  FCE_CHECK(net && valid_buf(net, dup, false) && dup_c > 0 && dup_c % 8 == 0 && dup_lo >= 0 && dup_lo % 8 == 0 &&
                d && d->k == 1 && dup_lo + dup_c <= d->cout && net->bufs[dup].c == dup_c &&
                net->bufs[dup].dtype == FCE_F16,
            "fce_net_add_conv_dup: bad duplicate-store buffer or channel range");
  // every check before the op is added: a failed call leaves the op list unchanged
  FCE_CHECK(valid_buf(net, out, false) && net->bufs[dup].shift == net->bufs[out].shift,
            "fce_net_add_conv_dup: dup buffer size differs");
  return add_conv(net, d, in, in_coff, out, out_coff, res, res_coff, w, b, dup, dup_lo, dup_c);
}

int fce_net_add_maxpool_chain(fce_net* net, int buf, int in_coff, int c, int k) {
  FCE_CHECK(net && valid_buf(net, buf, false), "fce_net_add_maxpool_chain: bad buffer");
  // the three pooled maps follow the input in its buffer
  OpDesc op = make_op(OP_MAXPOOL, buf, in_coff, c, buf, in_coff + c, 3 * c);
  op.k = k;
  return push_op(net, op);
}

int fce_net_add_weighted_add(fce_net* net, int in, int in_coff, int c, int up, const float* fw, int fn, int fi,
                             int accumulate, int out, int out_coff) {
  FCE_CHECK(net && fw && valid_buf(net, in, false) && valid_buf(net, out, false), "fce_net_add_weighted_add: bad arg");
  OpDesc op = make_op(OP_WADD, in, in_coff, c, out, out_coff, c);
  op.up = up;
  op.fw = fw;
  op.fn = fn;
  op.fi = fi;
  op.accumulate = accumulate;
  return push_op(net, op);
}

int fce_net_add_coord(fce_net* net, int kind, const fce_coord_desc* d, int in, int in_coff, int out, int out_coff) {
  FCE_CHECK(net && d && kind >= 0 && kind <= 2 && valid_buf(net, in, false) && valid_buf(net, out, false),
            "fce_net_add_coord: bad argument");
  OpDesc op = make_op(OP_COORD, in, in_coff, d->inp, out, out_coff, d->oup);
  op.coord_kind = kind;
  op.coord = *d;
  return push_op(net, op);
}

int fce_net_add_psa_attention(fce_net* net, int qkv, int heads, int kd, int hd, const float* pe_w, const float* pe_b,
                              int out, int out_coff) {
  FCE_CHECK(net && pe_w && pe_b && valid_buf(net, qkv, false) && valid_buf(net, out, false),
            "fce_net_add_psa_attention: bad argument");
  OpDesc op = make_op(OP_PSA, qkv, 0, heads * (2 * kd + hd), out, out_coff, heads * hd);
  op.heads = heads;
  op.key_dim = kd;
  op.head_dim = hd;
  op.pe_w = pe_w;
  op.pe_b = pe_b;
  return push_op(net, op);
}

int fce_net_add_detect(fce_net* net, int nl, const int* maps, const float* strides, int reg_max) {
  FCE_CHECK(net && maps && strides && nl >= 1 && nl <= 4, "fce_net_add_detect: bad argument");
  OpDesc op = make_op(OP_DETECT, -1, 0, 0, -1, 0, 0);  // reads its maps, writes pred (acc_detect)
  op.nl = nl;
  for (int i = 0; i < nl; ++i) {
    FCE_CHECK(valid_buf(net, maps[i], false), "fce_net_add_detect: bad buffer");
    FCE_CHECK(net->bufs[maps[i]].dtype == FCE_F32 && net->bufs[maps[i]].c > 4 * reg_max, "detect maps must be f32");
    op.box[i] = maps[i];
    op.cls[i] = maps[i];
    op.strides[i] = strides[i];
  }
  op.reg_max = reg_max;
  net->nc = net->bufs[maps[0]].c - 4 * reg_max;
  return push_op(net, op);
}

int fce_net_add_conv_detect(fce_net* net, const fce_conv_desc* d, int in, int in_coff, int part, int level,
                            float stride, int nc, int reg_max, const void* w, const float* b) {
  FCE_CHECK(net && d && w && b && valid_buf(net, in, false), "fce_net_add_conv_detect: bad argument");
  FCE_CHECK(part == 0 || part == 1, "fce_net_add_conv_detect: part must be 0 (box) or 1 (cls)");
  FCE_CHECK(level >= 0 && level < 8, "fce_net_add_conv_detect: level out of range");
  OpDesc op = make_op(OP_CONV_DETECT, in, in_coff, d->cin, -1, 0, 0);  // writes its block of pred (acc_detect_tail)
  op.conv = *d;
  op.part = part;
  op.level = level;
  op.strides[0] = stride;
  op.nc = nc;
  op.reg_max = reg_max;
  op.w = w;
  op.b = b;
  net->nc = nc;
  return push_op(net, op);
}

int fce_net_add_c3k2(fce_net* net, const fce_c3k2_desc* d, int in, int in_coff, int out, int out_coff) {
  return add_c3k2(net, d, in, in_coff, out, out_coff, -1, 0);
}

int fce_net_add_c3k2_alt(fce_net* net, const fce_c3k2_desc* d, int in, int in_coff, int out, int out_coff,
                         int first_op, int nops) {
  FCE_CHECK(last_ops(net, first_op, nops), "fce_net_add_c3k2_alt: the alternative must be the last ops added");
  FCE_CHECK(plain_ops(net, first_op, nops), "fce_net_add_c3k2_alt: the alternative must be plain conv ops");
  return add_c3k2(net, d, in, in_coff, out, out_coff, first_op, nops);
}

int fce_net_add_bneck_alt(fce_net* net, const fce_bneck_desc* d, int in, int in_coff, int out, int out_coff,
                          int first_op, int nops) {
  FCE_CHECK(last_ops(net, first_op, nops) && d && valid_buf(net, in, false) && valid_buf(net, out, false) &&
                (d->n == 1 || d->n == 2) && nops == 2 * d->n,
            "fce_net_add_bneck_alt: the alternative must be the last 2 n ops added");
  FCE_CHECK(bneck_fused_ok(*d), "fce_net_add_bneck_alt: unsupported channel configuration");
  const OpDesc* o = &net->ops[first_op];
  for (int j = 0; j < nops; ++j) {
    const fce_conv_desc& c = o[j].conv;
    const bool odd = j % 2 == 1;
    FCE_CHECK(plain_ops(net, first_op + j, 1) && o[j].dup < 0 && c.k == 3 && c.stride == 1 && c.groups == 1 &&
                  c.up == 0 && c.act == FCE_ACT_SILU && c.epilogue == FCE_EPI_STORE &&
                  c.cin == (odd ? d->c_mid : d->c) && c.cout == (odd ? d->c : d->c_mid) && o[j].w == d->w[j] &&
                  o[j].b == d->b[j],
              "fce_net_add_bneck_alt: the ops are not this chain's 3x3 SiLU convs (shapes, weights or epilogues differ)");
    // chain: conv j reads conv j - 1's whole output (the first reads the input); every odd conv adds its
    // Bottleneck's input (the input of conv j - 1) as the residual; only the last writes the given output
    const int src = j == 0 ? in : o[j - 1].out, src_off = j == 0 ? in_coff : o[j - 1].out_coff;
    FCE_CHECK(o[j].in == src && o[j].in_coff == src_off, "fce_net_add_bneck_alt: the ops must form one chain");
    if (odd)
      FCE_CHECK(o[j].res == o[j - 1].in && o[j].res_coff == o[j - 1].in_coff,
                "fce_net_add_bneck_alt: every second conv must add its Bottleneck's input");
    else
      FCE_CHECK(o[j].res < 0, "fce_net_add_bneck_alt: the first conv of a Bottleneck has no residual");
  }
  FCE_CHECK(o[nops - 1].out == out && o[nops - 1].out_coff == out_coff,
            "fce_net_add_bneck_alt: the last conv must write the given output");
  OpDesc op = make_op(OP_BNECK, in, in_coff, d->c, out, out_coff, d->c);
  op.bneck = *d;
  return push_alt(net, op, first_op, nops);
}

int fce_net_add_pw2_alt(fce_net* net, const fce_pw2_desc* d, int first_op) {
  FCE_CHECK(last_ops(net, first_op, 2) && d, "fce_net_add_pw2_alt: the alternative must be the last two ops added");
  FCE_CHECK(pw2_fused_ok(*d), "fce_net_add_pw2_alt: unsupported channel configuration");
  const OpDesc& o1 = net->ops[first_op];
  const OpDesc& o2 = net->ops[first_op + 1];
  const int cins[2] = {d->cin1, d->cin2}, couts[2] = {d->cout1, d->cout2};
  for (int j = 0; j < 2; ++j) {
    const OpDesc& o = j ? o2 : o1;
    const fce_conv_desc& c = o.conv;
    FCE_CHECK(plain_ops(net, first_op + j, 1) && o.in >= 0 && c.k == 1 && c.stride == 1 && c.groups == 1 &&
                  c.up == 0 && c.epilogue == (j ? FCE_EPI_STORE : d->epi1) && c.act == d->act[j] &&
                  (j || d->epi1 == FCE_EPI_STORE ||
                   (c.fusion_w == d->fw && c.fusion_n == d->fn && c.fusion_i == d->fi)) &&
                  c.cin == cins[j] && c.cout == couts[j] && o.w == d->w[j] && o.b == d->b[j] &&
                  net->bufs[o.out].dtype == FCE_F16 && net->bufs[o.in].dtype == FCE_F16 &&
                  net->bufs[o.in].shift == net->bufs[o1.in].shift,
              "fce_net_add_pw2_alt: the two ops are not this pair's 1x1 convs (shapes, weights or epilogues differ)");
  }
  FCE_CHECK(o1.dup < 0, "fce_net_add_pw2_alt: op 1 has a duplicate store");
  const int lo = std::max(o2.in_coff, o1.out_coff), hi = std::min(o2.in_coff + d->cin2, o1.out_coff + d->cout1);
  FCE_CHECK(o2.in == o1.out && hi > lo, "fce_net_add_pw2_alt: op 2 must read channels of op 1's output buffer");
  OpDesc op = make_op(OP_PW2, o1.in, o1.in_coff, d->cin1, o1.out, o1.out_coff, d->cout1);
  op.pw2 = *d;
  op.res = o1.res;
  op.res_coff = o1.res_coff;
  op.in2 = o2.in;
  op.in2_coff = o2.in_coff;
  op.res2 = o2.res;
  op.res2_coff = o2.res_coff;
  op.out2 = o2.out;
  op.out2_coff = o2.out_coff;
  op.dup = o2.dup;
  op.dup_lo = o2.dup_lo;
  op.dup_c = o2.dup_c;
  op.h_store = 1;  // fce_net_plan clears it when nothing else reads h
  return push_alt(net, op, first_op, 2);
}

int fce_net_add_stem_alt(fce_net* net, const fce_stem2_desc* d, int first_op, int nops) {
  FCE_CHECK(last_ops(net, first_op, nops) && d && nops == 2,
            "fce_net_add_stem_alt: the alternative must be the last two ops added");
  FCE_CHECK(stem_fused_ok(*d), "fce_net_add_stem_alt: unsupported channel configuration");
  const OpDesc& s0 = net->ops[first_op];
  const OpDesc& s1 = net->ops[first_op + 1];
  const fce_conv_desc &c0 = s0.conv, &c1 = s1.conv;
  FCE_CHECK(plain_ops(net, first_op, nops), "fce_net_add_stem_alt: the alternative must be two conv ops");
  FCE_CHECK(s0.in == -1 && c0.cin == 3 && c0.cout == d->c0 && c0.k == 3 && c0.stride == 2 && c0.groups == 1 &&
                c0.act == FCE_ACT_SILU && c0.epilogue == FCE_EPI_STORE && s0.res < 0 && s0.dup < 0 && s0.w == d->w[0] &&
                s0.b == d->b[0],
            "fce_net_add_stem_alt: the first op must be the 3x3 stride-2 SiLU stem on the network input");
  FCE_CHECK(s1.in == s0.out && s1.in_coff == s0.out_coff && c1.cin == d->c0 && c1.cout == d->c1 && c1.k == 3 &&
                c1.stride == 2 && c1.groups == 1 && c1.up == 0 && c1.act == FCE_ACT_SILU &&
                c1.epilogue == FCE_EPI_STORE && s1.res < 0 && s1.dup < 0 && s1.w == d->w[1] && s1.b == d->b[1],
            "fce_net_add_stem_alt: the second op must be the 3x3 stride-2 SiLU conv of the stem's output");
  OpDesc op = make_op(OP_STEM2, -1, 0, 3, s1.out, s1.out_coff, d->c1);
  op.stem2 = *d;
  return push_alt(net, op, first_op, nops);
}

int fce_net_add_detect_cls_alt(fce_net* net, const fce_dcls_desc* d, int in, int in_coff, int first_op, int nops) {
  FCE_CHECK(last_ops(net, first_op, nops) && d && valid_buf(net, in, false) && nops == 5,
            "fce_net_add_detect_cls_alt: the alternative must be the last five ops added");
  FCE_CHECK(detect_cls_fused_ok(*d), "fce_net_add_detect_cls_alt: unsupported channel configuration");
  const OpDesc* o = &net->ops[first_op];
  FCE_CHECK(plain_ops(net, first_op, nops, OP_CONV_DETECT),
            "fce_net_add_detect_cls_alt: the alternative must be four conv ops and a conv-detect op");
  const int ks[5] = {3, 1, 3, 1, 1}, cin[5] = {d->c0, d->c0, d->c3, d->c3, d->c3};
  const int cout[5] = {d->c0, d->c3, d->c3, d->c3, d->nc};
  for (int j = 0; j < 5; ++j) {
    const fce_conv_desc& c = o[j].conv;
    FCE_CHECK(c.k == ks[j] && c.cin == cin[j] && c.cout == cout[j] && c.stride == 1 && c.up == 0 &&
                  c.groups == (ks[j] == 3 ? c.cin : 1) && c.act == (j < 4 ? FCE_ACT_SILU : FCE_ACT_NONE) &&
                  c.epilogue == FCE_EPI_STORE && o[j].w == d->w[j] && o[j].b == d->b[j],
              "fce_net_add_detect_cls_alt: the five ops are not this branch (shapes, activations or weights differ)");
  }
  // the chain: x -> dw1 -> pw1 -> dw2 -> pw2 -> cls, each reading the previous op's whole output
  FCE_CHECK(o[0].in == in && o[0].in_coff == in_coff && o[0].res < 0 && o[0].dup < 0,
            "fce_net_add_detect_cls_alt: the first op must read the given input");
  for (int j = 1; j < 5; ++j)
    FCE_CHECK(o[j].in == o[j - 1].out && o[j].in_coff == o[j - 1].out_coff && o[j].res < 0 && o[j].dup < 0,
              "fce_net_add_detect_cls_alt: the five ops must form one chain");
  FCE_CHECK(o[4].part == 1 && o[4].nc == d->nc, "fce_net_add_detect_cls_alt: the last op must be the cls tail");
  OpDesc op = make_op(OP_DCLS, in, in_coff, d->c0, -1, 0, 0);  // writes the cls tail's block of pred
  op.dcls = *d;
  op.level = o[4].level;
  op.strides[0] = o[4].strides[0];
  op.nc = o[4].nc;
  op.reg_max = o[4].reg_max;
  op.part = 1;
  return push_alt(net, op, first_op, nops);
}

int fce_net_op_skipped(const fce_net* net, int i) {
  return net && i >= 0 && i < int(net->ops.size()) && net->ops[i].skip ? 1 : 0;
}

int fce_net_alt_form(const fce_net* net, int i) {
  if (!net || i < 0 || i >= int(net->ops.size())) return -1;
  const OpDesc& op = net->ops[i];
  return op.alt_first >= 0 ? (op.skip ? 0 : 1) : -1;
}

int fce_net_set_alt_form(fce_net* net, int i, int fused) {
  FCE_CHECK(fce_net_alt_form(net, i) >= 0, "fce_net_set_alt_form: not a fused op with an alternative");
  FCE_CHECK(!fused || !net->ops[i].alt_locked, "fce_net_set_alt_form: this fused op cannot run in this net");
  set_alt_form(net, net->ops[i], fused != 0);
  return FCE_OK;
}

// the same pair, for fused C3k2 ops only (a fused C3k2 is never locked)
int fce_net_c3k2_form(const fce_net* net, int i) {
  const int form = fce_net_alt_form(net, i);
  return form >= 0 && net->ops[i].kind == OP_C3K2 ? form : -1;
}

int fce_net_set_c3k2_form(fce_net* net, int i, int fused) {
  FCE_CHECK(fce_net_c3k2_form(net, i) >= 0, "fce_net_set_c3k2_form: not a fused C3k2 op with an alternative");
  return fce_net_set_alt_form(net, i, fused);
}

int fce_net_op_variant(const fce_net* net, int i) {
  return net && i >= 0 && i < int(net->ops.size()) ? net->ops[i].tile : -1;
}

}  // extern "C"
