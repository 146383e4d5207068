// Convolutions for gfx950: weight packing, the generic MFMA implicit GEMM (dense 1x1 / 3x3), and the dispatcher
// over the kernel families (the kFamilies table below; conv_variant.h says what a family is).  The other families
// live in conv1x1.hip, conv3x3_tile.hip, conv3x3_ring.hip, conv3x3_big.hip, conv3x3_wide.hip, conv3x3_dring.hip and
// conv_big.hip; depthwise 3x3 in dwconv.hip, the Cin<=4 stem (NCHW network input) in stem.hip.
//
// Replaces (reference, ultralytics/): nn/modules/conv.py:39-89 Conv.forward_fuse with the BN
// folded by utils/torch_utils.py:237-267; conv.py:185-200 DWConv; the Detect 1x1 nn.Conv2d
// (head.py:86-107); Bottleneck's residual add (block.py:474-476); torch.cat / chunk of
// C2f / C3 / SPPF / C2PSA (block.py:303-307, 338-340, 228-232, 1453-1464) through channel-offset
// reads and writes; nn.Upsample(x2, nearest) feeding a 1x1 conv through `up`.
//
// Data layout: activations NHWC fp16, any view may be a channel slice of a wider buffer.
// Dense conv as GEMM  D[cout][pixel] = sum_k W[cout][k] * X[k][pixel],  k = (tap, cin):
//   v_mfma_f32_16x16x32_f16 with A = weights (16 couts x 32 k), B = activations (32 k x 16 px).
//   Lane l owns A[co = l&15][k = 8(l>>4)+j] and B[k = 8(l>>4)+j][px = l&15]: one 16-byte load
//   of 8 consecutive input channels of one pixel (coalesced along NHWC) per fragment; the
//   weight fragments are pre-packed in exactly this lane order (1 KiB per fragment).
//   D: lane l holds px = l&15, couts 4(l>>4)+0..3  -> 8-byte NHWC stores.
#include "conv_variant.h"
#include "ops.h"

namespace fce {

// ============================================================================ packing (host)
// (dense_geom, conv_variant.h: the fragment counts per cout tile)
size_t conv_weight_bytes(const fce_conv_desc& d) {
  if (is_stem(d))  // [cin*k*k][cout] fp32 (+ MFMA fragments)
    return stem_fp32_bytes(d) + (stem_mfma_ok(d) ? size_t((d.cout + 15) / 16) * 64 * 8 * sizeof(_Float16) : 0);
  if (is_dw(d)) return size_t(d.k) * d.k * d.cin * sizeof(float);             // [k*k][c] fp32
  DenseGeom g = dense_geom(d);
  return size_t(g.cotiles) * g.nalloc * 64 * 8 * sizeof(_Float16);
}

int conv_pack(const fce_conv_desc& d, const float* w, void* out) {
  const int k = d.k, kk = k * k;
  if (is_stem(d)) {  // [ci][ky][kx][co]
    float* o = static_cast<float*>(out);
    for (int co = 0; co < d.cout; ++co)
      for (int ci = 0; ci < d.cin; ++ci)
        for (int t = 0; t < kk; ++t) o[(ci * kk + t) * d.cout + co] = w[(co * d.cin + ci) * kk + t];
    if (stem_mfma_ok(d)) {  // lane l of tile ct: cout ct*16 + (l & 15), k = 8 (l >> 4) + j
      _Float16* f = reinterpret_cast<_Float16*>(static_cast<char*>(out) + stem_fp32_bytes(d));
      for (int ct = 0; ct < (d.cout + 15) / 16; ++ct)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j) {
            const int co = ct * 16 + (l & 15), kq = 8 * (l >> 4) + j;
            f[(ct * 64 + l) * 8 + j] = (_Float16)((co < d.cout && kq < d.cin * 9) ? w[co * d.cin * 9 + kq] : 0.f);
          }
    }
    return FCE_OK;
  }
  if (is_dw(d)) {  // [t][c]
    float* o = static_cast<float*>(out);
    for (int c = 0; c < d.cin; ++c)
      for (int t = 0; t < kk; ++t) o[t * d.cin + c] = w[c * kk + t];
    return FCE_OK;
  }
  // K-step order: cin % 32 == 0 -> chunk-major, step s = (32-channel chunk) * k*k + tap (the order
  // of the LDS-tile 3x3 kernel, so both kernels sum every output in the same order); otherwise
  // 8-channel chunks c = 4s + lane/16 in tap-major order (tap = c / (cin/8)).
  DenseGeom g = dense_geom(d);
  const bool chunk_major = d.cin % 32 == 0;
  _Float16* o = static_cast<_Float16*>(out);
  for (int ct = 0; ct < g.cotiles; ++ct)
    for (int s = 0; s < g.nalloc; ++s)
      for (int l = 0; l < 64; ++l) {
        const int co = ct * 16 + (l & 15);
        _Float16* dst = o + ((size_t(ct) * g.nalloc + s) * 64 + l) * 8;
        int tap, ci0;
        bool in;
        if (chunk_major) {
          tap = s % kk;
          ci0 = (s / kk) * 32 + (l >> 4) * 8;
          in = s < g.nsteps;
        } else {
          const int c = s * 4 + (l >> 4);
          tap = c / g.cpt;
          ci0 = (c % g.cpt) * 8;
          in = c < g.nchunk;
        }
        for (int j = 0; j < 8; ++j) {
          float v = 0.f;
          if (co < d.cout && in) v = w[(size_t(co) * d.cin + ci0 + j) * kk + tap];
          dst[j] = (_Float16)v;
        }
      }
  return FCE_OK;
}

// ============================================================================ dense MFMA kernel
// Software-pipeline depth: K-steps of fragments in flight per wave.  Small register tiles have little
// MFMA work per step to cover a load's latency, so they keep more steps in flight (the summation
// order over K is the same for every depth).
template <int RC, int RP>
struct ConvDepth {
  static constexpr int D = RC * RP == 1 ? 8 : RC * RP == 2 ? 4 : 2;
};

// conv_epilogue (the dense MFMA kernels' epilogue) lives in conv_args.h, shared with conv_big.hip

template <int KS, int RC, int RP, int OUT, bool FAST>
__global__ __launch_bounds__(256) void conv_mfma_kernel(ConvArgs a) {
  constexpr int D = ConvDepth<RC, RP>::D;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;
  const int grp = lane >> 4;
  // XCD-aware block order.  The grid is 1-D (gx pixel tiles x gy cout tiles); the hardware deals
  // block b to XCD b % 8.  Remap so each XCD owns one contiguous range of logical tiles
  // (pixel-tile major, cout tile minor): the cout tiles that re-read a pixel tile's input, and the
  // neighbouring pixel tiles sharing its 3x3 halo rows, run on the same XCD and hit its L2.
  int bx, by;
  {
    const int total = a.gx * a.gy, b = blockIdx.x;
    const int per = total >> 3, body = per << 3;
    const int L = b < body ? (b & 7) * per + (b >> 3) : b;
    bx = L / a.gy;
    by = L - bx * a.gy;
  }
  const int pix_base = (bx * 4 + wave) * (RP * 16);
  const int cot0 = by * RC;
  const int cotiles = (a.cout + 15) >> 4;

  // Per pixel-rep (this lane's B column): element offset of the tap-(0,0) source pixel, and a
  // bit mask of the taps that fall inside the image (zero padding = the other taps).  Computed
  // once, so a B load in the K loop costs a bit test, a 64-bit add and a pointer select.
  int64_t pbase[RP];
  unsigned vmask[RP];
#pragma unroll
  for (int p = 0; p < RP; ++p) {
    int pix = pix_base + p * 16 + col;
    const bool pv = pix < a.P;
    pix = pv ? pix : 0;
    const int hw = a.Ho * a.Wo;
    const int n = pix / hw;
    const int r = pix - n * hw;
    const int iy0 = (r / a.Wo) * a.stride - (KS / 2);
    const int ix0 = (r % a.Wo) * a.stride - (KS / 2);
    unsigned m = 0;
#pragma unroll
    for (int t = 0; t < KS * KS; ++t) {
      const int iy = iy0 + t / KS, ix = ix0 + t % KS;
      m |= unsigned(pv && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win) << t;
    }
    vmask[p] = m;
    // KS == 3 requires up == 0 (host materialises upsampled inputs first)
    pbase[p] = KS == 1 ? nhwc_off(n, iy0 >> a.up, ix0 >> a.up, a.Hs, a.Ws, a.xcs)
                       : (int64_t(n) * a.Hs + iy0) * a.Ws * int64_t(a.xcs) + int64_t(ix0) * a.xcs;
  }

  f4 acc[RC][RP];
#pragma unroll
  for (int r = 0; r < RC; ++r)
#pragma unroll
    for (int p = 0; p < RP; ++p) acc[r][p] = f4{0.f, 0.f, 0.f, 0.f};

  // Branch-free K loop: an out-of-image tap or padded K chunk loads a 16-byte zero line (address
  // select, never a value mask), so no load is conditional and hipcc places counted vmcnt waits;
  // D K-steps of fragments stay in flight (a ring of D register sets, unrolled: static indices).
  // FAST (cin % 32 == 0): a K-step is 32 channels of ONE tap, ordered chunk-major (step =
  // chunk * taps + tap, see conv_pack), so the (chunk, tap) cursor is wave-uniform (scalar).
  // Otherwise each lane decodes its chunk c = 4s+grp with a magic divide.
  const h8* wfrag[RC];
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const int ct = min(cot0 + r, cotiles - 1);
    wfrag[r] = reinterpret_cast<const h8*>(a.w) + (size_t(ct) * a.nalloc) * 64 + lane;
  }
  const h8* zline = reinterpret_cast<const h8*>(g_zero_line);
  const int spt = a.cpt >> 2;  // 32-channel chunks (FAST)
  int lt = 0, ls = 0;          // load cursor: tap, chunk (FAST)
  auto tap_off = [&](int t) -> int64_t {
    const int ky = (t * 11) >> 5;  // t / 3 for t < 9
    return KS == 1 ? 0 : (int64_t(ky) * a.Ws + (t - ky * 3)) * a.xcs;
  };
  auto load_b = [&](int s, h8 (&b)[RP]) {
    int t, ce;  // tap and element offset within the pixel's channels
    bool tin;   // a real K-step (padded steps past the end load the zero line)
    if (FAST) {
      t = lt;
      ce = ls * 32 + grp * 8;
      tin = ls < spt;
      if (++lt == KS * KS) {
        lt = 0;
        ++ls;
      }
    } else {
      const unsigned c = unsigned(s * 4 + grp);
      t = a.cpt == 1 ? int(c) : int(__umulhi(c, a.cmagic));
      ce = (int(c) - t * a.cpt) * 8;
      tin = t < KS * KS;
    }
    const int64_t toff = tap_off(t) + ce;
#pragma unroll
    for (int p = 0; p < RP; ++p) {
      const bool ok = tin && ((vmask[p] >> (t & 31)) & 1u);
      const h8* src = ok ? reinterpret_cast<const h8*>(a.x + pbase[p] + toff) : zline;
      b[p] = *src;
    }
  };
  auto load_a = [&](int s, h8 (&w)[RC]) {  // past the last step: one broadcast zero line, not a 1 KiB fragment
    const bool in = s < a.nsteps;
#pragma unroll
    for (int r = 0; r < RC; ++r) w[r] = *(in ? wfrag[r] + s * 64 : zline);
  };
  h8 bq[D][RP], aq[D][RC];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    load_b(d, bq[d]);
    load_a(d, aq[d]);
  }
  const int full = a.nsteps - a.nsteps % D;
  for (int s = 0; s < full; s += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
#pragma unroll
      for (int r = 0; r < RC; ++r)
#pragma unroll
        for (int p = 0; p < RP; ++p)
          acc[r][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aq[d][r], bq[d][p], acc[r][p], 0, 0, 0);
      load_b(s + D + d, bq[d]);  // reads at most step nsteps + D - 1 < nalloc (zero padded)
      load_a(s + D + d, aq[d]);
    }
  }
  // tail: steps full .. nsteps-1 already sit in ring slots 0 .. rem-1
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (d < a.nsteps - full) {
#pragma unroll
      for (int r = 0; r < RC; ++r)
#pragma unroll
        for (int p = 0; p < RP; ++p)
          acc[r][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aq[d][r], bq[d][p], acc[r][p], 0, 0, 0);
    }
  }

  // ---------------------------------------------------------------- epilogue
  conv_epilogue<RC, RP, OUT>(a, acc, pix_base, cot0, col, grp);
}

// ============================================================================ dispatch

template <int KS, int RC, int RP>
static void launch_dense(const ConvArgs& a, int out_kind, bool fast, dim3 grid, hipStream_t s) {
#define CONV_L(O, F) FCE_LAUNCH((conv_mfma_kernel<KS, RC, RP, O, F>), grid, dim3(256), 0, s, a)
#define CONV_O(O)  \
  if (fast)        \
    CONV_L(O, true); \
  else             \
    CONV_L(O, false);
  if (KS == 3) {  // 3x3 convs always store fp16 (Conv + BN + SiLU [+ residual])
    CONV_O(OUT_F16);
    return;
  }
  switch (out_kind) {
    case OUT_F16:
      CONV_O(OUT_F16);
      break;
    case OUT_F32:
      CONV_O(OUT_F32);
      break;
    case OUT_WSTORE:
      CONV_O(OUT_WSTORE);
      break;
    case OUT_DFL:
      CONV_O(OUT_DFL);
      break;
    case OUT_CLS:
      CONV_O(OUT_CLS);
      break;
    default:
      CONV_O(OUT_ACCUM);
      break;
  }
#undef CONV_O
#undef CONV_L
}

template <int KS, int RP>
static void launch_dense_rp(const ConvArgs& a, int out_kind, bool fast, int rc, hipStream_t s) {
  const int cotiles = (a.cout + 15) / 16;
  ConvArgs b = a;
  b.gx = (a.P + 64 * RP - 1) / (64 * RP);
  b.gy = (cotiles + rc - 1) / rc;
  dim3 grid(unsigned(b.gx * b.gy));
  if (rc == 1)
    launch_dense<KS, 1, RP>(b, out_kind, fast, grid, s);
  else if (rc == 2)
    launch_dense<KS, 2, RP>(b, out_kind, fast, grid, s);
  else
    launch_dense<KS, 4, RP>(b, out_kind, fast, grid, s);
}

// Tile choice: a wave owns (16*RC couts) x (16*RP pixels).  Big tiles reuse each loaded fragment
// more; small layers (20x20, 40x40 maps) need more waves in flight to hide load latency, so the
// tile shrinks until the launch has >= ~4 waves per SIMD (4096 waves on 256 CUs) or hits 1x1.
static void pick_tile(int P, int cotiles, bool need_rc4, int* rc, int* rp) {
  constexpr int64_t kTargetWaves = 4096;
  int c = cotiles >= 4 ? 4 : cotiles >= 2 ? 2 : 1;
  int p = 4;
  auto waves = [&](int c_, int p_) { return int64_t((P + 16 * p_ - 1) / (16 * p_)) * ((cotiles + c_ - 1) / c_); };
  while (waves(c, p) < kTargetWaves) {
    if (p > 1) {
      p /= 2;
    } else if (c > 1 && !need_rc4) {
      c /= 2;
    } else {
      break;
    }
  }
  *rc = c;
  *rp = p;
}

template <int KS>
static void launch_dense_rc(const ConvArgs& a, int out_kind, bool fast, int rc, int rp, hipStream_t s) {
  if (rp == 1)
    launch_dense_rp<KS, 1>(a, out_kind, fast, rc, s);
  else if (rp == 2)
    launch_dense_rp<KS, 2>(a, out_kind, fast, rc, s);
  else
    launch_dense_rp<KS, 4>(a, out_kind, fast, rc, s);
}

// Generic register tiles, coded rc | rp << 4 (kind 0): the one family every dense conv can run
struct GenericCfg {
  int rc, rp;
};
static int generic_encode(GenericCfg c) { return c.rc | (c.rp << 4); }
static GenericCfg generic_decode(int code) { return {code & 15, code >> 4}; }

void generic_offer(const fce_conv_desc& d, int det_box, CodeList& out) {
  const int cotiles = (d.cout + 15) / 16;
  for (int rc : {1, 2, 4}) {
    if (det_box ? rc != 4 : !cotiles_want(rc, cotiles)) continue;
    for (int rp : {1, 2, 4}) out.add(generic_encode({rc, rp}));
  }
}

static int launch_generic(const ConvCall& c, int rc, int rp) {
  const fce_conv_desc& d = c.d;
  if (c.out_kind == OUT_DFL) FCE_CHECK(rc == 4 && c.g.cotiles == 4, "conv detect epilogue: one wave must own all 64 bins");
  if (d.k == 3) FCE_CHECK(d.up == 0 && c.out_kind == OUT_F16, "conv 3x3: plain fp16 store, no fused upsampling");
  const bool fast = d.cin % 32 == 0;
  if (d.k == 1)
    launch_dense_rc<1>(c.a, c.out_kind, fast, rc, rp, c.s);
  else
    launch_dense_rc<3>(c.a, c.out_kind, fast, rc, rp, c.s);
  return launch_status("conv_mfma_kernel");
}

int generic_launch(const ConvCall& c, int code) {
  const GenericCfg t = generic_decode(code);
  FCE_CHECK((t.rc == 1 || t.rc == 2 || t.rc == 4) && (t.rp == 1 || t.rp == 2 || t.rp == 4), "conv: bad tile hint");
  return launch_generic(c, t.rc, t.rp);
}

// ============================================================================ process-wide launch state
// One definition each (conv_variant.h declares them): the families that share them sit in several translation units.
int cus_per_xcd() {
  static const int v = [] {
    int d = 0, n = 0;
    if (hipGetDevice(&d) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess) {
      (void)hipGetLastError();
      n = 256;
    }
    return std::max(1, n / 8);
  }();
  return v;
}
int persist_cap(int occ) {
  static const int cap = [] {
    const char* e = getenv("FCE_PERSIST_OCC");
    return e ? atoi(e) : 0;
  }();
  return cap > 0 ? std::min(occ, cap) : occ;
}
bool no_ring() {
  static const bool v = env_on("FCE_NO_RING");
  return v;
}

// ============================================================================ the family table
// Register tiles a dense conv may run with, or depthwise kernel variants (the executor times them at plan time and
// keeps the first strictly fastest; no family changes the per-output summation order, so results are bitwise the
// same for every choice).  The row order IS the candidate order: tune logs and reports follow it and `cap` truncates
// by position.  Kind 1 has two rows: the A-in-LDS halo tiles (opt-in) are listed last.
static constexpr ConvFamily kFamilies[] = {
    {0, "generic register tile", generic_offer, generic_launch},
    {3, "1x1 streaming", stream1_offer, stream1_launch},
    {4, "1x1 LDS-staged", lds1_offer, lds1_launch},
    {5, "1x1 LDS ring", ring1_offer, ring1_launch},
    {11, "1x1 256-wide tile", big1_offer, big1_launch},
    {7, "1x1 K-pipelined big tile", pipe1_offer, pipe1_launch},
    {2, "3x3 small-cin LDS tile", small3_offer, small3_launch},
    {6, "3x3 register ring", ring3_offer, ring3_launch},
    {13, "3x3 LDS-DMA ring", dring_offer, dring_launch},
    {9, "3x3 32x32x16 ring", ring32_offer, ring32_launch},
    {1, "3x3 LDS halo tile", tile3_offer, tile3_launch},
    {8, "3x3 LDS-DMA big tile", big3_offer, big3_launch},
    {12, "3x3 256-wide implicit GEMM", big3g_offer, big3g_launch},
    {10, "3x3 wide tile", wide3_offer, wide3_launch},
    {1, "3x3 LDS halo tile, A in LDS", tile3al_offer, tile3_launch},
};

// no two rows claim one kind, except the declared kind-1 pair (which must share its launch)
static constexpr bool families_distinct() {
  constexpr int n = sizeof(kFamilies) / sizeof(kFamilies[0]);
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (kFamilies[i].kind == kFamilies[j].kind && (kFamilies[i].kind != 1 || kFamilies[i].launch != kFamilies[j].launch))
        return false;
  return true;
}
static_assert(families_distinct(), "conv family table: two rows claim the same kind");

// Returns the count; 0 for the stem.
int conv_tile_candidates(const fce_conv_desc& d, int det_box, int in_w, int* out, int cap) {
  if (is_stem(d)) return 0;
  if (is_dw(d)) return dwconv_candidates(d, in_w, out, cap);
  CodeList list{out, cap, 0};
  for (const ConvFamily& f : kFamilies) f.offer(d, det_box, list);
  return list.n;
}

int conv2d_impl(const fce_conv_desc& d, const fce_tensor& x, const void* w, const float* bias, const fce_tensor* res,
                const fce_tensor& y, const fce_detect_epi* det, hipStream_t s, int tile, const fce_tensor* dup,
                int duplo) {
  FCE_CHECK(d.k == 1 || d.k == 3 || (is_stem(d) && d.k <= 7), "conv: kernel size must be 1 or 3");
  FCE_CHECK(d.stride >= 1 && d.stride <= 2, "conv: stride must be 1 or 2");
  FCE_CHECK(x.n == y.n && x.c == d.cin && y.c == d.cout, "conv: channel/batch mismatch");
  const int Hin = x.h << d.up, Win = x.w << d.up;
  const int pad = d.k / 2;
  const int Ho = (Hin + 2 * pad - d.k) / d.stride + 1, Wo = (Win + 2 * pad - d.k) / d.stride + 1;
  FCE_CHECK(y.h == Ho && y.w == Wo, "conv: output spatial size mismatch");
  FCE_CHECK(y.layout == FCE_NHWC, "conv: output must be NHWC");
  if (int64_t(y.n) * Ho * Wo == 0) return FCE_OK;

  if (is_stem(d)) return launch_stem(d, x, w, bias, res, y, Ho, Wo, s);

  FCE_CHECK(x.layout == FCE_NHWC && x.dtype == FCE_F16, "conv: input must be NHWC f16");
  FCE_CHECK(x.cstride % 8 == 0 && x.coff % 8 == 0, "conv: input slice must be 8-channel aligned");

  if (is_dw(d)) {
    FCE_CHECK(d.groups == d.cin && d.cin == d.cout && d.cin % 8 == 0, "dwconv: groups == cin == cout, cin % 8 == 0");
    FCE_CHECK(y.dtype == FCE_F16 && d.up == 0 && res == nullptr && d.epilogue == FCE_EPI_STORE && d.k == 3,
              "dwconv: 3x3, plain f16 store only");
    return dwconv_launch(d, x, w, bias, y, s, tile);
  }

  FCE_CHECK(d.cin % 8 == 0, "conv: cin must be a multiple of 8");
  int out_kind;
  if (det) {
    FCE_CHECK(det->pred && det->part >= 0 && det->part <= 1 && d.k == 1 && d.up == 0 && res == nullptr,
              "conv detect epilogue: 1x1 conv into pred");
    FCE_CHECK(det->part == 1 || (d.cout == 4 * det->reg_max && det->reg_max == 16),
              "conv detect epilogue: box branch needs 4 x reg_max(16) outputs");
    FCE_CHECK(det->part == 0 || d.cout == det->nc, "conv detect epilogue: cls branch needs nc outputs");
    out_kind = det->part == 0 ? OUT_DFL : OUT_CLS;
  } else if (y.dtype == FCE_F32) {
    FCE_CHECK(d.epilogue == FCE_EPI_STORE && res == nullptr, "conv: f32 output supports plain store only");
    out_kind = OUT_F32;
  } else {
    out_kind = d.epilogue == FCE_EPI_WSTORE ? OUT_WSTORE : d.epilogue == FCE_EPI_ACCUM ? OUT_ACCUM : OUT_F16;
  }
  if (res) {
    FCE_CHECK(res->layout == FCE_NHWC && res->dtype == FCE_F16 && res->c == d.cout && res->h == Ho && res->w == Wo,
              "conv: residual must match the output view");
  }
  DenseGeom g = dense_geom(d);
  ConvArgs a;
  a.x = static_cast<const _Float16*>(x.data) + x.coff;
  a.N = x.n;
  a.Hs = x.h;
  a.Ws = x.w;
  a.xcs = x.cstride;
  a.Hin = Hin;
  a.Win = Win;
  a.up = d.up;
  a.cin = d.cin;
  a.cout = d.cout;
  a.stride = d.stride;
  a.Ho = Ho;
  a.Wo = Wo;
  a.P = y.n * Ho * Wo;
  a.w = static_cast<const _Float16*>(w);
  a.bias = bias;
  a.res = res ? static_cast<const _Float16*>(res->data) + res->coff : nullptr;
  a.rcs = res ? res->cstride : 0;
  a.ycs = y.cstride;
  a.y = y.dtype == FCE_F32 ? static_cast<void*>(static_cast<float*>(y.data) + y.coff)
                           : static_cast<void*>(static_cast<_Float16*>(y.data) + y.coff);
  a.act = d.act;
  a.fw = d.fusion_w;
  a.fn = d.fusion_n;
  a.fi = d.fusion_i;
  a.cpt = g.cpt;
  a.nchunk = g.nchunk;
  a.nsteps = g.nsteps;
  a.nalloc = g.nalloc;
  a.cmagic = g.cpt > 1 ? unsigned(0xFFFFFFFFull / unsigned(g.cpt) + 1ull) : 0u;
  FCE_CHECK(g.nalloc >= ((g.nsteps + 7) & ~7) + 8 && g.nchunk + 64 < 65536, "conv: K too large for the chunk cursor");
  a.vec_ok = (y.cstride % 4 == 0 && y.coff % 4 == 0 && (!res || (res->cstride % 4 == 0 && res->coff % 4 == 0))) ? 1 : 0;
  static const bool no_stg = [] {
    const char* e = getenv("FCE_NO_STG");
    return e && atoi(e) != 0;
  }();
  a.stg = !no_stg && (out_kind == OUT_F16 || out_kind == OUT_WSTORE) && y.dtype == FCE_F16 && d.cout % 8 == 0 &&
          y.cstride % 8 == 0 && y.coff % 8 == 0 && a.vec_ok;
  if (out_kind == OUT_WSTORE || out_kind == OUT_ACCUM) FCE_CHECK(d.fusion_w && d.fusion_n > d.fusion_i, "conv: fusion weights");
  a.pred = det ? det->pred : nullptr;
  a.det_A = det ? det->anchors : 0;
  a.det_a0 = det ? det->anchor_offset : 0;
  a.det_nc = det ? det->nc : 0;
  a.det_hw = Ho * Wo;
  a.det_w = Wo;
  a.det_stride = det ? det->stride : 0.f;
  a.det_best = det ? det->best : nullptr;
  a.dup = nullptr;
  a.dupcs = a.duplo = a.dupn = 0;
  if (dup) {
    FCE_CHECK(d.k == 1 && !is_dw(d) && out_kind == OUT_F16 && dup->layout == FCE_NHWC && dup->dtype == FCE_F16 &&
                  dup->n == y.n && dup->h == Ho && dup->w == Wo && duplo >= 0 && duplo % 8 == 0 && dup->c % 8 == 0 &&
                  duplo + dup->c <= d.cout && dup->cstride % 8 == 0 && dup->coff % 8 == 0 && a.vec_ok,
              "conv: duplicate store needs a 1x1 fp16 plain store and 8-aligned channel ranges");
    a.dup = static_cast<_Float16*>(dup->data) + dup->coff;
    a.dupcs = dup->cstride;
    a.duplo = duplo;
    a.dupn = dup->c;
  }
  const ConvCall call{d, a, out_kind, g, x.n, s, x, w, bias, res, y, det, dup, duplo};
  if (tile < 0) {  // no hint: the generic kernel on a heuristic tile
    int rc, rp;
    pick_tile(a.P, g.cotiles, out_kind == OUT_DFL, &rc, &rp);
    return launch_generic(call, rc, rp);
  }
  const int kind = (tile >> 8) & 15;
  for (const ConvFamily& f : kFamilies)
    if (f.kind == kind) return f.launch(call, tile);
  return fail(FCE_ERR_INVALID, "conv: unknown kernel variant");
}

int conv2d(const fce_conv_desc& d, const fce_tensor& x, const void* w, const float* bias, const fce_tensor* res,
           const fce_tensor& y, hipStream_t s, int tile, const fce_tensor* dup, int duplo) {
  return conv2d_impl(d, x, w, bias, res, y, nullptr, s, tile, dup, duplo);
}

int conv2d_detect(const fce_conv_desc& d, const fce_tensor& x, const void* w, const float* bias,
                  const fce_detect_epi& e, hipStream_t s, int tile) {
  // the output view only carries the spatial geometry; results go to e.pred
  fce_tensor y{nullptr, FCE_F32, FCE_NHWC, x.n, d.cout, x.h, x.w, d.cout, 0};
  return conv2d_impl(d, x, w, bias, nullptr, y, &e, s, tile);
}

}  // namespace fce
