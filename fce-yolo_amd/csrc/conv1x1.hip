// 1x1 convolution families besides the generic implicit GEMM (conv.hip): streaming waves (0x300), LDS-staged pixel
// tiles (0x400), the persistent LDS ring (0x500) and the K-pipelined big tile (0x700).  Each ends in its family
// section: the code's encode / decode pair, its capability predicate, offer() and launch() (conv_variant.h).
// Replaces (reference, ultralytics/): nn/modules/conv.py:39-89 Conv.forward_fuse (1x1, BN folded by
// utils/torch_utils.py:237-267), the Detect 1x1 nn.Conv2d (head.py:86-107) and nn.Upsample(x2, nearest) feeding a
// 1x1 conv through `up`.  Per output the K order is conv_mfma_kernel's: bitwise-identical results.
#include "conv_variant.h"

namespace fce {

// ============================================================================ 1x1, streaming waves
// For 1x1 convs with cin % 32 == 0 and few K-steps (cin <= 32 * NSM): in the implicit-GEMM kernel a
// wave then does a handful of MFMAs behind one load latency and exits.  Here a wave keeps the weight
// fragments of its RC cout tiles for ALL K-steps in registers (loaded once) and walks a strided
// sequence of pixel tiles (RP x 16 pixels), the next tile's B fragments in flight while the current
// tile's MFMAs and epilogue run.  Waves gw of a launch: cout group gw % gy, tile sequence
// gw / gy, + W, + 2W, ...  (adjacent waves = the cout groups of the same pixels, on one CU).  Per
// output the K order is the implicit-GEMM kernel's (steps 0..nsteps-1): bitwise-identical results.
template <int RC, int RP, int NSM, int OUT>
__global__ __launch_bounds__(256) void conv1x1_stream_kernel(ConvArgs a, int W) {
  const int lane = threadIdx.x & 63, col = lane & 15, grp = lane >> 4;
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int g = gw % a.gy, i0 = gw / a.gy;
  const int ns = a.nsteps;
  const int cot0 = g * RC;
  const int cotiles = (a.cout + 15) >> 4;
  const int ntiles = (a.P + 16 * RP - 1) / (16 * RP);
  h8 aw[NSM][RC];
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const h8* wf = reinterpret_cast<const h8*>(a.w) + (size_t(min(cot0 + r, cotiles - 1)) * a.nalloc) * 64 + lane;
#pragma unroll
    for (int st = 0; st < NSM; ++st) aw[st][r] = st < ns ? wf[st * 64] : h8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  const int hw = a.Ho * a.Wo;
  auto load_tile = [&](int t, h8 (&b)[NSM][RP]) {
#pragma unroll
    for (int p = 0; p < RP; ++p) {
      int pix = t * 16 * RP + p * 16 + col;
      pix = pix < a.P ? pix : 0;  // past the end: any valid pixel (the epilogue skips it)
      const int n = pix / hw, r = pix - n * hw;
      const int oy = r / a.Wo, ox = r - oy * a.Wo;
      const _Float16* src = a.x + nhwc_off(n, oy >> a.up, ox >> a.up, a.Hs, a.Ws, a.xcs) + grp * 8;
#pragma unroll
      for (int st = 0; st < NSM; ++st)
        if (st < ns) b[st][p] = *reinterpret_cast<const h8*>(src + st * 32);
    }
  };
  h8 bq[NSM][RP];
  if (i0 < ntiles) load_tile(i0, bq);
  for (int t = i0; t < ntiles; t += W) {
    h8 bc[NSM][RP];
#pragma unroll
    for (int st = 0; st < NSM; ++st)
#pragma unroll
      for (int p = 0; p < RP; ++p) bc[st][p] = bq[st][p];
    if (t + W < ntiles) load_tile(t + W, bq);
    f4 acc[RC][RP];
#pragma unroll
    for (int r = 0; r < RC; ++r)
#pragma unroll
      for (int p = 0; p < RP; ++p) acc[r][p] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < NSM; ++st) {
      if (st < ns) {
#pragma unroll
        for (int r = 0; r < RC; ++r)
#pragma unroll
          for (int p = 0; p < RP; ++p)
            acc[r][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aw[st][r], bc[st][p], acc[r][p], 0, 0, 0);
      }
    }
    conv_epilogue<RC, RP, OUT>(a, acc, t * 16 * RP, cot0, col, grp);
  }
}

static bool stream_ok(int nsm, int rc, int rp) { return nsm * (rc + 2 * rp) <= 40; }

template <int RC, int RP, int NSM>
static void launch_stream_o(const ConvArgs& a, int out_kind, dim3 grid, int W, hipStream_t s) {
#define STREAM_L(O) FCE_LAUNCH((conv1x1_stream_kernel<RC, RP, NSM, O>), grid, dim3(256), 0, s, a, W)
  switch (out_kind) {
    case OUT_F16: STREAM_L(OUT_F16); break;
    case OUT_F32: STREAM_L(OUT_F32); break;
    case OUT_WSTORE: STREAM_L(OUT_WSTORE); break;
    case OUT_DFL: STREAM_L(OUT_DFL); break;
    case OUT_CLS: STREAM_L(OUT_CLS); break;
    default: STREAM_L(OUT_ACCUM); break;
  }
#undef STREAM_L
}

template <int NSM>
static void launch_stream_n(const ConvArgs& a, int out_kind, int rc, int rp, dim3 grid, int W, hipStream_t s) {
  if constexpr (NSM <= 4) {
    if (rc == 4 && rp == 2) return launch_stream_o<4, 2, NSM>(a, out_kind, grid, W, s);
    if (rc == 2 && rp == 2) return launch_stream_o<2, 2, NSM>(a, out_kind, grid, W, s);
    if (rc == 4 && rp == 1) return launch_stream_o<4, 1, NSM>(a, out_kind, grid, W, s);
  }
  if (rc == 1 && rp == 2) return launch_stream_o<1, 2, NSM>(a, out_kind, grid, W, s);
  if (rc == 2 && rp == 1) return launch_stream_o<2, 1, NSM>(a, out_kind, grid, W, s);
  launch_stream_o<1, 1, NSM>(a, out_kind, grid, W, s);
}

static int stream_nsm(int nsteps) { return nsteps <= 2 ? 2 : nsteps <= 4 ? 4 : nsteps <= 8 ? 8 : 0; }

// waves per cout group: enough pixel-tile streams to fill the GPU (about 8 waves per SIMD in all),
// but every wave gets at least 2 tiles so the prefetch has something to overlap
static int launch_stream(const ConvArgs& a0, int out_kind, int rc, int rp, hipStream_t s) {
  const int nsm = stream_nsm(a0.nsteps);
  FCE_CHECK(nsm > 0 && stream_ok(nsm, rc, rp), "conv 1x1 stream: K too deep for the register budget");
  ConvArgs a = a0;
  const int cotiles = (a.cout + 15) / 16;
  a.gy = (cotiles + rc - 1) / rc;
  const int ntiles = (a.P + 16 * rp - 1) / (16 * rp);
  int W = std::max(1, std::min((ntiles + 1) / 2, 8192 / a.gy));
  while ((int64_t(W) * a.gy) % 4) ++W;  // whole blocks of 4 waves
  const dim3 grid(unsigned(int64_t(W) * a.gy / 4));
  if (nsm == 2)
    launch_stream_n<2>(a, out_kind, rc, rp, grid, W, s);
  else if (nsm == 4)
    launch_stream_n<4>(a, out_kind, rc, rp, grid, W, s);
  else
    launch_stream_n<8>(a, out_kind, rc, rp, grid, W, s);
  return launch_status("conv1x1_stream_kernel");
}

// Staged fp16 store for the LDS-tile 1x1 kernels (OUT_F16 / OUT_WSTORE with a.stg): the block's output
// tile (TPB pixels x CB*16 couts) is assembled in LDS (`ot`, rows of CB*16 halves, 16-byte slot sl of
// pixel px at sl ^ (px & (2 CB - 1))) and written with 16-byte lane stores, whole pixel rows per 2 CB
// lanes, instead of 8-byte stores scattered over 16 pixels.  Values are computed exactly as in
// conv_epilogue (bias, SiLU, residual, BiFPN alpha, then one fp16 rounding): bitwise the same.
// Caller: every thread of the block, after the last B read of `ot`'s memory (barrier inside).
template <int RC, int RP, int CB, int TPB, int OUT>
__device__ __forceinline__ void conv_store_staged(const ConvArgs& a, f4 (&acc)[RC][RP], int pix0, int pw, int cbl0,
                                                  int wc, int col, int grp, _Float16* ot) {
  constexpr int ROW = CB * 16, NSL = 2 * CB;
  const int cotiles = (a.cout + 15) >> 4;
  float alpha = 1.f;
  if (OUT == OUT_WSTORE) alpha = fusion_alpha(a.fw, a.fn, a.fi);
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const int ctl = wc * RC + r;  // local cout tile
    const int co0 = (cbl0 + ctl) * 16 + grp * 4;
    if (cbl0 + ctl >= cotiles) continue;
    float bz[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bz[j] = bias_or0(a.bias, co0 + j, a.cout);
#pragma unroll
    for (int p = 0; p < RP; ++p) {
      const int px = pw + p * 16 + col, pix = pix0 + px;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float t = acc[r][p][j] + bz[j];
        v[j] = a.act ? silu(t) : t;
      }
      if (a.res && pix < a.P) {
        const _Float16* ro = a.res + int64_t(pix) * a.rcs + co0;
        if (a.vec_ok && co0 + 3 < a.cout) {
          const h4 rv = *reinterpret_cast<const h4*>(ro);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = fpin(v[j] + (float)rv[j]);
        } else {
          for (int j = 0; j < 4; ++j)
            if (co0 + j < a.cout) v[j] = fpin(v[j] + (float)ro[j]);
        }
      }
      if (OUT == OUT_WSTORE) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fpin(v[j] * alpha);
      }
      const int sl = ctl * 2 + (grp >> 1);
      *reinterpret_cast<h4*>(ot + px * ROW + ((sl ^ (px & (NSL - 1))) * 8) + (grp & 1) * 4) =
          h4{(_Float16)fpin(v[0]), (_Float16)fpin(v[1]), (_Float16)fpin(v[2]), (_Float16)fpin(v[3])};
    }
  }
  __syncthreads();
  constexpr int NP = TPB * NSL;  // 16-byte pieces of the tile
#pragma unroll
  for (int e0 = 0; e0 < NP; e0 += 256) {
    const int e = e0 + int(threadIdx.x);
    if (NP % 256 != 0 && e >= NP) break;
    const int px = e / NSL, sl = e - px * NSL;
    const int pix = pix0 + px, co = cbl0 * 16 + sl * 8;
    if (pix < a.P && co < a.cout) {
      const h8 hv = *reinterpret_cast<const h8*>(ot + px * ROW + (sl ^ (px & (NSL - 1))) * 8);
      *reinterpret_cast<h8*>(static_cast<_Float16*>(a.y) + int64_t(pix) * a.ycs + co) = hv;
      if (OUT == OUT_F16 && a.dup && co >= a.duplo && co < a.duplo + a.dupn)  // duplo, dupn % 8 == 0 (host)
        *reinterpret_cast<h8*>(a.dup + int64_t(pix) * a.dupcs + (co - a.duplo)) = hv;
    }
  }
}

// ============================================================================ 1x1, LDS-staged pixel tiles
// For 1x1 stride-1 convs (any cin % 8 == 0, optional fused nearest upsampling).  A block (4 waves)
// owns TPB = WP*RP*16 consecutive output pixels and CB = (4/WP)*RC cout tiles; wave (wc, wp) computes
// RC cout tiles x RP 16-pixel groups.  Per K chunk of NSC 32-channel steps the block stages its
// pixels' input rows in LDS with full-line loads (8 lanes = one pixel's 128-byte pair of steps) and
// every wave reads its B fragments from there, instead of each wave issuing fragment-shaped
// (16 pixels x 64 B) loads that re-read the input once per cout group.
// LDS image per pair of steps: [pixel][8 x 16 B]; piece j of pixel p sits in slot j ^ ((p >> 1) & 7).
// That is conflict-free for the staging ds_write_b128 (8 lanes = the 8 slots of one 128-B row) and
// for the B-fragment ds_read_b128 (each 16-lane group meets 16 distinct 16-B slots of the bank row).
// Channels past cin are staged as zeros.  A fragments, K-step contents and the per-output summation
// order are the implicit-GEMM kernel's, so the results are bitwise identical.
template <int RC, int RP, int WP, int NSC, int OUT>
__global__ __launch_bounds__(256) void conv1x1_lds_kernel(ConvArgs a) {
  constexpr int TPB = WP * RP * 16;
  constexpr int NPAIR = (NSC + 1) / 2;
  constexpr int NPC = TPB * NPAIR * 8;  // 16-byte pieces staged per chunk
  static_assert(NPC % 256 == 0, "whole staging rounds");
  constexpr int IT = NPC / 256;
  extern __shared__ __attribute__((aligned(16))) h8 xt[];  // [NPAIR][TPB][8]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int wc = wave / WP, wp = wave - wc * WP;
  int bx, by;  // XCD-aware order, as conv_mfma_kernel: a pixel tile's cout groups share an XCD's L2
  {
    const int total = a.gx * a.gy, b = blockIdx.x;
    const int per = total >> 3, body = per << 3;
    const int L = b < body ? (b & 7) * per + (b >> 3) : b;
    bx = L / a.gy;
    by = L - bx * a.gy;
  }
  const int pix0 = bx * TPB;
  const int cot0 = (by * (4 / WP) + wc) * RC;
  const int cotiles = (a.cout + 15) >> 4;
  const h8* wfrag[RC];
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const int ct = min(cot0 + r, cotiles - 1);
    wfrag[r] = reinterpret_cast<const h8*>(a.w) + (size_t(ct) * a.nalloc) * 64 + lane;
  }
  // staging: piece e = threadIdx.x + 256 i -> (pixel p = e / (8 NPAIR), pair q, piece j): a pixel's
  // chunk is contiguous in global memory, so consecutive lanes read consecutive 16-byte pieces
  int64_t soff[IT];
  int spos[IT], sch[IT];
  bool spv[IT];
  const int hw = a.Ho * a.Wo;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int e = threadIdx.x + 256 * i;
    const int j = e & 7, rest = e >> 3;
    const int p = rest / NPAIR, q = rest - p * NPAIR;
    const int pix = pix0 + p;
    spv[i] = pix < a.P;
    const int pc = spv[i] ? pix : 0;
    if (a.up) {
      const int n = pc / hw, r = pc - n * hw;
      const int oy = r / a.Wo, ox = r - oy * a.Wo;
      soff[i] = nhwc_off(n, oy >> a.up, ox >> a.up, a.Hs, a.Ws, a.xcs);
    } else {
      soff[i] = int64_t(pc) * a.xcs;
    }
    sch[i] = q * 64 + j * 8;
    spos[i] = (q * TPB + p) * 8 + (j ^ ((p >> 1) & 7));
  }
  f4 acc[RC][RP];
#pragma unroll
  for (int r = 0; r < RC; ++r)
#pragma unroll
    for (int p = 0; p < RP; ++p) acc[r][p] = f4{0.f, 0.f, 0.f, 0.f};
  const int pw = wp * RP * 16;  // this wave's first pixel within the tile
  for (int k0 = 0; k0 < a.nsteps; k0 += NSC) {
    if (k0) __syncthreads();  // previous chunk's B reads done
    h8 af[NSC][RC];           // packed A is zero-padded past nsteps: always in bounds
#pragma unroll
    for (int s = 0; s < NSC; ++s)
#pragma unroll
      for (int r = 0; r < RC; ++r) af[s][r] = wfrag[r][(k0 + s) * 64];
    h8 v[IT];
    const int cbase = k0 * 32;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int c = cbase + sch[i];
      const bool ok = spv[i] && c < a.cin;
      v[i] = *(ok ? reinterpret_cast<const h8*>(a.x + soff[i] + c) : reinterpret_cast<const h8*>(g_zero_line));
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) xt[spos[i]] = v[i];
    __syncthreads();
    const int nsc = min(NSC, a.nsteps - k0);
#pragma unroll
    for (int s = 0; s < NSC; ++s) {
      if (s < nsc) {
        h8 bf[RP];
#pragma unroll
        for (int p = 0; p < RP; ++p) {
          const int px = pw + p * 16 + col;
          const int j = (s & 1) * 4 + grp;
          bf[p] = xt[((s >> 1) * TPB + px) * 8 + (j ^ ((px >> 1) & 7))];
        }
#pragma unroll
        for (int r = 0; r < RC; ++r)
#pragma unroll
          for (int p = 0; p < RP; ++p)
            acc[r][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s][r], bf[p], acc[r][p], 0, 0, 0);
      }
    }
  }
  if constexpr (OUT == OUT_F16 || OUT == OUT_WSTORE) {
    if (a.stg) {
      __syncthreads();  // every wave's last B read done: the staging image becomes the output tile
      conv_store_staged<RC, RP, (4 / WP) * RC, TPB, OUT>(a, acc, pix0, pw, by * (4 / WP) * RC, wc, col, grp,
                                                         reinterpret_cast<_Float16*>(xt));
      return;
    }
  }
  conv_epilogue<RC, RP, OUT>(a, acc, pix0 + pw, cot0, col, grp);
}

// Source element offset of output pixel pix of a stride-1 1x1 conv (nearest upsampling folded in).

// 1x1 with the whole K (nsteps <= NSC <= 8) in one LDS image, as a persistent double-buffered ring:
// the same tile geometry, LDS image and fragment reads as conv1x1_lds_kernel, but each block walks a
// sequence of pixel tiles and issues the global loads of tile i+1 into registers before it computes
// and stores tile i, so HBM reads stay in flight through the MFMA and epilogue phases (one barrier per
// tile).  Block b: XCD b % 8, cout group by, slot; pixel tiles bx = xcd + 8 (slot + k nslot): the gy
// blocks that read the same pixel tiles sit on one XCD and walk them in step (L2 hits), and a block's
// cout group never changes, so its A fragments are loaded once.  Bitwise identical to the others.
template <int RC, int RP, int WP, int NSC, int OUT>
__global__ __launch_bounds__(256) void conv1x1_ring_kernel(ConvArgs a, int nslot) {
  constexpr int TPB = WP * RP * 16;
  constexpr int NPAIR = (NSC + 1) / 2;
  constexpr int BUF = NPAIR * TPB * 8;  // h8 per LDS buffer
  static_assert(BUF % 256 == 0, "whole staging rounds");
  constexpr int IT = BUF / 256;
  extern __shared__ __attribute__((aligned(16))) h8 xr[];  // [2][NPAIR][TPB][8]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int wc = wave / WP, wp = wave - wc * WP;
  const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
  const int by = loc % a.gy, slot = loc / a.gy;
  int bx = xcd + 8 * slot;
  if (bx >= a.gx) return;  // block-uniform
  const int cot0 = (by * (4 / WP) + wc) * RC;
  const int cotiles = (a.cout + 15) >> 4;
  h8 af[NSC][RC];
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const h8* wf = reinterpret_cast<const h8*>(a.w) + (size_t(min(cot0 + r, cotiles - 1)) * a.nalloc) * 64 + lane;
#pragma unroll
    for (int s = 0; s < NSC; ++s) af[s][r] = wf[s * 64];  // zero-padded past nsteps
  }
  // (the upsampling branch is hoisted out of the unrolled loads: per-piece branches make hipcc wrap
  // every load in its own exec branch)
  auto stage_load_t = [&](auto up_tag, int tile, h8 (&v)[IT]) {
    constexpr bool UP = decltype(up_tag)::value;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = threadIdx.x + 256 * i;
      const int j = e & 7, rest = e >> 3;
      const int p = rest / NPAIR, q = rest - p * NPAIR;
      const int pix = tile * TPB + p, c = q * 64 + j * 8;
      const bool ok = pix < a.P && c < a.cin;
      const int64_t off = UP ? conv1x1_src(a, ok ? pix : 0) : int64_t(ok ? pix : 0) * a.xcs;
      v[i] = *(ok ? reinterpret_cast<const h8*>(a.x + off + c) : reinterpret_cast<const h8*>(g_zero_line));
    }
  };
  auto stage_load = [&](int tile, h8 (&v)[IT]) {
    if (a.up)
      stage_load_t(std::true_type{}, tile, v);
    else
      stage_load_t(std::false_type{}, tile, v);
  };
  auto stage_store = [&](int buf, const h8 (&v)[IT]) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = threadIdx.x + 256 * i;
      const int j = e & 7, rest = e >> 3;
      const int p = rest / NPAIR, q = rest - p * NPAIR;
      xr[buf * BUF + (q * TPB + p) * 8 + (j ^ ((p >> 1) & 7))] = v[i];
    }
  };
  const int pw = wp * RP * 16;
  const int step = 8 * nslot;
  h8 v[IT];
  stage_load(bx, v);
  for (int cur = 0; bx < a.gx; cur ^= 1) {
    stage_store(cur, v);
    __syncthreads();
    const int nbx = bx + step;
    if (nbx < a.gx) stage_load(nbx, v);
    f4 acc[RC][RP];
#pragma unroll
    for (int r = 0; r < RC; ++r)
#pragma unroll
      for (int p = 0; p < RP; ++p) acc[r][p] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NSC; ++s) {
      if (s < a.nsteps) {
        h8 bf[RP];
#pragma unroll
        for (int p = 0; p < RP; ++p) {
          const int px = pw + p * 16 + col;
          const int j = (s & 1) * 4 + grp;
          bf[p] = xr[cur * BUF + ((s >> 1) * TPB + px) * 8 + (j ^ ((px >> 1) & 7))];
        }
#pragma unroll
        for (int r = 0; r < RC; ++r)
#pragma unroll
          for (int p = 0; p < RP; ++p)
            acc[r][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s][r], bf[p], acc[r][p], 0, 0, 0);
      }
    }
    conv_epilogue<RC, RP, OUT>(a, acc, bx * TPB + pw, cot0, col, grp);
    bx = nbx;
  }
}

// LDS-staged 1x1 configurations (their codes: lds1_encode / ring1_encode below)
static bool lds1_cfg_ok(int rc, int rp, int wp) {
  return (rc == 1 && rp == 4 && wp == 1) || (rc == 2 && rp == 4 && wp == 1) || (rc == 2 && rp == 2 && wp == 2) ||
         (rc == 1 && rp == 4 && wp == 2) || (rc == 1 && rp == 2 && wp == 4) || (rc == 4 && rp == 1 && wp == 4) ||
         (rc == 4 && rp == 2 && wp == 4);
}
static int lds1_nsc(int nsteps, int rc) {
  const int cap = rc == 4 ? 4 : 8;
  return nsteps <= 2 ? 2 : nsteps <= 4 || cap == 4 ? 4 : 8;
}
static size_t lds1_bytes(int rp, int wp, int nsc) { return size_t(wp) * rp * 16 * ((nsc + 1) / 2) * 128; }
static size_t lds1_out_bytes(int rc, int rp, int wp) { return size_t(wp) * rp * 16 * (4 / wp) * rc * 16 * 2; }

template <int RC, int RP, int WP, int NSC>
static void launch_lds1_o(const ConvArgs& a, int out_kind, dim3 grid, size_t lds, hipStream_t s) {
#define LDS1_L(O) FCE_LAUNCH((conv1x1_lds_kernel<RC, RP, WP, NSC, O>), grid, dim3(256), lds, s, a)
  switch (out_kind) {
    case OUT_F16: LDS1_L(OUT_F16); break;
    case OUT_F32: LDS1_L(OUT_F32); break;
    case OUT_WSTORE: LDS1_L(OUT_WSTORE); break;
    case OUT_CLS: LDS1_L(OUT_CLS); break;
    case OUT_DFL:
      if constexpr (RC == 4) LDS1_L(OUT_DFL);
      break;
    default: LDS1_L(OUT_ACCUM); break;
  }
#undef LDS1_L
}

template <int RC, int RP, int WP>
static void launch_lds1_n(const ConvArgs& a, int out_kind, int nsc, dim3 grid, size_t lds, hipStream_t s) {
  if (nsc == 2)
    launch_lds1_o<RC, RP, WP, 2>(a, out_kind, grid, lds, s);
  else if (nsc == 4 || RC == 4)
    launch_lds1_o<RC, RP, WP, 4>(a, out_kind, grid, lds, s);
  else
    launch_lds1_o<RC, RP, WP, (RC == 4 ? 4 : 8)>(a, out_kind, grid, lds, s);
}

static int ring_nsc(int nsteps) { return nsteps <= 2 ? 2 : nsteps <= 4 ? 4 : nsteps <= 6 ? 6 : nsteps <= 8 ? 8 : 0; }
static bool ring_ok(int nsteps, int rc, int rp, int wp) {
  const int nsc = ring_nsc(nsteps);
  return nsc > 0 && lds1_cfg_ok(rc, rp, wp) && nsc * rc <= 16 && 2 * lds1_bytes(rp, wp, nsc) <= 64 * 1024;
}

template <int RC, int RP, int WP, int NSC>
static void launch_ring_o(const ConvArgs& a, int out_kind, dim3, size_t lds, int, hipStream_t s) {
#define RING_L(O)                                                                                  \
  {                                                                                                \
    static const int occ = blocks_per_cu(conv1x1_ring_kernel<RC, RP, WP, NSC, O>, lds);            \
    const int nslot = ring_slots(a.gx, a.gy, occ);                                                 \
    FCE_LAUNCH((conv1x1_ring_kernel<RC, RP, WP, NSC, O>), dim3(unsigned(8 * a.gy * nslot)), dim3(256), lds, s, a, \
               nslot);                                                                             \
  }
  switch (out_kind) {
    case OUT_F16: RING_L(OUT_F16); break;
    case OUT_F32: RING_L(OUT_F32); break;
    case OUT_WSTORE: RING_L(OUT_WSTORE); break;
    case OUT_CLS: RING_L(OUT_CLS); break;
    case OUT_DFL:
      if constexpr (RC == 4) RING_L(OUT_DFL);
      break;
    default: RING_L(OUT_ACCUM); break;
  }
#undef RING_L
}

template <int RC, int RP, int WP>
static bool launch_ring_n(const ConvArgs& a, int out_kind, int nsc, dim3 grid, size_t lds, int nslot, hipStream_t s) {
  if constexpr (RC * 4 <= 16)
    if (nsc == 4) return launch_ring_o<RC, RP, WP, 4>(a, out_kind, grid, lds, nslot, s), true;
  if constexpr (RC * 6 <= 16 && 2 * WP * RP * 16 * 3 * 128 <= 64 * 1024)
    if (nsc == 6) return launch_ring_o<RC, RP, WP, 6>(a, out_kind, grid, lds, nslot, s), true;
  if constexpr (RC * 8 <= 16 && 2 * WP * RP * 16 * 4 * 128 <= 64 * 1024)
    if (nsc == 8) return launch_ring_o<RC, RP, WP, 8>(a, out_kind, grid, lds, nslot, s), true;
  if (nsc != 2) return false;
  launch_ring_o<RC, RP, WP, 2>(a, out_kind, grid, lds, nslot, s);
  return true;
}

static int launch_ring(const ConvArgs& a0, int out_kind, int rc, int rp, int wp, hipStream_t s) {
  FCE_CHECK(ring_ok(a0.nsteps, rc, rp, wp), "conv 1x1 ring: bad configuration");
  ConvArgs a = a0;
  const int cotiles = (a.cout + 15) / 16, cb = (4 / wp) * rc, tpb = wp * rp * 16;
  a.gx = (a.P + tpb - 1) / tpb;
  a.gy = (cotiles + cb - 1) / cb;
  const int nsc = ring_nsc(a.nsteps);
  const size_t lds = 2 * lds1_bytes(rp, wp, nsc);
  FCE_CHECK(int64_t(8) * a.gy * cus_per_xcd() * 8 < (int64_t(1) << 31), "conv 1x1 ring: grid too large");
  const int nslot = 0;  // per instantiation, from its occupancy (launch_ring_o)
  const dim3 grid(1);
  bool ok;
  if (rc == 1 && rp == 4 && wp == 1) ok = launch_ring_n<1, 4, 1>(a, out_kind, nsc, grid, lds, nslot, s);
  else if (rc == 2 && rp == 4 && wp == 1) ok = launch_ring_n<2, 4, 1>(a, out_kind, nsc, grid, lds, nslot, s);
  else if (rc == 2 && rp == 2 && wp == 2) ok = launch_ring_n<2, 2, 2>(a, out_kind, nsc, grid, lds, nslot, s);
  else if (rc == 1 && rp == 4 && wp == 2) ok = launch_ring_n<1, 4, 2>(a, out_kind, nsc, grid, lds, nslot, s);
  else if (rc == 1 && rp == 2 && wp == 4) ok = launch_ring_n<1, 2, 4>(a, out_kind, nsc, grid, lds, nslot, s);
  else if (rc == 4 && rp == 1 && wp == 4) ok = launch_ring_n<4, 1, 4>(a, out_kind, nsc, grid, lds, nslot, s);
  else ok = launch_ring_n<4, 2, 4>(a, out_kind, nsc, grid, lds, nslot, s);
  FCE_CHECK(ok, "conv 1x1 ring: no instantiation for this K depth");
  return launch_status("conv1x1_ring_kernel");
}

static int launch_lds1(const ConvArgs& a0, int out_kind, int rc, int rp, int wp, hipStream_t s) {
  FCE_CHECK(lds1_cfg_ok(rc, rp, wp), "conv 1x1 LDS tile: bad configuration");
  ConvArgs a = a0;
  const int cotiles = (a.cout + 15) / 16, cb = (4 / wp) * rc, tpb = wp * rp * 16;
  a.gx = (a.P + tpb - 1) / tpb;
  a.gy = (cotiles + cb - 1) / cb;
  FCE_CHECK(int64_t(a.gx) * a.gy < (int64_t(1) << 31), "conv 1x1 LDS tile: grid too large");
  const int nsc = lds1_nsc(a.nsteps, rc);
  const size_t lds = std::max(lds1_bytes(rp, wp, nsc), a.stg ? lds1_out_bytes(rc, rp, wp) : size_t(0));
  const dim3 grid(unsigned(a.gx * a.gy));
  if (rc == 1 && rp == 4 && wp == 1) launch_lds1_n<1, 4, 1>(a, out_kind, nsc, grid, lds, s);
  else if (rc == 2 && rp == 4 && wp == 1) launch_lds1_n<2, 4, 1>(a, out_kind, nsc, grid, lds, s);
  else if (rc == 2 && rp == 2 && wp == 2) launch_lds1_n<2, 2, 2>(a, out_kind, nsc, grid, lds, s);
  else if (rc == 1 && rp == 4 && wp == 2) launch_lds1_n<1, 4, 2>(a, out_kind, nsc, grid, lds, s);
  else if (rc == 1 && rp == 2 && wp == 4) launch_lds1_n<1, 2, 4>(a, out_kind, nsc, grid, lds, s);
  else if (rc == 4 && rp == 1 && wp == 4) launch_lds1_n<4, 1, 4>(a, out_kind, nsc, grid, lds, s);
  else launch_lds1_n<4, 2, 4>(a, out_kind, nsc, grid, lds, s);
  return launch_status("conv1x1_lds_kernel");
}

// ============================================================================ 1x1, big tiles, K-pipelined
// For the wide 1x1 convs of the m/l scales (cin, cout >= 64: up to tens of K-steps per output), where
// conv1x1_lds_kernel's 64-cout blocks re-stage each pixel tile once per cout group and wait on every
// chunk's loads.  Each wave owns RC=4 cout tiles x RP=4 pixel groups (64 x 64 outputs: 16 MFMAs per
// K-step per 4 A + 4 B fragment reads); the block (4 waves, WP of them along pixels) owns TPB = WP*64
// pixels x CBT = (4/WP)*4 cout tiles.  The K loop walks pairs of steps (64 channels): per pair the block
// stages its B rows (TPB x 128 B, the swizzled image of conv1x1_lds_kernel) and its A fragments (CBT x
// 2 x 1 KiB, packed order) in one of two LDS buffers with coalesced 16-byte loads, 8 per thread.  Two
// pairs are in flight in registers: the loads of pair k+2 are issued before pair k's MFMAs, pair k+1's
// registers are stored to the other buffer after them, one barrier per pair, so each load has two
// compute phases to land.  Per-output K order (steps 0..nsteps-1) is the implicit-GEMM kernel's:
// bitwise identical to every other variant.
template <int WP, int OUT>
__global__ __launch_bounds__(256, 2) void conv1x1_pipe_kernel(ConvArgs a) {
  constexpr int RC = 4, RP = 4;
  constexpr int TPB = WP * RP * 16;
  constexpr int CBT = (4 / WP) * RC;
  constexpr int BB = TPB * 8;        // h8 of B per buffer (one pair of steps)
  constexpr int AB = CBT * 2 * 64;   // h8 of A per buffer
  constexpr int BUF = BB + AB;
  constexpr int ITB = BB / 256, ITA = AB / 256, IT = ITB + ITA;
  static_assert(BB % 256 == 0 && AB % 256 == 0, "whole staging rounds");
  extern __shared__ __attribute__((aligned(16))) h8 xp[];  // [2][B image | A fragments]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int wc = wave / WP, wp = wave - wc * WP;
  int bx, by;  // XCD-aware order: a pixel tile's cout groups share an XCD's L2
  {
    const int total = a.gx * a.gy, b = blockIdx.x;
    const int per = total >> 3, body = per << 3;
    const int L = b < body ? (b & 7) * per + (b >> 3) : b;
    bx = L / a.gy;
    by = L - bx * a.gy;
  }
  const int pix0 = bx * TPB;
  const int cbl0 = by * CBT;
  const int cotiles = (a.cout + 15) >> 4;
  // staging pieces: B piece e = threadIdx.x + 256 i -> pixel e >> 3, 16-byte piece j = e & 7 of its
  // 128-byte pair; A piece e -> cout tile e >> 7, step (e >> 6) & 1, lane e & 63 (2 KiB per tile)
  const h8* sptr[IT];
  int spos[IT], sch[ITB];
  bool spv[ITB];
#pragma unroll
  for (int i = 0; i < ITB; ++i) {
    const int e = threadIdx.x + 256 * i;
    const int j = e & 7, p = e >> 3;
    const int pix = pix0 + p;
    spv[i] = pix < a.P;
    sptr[i] = reinterpret_cast<const h8*>(a.x + conv1x1_src(a, spv[i] ? pix : 0) + j * 8);
    sch[i] = j * 8;
    spos[i] = p * 8 + (j ^ ((p >> 1) & 7));
  }
#pragma unroll
  for (int i = 0; i < ITA; ++i) {
    const int e = threadIdx.x + 256 * i;
    const int t = e >> 7, sl = e & 127;  // sl = step * 64 + lane
    sptr[ITB + i] = reinterpret_cast<const h8*>(a.w) + size_t(min(cbl0 + t, cotiles - 1)) * a.nalloc * 64 + sl;
    spos[ITB + i] = BB + e;
  }
  auto load = [&](int k0, h8 (&v)[IT]) {  // packed A is zero-padded past nsteps: in bounds
    const int cbase = k0 * 32;
#pragma unroll
    for (int i = 0; i < ITB; ++i) {
      const bool ok = spv[i] && cbase + sch[i] < a.cin;
      v[i] = *(ok ? sptr[i] + cbase / 8 : reinterpret_cast<const h8*>(g_zero_line));
    }
#pragma unroll
    for (int i = 0; i < ITA; ++i) v[ITB + i] = sptr[ITB + i][size_t(k0) * 64];
  };
  auto store = [&](int buf, const h8 (&v)[IT]) {
#pragma unroll
    for (int i = 0; i < IT; ++i) xp[buf * BUF + spos[i]] = v[i];
  };
  f4 acc[RC][RP];
#pragma unroll
  for (int r = 0; r < RC; ++r)
#pragma unroll
    for (int p = 0; p < RP; ++p) acc[r][p] = f4{0.f, 0.f, 0.f, 0.f};
  const int pw = wp * RP * 16;
  const int npair = (a.nsteps + 1) >> 1;
  h8 v0[IT], v1[IT];
  load(0, v0);
  if (npair > 1) load(2, v1);
  store(0, v0);
  __syncthreads();
  for (int k = 0; k < npair; ++k) {
    const int cur = k & 1;
    if (k + 2 < npair) load(2 * (k + 2), v0);  // v0 was stored last iteration
    const int nsc = min(2, a.nsteps - 2 * k);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s < nsc) {
        h8 af[RC], bf[RP];
#pragma unroll
        for (int r = 0; r < RC; ++r) af[r] = xp[cur * BUF + BB + ((wc * RC + r) * 2 + s) * 64 + lane];
#pragma unroll
        for (int p = 0; p < RP; ++p) {
          const int px = pw + p * 16 + col;
          const int j = s * 4 + grp;
          bf[p] = xp[cur * BUF + px * 8 + (j ^ ((px >> 1) & 7))];
        }
#pragma unroll
        for (int r = 0; r < RC; ++r)
#pragma unroll
          for (int p = 0; p < RP; ++p)
            acc[r][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[r], bf[p], acc[r][p], 0, 0, 0);
      }
    }
    if (k + 1 < npair) store(cur ^ 1, v1);
    __syncthreads();  // pair k's reads and pair k+1's stores done
#pragma unroll
    for (int i = 0; i < IT; ++i) v1[i] = v0[i];
  }
  if constexpr (OUT == OUT_F16 || OUT == OUT_WSTORE) {
    if (a.stg) {  // launch_pipe1 sizes the LDS for the output tile too (TPB x CBT*16 couts x 2 bytes)
      conv_store_staged<RC, RP, CBT, TPB, OUT>(a, acc, pix0, pw, cbl0, wc, col, grp, reinterpret_cast<_Float16*>(xp));
      return;
    }
  }
  conv_epilogue<RC, RP, OUT>(a, acc, pix0 + pw, cbl0 + wc * RC, col, grp);
}

// big-tile configurations (their code: pipe1_encode below; rc = rp = 4)
static bool pipe1_ok(const fce_conv_desc& d, int det_box) {
  return d.k == 1 && d.stride == 1 && !det_box && d.cout >= 64 && d.cin >= 64;
}

template <int WP>
static int launch_pipe1_w(const ConvArgs& a, int out_kind, dim3 grid, size_t lds, hipStream_t s) {
#define PIPE1_L(O)                                                                                      \
  {                                                                                                     \
    static const bool lds_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_pipe_kernel<WP, O>), \
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024) == hipSuccess; \
    FCE_CHECK(lds_ok || lds <= 64 * 1024, "conv 1x1 big tile: cannot opt in to >64 KiB LDS");          \
    FCE_LAUNCH((conv1x1_pipe_kernel<WP, O>), grid, dim3(256), lds, s, a);                               \
  }
  switch (out_kind) {
    case OUT_F16: PIPE1_L(OUT_F16); break;
    case OUT_F32: PIPE1_L(OUT_F32); break;
    case OUT_WSTORE: PIPE1_L(OUT_WSTORE); break;
    case OUT_CLS: PIPE1_L(OUT_CLS); break;
    default: PIPE1_L(OUT_ACCUM); break;
  }
#undef PIPE1_L
  return FCE_OK;
}

static int launch_pipe1(const ConvArgs& a0, int out_kind, int wp, hipStream_t s) {
  FCE_CHECK(out_kind != OUT_DFL && (wp == 1 || wp == 2 || wp == 4), "conv 1x1 big tile: bad configuration");
  ConvArgs a = a0;
  const int cotiles = (a.cout + 15) / 16, cb = (4 / wp) * 4, tpb = wp * 64;
  a.gx = (a.P + tpb - 1) / tpb;
  a.gy = (cotiles + cb - 1) / cb;
  FCE_CHECK(int64_t(a.gx) * a.gy < (int64_t(1) << 31), "conv 1x1 big tile: grid too large");
  const size_t lds = std::max(size_t(2) * (tpb * 128 + cb * 2048), a.stg ? size_t(tpb) * cb * 16 * 2 : size_t(0));
  const dim3 grid(unsigned(a.gx * a.gy));
  const int st = wp == 1 ? launch_pipe1_w<1>(a, out_kind, grid, lds, s)
                 : wp == 2 ? launch_pipe1_w<2>(a, out_kind, grid, lds, s)
                           : launch_pipe1_w<4>(a, out_kind, grid, lds, s);
  if (st != FCE_OK) return st;
  return launch_status("conv1x1_pipe_kernel");
}

// ============================================================================ family: streaming 1x1 (kind 3)
// coded 0x300 | rc | rp << 4
struct Stream1Cfg {
  int rc, rp;
};
static int stream1_encode(Stream1Cfg c) { return 0x300 | c.rc | (c.rp << 4); }
static Stream1Cfg stream1_decode(int code) { return {code & 15, (code >> 4) & 15}; }
static bool stream1_ok(const fce_conv_desc& d, int rc, int rp) {
  return d.k == 1 && d.cin % 32 == 0 && (rc == 1 || rc == 2 || rc == 4) && (rp == 1 || rp == 2);
}

void stream1_offer(const fce_conv_desc& d, int det_box, CodeList& out) {
  const int cotiles = (d.cout + 15) / 16, nsm = stream_nsm(d.cin / 32);
  for (int rc : {1, 2, 4}) {
    if (det_box ? rc != 4 : !cotiles_want(rc, cotiles)) continue;
    for (int rp : {1, 2})
      if (stream1_ok(d, rc, rp) && nsm > 0 && stream_ok(nsm, rc, rp)) out.add(stream1_encode({rc, rp}));
  }
}

int stream1_launch(const ConvCall& c, int code) {
  const Stream1Cfg t = stream1_decode(code);
  FCE_CHECK(stream1_ok(c.d, t.rc, t.rp), "conv: bad stream hint");
  if (c.out_kind == OUT_DFL) FCE_CHECK(t.rc == 4 && c.g.cotiles == 4, "conv detect epilogue: one wave must own all 64 bins");
  return launch_stream(c.a, c.out_kind, t.rc, t.rp, c.s);
}

// ============================================================================ families: LDS-staged 1x1 (kind 4), ring (kind 5)
// coded 0x400 | rc | rp << 4 | log2(wp) << 12, the persistent ring 0x500 | the same bits
struct Lds1Cfg {
  int rc, rp, wp;
};
static int lds1_bits(Lds1Cfg c) { return c.rc | (c.rp << 4) | (ilog2(c.wp) << 12); }
static int lds1_encode(Lds1Cfg c) { return 0x400 | lds1_bits(c); }
static int ring1_encode(Lds1Cfg c) { return 0x500 | lds1_bits(c); }
static Lds1Cfg lds1_decode(int code) { return {code & 15, (code >> 4) & 15, 1 << ((code >> 12) & 3)}; }
static bool lds1_ok(const fce_conv_desc& d, const Lds1Cfg& t) {
  return d.k == 1 && d.stride == 1 && lds1_cfg_ok(t.rc, t.rp, t.wp);
}
static bool ring1_ok(const fce_conv_desc& d, const Lds1Cfg& t) {
  return d.k == 1 && d.stride == 1 && ring_ok(dense_geom(d).nsteps, t.rc, t.rp, t.wp);
}

// both list wp-major; the Detect box conv needs one wave to own all 64 bins (rc 4, wp 4)
static void lds1_offer_as(int (*encode)(Lds1Cfg), bool (*ok)(const fce_conv_desc&, const Lds1Cfg&),
                          const fce_conv_desc& d, int det_box, CodeList& out) {
  const int cotiles = (d.cout + 15) / 16;
  for (int wp : {1, 2, 4})
    for (int rc : {1, 2, 4})
      for (int rp : {1, 2, 4}) {
        const Lds1Cfg t{rc, rp, wp};
        if (!ok(d, t)) continue;
        if (det_box ? (rc != 4 || wp != 4) : !cotiles_want((4 / wp) * rc, cotiles)) continue;
        out.add(encode(t));
      }
}
void lds1_offer(const fce_conv_desc& d, int det_box, CodeList& out) { lds1_offer_as(lds1_encode, lds1_ok, d, det_box, out); }
void ring1_offer(const fce_conv_desc& d, int det_box, CodeList& out) {
  if (!no_ring()) lds1_offer_as(ring1_encode, ring1_ok, d, det_box, out);
}

int lds1_launch(const ConvCall& c, int code) {
  const Lds1Cfg t = lds1_decode(code);
  FCE_CHECK(lds1_ok(c.d, t), "conv: bad LDS 1x1 hint");
  if (c.out_kind == OUT_DFL)
    FCE_CHECK(t.rc == 4 && t.wp == 4 && c.g.cotiles == 4, "conv detect epilogue: one wave must own all 64 bins");
  return launch_lds1(c.a, c.out_kind, t.rc, t.rp, t.wp, c.s);
}

int ring1_launch(const ConvCall& c, int code) {
  const Lds1Cfg t = lds1_decode(code);
  FCE_CHECK(ring1_ok(c.d, t), "conv: bad 1x1 ring hint");
  if (c.out_kind == OUT_DFL)
    FCE_CHECK(t.rc == 4 && t.wp == 4 && c.g.cotiles == 4, "conv detect epilogue: one wave must own all 64 bins");
  return launch_ring(c.a, c.out_kind, t.rc, t.rp, t.wp, c.s);
}

// ============================================================================ family: K-pipelined big-tile 1x1 (kind 7)
// coded 0x700 | log2(wp) << 12 (rc = rp = 4; the low byte stays 0)
struct Pipe1Cfg {
  int wp, low;
};
static int pipe1_encode(int wp) { return 0x700 | (ilog2(wp) << 12); }
static Pipe1Cfg pipe1_decode(int code) { return {1 << ((code >> 12) & 3), code & 0xFF}; }

void pipe1_offer(const fce_conv_desc& d, int det_box, CodeList& out) {
  if (!pipe1_ok(d, det_box)) return;
  const int cotiles = (d.cout + 15) / 16;
  for (int wp : {1, 2, 4})
    if (cotiles_want((4 / wp) * 4, cotiles)) out.add(pipe1_encode(wp));
}

int pipe1_launch(const ConvCall& c, int code) {
  const Pipe1Cfg t = pipe1_decode(code);
  FCE_CHECK(pipe1_ok(c.d, c.out_kind == OUT_DFL) && t.low == 0 && t.wp <= 4, "conv: bad big-tile 1x1 hint");
  return launch_pipe1(c.a, c.out_kind, t.wp, c.s);
}

}  // namespace fce

