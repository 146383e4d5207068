// Persistent 3x3 convolution rings for cin 32 / 64: A fragments in registers, the staged input double-buffered in
// LDS.  The 16x16x32 register ring (0x600) and the 32x32x16 ring (0x900, opt-in); each family's encode / decode pair,
// capability predicate, offer() and launch() close the file (conv_variant.h).
// Replaces (reference, ultralytics/): nn/modules/conv.py:39-89 Conv.forward_fuse (3x3, BN folded by
// utils/torch_utils.py:237-267) and Bottleneck's residual add (block.py:474-476).
#include "conv_variant.h"

namespace fce {

// ============================================================================ 3x3, persistent, A in registers
// For cin = 32 * NCH (NCH = 1, 2: the 32/64-channel 3x3 convs of the n/s scales, which the tile kernels
// run far below the MFMA rate because every wave re-reads its weight fragments from L2 for each
// 64-pixel tile).  Each wave owns ONE cout tile and keeps its 9 * NCH A fragments in registers for the
// whole launch; the block (4 cout tiles) walks a sequence of TH = RP row x 16 column output tiles,
// staging each tile's input (+ halo, all cin, 64 * NCH bytes per pixel, the swizzled image of the tile
// kernels) in one of two LDS buffers while the previous tile computes (the next tile's global loads are
// issued before this tile's MFMAs).  Block b: XCD b % 8, cout group, slot; XCD x owns the contiguous tile
// range [x chunk, (x + 1) chunk) and its slot-th blocks take tiles x chunk + slot + k nslot, so the tiles
// whose halos overlap are in flight on one XCD's L2 at the same time.
// K order (chunk, tap) is the implicit-GEMM kernel's: bitwise identical.
// PD = 2 (round 4): two register sets of staged input, the loop unrolled by two so each set's loads are issued two
// tiles ahead of their LDS store (two compute phases to land instead of one).
template <int S, int RP, int NCH, int PD = 1>
__global__ __launch_bounds__(256) void conv3x3_ring_kernel(ConvArgs a, int nslot) {
  constexpr int TW = 16, TH = RP;
  constexpr int RI = (TH - 1) * S + 3, CI = (TW - 1) * S + 3;
  // BUF = NL * 256 >= NE: slots past NE absorb the dummy pieces of the last staging round, so every
  // staging load and LDS store is unconditional (a guarded store lets hipcc sink the load under a
  // branch and serialise the loads with vmcnt waits)
  constexpr int NQ = 4 * NCH, NE = RI * CI * NQ, NL = (NE + 255) / 256, BUF = NL * 256;
  constexpr int KP = NCH;  // slot swizzle of the tile kernels for 4 * NCH pieces per pixel
  __shared__ __attribute__((aligned(16))) h8 tile[2 * BUF];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
  const int by = loc % a.gy, slot = loc / a.gy;
  const int tiles_x = (a.Wo + TW - 1) / TW, tiles_y = (a.Ho + TH - 1) / TH;
  const int ntiles = tiles_x * tiles_y * a.N;
  const int chunk = (ntiles + 7) >> 3, tend = min(ntiles, (xcd + 1) * chunk);
  int t = xcd * chunk + slot;
  if (t >= tend) return;  // block-uniform
  const int cot0 = by * 4 + wave;
  const int cotiles = (a.cout + 15) >> 4;
  h8 af[NCH * 9];
  {
    const h8* wf = reinterpret_cast<const h8*>(a.w) + (size_t(min(cot0, cotiles - 1)) * a.nalloc) * 64 + lane;
#pragma unroll
    for (int k = 0; k < NCH * 9; ++k) af[k] = wf[k * 64];
  }
  auto stage_load = [&](int tt, h8 (&v)[NL], int (&sl)[NL]) {
    const int tx = tt % tiles_x, r0 = tt / tiles_x, ty = r0 % tiles_y, n = r0 / tiles_y;
    const int iy0 = ty * TH * S - 1, ix0 = tx * TW * S - 1;
    const _Float16* xn = a.x + int64_t(n) * a.Hs * a.Ws * a.xcs;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int e = threadIdx.x + 256 * i;
      const int pc = e / NQ, q = e - pc * NQ;
      const int r = pc / CI, c = pc - r * CI;
      const int iy = iy0 + r, ix = ix0 + c;
      const int u = r * CI + tile_col<S, CI>(c);
      sl[i] = e < NE ? u * NQ + tile_slot<KP>(u, q) : e;
      const bool ok = e < NE && iy >= 0 && iy < a.Hs && ix >= 0 && ix < a.Ws;
      v[i] = *(ok ? reinterpret_cast<const h8*>(xn + (int64_t(iy) * a.Ws + ix) * a.xcs + q * 8)
                  : reinterpret_cast<const h8*>(g_zero_line));
    }
  };
  h8 v[NL], v2[NL];
  int sl[NL], sl2[NL];
  const int step = nslot;
  // one tile: vv holds its staged input; vv is then reloaded with the tile PD steps on
  auto iter = [&](h8 (&vv)[NL], int (&ss)[NL], int cur) {
#pragma unroll
    for (int i = 0; i < NL; ++i) tile[cur * BUF + ss[i]] = vv[i];
    __syncthreads();
    const int tx = t % tiles_x, r0 = t / tiles_x, ty = r0 % tiles_y, n = r0 / tiles_y;
    Tile3Pre<RP> pre;  // residual + bias, issued before the prefetch (see tile3_pre)
    tile3_pre<RP>(a, n, ty * TH, tx * TW, cot0, grp, col, pre);
    // unconditional (clamped to the last tile, whose loads are then unused): a prefetch under a branch leaves the
    // waitcnt pass a join with nothing in flight on one side, and it waits vmcnt(0) for the residual there
    stage_load(min(t + PD * step, tend - 1), vv, ss);
    f4 acc[RP];
#pragma unroll
    for (int p = 0; p < RP; ++p) acc[p] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
        for (int p = 0; p < RP; ++p) {
          const int u = (p * S + ky) * CI + tile_col<S, CI>(col * S + kx);
          const h8 bf = tile[cur * BUF + u * NQ + tile_slot<KP>(u, k * 4 + grp)];
          acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[k * 9 + tap], bf, acc[p], 0, 0, 0);
        }
      }
    tile3_post<RP>(a, acc, pre, n, ty * TH, tx * TW, cot0, col, grp);
    t += step;
  };
  stage_load(t, v, sl);
  if (PD == 1) {
    for (int cur = 0; t < tend; cur ^= 1) iter(v, sl, cur);
  } else {
    if (t + step < tend) stage_load(t + step, v2, sl2);
    for (int cur = 0; t < tend;) {
      iter(v, sl, cur);
      cur ^= 1;
      if (t >= tend) break;
      iter(v2, sl2, cur);
      cur ^= 1;
    }
  }
}

// ============================================================================ 3x3, persistent, 32x32x16 MFMA
// The ring above on v_mfma_f32_32x32x16_f16: a wave owns 32 couts x 32 pixels (2 rows x 16 columns) per MFMA, so each
// B fragment read from LDS (1 KiB: 16 k x 32 pixels) feeds 32 x 32 x 16 MACs instead of 16 x 16 x 32 -- half the LDS
// bytes per MAC, the ring's bound on the 64 -> 64 convs.  Bitwise identical to the 16x16x32 variants:
// each 32-deep K-step runs as two 32x32x16 MFMAs over its chunks (4s, 4s+1) then (4s+2, 4s+3), which is how
// v_mfma_f32_16x16x32_f16 sums a step (profiles/r05_mfma_order.txt: 0 of 200 000 random steps differ).
// Block: WC waves along the couts (32 each) x WR = 4 / WC along the rows, RPW 2-row pixel tiles per wave: a tile is
// TH = 2 RPW WR rows x 16 columns, staged like the ring's (swizzled halo image, double-buffered LDS, the next tile's
// loads issued before this tile's MFMAs).  A: lane l holds cout cb + (l & 31) and chunk 4 s + 2 h + (l >> 5) of
// K-step s, i.e. lane (l & 15) + 16 (l >> 5) + 32 h of the packed 16x16x32 fragment of cout tile (cb + (l & 31)) / 16.
// D: register r of lane l is cout cb + 8 (r / 4) + 4 (l >> 5) + r % 4, pixel l & 31.
typedef float f16v __attribute__((ext_vector_type(16)));

// the double-buffered staged tile of a ring32 configuration fits the 64 KiB of static LDS
static constexpr bool ring32_fits(int s, int nch, int wc, int rpw) {
  return wc >= 1 && 2 * ((((2 * rpw * (4 / wc) - 1) * s + 3) * (15 * s + 3) * 4 * nch + 255) / 256) * 256 * 16 <= 64 * 1024;
}

template <int S, int NCH, int WC, int RPW>
__global__ __launch_bounds__(256) void conv3x3_ring32_kernel(ConvArgs a, int nslot) {
  constexpr int WR = 4 / WC, TW = 16, TH = 2 * RPW * WR;
  constexpr int RI = (TH - 1) * S + 3, CI = (TW - 1) * S + 3;
  constexpr int NQ = 4 * NCH, NE = RI * CI * NQ, NL = (NE + 255) / 256, BUF = NL * 256;
  constexpr int KP = NCH;
  __shared__ __attribute__((aligned(16))) h8 tile[2 * BUF];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wc = wave % WC, wr = wave / WC, hi = lane >> 5;
  const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
  const int by = loc % a.gy, slot = loc / a.gy;
  const int tiles_x = (a.Wo + TW - 1) / TW, tiles_y = (a.Ho + TH - 1) / TH;
  const int ntiles = tiles_x * tiles_y * a.N;
  const int chunk = (ntiles + 7) >> 3, tend = min(ntiles, (xcd + 1) * chunk);
  int t = xcd * chunk + slot;
  if (t >= tend) return;  // block-uniform
  const int cb = (by * WC + wc) * 32;  // the wave's first cout
  const int cotiles = (a.cout + 15) >> 4;
  h8 af[NCH * 9][2];
  {
    const int ct = min((cb + (lane & 31)) >> 4, cotiles - 1);
    const h8* wf = reinterpret_cast<const h8*>(a.w) + size_t(ct) * a.nalloc * 64 + (lane & 15) + 16 * hi;
#pragma unroll
    for (int k = 0; k < NCH * 9; ++k) {
      af[k][0] = wf[k * 64];
      af[k][1] = wf[k * 64 + 32];
    }
  }
  float bz[4][4];  // the wave's biases: couts cb + 8 g + 4 hi + j
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int j = 0; j < 4; ++j) bz[g][j] = bias_or0(a.bias, cb + 8 * g + 4 * hi + j, a.cout);
  const bool vres = a.res && a.vec_ok;
  auto stage_load = [&](int tt, h8 (&v)[NL], int (&sl)[NL]) {
    const int tx = tt % tiles_x, r0 = tt / tiles_x, ty = r0 % tiles_y, n = r0 / tiles_y;
    const int iy0 = ty * TH * S - 1, ix0 = tx * TW * S - 1;
    const _Float16* xn = a.x + int64_t(n) * a.Hs * a.Ws * a.xcs;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int e = threadIdx.x + 256 * i;
      const int pc = e / NQ, q = e - pc * NQ;
      const int r = pc / CI, c = pc - r * CI;
      const int iy = iy0 + r, ix = ix0 + c;
      const int u = r * CI + tile_col<S, CI>(c);
      sl[i] = e < NE ? u * NQ + tile_slot<KP>(u, q) : e;
      const bool ok = e < NE && iy >= 0 && iy < a.Hs && ix >= 0 && ix < a.Ws;
      v[i] = *(ok ? reinterpret_cast<const h8*>(xn + (int64_t(iy) * a.Ws + ix) * a.xcs + q * 8)
                  : reinterpret_cast<const h8*>(g_zero_line));
    }
  };
  h8 v[NL];
  int sl[NL];
  const int step = nslot;
  stage_load(t, v, sl);
  for (int cur = 0; t < tend; cur ^= 1) {
#pragma unroll
    for (int i = 0; i < NL; ++i) tile[cur * BUF + sl[i]] = v[i];
    __syncthreads();
    const int tx = t % tiles_x, r0 = t / tiles_x, ty = r0 % tiles_y, n = r0 / tiles_y;
    // residuals of the wave's outputs (clamped, unconditional), issued before the prefetch: vmcnt retires in order
    h4 rres[RPW][4];
    if (vres) {
#pragma unroll
      for (int p = 0; p < RPW; ++p) {
        const int px = lane & 31;
        const int oy = min(ty * TH + (wr * RPW + p) * 2 + (px >> 4), a.Ho - 1), ox = min(tx * TW + (px & 15), a.Wo - 1);
        const int64_t pix = (int64_t(n) * a.Ho + oy) * a.Wo + ox;
#pragma unroll
        for (int g = 0; g < 4; ++g)
          rres[p][g] = *reinterpret_cast<const h4*>(a.res + pix * a.rcs + min(cb + 8 * g + 4 * hi, (a.cout - 4) & ~3));
      }
    }
    stage_load(min(t + step, tend - 1), v, sl);  // unconditional (clamped): see conv3x3_ring_kernel
    f16v acc[RPW];
#pragma unroll
    for (int p = 0; p < RPW; ++p)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[p][j] = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
        for (int p = 0; p < RPW; ++p) {
          const int px = lane & 31, rr = (wr * RPW + p) * 2 + (px >> 4);
          const int u = (rr * S + ky) * CI + tile_col<S, CI>((px & 15) * S + kx);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const h8 bf = tile[cur * BUF + u * NQ + tile_slot<KP>(u, k * 4 + 2 * h + hi)];
            acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[k * 9 + tap][h], bf, acc[p], 0, 0, 0);
          }
        }
      }
    // epilogue: tile3_post's arithmetic (bias, SiLU, residual, fp16)
#pragma unroll
    for (int p = 0; p < RPW; ++p) {
      const int px = lane & 31;
      const int oy = ty * TH + (wr * RPW + p) * 2 + (px >> 4), ox = tx * TW + (px & 15);
      if (oy >= a.Ho || ox >= a.Wo) continue;
      const int64_t pix = (int64_t(n) * a.Ho + oy) * a.Wo + ox;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int co0 = cb + 8 * g + 4 * hi;
        if (co0 >= a.cout) continue;
        float vv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float tt = acc[p][4 * g + j] + bz[g][j];
          vv[j] = a.act ? silu(tt) : tt;
        }
        _Float16* yo = static_cast<_Float16*>(a.y) + pix * a.ycs + co0;
        const bool vec = a.vec_ok && co0 + 3 < a.cout;
        if (a.res) {
          if (vec && vres) {
#pragma unroll
            for (int j = 0; j < 4; ++j) vv[j] = fpin(vv[j] + (float)rres[p][g][j]);
          } else {
            const _Float16* ro = a.res + pix * a.rcs + co0;
            for (int j = 0; j < 4; ++j)
              if (co0 + j < a.cout) vv[j] = fpin(vv[j] + (float)ro[j]);
          }
        }
        if (vec) {
          *reinterpret_cast<h4*>(yo) = h4{(_Float16)fpin(vv[0]), (_Float16)fpin(vv[1]), (_Float16)fpin(vv[2]), (_Float16)fpin(vv[3])};
        } else {
          for (int j = 0; j < 4; ++j)
            if (co0 + j < a.cout) yo[j] = (_Float16)fpin(vv[j]);
        }
      }
    }
    t += step;
  }
}

template <int S, int RP, int NCH, int PD>
static void launch_ring3_k(const ConvArgs& a, dim3, int ntiles, hipStream_t s) {
  static const int occ = blocks_per_cu(conv3x3_ring_kernel<S, RP, NCH, PD>, 0);
  const int nslot = ring_slots(ntiles, a.gy, occ);
  FCE_LAUNCH((conv3x3_ring_kernel<S, RP, NCH, PD>), dim3(unsigned(8 * a.gy * nslot)), dim3(256), 0, s, a, nslot);
}

template <int S, int NCH>
static void launch_ring3_s(const ConvArgs& a, int rp, int pd, dim3 grid, int nslot, hipStream_t s) {
  if (pd == 2) {
    if (rp == 1)
      launch_ring3_k<S, 1, NCH, 2>(a, grid, nslot, s);
    else if (rp == 2)
      launch_ring3_k<S, 2, NCH, 2>(a, grid, nslot, s);
    else
      launch_ring3_k<S, 4, NCH, 2>(a, grid, nslot, s);
  } else if (rp == 1) {
    launch_ring3_k<S, 1, NCH, 1>(a, grid, nslot, s);
  } else if (rp == 2) {
    launch_ring3_k<S, 2, NCH, 1>(a, grid, nslot, s);
  } else {
    launch_ring3_k<S, 4, NCH, 1>(a, grid, nslot, s);
  }
}


template <int S, int NCH, int WC, int RPW>
static void launch_ring32_k(const ConvArgs& a, int ntiles, hipStream_t s) {
  if constexpr (!ring32_fits(S, NCH, WC, RPW)) {
    return;  // not a candidate (ring32_offer checks ring32_fits)
  } else {
  static const int occ = blocks_per_cu(conv3x3_ring32_kernel<S, NCH, WC, RPW>, 0);
  const int nslot = ring_slots(ntiles, a.gy, occ);
  FCE_LAUNCH((conv3x3_ring32_kernel<S, NCH, WC, RPW>), dim3(unsigned(8 * a.gy * nslot)), dim3(256), 0, s, a, nslot);
  }
}

template <int S, int NCH>
static void launch_ring32_s(const ConvArgs& a, int wc, int rpw, int ntiles, hipStream_t s) {
  if (wc == 1)
    rpw == 1 ? launch_ring32_k<S, NCH, 1, 1>(a, ntiles, s) : launch_ring32_k<S, NCH, 1, 2>(a, ntiles, s);
  else if (wc == 2)
    rpw == 1 ? launch_ring32_k<S, NCH, 2, 1>(a, ntiles, s) : launch_ring32_k<S, NCH, 2, 2>(a, ntiles, s);
  else
    rpw == 1 ? launch_ring32_k<S, NCH, 4, 1>(a, ntiles, s) : launch_ring32_k<S, NCH, 4, 2>(a, ntiles, s);
}

static int launch_ring32(const ConvArgs& a0, int wc, int rpw, int stride, hipStream_t s) {
  FCE_CHECK((a0.cin == 32 || a0.cin == 64) && a0.cout % 32 == 0 && (wc == 1 || wc == 2 || wc == 4) &&
                (rpw == 1 || rpw == 2) && (stride == 1 || stride == 2) && ring32_fits(stride, a0.cin / 32, wc, rpw),
            "conv 3x3 ring32: bad configuration");
  ConvArgs a = a0;
  const int th = 2 * rpw * (4 / wc);
  const int64_t ntiles = int64_t((a.Wo + 15) / 16) * ((a.Ho + th - 1) / th) * a.N;
  FCE_CHECK(ntiles < (int64_t(1) << 30), "conv 3x3 ring32: too many tiles");
  a.gy = (a.cout + 32 * wc - 1) / (32 * wc);
  const int nch = a.cin / 32;
  if (stride == 1)
    nch == 1 ? launch_ring32_s<1, 1>(a, wc, rpw, int(ntiles), s) : launch_ring32_s<1, 2>(a, wc, rpw, int(ntiles), s);
  else
    nch == 1 ? launch_ring32_s<2, 1>(a, wc, rpw, int(ntiles), s) : launch_ring32_s<2, 2>(a, wc, rpw, int(ntiles), s);
  return launch_status("conv3x3_ring32_kernel");
}

// pd: tiles of staged input in flight ahead of the LDS store (1, or 2: two register sets)
int launch_ring3(const ConvArgs& a0, int rp, int pd, int stride, hipStream_t s) {
  FCE_CHECK((a0.cin == 32 || a0.cin == 64) && (rp == 1 || rp == 2 || rp == 4), "conv 3x3 ring: bad configuration");
  ConvArgs a = a0;
  const int nch = a.cin / 32;
  const int64_t ntiles = int64_t((a.Wo + 15) / 16) * ((a.Ho + rp - 1) / rp) * a.N;
  FCE_CHECK(ntiles < (int64_t(1) << 30), "conv 3x3 ring: too many tiles");
  a.gy = ((a.cout + 15) / 16 + 3) / 4;
  const int nslot = int(ntiles);  // the leaf launcher turns the tile count into slots (occupancy)
  const dim3 grid(1);
  if (stride == 1)
    nch == 1 ? launch_ring3_s<1, 1>(a, rp, pd, grid, nslot, s) : launch_ring3_s<1, 2>(a, rp, pd, grid, nslot, s);
  else
    nch == 1 ? launch_ring3_s<2, 1>(a, rp, pd, grid, nslot, s) : launch_ring3_s<2, 2>(a, rp, pd, grid, nslot, s);
  return launch_status("conv3x3_ring_kernel");
}

// ============================================================================ family: register ring (kind 6)
// coded 0x600 | rp << 4 | (pd - 1): 0x6x1 keeps two tiles of input in flight; bits 1-3 stay 0
struct Ring3Cfg {
  int rp, pd, rest;
};
static int ring3_encode(int rp, int pd) { return 0x600 | (rp << 4) | (pd - 1); }
static Ring3Cfg ring3_decode(int code) { return {(code >> 4) & 15, (code & 1) ? 2 : 1, code & 14}; }
static bool ring3_ok(const fce_conv_desc& d) { return d.k == 3 && (d.cin == 32 || d.cin == 64) && d.up == 0; }

void ring3_offer(const fce_conv_desc& d, int det_box, CodeList& out) {
  if (!ring3_ok(d) || det_box || no_ring()) return;
  for (int rp : {1, 2, 4})
    for (int pd : {1, 2}) out.add(ring3_encode(rp, pd));
}

int ring3_launch(const ConvCall& c, int code) {
  const Ring3Cfg t = ring3_decode(code);
  FCE_CHECK(ring3_ok(c.d) && c.out_kind == OUT_F16 && t.rest == 0, "conv: bad 3x3 ring hint");
  return launch_ring3(c.a, t.rp, t.pd, c.d.stride, c.s);
}

// ============================================================================ family: 32x32x16 ring (kind 9)
// coded 0x900 | rpw << 4 | log2(wc) << 12; the low nibble stays 0.  Opt-in, FCE_RING32=1 (read per call: the variant
// tests switch it on mid-process): on every shape they apply to in the BASELINE models (the 64 -> 64 Detect box 3x3s,
// the 32 / 64-channel bottlenecks) they ran slower than the 16x16x32 ring, e.g. 33.4 against 23.8 us on n32's P3 box
// convs (256 VGPRs: one wave per SIMD), profiles/r05_ring32_tune.txt
struct Ring32Cfg {
  int wc, rpw, low;
};
static int ring32_encode(int wc, int rpw) { return 0x900 | (rpw << 4) | (ilog2(wc) << 12); }
static Ring32Cfg ring32_decode(int code) { return {1 << ((code >> 12) & 3), (code >> 4) & 15, code & 0xF}; }
static bool ring32_ok(const fce_conv_desc& d) {
  return d.k == 3 && (d.cin == 32 || d.cin == 64) && d.cout % 32 == 0 && d.up == 0;
}

void ring32_offer(const fce_conv_desc& d, int det_box, CodeList& out) {
  if (!ring32_ok(d) || det_box || no_ring() || !env_on("FCE_RING32")) return;
  for (int wc : {1, 2, 4})
    for (int rpw : {1, 2})
      if (((32 * wc) >> 1) < d.cout && ring32_fits(d.stride, d.cin / 32, wc, rpw)) out.add(ring32_encode(wc, rpw));
}

int ring32_launch(const ConvCall& c, int code) {
  const Ring32Cfg t = ring32_decode(code);
  FCE_CHECK(ring32_ok(c.d) && c.out_kind == OUT_F16 && t.low == 0, "conv: bad 3x3 ring32 hint");
  return launch_ring32(c.a, t.wc, t.rpw, c.d.stride, c.s);
}

}  // namespace fce

