// 3x3 convolution on LDS-staged tiles: the halo-tile kernel for cin % 32 == 0 (0x100, with the opt-in A-in-LDS
// form) and the small-cin tile kernel (0x200).  Each family's encode / decode pair, capability predicate, offer() and
// launch() close the file (conv_variant.h).
// Replaces (reference, ultralytics/): nn/modules/conv.py:39-89 Conv.forward_fuse (3x3, BN folded by
// utils/torch_utils.py:237-267) and Bottleneck's residual add (block.py:474-476).
#include "conv_variant.h"

namespace fce {

// ============================================================================ 3x3, LDS halo tiles
// For cin % 32 == 0.  A block (4 waves) owns a 2-D output tile of TW = 16 columns x TH = 4*RP rows
// of one image and RC*16 couts; wave w owns rows [w*RP, w*RP+RP) (one 16-pixel B fragment per row).
// Per 32-channel chunk the input tile + halo ((TH-1)*S+3 x (TW-1)*S+3 pixels x 64 B) is staged in
// LDS once with coalesced 16-byte loads, and all 9 taps read their B fragments from it (a wave
// reads 16 consecutive pixels x 64 B = 1 KiB contiguous per fragment), instead of every tap
// re-fetching the pixels from L2 as the implicit-GEMM kernel does.  A fragments: the same packed
// layout (K-step = chunk * 9 + tap).  Per output element the K order (chunk-major, tap, channel)
// is the implicit-GEMM kernel's, so both kernels give bitwise-identical results.
// Tile-kernel geometry (template): CW waves split the block's cout tiles (CW*RC of them), the other
// 4/CW split its rows (RP rows each, TH = (4/CW)*RP); KP 32-channel chunks are staged per barrier
// (KP = 2: 128 bytes per pixel, full-line loads, half the barriers).  Slot swizzle: tile_slot (conv_args.h).
// AL = true: the block's weight fragments (CW * RC cout tiles x 9 taps x KP chunks, 1 KiB each) are
// staged in LDS next to the input tile, once per block per chunk group, and every wave reads its A
// fragments with ds_read_b128 (conflict-free: lane order).  Without it each wave streams its own A
// fragments from L2 for every K-step, and at the m/l scales (rc * rp MFMAs per fragment load) the
// per-CU vector-memory path, not the MFMA, sets the rate.  Same K order: bitwise identical.
template <int S, int RC, int RP, int CW, int KP, bool AL>
struct Tile3Geom {
  static constexpr int TW = 16, RW = 4 / CW, TH = RW * RP;
  static constexpr int RI = (TH - 1) * S + 3, CI = (TW - 1) * S + 3;
  static constexpr int NQ = 4 * KP;
  static constexpr int NE = RI * CI * NQ, NL = (NE + 255) / 256;
  static constexpr int NA = AL ? CW * RC * 9 * KP * 64 : 0, NLA = (NA + 255) / 256;
  // register prefetch of the next stage (rc 1 has the registers for 10 pieces: stride-2 rp 8 tiles)
  static constexpr bool PF = AL ? NL + NLA <= 16 : NL <= (RC == 1 ? 10 : 8);
  static constexpr size_t lds = size_t(PF ? NL * 256 : NE) * 16 + size_t(AL ? (PF ? NLA * 256 : NA) : 0) * 16;
};

template <int S, int RC, int RP, int CW, int KP, bool AL>
__global__ __launch_bounds__(256) void conv3x3_tile_kernel(ConvArgs a) {
  using G = Tile3Geom<S, RC, RP, CW, KP, AL>;
  constexpr int TW = 16, RW = 4 / CW, TH = RW * RP;
  constexpr int RI = (TH - 1) * S + 3, CI = (TW - 1) * S + 3;  // staged input rows / cols
  constexpr int NQ = 4 * KP;                                    // 16-byte pieces per staged pixel
  constexpr int NL0 = G::NL;
  // with the register prefetch the image is padded to NL0 * 256 pieces so that the last staging round
  // stores unconditionally (see conv3x3_ring_kernel)
  __shared__ __attribute__((aligned(16))) h8 tile[G::PF ? NL0 * 256 : G::NE];
  __shared__ __attribute__((aligned(16))) h8 atile[AL ? (G::PF ? G::NLA * 256 : G::NA) : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int wc = wave / RW, wr = wave - wc * RW;
  const int tiles_x = (a.Wo + TW - 1) / TW, tiles_y = (a.Ho + TH - 1) / TH;
  int t, cog;
  tile_block(a.gy, t, cog);
  const int tx = t % tiles_x;
  t /= tiles_x;
  const int ty = t % tiles_y;
  const int n = t / tiles_y;
  const int ox0 = tx * TW, oy0 = ty * TH;
  const int cot0 = (cog * CW + wc) * RC;
  const int cotiles = (a.cout + 15) >> 4;
  const int spt = a.cin >> 5;  // 32-channel chunks = K-steps per tap
  const h8* wfrag[RC];
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const int ct = min(cot0 + r, cotiles - 1);
    wfrag[r] = reinterpret_cast<const h8*>(a.w) + (size_t(ct) * a.nalloc) * 64 + lane;
  }
  f4 acc[RC][RP];
#pragma unroll
  for (int r = 0; r < RC; ++r)
#pragma unroll
    for (int p = 0; p < RP; ++p) acc[r][p] = f4{0.f, 0.f, 0.f, 0.f};
  h8 af[RC];  // A fragments of the current K-step (prefetched one step ahead in the tap loop)
  if constexpr (!AL) {
#pragma unroll
    for (int r = 0; r < RC; ++r) af[r] = wfrag[r][0];
  }
  const _Float16* xn = a.x + int64_t(n) * a.Hs * a.Ws * a.xcs;
  const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
  // Staging: NL pieces per thread.  When they fit in registers (NL <= 8) the next stage's global
  // loads are issued right after this stage's LDS image is complete, so they are in flight during
  // this stage's MFMAs (register double buffer; one LDS image).
  constexpr int NE = G::NE, NL = G::NL, NA = G::NA, NLA = G::NLA;
  constexpr bool PF = G::PF;
  // A piece e of chunk group c0: fragment f = (block cout tile, k, tap) in that order, lane e & 63
  const h8* wblk = reinterpret_cast<const h8*>(a.w);
  const int ct_blk = cog * CW * RC;
  auto apiece = [&](int e, int c0) -> h8 {
    const int f = e >> 6, l = e & 63;
    const int rb = f / (9 * KP), rem = f - rb * (9 * KP);
    const int ct = min(ct_blk + rb, cotiles - 1);
    // select the address, not the loaded value: a select of two h8 values is done per 16-bit half and
    // makes the prefetch wait for its own loads right after issuing them
    return *(e < NA ? wblk + (size_t(ct) * a.nalloc + c0 * 9 + rem) * 64 + l : reinterpret_cast<const h8*>(g_zero_line));
  };
  auto piece = [&](int e, int c0, int& u, int& slot) -> h8 {
    const int pc = e / NQ, q = e - pc * NQ;
    const int r = pc / CI, c = pc - r * CI;
    const int iy = iy0 + r, ix = ix0 + c;
    u = r * CI + tile_col<S, CI>(c);
    slot = e < NE ? u * NQ + tile_slot<KP>(u, q) : e;
    const bool ok = e < NE && iy >= 0 && iy < a.Hs && ix >= 0 && ix < a.Ws && (KP == 1 || c0 + (q >> 2) < spt);
    return *(ok ? reinterpret_cast<const h8*>(xn + (int64_t(iy) * a.Ws + ix) * a.xcs + c0 * 32 + q * 8)
                : reinterpret_cast<const h8*>(g_zero_line));
  };
  h8 pv[PF ? NL : 1];
  int ps[PF ? NL : 1];
  h8 pa[PF && AL ? NLA : 1];
  if constexpr (PF) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      int u;
      pv[i] = piece(threadIdx.x + 256 * i, 0, u, ps[i]);
    }
    if constexpr (AL) {
#pragma unroll
      for (int i = 0; i < NLA; ++i) pa[i] = apiece(threadIdx.x + 256 * i, 0);
    }
  }
  for (int c0 = 0; c0 < spt; c0 += KP) {
    __syncthreads();  // previous stage's reads done
    if constexpr (PF) {
#pragma unroll
      for (int i = 0; i < NL; ++i) tile[ps[i]] = pv[i];
      if constexpr (AL) {
#pragma unroll
        for (int i = 0; i < NLA; ++i) atile[threadIdx.x + 256 * i] = pa[i];
      }
    } else {
      for (int e = threadIdx.x; e < NE; e += 256) {
        int u, sl;
        const h8 v = piece(e, c0, u, sl);
        tile[sl] = v;
      }
      if constexpr (AL)
        for (int e = threadIdx.x; e < NA; e += 256) atile[e] = apiece(e, c0);
    }
    __syncthreads();
    if constexpr (PF) {
      if (c0 + KP < spt) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          int u;
          pv[i] = piece(threadIdx.x + 256 * i, c0 + KP, u, ps[i]);
        }
        if constexpr (AL) {
#pragma unroll
          for (int i = 0; i < NLA; ++i) pa[i] = apiece(threadIdx.x + 256 * i, c0 + KP);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if (KP > 1 && c0 + k >= spt) break;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
        h8 bf[RP];
        // A fragments one K-step ahead (the last step of the last chunk re-reads its own; weights only,
        // no LDS hazard across the staging barrier): the L2 latency hides under this step's MFMAs
        const int ks = (c0 + k) * 9 + tap + 1;
        const int ksn = ks < spt * 9 ? ks : ks - 1;
        h8 an[RC];
        if constexpr (AL) {
#pragma unroll
          for (int r = 0; r < RC; ++r) af[r] = atile[(((wc * RC + r) * KP + k) * 9 + tap) * 64 + lane];
        } else {
#pragma unroll
          for (int r = 0; r < RC; ++r) an[r] = wfrag[r][ksn * 64];
        }
#pragma unroll
        for (int p = 0; p < RP; ++p) {
          const int ry = (wr * RP + p) * S + ky;
          const int u = ry * CI + tile_col<S, CI>(col * S + kx);
          bf[p] = tile[u * NQ + tile_slot<KP>(u, k * 4 + grp)];
        }
#pragma unroll
        for (int r = 0; r < RC; ++r)
#pragma unroll
          for (int p = 0; p < RP; ++p)
            acc[r][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[r], bf[p], acc[r][p], 0, 0, 0);
        if constexpr (!AL) {
#pragma unroll
          for (int r = 0; r < RC; ++r) af[r] = an[r];
        }
      }
    }
  }
  tile3_store<RC, RP>(a, acc, n, oy0 + wr * RP, ox0, cot0, col, grp);
}

// ============================================================================ 3x3, small cin, LDS tiles
// For cin % 8 == 0 and cin % 32 != 0 (cin <= 64: the C3k2 bottlenecks and early convs of small models,
// e.g. 8 -> 8 at 160 x 160).  Same block / wave geometry as conv3x3_tile_kernel, but the whole input
// tile + halo with ALL cin channels ((TH-1)*S+3 x (TW-1)*S+3 pixels x cin*2 B) is staged in LDS once,
// and the K loop walks the implicit-GEMM kernel's tap-major 8-channel chunks (c = 4 s + lane/16,
// tap = c / cpt): the same A fragments and the same per-output summation order as conv_mfma_kernel, so
// the two give bitwise-identical results.  Input pixels are read from HBM once (plus halo) instead of
// once per tap from L2.
// CPT > 0: cin = 8 CPT at compile time (the staging's index divisions, the K loop's tap / chunk arithmetic and
// its trip count become constants: the loop unrolls, every B read is base + a constant); 0: runtime cin.
template <int S, int RC, int RP, int CPT = 0>
__global__ __launch_bounds__(256) void conv3x3_tile_small_kernel(ConvArgs a) {
  constexpr int TW = 16, TH = 4 * RP;
  constexpr int RI = (TH - 1) * S + 3, CI = (TW - 1) * S + 3;
  extern __shared__ __attribute__((aligned(16))) h8 stile[];  // [RI][CI][cpt]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int cpt = CPT ? CPT : a.cpt;
  const int nsteps = CPT ? (9 * CPT + 3) / 4 : a.nsteps;
  const int tiles_x = (a.Wo + TW - 1) / TW, tiles_y = (a.Ho + TH - 1) / TH;
  int t, cog;
  tile_block(a.gy, t, cog);
  const int tx = t % tiles_x;
  t /= tiles_x;
  const int ty = t % tiles_y;
  const int n = t / tiles_y;
  const int ox0 = tx * TW, oy0 = ty * TH;
  const int cot0 = cog * RC;
  const int cotiles = (a.cout + 15) >> 4;
  const h8* wfrag[RC];
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const int ct = min(cot0 + r, cotiles - 1);
    wfrag[r] = reinterpret_cast<const h8*>(a.w) + (size_t(ct) * a.nalloc) * 64 + lane;
  }
  // A fragments of step 0 in flight while the tile is staged
  h8 an[RC];
#pragma unroll
  for (int r = 0; r < RC; ++r) an[r] = wfrag[r][0];
  const _Float16* xn = a.x + int64_t(n) * a.Hs * a.Ws * a.xcs;
  const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
  const int ne = RI * CI * cpt;
  for (int e = threadIdx.x; e < ne; e += 256) {
    const int pc = e / cpt, q = e - pc * cpt;
    const int r = pc / CI, c = pc - r * CI;
    const int iy = iy0 + r, ix = ix0 + c;
    h8 v = h8{0, 0, 0, 0, 0, 0, 0, 0};
    if (iy >= 0 && iy < a.Hs && ix >= 0 && ix < a.Ws)
      v = *reinterpret_cast<const h8*>(xn + (int64_t(iy) * a.Ws + ix) * a.xcs + q * 8);
    stile[e] = v;
  }
  __syncthreads();
  f4 acc[RC][RP];
#pragma unroll
  for (int r = 0; r < RC; ++r)
#pragma unroll
    for (int p = 0; p < RP; ++p) acc[r][p] = f4{0.f, 0.f, 0.f, 0.f};
  const h8 zero = h8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int st = 0; st < nsteps; ++st) {
    h8 af[RC];
#pragma unroll
    for (int r = 0; r < RC; ++r) af[r] = an[r];
    if (st + 1 < nsteps) {
#pragma unroll
      for (int r = 0; r < RC; ++r) an[r] = wfrag[r][(st + 1) * 64];
    }
    const unsigned c = unsigned(st * 4 + grp);
    const int tap = CPT ? int(c) / CPT : cpt == 1 ? int(c) : int(__umulhi(c, a.cmagic));
    const int ch = int(c) - tap * cpt;
    const bool tin = tap < 9;
    const int ky = (tap * 11) >> 5, kx = tap - ky * 3;  // tap / 3 for tap < 9
    h8 bf[RP];
#pragma unroll
    for (int p = 0; p < RP; ++p) {
      const int ry = (wave * RP + p) * S + ky, cx = col * S + kx;
      bf[p] = tin ? stile[(ry * CI + cx) * cpt + ch] : zero;
    }
#pragma unroll
    for (int r = 0; r < RC; ++r)
#pragma unroll
      for (int p = 0; p < RP; ++p) acc[r][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[r], bf[p], acc[r][p], 0, 0, 0);
  }
  tile3_store<RC, RP>(a, acc, n, oy0 + wave * RP, ox0, cot0, col, grp);  // bias, SiLU, residual, fp16 store
}

static size_t small_tile_lds(int stride, int rp, int cin) {
  const int th = 4 * rp, ri = (th - 1) * stride + 3, ci = 15 * stride + 3;
  return size_t(ri) * ci * (cin / 8) * 16;
}

// Tile-kernel configurations (their code: tile3_encode below)
static constexpr size_t tile3_lds(int s, int rp, int cw, int kp) {
  return size_t(((4 / cw) * rp - 1) * s + 3) * (15 * s + 3) * 4 * kp * 16;
}
// A-in-LDS variants: rc 2 / 4, rc * rp <= 16 (registers: the accumulators plus up to 16 staged pieces
// per thread), input tile + weight stage within 96 KiB
static constexpr bool tile3al_ok(int s, int rc, int rp, int cw, int kp) {
  return (rc == 2 || rc == 4) && (rp == 2 || rp == 4 || rp == 8) && (cw == 1 || cw == 2 || cw == 4) &&
         (kp == 1 || kp == 2) && rc * rp <= 16 &&
         tile3_lds(s, rp, cw, kp) + size_t(cw) * rc * 9 * kp * 1024 <= 96 * 1024;
}
// rp = 8 (8 output rows per wave: every A fragment read from L2 feeds 8 MFMAs, the m/l-scale 3x3 convs
// are L2-bound at rp <= 4) with rc 1 (any cw: the weight stream per output pixel halves at 32 accumulator
// registers) or with the couts split over 2 / 4 waves
static bool tile3_ok(int s, int rc, int rp, int cw, int kp) {
  return (rc == 1 || rc == 2 || rc == 4) && (rp == 1 || rp == 2 || rp == 4 || (rp == 8 && (rc == 1 || cw >= 2))) &&
         (cw == 1 || cw == 2 || cw == 4) && (kp == 1 || kp == 2) && rc * rp <= 32 &&
         tile3_lds(s, rp, cw, kp) <= 80 * 1024;
}

template <int S, int RC, int RP, int CW, int KP>
static void launch_tile3_k(const ConvArgs& a, bool al, dim3 grid, hipStream_t s) {
  if (al) {
    if constexpr (tile3al_ok(S, RC, RP, CW, KP)) {
      static_assert(Tile3Geom<S, RC, RP, CW, KP, true>::lds <= 160 * 1024, "A-in-LDS tile too large");
      FCE_LAUNCH((conv3x3_tile_kernel<S, RC, RP, CW, KP, true>), grid, dim3(256), 0, s, a);
    }
  } else if constexpr (tile3_lds(S, RP, CW, KP) <= 80 * 1024) {
    FCE_LAUNCH((conv3x3_tile_kernel<S, RC, RP, CW, KP, false>), grid, dim3(256), 0, s, a);
  }
}

template <int S, int RC, int RP>
static void launch_tile3_w(const ConvArgs& a, int cw, int kp, bool al, dim3 grid, hipStream_t s) {
  if (cw == 1)
    kp == 1 ? launch_tile3_k<S, RC, RP, 1, 1>(a, al, grid, s) : launch_tile3_k<S, RC, RP, 1, 2>(a, al, grid, s);
  else if (cw == 2)
    kp == 1 ? launch_tile3_k<S, RC, RP, 2, 1>(a, al, grid, s) : launch_tile3_k<S, RC, RP, 2, 2>(a, al, grid, s);
  else
    kp == 1 ? launch_tile3_k<S, RC, RP, 4, 1>(a, al, grid, s) : launch_tile3_k<S, RC, RP, 4, 2>(a, al, grid, s);
}

template <int S, int RC>
static void launch_tile3_rc(const ConvArgs& a, int rp, int cw, int kp, bool al, dim3 grid, hipStream_t s) {
  if (rp == 1)
    launch_tile3_w<S, RC, 1>(a, cw, kp, al, grid, s);
  else if (rp == 2)
    launch_tile3_w<S, RC, 2>(a, cw, kp, al, grid, s);
  else if (rp == 4)
    launch_tile3_w<S, RC, 4>(a, cw, kp, al, grid, s);
  else {  // rp == 8: rc 1 or cw 2 / 4 (tile3_ok), any cw with A in LDS (tile3al_ok)
    if (cw == 1)
      kp == 1 ? launch_tile3_k<S, RC, 8, 1, 1>(a, al, grid, s) : launch_tile3_k<S, RC, 8, 1, 2>(a, al, grid, s);
    else if (cw == 2)
      kp == 1 ? launch_tile3_k<S, RC, 8, 2, 1>(a, al, grid, s) : launch_tile3_k<S, RC, 8, 2, 2>(a, al, grid, s);
    else
      kp == 1 ? launch_tile3_k<S, RC, 8, 4, 1>(a, al, grid, s) : launch_tile3_k<S, RC, 8, 4, 2>(a, al, grid, s);
  }
}

template <int S>
static void launch_tile3_s(const ConvArgs& a, int rc, int rp, int cw, int kp, bool al, dim3 grid, hipStream_t s) {
  if (rc == 1)
    launch_tile3_rc<S, 1>(a, rp, cw, kp, al, grid, s);
  else if (rc == 2)
    launch_tile3_rc<S, 2>(a, rp, cw, kp, al, grid, s);
  else
    launch_tile3_rc<S, 4>(a, rp, cw, kp, al, grid, s);
}

template <int S, int RC>
static void launch_small3_rc(const ConvArgs& a, int rp, dim3 grid, size_t lds, hipStream_t s) {
  // compile-time cin for 8 and 16 channels (the n / s scales' small-cin 3x3s), runtime otherwise
#define SMALL3(RPV)                                                                                     \
  do {                                                                                                  \
    if (a.cpt == 1)                                                                                     \
      FCE_LAUNCH((conv3x3_tile_small_kernel<S, RC, RPV, 1>), grid, dim3(256), lds, s, a);               \
    else if (a.cpt == 2)                                                                                \
      FCE_LAUNCH((conv3x3_tile_small_kernel<S, RC, RPV, 2>), grid, dim3(256), lds, s, a);               \
    else                                                                                                \
      FCE_LAUNCH((conv3x3_tile_small_kernel<S, RC, RPV, 0>), grid, dim3(256), lds, s, a);               \
  } while (0)
  if (rp == 1)
    SMALL3(1);
  else if (rp == 2)
    SMALL3(2);
  else
    SMALL3(4);
#undef SMALL3
}

template <int S>
static void launch_small3_s(const ConvArgs& a, int rc, int rp, dim3 grid, size_t lds, hipStream_t s) {
  if (rc == 1)
    launch_small3_rc<S, 1>(a, rp, grid, lds, s);
  else if (rc == 2)
    launch_small3_rc<S, 2>(a, rp, grid, lds, s);
  else
    launch_small3_rc<S, 4>(a, rp, grid, lds, s);
}

static int launch_small3(const ConvArgs& a, int rc, int rp, int stride, int n, hipStream_t s) {
  const int th = 4 * rp;
  const int64_t tiles = int64_t((a.Wo + 15) / 16) * ((a.Ho + th - 1) / th) * n;
  FCE_CHECK(tiles < (int64_t(1) << 31), "conv 3x3 small tile: grid too large");
  const size_t lds = small_tile_lds(stride, rp, a.cin);
  FCE_CHECK(lds <= 64 * 1024, "conv 3x3 small tile: LDS tile too large");
  ConvArgs b = a;
  b.gy = ((a.cout + 15) / 16 + rc - 1) / rc;
  FCE_CHECK(tiles * b.gy < (int64_t(1) << 31), "conv 3x3 small tile: grid too large");
  const dim3 grid(unsigned(tiles * b.gy));
  if (stride == 1)
    launch_small3_s<1>(b, rc, rp, grid, lds, s);
  else
    launch_small3_s<2>(b, rc, rp, grid, lds, s);
  return launch_status("conv3x3_tile_small_kernel");
}

static int launch_tile3(const ConvArgs& a, int rc, int rp, int cw, int kp, bool al, int stride, int n, hipStream_t s) {
  FCE_CHECK(al ? tile3al_ok(stride, rc, rp, cw, kp) : tile3_ok(stride, rc, rp, cw, kp), "conv 3x3 tile: bad configuration");
  const int th = (4 / cw) * rp;
  const int64_t tiles = int64_t((a.Wo + 15) / 16) * ((a.Ho + th - 1) / th) * n;
  FCE_CHECK(tiles < (int64_t(1) << 31), "conv 3x3 tile: grid too large");
  ConvArgs b = a;
  b.gy = ((a.cout + 15) / 16 + cw * rc - 1) / (cw * rc);
  FCE_CHECK(tiles * b.gy < (int64_t(1) << 31), "conv 3x3 tile: grid too large");
  const dim3 grid(unsigned(tiles * b.gy));
  if (stride == 1)
    launch_tile3_s<1>(b, rc, rp, cw, kp, al, grid, s);
  else
    launch_tile3_s<2>(b, rc, rp, cw, kp, al, grid, s);
  return launch_status("conv3x3_tile_kernel");
}

// ============================================================================ family: LDS halo tile (kind 1)
// coded 0x100 | rc | rp << 4 | log2(cw) << 12 | (kp - 1) << 14 | al << 15
struct Tile3Cfg {
  int rc, rp, cw, kp;
  bool al;
};
static int tile3_encode(const Tile3Cfg& t) {
  return 0x100 | t.rc | (t.rp << 4) | (ilog2(t.cw) << 12) | ((t.kp - 1) << 14) | (int(t.al) << 15);
}
static Tile3Cfg tile3_decode(int code) {
  return {code & 15, (code >> 4) & 15, 1 << ((code >> 12) & 3), ((code >> 14) & 1) + 1, bool((code >> 15) & 1)};
}
static bool tile3_cfg_ok(const fce_conv_desc& d, const Tile3Cfg& t) {
  return d.k == 3 && d.cin % 32 == 0 && d.up == 0 &&
         (t.al ? tile3al_ok(d.stride, t.rc, t.rp, t.cw, t.kp) : tile3_ok(d.stride, t.rc, t.rp, t.cw, t.kp)) &&
         (t.kp == 1 || d.cin % 64 == 0);
}

// kp-major, then cw, rc, rp; blocks of cw * rc cout tiles
static void tile3_offer_al(bool al, const fce_conv_desc& d, CodeList& out) {
  const int cotiles = (d.cout + 15) / 16;
  for (int kp : {1, 2})
    for (int cw : {1, 2, 4})
      for (int rc : {1, 2, 4}) {
        if (!cotiles_want(cw * rc, cotiles)) continue;
        for (int rp : {1, 2, 4, 8}) {
          const Tile3Cfg t{rc, rp, cw, kp, al};
          if (tile3_cfg_ok(d, t)) out.add(tile3_encode(t));
        }
      }
}
void tile3_offer(const fce_conv_desc& d, int, CodeList& out) { tile3_offer_al(false, d, out); }
// FCE_TILE3AL=1 adds the A-in-LDS variants from 128 input channels (they lose on every l / m layer measured, so the
// planner does not spend autotune time on them by default); read per call: the variant tests switch it on mid-process
void tile3al_offer(const fce_conv_desc& d, int, CodeList& out) {
  if (d.cin >= 128 && env_on("FCE_TILE3AL")) tile3_offer_al(true, d, out);
}

int tile3_launch(const ConvCall& c, int code) {
  const Tile3Cfg t = tile3_decode(code);
  FCE_CHECK(tile3_cfg_ok(c.d, t) && c.out_kind == OUT_F16, "conv: bad LDS-tile hint");
  return launch_tile3(c.a, t.rc, t.rp, t.cw, t.kp, t.al, c.d.stride, c.n, c.s);
}

// ============================================================================ family: small-cin LDS tile (kind 2)
// coded 0x200 | rc | rp << 4
struct Small3Cfg {
  int rc, rp;
};
static int small3_encode(Small3Cfg t) { return 0x200 | t.rc | (t.rp << 4); }
static Small3Cfg small3_decode(int code) { return {code & 15, (code >> 4) & 15}; }
static bool small3_ok(const fce_conv_desc& d, Small3Cfg t) {
  return d.k == 3 && d.cin % 32 != 0 && d.cin <= 64 && d.up == 0 && (t.rc == 1 || t.rc == 2 || t.rc == 4) &&
         (t.rp == 1 || t.rp == 2 || t.rp == 4);
}

void small3_offer(const fce_conv_desc& d, int det_box, CodeList& out) {
  if (det_box) return;
  const int cotiles = (d.cout + 15) / 16;
  for (int rc : {1, 2, 4}) {
    if (!cotiles_want(rc, cotiles)) continue;
    for (int rp : {1, 2, 4})
      if (small3_ok(d, {rc, rp}) && small_tile_lds(d.stride, rp, d.cin) <= 64 * 1024) out.add(small3_encode({rc, rp}));
  }
}

int small3_launch(const ConvCall& c, int code) {
  const Small3Cfg t = small3_decode(code);
  FCE_CHECK(small3_ok(c.d, t) && c.out_kind == OUT_F16, "conv: bad small-cin LDS-tile hint");
  return launch_small3(c.a, t.rc, t.rp, c.d.stride, c.n, c.s);
}

}  // namespace fce

