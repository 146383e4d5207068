// What a dense-conv kernel family is to the dispatcher (conv.hip), and the host helpers the families share.
//
// A variant code is kind << 8 | the family's own bits (kind = (code >> 8) & 15; the generic register tile is kind 0,
// code rc | rp << 4).  Each family keeps its bit layout in ONE encode / decode pair next to its kernels: its offer()
// builds codes only through encode, its launch() reads them only through decode, and nothing else spells the bits.
//   capability = what launch() accepts (the family's *_ok predicate, FCE_CHECKed);
//   policy     = what offer() lists for the autotuner (cout-tile rules, Detect box restrictions, env opt-ins / outs).
// A valid code that is not offered still launches.  conv.hip's kFamilies table fixes the order of the candidate list.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "conv_args.h"

namespace fce {

// ---------------------------------------------------------------------------- packed-weight geometry
// nsteps K-steps of 32 (4 chunks of 8 input channels); each cout tile stores nalloc >= nsteps
// fragments: rounded up to a multiple of 8 (the main loop consumes steps in groups of its pipeline
// depth D <= 8) + 8 zero fragments, so the branch-free prefetch D steps ahead never reads past the
// image.
struct DenseGeom {
  int cpt, taps, nchunk, nsteps, nalloc, cotiles;
};
inline DenseGeom dense_geom(const fce_conv_desc& d) {
  DenseGeom g;
  g.cpt = d.cin / 8;
  g.taps = d.k * d.k;
  g.nchunk = g.taps * g.cpt;
  g.nsteps = (g.nchunk + 3) / 4;
  g.nalloc = ((g.nsteps + 7) & ~7) + 8;
  g.cotiles = (d.cout + 15) / 16;
  return g;
}

inline bool is_stem(const fce_conv_desc& d) { return d.groups == 1 && d.cin <= 4; }
inline bool is_dw(const fce_conv_desc& d) { return d.groups > 1; }

// 3x3 stems with cin * 9 <= 32 also carry one MFMA K-step of fp16 fragments (k = ci * 9 + tap, zero
// padded to 32) per 16-cout tile after the fp32 table: the stem_mfma_kernel's A operand
inline bool stem_mfma_ok(const fce_conv_desc& d) { return d.k == 3 && d.cin * 9 <= 32 && d.cout <= 64; }
inline size_t stem_fp32_bytes(const fce_conv_desc& d) { return size_t(d.cin) * d.k * d.k * d.cout * sizeof(float); }

// ---------------------------------------------------------------------------- launch helpers
inline int grid_cap(int64_t blocks) { return int(blocks < 65535 * 16 ? blocks : 65535 * 16); }

// Persistent launches size their grid from the kernel's real occupancy (registers and LDS), queried
// once per instantiation: blocks beyond one resident wave would start only when a first-wave block
// finishes its whole tile sequence.
int cus_per_xcd();  // conv.hip, queried once per process
template <typename K>
inline int blocks_per_cu(K kernel, size_t lds) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, lds) != hipSuccess) {
    (void)hipGetLastError();
    n = 1;
  }
  return std::max(1, n);
}
// FCE_PERSIST_OCC=k (experiment): at most k resident blocks per CU for the persistent grids, leaving the rest of
// each CU to the other lanes' kernels
int persist_cap(int occ);  // conv.hip, the knob is read once per process
inline int ring_slots(int units, int gy, int occ) {
  return std::max(1, std::min((units + 7) / 8, cus_per_xcd() * persist_cap(occ) / std::max(1, gy)));
}

// ---------------------------------------------------------------------------- env knobs
inline bool env_on(const char* name) {  // read at every call: the variant tests flip these mid-process
  const char* e = getenv(name);
  return e && atoi(e) != 0;
}
bool no_ring();  // diagnostics: FCE_NO_RING=1 drops the persistent (ring) variants; conv.hip, read once per process

// ---------------------------------------------------------------------------- the family interface
// Candidate codes in list order; `cap` truncates by position.
struct CodeList {
  int* out;
  int cap, n;
  void add(int code) {
    if (n < cap) out[n++] = code;
  }
};

// What conv2d_impl has after the ConvArgs fill.
struct ConvCall {
  const fce_conv_desc& d;
  const ConvArgs& a;
  int out_kind;
  DenseGeom g;
  int n;  // x.n
  hipStream_t s;
  // the original tensors, for a family that falls back to the heuristic path
  const fce_tensor& x;
  const void* w;
  const float* bias;
  const fce_tensor* res;
  const fce_tensor& y;
  const fce_detect_epi* det;
  const fce_tensor* dup;
  int duplo;
};

struct ConvFamily {
  int kind;  // (code >> 8) & 15
  const char* name;
  void (*offer)(const fce_conv_desc& d, int det_box, CodeList& out);  // policy: appends this family's candidates
  int (*launch)(const ConvCall& c, int code);                         // decodes, FCE_CHECKs capability, launches
};

// log2 of the power-of-two wave splits (wp, cw, wc = 1 / 2 / 4) that the codes store
inline int ilog2(int v) { return v >= 4 ? 2 : v >= 2 ? 1 : 0; }

// A block of `cb` cout tiles is offered only where the next smaller block (cb / 2) does not already cover the couts.
inline bool cotiles_want(int cb, int cotiles) { return !(cb > 1 && (cb >> 1) >= cotiles); }

// conv.hip: generic register tile (kind 0)
void generic_offer(const fce_conv_desc& d, int det_box, CodeList& out);
int generic_launch(const ConvCall& c, int code);
// conv1x1.hip
void stream1_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0x300
int stream1_launch(const ConvCall& c, int code);
void lds1_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0x400
int lds1_launch(const ConvCall& c, int code);
void ring1_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0x500
int ring1_launch(const ConvCall& c, int code);
void pipe1_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0x700
int pipe1_launch(const ConvCall& c, int code);
// conv3x3_tile.hip
void tile3_offer(const fce_conv_desc& d, int det_box, CodeList& out);    // 0x100
void tile3al_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0x100 with the A-in-LDS bit (opt-in)
int tile3_launch(const ConvCall& c, int code);
void small3_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0x200
int small3_launch(const ConvCall& c, int code);
// conv3x3_ring.hip
void ring3_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0x600
int ring3_launch(const ConvCall& c, int code);
void ring32_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0x900 (opt-in)
int ring32_launch(const ConvCall& c, int code);
// conv3x3_big.hip
void big3_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0x800
int big3_launch(const ConvCall& c, int code);
// conv3x3_wide.hip
void wide3_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0xA00 (opt-in)
int wide3_launch(const ConvCall& c, int code);
// conv_big.hip
void big1_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0xB00
int big1_launch(const ConvCall& c, int code);
void big3g_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0xC00
int big3g_launch(const ConvCall& c, int code);
// conv3x3_dring.hip
void dring_offer(const fce_conv_desc& d, int det_box, CodeList& out);  // 0xD00
int dring_launch(const ConvCall& c, int code);

// ---------------------------------------------------------------------------- cross-family entry points
// the register ring (conv3x3_ring.hip): the LDS-DMA ring's fallback on views it cannot address
int launch_ring3(const ConvArgs& a0, int rp, int pd, int stride, hipStream_t s);
int conv2d_impl(const fce_conv_desc& d, const fce_tensor& x, const void* w, const float* bias, const fce_tensor* res,
                const fce_tensor& y, const fce_detect_epi* det, hipStream_t s, int tile, const fce_tensor* dup = nullptr,
                int duplo = 0);
// dwconv.hip: depthwise variants, coded 100 + variant
int dwconv_candidates(const fce_conv_desc& d, int in_w, int* out, int cap);
int dwconv_launch(const fce_conv_desc& d, const fce_tensor& x, const void* w, const float* bias, const fce_tensor& y,
                  hipStream_t s, int code);
// stem.hip: the three stem kernels (NCHW input, cin <= 4)
int launch_stem(const fce_conv_desc& d, const fce_tensor& x, const void* w, const float* bias, const fce_tensor* res,
                const fce_tensor& y, int Ho, int Wo, hipStream_t s);

}  // namespace fce
