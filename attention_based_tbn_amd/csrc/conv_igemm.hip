// Implicit-GEMM 2-D convolution for gfx950 on the fp32 MFMA (v_mfma_f32_32x32x2_f32).
//
// Replaces, for the TBN hot path, what the reference gets from cuDNN through nn.Conv2d
// (graph: reference core/models/bn_inception_audio.py:24-401; 7x7 stem bn_inception.py:75-77).
//
// Data layout (MI355X-first, not the reference's NCHW):
//   activations NHWC fp32 with an explicit row pitch `ld` so a conv can read / write a channel
//   slice of a wider concat buffer; weights [Cout][R][S][Cin] (= torch channels_last memory of the
//   OIHW parameter), i.e. GEMM-B rows are K-contiguous.
// GEMM view:  M = N*OH*OW output pixels, N = Cout, K = R*S*Cin.
//   A (pixels x K) is gathered on the fly (im2col never materialised), staged through LDS in
//   [row][32+4] fp32 tiles: 128-B coalesced global reads per 8 lanes, ds_write_b128, and
//   conflict-free ds_read_b128 fragments (k is permuted identically for A and B, so one b128
//   read feeds 4 MFMAs).  4 waves per workgroup stacked along M, each owning (32*MT) x (32*NT).
//   blockIdx -> tile mapping is XCD-aware: the 8 tiles that share an activation row-panel
//   sit on one XCD so the panel is fetched into one L2 only.
// Epilogues (runtime switch): plain(+bias,+relu,+accumulate) | raw+bias with fused per-channel
//   sum / sum-of-squares partials for training-mode BatchNorm | eval BN folded scale/shift + ReLU.
// The same kernel is the data-gradient: dgrad = conv of dy with tap-flipped, channel-transposed
//   weights (`up` = forward stride handles strided layers by zero-insertion on the fly).
// ROWMODE is the 7x7 / stride 2 stem as a 4x4 / stride 1 conv on the 2x2 space-to-depth image (pool.hip): the K of an
//   output pixel is R contiguous runs of `Cin` floats (4 s2d pixels x 4*cin channels), one per s2d row, packed back to
//   back -- 32-float K chunks straddle runs -- and the image carries its zero border physically, so the loads need
//   no masks at all.
// SHARED PIECES.  Device: the four GEMM bodies (conv_igemm_body: register-staged generic, conv_halo_body: 3x3 with the
//   input patch staged once, conv_dma_body: LDS-DMA staging, conv_sk4_body: 32-row tiles whose waves split K) differ in how
//   a tile gets into LDS and share CONV_KSTEP (the fragment reads, MFMA groups and scheduling chain of one 32-float K step;
//   a body supplies the two fragment addresses), CONV_ROW_DECODE (GEMM row -> input pixel offset and tap-validity mask;
//   conv_dma_body keeps a copy of its own), dma_swizzle (THE slot swizzle of an LDS-DMA tile) and, from tbn_conv_dev.h,
//   xcd_tile and conv_epilogue.  The K step and the row decode are macros, and the accumulator clear and the
//   register-staged B tile stay written out: as functions they changed the code the compiler emits
//   (profiles/conv_igemm_refactor.md).  The weight-gradient kernel has its own K loop (b32 fragments, rotating accumulators).
// Host: every family's instantiation is chosen by with_tile / with_wgrad_tile and a compile-time (epilogue | stages, reduce)
//   selection; conv_prepare fills the derived geometry, conv_build_phases the parity phases of a strided data gradient
//   (parity_tap: THE contribution rule, conv_push_tap: a tap-table entry); conv_stages, conv_set_tiles, conv_longest_first,
//   rider_arg and tbn_raise_dyn_lds (tbn_kernels.h) each state one launch rule.
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include <cstring>
#include "tbn_common.h"
#include "tbn_kernels.h"
#include "tbn_rider_dev.h"

#define LDT 36  // LDS row pitch in floats (32 + 4): 16-B aligned rows, conflict-free b128 reads
// Timing ablations of the main loop (scripts/conv_ablate.py) exist only in a -DTBN_ABLATE=1 build: as run-time
// flags their scalar branches cut the K loop into basic blocks and cost the production kernel ~10 %.
#ifndef TBN_ABLATE
#define TBN_ABLATE 0
#endif
#ifndef TBN_DIAG
#define TBN_DIAG 0   // timing-diagnostic build: see ConvP::fold_scale
#endif
#define ABL(bit) (TBN_ABLATE && (p.flags & (bit)))
#define WABL(bit) (TBN_ABLATE && (p.ablate & (bit)))   // weight-gradient kernel: 1 no loop loads, 2 no LDS stores, 4 no MFMA

#include "tbn_conv_dev.h"

// Row decode of the generic-tap bodies, stated once: GEMM row `m` -> `off`, the byte offset of the row's (n, iy0, ix0)
// input pixel, and `mask`, bit t of which says that tap t of the row lies inside the image.  The taps form a (tny x tnx)
// grid starting at (ty0, tx0): validity = row bits x column bits.  Rows >= M keep what the caller preset (no tap).
// RM (the stem's packed rows): no masks, the border is in the image, and the pixel pitch is cp.
// Several lanes share each tile row, so every body decodes a row ONCE (thread t < BM takes row m0 + t) into an LDS table
// of (off, mask) that overlays the tile buffer, and reads its own rows back from there.
// A macro for the reason given at CONV_KSTEP: as a function it moved 192 kernels of this file.  Used by conv_igemm_body and
// conv_sk4_body; conv_dma_body keeps its own copy (see there).
#define CONV_ROW_DECODE(RM, m, off, mask)                                                          \
  if ((m) < p.M) {                                                                                 \
    const uint32_t n_ = fdiv((uint32_t)(m), p.div_ohw);                                            \
    const uint32_t rem_ = (uint32_t)(m) - n_ * p.div_ohw.d;                                        \
    const uint32_t a_ = fdiv(rem_, p.div_ow);                                                      \
    const uint32_t b_ = rem_ - a_ * p.div_ow.d;                                                    \
    const int iy0_ = (int)a_ * p.in_sy;                                                            \
    const int ix0_ = (int)b_ * p.in_sx;                                                            \
    if (RM) {                                                                                      \
      off = (unsigned)((((int)n_ * p.H + iy0_) * p.W + ix0_) * p.cp * 4);                          \
    } else {                                                                                       \
      unsigned yb_ = 0, xb_ = 0;                                                                   \
      _Pragma("unroll") for (int r_ = 0; r_ < 3; ++r_)                                             \
        if (r_ < p.tny && (unsigned)(iy0_ + p.ty0 + r_) < (unsigned)p.H) yb_ |= 1u << r_;          \
      off = (unsigned)((((int)n_ * p.H + iy0_) * p.W + ix0_) * p.in_ld * 4);                       \
      _Pragma("unroll") for (int c_ = 0; c_ < 3; ++c_)                                             \
        if (c_ < p.tnx && (unsigned)(ix0_ + p.tx0 + c_) < (unsigned)p.W) xb_ |= 1u << c_;          \
      _Pragma("unroll") for (int r_ = 0; r_ < 3; ++r_)                                             \
        if ((yb_ >> r_) & 1u) mask |= xb_ << (r_ * p.tnx);                                         \
    }                                                                                              \
  }

// One 32-float K step of a wave's (32 MT) x (32 NT) tile, stated once for the four GEMM bodies.  A_FRAG is the address
// of this lane's float4 of A sub-tile row `i` in the 8-wide k group `kg`, B_FRAG the same for B sub-tile row `j`: two
// expressions in those names, all a body has to supply.
// Software pipeline over the four k groups: the fragments of group g + 1 are read while group g multiplies; the
// sched_group_barrier chain pins that order (DS-read group, MFMA group, ...).  The fragment reads and MFMAs are ONE basic
// block (no run-time conditions inside), so the scheduler issues the ds_reads ahead of the MFMAs that hide them.
// The 4 MFMAs of one accumulator stay back to back: a dependent MFMA is only free when it directly follows its
// producer (scripts/ubench: alternating two accumulators halves the rate).
// -DTBN_ABLATE=1 builds: flag 32 drops the LDS fragment reads, flag 8 the MFMAs (in every family).
// A macro, expanded where p, MT, NT and acc[MT][NT] are in scope (its own names end in an underscore): as a
// __forceinline__ function template taking the two addresses as lambdas the same text moved 170 of this file's kernels
// (profiles/conv_igemm_refactor.md); expanded in place every kernel is the machine code it was with the block written out.
#define CONV_KSTEP(A_FRAG, B_FRAG)                                                                                       \
  {                                                                                                                      \
    float4 fa_[2][MT], fb_[2][NT];                                                                                       \
    auto frag_load_ = [&](int buf_, int kg) {                                                                            \
      _Pragma("unroll") for (int i = 0; i < MT; ++i) fa_[buf_][i] = *reinterpret_cast<const float4*>(A_FRAG);            \
      _Pragma("unroll") for (int j = 0; j < NT; ++j) fb_[buf_][j] = *reinterpret_cast<const float4*>(B_FRAG);            \
    };                                                                                                                   \
    auto mfma_group_ = [&](int buf_) {                                                                                   \
      _Pragma("unroll") for (int j = 0; j < NT; ++j) _Pragma("unroll") for (int i = 0; i < MT; ++i) {                    \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa_[buf_][i].x, fb_[buf_][j].x, acc[i][j], 0, 0, 0);            \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa_[buf_][i].y, fb_[buf_][j].y, acc[i][j], 0, 0, 0);            \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa_[buf_][i].z, fb_[buf_][j].z, acc[i][j], 0, 0, 0);            \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa_[buf_][i].w, fb_[buf_][j].w, acc[i][j], 0, 0, 0);            \
      }                                                                                                                  \
    };                                                                                                                   \
    if (!ABL(32)) {                                                                                                      \
      frag_load_(0, 0);                                                                                                  \
      frag_load_(1, 1);                                                                                                  \
    }                                                                                                                    \
    if (!ABL(8)) mfma_group_(0);                                                                                         \
    if (!ABL(32)) frag_load_(0, 2);                                                                                      \
    if (!ABL(8)) mfma_group_(1);                                                                                         \
    if (!ABL(32)) frag_load_(1, 3);                                                                                      \
    if (!ABL(8)) mfma_group_(0);                                                                                         \
    if (!ABL(8)) mfma_group_(1);                                                                                         \
    if (!TBN_ABLATE) {                                                                                                   \
      constexpr int NR_ = MT + NT, NM_ = 4 * MT * NT;                                                                    \
      __builtin_amdgcn_sched_group_barrier(0x100, 2 * NR_, 0);                                                           \
      __builtin_amdgcn_sched_group_barrier(0x008, NM_, 0);                                                               \
      __builtin_amdgcn_sched_group_barrier(0x100, NR_, 0);                                                               \
      __builtin_amdgcn_sched_group_barrier(0x008, NM_, 0);                                                               \
      __builtin_amdgcn_sched_group_barrier(0x100, NR_, 0);                                                               \
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * NM_, 0);                                                           \
      __builtin_amdgcn_sched_barrier(0); /* what follows (a barrier and its lgkmcnt(0)) stays below the last MFMA group */ \
    }                                                                                                                    \
  }

// EPI: 0 plain (+bias, optional ReLU / accumulate), 1 training-BN statistics, 2 eval-BN fold + ReLU,
//      3 plain with output scatter (parity phase of a strided data gradient)
// RED (EPI 0 / 3 only): the epilogue also forms the BN-backward reduce partials of the layers that produced the
//      activation whose gradient this launch finishes (RedSeg in tbn_kernels.h)
template <int MT, int NT, bool ROWMODE, int EPI, int STAGES, bool RED = false>
__device__ __forceinline__ void conv_igemm_body(const ConvP& p, const int bid, float* lds) {
  constexpr int BM = 128 * MT, BN = 32 * NT;
  constexpr int AR = 4 * MT;  // A rows per thread
  constexpr int TILE_F = (BM + BN) * LDT;  // floats per LDS stage (A rows then B rows)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int tm, tn;
  xcd_tile(bid, p.tiles_m, p.tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  // descriptors are built from kernel arguments only (wave-uniform): loads need no branches, an
  // out-of-image tap / out-of-range row is an out-of-range OFFSET and reads zeros
  const i32x4 in_rsrc = make_rsrc(p.in, p.in_bytes);
  const i32x4 wt_rsrc = make_rsrc(p.wt, p.wt_bytes);

  const int c4 = tid & 7, r0 = tid >> 3;
  unsigned a_off[AR];   // byte offset of the row's (n, iy0, ix0) pixel (ROWMODE: out of range for rows >= M)
  unsigned a_mask[AR];  // bit t: tap t of this row lies inside the image (unused in ROWMODE: the border is physical)
  // Row setup (VALU diet, round 3).  Eight threads (c4 = 0..7) share each tile row: decoding the rows per thread ran the
  // two magic divisions and the tap masks 8x per row, ~35 VALU x 4*MT rows per thread.  Now a pointwise launch (1x1,
  // stride 1, no padding: every fused 1x1 group) needs no decode at all -- the input pixel IS the output row -- and
  // every other launch decodes each row ONCE (thread t < BM takes row t) into an LDS table the threads then read.
  const bool pointwise = !ROWMODE && p.ntaps == 1 && p.in_sy == 1 && p.in_sx == 1 && p.ty0 == 0 && p.tx0 == 0 &&
                         p.OHs == p.H && p.OWs == p.W;
  if (pointwise) {
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int m = m0 + r0 + 32 * i;
      a_off[i] = (unsigned)m * (unsigned)p.in_ld * 4u;
      a_mask[i] = m < p.M ? 1u : 0u;
    }
  } else {
    unsigned* rowtab = reinterpret_cast<unsigned*>(lds);   // [BM][2]: the tiles are not staged yet
    if (tid < BM) {
      const int m = m0 + tid;
      unsigned mask = 0;
      unsigned off = ROWMODE ? TBN_OOB : 0u;
      CONV_ROW_DECODE(ROWMODE, m, off, mask)
      rowtab[2 * tid] = off;
      rowtab[2 * tid + 1] = mask;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const uint2 e = *reinterpret_cast<const uint2*>(&rowtab[2 * (r0 + 32 * i)]);
      a_off[i] = e.x;
      a_mask[i] = e.y;
    }
    __syncthreads();   // everyone has read the table before the first tile store overwrites it
  }

  if (ABL(128)) {  // ablation: exit after the per-row setup
    if (a_off[0] == 0x12345u && a_mask[AR - 1] == 77u) p.seg[0].ptr[0] = 1.f;
    return;
  }
  f32x16 acc[MT][NT];   // (the clear stays written out in the four bodies: as a helper it moved 232 kernels, profiles/bf16x_refactor.md)
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int ksteps = p.K >> 5;
  float4 ra[AR], rb[NT];
  const unsigned b_row = (unsigned)(n0 + r0) * (unsigned)p.Krow * 4u + (unsigned)c4 * 16u;

  // (tap, c0) of the NEXT tile to fetch advance incrementally: no division, tap tables are read with
  // scalar loads only when the tap changes
  int l_tap = 0, l_c0 = 0;
  unsigned l_toff = (unsigned)p.tap_off[0], l_koff = (unsigned)p.tap_koff[0] * 4u;
  unsigned a_cur[AR];  // per-row byte offset for the CURRENT tap (or OOB): recomputed only when the tap changes;
                       // the channel-chunk offset rides in the instruction's scalar offset -> no VALU per load
  unsigned b_voff[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) b_voff[i] = b_row + (unsigned)(32 * i) * (unsigned)p.Krow * 4u;
  const unsigned rm_pitch = (unsigned)(p.W * p.cp) * 4u;   // ROWMODE: bytes between the runs of a pixel (one image row)
  auto load_tiles = [&]() {
    if (!ROWMODE) {
      if (l_c0 == 0) {
        const unsigned toff = l_toff + (unsigned)c4 * 16u;
#pragma unroll
        for (int i = 0; i < AR; ++i) a_cur[i] = ((a_mask[i] >> l_tap) & 1u) ? a_off[i] + toff : TBN_OOB;
      }
      const unsigned soff = (unsigned)l_c0 * 4u;
#pragma unroll
      for (int i = 0; i < AR; ++i) ra[i] = buf_load4(in_rsrc, a_cur[i], soff);
    } else {
      // l_c0 counts the packed K floats: this lane's float4 sits in run t at float4 w4 (one division per K-step,
      // shared by the thread's AR rows; no masks -- the zero border is in the image)
      const uint32_t f = ((uint32_t)l_c0 >> 2) + (uint32_t)c4;
      const uint32_t t = fdiv(f, p.div_rl4);
      const unsigned roff = t * rm_pitch + (f - t * p.div_rl4.d) * 16u;
#pragma unroll
      for (int i = 0; i < AR; ++i) ra[i] = buf_load4(in_rsrc, a_off[i] + roff);   // rows >= M: 2^31 + roff stays out of range
    }
    const unsigned koff = l_koff + (unsigned)l_c0 * 4u;
#pragma unroll
    for (int i = 0; i < NT; ++i)  // rows >= Cout are beyond wt_bytes -> zeros
      rb[i] = buf_load4(wt_rsrc, b_voff[i], koff);
    l_c0 += 32;
    if (!ROWMODE && l_c0 == p.Cin) {
      l_c0 = 0;
      ++l_tap;
      if (l_tap < p.ntaps) {
        l_toff = (unsigned)p.tap_off[l_tap];
        l_koff = (unsigned)p.tap_koff[l_tap] * 4u;
      }
    }
  };
  auto store_tiles = [&](float* stage) {
    float* As = stage;
    float* Bs = stage + BM * LDT;
#pragma unroll
    for (int i = 0; i < AR; ++i) *reinterpret_cast<float4*>(&As[(r0 + 32 * i) * LDT + c4 * 4]) = ra[i];
#pragma unroll
    for (int i = 0; i < NT; ++i) *reinterpret_cast<float4*>(&Bs[(r0 + 32 * i) * LDT + c4 * 4]) = rb[i];
  };

  load_tiles();
  store_tiles(lds);
  __syncthreads();
  if (ABL(256)) {  // ablation: exit after the prologue tile
    if (lds[tid] == 12345.678f) p.seg[0].ptr[0] = 1.f;
    return;
  }

  const int lrow = lane & 31, lhalf = lane >> 5;
  // two LDS stages, ONE barrier per K-step: the stage written in step ks was last read in step ks-1,
  // and every wave has passed the barrier that ended step ks-1 before any wave writes it.
  // A ragged last N tile multiplies its zero-filled weight rows (rows >= Cout are out-of-range loads) instead of
  // branching around MFMAs.
  for (int ks = 0; ks < ksteps; ++ks) {
    const bool more = (ks + 1 < ksteps) && !ABL(4);   // flag 4: ablation, no loads in the loop
    if (more) load_tiles();  // global loads stay in flight under the MFMA phase
    const float* As = lds + (STAGES == 2 ? (ks & 1) * TILE_F : 0);
    const float* Bs = As + BM * LDT;
    CONV_KSTEP(&As[(wave * 32 * MT + i * 32 + lrow) * LDT + kg * 8 + lhalf * 4], &Bs[(j * 32 + lrow) * LDT + kg * 8 + lhalf * 4])
    if (STAGES == 2) {
      if (more) store_tiles(lds + ((ks + 1) & 1) * TILE_F);
      if (!ABL(64)) __syncthreads();   // flag 64: ablation, no barrier
    } else {  // single stage: everyone must be done reading before the tile is overwritten
      __syncthreads();
      if (more) {
        store_tiles(lds);
        __syncthreads();
      }
    }
  }

  conv_epilogue<MT, NT, EPI, RED>(p, acc, lds, tm, m0, n0);
}

template <int MT, int NT, bool ROWMODE, int EPI, int STAGES, bool RED = false>
__global__ __launch_bounds__(256) void conv_igemm_kernel(ConvP p, RiderP rider) {
  __shared__ __attribute__((aligned(16))) float lds[STAGES * (128 * MT + 32 * NT) * LDT];
  TBN_RIDER_DISPATCH(rider, bid)
  conv_igemm_body<MT, NT, ROWMODE, EPI, STAGES, RED>(p, bid, lds);
}

// LDS-DMA primitive (see the LDS-DMA variant of the generic kernel further down for the protocol): lane l's 16 bytes land at
// (wave-uniform LDS address in M0) + 16 l
__device__ __forceinline__ void lds_dma16(i32x4 rsrc, unsigned lds_dst, unsigned voff, unsigned soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :
               : "s"(lds_dst), "v"(voff), "s"(rsrc), "s"(soff)
               : "memory");   // (m0 cannot be named as a clobber: clang rejects it as a reserved register; nothing else in this
                              //  kernel keeps a value in M0 -- no readlane / movrel / LDS-direct uses)
}
// THE SWIZZLE of an LDS-DMA tile.  A wave instruction writes 8 rows x 128 B, so rows are UNPADDED and conflict-free b128
// fragment reads come from an XOR swizzle instead: 16-B slot q of tile row r lives at slot q ^ ((r >> 1) & 7).  Returns the
// byte offset inside the row.  Applied twice: on the global SOURCE address of each lane (the lane whose bytes land in
// slot q of row r fetches chunk q ^ f(r)) and again on the fragment read (logical chunk 2 kg + lhalf).
__device__ __forceinline__ constexpr unsigned dma_swizzle(const int q, const int r) { return (unsigned)((q ^ ((r >> 1) & 7)) << 4); }

// Round 6: the LDS-halo kernel's WEIGHT tiles (one 32*NT x 32 tile per tap) go global -> LDS by LDS-DMA for the MT = 1 tiles -- no
// VGPR round trip, no ds_write, the store's issue slots go to the MFMAs (scripts/ubench/kstep_cost.hip: the tile store costs the
// K-step 3.5 % of the peak).  Measured (profiles/r06_ab_halo_dma_b.txt, r06_conv_variants_halo_dma_b.txt): steady state <1,1> +0.8 %,
// <1,2> +2.6 %, <1,3> +0.7 %; <2,x> -0.4 ... -1.2 % (they stay register-staged); one-stream conv stage of the bench +1.1 points
// (3 of 3), three-stream step +-0.  -DTBN_HALO_DMA_B=0 restores the register-staged form for every tile.
#ifndef TBN_HALO_DMA_B
#define TBN_HALO_DMA_B 1
#endif

// ------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 convolution (forward of such a layer, and its data gradient, which has the same form) with
// the INPUT PATCH STAGED ONCE PER 32-CHANNEL CHUNK.  The generic body above gathers an im2col A tile per filter tap:
// nine global -> LDS copies of (almost) the same pixels.  Here the flat NHWC pixel range of a 128*MT-row output tile,
// widened by W + 1 pixels on both sides (a "flat halo": BM + 2W + 2 consecutive pixels, contiguous in HBM), is loaded
// once per channel chunk and the nine taps read it at nine row shifts:
//   tap (dy, dx) of output pixel m  ->  halo row (m - m0) + (W + 1) + dy*W + dx.
// Where that shift leaves the image (top / bottom row, left / right column, frame boundary) the lane reads a row of
// zeros instead: the nine per-lane row addresses are loop invariants computed once.  Global -> LDS traffic of the A
// operand drops by 9*BM / (BM + 2W + 2) (4.8x at W = 56, 6.2x at W = 28 for BM = 128), its load / ds_write instructions
// and the per-tap address VALU likewise.  Weights stream as before: one (32*NT) x 32 B tile per tap, double buffered.
// LDS: [BM + 2W + 3 rows] A (one buffer: the next chunk waits in registers) + 2 x [32*NT rows] B, pitch LDT.
template <int MT, int NT, int EPI, bool RED>
__device__ __forceinline__ void conv_halo_body(const ConvP& p, const int bid, float* lds) {
  constexpr int BM = 128 * MT, BN = 32 * NT;
  constexpr int NJ = (BM + 2 * 64 + 2 + 31) / 32;   // float4 slots per thread for a halo of up to W = 64
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int tm, tn;
  xcd_tile(bid, p.tiles_m, p.tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int W = p.W, HR = BM + 2 * W + 2;   // halo rows; row HR is the zero row
  float* As = lds;
  float* Bs0 = lds + (HR + 1) * LDT;

  const i32x4 in_rsrc = make_rsrc(p.in, p.in_bytes);
  const i32x4 wt_rsrc = make_rsrc(p.wt, p.wt_bytes);
  const int c4 = tid & 7, r0 = tid >> 3;
  const int lrow = lane & 31, lhalf = lane >> 5;

  // per-lane LDS byte address of each tap's A fragment row (or the zero row)
  unsigned fa_off[MT][9];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int lr = wave * 32 * MT + i * 32 + lrow;
    const int m = m0 + lr;
    const uint32_t n = fdiv((uint32_t)m, p.div_ohw);
    const uint32_t rem = (uint32_t)m - n * p.div_ohw.d;
    const int y = (int)fdiv(rem, p.div_ow);
    const int x = (int)rem - y * W;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dy = t / 3 - 1, dx = t % 3 - 1;
      const bool ok = (m < p.M) && ((unsigned)(y + dy) < (unsigned)p.H) && ((unsigned)(x + dx) < (unsigned)W);
      const int row = ok ? lr + (W + 1) + dy * W + dx : HR;
      fa_off[i][t] = (unsigned)(row * LDT + lhalf * 4) * 4u;
    }
  }
  // halo slot j of this thread: row (tid >> 3) + 32 j, 16-B column c4
  const int pix0 = m0 - (W + 1) + r0;
  float4 ha[NJ];
  auto load_halo = [&](int c0) {
    const unsigned soff = (unsigned)c0 * 4u;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int h = r0 + 32 * j, pix = pix0 + 32 * j;
      const bool ok = (h < HR) && ((unsigned)pix < (unsigned)p.M);
      ha[j] = buf_load4(in_rsrc, ok ? (unsigned)pix * (unsigned)p.in_ld * 4u + (unsigned)c4 * 16u : TBN_OOB, soff);
    }
  };
  auto store_halo = [&](int c0) {
#if TBN_DIAG
    if (p.fold_scale != nullptr) {   // cost probe: BN apply + ReLU of the producer layer at staging time (zero padding kept)
      const float4 fs = *reinterpret_cast<const float4*>(p.fold_scale + c0 + c4 * 4);
      const float4 fh = *reinterpret_cast<const float4*>(p.fold_shift + c0 + c4 * 4);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const bool ok = (r0 + 32 * j < HR) && ((unsigned)(pix0 + 32 * j) < (unsigned)p.M);
        ha[j].x = ok ? fmaxf(fmaf(ha[j].x, fs.x, fh.x), 0.f) : 0.f;
        ha[j].y = ok ? fmaxf(fmaf(ha[j].y, fs.y, fh.y), 0.f) : 0.f;
        ha[j].z = ok ? fmaxf(fmaf(ha[j].z, fs.z, fh.z), 0.f) : 0.f;
        ha[j].w = ok ? fmaxf(fmaf(ha[j].w, fs.w, fh.w), 0.f) : 0.f;
      }
    }
#endif
    (void)c0;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (r0 + 32 * j < HR) *reinterpret_cast<float4*>(&As[(r0 + 32 * j) * LDT + c4 * 4]) = ha[j];
  };
  constexpr bool DMAB = (TBN_HALO_DMA_B != 0) && MT == 1;
  float4 rb[NT];
  unsigned b_voff[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
    b_voff[i] = (unsigned)(n0 + r0 + 32 * i) * (unsigned)p.Krow * 4u + (unsigned)c4 * 16u;   // rows >= Cout: beyond wt_bytes
  auto load_b = [&](int t, int c0) {
    const unsigned koff = (unsigned)(t * p.Cin + c0) * 4u;
#pragma unroll
    for (int i = 0; i < NT; ++i) rb[i] = buf_load4(wt_rsrc, b_voff[i], koff);
  };
  auto store_b = [&](float* Bs) {
#pragma unroll
    for (int i = 0; i < NT; ++i) *reinterpret_cast<float4*>(&Bs[(r0 + 32 * i) * LDT + c4 * 4]) = rb[i];
  };
  // DMAB: the weight tile of a tap goes global -> LDS directly (no VGPR round trip, no ds_write): rows are 128 B, unpadded,
  // their 16-B slots swizzled (dma_swizzle); a wave instruction writes 8 rows
  const int dr = lane >> 3, dslot = lane & 7;
  unsigned bd_voff[NT], fb_addr[NT][4];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int r = (wave + 4 * i) * 8 + dr;
    bd_voff[i] = (unsigned)(n0 + r) * (unsigned)p.Krow * 4u + dma_swizzle(dslot, r);
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int r = j * 32 + lrow;
#pragma unroll
    for (int kg = 0; kg < 4; ++kg) fb_addr[j][kg] = (unsigned)(r * 128) + dma_swizzle(2 * kg + lhalf, r);
  }
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const unsigned ldsB = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)reinterpret_cast<char*>(Bs0));
  auto dma_b = [&](int t, int c0, int stage) {
    const unsigned koff = (unsigned)__builtin_amdgcn_readfirstlane((t * p.Cin + c0) * 4);
#pragma unroll
    for (int i = 0; i < NT; ++i) lds_dma16(wt_rsrc, ldsB + (unsigned)(stage * BN * 128 + (wv + 4 * i) * 1024), bd_voff[i], koff);
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // prologue: zero row, halo of chunk 0, B tile of (tap 0, chunk 0)
  load_halo(0);
  if (DMAB)
    dma_b(0, 0, 0);
  else
    load_b(0, 0);
  if (tid < LDT) As[HR * LDT + tid] = 0.f;
  store_halo(0);
  if (DMAB)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else
    store_b(Bs0);
  __syncthreads();

  const int nchunks = p.Cin >> 5;
  const char* As_b = reinterpret_cast<const char*>(As);
  int ks = 0;
  // One 32-channel chunk = nine taps.  NEXT (a type, so every `if` on it is resolved at compile time): there is another
  // chunk behind this one -- its halo is fetched at the top and the B tile of its tap 0 during tap 8.  The last chunk is a
  // second copy of the body WITHOUT those parts rather than the same code under `if (c + 1 < nchunks)`: with the prefetches
  // under a run-time condition the compiler's wait-count pass must assume that the B-tile loads of the previous trip may
  // still be in flight where the first ds_read of a trip reuses their registers, and put `s_waitcnt vmcnt(1)` there --
  // right behind the thirteen halo loads just issued, i.e. every chunk started by waiting for its successor's halo.
  auto chunk = [&](const int c, auto next_tag) {
    constexpr bool NEXT = decltype(next_tag)::value;
    if (NEXT) load_halo((c + 1) * 32);   // lands during tap 0 (the first B-tile wait is behind it in vmcnt order)
#pragma unroll
    for (int t = 0; t < 9; ++t, ++ks) {
      const bool more = NEXT || t < 8;
      if (more) {
        // DMAB: straight into the other stage (last read in the previous tap: every wave is past that tap's barrier)
        if (DMAB)
          dma_b(t < 8 ? t + 1 : 0, t < 8 ? c * 32 : (c + 1) * 32, (ks + 1) & 1);
        else
          load_b(t < 8 ? t + 1 : 0, t < 8 ? c * 32 : (c + 1) * 32);
      }
      const float* Bs = Bs0 + (ks & 1) * (BN * LDT);
      const char* Bd = reinterpret_cast<const char*>(Bs0) + (ks & 1) * (BN * 128);
      // (the B-tile loads of the next tap are left to the scheduler, which sinks them to 4-12 MFMAs in front of the
      // ds_write that waits for them: pinning them to the top of the tap with a VMEM group in the K step's chain measured
      // 0-2 % SLOWER on warm clocks, 25 % on one <1,3> shape -- the weights are L2 hits and the early loads lengthen
      // live ranges)
      CONV_KSTEP(As_b + fa_off[i][t] + kg * 32,
                 DMAB ? Bd + fb_addr[j][kg] : reinterpret_cast<const char*>(&Bs[(j * 32 + lrow) * LDT + kg * 8 + lhalf * 4]))
      if (DMAB)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA of the next tap's weights has landed (and so has
                                                           // the next chunk's halo prefetch issued at the top of tap 0)
      else if (more)
        store_b(Bs0 + ((ks + 1) & 1) * (BN * LDT));
      __syncthreads();
    }
    if (NEXT) {   // every wave is past its last read of this chunk's halo (barrier above)
      store_halo((c + 1) * 32);
      __syncthreads();
    }
  };
  for (int c = 0; c + 1 < nchunks; ++c) chunk(c, std::true_type{});
  chunk(nchunks - 1, std::false_type{});
  conv_epilogue<MT, NT, EPI, RED>(p, acc, lds, tm, m0, n0);
}

template <int MT, int NT, int EPI, bool RED>
__global__ __launch_bounds__(256) void conv_halo_kernel(ConvP p, RiderP rider) {
  extern __shared__ __attribute__((aligned(16))) float dyn_lds[];
  TBN_RIDER_DISPATCH(rider, bid)
  conv_halo_body<MT, NT, EPI, RED>(p, bid, dyn_lds);
}

// ------------------------------------------------------------------------------------------
// LDS-DMA variant of the generic implicit GEMM (1x1 / 3x3, any stride; not the stem): the A and B tiles go from
// global memory STRAIGHT into LDS (`buffer_load_dwordx4 ... lds`: no VGPR round trip, no ds_write issue, 4*MT + NT
// fewer VGPR quads), two stages, one barrier per K-step.  An LDS-DMA instruction writes lane l's 16 bytes at
// (wave-uniform base) + 16 l, i.e. 8 rows x 128 B per wave instruction: rows are UNPADDED and their 16-B slots swizzled
// (dma_swizzle, above: on the source address and again on the fragment read).  Out-of-image taps / rows beyond M or Cout
// are out-of-range buffer offsets: the DMA writes zeros.
// The DMA is issued through inline asm: hipcc would otherwise treat each LDS-DMA as a pending LDS write and put an
// `s_waitcnt vmcnt(0)` in front of the next fragment read -- draining the prefetch it is supposed to overlap.  The
// asm statement is invisible to that bookkeeping; the wait is placed by hand before the barrier that publishes the
// stage (cdna_hip_programming.md 5.7: M0 is written in the same statement that uses it).

template <int MT, int NT, int EPI, bool RED>
__device__ __forceinline__ void conv_dma_body(const ConvP& p, const int bid, float* lds) {
  constexpr int BM = 128 * MT, BN = 32 * NT;
  constexpr int AR = 4 * MT;                 // 8-row DMA instructions per wave for the A tile
  constexpr int TILE_B = (BM + BN) * 128;    // bytes per LDS stage (A rows then B rows, 128 B each)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int tm, tn;
  xcd_tile(bid, p.tiles_m, p.tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const i32x4 in_rsrc = make_rsrc(p.in, p.in_bytes);
  const i32x4 wt_rsrc = make_rsrc(p.wt, p.wt_bytes);

  const int rl = lane >> 3, slot = lane & 7;   // row within the 8-row group / 16-B slot this lane's bytes land in
  unsigned a_off[AR], a_mask[AR];
  {
    // each tile row is decoded once (thread t < BM takes row t) into an LDS table -- eight lanes share a row; decoding
    // per lane repeated the two magic divisions and the tap masks 8x (see conv_igemm_body)
    // (CONV_ROW_DECODE written out, with the offset formed LAST: the order of these statements decides the code of this
    // body's 32 kernels, and the macro's order is the one the 160 kernels of the other two bodies need --
    // profiles/conv_igemm_refactor.md.  Same values.)
    unsigned* rowtab = reinterpret_cast<unsigned*>(lds);   // [BM][2]: no DMA has been issued yet
    if (tid < BM) {
      const int m = m0 + tid;
      unsigned mask = 0;
      int off = 0;
      if (m < p.M) {
        const uint32_t n = fdiv((uint32_t)m, p.div_ohw);
        const uint32_t rem = (uint32_t)m - n * p.div_ohw.d;
        const uint32_t a = fdiv(rem, p.div_ow);
        const uint32_t b = rem - a * p.div_ow.d;
        const int iy0 = (int)a * p.in_sy, ix0 = (int)b * p.in_sx;
        unsigned yb = 0, xb = 0;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
          if (rr < p.tny && (unsigned)(iy0 + p.ty0 + rr) < (unsigned)p.H) yb |= 1u << rr;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (c < p.tnx && (unsigned)(ix0 + p.tx0 + c) < (unsigned)p.W) xb |= 1u << c;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
          if ((yb >> rr) & 1u) mask |= xb << (rr * p.tnx);
        off = (((int)n * p.H + iy0) * p.W + ix0) * p.in_ld * 4;
      }
      rowtab[2 * tid] = (unsigned)off;
      rowtab[2 * tid + 1] = mask;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int r = (wave * AR + i) * 8 + rl;    // tile row
      const uint2 e = *reinterpret_cast<const uint2*>(&rowtab[2 * r]);
      a_off[i] = e.x + dma_swizzle(slot, r);   // swizzled source chunk (masked rows never load)
      a_mask[i] = e.y;
    }
    __syncthreads();   // the table is dead: the first DMA may overwrite it
  }
  unsigned b_voff[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int r = (wave + 4 * i) * 8 + rl;     // B tile row (= output channel n0 + r); rows >= Cout: beyond wt_bytes
    b_voff[i] = (unsigned)(n0 + r) * (unsigned)p.Krow * 4u + dma_swizzle(slot, r);
  }
  // wave-uniform LDS byte addresses of this wave's DMA instructions (stage 0)
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  char* const lds_b = reinterpret_cast<char*>(lds);
  // (the low 32 bits of a generic pointer into LDS are the LDS byte offset)
  const unsigned lds0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)lds_b);

  // unit-stride launches only (no parity phases): tap t's weights start at K offset t * Cin, so the weight-row byte
  // offset of a K-step is a plain scalar counter
  int l_tap = 0, l_c0 = 0;
  unsigned l_toff = (unsigned)p.tap_off[0], k_byte = 0u;
  unsigned a_cur[AR];
  auto issue_tiles = [&](int stage) {
    if (l_c0 == 0) {
#pragma unroll
      for (int i = 0; i < AR; ++i) a_cur[i] = ((a_mask[i] >> l_tap) & 1u) ? a_off[i] + l_toff : TBN_OOB;
    }
    // (the loop-carried counters end up in VGPRs -- SIFixSGPRCopies -- and an "s" asm operand is not legalised: readfirstlane)
    const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(l_c0 * 4);
    const unsigned st = lds0 + (unsigned)(stage * TILE_B);
#pragma unroll
    for (int i = 0; i < AR; ++i) lds_dma16(in_rsrc, st + (unsigned)((wv * AR + i) * 1024), a_cur[i], soff);
    const unsigned koff = (unsigned)__builtin_amdgcn_readfirstlane((int)k_byte);
#pragma unroll
    for (int i = 0; i < NT; ++i) lds_dma16(wt_rsrc, st + (unsigned)(BM * 128 + (wv + 4 * i) * 1024), b_voff[i], koff);
    k_byte += 128u;
    l_c0 += 32;
    if (l_c0 == p.Cin) {
      l_c0 = 0;
      ++l_tap;
      if (l_tap < p.ntaps) l_toff = (unsigned)p.tap_off[l_tap];
    }
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // fragment addresses (bytes, stage 0): logical 16-B chunk (2 kg + lhalf) of row r sits at slot chunk ^ f(r)
  const int lrow = lane & 31, lhalf = lane >> 5;
  unsigned fa_addr[MT][4], fb_addr[NT][4];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int r = wave * 32 * MT + i * 32 + lrow;
#pragma unroll
    for (int kg = 0; kg < 4; ++kg) fa_addr[i][kg] = (unsigned)(r * 128) + dma_swizzle(2 * kg + lhalf, r);
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int r = j * 32 + lrow;
#pragma unroll
    for (int kg = 0; kg < 4; ++kg)
      fb_addr[j][kg] = (unsigned)(BM * 128 + r * 128) + dma_swizzle(2 * kg + lhalf, r);
  }

  const int ksteps = p.K >> 5;
  issue_tiles(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();   // publishes stage 0

  auto compute = [&](const char* sb) {
    CONV_KSTEP(sb + fa_addr[i][kg], sb + fb_addr[j][kg])
  };
  // two K-steps per iteration: the stage is a compile-time constant (fragment offsets stay immediates)
  for (int ks = 0; ks < ksteps; ks += 2) {
    if (ks + 1 < ksteps) issue_tiles(1);     // stage 1 was last read in step ks - 1: every wave is past that barrier
    compute(lds_b);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA of the next stage has landed ...
    __syncthreads();                                    // ... and so has everyone else's
    if (ks + 1 >= ksteps) break;
    if (ks + 2 < ksteps) issue_tiles(0);
    compute(lds_b + TILE_B);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  conv_epilogue<MT, NT, EPI, RED>(p, acc, lds, tm, m0, n0);
}

template <int MT, int NT, int EPI, bool RED>
__global__ __launch_bounds__(256) void conv_dma_kernel(ConvP p, RiderP rider) {
  __shared__ __attribute__((aligned(1024))) float lds[2 * (128 * MT + 32 * NT) * 32];
  TBN_RIDER_DISPATCH(rider, bid)
  conv_dma_body<MT, NT, EPI, RED>(p, bid, lds);
}

// ------------------------------------------------------------------------------------------
// Small-M GEMMs (the 7x7 / 8x8 maps: M = 4704 rows at 96 frames; the head Linear layers: M = 96): with 128-row tiles
// the grid is 37 M-tiles x a few N-tiles -- e.g. 259 workgroups for Cout = 224, one round of 256 CUs plus three
// stragglers that double the launch time.  Here a workgroup owns a (32*MT) x (32*NT) tile and its FOUR WAVES SPLIT K
// (wave w takes the 32-float K chunks w, w+4, ...): 4x more, 4x smaller tiles (1029 for that layer) that balance over the
// CUs, and K = 9 * Cin is long enough that a quarter of it still amortises the tile's prologue.  Each wave stages its own
// A / B chunk in a wave-private LDS tile -- no workgroup barrier in the K loop (wave-private LDS operations execute
// in program order) -- the four partial tiles are summed through LDS in fixed order (deterministic) and wave 0 runs the
// usual epilogue on the finished tile (conv_epilogue with WM = 1: partial-sum rows go straight to global memory).
template <int MT, int NT, int EPI, bool RED>
__device__ __forceinline__ void conv_sk4_body(const ConvP& p, const int bid, float* lds) {
  constexpr int BM = 32 * MT, BN = 32 * NT;
  constexpr int AR = 4 * MT, BR = 4 * NT;   // float4 loads per lane per K-step: 8 tile rows per wave instruction
  constexpr int TILE_F = (BM + BN) * LDT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int tm, tn;
  xcd_tile(bid, p.tiles_m, p.tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const i32x4 in_rsrc = make_rsrc(p.in, p.in_bytes);
  const i32x4 wt_rsrc = make_rsrc(p.wt, p.wt_bytes);

  const int c4 = lane & 7, r0 = lane >> 3;
  unsigned a_off[AR], a_mask[AR];
  {
    // the four waves stage the SAME 32*MT rows (different K chunks): decoded once per row into an LDS table instead of
    // by every lane of every wave (32x redundant: ~35 VALU x 4*MT rows per lane)
    unsigned* rowtab = reinterpret_cast<unsigned*>(lds);   // [BM][2]: nothing is staged yet
    if (tid < BM) {
      const int m = m0 + tid;
      unsigned mask = 0, off = 0;
      CONV_ROW_DECODE(false, m, off, mask)
      rowtab[2 * tid] = off;
      rowtab[2 * tid + 1] = mask;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const uint2 e = *reinterpret_cast<const uint2*>(&rowtab[2 * (r0 + 8 * i)]);
      a_off[i] = e.x;
      a_mask[i] = e.y;
    }
    __syncthreads();   // the table is dead: the waves' private tiles may overwrite it
  }
  unsigned b_voff[BR];
#pragma unroll
  for (int i = 0; i < BR; ++i) b_voff[i] = (unsigned)(n0 + r0 + 8 * i) * (unsigned)p.Krow * 4u + (unsigned)c4 * 16u;

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int ksteps = p.K >> 5, cpt = p.Cin >> 5;
  int l_tap = wave / cpt, l_c0 = (wave - l_tap * cpt) * 32;   // (tap, channel offset) of this wave's next chunk (scalar)
  float* As = lds + wave * TILE_F;
  float* Bs = As + BM * LDT;
  float4 ra[AR], rb[BR];
  auto load_tiles = [&]() {
    const unsigned toff = (unsigned)p.tap_off[l_tap] + (unsigned)c4 * 16u, soff = (unsigned)l_c0 * 4u;
#pragma unroll
    for (int i = 0; i < AR; ++i) ra[i] = buf_load4(in_rsrc, ((a_mask[i] >> l_tap) & 1u) ? a_off[i] + toff : TBN_OOB, soff);
    const unsigned koff = ((unsigned)p.tap_koff[l_tap] + (unsigned)l_c0) * 4u;
#pragma unroll
    for (int i = 0; i < BR; ++i) rb[i] = buf_load4(wt_rsrc, b_voff[i], koff);   // rows >= Cout: beyond wt_bytes -> zeros
    l_c0 += 128;                 // four chunks on
    while (l_c0 >= p.Cin) {
      l_c0 -= p.Cin;
      ++l_tap;
    }
  };
  auto store_tiles = [&]() {
#pragma unroll
    for (int i = 0; i < AR; ++i) *reinterpret_cast<float4*>(&As[(r0 + 8 * i) * LDT + c4 * 4]) = ra[i];
#pragma unroll
    for (int i = 0; i < BR; ++i) *reinterpret_cast<float4*>(&Bs[(r0 + 8 * i) * LDT + c4 * 4]) = rb[i];
  };
  const int lrow = lane & 31, lhalf = lane >> 5;
  if (wave < ksteps) {
    load_tiles();
    store_tiles();
  }
  for (int q = wave; q < ksteps; q += 4) {
    const bool more = q + 4 < ksteps;
    __builtin_amdgcn_wave_barrier();
    if (more) load_tiles();   // in flight under the MFMA phase
    CONV_KSTEP(&As[(i * 32 + lrow) * LDT + kg * 8 + lhalf * 4], &Bs[(j * 32 + lrow) * LDT + kg * 8 + lhalf * 4])
    __builtin_amdgcn_wave_barrier();
    if (more) store_tiles();   // behind this step's fragment reads in the wave's LDS queue
  }
  __syncthreads();   // the reduction buffer overlays every wave's tile
  float* red = lds;  // [3 waves][MT*NT][16][64 lanes]
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) red[(((wave - 1) * MT * NT + i * NT + j) * 16 + e) * 64 + lane] = acc[i][j][e];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int o = ((i * NT + j) * 16 + e) * 64 + lane;
        acc[i][j][e] = ((acc[i][j][e] + red[o]) + red[MT * NT * 1024 + o]) + red[2 * MT * NT * 1024 + o];
      }
  conv_epilogue<MT, NT, EPI, RED, 1>(p, acc, lds, tm, m0, n0);
}

template <int MT, int NT, int EPI, bool RED>
__global__ __launch_bounds__(256) void conv_sk4_kernel(ConvP p, RiderP rider) {
  __shared__ __attribute__((aligned(16))) float lds[4 * (32 * MT + 32 * NT) * LDT];
  TBN_RIDER_DISPATCH(rider, bid)
  conv_sk4_body<MT, NT, EPI, RED>(p, bid, lds);
}

#undef CONV_KSTEP
#undef CONV_ROW_DECODE

// The four output-parity phases of a stride-2 data gradient in ONE launch: each phase alone is a small GEMM
// (M / 4 rows, 1-4 taps) that leaves most CUs idle; a workgroup finds its phase by a scalar scan.
struct ConvPhases {
  ConvP ph[4];
  int blk0[5];
  int n;
};
template <int MT, int NT, int STAGES, bool RED = false>
__global__ __launch_bounds__(256) void conv_igemm_phases_kernel(ConvPhases q, RiderP rider) {
  __shared__ __attribute__((aligned(16))) float lds[STAGES * (128 * MT + 32 * NT) * LDT];
  TBN_RIDER_DISPATCH(rider, bid)
  int ph = 0;
  while (ph + 1 < q.n && bid >= q.blk0[ph + 1]) ++ph;
  conv_igemm_body<MT, NT, false, 3, STAGES, RED>(q.ph[ph], bid - q.blk0[ph], lds);
}

// ------------------------------------------------------------------------------------------
// Weight gradient:  dW[co][tap][ci] = sum_m dy[m][co] * x[pix(m) + tap][ci]
// GEMM with the *pixel* index as the reduction dim.  Both operands are read as K-major rows
// (pixel rows, channel-contiguous) and used straight from a [k][32*T+4] LDS tile with
// ds_read_b32 fragments (lane -> (k = lane>>5, i = lane&31) is conflict-free).  Each of the 4
// waves of a workgroup reduces a different quarter of the workgroup's pixel range over the same
// (32*MT co) x (32*NT ci) tile of one filter tap; the 4 partial tiles are summed through LDS
// in fixed order (deterministic), then stored to `out` (final dW or a split-K slab).
// MODE 0: any filter / stride / pad (the x row of an output pixel is found from its in-frame index, see below);
//      1: the packed-row stem (ROWMODE of conv_igemm_body: the "Cin" columns are R runs of `rl` floats of a physically
//         zero-padded image, no masks);  2: pointwise (1x1 / stride 1 / pad 0, and the Linear layers): x row = dy row.
// VALU diet (the fp32 MFMA shares its issue port with the VALU: every VALU instruction in this loop is ~4 of an MFMA's 64
// cycles, and a (64-row) step of a 64 x 64 tile is only 32 MFMAs).  A lane owns ONE pixel row of the 16-row step
// (row = l >> 2) and the float4 columns {q, q+4, q+8, ...} (q = l & 3).  Round 2 decoded the row from scratch every
// step (two 64-bit magic divisions, bounds compares, one select per load for ragged column tiles: 38-46 VALU per
// step, 1.3 per MFMA for the 64 x 64 tile, 2.4 for 64 x 32).  Now the row state advances incrementally:
//   * dy: byte offset += 64 rows; rows >= M lie beyond the buffer extent (the hardware returns zeros), a split never
//     ends inside a step (rows_per_split is a multiple of 64), column offsets ride in the instruction's immediate;
//     ragged column tiles read finite neighbours / zeros beyond the extent into accumulator rows that are never stored;
//   * x: the in-frame output pixel index pp (+= 64 mod OH*OW with one conditional wrap, the frame byte base follows)
//     gives (oy, ox) with ONE v_mul_hi (exact: pp * OW < 2^32), the input pixel with 24-bit multiply-adds;
//   pointwise layers need none of it (2 VALU per step), the general form 15, the stem 11 + one add per load.
template <int MT, int NT, int MODE>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradP p) {
  constexpr bool ROWMODE = (MODE == 1);
  constexpr int WA = 32 * MT + 4, WB = 32 * NT + 4;  // LDS pitches (a +16 pad removes the write conflicts but gains nothing)
  constexpr int KR = 16;                             // pixel rows per wave step
  constexpr int TILE = KR * (WA + WB);
  constexpr int LDSF = (4 * TILE > 4 * 1024 ? 4 * TILE : 4 * 1024);
  __shared__ __attribute__((aligned(16))) float lds[LDSF];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* At = lds + wave * TILE;
  float* Bt = At + KR * WA;

  // block -> (split, tap, tile_ci, tile_co), split slowest.  All tiles x taps of one split re-read the same
  // dy / x row slab, so the XCD-aware bijective remap (blocks b, b+8, ... share an XCD and its L2) hands each
  // XCD a CONTIGUOUS run of logical ids: a slab is then fetched into one L2 instead of all eight.
  int b = xcd_remap(blockIdx.x, gridDim.x);
  const int tco = b % p.tiles_co;
  b /= p.tiles_co;
  const int tci = b % p.tiles_ci;
  b /= p.tiles_ci;
  const int tap = b % p.taps;
  const int split = b / p.taps;
  const int co0 = tco * 32 * MT, ci0 = tci * 32 * NT;
  int r, s;
  if (ROWMODE) {
    r = tap;
    s = 0;
  } else {
    r = tap / p.S;
    s = tap - r * p.S;
  }
  const int pbeg = split * p.rows_per_split;

  // K-split accumulators per sub-tile so that >= 4 independent accumulators rotate (see the main loop)
  constexpr int KS = (MT * NT >= 4) ? 1 : (MT * NT == 1 ? 4 : 2);
  f32x16 acc[MT][NT][KS];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int q = 0; q < KS; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][q][e] = 0.f;

  constexpr int AI = 2 * MT, BI = 2 * NT;
  float4 ra[AI], rb[BI];
  const int lrow16 = lane >> 2, lq = lane & 3;
  const i32x4 dy_rsrc = make_rsrc(p.dy, p.dy_bytes);
  const i32x4 x_rsrc = make_rsrc(p.x, p.x_bytes);
  // row state of this lane: row m = pbeg + (4 it + wave) * 16 + lrow16 in step `it`
  const unsigned m0 = (unsigned)(pbeg + wave * KR + lrow16);
  unsigned dyo = (m0 * (unsigned)p.dy_ld + (unsigned)(co0 + lq * 4)) * 4u;
  const unsigned dy_step = (unsigned)(4 * KR * p.dy_ld) * 4u;
  unsigned xo = 0, pp = 0, fb = 0;
  unsigned rm_off[BI];
  if (MODE == 2) {
    xo = (m0 * (unsigned)p.x_ld + (unsigned)(ci0 + lq * 4)) * 4u;
  } else {
    const uint32_t n = fdiv(m0, p.div_ohw);
    pp = m0 - n * p.div_ohw.d;
    fb = n * p.frame_bytes + (ROWMODE ? 0u : (unsigned)(ci0 + lq * 4) * 4u);
    if (ROWMODE) {
      // this lane's columns are fixed: their (run, offset) byte displacements from the pixel's first run, once
#pragma unroll
      for (int k = 0; k < BI; ++k) {
        const int cc = ci0 + lq * 4 + 16 * k;
        const uint32_t f = (uint32_t)cc >> 2, t = fdiv(f, p.div_rl4);
        rm_off[k] = (t * (uint32_t)(p.W * p.cp) + (f - t * p.div_rl4.d) * 4u) * 4u;
      }
    }
  }
  const unsigned x_step = (unsigned)(4 * KR * p.x_ld) * 4u;
  const int tap_y = r - p.pad, tap_x = s - p.pad;
  const unsigned xld4 = (unsigned)p.x_ld * 4u;
#if TBN_DIAG
  bool x_ok_staged = false;   // validity of the x row in flight (cost probe below)
#endif
  auto load_tiles = [&]() {
#pragma unroll
    for (int k = 0; k < AI; ++k) ra[k] = buf_load4(dy_rsrc, dyo + 64u * k);
    dyo += dy_step;
    if (MODE == 2) {
#pragma unroll
      for (int k = 0; k < BI; ++k) rb[k] = buf_load4(x_rsrc, xo + 64u * k);
      xo += x_step;
    } else {
      const unsigned oy = p.mul_ow != 0u ? __umulhi(pp, p.mul_ow) : pp;   // (OW == 1: the magic number 2^32 does not fit)
      const unsigned ox = pp - __umul24(oy, (unsigned)p.OW);
      if (MODE == 0) {
        const unsigned iy = __umul24(oy, (unsigned)p.stride) + (unsigned)tap_y;   // wraps below zero: fails the unsigned compare
        const unsigned ix = __umul24(ox, (unsigned)p.stride) + (unsigned)tap_x;
        const bool ok = (iy < (unsigned)p.H) && (ix < (unsigned)p.W);
        const unsigned off = fb + __umul24(__umul24(iy, (unsigned)p.W) + ix, xld4);
        const unsigned voff = ok ? off : TBN_OOB;
#if TBN_DIAG
        x_ok_staged = ok;
#endif
#pragma unroll
        for (int k = 0; k < BI; ++k) rb[k] = buf_load4(x_rsrc, voff + 64u * k);
      } else {
        // no masks: the border is in the image; rows >= M start beyond the image extent -> zeros
        const unsigned off = fb + __umul24(oy, p.row_step) + __umul24(ox, p.col_step);
#pragma unroll
        for (int k = 0; k < BI; ++k) rb[k] = buf_load4(x_rsrc, off + rm_off[k]);
      }
      // 64 rows on: in-frame index and frame base (64 = q64 * OH*OW + r64)
      pp += p.r64;
      const bool wrap = pp >= p.div_ohw.d;
      pp = wrap ? pp - p.div_ohw.d : pp;
      fb += wrap ? p.fb_hi : p.fb_lo;
    }
  };
#if TBN_DIAG
  // cost probe (see ConvP::fold_scale): BN apply + ReLU of the producer layer on the staged x rows; out-of-image taps stay zero
  float4 fsc[BI], fsh[BI];
  if (MODE == 0 && p.fold_scale != nullptr) {
#pragma unroll
    for (int k = 0; k < BI; ++k) {
      const int cc = min(ci0 + lq * 4 + 16 * k, p.Cin - 4);
      fsc[k] = *reinterpret_cast<const float4*>(p.fold_scale + cc);
      fsh[k] = *reinterpret_cast<const float4*>(p.fold_shift + cc);
    }
  }
#endif
  auto store_tiles = [&]() {
#if TBN_DIAG
    if (MODE == 0 && p.fold_scale != nullptr) {
#pragma unroll
      for (int k = 0; k < BI; ++k) {
        rb[k].x = x_ok_staged ? fmaxf(fmaf(rb[k].x, fsc[k].x, fsh[k].x), 0.f) : 0.f;
        rb[k].y = x_ok_staged ? fmaxf(fmaf(rb[k].y, fsc[k].y, fsh[k].y), 0.f) : 0.f;
        rb[k].z = x_ok_staged ? fmaxf(fmaf(rb[k].z, fsc[k].z, fsh[k].z), 0.f) : 0.f;
        rb[k].w = x_ok_staged ? fmaxf(fmaf(rb[k].w, fsc[k].w, fsh[k].w), 0.f) : 0.f;
      }
    }
#endif
#pragma unroll
    for (int k = 0; k < AI; ++k) *reinterpret_cast<float4*>(&At[lrow16 * WA + lq * 4 + 16 * k]) = ra[k];
#pragma unroll
    for (int k = 0; k < BI; ++k) *reinterpret_cast<float4*>(&Bt[lrow16 * WB + lq * 4 + 16 * k]) = rb[k];
  };

  // The LDS tiles are wave-private and a wave's LDS operations execute in program order, so the main loop
  // needs NO workgroup barrier: the four waves run decoupled (wave_barrier only pins the compiler's order).
  const int nsteps = (p.rows_per_split + 4 * KR - 1) / (4 * KR);
  const int lrow = lane & 31, lhalf = lane >> 5;
  load_tiles();
  for (int it = 0; it < nsteps; ++it) {
    if (!WABL(2) || it == 0) store_tiles();
    __builtin_amdgcn_wave_barrier();
    if (it + 1 < nsteps && !WABL(1)) load_tiles();
    if (WABL(4)) continue;
    // Fragments of k-pair kp+1 are read while k-pair kp multiplies (two register sets; the sched_group_barrier
    // chain pins the DS-read group / MFMA group alternation).  Consecutive MFMAs rotate over FOUR independent
    // accumulators: a dependent MFMA is only free right behind its producer or >= 4 MFMAs later -- alternating
    // two accumulators halves the rate (scripts/ubench, conv_igemm_kernel) -- so tiles with fewer than four
    // 32x32 sub-tiles split K over KS accumulators per sub-tile (summed before the cross-wave reduction).
    float a[2][MT], bb[2][NT];
    auto frag = [&](int buf, int kp) {
#pragma unroll
      for (int i = 0; i < MT; ++i) a[buf][i] = At[(2 * kp + lhalf) * WA + i * 32 + lrow];
#pragma unroll
      for (int j = 0; j < NT; ++j) bb[buf][j] = Bt[(2 * kp + lhalf) * WB + j * 32 + lrow];
    };
    frag(0, 0);
#pragma unroll
    for (int kp = 0; kp < KR / 2; ++kp) {
      if (kp + 1 < KR / 2) frag((kp + 1) & 1, kp + 1);
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j][kp % KS] =
              __builtin_amdgcn_mfma_f32_32x32x2f32(a[kp & 1][i], bb[kp & 1][j], acc[i][j][kp % KS], 0, 0, 0);
    }
    {
      constexpr int NM = MT * NT;
      constexpr int NRD = (MT + 1) / 2 + (NT + 1) / 2;   // b32 fragment reads are merged pairwise into ds_read2_b32
      __builtin_amdgcn_sched_group_barrier(0x100, 2 * NRD, 0);
#pragma unroll
      for (int g = 0; g < KR / 2 - 2; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, NRD, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * NM, 0);
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();  // the reduction buffer below overlays every wave's tiles

  // cross-wave reduction, one 32x32 sub-tile at a time: red[wave][32*32]
  float* red = lds;
  float* obase = p.out + (size_t)split * p.Cout * p.K;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = 8 * (e >> 2) + 4 * lhalf + (e & 3);
        float v = acc[i][j][0][e];
#pragma unroll
        for (int q = 1; q < KS; ++q) v += acc[i][j][q][e];
        red[wave * 1024 + row * 32 + lrow] = v;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int el = tid + 256 * t;
        const float v = (red[el] + red[1024 + el]) + (red[2048 + el] + red[3072 + el]);
        const int row = el >> 5, col = el & 31;
        const int co = co0 + i * 32 + row, ci = ci0 + j * 32 + col;
        if (co < p.Cout && ci < p.Cin) obase[(size_t)co * p.K + tap * p.Cin + ci] = v;
      }
      __syncthreads();
    }
}

// Sums the split-K slabs of a weight gradient.  256 threads = (256 / SG) float4 outputs x SG slab lanes: lane g adds
// slabs g, g+SG, ... (two independent chains), the SG partial sums are combined through LDS in fixed order
// (deterministic).  SG = 16 for many slabs of a small matrix (the 7x7 stem: ~110 slabs of 57 KB) so that the
// grid still covers the chip; SG = 4 otherwise.
template <int SG>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                            int n4, int splits, size_t slab4) {
  constexpr int NO = 256 / SG;
  __shared__ float4 red[256];
  const int o = threadIdx.x % NO, g = threadIdx.x / NO;
  const int i = blockIdx.x * NO + o;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  if (i < n4) {
    int s = g;
    for (; s + SG < splits; s += 2 * SG) {
      const float4 u = tbn_ld4<(TBN_BN_NT & 8) != 0>(part + 4 * ((size_t)s * slab4 + i)), v = tbn_ld4<(TBN_BN_NT & 8) != 0>(part + 4 * ((size_t)(s + SG) * slab4 + i));
      a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
      b.x += v.x; b.y += v.y; b.z += v.z; b.w += v.w;
    }
    if (s < splits) {
      const float4 u = tbn_ld4<(TBN_BN_NT & 8) != 0>(part + 4 * ((size_t)s * slab4 + i));
      a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
    }
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  }
  red[threadIdx.x] = a;
  __syncthreads();
  if (g == 0 && i < n4) {
#pragma unroll
    for (int k = 1; k < SG; ++k) {
      const float4 v = red[k * NO + o];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    reinterpret_cast<float4*>(out)[i] = a;
  }
}

// Wt[ci][T-1-tap][co] = W[co][tap][ci]  (tap-flipped, channel-transposed weights for dgrad)
__global__ void weight_flip_transpose_kernel(const float* __restrict__ w, float* __restrict__ wt, int Cout, int taps,
                                             int Cin) {
  __shared__ float tile[32][33];
  const int tap = blockIdx.z;
  const int co0 = blockIdx.y * 32, ci0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int co = co0 + i, ci = ci0 + tx;
    tile[i][tx] = (co < Cout && ci < Cin) ? w[((size_t)co * taps + tap) * Cin + ci] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int ci = ci0 + i, co = co0 + tx;
    if (ci < Cin && co < Cout) wt[((size_t)ci * taps + (taps - 1 - tap)) * Cout + co] = tile[tx][i];
  }
}

// ------------------------------------------------------------------------------------------ host
// The epilogue a launch runs: template argument EPI (0 plain, 1 BN statistics, 2 eval BN + ReLU, 3 plain with the strided
// scatter of a parity phase) and RED (a plain epilogue that also forms the BN-backward reduce partials).  The ONE place
// that maps launch parameters to them: the kernel dispatch of every family and the profiler's kernel names both read it.
struct EpiSel {
  int epi;
  bool red;
};
static EpiSel conv_epilogue(int mode, int nred, bool scatter, bool rowmode) {
  const int epi = mode == CONV_EPI_STATS ? 1 : (mode == CONV_EPI_EVAL ? 2 : ((scatter && !rowmode) ? 3 : 0));
  return {epi, epi == 0 && nred > 0 && !rowmode};
}
// f(integral_constant<int, EPI>, bool_constant<RED>) for the selected epilogue.  SCATTER / REDUCE: whether the kernel
// family has epilogue 3 / the RED form at all -- a combination outside the family's set is refused, never instantiated
template <bool SCATTER, bool REDUCE, class F>
static int with_epilogue(EpiSel e, F&& f) {
  if (e.epi == 1) return f(std::integral_constant<int, 1>{}, std::false_type{});
  if (e.epi == 2) return f(std::integral_constant<int, 2>{}, std::false_type{});
  if constexpr (SCATTER)
    if (e.epi == 3) return f(std::integral_constant<int, 3>{}, std::false_type{});
  if constexpr (REDUCE)
    if (e.epi == 0 && e.red) return f(std::integral_constant<int, 0>{}, std::true_type{});
  if (e.epi == 0 && !e.red) return f(std::integral_constant<int, 0>{}, std::false_type{});
  tbn_set_error("conv: epilogue %d%s is not built for this kernel family", e.epi, e.red ? " + reduce" : "");
  return TBN_ERR_UNSUPPORTED;
}
// the instantiation's name as the profiler reports it: kernel<mt, nt, [rowmode, ]epi[, stages][, true]>
static void conv_kernel_name(char (&nm)[64], const char* kernel, int mt, int nt, const char* rowmode, EpiSel e, int stages) {
  char stg[8] = "";
  if (stages > 0) snprintf(stg, sizeof(stg), ", %d", stages);
  snprintf(nm, sizeof(nm), "%s<%d, %d, %s%d%s%s>", kernel, mt, nt, rowmode, e.epi, stg, e.red ? ", true" : "");
}

// the rider of a launch as the by-value kernel argument: a copy of *rider, or all zeros (span 0: no rider)
static RiderP& rider_arg(const RiderP* rider) {
  static thread_local RiderP rd;
  if (rider != nullptr)
    rd = *rider;
  else
    memset(&rd, 0, sizeof(rd));
  return rd;
}
// LDS stages of the register-staged kernel where the caller does not say: big tiles take one (keeps 2 workgroups per CU)
static int conv_stages(int asked, int mt) { return (asked == 1 || asked == 2) ? asked : ((mt == 1) ? 2 : 1); }
// Longest workgroups first: the dispatcher hands out workgroups in block order, so the members of a joint launch (parity
// phases, a pair) are ordered by the length of their K loop -- a launch should not end with its long workgroups running
// alone.  A/B runs: TBN_LPT=0 keeps the original order.
static bool conv_longest_first() {
  static const int lpt = tbn_env_int("TBN_LPT", 1, 0, 1);
  return lpt != 0;
}

// `rd` = the rider riding in this launch (rd.span == 0: none), `grid` = GEMM workgroups + rd.span (tbn_rider_place)
template <int MT, int NT, bool RM, int EPI, bool RED>
static int launch_conv_e(const ConvP& p, const RiderP& rd, int grid, hipStream_t st) {
  if (p.stages == 2)
    TBN_LAUNCH((conv_igemm_kernel<MT, NT, RM, EPI, 2, RED>), dim3(grid), dim3(256), 0, st, p, rd);
  else
    TBN_LAUNCH((conv_igemm_kernel<MT, NT, RM, EPI, 1, RED>), dim3(grid), dim3(256), 0, st, p, rd);
  return TBN_OK;
}

// LDS bytes of the halo kernel; 0 if the shape is not a 3x3 / stride 1 / pad 1 layer it handles
size_t tbn_conv_halo_lds_bytes(const ConvP& p, int mt, int nt) {
  if (p.R != 3 || p.S != 3 || p.stride != 1 || p.pad != 1 || p.up != 1 || p.OH != p.H || p.OW != p.W || p.W > 64) return 0;
  return (size_t)(128 * mt + 2 * p.W + 3 + 2 * 32 * nt) * LDT * sizeof(float);
}

template <int MT, int NT, int EPI, bool RED>
static int launch_halo_e(const ConvP& p, const RiderP& rd, int grid, size_t lds_bytes, hipStream_t st) {
  static size_t allowed = TBN_DYN_LDS_DEFAULT;   // per instantiation
  const int rc = tbn_raise_dyn_lds(reinterpret_cast<const void*>(&conv_halo_kernel<MT, NT, EPI, RED>), lds_bytes, allowed, "conv_halo");
  if (rc != TBN_OK) return rc;
  TBN_LAUNCH((conv_halo_kernel<MT, NT, EPI, RED>), dim3(grid), dim3(256), lds_bytes, st, p, rd);
  return TBN_OK;
}

void tbn_conv_pick_tile(int M, int Cout, int K, int* mt_out, int* nt_out) {
  double best = 1e300;
  int bm = 1, bn = 1;
  for (int mt = 1; mt <= 2; ++mt)
    for (int nt = 1; nt <= 4; ++nt) {
      const int tiles_m = cdiv(M, 128 * mt), tiles_n = cdiv(Cout, 32 * nt);
      const double blocks = (double)tiles_m * tiles_n;
      const double rounds = (double)((long)((blocks + 255) / 256));
      // MFMA cycles per k-step per wave + fixed per-step (barriers, exposed latency) + per-block cost
      const double per_block = (K / 32.0) * (mt * nt * 1024.0 + 350.0) + 4000.0;
      // wasted columns in the last N tile still cost load/issue slots but no MFMA (skipped)
      double cost = rounds * per_block;
      // prefer bigger tiles on ties (less L2 traffic)
      cost *= 1.0 + 0.01 / (mt * nt);
      if (cost < best) {
        best = cost;
        bm = mt;
        bn = nt;
      }
    }
  *mt_out = bm;
  *nt_out = bn;
}

// Stride-2 data gradient, one axis: filter tap r reaches a real (not zero-inserted) dy sample of the output pixels of
// parity `par` when par - pad + r is even; *d = that sample's offset in dy (the number halved is even, possibly
// negative: the division is exact)
static bool parity_tap(int par, int pad, int r, int* d) {
  const int o = par - pad + r;
  *d = o / 2;
  return (o & 1) == 0;
}
// one axis of a parity phase: does any of the `ksize` taps contribute to the output pixels of parity `par`
static bool parity_has_tap(int par, int pad, int ksize) {
  int d;
  for (int r = 0; r < ksize; ++r)
    if (parity_tap(par, pad, r, &d)) return true;
  return false;
}

// number of partial rows (M tiles) a data-gradient launch with a fused BN-backward reduce writes per reduce segment: the
// M tiles of every parity phase that launches (tbn_launch_conv skips a parity with pixels but no tap: 1x1 / stride 2).
// ksize / pad: the FORWARD layer's (the launch pads by ksize - 1 - pad)
int tbn_conv_red_rows(int N, int OH, int OW, int up, int ksize, int pad, int tile_rows) {
  if (up == 1) return cdiv(N * OH * OW, tile_rows);
  int rows = 0;
  for (int py = 0; py < 2; ++py)
    for (int px = 0; px < 2; ++px) {
      const int ohs = (OH - py + 1) / 2, ows = (OW - px + 1) / 2;
      if (ohs <= 0 || ows <= 0) continue;
      if (!parity_has_tap(py, ksize - 1 - pad, ksize) || !parity_has_tap(px, ksize - 1 - pad, ksize)) continue;
      rows += cdiv(N * ohs * ows, tile_rows);
    }
  return rows;
}

// algorithmic HBM bytes of one conv launch: the input read once, the weights once, the output written once (read
// once more when accumulating; + the BN input read by a fused backward reduce)
static double conv_alg_bytes(const ConvP& p, int rowmode) {
  const double in = (double)p.N * p.H * p.W * (rowmode ? p.cp : p.Cin);
  double out = (double)p.M * p.Cout;
  if (p.flags & CONV_FLAG_ACCUM) out *= 2.0;
  if (p.nred > 0) out += (double)p.M * p.Cout;
  return 4.0 * (in + (double)p.Cout * p.Krow + out);
}

static int launch_conv_tiles(ConvP& p, int rowmode, int mt, int nt, hipStream_t st, const RiderP* rider) {
  if (p.flags & (CONV_FLAG_BF16X6 | CONV_FLAG_BF16X3))
    return tbn_launch_conv_bf16x(p, rowmode, mt, nt, conv_alg_bytes(p, rowmode), st, rider);
  RiderP& rd = rider_arg(rider);
  const bool scatter = (p.out_sy != 1) || (p.out_sx != 1);
  if ((mt <= 0 || nt <= 0) && !rowmode && !scatter) {
    // heuristic launches (the head Linear layers: M = 96 ... 768 rows): a grid of 128-row tiles that leaves most CUs
    // idle takes the split-K tile kernel instead (never with partial-sum epilogues: their row count is the caller's)
    if (p.halo == 0 && p.mode != CONV_EPI_STATS && p.nred == 0 && p.K >= 256 &&
        cdiv(p.M, 128) * cdiv(p.Cout, 32) <= 128)
      p.halo = 3;
    if (p.halo == 3) mt = nt = 1;
  }
  if (mt <= 0 || nt <= 0) tbn_conv_pick_tile(p.M, p.Cout, p.K, &mt, &nt);
  p.stages = conv_stages(p.stages, mt);
  // kernel family: 0 register-staged generic (the only one with packed rows and the scatter epilogue), 1 LDS-halo,
  // 2 LDS-DMA staging, 3 split-K tile (small-M layers: 32-row tiles, the four waves split K)
  const int family = (rowmode || p.halo < 1 || p.halo > 3) ? 0 : p.halo;
  static const char* const kName[4] = {"conv_igemm", "conv_halo", "conv_dma", "conv_sk4"};
  size_t lds_bytes = 0;
  if (family == 3) TBN_REQUIRE(!scatter && mt <= 2 && nt <= 2, "conv: the split-K tile kernel does not handle this launch");
  if (family == 2) TBN_REQUIRE(!scatter && mt <= 2 && nt <= 4, "conv: the LDS-DMA kernel does not handle this launch");
  if (family == 1) {
    lds_bytes = tbn_conv_halo_lds_bytes(p, mt, nt);
    TBN_REQUIRE(lds_bytes > 0 && lds_bytes <= 160 * 1024, "conv: the LDS-halo kernel does not handle this shape / tile");
    TBN_REQUIRE(!scatter && mt <= 2 && nt <= 4, "conv: unsupported halo launch (tile %dx%d)", mt, nt);
  }
  conv_set_tiles(p, family == 3 ? 32 : 128, mt, nt);
  const int grid = tbn_rider_place(&rd, p.tiles_m * p.tiles_n);
  const EpiSel es = conv_epilogue(p.mode, p.nred, scatter, rowmode != 0);
  char nm[64], kernel[32];
  snprintf(kernel, sizeof(kernel), "%s_kernel", kName[family]);
  conv_kernel_name(nm, kernel, mt, nt, family != 0 ? "" : (rowmode ? "true, " : "false, "), es, family != 0 ? 0 : p.stages);
  tbn_prof_begin(nm, p.alg_flops, st, conv_alg_bytes(p, rowmode));
  int rc;
  if (family == 3) {
    rc = with_tile<2, 2>(mt, nt, [&](auto MT, auto NT) {
      return with_epilogue<false, true>(es, [&](auto EPI, auto RED) {
        TBN_LAUNCH((conv_sk4_kernel<MT, NT, EPI, RED>), dim3(grid), dim3(256), 0, st, p, rd);
        return TBN_OK;
      });
    });
  } else if (family == 2) {
    rc = with_tile<2, 4>(mt, nt, [&](auto MT, auto NT) {
      return with_epilogue<false, true>(es, [&](auto EPI, auto RED) {
        TBN_LAUNCH((conv_dma_kernel<MT, NT, EPI, RED>), dim3(grid), dim3(256), 0, st, p, rd);
        return TBN_OK;
      });
    });
  } else if (family == 1) {
    rc = with_tile<2, 4>(mt, nt, [&](auto MT, auto NT) {
      return with_epilogue<false, true>(
          es, [&](auto EPI, auto RED) { return launch_halo_e<MT, NT, EPI, RED>(p, rd, grid, lds_bytes, st); });
    });
  } else if (rowmode) {   // packed rows: no scatter, no fused reduce
    rc = with_tile<2, 4>(mt, nt, [&](auto MT, auto NT) {
      return with_epilogue<false, false>(
          es, [&](auto EPI, auto RED) { return launch_conv_e<MT, NT, true, EPI, RED>(p, rd, grid, st); });
    });
  } else {
    rc = with_tile<2, 4>(mt, nt, [&](auto MT, auto NT) {
      return with_epilogue<true, true>(
          es, [&](auto EPI, auto RED) { return launch_conv_e<MT, NT, false, EPI, RED>(p, rd, grid, st); });
    });
  }
  tbn_prof_end(st);
  if (rc != TBN_OK) return rc;
  TBN_CHECK_LAUNCH(kName[family]);
  return TBN_OK;
}

// appends a tap to the launch's tap table: input offset (dy, dx) from the window origin pixel (padding folded in), weights
// at float `koff` of a weight row (packed rows: the runs are addressed by the kernel, no byte offset)
static void conv_push_tap(ConvP& q, int dy, int dx, int koff, bool rowmode = false) {
  const int t = q.ntaps++;
  q.tap_dy[t] = dy;
  q.tap_dx[t] = dx;
  q.tap_koff[t] = koff;
  q.tap_off[t] = rowmode ? 0 : (dy * q.W + dx) * q.in_ld * 4;
}

// validation + derived fields common to every launch form; `*single` = 1 when the launch is a single GEMM
// (up == 1: geometry completely filled), 0 when the caller still has to split it into parity phases (up == 2)
static int conv_prepare(ConvP& p, int rowmode, int* single) {
  if (rowmode) {
    // R contiguous runs of Cin floats per output pixel, read from a physically zero-padded image without masks
    // K = the R runs, padded to a multiple of 32 with the first floats of a further run (zero weights; the caller's
    // image holds that row)
    const int kruns = cdiv(cdiv(p.R * p.Cin, 32) * 32, p.Cin);   // runs the padded K touches
    p.K = cdiv(p.R * p.Cin, 32) * 32;
    TBN_REQUIRE(p.Cin % 4 == 0 && p.cp >= 1 && p.pad == 0 && p.up == 1,
                "conv: packed-row mode needs run lengths in multiples of 4 floats, pad 0 (K = %d)", p.K);
    TBN_REQUIRE((p.OH - 1) * p.stride + kruns <= p.H && (p.OW - 1) * p.stride + cdiv(p.Cin, p.cp) <= p.W,
                "conv: packed-row mode reads beyond the padded image (%dx%d)", p.H, p.W);
  } else {
    TBN_REQUIRE(p.K % 32 == 0 && p.Cin % 32 == 0, "conv: K (%d) and per-tap Cin (%d) must be multiples of 32", p.K,
                p.Cin);
    TBN_REQUIRE(p.R <= 3 && p.S <= 3, "conv: filters larger than 3x3 take the packed-row (stem) path");
  }
  TBN_REQUIRE((rowmode || p.in_ld % 4 == 0) && p.nseg >= 1 && p.nseg <= TBN_CONV_MAXSEG, "conv: bad in_ld %d / nseg %d", p.in_ld,
              p.nseg);
  TBN_REQUIRE(p.nred >= 0 && p.nred <= TBN_CONV_MAXSEG && (p.nred == 0 || (p.mode == CONV_EPI_PLAIN && !rowmode)),
              "conv: the fused BN-backward reduce belongs to a plain (data-gradient) epilogue");
  for (int i = 0; i < p.nred; ++i) {
    TBN_REQUIRE(p.red[i].col_begin % 32 == 0 && (i == 0 ? p.red[i].col_begin == 0 : p.red[i].col_begin >= p.red[i - 1].col_begin + p.red[i - 1].C),
                "conv: reduce segment %d starts at column %d (x32, ascending, disjoint)", i, p.red[i].col_begin);
    if (p.red[i].y != nullptr) {
      TBN_REQUIRE(p.red[i].partial && p.red[i].stats && p.red[i].C > 0, "conv: reduce segment %d incomplete", i);
      const size_t yb = (((size_t)p.N * p.OH * p.OW - 1) * p.red[i].y_ld + p.red[i].C) * sizeof(float);
      TBN_REQUIRE(yb < (1ull << 31), "conv: reduce segment extent %zu B >= 2 GiB", yb);
      p.red[i].y_bytes = (unsigned)yb;
    }
  }
  TBN_REQUIRE(p.up == 1 || p.up == 2, "conv: up must be 1 or 2");
  if (p.flags & CONV_FLAG_HALO) p.halo = 1;
  if (p.flags & CONV_FLAG_DMA) p.halo = 2;
  if (p.flags & CONV_FLAG_SK4) p.halo = 3;
  TBN_REQUIRE(p.M > 0, "conv: empty problem");
  const size_t in_bytes = (size_t)p.N * p.H * p.W * (rowmode ? p.cp : p.in_ld) * sizeof(float);
  TBN_REQUIRE(in_bytes < (1ull << 31), "conv: input extent %zu B >= 2 GiB (process the frames in chunks)", in_bytes);
  p.in_bytes = (unsigned)in_bytes;
  if (p.alg_flops <= 0.0) p.alg_flops = 2.0 * p.M * (double)p.Cout * p.K;
  for (int i = 0; i < p.nseg; ++i) {
    const int cols = (i + 1 < p.nseg ? p.seg[i + 1].col_begin : p.Cout) - p.seg[i].col_begin;
    const size_t ob = (((size_t)p.N * p.OH * p.OW - 1) * p.seg[i].ld + cols) * sizeof(float);
    TBN_REQUIRE(ob < (1ull << 31), "conv: output extent %zu B >= 2 GiB (process the frames in chunks)", ob);
    // the epilogue picks the destination per 32-column sub-tile: segments must start on 32-column boundaries
    TBN_REQUIRE(i == 0 || p.seg[i].col_begin % 32 == 0, "conv: segment %d starts at column %d (must be a multiple of 32)",
                i, p.seg[i].col_begin);
    p.seg_bytes[i] = (unsigned)ob;
  }
  const int taps_full = rowmode ? 1 : p.R * p.S;
  p.Krow = rowmode ? p.K : taps_full * p.Cin;
  p.wt_bytes = (unsigned)((size_t)p.Cout * p.Krow * sizeof(float));
  p.div_rl4 = make_fastdiv((uint32_t)(rowmode ? p.Cin / 4 : 1));
  if (p.up == 1) {
    TBN_REQUIRE(taps_full <= 9, "conv: at most 9 taps (3x3)");
    p.OHs = p.OH;
    p.OWs = p.OW;
    p.out_sy = p.out_sx = 1;
    p.out_oy = p.out_ox = 0;
    p.in_sy = p.in_sx = p.stride;
    p.ntaps = 0;
    for (int t = 0; t < taps_full; ++t) {
      const int r = rowmode ? 0 : t / p.S, s = rowmode ? 0 : t % p.S;
      conv_push_tap(p, r - p.pad, s - p.pad, t * p.Cin, rowmode != 0);
    }
    if (!rowmode) p.K = p.ntaps * p.Cin;
    p.ty0 = -p.pad;
    p.tny = rowmode ? 1 : p.R;
    p.tx0 = -p.pad;
    p.tnx = rowmode ? 1 : p.S;
    p.div_ohw = make_fastdiv((uint32_t)(p.OHs * p.OWs));
    p.div_ow = make_fastdiv((uint32_t)p.OWs);
    *single = 1;
    return TBN_OK;
  }
  *single = 0;
  return TBN_OK;
}

// The output-parity phases of the strided data gradient `p` (prepared, up == 2): each phase is a unit-stride GEMM over
// the output pixels of one parity with the taps that contribute there.  *empty_phase: a parity with pixels but no tap
// (1x1 / stride 2 only) -- its gradient is zero and no phase writes it.
static void conv_build_phases(const ConvP& p, ConvPhases& phases, bool* empty_phase) {
  const int full_M = p.N * p.OH * p.OW;
  phases.n = 0;
  *empty_phase = false;
  for (int py = 0; py < 2; ++py)
    for (int px = 0; px < 2; ++px) {
      ConvP q = p;
      q.OHs = (p.OH - py + 1) / 2;
      q.OWs = (p.OW - px + 1) / 2;
      if (q.OHs <= 0 || q.OWs <= 0) continue;
      q.out_sy = q.out_sx = 2;
      q.out_oy = py;
      q.out_ox = px;
      q.in_sy = q.in_sx = 1;
      q.div_ohw = make_fastdiv((uint32_t)(q.OHs * q.OWs));
      q.div_ow = make_fastdiv((uint32_t)q.OWs);
      // the tap grid of this parity: (tny x tnx) taps, the first at (ty0, tx0) (offsets grow with r / s)
      q.ntaps = 0;
      q.tny = q.tnx = 0;
      q.ty0 = q.tx0 = 1 << 20;
      int dy, dx;
      for (int r = 0; r < p.R; ++r) {
        if (!parity_tap(py, p.pad, r, &dy)) continue;
        if (q.tny++ == 0) q.ty0 = dy;
        q.tnx = 0;   // the same columns in every contributing row
        for (int s2 = 0; s2 < p.S; ++s2) {
          if (!parity_tap(px, p.pad, s2, &dx)) continue;
          if (q.tnx++ == 0) q.tx0 = dx;
          conv_push_tap(q, dy, dx, (r * p.S + s2) * p.Cin);
        }
      }
      q.M = p.N * q.OHs * q.OWs;
      q.alg_flops = p.alg_flops * ((double)q.M / full_M);
      if (q.ntaps == 0) {
        *empty_phase = true;
        continue;
      }
      q.K = q.ntaps * p.Cin;
      phases.ph[phases.n++] = q;
    }
  // longest workgroups first: a phase's K is (its taps) x Cin -- 1, 2, 2 and 4 taps for a 3x3 / stride-2 layer; with the
  // 4-tap phase LAST (parity order) its 4x longer workgroups started when the others were nearly done
  for (int a = 0; a < phases.n && conv_longest_first(); ++a)
    for (int b = a + 1; b < phases.n; ++b)
      if (phases.ph[b].K > phases.ph[a].K) {
        const ConvP t = phases.ph[a];
        phases.ph[a] = phases.ph[b];
        phases.ph[b] = t;
      }
}

// Fills the derived geometry and launches: pre-checks, conv_prepare, then a single GEMM (launch_conv_tiles) or, for
// `up == 2` (data gradient of a stride-2 conv; the caller passes stride 1, pad = k-1-pad_fwd and tap-flipped weights), the
// output-parity phases in one launch: each phase only visits the taps that hit a real (non zero-inserted) dy sample, so
// no MFMA work is spent on inserted zeros (2.25 instead of 9 taps per output pixel for 3x3).
int tbn_launch_conv(ConvP p, int rowmode, int mt, int nt, hipStream_t st, const RiderP* rider) {
  if (p.flags & CONV_FLAG_BF16X_PLANES) {   // refused here, in bf16x terms, before the generic checks see the launch
    TBN_REQUIRE((p.flags & (CONV_FLAG_BF16X6 | CONV_FLAG_BF16X3)) != 0,
                "conv: flag 128 (pre-split bf16x weight planes) is only valid with a bf16x math flag (32 / 64)");
    TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, !rowmode && bf16x_gemm_ok(p.stride, p.Cin),
                   "conv: the bf16x kernels on weight planes (flag 128) need stride 1 and cin a multiple of 32 (got stride %d, cin %d)",
                   p.stride, p.Cin);
  }
  int single = 0;
  const int prc = conv_prepare(p, rowmode, &single);
  if (prc != TBN_OK) return prc;
  if (single) return launch_conv_tiles(p, rowmode, mt, nt, st, rider);
  TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, (p.flags & (CONV_FLAG_BF16X6 | CONV_FLAG_BF16X3 | CONV_FLAG_BF16X_PLANES)) == 0,
                 "conv: the bf16x kernels (flags 32 / 64) do not compute strided data gradients");
  TBN_REQUIRE(!rowmode && p.stride == 1 && p.R == p.S && p.R * p.S <= 9, "conv: unsupported strided data gradient");
  const int full_M = p.N * p.OH * p.OW;
  {
    // the scatter epilogue forms its byte offsets as 24-bit products (output pixel) x (row pitch in bytes): v_mul_u32_u24
    // silently drops the high bits, so both factors are checked here (the 2-GiB extent checks alone do not imply it
    // for narrow pitches)
    bool pitches_ok = true;
    for (int i = 0; i < p.nseg; ++i) pitches_ok = pitches_ok && (size_t)p.seg[i].ld * 4 < (1u << 24);
    for (int i = 0; i < p.nred; ++i) pitches_ok = pitches_ok && (size_t)p.red[i].y_ld * 4 < (1u << 24);
    TBN_REQUIRE(full_M < (1 << 24) && pitches_ok,
                "conv: strided data gradient of %d output pixels / a pitch beyond the 24-bit scatter arithmetic (chunk the frames)",
                full_M);
  }
  static thread_local ConvPhases phases;   // ~2 KB kernel argument, built in place
  bool empty_phase = false;
  conv_build_phases(p, phases, &empty_phase);
  // the fused reduce sums the gradient of the pixels its phases visit: where a parity has no phase, an accumulating launch
  // leaves the earlier gradient of those pixels out of the sums
  TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, !(empty_phase && p.nred > 0 && (p.flags & CONV_FLAG_ACCUM)),
                 "conv: an accumulating 1x1 strided data gradient cannot carry the fused BN-backward reduce");
  if (empty_phase && !(p.flags & CONV_FLAG_ACCUM)) {
    // pixels no phase writes: clear the whole destination first (stream order keeps this ahead of the phases)
    TBN_REQUIRE(p.nseg == 1, "conv: 1x1 strided data gradient writes one segment");
    if (hipMemset2DAsync(p.seg[0].ptr, (size_t)p.seg[0].ld * sizeof(float), 0, (size_t)p.Cout * sizeof(float),
                         (size_t)full_M, st) != hipSuccess) {
      tbn_set_error("conv: hipMemset2DAsync failed");
      return TBN_ERR_LAUNCH;
    }
  }
  if (phases.n == 0) return TBN_OK;
  // one tile shape for all phases (picked on the largest one), one launch
  int pmt = mt, pnt = nt;
  if (pmt <= 0 || pnt <= 0) {
    int big = 0;
    for (int i = 1; i < phases.n; ++i)
      if (phases.ph[i].M > phases.ph[big].M) big = i;
    tbn_conv_pick_tile(phases.ph[big].M, p.Cout, phases.ph[big].K, &pmt, &pnt);
  }
  const int stages = conv_stages(p.stages, pmt);
  phases.blk0[0] = 0;
  int red_rows = p.red_row0;
  for (int i = 0; i < phases.n; ++i) {
    ConvP& q = phases.ph[i];
    q.stages = stages;
    conv_set_tiles(q, 128, pmt, pnt);
    q.red_row0 = red_rows;      // the phases of one layer append their M tiles to the same partial buffers
    red_rows += q.tiles_m;
    phases.blk0[i + 1] = phases.blk0[i] + q.tiles_m * q.tiles_n;
  }
  {
    char nm[64];
    snprintf(nm, sizeof(nm), "conv_igemm_phases_kernel<%d, %d, %d%s>", pmt, pnt, stages, p.nred > 0 ? ", true" : "");
    tbn_prof_begin(nm, p.alg_flops, st, conv_alg_bytes(p, 0));
  }
  RiderP& prd = rider_arg(rider);
  const int pgrid = tbn_rider_place(&prd, phases.blk0[phases.n]);
  const int rc = with_tile<2, 4>(pmt, pnt, [&](auto MT, auto NT) {
    auto go = [&](auto STG, auto RED) {
      TBN_LAUNCH((conv_igemm_phases_kernel<MT, NT, STG, RED>), dim3(pgrid), dim3(256), 0, st, phases, prd);
      return TBN_OK;
    };
    using std::integral_constant;
    if (stages == 2) return p.nred > 0 ? go(integral_constant<int, 2>{}, std::true_type{}) : go(integral_constant<int, 2>{}, std::false_type{});
    return p.nred > 0 ? go(integral_constant<int, 1>{}, std::true_type{}) : go(integral_constant<int, 1>{}, std::false_type{});
  });
  tbn_prof_end(st);
  if (rc != TBN_OK) return rc;
  TBN_CHECK_LAUNCH("conv_igemm_phases");
  return TBN_OK;
}

// ------------------------------------------------------------------------------------------
// Two INDEPENDENT convolutions in one launch: the 3x3 and double_3x3_1 layers of an inception block read different
// inputs and write different outputs, each alone leaves the chip partly idle on the 14x14 / 7x7 maps (259 .. 735
// workgroups on 256 CUs) and pays its own launch ramp and last-round tail.  One grid holds the tiles of both; a
// workgroup finds its member by a scalar compare.  Members share the tile shape, the kernel variant and the epilogue.
struct ConvPair {
  ConvP m[2];
  int blk1;   // first workgroup of member 1
};
template <int MT, int NT, int EPI, int STAGES, bool RED>
__global__ __launch_bounds__(256) void conv_pair_igemm_kernel(ConvPair q, RiderP rider) {
  __shared__ __attribute__((aligned(16))) float lds[STAGES * (128 * MT + 32 * NT) * LDT];
  TBN_RIDER_DISPATCH(rider, bid)
  const int mi = bid >= q.blk1 ? 1 : 0;
  conv_igemm_body<MT, NT, false, EPI, STAGES, RED>(q.m[mi], bid - (mi ? q.blk1 : 0), lds);
}
template <int MT, int NT, int EPI, bool RED>
__global__ __launch_bounds__(256) void conv_pair_halo_kernel(ConvPair q, RiderP rider) {
  extern __shared__ __attribute__((aligned(16))) float dyn_lds[];
  TBN_RIDER_DISPATCH(rider, bid)
  const int mi = bid >= q.blk1 ? 1 : 0;
  conv_halo_body<MT, NT, EPI, RED>(q.m[mi], bid - (mi ? q.blk1 : 0), dyn_lds);
}

template <int MT, int NT, int EPI, bool RED>
static int launch_pair_v(const ConvPair& q, const RiderP& rd, int blocks, int variant, size_t lds_bytes, hipStream_t st) {
  if (variant == 0) {   // LDS-halo members
    static size_t allowed = TBN_DYN_LDS_DEFAULT;   // per instantiation
    const int rc = tbn_raise_dyn_lds(reinterpret_cast<const void*>(&conv_pair_halo_kernel<MT, NT, EPI, RED>), lds_bytes, allowed, "conv_pair");
    if (rc != TBN_OK) return rc;
    TBN_LAUNCH((conv_pair_halo_kernel<MT, NT, EPI, RED>), dim3(blocks), dim3(256), lds_bytes, st, q, rd);
  } else if (variant == 2) {
    TBN_LAUNCH((conv_pair_igemm_kernel<MT, NT, EPI, 2, RED>), dim3(blocks), dim3(256), 0, st, q, rd);
  } else {
    TBN_LAUNCH((conv_pair_igemm_kernel<MT, NT, EPI, 1, RED>), dim3(blocks), dim3(256), 0, st, q, rd);
  }
  return TBN_OK;
}
// variant: 0 LDS-halo (both members 3x3 / stride 1), 1 / 2 register-staged generic kernel with 1 / 2 LDS stages.
// Tiles: (1,1) (1,2) (2,1) (2,2).  Both members: unit-stride launches (no parity phases), same epilogue mode, reduce
// segments on both or on neither.
int tbn_launch_conv_pair(ConvP a, ConvP b, int variant, int mt, int nt, hipStream_t st, const RiderP* rider) {
  static thread_local ConvPair q;
  if ((a.flags | b.flags) & (CONV_FLAG_BF16X6 | CONV_FLAG_BF16X3 | CONV_FLAG_BF16X_PLANES)) {
    tbn_set_error("conv_pair: the bf16x kernels (flags 32 / 64, weight planes 128) are single launches");
    return TBN_ERR_UNSUPPORTED;
  }
  RiderP& rd = rider_arg(rider);
  int sa = 0, sb = 0;
  int rc = conv_prepare(a, 0, &sa);
  if (rc != TBN_OK) return rc;
  rc = conv_prepare(b, 0, &sb);
  if (rc != TBN_OK) return rc;
  TBN_REQUIRE(sa && sb, "conv_pair: members must be unit-stride launches (no parity phases)");
  TBN_REQUIRE(a.mode == b.mode && (a.nred > 0) == (b.nred > 0) && a.flags == b.flags,
              "conv_pair: members must share the epilogue");
  TBN_REQUIRE(variant >= 0 && variant <= 2 && mt >= 1 && mt <= 2 && nt >= 1 && nt <= 2, "conv_pair: unsupported variant / tile");
  size_t lds_bytes = 0;
  if (variant == 0) {
    const size_t la = tbn_conv_halo_lds_bytes(a, mt, nt), lb = tbn_conv_halo_lds_bytes(b, mt, nt);
    TBN_REQUIRE(la > 0 && lb > 0 && la <= 160 * 1024 && lb <= 160 * 1024, "conv_pair: a member is not an LDS-halo shape");
    lds_bytes = la > lb ? la : lb;
  }
  ConvP* ms[2] = {&a, &b};
  if (b.K > a.K && conv_longest_first()) {   // the member with the longer K loop first
    ms[0] = &b;
    ms[1] = &a;
  }
  for (int i = 0; i < 2; ++i) {
    conv_set_tiles(*ms[i], 128, mt, nt);
    ms[i]->stages = variant == 2 ? 2 : 1;
    ms[i]->halo = variant == 0 ? 1 : 0;
    q.m[i] = *ms[i];
  }
  q.blk1 = ms[0]->tiles_m * ms[0]->tiles_n;
  const int blocks = tbn_rider_place(&rd, q.blk1 + ms[1]->tiles_m * ms[1]->tiles_n);
  const EpiSel es = conv_epilogue(a.mode, a.nred, false, false);
  char nm[64];
  conv_kernel_name(nm, variant == 0 ? "conv_pair_halo_kernel" : "conv_pair_igemm_kernel", mt, nt, "", es, variant);
  tbn_prof_begin(nm, a.alg_flops + b.alg_flops, st, conv_alg_bytes(a, 0) + conv_alg_bytes(b, 0));
  rc = with_tile<2, 2>(mt, nt, [&](auto MT, auto NT) {
    return with_epilogue<false, true>(
        es, [&](auto EPI, auto RED) { return launch_pair_v<MT, NT, EPI, RED>(q, rd, blocks, variant, lds_bytes, st); });
  });
  tbn_prof_end(st);
  if (rc != TBN_OK) return rc;
  TBN_CHECK_LAUNCH("conv_pair");
  return TBN_OK;
}

template <int MT, int NT, int MODE>
static void launch_wgrad(const WgradP& p, int blocks, hipStream_t st) {
  // (round 6: an LDS-DMA form of this kernel -- dy / x rows global -> LDS without the VGPR round trip, two stages per wave,
  //  bit-identical results, commit 2773a1b -- measured 7 % SLOWER per launch, 499 -> 538 us on conv2_3x3: two stages of the
  //  64 x 64 tile need 74 KB of LDS = two workgroups per CU instead of four, and a DMA issued one step ahead has 0.85 us to land;
  //  profiles/r06_ab_wgrad_dma.txt.  Removed.)
  // experiment knob (A/B runs only): unused dynamic LDS caps the workgroups per CU (the 64 x 64 tile needs 64 registers and
  // 34 KB of LDS: four per CU; each split's 54 tile x tap workgroups share an x / dy slab through the XCD's 4-MB L2)
  // (clamped to what still launches: 64 KB of dynamic LDS minus the kernel's 34 KB of static LDS)
  static const int pad = tbn_env_int("TBN_WGRAD_LDS_PAD", 0, 0, 64 * 1024 - 36 * 1024);
  TBN_LAUNCH((conv_wgrad_kernel<MT, NT, MODE>), dim3(blocks), dim3(256), (MT == 2 && NT == 2) ? pad : 0, st, p);
}

// The weight-gradient tiles, in row order: {1, 2, 3, 5} x {1, 2, 3} without (5, 3), which does not fit the register file
constexpr int kWgradTiles = 11;
constexpr int wgrad_tile_mt(int i) { return i / 3 == 3 ? 5 : i / 3 + 1; }
constexpr int wgrad_tile_nt(int i) { return i % 3 + 1; }

// f(integral_constant<int, MT>, integral_constant<int, NT>) for the weight-gradient tile (mt, nt); any tile outside the
// table above is refused (I walks it)
template <int I = 0, class F>
static int with_wgrad_tile(int mt, int nt, F&& f) {
  if constexpr (I == kWgradTiles) {
    tbn_set_error("wgrad: unsupported tile");
    return TBN_ERR_UNSUPPORTED;
  } else {
    constexpr int MT = wgrad_tile_mt(I), NT = wgrad_tile_nt(I);
    if (mt == MT && nt == NT) return f(std::integral_constant<int, MT>{}, std::integral_constant<int, NT>{});
    return with_wgrad_tile<I + 1>(mt, nt, f);
  }
}

// THE tile rule of every entry that takes a weight-gradient tile (the conv and stem C-ABI entries, plan import): 0 x 0 = the
// heuristic, or a tile of the table.  Anything else -- tbn_wgrad_plan would replace it silently -- is for the caller to refuse.
bool tbn_wgrad_tile_ok(int mt, int nt) {
  if (mt == 0 && nt == 0) return true;
  for (int i = 0; i < kWgradTiles; ++i)
    if (mt == wgrad_tile_mt(i) && nt == wgrad_tile_nt(i)) return true;
  return false;
}

// 32-column sub-tiles per workgroup along one dimension: 3 for 96 (and other odd multiples of 96), else 2 when the
// extent is a multiple of 64 or large, else 1
static int pick_wtile(int c) { return (c % 96 == 0 && c % 64 != 0) ? 3 : ((c % 64 == 0 || c > 96) ? 2 : 1); }

// plan: tile (0 = heuristic) + split-K.  The kernel's register budget admits `occ` workgroups per CU, so a grid runs
// in rounds of 256 * occ workgroups and a partly filled last round costs a full one: for every round count R = 1..8
// take the largest split count that still fits R rounds and keep the cheapest by
//   rounds * (K-steps per workgroup + 1) * step time  +  split-K reduce traffic
// (fitted to a sweep of 12 layer shapes x 24 plans, scripts/wgrad_ablate.py SWEEP=1: within 2 % of the best measured
// plan per layer, 11 % below the former "about 768 workgroups" rule on one stream).  Every split keeps >= 256 rows.
void tbn_wgrad_plan(int M, int Cout, int Cin, int taps, int* mt, int* nt, int* splits, int* rows_per_split) {
  if ((*mt < 1 || *mt > 3) && *mt != 5) {
    *mt = pick_wtile(Cout);
    // 160 output channels (3c / 4c 3x3 branches): 64-wide tiles multiply 17 % zero rows; one 160-wide tile (5 sub-tiles,
    // not the data-parallel stem path) fits exactly
    if (Cout == 160) *mt = 5;
  }
  if (*nt < 1 || *nt > 3) {
    *nt = pick_wtile(Cin);
    // 160 / 224 input channels: 64-wide tiles would multiply 20 / 14 % zero columns; 32-wide ones measured 5-22 %
    // faster there (profiles/r01_wgrad_tiles.txt).  The Cout side keeps its 64-wide tiles (narrow ones lose more
    // than the padding costs).
    if (*nt == 2 && Cin % 64 != 0 && cdiv(Cin, 64) * 64 * 100 >= Cin * 112) *nt = 1;
    // few rows, many input channels (the 1056-channel 1x1 group of 5a on the 7x7 maps): the 96-wide tile's single
    // workgroup per CU leaves 2.8 rounds of short loops; 64-wide tiles (3 % zero columns) run two per CU
    if (*nt == 3 && M <= 5120 && Cin >= 512) *nt = 2;   // (at 6144 rows, the 8x8 audio maps, the 96-wide tile still wins)
  }
  if (*mt == 5 && *nt == 3) *nt = 2;   // 5 x 3 sub-tiles do not fit the register file
  const int tiles = cdiv(Cout, 32 * *mt) * cdiv(Cin, 32 * *nt) * taps;
  const int max_splits = cdiv(M, 256);
  auto settle = [&](int s, int* rps) {
    if (s > max_splits) s = max_splits;
    if (s < 1) s = 1;
    *rps = cdiv(cdiv(M, s), 64) * 64;
    return cdiv(M, *rps);
  };
#if TBN_ABLATE
  if (const char* e = getenv("TBN_WGRAD_TARGET")) {   // scripts/wgrad_ablate.py: fixed grid target
    *splits = settle(cdiv(atoi(e), tiles), rows_per_split);
    return;
  }
#endif
  int occ = (*mt == 3 || *nt == 3 || (*mt == 5 && *nt > 1)) ? 1 : 2;   // workgroups per CU the cost model assumes
  {
    // experiment knob (A/B runs only): with VGPR-form accumulators the 64 x 64 and smaller tiles fit FOUR workgroups per CU
    static const int occ_env = tbn_env_int("TBN_WGRAD_OCC", 0, 0, 8);
    if (occ_env > 0 && occ == 2) occ = occ_env;
  }
  const int slots = 256 * occ;
  const double step_us = *mt * *nt * 8 * 64 / 2.4e3 * occ;  // 8 k-pairs x MT*NT MFMAs of 64 cycles, SIMD shared by occ waves
  const double slab_mb = (double)Cout * Cin * taps * 4e-6;
  double best = 0.0;
  for (int R = 1; R <= 8; ++R) {
    int rps;
    const int s = settle(R * slots / tiles, &rps);
    const double cost = cdiv(tiles * s, slots) * (rps / 64 + 1) * step_us + (s > 1 ? 0.3 * s * slab_mb : 0.0);
    if (R == 1 || cost < best) {
      best = cost;
      *splits = s;
      *rows_per_split = rps;
    }
  }
}

// split-K slab floats: the worst case over every tile the autotuner may choose
size_t tbn_wgrad_workspace_floats(int M, int Cout, int Cin, int taps) {
  size_t worst = 0;
  for (int mt = 1; mt <= 4; ++mt)
    for (int nt = 1; nt <= 3; ++nt) {
      int m = mt == 4 ? 5 : mt, n = nt, s, rps;
      tbn_wgrad_plan(M, Cout, Cin, taps, &m, &n, &s, &rps);
      const size_t need = s > 1 ? (size_t)s * Cout * taps * Cin : 0;
      if (need > worst) worst = need;
    }
  return worst;
}

// Every launch decision of tbn_launch_wgrad in one place (the launcher runs exactly this; tbn_conv2d_wgrad_plan reports it)
WgradLaunchPlan tbn_wgrad_launch_plan(const WgradP& p, int rowmode) {
  WgradLaunchPlan q;
  q.mt = p.mt;   // 0: heuristic tile
  q.nt = p.nt;
  tbn_wgrad_plan(p.M, p.Cout, p.Cin, p.taps, &q.mt, &q.nt, &q.splits, &q.rows_per_split);
  q.tiles_co = cdiv(p.Cout, 32 * q.mt);
  q.tiles_ci = cdiv(p.Cin, 32 * q.nt);
  q.mode = rowmode ? 1 : ((p.taps == 1 && p.stride == 1 && p.pad == 0 && p.OH == p.H && p.OW == p.W) ? 2 : 0);
  const size_t n4 = (size_t)p.Cout * p.taps * p.Cin / 4;
  // many slabs of a small matrix: 16 slab lanes per output so that the reduce grid still covers the chip
  q.reduce = q.splits > 1 ? ((q.splits >= 32 && n4 < 64 * 1024) ? 16 : 4) : 0;
  q.ws_floats = q.splits > 1 ? (size_t)q.splits * p.Cout * p.taps * p.Cin : 0;
  return q;
}

int tbn_launch_wgrad(WgradP p, int rowmode, float* dw, float* workspace, hipStream_t st) {
  TBN_REQUIRE(p.Cin % 4 == 0 && p.Cout % 4 == 0 && p.dy_ld % 4 == 0 && (rowmode || p.x_ld % 4 == 0),
              "wgrad: channel counts / pitches must be multiples of 4");
  TBN_REQUIRE(p.M > 0, "wgrad: empty problem");
  {
    // exact extents: the kernel relies on the hardware range check for rows >= M and for ragged column tiles
    const size_t xb = rowmode ? (size_t)p.N * p.H * p.W * p.cp * sizeof(float)
                              : (((size_t)p.N * p.H * p.W - 1) * p.x_ld + p.Cin) * sizeof(float);
    const size_t db = (((size_t)p.M - 1) * p.dy_ld + p.Cout) * sizeof(float);
    TBN_REQUIRE(xb < (1ull << 31) && db < (1ull << 31), "wgrad: operand extent >= 2 GiB (process the frames in chunks)");
    p.x_bytes = (unsigned)xb;
    p.dy_bytes = (unsigned)db;
  }
#if TBN_ABLATE
  if (const char* e = getenv("TBN_WGRAD_ABLATE")) p.ablate = atoi(e);
  if (const char* e = getenv("TBN_WGRAD_MT")) p.mt = atoi(e);
  if (const char* e = getenv("TBN_WGRAD_NT")) p.nt = atoi(e);
#endif
  if (rowmode) {
    TBN_REQUIRE(p.taps == 1 && p.pad == 0 && p.rl > 0 && p.rl % 4 == 0 && p.cp >= 1 && p.Cin % p.rl == 0,
                "wgrad: packed-row mode needs taps 1, pad 0, Cin = R * rl, rl a multiple of 4");
    // (the last column tile may reach into one further run: finite image data into accumulator columns never stored)
    TBN_REQUIRE((p.OH - 1) * p.stride + p.Cin / p.rl <= p.H && (p.OW - 1) * p.stride + cdiv(p.rl, p.cp) <= p.W,
                "wgrad: packed-row mode reads beyond the padded image (%dx%d)", p.H, p.W);
  }
  p.div_rl4 = make_fastdiv((uint32_t)(rowmode ? p.rl / 4 : 1));
  const WgradLaunchPlan plan = tbn_wgrad_launch_plan(p, rowmode);
  const int mt = plan.mt, nt = plan.nt, splits = plan.splits, rps = plan.rows_per_split, mode = plan.mode;
  p.K = p.taps * p.Cin;
  p.tiles_co = plan.tiles_co;
  p.tiles_ci = plan.tiles_ci;
  p.rows_per_split = rps;
  p.div_ohw = make_fastdiv((uint32_t)(p.OH * p.OW));
  p.div_ow = make_fastdiv((uint32_t)p.OW);
  // incremental row addressing (see the kernel): 64 rows per step
  TBN_REQUIRE(rps % 64 == 0, "wgrad: rows per split must be a multiple of 64");
  {
    const uint64_t ohw = (uint64_t)p.OH * p.OW;
    TBN_REQUIRE(ohw * p.OW < (1ull << 32) && p.H < (1 << 23) && p.W < (1 << 23) && (uint64_t)p.H * p.W < (1ull << 24) &&
                    (uint64_t)p.x_ld * 4 < (1ull << 24),
                "wgrad: feature map too large for the 24-bit row arithmetic");
    p.mul_ow = p.OW == 1 ? 0u : (unsigned)(((1ull << 32) + p.OW - 1) / p.OW);   // 0: oy = pp (one-column maps)
    p.r64 = (unsigned)(64 % ohw);
    p.frame_bytes = (unsigned)((size_t)p.H * p.W * (rowmode ? p.cp : p.x_ld) * sizeof(float));
    p.fb_lo = (unsigned)(64 / ohw) * p.frame_bytes;
    p.fb_hi = p.fb_lo + p.frame_bytes;
    p.row_step = (unsigned)((size_t)p.stride * p.W * p.cp * sizeof(float));
    p.col_step = (unsigned)((size_t)p.stride * p.cp * sizeof(float));
    TBN_REQUIRE(!rowmode || (p.row_step < (1u << 24) && p.col_step < (1u << 24)), "wgrad: padded image row too long");
  }
  TBN_REQUIRE(splits == 1 || workspace != nullptr, "wgrad: split-K needs a workspace");
  p.out = splits > 1 ? workspace : dw;
  const int blocks = p.tiles_co * p.tiles_ci * p.taps * splits;
  if (p.alg_flops <= 0.0) p.alg_flops = 2.0 * p.M * (double)p.Cout * p.K;
  {
    char nm[64];
    snprintf(nm, sizeof(nm), "conv_wgrad_kernel<%d, %d, %d>", mt, nt, mode);
    // algorithmic bytes: dy and x read once, dW written once (split-K slabs are overhead, not counted)
    tbn_prof_begin(nm, p.alg_flops, st,
                   4.0 * ((double)p.M * p.Cout + (double)p.N * p.H * p.W * (rowmode ? p.cp : p.Cin) + (double)p.Cout * p.K));
  }
  const int rc = with_wgrad_tile(mt, nt, [&](auto MT, auto NT) {
    if (mode == 1)
      launch_wgrad<MT, NT, 1>(p, blocks, st);
    else if (mode == 2)
      launch_wgrad<MT, NT, 2>(p, blocks, st);
    else
      launch_wgrad<MT, NT, 0>(p, blocks, st);
    return TBN_OK;
  });
  tbn_prof_end(st);
  if (rc != TBN_OK) return rc;
  TBN_CHECK_LAUNCH("conv_wgrad");
  if (splits > 1) {
    const size_t n = (size_t)p.Cout * p.K;
    const int n4 = (int)(n / 4);
    if (plan.reduce == 16)
      TBN_KLAUNCH(splitk_reduce_kernel<16>, dim3(cdiv(n4, 16)), dim3(256), 0, st, workspace, dw, n4, splits, n / 4);
    else
      TBN_KLAUNCH(splitk_reduce_kernel<4>, dim3(cdiv(n4, 64)), dim3(256), 0, st, workspace, dw, n4, splits, n / 4);
    TBN_CHECK_LAUNCH("splitk_reduce");
  }
  return TBN_OK;
}

int tbn_launch_weight_flip_transpose(const float* w, float* wt, int Cout, int taps, int Cin, hipStream_t st) {
  TBN_KLAUNCH(weight_flip_transpose_kernel, dim3(cdiv(Cin, 32), cdiv(Cout, 32), taps), dim3(256), 0, st, w,
                     wt, Cout, taps, Cin);
  TBN_CHECK_LAUNCH("weight_flip_transpose");
  return TBN_OK;
}

// All layers of a backbone in ONE launch (the per-layer launches are ~4 us of pure latency each, 50 per
// backward pass): the layer table rides in the kernel arguments, a workgroup finds its layer by a scalar binary
// search (the former linear scan over up to 64 layers made this 10 M-float transpose take 218 us) and moves one
// 32 x 32 (co, ci) tile of every filter tap.
__global__ __launch_bounds__(256) void weight_flip_transpose_all_kernel(const float* __restrict__ w,
                                                                        float* __restrict__ wt, FlipTab tab) {
  // all taps of the tile are loaded first (up to 36 loads in flight per thread), ONE barrier, then all are written:
  // the former tap-by-tap form (two barriers per 4-KB tap slice) ran the 40 MB of a backbone at ~1 TB/s
  __shared__ float tile[9][32][33];   // indexed by tap < tab.taps[l] <= 9 (checked by the launcher)
  int lo = 0, hi = tab.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int)blockIdx.x >= tab.blk0[mid])
      lo = mid;
    else
      hi = mid;
  }
  const int l = lo;
  const int Cout = tab.cout[l], Cin = tab.cin[l], taps = tab.taps[l];
  const int tci = (Cin + 31) >> 5;
  const int b = blockIdx.x - tab.blk0[l];
  const int ci0 = (b % tci) * 32, co0 = (b / tci) * 32;
  const float* wl = w + tab.w_off[l];
  float* wtl = wt + tab.w_off[l];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int tap = 0; tap < taps; ++tap)
#pragma unroll
    for (int i = ty; i < 32; i += 8) {
      const int co = co0 + i, ci = ci0 + tx;
      tile[tap][i][tx] = (co < Cout && ci < Cin) ? wl[((size_t)co * taps + tap) * Cin + ci] : 0.f;
    }
  __syncthreads();
  for (int tap = 0; tap < taps; ++tap)
#pragma unroll
    for (int i = ty; i < 32; i += 8) {
      const int ci = ci0 + i, co = co0 + tx;
      if (ci < Cin && co < Cout) wtl[((size_t)ci * taps + (taps - 1 - tap)) * Cout + co] = tile[tap][tx][i];
    }
}

int tbn_launch_weight_flip_transpose_all(const float* w, float* wt, const FlipTab& tab, hipStream_t st) {
  if (tab.n == 0) return TBN_OK;
  for (int l = 0; l < tab.n; ++l)   // the kernel stages every tap of a tile at once: tile[9][32][33]
    TBN_REQUIRE(tab.taps[l] >= 1 && tab.taps[l] <= 9, "weight_flip: layer %d has %d taps (at most 9 = 3x3)", l, (int)tab.taps[l]);
  TBN_KLAUNCH(weight_flip_transpose_all_kernel, dim3(tab.blk0[tab.n]), dim3(256), 0, st, w, wt, tab);
  TBN_CHECK_LAUNCH("weight_flip_transpose_all");
  return TBN_OK;
}
