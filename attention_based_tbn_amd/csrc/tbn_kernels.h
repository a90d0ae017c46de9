// Internal launch-level interface between the HIP kernels and the C-ABI / backbone engine.
#pragma once
#include "tbn_common.h"
#include <hip/hip_ext.h>
#include <type_traits>

enum { CONV_EPI_PLAIN = 0, CONV_EPI_STATS = 1, CONV_EPI_EVAL = 2 };
enum {
  CONV_FLAG_ACCUM = 1,
  CONV_FLAG_RELU = 2,
  CONV_FLAG_HALO = 4,   // host only: use the LDS-halo kernel
  CONV_FLAG_DMA = 8,    // host only: use the LDS-DMA staging kernel
  CONV_FLAG_SK4 = 16,   // host only: 32-row tiles whose four waves split K (small-M launches)
  CONV_FLAG_BF16X6 = 32,   // host only: split-bf16 kernel (conv_bf16x.hip), six plane products
  CONV_FLAG_BF16X3 = 64,   // host only: the same with three plane products
  CONV_FLAG_BF16X_PLANES = 128,  // host only, with 32 / 64: ConvP::wt points at pre-split bf16 weight planes (conv_bf16x.hip)
  CONV_FLAG_DESC_OUT2 = 256      // tbn_conv_desc only (consumed by the C-ABI, never reaches a launcher): its out2* fields are set
};

// BN-backward reduce fused into a data-gradient epilogue (the launch that writes the FINAL value of dz): for the output
// columns [col_begin, col_begin + C) -- one BN layer of the producer side -- the epilogue forms
//   g = dz * [y*scale+shift > 0],  S1 = sum g,  S2 = sum g * (y-mean)*rstd
// per M tile and writes them as partial[(tile*2 + {0,1}) * C + (col - col_begin)] (what bn_bwd_reduce would have
// produced from a second pass over dz and y).  y == nullptr: columns without a BN (pass-through pool slice).
#define TBN_CONV_MAXSEG 4
struct RedSeg {
  const float* y;         // BN input of that layer at column col_begin (pitch y_ld), same pixel order as the output
  float* partial;
  const float* stats;     // mean at stats[c], rstd at stats[chan + c], scale at stats[2*chan + c], shift at stats[3*chan + c]
  int y_ld, col_begin, C, c_off;
  unsigned y_bytes;
};

struct ConvP {
  const float* in;
  const float* wt;
  const float* bias;      // may be null
  const float* scale;     // EVAL epilogue
  const float* shift;     // EVAL epilogue
  float* stat_partial;    // STATS epilogue: [tiles_m][2][Cout]
  Seg seg[TBN_CONV_MAXSEG];
  int nseg;
  int raw_seg1;           // EVAL epilogue: 1 + index of a segment written as the bare accumulator (no BN fold / ReLU); 0 = none
  int in_ld;
  // fused BN-backward reduce (PLAIN epilogue of a data gradient), see RedSeg
  RedSeg red[TBN_CONV_MAXSEG];
  int nred;               // 0 = off
  int red_chan;           // stride between the mean / rstd / scale / shift arrays
  int red_row0;           // first partial row of this launch (parity phases of one layer share a partial buffer)
  // ---- caller-facing geometry (host side fills the derived fields below from these)
  int N, H, W;            // input spatial dims (for dgrad: dims of dy)
  int OH, OW;             // full output dims
  int Cin;                // K per tap (ROWMODE: floats of one contiguous input run; R runs make the K of a pixel)
  int Cout;
  int R, S, stride, pad, up;
  int M, K;               // GEMM M (output pixels of this launch) and reduction length of this launch
  int cp;                 // ROWMODE: floats per pixel of the (physically zero-padded) input image
  int tiles_m, tiles_n;
  int mode, flags;
  double alg_flops;       // host only: algorithmic FLOPs of this launch (profiling)
  int stages;             // host only: LDS stages (1 = two barriers per K-step, 2 = double buffered); 0 = default
  int halo;               // host only: 1 = LDS-halo kernel (3x3 / stride 1 / pad 1 layers: input patch staged once per chunk),
                          //            2 = LDS-DMA staging of the generic kernel, 3 = 32-row tiles with the waves splitting K
                          //            (statistics / reduce partial rows are then per 32*mt rows, not 128*mt)
  // ---- derived by tbn_launch_conv
  unsigned in_bytes, wt_bytes;          // buffer extents: out-of-range lanes read zeros (hardware check)
  unsigned seg_bytes[TBN_CONV_MAXSEG];  // extent of each output segment from seg[i].ptr
  int OHs, OWs;                         // output sub-grid this launch covers (m -> n, a, b)
  int out_sy, out_oy, out_sx, out_ox;   // full-grid output pixel = (a*out_sy+out_oy, b*out_sx+out_ox)
  int in_sy, in_sx;                     // input step per sub-grid step
  int Krow;                             // floats per weight row (all taps)
  int ntaps;
  int tap_dy[9], tap_dx[9];             // input offset of tap t (padding folded in)
  int tap_koff[9];                      // float offset of tap t inside a weight row
  int tap_off[9];                       // byte offset of tap t relative to the window origin pixel
  int ty0, tny, tx0, tnx;               // the taps form a grid: tap (ry, rx) = (ty0 + ry, tx0 + rx), t = ry*tnx + rx
  FastDiv div_ohw, div_ow;              // m -> (n, a, b) without integer division
  FastDiv div_rl4;                      // ROWMODE: float4 index inside K -> (run, float4 inside the run)
  // -DTBN_DIAG=1 builds only (scripts/README.md, TBN_DIAG_FOLD): per-input-channel scale / shift applied with a ReLU when
  // the LDS-halo kernel stages its patch -- the COST side of folding the producer's BN apply into this conv's operand
  // staging (the engine passes ones / zeros: results unchanged); null = off, never read by the shipped build
  const float* fold_scale;
  const float* fold_shift;
};

// ---- riders: elementwise BN passes of INDEPENDENT layers executed by extra workgroups of a conv-GEMM launch.
// Inside an inception block (reference dataflow core/models/bn_inception_audio.py:437-1003, concat :485-493) the BN apply
// of the `1x1` column range does not feed the `3x3 | double_3x3_1` GEMMs, the BN apply of `3x3` / `pool_proj` does not
// feed `double_3x3_2`, and in backward the BN-backward apply of `1x1` / `3x3` / `pool_proj` does not feed the data gradient
// of `double_3x3_2`.  Cross-stream dependencies are the expensive primitive on this runtime (DESIGN.md finding 15), so the
// concurrency comes from ONE launch: the grid of the GEMM is extended by `span` workgroups that run the HBM-bound pass
// (same device code as the stand-alone bn_*_multi kernels: bit-identical results) beside the MFMA-bound tiles.
#define TBN_RIDER_MAXL 3
struct RiderLayer {
  const float* y;       // BN input rows (pitch y_ld)
  const float* dz;      // kind 2: gradient wrt z (pitch dz_ld)
  float* out;           // kind 1: z (pitch out_ld); kind 2: dy (pitch y_ld, in place over y)
  const float* scale;
  const float* shift;
  const float* coef;    // kind 2: [3][C]
  int y_ld, dz_ld, out_ld, P, C, rows;   // rows = pixel rows per rider workgroup
};
struct RiderP {
  int span;     // grid slots reserved for the rider (0: none)
  int first;    // first grid slot of the rider: 0 (front of the grid) or the GEMM's workgroup count (behind it)
  int gemm0;    // grid slot of GEMM workgroup 0 (front placement: span, a multiple of 8 -- keeps the XCD-aware tile maps)
  int nblk;     // rider workgroups that do work (<= span)
  int kind;     // 1: z = relu(y * scale + shift);  2: dy = a * [z > 0] dz + b * y + c
  int n;
  int blk0[TBN_RIDER_MAXL + 1];
  RiderLayer l[TBN_RIDER_MAXL];
};
// places a rider with `nblk` workgroups around a GEMM grid of `gemm_blocks`; returns the launch's grid size
int tbn_rider_place(RiderP* r, int gemm_blocks);

struct WgradP {
  const float* dy;
  const float* x;
  float* out;
  int dy_ld, x_ld;
  int N, H, W, OH, OW;
  int Cin, Cout;          // per tap (ROWMODE: taps = 1 and Cin = the whole packed K of a pixel = R runs of `rl` floats)
  int R, S, stride, pad;
  int taps;
  int M, K;
  int cp, rl;             // ROWMODE: floats per pixel of the padded input image / floats per contiguous run
  int tiles_co, tiles_ci;
  int rows_per_split;
  int mt, nt;             // host only: tile (32-column sub-tiles of Cout / Cin per workgroup), 0 = heuristic
  FastDiv div_ohw, div_ow, div_rl4;
  // incremental row addressing of the kernel (filled by tbn_launch_wgrad): a lane's row advances 64 output pixels per step
  unsigned mul_ow;        // ceil(2^32 / OW): oy = umulhi(pp, mul_ow) for the in-frame pixel index pp (pp * OW < 2^32); 0 when OW == 1
  unsigned r64;           // 64 % (OH*OW)
  unsigned frame_bytes;   // bytes of one input frame (H * W * pitch)
  unsigned fb_lo, fb_hi;  // frame-base advance per step: (64 / (OH*OW)) frames, one more when pp wraps
  unsigned row_step, col_step;   // ROWMODE: bytes per output row / column step in the padded image (stride folded in)
  double alg_flops;       // host only
  unsigned dy_bytes, x_bytes;   // exact extents (last row ends at its last column): lanes beyond them read zeros
  const float* fold_scale;      // -DTBN_DIAG=1 builds only: as ConvP::fold_scale, applied to the staged x operand
  const float* fold_shift;
  int ablate;             // timing ablations, honoured by -DTBN_ABLATE=1 builds only (scripts/wgrad_ablate.py)
};

// THE GEOMETRY OF THE STEM -- the 7x7 / stride 2 / pad 3 conv1 as the packed-row (ROWMODE) launches execute it, a function
// of the input alone.  Stated here only: the engine's plan (engine.hip build_graph, layout 0) and the stem entries of the
// C-ABI (api.hip tbn_stem_*) read it.  Two input-image layouts (pool.hip):
//   mode 0, space-to-depth: 4 rows / stride 1 of the zero-bordered 2x2 space-to-depth image [N][ceil(H/2)+3][ceil(W/2)+3]
//           [4*cin]; a filter row = kw = 4 pixels * cp contiguous floats, K = 4 * kw = 64 * cin;
//   mode 1, row runs: 7 rows / stride 2 of the zero-bordered NHWC image [N][2(OH-1)+8][2(OW-1)+8][cin]; a filter row = a run
//           of kw = 7 * cin floats rounded up to x4, K = 7 * kw rounded up to x32 (the padding meets zero weights).
// THE LAYOUT RULE (layout 0): row runs when they multiply fewer K columns (flow: 512 instead of 640; RGB / audio: the same
// 192 / 64 either way -- they keep the space-to-depth form and its 16-B aligned loads), i.e. from 4 input channels on.
enum { STEM_LAYOUT_RULE = 0, STEM_LAYOUT_S2D = 1, STEM_LAYOUT_ROWS = 2 };
struct StemGeom {
  int mode;                // 0 space-to-depth, 1 row runs
  int cp, kw;              // floats per pixel of the bordered image / per filter-row run
  int rows, stride, pad;   // the conv the GEMM kernels see: `rows` runs per output pixel, image steps per output step
  int H, W;                // bordered image
  int K;                   // multiplied K columns of the forward GEMM (a multiple of 32)
  int OH, OW;              // output map
};
static inline StemGeom stem_geom(int cin, int H, int W, int layout) {
  StemGeom g;
  g.OH = (H + 6 - 7) / 2 + 1;
  g.OW = (W + 6 - 7) / 2 + 1;
  g.pad = 0;
  const int rl = (7 * cin + 3) / 4 * 4, krows = (7 * rl + 31) / 32 * 32;
  if (layout == STEM_LAYOUT_ROWS || (layout == STEM_LAYOUT_RULE && krows < 64 * cin)) {
    g.mode = 1;
    g.cp = cin;
    g.kw = rl;
    g.rows = 7;
    g.stride = 2;
    g.H = 2 * (g.OH - 1) + 8;
    g.W = 2 * (g.OW - 1) + 8;
    g.K = krows;
  } else {
    g.mode = 0;
    g.cp = 4 * cin;
    g.kw = 4 * g.cp;
    g.rows = 4;
    g.stride = 1;
    g.H = (H + 1) / 2 + 3;
    g.W = (W + 1) / 2 + 3;
    g.K = g.rows * g.kw;
  }
  return g;
}

// optional in-process profiler: every conv-GEMM launch gets a pair of hipEvents on its stream.  The events ride ON the
// kernel's dispatch packet (hipExtLaunchKernelGGL: begin / end timestamps of the kernel itself, what rocprofv3's kernel
// trace reports); rounds 1-2 recorded two separate marker packets around the launch, whose processing sat inside the
// bracket (HIP-event averages 2.8 % above rocprofv3's for the same launches, round-2 verdict).
void tbn_prof_begin(const char* kernel, double flops, hipStream_t st, double alg_bytes = 0.0);
void tbn_prof_end(hipStream_t st);
void tbn_prof_label(const char* label);
bool tbn_prof_launch_events(hipEvent_t* start, hipEvent_t* stop);   // true: an open profiler record wants this launch timed
#define TBN_LAUNCH(kernel, grid, block, lds, st, ...)                                            \
  do {                                                                                           \
    hipEvent_t tbn_e0__, tbn_e1__;                                                               \
    if (tbn_prof_launch_events(&tbn_e0__, &tbn_e1__))                                            \
      hipExtLaunchKernelGGL(kernel, grid, block, lds, st, tbn_e0__, tbn_e1__, 0, __VA_ARGS__);  \
    else                                                                                         \
      TBN_KLAUNCH(kernel, grid, block, lds, st, __VA_ARGS__);                                    \
  } while (0)

// conv_igemm.hip
void tbn_conv_pick_tile(int M, int Cout, int K, int* mt, int* nt);
int tbn_launch_conv(ConvP p, int rowmode, int mt, int nt, hipStream_t st, const RiderP* rider = nullptr);
// two independent unit-stride convs in one launch (variant 0 LDS-halo, 1 / 2 generic with 1 / 2 LDS stages; tiles <= (2,2))
int tbn_launch_conv_pair(ConvP a, ConvP b, int variant, int mt, int nt, hipStream_t st, const RiderP* rider = nullptr);
int tbn_conv_red_rows(int N, int OH, int OW, int up, int ksize, int pad, int tile_rows);   // tile_rows = M rows per workgroup tile (128 * mt; 32 * mt for the split-K tile kernel)
size_t tbn_conv_halo_lds_bytes(const ConvP& p, int mt, int nt);   // 0: shape not handled by the LDS-halo kernel
// f(integral_constant<int, MT>, integral_constant<int, NT>) for the tile (mt, nt) of a kernel family that admits
// 1..MAXM x 1..MAXN; any other tile is refused (I walks the admitted tiles in row order)
template <int MAXM, int MAXN, int I = 0, class F>
static int with_tile(int mt, int nt, F&& f) {
  if constexpr (I == MAXM * MAXN) {
    tbn_set_error("conv: unsupported tile %dx%d", mt, nt);
    return TBN_ERR_UNSUPPORTED;
  } else {
    constexpr int MT = I / MAXN + 1, NT = I % MAXN + 1;
    if (mt == MT && nt == NT) return f(std::integral_constant<int, MT>{}, std::integral_constant<int, NT>{});
    return with_tile<MAXM, MAXN, I + 1>(mt, nt, f);
  }
}

// output tiles of a conv GEMM launch: `tile_rows` x mt rows (128; 32 for the split-K tile kernel) by 32 x nt columns
static inline void conv_set_tiles(ConvP& p, int tile_rows, int mt, int nt) {
  p.tiles_m = cdiv(p.M, tile_rows * mt);
  p.tiles_n = cdiv(p.Cout, 32 * nt);
}
// A kernel with dynamic LDS may use 64 KB of it until the limit of THAT instantiation is raised (to the CU's 160 KB).
// Raises it once, when a launch first needs more: `allowed` is a `static size_t allowed = TBN_DYN_LDS_DEFAULT` that the
// launcher keeps per instantiation; `who` prefixes the error message.
enum { TBN_DYN_LDS_DEFAULT = 64 * 1024, TBN_DYN_LDS_MAX = 160 * 1024 };
static inline int tbn_raise_dyn_lds(const void* kernel, size_t need, size_t& allowed, const char* who) {
  if (need <= allowed) return TBN_OK;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TBN_DYN_LDS_MAX) != hipSuccess) {
    tbn_set_error("%s: cannot raise the dynamic LDS limit", who);
    return TBN_ERR_LAUNCH;
  }
  allowed = TBN_DYN_LDS_MAX;
  return TBN_OK;
}

// conv_bf16x.hip: eval-forward convolutions on the bf16 MFMA (np = 6 | 3 plane products); tbn_launch_conv routes a launch
// whose flags carry CONV_FLAG_BF16X6 / _BF16X3 there and refuses what those kernels do not cover.
// THE SHAPE RULE -- which layer runs on which split-bf16 kernel, a function of the layer alone.  Everything that has to
// agree on it reads it here: the launcher's classifier (conv_bf16x.hip), the pre-check of tbn_launch_conv, the engine's
// routing and plane layout (engine.hip) and the one-tensor plane size / split of the C-ABI (api.hip).
enum Bf16xLayer { BF16X_LAYER_NONE = 0, BF16X_LAYER_3X3, BF16X_LAYER_PW };
// what every split-bf16 GEMM needs: unit stride and whole 32-channel K chunks (one plane record each)
static inline bool bf16x_gemm_ok(int stride, int cin) { return stride == 1 && cin % 32 == 0; }
static inline Bf16xLayer bf16x_layer_kind(int k, int stride, int pad, int cin) {
  if (!bf16x_gemm_ok(stride, cin)) return BF16X_LAYER_NONE;
  if (k == 3 && pad == 1) return BF16X_LAYER_3X3;
  if (k == 1 && pad == 0) return BF16X_LAYER_PW;   // on pre-split weight planes only (CONV_FLAG_BF16X_PLANES)
  return BF16X_LAYER_NONE;
}
// The 3x3 kernel stages the halo of its tile in a fixed number of register slots: the MAP it runs on is at most 64 wide
// (the pointwise kernel has no such limit).  Deliberately NOT part of the rule above: the weight-plane layout asks the rule
// alone, so it is a function of the graph and np, and ONE plane buffer serves every plan of a backbone (any frame count and
// input size).  The price: a 3x3 layer on a wider map stays on the fp32 kernel and its planes are written and never read.
static inline bool bf16x_3x3_map_ok(int W) { return W <= 64; }
int tbn_launch_conv_bf16x(ConvP& p, int rowmode, int mt, int nt, double alg_bytes, hipStream_t st, const RiderP* rider);
// weight planes (layout: include/tbn_hip.h): up to 64 weight tensors of one flat fp32 array split in ONE launch
struct SplitTab {
  int n;
  size_t w_off[64];    // float offset of the tensor inside the fp32 array
  size_t p_off[64];    // byte offset of its records inside the plane buffer
  size_t floats[64];   // cout * taps * cin (cin a multiple of 32)
  int blk0[65];        // first workgroup of each tensor (1024 floats per workgroup); blk0[n] = grid size
};
// appends a tensor to `tab` (tab.n = 0: an empty table); false: the table is full
static inline bool split_tab_push(SplitTab& tab, size_t w_off, size_t p_off, size_t floats) {
  if (tab.n >= 64) return false;
  if (tab.n == 0) tab.blk0[0] = 0;
  tab.w_off[tab.n] = w_off;
  tab.p_off[tab.n] = p_off;
  tab.floats[tab.n] = floats;
  tab.blk0[tab.n + 1] = tab.blk0[tab.n] + (int)((floats + 1023) / 1024);
  ++tab.n;
  return true;
}
size_t tbn_bf16x_planes_bytes(size_t floats, int np);
int tbn_launch_bf16x_split(const float* w, void* planes, const SplitTab& tab, int np, hipStream_t st);
void tbn_wgrad_plan(int M, int Cout, int Cin, int taps, int* mt, int* nt, int* splits, int* rows_per_split);
size_t tbn_wgrad_workspace_floats(int M, int Cout, int Cin, int taps);
bool tbn_wgrad_tile_ok(int mt, int nt);   // 0 x 0 (the heuristic) or a tile the kernel is instantiated for
// what tbn_launch_wgrad runs for a problem (p: geometry and the requested tile p.mt x p.nt; host only, no device call)
struct WgradLaunchPlan {
  int mt, nt;             // the tile run
  int mode;               // kernel MODE: 0 general, 1 packed-row stem, 2 pointwise
  int splits, rows_per_split;
  int tiles_co, tiles_ci;
  int reduce;             // slab lanes of splitk_reduce_kernel: 0 (no split-K), 4 or 16
  size_t ws_floats;       // split-K slabs this tile needs
};
WgradLaunchPlan tbn_wgrad_launch_plan(const WgradP& p, int rowmode);
int tbn_launch_wgrad(WgradP p, int rowmode, float* dw, float* workspace, hipStream_t st);
int tbn_launch_weight_flip_transpose(const float* w, float* wt, int Cout, int taps, int Cin, hipStream_t st);
// layer table of the one-launch flip/transpose of every data-gradient weight of a backbone (kernel argument)
struct FlipTab {
  int n;
  int w_off[64];     // float offset of the layer inside the flat weight array (same offset in the flipped copy)
  short cout[64], cin[64], taps[64];
  int blk0[65];      // first workgroup of each layer; blk0[n] = grid size
};
int tbn_launch_weight_flip_transpose_all(const float* w, float* wt, const FlipTab& tab, hipStream_t st);

// Rows per workgroup of the BN reduce passes (forward statistics, backward sums): about 512 workgroups, at least 64
// rows each, rounded up to the row-lane count 256 / (C / 4) so that every row lane walks the same number of rows.
// bn.hip, bn_multi.hip and whoever sizes a partial buffer (tbn_bn_stats_parts, tbn_bn_bwd_pooled_parts) use this one rule.
static inline int tbn_bn_reduce_chunk(int P, int C) {
  const int rp = 256 / (C / 4);
  int pch = cdiv(P, 512);
  if (pch < 64) pch = 64;
  return cdiv(pch, rp) * rp;
}
static inline int tbn_bn_reduce_parts(int P, int C) { return cdiv(P, tbn_bn_reduce_chunk(P, C)); }
// pitch and first column of every segment (Seg or CSeg) are multiples of 4: the kernels move float4
template <class S>
static inline bool tbn_segs_x4(const S* s, int n) {
  for (int i = 0; i < n; ++i)
    if (s[i].ld % 4 != 0 || s[i].col_begin % 4 != 0) return false;
  return true;
}

// bn.hip
int tbn_launch_bn_stats(const float* y, int ld, int P, int C, float* partial, int* nparts, hipStream_t st);
int tbn_bn_stats_parts(int P, int C);
int tbn_launch_bn_finalize(const float* partial, int nparts, int P, int C, const float* gamma, const float* beta,
                           const float* conv_bias, float* running_mean, float* running_var, float momentum, float eps,
                           float* save_mean, float* save_rstd, float* scale, float* shift, hipStream_t st);
int tbn_launch_bn_apply(const float* y, int P, int C, const float* scale, const float* shift, const Seg* segs,
                        int nseg, hipStream_t st);
int tbn_launch_bn_apply_maxpool(const float* y, int N, int H, int W, int C, const float* scale, const float* shift,
                                float* out, int out_ld, unsigned char* argmax, int OH, int OW, int stride, int pad,
                                hipStream_t st);
int tbn_launch_bn_bwd_reduce_pooled(const float* dpooled, int dpooled_ld, const unsigned char* argmax, int N, int H,
                                    int W, int OH, int OW, int stride, int pad, const float* y, int C,
                                    const float* scale, const float* shift, const float* mean, const float* rstd,
                                    float* partial, hipStream_t st);
int tbn_bn_bwd_pooled_parts(int N, int H, int W, int C, int stride, int pad);   // partial rows of the pooled reduce
int tbn_launch_bn_bwd_apply_pooled(const float* dpooled, int dpooled_ld, const unsigned char* argmax, int N, int H, int W,
                                   int OH, int OW, int stride, int pad, const float* y, int C, const float* scale,
                                   const float* shift, const float* coef, float* dy, hipStream_t st);
// batched training-BN launches over up to three independent layers (bn_multi.hip)
#define TBN_BN_MAXL 4
struct BnFwdLayer {
  const float* y;           // BN input (P, C) with pitch y_ld (a column range of a wider conv output)
  int y_ld;
  int P, C;
  const float* partial;     // statistics partials: partial[(i*2 + {0,1}) * pld + c], i < nparts
  int pld, nparts;
  const float *gamma, *beta, *conv_bias;
  float *running_mean, *running_var, *save_mean, *save_rstd, *scale, *shift;
  Seg seg[3];               // destination column ranges of z
  int nseg;
  int app_rows;             // filled by the launcher: rows per workgroup of the apply kernel
};
struct BnFwdBatch {
  int n;
  float momentum, eps;
  BnFwdLayer l[TBN_BN_MAXL];
  int fin_blk0[TBN_BN_MAXL + 1], app_blk0[TBN_BN_MAXL + 1];   // filled by the launcher
};
struct BnBwdLayer {
  CSeg dz[3];               // gradient wrt z, by column range
  int nseg;
  const float* y;           // BN input (pitch y_ld); dy is written in place
  float* dy;
  int y_ld;
  int P, C;
  const float *scale, *shift, *mean, *rstd;
  float* partial;           // [nparts][2][C]: scratch of the reduce kernel, or -- ext_parts > 0 -- already filled by the
  int ext_parts;            //   data-gradient epilogue that finished dz (conv RedSeg): no reduce pass for this layer
  float* coef;              // scratch [3][C]
  float *dgamma, *dbeta, *dbias;
  int pch, nparts;          // filled by the launcher
  int app_rows;             // filled by the launcher: rows per workgroup of the apply kernel
};
struct BnBwdBatch {
  int n;
  BnBwdLayer l[TBN_BN_MAXL];
  int red_blk0[TBN_BN_MAXL + 1], fin_blk0[TBN_BN_MAXL + 1], app_blk0[TBN_BN_MAXL + 1];   // filled by the launcher
};
int tbn_launch_bn_fwd_multi(BnFwdBatch& b, hipStream_t st);   // finalize + apply of every layer: 2 launches
int tbn_launch_bn_bwd_multi(BnBwdBatch& b, hipStream_t st);   // reduce + finalize + apply: 3 launches
// the same with some members' APPLY pass taken out (bit i of `defer_mask`): those are described in `*rider` instead (to be
// executed inside a later conv launch: tbn_launch_conv(..., rider)); every member is still reduced / finalized here
int tbn_launch_bn_fwd_multi_defer(BnFwdBatch& b, unsigned defer_mask, RiderP* rider, hipStream_t st);
int tbn_launch_bn_bwd_multi_defer(BnBwdBatch& b, unsigned defer_mask, RiderP* rider, hipStream_t st);
bool tbn_prof_enabled();   // the opt-in profiler brackets every conv launch: riders would be charged to their hosts
int tbn_launch_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, const float* bias,
                       float eps, float* scale, float* shift, int C, hipStream_t st);
int tbn_bn_bwd_parts(int P, int C);
int tbn_launch_bn_bwd_reduce(const CSeg* dz, int nseg, const float* y, int P, int C, const float* scale,
                             const float* shift, const float* mean, const float* rstd, float* partial, hipStream_t st);
int tbn_launch_bn_bwd_finalize(const float* partial, int nparts, int P, int C, const float* scale, const float* mean,
                               const float* rstd, float* coef, float* dgamma, float* dbeta, float* dbias,
                               hipStream_t st);
int tbn_launch_bn_bwd_apply(const CSeg* dz, int nseg, const float* y, int P, int C, const float* scale,
                            const float* shift, const float* coef, float* dy, hipStream_t st);

// pool.hip
int tbn_launch_maxpool_fwd(const float* in, int in_ld, float* out, int out_ld, uint8_t* argmax, int N, int H, int W,
                           int C, int OH, int OW, int stride, int pad, hipStream_t st);
int tbn_launch_maxpool_bwd(const float* dout, int dout_ld, const uint8_t* argmax, float* din, int din_ld, int N,
                           int H, int W, int C, int OH, int OW, int stride, int pad, int accumulate, hipStream_t st);
int tbn_launch_avgpool3_fwd(const float* in, int in_ld, float* out, int out_ld, int N, int H, int W, int C,
                            int accumulate, hipStream_t st);
int tbn_launch_spatial_mean_fwd(const float* in, int in_ld, float* out, int out_ld, int N, int H, int W, int C,
                                int freq_only, hipStream_t st);
int tbn_launch_spatial_mean_bwd(const float* dout, int dout_ld, float* din, int din_ld, int N, int H, int W, int C,
                                int freq_only, hipStream_t st);
int tbn_launch_nchw_to_s2d_pad(const float* in, float* out, int N, int C, int H, int W, hipStream_t st);
int tbn_launch_pack_stem_weight_s2d(const float* w, float* wp, int Cout, int C, hipStream_t st);
int tbn_launch_unpack_stem_wgrad_s2d(const float* dwp, float* dw, int Cout, int C, hipStream_t st);
// row-run stem (bordered NHWC image, pool.hip): image [N][HP][WP][C], run length RL = 7*C rounded up to x4, K padded to x32
int tbn_launch_nchw_to_nhwc_pad(const float* in, float* out, int N, int C, int H, int W, int HP, int WP, hipStream_t st);
int tbn_launch_pack_stem_weight_rows(const float* w, float* wp, int Cout, int C, int RL, int K, hipStream_t st);
int tbn_launch_unpack_stem_wgrad_rows(const float* dwp, float* dw, int Cout, int C, int RL, hipStream_t st);
