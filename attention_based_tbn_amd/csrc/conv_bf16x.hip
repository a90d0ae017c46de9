// Split-bf16 3x3 / stride 1 / pad 1 forward convolution for gfx950: the fp32 product on v_mfma_f32_32x32x16_bf16.
//
// Replaces, under model.eval() / torch.no_grad() (reference core/tools/test.py:67-87), what the reference gets from cuDNN
// through the 3x3 nn.Conv2d layers of core/models/bn_inception_audio.py:24-401 -- fp32 in, fp32 out, opt-in.
//
// An fp32 value is exactly hi + mid + lo with three bf16 planes (8 + 8 + 8 significand bits):
//   hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)      (round to nearest even; both subtractions are exact)
// and a bf16 x bf16 product is exact in the fp32 accumulator of the MFMA.  With the planes numbered 0 / 1 / 2:
//   bf16x6: the six plane products with i + j <= 2 -- a*b to about 2^-25 relative, below the fp32 accumulation's own rounding;
//   bf16x3: the three with i + j <= 1               -- at most 2^-17 + 2^-17 + 2^-18 < 1.25 * 2^-16 relative per product.
// One fp32 accumulator per output tile; inside a 16-channel K step the small products go first
// (lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi).
//
// Geometry is the LDS-halo kernel's (conv_igemm.hip: conv_halo_body): the flat NHWC pixel range of a 128*MT-row output
// tile widened by W + 1 pixels on both sides is staged ONCE per 32-channel chunk and read at nine row shifts; a lane whose
// shift leaves the image reads a row of zeros.  THE SPLIT HAPPENS WHILE STAGING: global fp32 -> registers -> planes ->
// LDS, for the input patch once per chunk and for the (32*NT) x 32 weight tile once per tap (double buffered), so the
// tap loop holds ds_read_b128 fragment reads and MFMAs plus the staging of the NEXT weight tile, and no HBM buffer is
// added.  bf16x6 stages three planes per operand (6 B per element), bf16x3 two (4 B).
// LDS image: one row per pixel / output channel = [plane 0: 32 bf16 | plane 1 | (plane 2) | 16 B pad], i.e. a pitch of
// 208 B (bf16x6) or 144 B (bf16x3) = 52 / 36 banks: the 16 lanes of a ds_read_b128 pass (consecutive rows, same column)
// start on 16 distinct multiples of 4 banks -- conflict free, like the fp32 tiles' 36-float pitch.
// Fragments (cdna_hip_programming.md section 3): lane l holds A[row l & 31][k = 8 (l >> 5) + j] and
// B[k = 8 (l >> 5) + j][col l & 31], j = 0..7: one 16-B read at byte (plane * 64 + kstep * 32 + (l >> 5) * 16) of the
// row.  C/D is laid out as the fp32 MFMA's, so the epilogue is the fp32 kernels' (tbn_conv_dev.h).
// Tiles: MT in {1, 2} x NT in {1..4} as the LDS-halo kernel; the largest, <2,4> bf16x6 at W = 64, needs 134 KB of LDS.
// Subnormals: the lo plane of an input below about 2^-110 is a bf16 subnormal and the guides do not say whether the
// bf16 MFMA flushes subnormal A/B inputs; the absolute error that could cause is < 2^-126 per product.  A value that
// rounds to a bf16 infinity (|x| > 3.39e38) gives NaN planes, where the fp32 kernel would return an infinity.
//
// PRE-SPLIT WEIGHT PLANES (CONV_FLAG_BF16X_PLANES, eval mode: the weights are constants).  bf16x_split_planes_kernel writes
// the planes of a whole [Cout][taps][Cin] weight tensor ONCE, as one record per (cout row, tap, 32-channel chunk) =
// [hi 32 | mid 32 | (lo 32)] bf16 -- the LDS row image above minus its pad, record index = (float index of the chunk) / 32.
// With PL = true the 3x3 kernel copies its B tile from those records with 16-B loads (same values in the same LDS image,
// same MFMA order: bit-identical results) and the tap loop loses the weight split's VALU work.
// conv_bf16x_pw_kernel is the pointwise (1x1 / stride 1 / pad 0) kernel on planes: a plain [M x Cin] . [Cin x Cout] GEMM over
// the NHWC rows, no map-width limit; the activation tile is still split while it is staged, now once per 32-channel chunk
// and N tile with no nine-tap reuse behind it, so wide N tiles are what amortises it.
//
// SHARED PIECES.  Device: bf16x_split_store (fp32 -> planes in LDS), BF16X_KSTEP (the fragment reads and plane products of
// one 32-channel chunk: THE product order), Bf16xPlaneTile (load / store of a weight tile's plane records), and from
// tbn_conv_dev.h xcd_tile / conv_epilogue.  The offsets of a staged tile and the accumulator clear stay written out in
// each kernel: as helper functions they changed the code the compiler emits (profiles/bf16x_refactor.md).
// Host: Bf16xKind names the three kernels, bf16x_kind classifies a launch on the shape rule of tbn_kernels.h
// (bf16x_layer_kind, bf16x_3x3_map_ok), bf16x_lds_bytes and bf16x_pick_tile take the kind, and launch_bf16x is the one
// function that selects and launches an instantiation.
#include <cstdio>
#include <cstring>

#include "tbn_common.h"
#include "tbn_kernels.h"
#include "tbn_conv_dev.h"

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// planes of four fp32 values -> 8 B each at dst + plane * 64
template <int P>
__device__ __forceinline__ void bf16x_split_store(char* dst, const float4 v4) {
  f32x4 r = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
  for (int pl = 0; pl < P; ++pl) {
    const bf16x4 b = __builtin_convertvector(r, bf16x4);   // round to nearest even (v_cvt_pk_bf16_f32)
    *reinterpret_cast<bf16x4*>(dst + pl * 64) = b;
    if (pl + 1 < P) r -= __builtin_convertvector(b, f32x4);   // exact
  }
}

// One 32-channel chunk of the (32 MT) x (32 NT) tile of a wave: two K steps of 16 channels, each the ds_read_b128
// fragment reads of every plane (A row i at A + a_off[i], B row j at B + b_off[j]) and then the plane products,
// small ones first, into the one accumulator per sub-tile.  The product order and the j-outer / i-inner nesting are
// stated HERE and nowhere else (tests/test_conv_bf16x_census_gpu.py pins the product set).
// A macro, expanded where NP, P, MT, NT and acc[MT][NT] are in scope (its own names end in an underscore): as a
// __forceinline__ function the same text made the compiler allocate more registers in four instantiations
// (profiles/bf16x_refactor.md); expanded in place every kernel is the machine code it was with the block written out.
#define BF16X_KSTEP(A, a_off, B, b_off)                                                                                              \
  _Pragma("unroll") for (int ks_ = 0; ks_ < 2; ++ks_) {                                                                              \
    bf16x8 fa_[MT][P], fb_[NT][P];                                                                                                   \
    _Pragma("unroll") for (int pl_ = 0; pl_ < P; ++pl_) {                                                                            \
      _Pragma("unroll") for (int i_ = 0; i_ < MT; ++i_)                                                                              \
        fa_[i_][pl_] = *reinterpret_cast<const bf16x8*>((A) + (a_off)[i_] + pl_ * 64 + ks_ * 32);                                    \
      _Pragma("unroll") for (int j_ = 0; j_ < NT; ++j_)                                                                              \
        fb_[j_][pl_] = *reinterpret_cast<const bf16x8*>((B) + (b_off)[j_] + pl_ * 64 + ks_ * 32);                                    \
    }                                                                                                                                \
    _Pragma("unroll") for (int j_ = 0; j_ < NT; ++j_) _Pragma("unroll") for (int i_ = 0; i_ < MT; ++i_) {                            \
      if (NP == 6) {                                                                                                                 \
        acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa_[i_][P - 1], fb_[j_][0], acc[i_][j_], 0, 0, 0); /* lo * hi */       \
        acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa_[i_][0], fb_[j_][P - 1], acc[i_][j_], 0, 0, 0); /* hi * lo */       \
        acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa_[i_][1], fb_[j_][1], acc[i_][j_], 0, 0, 0);     /* mid * mid */     \
      }                                                                                                                              \
      acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa_[i_][1], fb_[j_][0], acc[i_][j_], 0, 0, 0); /* mid * hi */            \
      acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa_[i_][0], fb_[j_][1], acc[i_][j_], 0, 0, 0); /* hi * mid */            \
      acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa_[i_][0], fb_[j_][0], acc[i_][j_], 0, 0, 0); /* hi * hi */             \
    }                                                                                                                                \
  }

// The (32 NT) x 32 weight tile of one K chunk, copied from its plane records by the 256 threads: 16-B piece q of the tile
// = piece q % (4 P) of row q / (4 P), to the same place of the LDS row; thread tid moves pieces tid, tid + 256, ...
// voff / loff (global byte offset of the piece inside its record row, LDS byte offset; 0xffffffff: no piece) are set up by
// the kernel, which knows the row pitch in records and the tile's first LDS row.
// (every array is indexed by unrolled loops only: registers, cdna_hip_programming.md pitfall 20)
template <int P, int NT>
struct Bf16xPlaneTile {
  static constexpr int NB = (NT * P + 1) / 2;
  float4 r[NB];
  unsigned voff[NB], loff[NB];
  __device__ __forceinline__ void load(const i32x4 rsrc, const unsigned koff) {   // koff: byte offset of the K chunk's record
#pragma unroll
    for (int i = 0; i < NB; ++i) r[i] = buf_load4(rsrc, voff[i], koff);
  }
  __device__ __forceinline__ void store(char* lds) const {
#pragma unroll
    for (int i = 0; i < NB; ++i)
      if (loff[i] != 0xffffffffu) *reinterpret_cast<float4*>(lds + loff[i]) = r[i];
  }
};

// NP = plane products (6 | 3); EPI 0 plain (+bias, optional ReLU / accumulate) | 2 eval-BN fold + ReLU
// PL: p.wt holds pre-split weight planes (records, see the head of the file) instead of fp32 weights
template <int NP, int MT, int NT, int EPI, bool PL = false>
__global__ __launch_bounds__(256) void conv_bf16x_kernel(ConvP p) {
  extern __shared__ __attribute__((aligned(16))) float dyn_lds[];
  constexpr int P = NP == 6 ? 3 : 2;
  constexpr int PITCH = P * 64 + 16;   // bytes per LDS row
  constexpr int BM = 128 * MT, BN = 32 * NT;
  constexpr int NJ = (BM + 2 * 64 + 2 + 31) / 32;   // float4 slots per thread for a halo of up to W = 64
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int tm, tn;
  xcd_tile(blockIdx.x, p.tiles_m, p.tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int W = p.W, HR = BM + 2 * W + 2;   // halo rows; row HR is the zero row
  char* As = reinterpret_cast<char*>(dyn_lds);
  char* Bs0 = As + (HR + 1) * PITCH;

  const i32x4 in_rsrc = make_rsrc(p.in, p.in_bytes);
  const i32x4 wt_rsrc = make_rsrc(p.wt, p.wt_bytes);
  const int c4 = tid & 7, r0 = tid >> 3;
  const int lrow = lane & 31, lhalf = lane >> 5;

  // per-lane LDS byte address of each tap's A fragment row (or the zero row)
  unsigned fa_off[9][MT];
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
      fa_off[t][i] = (unsigned)(row * PITCH + lhalf * 16);
    }
  }
  unsigned fb_off[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) fb_off[j] = (unsigned)((j * 32 + lrow) * PITCH + lhalf * 16);

  // halo slot j of this thread: row (tid >> 3) + 32 j, channels 4 c4 .. 4 c4 + 3 of the chunk
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
  auto store_halo = [&]() {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (r0 + 32 * j < HR) bf16x_split_store<P>(As + (r0 + 32 * j) * PITCH + c4 * 8, ha[j]);
  };
  // B tile of (tap t, channels c0 ..): NT float4 of fp32 weights per thread, split while they are stored, or (PL) the
  // tile's plane records
  Bf16xPlaneTile<P, NT> bp;
  float4 rb[NT];
  unsigned b_voff[NT], b_lds[NT];
  if (PL) {
#pragma unroll
    for (int i = 0; i < bp.NB; ++i) {
      const int q = tid + 256 * i, row = q / (4 * P), pc = q - row * (4 * P);
      const bool ok = q < BN * 4 * P;
      // rows >= Cout: beyond wt_bytes
      bp.voff[i] = ok ? (unsigned)(n0 + row) * (unsigned)(p.Krow >> 5) * (unsigned)(P * 64) + (unsigned)pc * 16u : TBN_OOB;
      bp.loff[i] = ok ? (unsigned)(row * PITCH + pc * 16) : 0xffffffffu;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      b_voff[i] = (unsigned)(n0 + r0 + 32 * i) * (unsigned)p.Krow * 4u + (unsigned)c4 * 16u;   // rows >= Cout: beyond wt_bytes
      b_lds[i] = (unsigned)((r0 + 32 * i) * PITCH + c4 * 8);
    }
  }
  auto load_b = [&](int t, int c0) {
    if (PL) {
      bp.load(wt_rsrc, (unsigned)((t * p.Cin + c0) >> 5) * (unsigned)(P * 64));
    } else {
#pragma unroll
      for (int i = 0; i < NT; ++i) rb[i] = buf_load4(wt_rsrc, b_voff[i], (unsigned)(t * p.Cin + c0) * 4u);
    }
  };
  auto store_b = [&](char* Bs) {
    if (PL) {
      bp.store(Bs);
    } else {
#pragma unroll
      for (int i = 0; i < NT; ++i) bf16x_split_store<P>(Bs + b_lds[i], rb[i]);
    }
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
  load_b(0, 0);
  if (tid < PITCH / 4) reinterpret_cast<float*>(As + HR * PITCH)[tid] = 0.f;
  store_halo();
  store_b(Bs0);
  __syncthreads();

  const int nchunks = p.Cin >> 5;
  int ks = 0;
  for (int c = 0; c < nchunks; ++c) {
    const bool next = c + 1 < nchunks;
    if (next) load_halo((c + 1) * 32);   // waits in registers until every wave is past this chunk's last tap
#pragma unroll
    for (int t = 0; t < 9; ++t, ++ks) {
      const bool more = next || t < 8;
      if (more) load_b(t < 8 ? t + 1 : 0, t < 8 ? c * 32 : (c + 1) * 32);
      const char* Bs = Bs0 + (ks & 1) * (BN * PITCH);
      BF16X_KSTEP(As, fa_off[t], Bs, fb_off)
      // the other stage was last read in the previous tap: every wave is past that tap's barrier
      if (more) store_b(Bs0 + ((ks + 1) & 1) * (BN * PITCH));
      __syncthreads();
    }
    if (next) {   // every wave is past its last read of this chunk's halo (barrier above)
      store_halo();
      __syncthreads();
    }
  }
  conv_epilogue<MT, NT, EPI, false>(p, acc, dyn_lds, tm, m0, n0);
}

// Pointwise (1x1 / stride 1 / pad 0) split-bf16 GEMM on pre-split weight planes: out[m][n] = sum_c in[m][c] * w[n][c] over
// the flat NHWC rows m.  Per 32-channel chunk the (128 MT) x 32 activation tile is loaded as fp32, split into planes and
// staged (four float4 per thread and M sub-tile), the (32 NT) x 32 weight tile is copied from its plane records; both are
// double buffered, one barrier per chunk.  Fragment layout, product order and epilogue are the 3x3 kernel's.
template <int NP, int MT, int NT, int EPI>
__global__ __launch_bounds__(256) void conv_bf16x_pw_kernel(ConvP p) {
  extern __shared__ __attribute__((aligned(16))) float dyn_lds[];
  constexpr int P = NP == 6 ? 3 : 2;
  constexpr int PITCH = P * 64 + 16;
  constexpr int BM = 128 * MT, BN = 32 * NT;
  constexpr int NA = 4 * MT;                 // float4 of the activation tile per thread
  constexpr int STAGE = (BM + BN) * PITCH;   // bytes of one LDS stage: A rows, then B rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int tm, tn;
  xcd_tile(blockIdx.x, p.tiles_m, p.tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  char* lds = reinterpret_cast<char*>(dyn_lds);

  const i32x4 in_rsrc = make_rsrc(p.in, p.in_bytes);
  const i32x4 wt_rsrc = make_rsrc(p.wt, p.wt_bytes);
  const int c4 = tid & 7, r0 = tid >> 3;
  const int lrow = lane & 31, lhalf = lane >> 5;

  unsigned fa_off[MT], fb_off[NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) fa_off[i] = (unsigned)((wave * 32 * MT + i * 32 + lrow) * PITCH + lhalf * 16);
#pragma unroll
  for (int j = 0; j < NT; ++j) fb_off[j] = (unsigned)((BM + j * 32 + lrow) * PITCH + lhalf * 16);

  float4 ra[NA];
  unsigned a_voff[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int m = m0 + r0 + 32 * j;   // rows >= M read zeros
    a_voff[j] = m < p.M ? (unsigned)m * (unsigned)p.in_ld * 4u + (unsigned)c4 * 16u : TBN_OOB;
  }
  const unsigned nchunks = (unsigned)p.Cin >> 5;
  Bf16xPlaneTile<P, NT> bp;
#pragma unroll
  for (int i = 0; i < bp.NB; ++i) {
    const int q = tid + 256 * i, row = q / (4 * P), pc = q - row * (4 * P);
    const bool ok = q < BN * 4 * P;
    bp.voff[i] = ok ? (unsigned)(n0 + row) * nchunks * (unsigned)(P * 64) + (unsigned)pc * 16u : TBN_OOB;
    bp.loff[i] = ok ? (unsigned)((BM + row) * PITCH + pc * 16) : 0xffffffffu;
  }
  auto load_ab = [&](int c) {
#pragma unroll
    for (int j = 0; j < NA; ++j) ra[j] = buf_load4(in_rsrc, a_voff[j], (unsigned)c * 128u);
    bp.load(wt_rsrc, (unsigned)c * (unsigned)(P * 64));
  };
  auto store_ab = [&](char* S) {
#pragma unroll
    for (int j = 0; j < NA; ++j) bf16x_split_store<P>(S + (r0 + 32 * j) * PITCH + c4 * 8, ra[j]);
    bp.store(S);
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  load_ab(0);
  store_ab(lds);
  __syncthreads();
  for (int c = 0; c < (int)nchunks; ++c) {
    const bool next = c + 1 < (int)nchunks;
    if (next) load_ab(c + 1);
    const char* S = lds + (c & 1) * STAGE;
    BF16X_KSTEP(S, fa_off, S, fb_off)
    // the other stage was last read in the previous chunk: every wave is past that chunk's barrier
    if (next) store_ab(lds + ((c + 1) & 1) * STAGE);
    __syncthreads();
  }
  conv_epilogue<MT, NT, EPI, false>(p, acc, dyn_lds, tm, m0, n0);
}

#undef BF16X_KSTEP

// Weight planes of up to 64 weight tensors in one launch: a workgroup splits 1024 consecutive floats (32 records) of one
// tensor; thread = one float4 = 8 B of each plane of its record.
template <int P>
__global__ __launch_bounds__(256) void bf16x_split_planes_kernel(const float* __restrict__ w, char* __restrict__ planes,
                                                                 SplitTab tab) {
  int l = 0;
  while (l + 1 < tab.n && (int)blockIdx.x >= tab.blk0[l + 1]) ++l;
  const size_t f = ((size_t)((int)blockIdx.x - tab.blk0[l]) * 256 + threadIdx.x) * 4;   // float index inside the tensor
  if (f >= tab.floats[l]) return;
  const float4 v = *reinterpret_cast<const float4*>(w + tab.w_off[l] + f);
  bf16x_split_store<P>(planes + tab.p_off[l] + (f >> 5) * (size_t)(P * 64) + ((f & 31) >> 2) * 8, v);
}

// ---------------------------------------------------------------------------------------------- host side
// the kernel a launch runs
enum Bf16xKind {
  BF16X_NONE = -1,
  BF16X_3X3 = 0,          // 3x3, weights split while staging
  BF16X_3X3_PLANES = 1,   // 3x3, weight tiles copied from pre-split planes
  BF16X_PW = 2            // pointwise, from pre-split planes (the only form it has)
};
// the shape rule (tbn_kernels.h) applied to a prepared single-GEMM launch: a same-size forward, not packed rows
static Bf16xKind bf16x_kind(const ConvP& p, int rowmode) {
  if (rowmode || p.R != p.S || p.up != 1 || p.OH != p.H || p.OW != p.W) return BF16X_NONE;
  const bool planes = (p.flags & CONV_FLAG_BF16X_PLANES) != 0;
  switch (bf16x_layer_kind(p.R, p.stride, p.pad, p.Cin)) {
    case BF16X_LAYER_3X3: return !bf16x_3x3_map_ok(p.W) ? BF16X_NONE : (planes ? BF16X_3X3_PLANES : BF16X_3X3);
    case BF16X_LAYER_PW: return planes ? BF16X_PW : BF16X_NONE;
    default: return BF16X_NONE;
  }
}

// dynamic LDS: 3x3 = halo rows + zero row of A, two stages of B rows; pointwise = two stages of A + B rows
static size_t bf16x_lds_bytes(Bf16xKind kind, int W, int np, int mt, int nt) {
  const size_t pitch = (np == 6 ? 3 : 2) * 64 + 16;
  return pitch * (kind == BF16X_PW ? 2 * (128 * mt + 32 * nt) : 128 * mt + 2 * W + 3 + 2 * 32 * nt);
}

// Tile heuristic: the cost model of tbn_conv_pick_tile with the MFMA cycles of these kernels -- per 32-channel K step
// and 32 x 32 sub-tile 2 * np instructions of 32 cycles (fp32 kernel: 16 of 64) -- so the fixed per-step cost weighs
// more and larger tiles win earlier.  The 350 / 4000 cycle constants are the fp32 kernel's; for these kernels the model is
// NOT measured (the <2,3> / <2,4> tiles it prefers for large M run at 256+ VGPRs, one wave per SIMD).
// Pointwise: plus the activation split.  A 1x1 has no nine-tap reuse of the split activation tile: every N tile of a row
// panel splits it again (per chunk and 128 rows: 4 float4 x (2 np / 3 + ...) VALU instructions per thread on the port the
// MFMA shares, priced at 150 cycles per M sub-tile), so the split is only amortised over the N tile -- the merged 1x1
// groups are 192 - 832 columns wide and the model therefore prefers WIDE NT (fewer N tiles = fewer splits of the same
// rows) over tall MT.
static void bf16x_pick_tile(Bf16xKind kind, int M, int Cout, int K, int np, int* mt_out, int* nt_out) {
  const bool pw = kind == BF16X_PW;
  double best = 1e300;
  int bm = 1, bn = 1;
  for (int mt = 1; mt <= 2; ++mt)
    for (int nt = 1; nt <= 4; ++nt) {
      const double blocks = (double)cdiv(M, 128 * mt) * cdiv(Cout, 32 * nt);
      const double rounds = (double)((long)((blocks + 255) / 256));
      const double per_block = (K / 32.0) * (mt * nt * 64.0 * np + (pw ? mt * 150.0 : 0.0) + 350.0) + 4000.0;
      double cost = rounds * per_block * (1.0 + 0.01 / (mt * nt));   // bigger tiles on ties (less L2 traffic)
      if (pw) cost *= 1.0 + 0.005 / nt;                              // ... then wider ones
      if (cost < best) {
        best = cost;
        bm = mt;
        bn = nt;
      }
    }
  *mt_out = bm;
  *nt_out = bn;
}

// selects the instantiation (np, epi, kind) of tile <MT, NT> and launches it
template <int MT, int NT>
static int launch_bf16x(const ConvP& p, int np, int epi, Bf16xKind kind, int grid, size_t lds_bytes, hipStream_t st) {
  auto go = [&](auto NPc, auto EPIc, auto KINDc) -> int {
    constexpr int NP = decltype(NPc)::value, EPI = decltype(EPIc)::value, KIND = decltype(KINDc)::value;
    static size_t allowed = TBN_DYN_LDS_DEFAULT;   // per instantiation
    const void* fn = KIND == BF16X_PW ? reinterpret_cast<const void*>(&conv_bf16x_pw_kernel<NP, MT, NT, EPI>)
                                      : reinterpret_cast<const void*>(&conv_bf16x_kernel<NP, MT, NT, EPI, KIND == BF16X_3X3_PLANES>);
    const int rc = tbn_raise_dyn_lds(fn, lds_bytes, allowed, "conv_bf16x");
    if (rc != TBN_OK) return rc;
    if (KIND == BF16X_PW)
      TBN_LAUNCH((conv_bf16x_pw_kernel<NP, MT, NT, EPI>), dim3(grid), dim3(256), lds_bytes, st, p);
    else
      TBN_LAUNCH((conv_bf16x_kernel<NP, MT, NT, EPI, KIND == BF16X_3X3_PLANES>), dim3(grid), dim3(256), lds_bytes, st, p);
    return TBN_OK;
  };
  using std::integral_constant;
  auto by_kind = [&](auto NPc, auto EPIc) -> int {
    if (kind == BF16X_PW) return go(NPc, EPIc, integral_constant<int, BF16X_PW>{});
    if (kind == BF16X_3X3_PLANES) return go(NPc, EPIc, integral_constant<int, BF16X_3X3_PLANES>{});
    return go(NPc, EPIc, integral_constant<int, BF16X_3X3>{});
  };
  if (np == 6)
    return epi == 2 ? by_kind(integral_constant<int, 6>{}, integral_constant<int, 2>{})
                    : by_kind(integral_constant<int, 6>{}, integral_constant<int, 0>{});
  return epi == 2 ? by_kind(integral_constant<int, 3>{}, integral_constant<int, 2>{})
                  : by_kind(integral_constant<int, 3>{}, integral_constant<int, 0>{});
}

size_t tbn_bf16x_planes_bytes(size_t floats, int np) { return floats * (np == 6 ? 6 : 4); }

int tbn_launch_bf16x_split(const float* w, void* planes, const SplitTab& tab, int np, hipStream_t st) {
  if (tab.n <= 0) return TBN_OK;
  if (np == 6)
    TBN_KLAUNCH((bf16x_split_planes_kernel<3>), dim3(tab.blk0[tab.n]), dim3(256), 0, st, w, (char*)planes, tab);
  else
    TBN_KLAUNCH((bf16x_split_planes_kernel<2>), dim3(tab.blk0[tab.n]), dim3(256), 0, st, w, (char*)planes, tab);
  TBN_CHECK_LAUNCH("bf16x_split_planes");
  return TBN_OK;
}

// `p` prepared by the caller (derived geometry filled, a single GEMM); mt, nt <= 0: heuristic tile
int tbn_launch_conv_bf16x(ConvP& p, int rowmode, int mt, int nt, double alg_bytes, hipStream_t st, const RiderP* rider) {
  const int both = CONV_FLAG_BF16X6 | CONV_FLAG_BF16X3;
  TBN_REQUIRE((p.flags & both) != both, "conv: bf16x6 and bf16x3 (flags 32 | 64) are exclusive");
  const int np = (p.flags & CONV_FLAG_BF16X6) ? 6 : 3;
  TBN_REQUIRE(!(p.flags & (CONV_FLAG_HALO | CONV_FLAG_DMA | CONV_FLAG_SK4)),
              "conv: the bf16x%d flag selects its own kernel: not with variant flags 4 / 8 / 16", np);
  TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, p.mode != CONV_EPI_STATS && p.nred == 0 && rider == nullptr,
                 "conv: the bf16x%d kernel has no training-statistics / reduce epilogue and hosts no rider (eval forward only)", np);
  const Bf16xKind kind = bf16x_kind(p, rowmode);
  // weights split while staging: the 3x3 kernel only; on pre-split planes (flag 128) also the pointwise kernel
  if (!(p.flags & CONV_FLAG_BF16X_PLANES))
    TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, kind != BF16X_NONE,
                   "conv: the bf16x%d kernel handles 3x3 / stride 1 / pad 1 layers on maps at most 64 wide (got %dx%d stride %d pad %d, width %d)",
                   np, p.R, p.S, p.stride, p.pad, p.W);
  else
    TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, kind != BF16X_NONE,
                   "conv: the bf16x%d kernels on weight planes (flag 128) handle 3x3 / stride 1 / pad 1 layers on maps at most 64 wide and 1x1 / stride 1 / pad 0 layers, cin a multiple of 32 (got %dx%d stride %d pad %d, width %d, cin %d)",
                   np, p.R, p.S, p.stride, p.pad, p.W, p.Cin);
  if (mt <= 0 || nt <= 0) bf16x_pick_tile(kind, p.M, p.Cout, p.K, np, &mt, &nt);
  TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, mt <= 2 && nt <= 4, "conv: unsupported bf16x%d tile %dx%d", np, mt, nt);
  const size_t lds_bytes = bf16x_lds_bytes(kind, p.W, np, mt, nt);
  if (kind != BF16X_3X3) {   // p.wt points at the plane records of this weight tensor: extent for the hardware range check
    const size_t pb = tbn_bf16x_planes_bytes((size_t)p.Cout * p.Krow, np);
    TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, pb < (1ull << 31), "conv: bf16x%d weight planes of %zu B >= 2 GiB", np, pb);
    p.wt_bytes = (unsigned)pb;
  }
  TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, lds_bytes <= 160 * 1024, "conv: bf16x%d tile %dx%d needs %zu B of LDS", np, mt, nt, lds_bytes);
  conv_set_tiles(p, 128, mt, nt);
  const int grid = p.tiles_m * p.tiles_n;
  const int epi = p.mode == CONV_EPI_EVAL ? 2 : 0;
  char nm[64];
  // conv_bf16x6_kernel: weights split while staging | conv_bf16x6_planes_kernel: 3x3 from planes | conv_bf16x6_pw_kernel: pointwise
  static const char* const kSuffix[3] = {"", "_planes", "_pw"};
  snprintf(nm, sizeof(nm), "conv_bf16x%d%s_kernel<%d, %d, %d>", np, kSuffix[kind], mt, nt, epi);
  tbn_prof_begin(nm, p.alg_flops, st, alg_bytes);
  const int rc = with_tile<2, 4>(mt, nt, [&](auto MT, auto NT) { return launch_bf16x<MT, NT>(p, np, epi, kind, grid, lds_bytes, st); });
  tbn_prof_end(st);
  if (rc != TBN_OK) return rc;
  TBN_CHECK_LAUNCH("conv_bf16x");
  return TBN_OK;
}
