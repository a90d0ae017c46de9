// Baseline JPEG decode into device frames: the step between the files on disk and the uint8 (n, H, W, C) frames that
// tbn_frames_to_tensor (frames.hip) reads.
//
// Reference (host, per frame): cv2.imread in core/dataset/dataset.py:303-305 (RGB, 3 channels B, G, R) and :355-370
// (Flow, cv2.imread(path, 0)), i.e. libjpeg-turbo at its defaults: ISLOW integer IDCT, "fancy" triangle upsampling,
// fixed-point YCbCr -> RGB.  All of it is integer arithmetic, restated here so that the frames are BYTE-IDENTICAL.
//
// Split: marker parsing and Huffman decoding are serial and stay on the host (tbn_jpeg_host.h, no HIP in it; run in
// worker threads).  Everything after the quantised coefficients runs here:
//   kernel A  dequantisation + 8x8 ISLOW IDCT  -> uint8 component planes (block-padded) in the workspace
//   kernel B  h2v1 / h2v2 fancy chroma upsampling + YCbCr -> BGR (or luma / gray copy) -> interleaved frames, cropped
// Arithmetic is 32-bit and wraps (unsigned adds / multiplies, arithmetic right shifts of the int reinterpretation):
// corrupt coefficients give garbage pixels, never undefined behaviour, and every address depends on the geometry only.
#include "tbn_common.h"
#include "tbn_jpeg_host.h"
#include "../../include/tbn_hip.h"

// ---------------------------------------------------------------- host entries (no HIP call in them) ------------------
extern "C" int tbn_jpeg_parse(const unsigned char* data, size_t size, tbn_jpeg_geometry* out) {
  char err[256];
  const int rc = tbn_jpeg_host_parse(data, size, out, err, sizeof(err));
  if (rc) tbn_set_error("%s", err);
  return rc;
}

extern "C" int tbn_jpeg_entropy_decode(const unsigned char* data, size_t size, const tbn_jpeg_geometry* expect,
                                       int16_t* coef, uint16_t* quant) {
  char err[256];
  const int rc = tbn_jpeg_host_entropy_decode(data, size, expect, coef, quant, err, sizeof(err));
  if (rc) tbn_set_error("%s", err);
  return rc;
}

// ---------------------------------------------------------------- device stage ----------------------------------------
struct JpegP {
  int n_img, W, H;
  int ncomp;                 // components reconstructed (1 when only luma is asked for)
  int file_comp;             // components in the file: strides of coef / quant
  int bw[3], bh[3];          // block extents of the planes
  uint32_t blk_off[4];       // first block of component c inside one image's reconstructed blocks; [ncomp] = their count
  uint32_t coef_off[3];      // first coefficient of component c inside one image
  uint32_t coef_per_img;
  uint32_t plane_off[3];     // first byte of component c inside one image's workspace
  uint32_t ws_per_img;
  int hs, vs;                // luma sampling factors (1 or 2)
  int out_c;
  int dword_ok;              // frames rows and quads are 4-byte aligned: packed dword stores
  FastDiv d_blocks, d_bw[3];
  FastDiv d_quads, d_h;
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t jmul(uint32_t a, int32_t k) { return a * (uint32_t)k; }
__device__ __forceinline__ uint32_t jdescale(uint32_t v, int s) { return (uint32_t)((int32_t)(v + (1u << (s - 1))) >> s); }

// jidctint.c's 1-D pass (CONST_BITS 13, PASS1_BITS 2) on eight values; out[i] = descale(., shift)
__device__ __forceinline__ void idct_1d(const uint32_t x[8], uint32_t out[8], int shift) {
  uint32_t z1 = jmul(x[2] + x[6], 4433);
  const uint32_t t2 = z1 - jmul(x[6], 15137), t3 = z1 + jmul(x[2], 6270);
  const uint32_t t0 = (x[0] + x[4]) << 13, t1 = (x[0] - x[4]) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  uint32_t a = x[7], b = x[5], c = x[3], d = x[1];
  z1 = a + d;
  uint32_t z2 = b + c, z3 = a + c, z4 = b + d;
  const uint32_t z5 = jmul(z3 + z4, 9633);
  a = jmul(a, 2446); b = jmul(b, 16819); c = jmul(c, 25172); d = jmul(d, 12299);
  z1 = jmul(z1, -7373); z2 = jmul(z2, -20995);
  z3 = jmul(z3, -16069) + z5; z4 = jmul(z4, -3196) + z5;
  a += z1 + z3; b += z2 + z4; c += z2 + z3; d += z1 + z4;
  out[0] = jdescale(t10 + d, shift); out[7] = jdescale(t10 - d, shift);
  out[1] = jdescale(t11 + c, shift); out[6] = jdescale(t11 - c, shift);
  out[2] = jdescale(t12 + b, shift); out[5] = jdescale(t12 - b, shift);
  out[3] = jdescale(t13 + a, shift); out[4] = jdescale(t13 - a, shift);
}

__device__ __forceinline__ uint32_t clamp255(int32_t v) { return (uint32_t)min(max(v, 0), 255); }

// Kernel A.  One 8x8 block per 8 lanes, 32 blocks per workgroup.  Lane j of a block loads coefficient ROW j (16 bytes,
// the block's 128 bytes are contiguous) and its quantiser row (16 bytes), dequantises, and hands the block through LDS
// to get COLUMN j for the first pass (libjpeg runs columns first; the rounding between the passes makes the order part
// of the result).  The column pass writes its outputs back transposed, each lane reads ROW j for the second pass and
// stores eight packed pixels (8 bytes) of the component plane.  LDS: 8 dwords per row so the 16-byte accesses stay
// aligned, 72 dwords per block: with the 4-byte accesses (32 banks, conflicts inside a 32-lane half = 4 blocks) block b
// starts on bank 8 b mod 32 and row r on 8 r, so lanes (b, j) hit bank 8 (b + r) + j: all 32 distinct.
constexpr int kJpegBlockLd = 72;
__global__ __launch_bounds__(256) void jpeg_idct_kernel(JpegP p, const int16_t* __restrict__ coef,
                                                        const uint16_t* __restrict__ quant,
                                                        unsigned char* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[32 * kJpegBlockLd];
  const int j = threadIdx.x & 7, lb = threadIdx.x >> 3;
  const uint32_t total = (uint32_t)p.n_img * p.blk_off[p.ncomp];
  const uint32_t gb = blockIdx.x * 32u + (uint32_t)lb;
  const bool live = gb < total;
  uint32_t* t = tile + lb * kJpegBlockLd;
  uint32_t img = 0, c = 0, brow = 0, bcol = 0;
  if (live) {
    img = fdiv(gb, p.d_blocks);
    uint32_t r = gb - img * p.d_blocks.d;
    c = (p.ncomp > 1 && r >= p.blk_off[1]) ? (r >= p.blk_off[2] ? 2u : 1u) : 0u;
    r -= p.blk_off[c];
    brow = fdiv(r, p.d_bw[c]);
    bcol = r - brow * p.d_bw[c].d;
    const size_t blk = (size_t)img * p.coef_per_img + p.coef_off[c] + ((size_t)brow * p.bw[c] + bcol) * 64;
    const u32x4 cv = *reinterpret_cast<const u32x4*>(coef + blk + j * 8);
    const u32x4 qv = *reinterpret_cast<const u32x4*>(quant + ((size_t)img * p.file_comp + c) * 64 + j * 8);
    u32x4 lo, hi;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t cw = cv[k], qw = qv[k];
      const uint32_t c0 = (uint32_t)(int32_t)(int16_t)(cw & 0xffffu), c1 = (uint32_t)((int32_t)cw >> 16);
      const uint32_t v0 = c0 * (qw & 0xffffu), v1 = c1 * (qw >> 16);
      if (k < 2) { lo[2 * k] = v0; lo[2 * k + 1] = v1; } else { hi[2 * k - 4] = v0; hi[2 * k - 3] = v1; }
    }
    *reinterpret_cast<u32x4*>(t + j * 8) = lo;
    *reinterpret_cast<u32x4*>(t + j * 8 + 4) = hi;
  }
  __syncthreads();
  uint32_t x[8], y[8];
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = t[r * 8 + j];
    idct_1d(x, y, 11);                       // CONST_BITS - PASS1_BITS
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) t[r * 8 + j] = y[r];
  }
  __syncthreads();
  if (live) {
    const u32x4 lo = *reinterpret_cast<const u32x4*>(t + j * 8), hi = *reinterpret_cast<const u32x4*>(t + j * 8 + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) { x[k] = lo[k]; x[k + 4] = hi[k]; }
    idct_1d(x, y, 18);                       // CONST_BITS + PASS1_BITS + 3
    uint32_t px[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) px[k] = clamp255((int32_t)(y[k] + 128u));   // y is a descaled int: |y| < 2^14 + wrap-free
    u32x2 o;
    o[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    o[1] = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
    const size_t pitch = (size_t)p.bw[c] * 8;
    unsigned char* dst = ws + (size_t)img * p.ws_per_img + p.plane_off[c] + ((size_t)brow * 8 + j) * pitch + (size_t)bcol * 8;
    *reinterpret_cast<u32x2*>(dst) = o;
  }
}

// fancy upsampling of one chroma sample (jdsample.c h2v1_fancy_upsample / h2v2_fancy_upsample) at output pixel (x, y).
// The neighbour index is clamped to the component's TRUE downsampled extent cw x ch: with p[-1] = p[0] and p[n] = p[n-1]
// the general formulas give exactly the special first / last columns ((4 p + 1) >> 2 = p, (4 s + 8) >> 4, (4 s + 7) >> 4),
// and the rows above the first / below the last are the first / last row, as libjpeg's context rows are.
template <int HS, int VS>
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ pl, int pitch, int cw, int ch, int x, int y) {
  if (HS == 1) return pl[(size_t)y * pitch + x];
  const int i = x >> 1, odd = x & 1;
  const int nb = min(max(i + (odd ? 1 : -1), 0), cw - 1);
  if (VS == 1) {
    const unsigned char* r = pl + (size_t)y * pitch;
    return (3 * r[i] + r[nb] + (odd ? 2 : 1)) >> 2;
  }
  const int rr = y >> 1;
  const int rn = min(max(rr + ((y & 1) ? 1 : -1), 0), ch - 1);
  const unsigned char* r0 = pl + (size_t)rr * pitch;
  const unsigned char* r1 = pl + (size_t)rn * pitch;
  const int s_i = 3 * r0[i] + r1[i], s_nb = 3 * r0[nb] + r1[nb];
  return (3 * s_i + s_nb + (odd ? 7 : 8)) >> 4;
}

// Kernel B.  One thread = four consecutive pixels of one output row (a "quad"): one dword of luma, the chroma taps by
// byte loads (neighbouring threads share them through the cache), and 4 x out_c packed bytes out -- three dwords (BGR) or
// one (gray) when the frame width is a multiple of 4, byte stores otherwise (frames are dense, so a row starts at
// y * W * out_c: only then is every quad aligned).
template <int HS, int VS>
__global__ __launch_bounds__(256) void jpeg_color_kernel(JpegP p, const unsigned char* __restrict__ ws,
                                                         unsigned char* __restrict__ frames) {
  const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
  const uint32_t quads = p.d_quads.d;
  if (gid >= (uint32_t)p.n_img * (uint32_t)p.H * quads) return;
  const uint32_t row = fdiv(gid, p.d_quads);
  const int x0 = (int)(gid - row * quads) * 4;
  const uint32_t img = fdiv(row, p.d_h);
  const int y = (int)(row - img * p.d_h.d);
  const unsigned char* base = ws + (size_t)img * p.ws_per_img;
  const int ypitch = p.bw[0] * 8;
  const uint32_t yw = *reinterpret_cast<const uint32_t*>(base + (size_t)y * ypitch + x0);   // pitch % 8 == 0, x0 % 4 == 0
  const bool color = p.ncomp == 3;
  const int cpitch = color ? p.bw[1] * 8 : 0;
  const int cw = (p.W + HS - 1) / HS, ch = (p.H + VS - 1) / VS;
  uint32_t px[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = (int)((yw >> (8 * k)) & 255u);
    const int x = min(x0 + k, p.W - 1);                 // lanes past the width recompute the last pixel, never stored
    if (p.out_c == 1) {
      px[k] = (uint32_t)yy;
    } else if (!color) {
      px[3 * k] = px[3 * k + 1] = px[3 * k + 2] = (uint32_t)yy;
    } else {
      const int cb = chroma_at<HS, VS>(base + p.plane_off[1], cpitch, cw, ch, x, y) - 128;
      const int cr = chroma_at<HS, VS>(base + p.plane_off[2], cpitch, cw, ch, x, y) - 128;
      px[3 * k + 0] = clamp255(yy + ((116130 * cb + 32768) >> 16));
      px[3 * k + 1] = clamp255(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      px[3 * k + 2] = clamp255(yy + ((91881 * cr + 32768) >> 16));
    }
  }
  unsigned char* dst = frames + (((size_t)img * p.H + y) * p.W + x0) * p.out_c;
  if (p.out_c == 1) {
#pragma unroll
    for (int k = 4; k < 12; ++k) px[k] = 0;
  }
  if (p.dword_ok) {
    uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int w = 0; w < 3; ++w)
      if (w < p.out_c) d4[w] = px[4 * w] | (px[4 * w + 1] << 8) | (px[4 * w + 2] << 16) | (px[4 * w + 3] << 24);
  } else {
    const int valid = min(4, p.W - x0) * p.out_c;
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < valid) dst[k] = (unsigned char)px[k];
  }
}

// shared argument check and launch parameters; `fn` names the entry in the messages
static int jpeg_params(const char* fn, const tbn_jpeg_geometry* g, int n_img, int out_channels, JpegP* p) {
  TBN_REQUIRE(g != nullptr, "%s: null geometry", fn);
  TBN_REQUIRE(n_img >= 0, "%s: n_img %d", fn, n_img);
  TBN_REQUIRE(out_channels == 1 || out_channels == 3, "%s: out_channels %d is not 1 or 3", fn, out_channels);
  TBN_REQUIRE(g->width > 0 && g->height > 0 && g->width <= 65535 && g->height <= 65535, "%s: bad image size %dx%d", fn,
              g->width, g->height);
  TBN_REQUIRE(g->components == 1 || g->components == 3, "%s: %d components (1 or 3)", fn, g->components);
  const int hs = g->hsamp[0], vs = g->vsamp[0];
  if (g->components == 1) {
    TBN_REQUIRE(hs == 1 && vs == 1, "%s: a 1-component image has sampling 1x1, got %dx%d", fn, hs, vs);
  } else {
    TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED,
                   ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)) && g->hsamp[1] == 1 &&
                       g->vsamp[1] == 1 && g->hsamp[2] == 1 && g->vsamp[2] == 1,
                   "%s: sampling %dx%d,%dx%d,%dx%d is not supported (4:4:4, 4:2:2 and 4:2:0 only)", fn, hs, vs, g->hsamp[1],
                   g->vsamp[1], g->hsamp[2], g->vsamp[2]);
  }
  // the block extents are a function of the size and the sampling: recomputed, not trusted
  const int mx = (g->width + 8 * hs - 1) / (8 * hs), my = (g->height + 8 * vs - 1) / (8 * vs);
  size_t coef = 0;
  for (int c = 0; c < g->components; ++c) {
    TBN_REQUIRE(g->blocks_w[c] == mx * g->hsamp[c] && g->blocks_h[c] == my * g->vsamp[c],
                "%s: block extents %dx%d of component %d do not belong to a %dx%d image", fn, g->blocks_w[c], g->blocks_h[c], c,
                g->width, g->height);
    coef += (size_t)64 * g->blocks_w[c] * g->blocks_h[c];
  }
  TBN_REQUIRE(coef == g->coef_count, "%s: coef_count %zu does not belong to this geometry (%zu)", fn, g->coef_count, coef);
  memset(p, 0, sizeof(*p));
  p->n_img = n_img; p->W = g->width; p->H = g->height;
  p->file_comp = g->components;
  p->ncomp = (out_channels == 1) ? 1 : g->components;     // gray output: chroma is not reconstructed at all
  p->hs = hs; p->vs = vs; p->out_c = out_channels;
  uint32_t boff = 0, coff = 0, woff = 0;
  for (int c = 0; c < g->components; ++c) {
    const uint32_t nb = (uint32_t)g->blocks_w[c] * (uint32_t)g->blocks_h[c];    // <= 8192^2 / 64 * 4
    p->bw[c] = g->blocks_w[c]; p->bh[c] = g->blocks_h[c];
    p->coef_off[c] = coff;
    coff += nb * 64;
    if (c < p->ncomp) {
      p->blk_off[c] = boff;
      p->plane_off[c] = woff;
      boff += nb;
      woff += nb * 64;
      p->d_bw[c] = make_fastdiv((uint32_t)g->blocks_w[c]);
    }
  }
  for (int c = p->ncomp; c < 4; ++c) p->blk_off[c] = boff;
  for (int c = p->ncomp; c < 3; ++c) p->d_bw[c] = make_fastdiv(1);
  p->coef_per_img = coff;
  p->ws_per_img = woff;
  const unsigned long long blocks = (unsigned long long)boff * (unsigned long long)n_img;
  const unsigned long long quads = (unsigned long long)n_img * g->height * ((g->width + 3) / 4);
  TBN_REQUIRE(coff < (1u << 31) && blocks < (1ull << 31) && quads < (1ull << 31), "%s: %d images of %dx%d are too many for one launch",
              fn, n_img, g->width, g->height);
  p->d_blocks = make_fastdiv(boff);
  p->d_quads = make_fastdiv((uint32_t)((g->width + 3) / 4));
  p->d_h = make_fastdiv((uint32_t)g->height);
  return TBN_OK;
}

extern "C" size_t tbn_jpeg_workspace_bytes(const tbn_jpeg_geometry* geometry, int n_img) {
  JpegP p;
  if (jpeg_params("jpeg_workspace_bytes", geometry, n_img, 3, &p) != TBN_OK) return 0;
  return (size_t)p.ws_per_img * (size_t)n_img;
}

extern "C" int tbn_jpeg_reconstruct(const int16_t* coef_dev, const uint16_t* quant_dev, int n_img,
                                    const tbn_jpeg_geometry* geometry, int out_channels, unsigned char* frames_dev,
                                    void* workspace, void* stream) {
  const char* fn = "jpeg_reconstruct";
  JpegP p;
  const int rc = jpeg_params(fn, geometry, n_img, out_channels, &p);
  if (rc != TBN_OK) return rc;
  if (n_img == 0) return TBN_OK;
  TBN_REQUIRE(coef_dev != nullptr && quant_dev != nullptr && frames_dev != nullptr && workspace != nullptr, "%s: null argument", fn);
  TBN_REQUIRE(((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)quant_dev & 15) == 0 && ((uintptr_t)workspace & 15) == 0,
              "%s: coef, quant and workspace must be 16-byte aligned", fn);
  p.dword_ok = (p.W % 4 == 0 && ((uintptr_t)frames_dev & 3) == 0) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t blocks = (uint32_t)n_img * p.blk_off[p.ncomp];
  TBN_KLAUNCH(jpeg_idct_kernel, dim3((blocks + 31) / 32), dim3(256), 0, st, p, coef_dev, quant_dev, (unsigned char*)workspace);
  TBN_CHECK_LAUNCH(fn);
  const uint32_t quads = (uint32_t)n_img * (uint32_t)p.H * p.d_quads.d;
  const dim3 grid((quads + 255) / 256), block(256);
  const unsigned char* ws = (const unsigned char*)workspace;
  if (p.ncomp == 1 || (p.hs == 1 && p.vs == 1)) {
    TBN_KLAUNCH((jpeg_color_kernel<1, 1>), grid, block, 0, st, p, ws, frames_dev);
  } else if (p.vs == 1) {
    TBN_KLAUNCH((jpeg_color_kernel<2, 1>), grid, block, 0, st, p, ws, frames_dev);
  } else {
    TBN_KLAUNCH((jpeg_color_kernel<2, 2>), grid, block, 0, st, p, ws, frames_dev);
  }
  TBN_CHECK_LAUNCH(fn);
  return TBN_OK;
}
