// Device code of the 3x3 pools, shared by pool.hip and the pool-fused BN kernels of bn.hip, each rule stated once:
//   tbn_xcd_block_id   XCD-contiguous workgroup order of the stencil kernels
//   TBN_MAX3X3         first-maximum scan of a 3x3 window with the packed arg-max word
//   TBN_POOL_GATHER_*  a max pool's input gradient gathered from the arg-max words (_S2: branch-free 3x3 / 2 / 0, _LOOPS)
//   pooled_grad_2x2    the same gather for a whole 2x2 input block of a 3x3 / 2 / 0 pool; TBN_BLK_DECODE finds the block
//   TBN_ST4_ACC        store with optional accumulate
#pragma once
#include "tbn_common.h"

// Stencil kernels re-read their neighbours' rows: workgroups b, b+8, ... share an XCD (and its L2), so the
// bijective remap hands every XCD a CONTIGUOUS run of workgroup ids -- a row is then fetched into one L2, not
// into all eight (measured: 3x the algorithmic HBM reads without it).
__device__ __forceinline__ unsigned tbn_xcd_block_id() {
  const unsigned nb = gridDim.x, bid = blockIdx.x;
  const unsigned q8 = nb >> 3, r8 = nb & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
}

// Declares float4 best = the maximum of the quad Z over the in-bounds taps of the 3x3 window at (y0, x0) of image n, for
// the channel quad at c (rows of pitch ld), and int bx, by, bz, bw (b = the prefix) = its four window indices, which
// tbn_argmax_word packs at the store.  Z names the quad compared: the loaded quad `v` itself, or one that the statements
// ZD derive from it.  The FIRST maximum in scan order, a NaN propagates (ATen's comparison); a lane where nothing compares
// greater than -inf keeps k0.  A macro of this shape because as a function template, with Z bound to a reference or a
// copy, or with the word packed at once, it moved both kernels that use it (profiles/bn_pool_refactor.md)
#define TBN_MAX3X3(best, b, in, ld, n, H, W, y0, x0, c, k0, Z, ZD)                                               \
  float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);                                       \
  const int k0__ = (k0);                                                                                       \
  int b##x = k0__, b##y = k0__, b##z = k0__, b##w = k0__;                                                      \
_Pragma("unroll")                                                                                              \
  for (int r = 0; r < 3; ++r)                                                                                  \
_Pragma("unroll")                                                                                              \
    for (int s = 0; s < 3; ++s) {                                                                              \
      const int iy = (y0) + r, ix = (x0) + s;                                                                  \
      if ((unsigned)iy < (unsigned)(H) && (unsigned)ix < (unsigned)(W)) {                                      \
        const float4 v = *reinterpret_cast<const float4*>((in) + ((size_t)((n) * (H) + iy) * (W) + ix) * (ld) + (c)); \
        ZD                                                                                                     \
        const int k = r * 3 + s;                                                                               \
        if (Z.x > best.x || Z.x != Z.x) { best.x = Z.x; b##x = k; }                                            \
        if (Z.y > best.y || Z.y != Z.y) { best.y = Z.y; b##y = k; }                                            \
        if (Z.z > best.z || Z.z != Z.z) { best.z = Z.z; b##z = k; }                                            \
        if (Z.w > best.w || Z.w != Z.w) { best.w = Z.w; b##w = k; }                                            \
      }                                                                                                        \
    }
// the arg-max word of a channel quad: one window index (0..8) per byte
__device__ __forceinline__ uint32_t tbn_argmax_word(int bx, int by, int bz, int bw) {
  return (uint32_t)bx | ((uint32_t)by << 8) | ((uint32_t)bz << 16) | ((uint32_t)bw << 24);
}

// Gradient of a 3x3 max pool's input pixel (n, iy, ix), channel quad at c, ADDED to the float4 acc: the sum of dout over
// the windows whose arg-max the pixel is (a deterministic gather, no float atomics).  3x3 / 2 / 0: an input pixel lies in
// window o = i >> 1 (tap i & 1) and, for even i, also in window o - 1 (tap 2); all four candidates are evaluated
// branch-free with their loads issued together (the looped form is latency-bound: 1.3 TB/s on the 308 MB stem tensors),
// invalid candidates read a clamped, in-range address and are masked; same summation order as the loops: (hi,hi) (hi,lo)
// (lo,hi) (lo,lo).  Otherwise the loops over the windows oy with oy*stride - pad <= iy <= oy*stride - pad + 2.
// Macros, one per arm: as a function (three forms) the gather moved maxpool_bwd_kernel, and as one macro the kernels of
// bn.hip, which leave the first arm with a return (profiles/bn_pool_refactor.md).  3x3 / 2 / 0:
#define TBN_POOL_GATHER_S2(acc, dout, dout_ld, argmax, C, OH, OW, n, iy, ix, c)                          \
  const int oyA = iy >> 1, ryA = iy & 1, oxA = ix >> 1, rxA = ix & 1;                                    \
  const bool vy[2] = {oyA < OH, (ryA == 0) && (oyA >= 1)}, vx[2] = {oxA < OW, (rxA == 0) && (oxA >= 1)}; \
  const int oy[2] = {vy[0] ? oyA : 0, vy[1] ? oyA - 1 : 0}, ry[2] = {ryA, 2};                            \
  const int ox[2] = {vx[0] ? oxA : 0, vx[1] ? oxA - 1 : 0}, rx[2] = {rxA, 2};                            \
  uint32_t am[4];                                                                                        \
  float4 d[4];                                                                                           \
_Pragma("unroll")                                                                                        \
  for (int a = 0; a < 2; ++a)                                                                            \
_Pragma("unroll")                                                                                        \
    for (int b = 0; b < 2; ++b) {                                                                        \
      const size_t opix = (size_t)(n * OH + oy[a]) * OW + ox[b];                                         \
      am[a * 2 + b] = *reinterpret_cast<const uint32_t*>(argmax + opix * C + c);                         \
      d[a * 2 + b] = *reinterpret_cast<const float4*>(dout + opix * dout_ld + c);                        \
    }                                                                                                    \
_Pragma("unroll")                                                                                        \
  for (int a = 0; a < 2; ++a)                                                                            \
_Pragma("unroll")                                                                                        \
    for (int b = 0; b < 2; ++b) {                                                                        \
      const uint32_t k = (uint32_t)(ry[a] * 3 + rx[b]), m = am[a * 2 + b];                               \
      const bool v = vy[a] && vx[b];                                                                     \
      if (v && (m & 0xff) == k) acc.x += d[a * 2 + b].x;                                                 \
      if (v && ((m >> 8) & 0xff) == k) acc.y += d[a * 2 + b].y;                                          \
      if (v && ((m >> 16) & 0xff) == k) acc.z += d[a * 2 + b].z;                                         \
      if (v && (m >> 24) == k) acc.w += d[a * 2 + b].w;                                                  \
    }
// every other 3x3 geometry
#define TBN_POOL_GATHER_LOOPS(acc, dout, dout_ld, argmax, C, OH, OW, stride, pad, n, iy, ix, c) \
  const int oy_hi = min(OH - 1, (iy + pad) / stride);                                           \
  const int ox_hi = min(OW - 1, (ix + pad) / stride);                                           \
  for (int oy = oy_hi; oy >= 0; --oy) {                                                         \
    const int r = iy - (oy * stride - pad);                                                     \
    if (r > 2) break;                                                                           \
    for (int ox = ox_hi; ox >= 0; --ox) {                                                       \
      const int s = ix - (ox * stride - pad);                                                   \
      if (s > 2) break;                                                                         \
      const uint32_t k = (uint32_t)(r * 3 + s);                                                 \
      const size_t opix = (size_t)(n * OH + oy) * OW + ox;                                      \
      const uint32_t am = *reinterpret_cast<const uint32_t*>(argmax + opix * C + c);            \
      const float4 d = *reinterpret_cast<const float4*>(dout + opix * dout_ld + c);             \
      if ((am & 0xff) == k) acc.x += d.x;                                                       \
      if (((am >> 8) & 0xff) == k) acc.y += d.y;                                                \
      if (((am >> 16) & 0xff) == k) acc.z += d.z;                                               \
      if ((am >> 24) == k) acc.w += d.w;                                                        \
    }                                                                                           \
  }

// *p = v, or *p += v when `accumulate`.  A macro: as a function it moved avgpool3_kernel (profiles/bn_pool_refactor.md)
#define TBN_ST4_ACC(p, v, accumulate)                                          \
  do {                                                                         \
    float4* o__ = reinterpret_cast<float4*>(p);                                \
    float4 acc__ = (v);                                                        \
    if (accumulate) {                                                          \
      const float4 prev = *o__;                                                \
      acc__.x += prev.x; acc__.y += prev.y; acc__.z += prev.z; acc__.w += prev.w; \
    }                                                                          \
    *o__ = acc__;                                                              \
  } while (0)

// 2x2-input-block form of the 3x3 / stride 2 / pad 0 gather: the four pixels of a block share the same four windows
struct PoolBlk {
  const float* dout;
  const unsigned char* argmax;
  int dout_ld, H, W, OH, OW, C, BH, BW;
  FastDiv div_bw, div_bh;
};
static inline PoolBlk make_poolblk(const float* dout, int dout_ld, const unsigned char* argmax, int H, int W, int OH, int OW, int C) {
  PoolBlk q;
  q.dout = dout; q.argmax = argmax; q.dout_ld = dout_ld;
  q.H = H; q.W = W; q.OH = OH; q.OW = OW; q.C = C;
  q.BH = (H + 1) / 2; q.BW = (W + 1) / 2;
  q.div_bw = make_fastdiv((uint32_t)q.BW);
  q.div_bh = make_fastdiv((uint32_t)q.BH);
  return q;
}
// declares image n, block row by and block column bx of block index q (< N * BH * BW).  A macro: as a function it moved
// bn_bwd_reduce_pooled2x2_kernel (profiles/bn_pool_refactor.md)
#define TBN_BLK_DECODE(pb, q, n, by, bx)                                         \
  const uint32_t row__ = fdiv((uint32_t)(q), (pb).div_bw); /* n*BH + by */       \
  const int bx = (int)(q) - (int)row__ * (pb).BW;                                \
  const uint32_t n##__ = fdiv(row__, (pb).div_bh);                               \
  const int by = (int)row__ - (int)n##__ * (pb).BH, n = (int)n##__
// g[0] = d z(2by, 2bx), g[1] = d z(2by, 2bx+1), g[2] = d z(2by+1, 2bx), g[3] = d z(2by+1, 2bx+1)
__device__ __forceinline__ void pooled_grad_2x2(const PoolBlk& q, int n, int by, int bx, int c, float4 (&g)[4]) {
  const bool vy[2] = {by < q.OH, by >= 1 && by - 1 < q.OH}, vx[2] = {bx < q.OW, bx >= 1 && bx - 1 < q.OW};
  const int oy[2] = {vy[0] ? by : 0, vy[1] ? by - 1 : 0}, ox[2] = {vx[0] ? bx : 0, vx[1] ? bx - 1 : 0};
  uint32_t am[4];
  float4 d[4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const size_t opix = (size_t)(n * q.OH + oy[a]) * q.OW + ox[b];
      am[a * 2 + b] = *reinterpret_cast<const uint32_t*>(q.argmax + opix * q.C + c);
      d[a * 2 + b] = *reinterpret_cast<const float4*>(q.dout + opix * q.dout_ld + c);
      if (!(vy[a] && vx[b])) am[a * 2 + b] = 0xffffffffu;   // matches no tap
    }
  auto take = [&](float4& acc, int w, uint32_t k) {
    const uint32_t m = am[w];
    if ((m & 0xff) == k) acc.x += d[w].x;
    if (((m >> 8) & 0xff) == k) acc.y += d[w].y;
    if (((m >> 16) & 0xff) == k) acc.z += d[w].z;
    if ((m >> 24) == k) acc.w += d[w].w;
  };
#pragma unroll
  for (int i = 0; i < 4; ++i) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  // window index w = a*2 + b: a = 0 window row by, 1 row by-1; b = 0 window column bx, 1 column bx-1
  take(g[0], 0, 0); take(g[0], 1, 2); take(g[0], 2, 6); take(g[0], 3, 8);   // even-even pixel: taps (0,0) (0,2) (2,0) (2,2)
  take(g[1], 0, 1); take(g[1], 2, 7);                                       // even row, odd column: (0,1) (2,1)
  take(g[2], 0, 3); take(g[2], 1, 5);                                       // odd row, even column: (1,0) (1,2)
  take(g[3], 0, 4);                                                         // odd-odd: (1,1)
}
