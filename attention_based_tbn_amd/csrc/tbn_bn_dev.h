// The formulas of the training-BN passes (bn.hip, bn_multi.hip, bn_res.hip, tbn_rider_dev.h), each stated once.
//
// Per float4 channel quad (a lane owns four fixed channels):
//   tbn_bn_relu4      z  = relu(y * scale + shift)                                   forward apply
//   tbn_bn_gate4      g  = y * scale + shift > 0 ? dz : 0                            the ReLU mask, recomputed from y
//   tbn_pos_gate4     g  = z > 0 ? dz : 0                                            the mask from a stored output (bn_res.hip)
//   tbn_bn_sums4      S1 += g,  S2 += g * xhat  with  xhat = (y - mean) * rstd       backward reduce
//   tbn_bn_dy4        dy = a * g + b * y + c                                         backward apply (coef rows a | b | c)
//   tbn_bn_gated_dy4  dy with the gate formed element by element                     where g is not needed on its own
// The first, second and fifth are written once per element (tbn_bn_relu1, tbn_bn_gate1, tbn_bn_dy1).
// Per reduce workgroup: every row lane stores its S1 / S2 quads to red[2 * 2048] (tbn_bn_red_put) and, after a barrier,
// TBN_BN_RED_FOLD adds the row lanes of each channel in lane order and writes ONE partial row pair -- a fixed order, so
// the partials do not depend on scheduling.
// Per channel, once the partials are summed in fp64 (tbn_sum_partials):
//   TBN_BN_FWD_FINALIZE   mean = S1 / P, var = max(S2 / P - mean^2, 0), rstd = 1 / sqrt(var + eps), scale = gamma * rstd,
//                         shift = beta - mean * scale; running statistics with the unbiased variance, and the conv bias
//                         added to the running mean (the statistics are those of the bias-free conv output)
//   TBN_BN_BWD_FINALIZE   a = scale, b = -scale * rstd * S2 / P, c = -scale * S1 / P - b * mean; dgamma = S2, dbeta = S1
// TBN_SEG_OF finds which of up to three destination / source column ranges a channel quad belongs to.
#pragma once
#include "tbn_common.h"

// the three per-element formulas; the quad forms below apply them to x, y, z, w in that order
__device__ __forceinline__ float tbn_bn_relu1(float y, float sc, float sh) { return fmaxf(fmaf(y, sc, sh), 0.f); }
__device__ __forceinline__ float tbn_bn_gate1(float y, float sc, float sh, float d) { return fmaf(y, sc, sh) > 0.f ? d : 0.f; }
__device__ __forceinline__ float tbn_bn_dy1(float a, float b, float c, float g, float y) { return fmaf(a, g, fmaf(b, y, c)); }

// (float4 arguments by reference: by value, the copies changed the code of bn_bwd_reduce_kernel<true>)
__device__ __forceinline__ float4 tbn_bn_relu4(const float4& v, const float4& sc, const float4& sh) {
  float4 z;
  z.x = tbn_bn_relu1(v.x, sc.x, sh.x);
  z.y = tbn_bn_relu1(v.y, sc.y, sh.y);
  z.z = tbn_bn_relu1(v.z, sc.z, sh.z);
  z.w = tbn_bn_relu1(v.w, sc.w, sh.w);
  return z;
}
__device__ __forceinline__ float4 tbn_bn_gate4(const float4& v, const float4& sc, const float4& sh, const float4& d) {
  float4 g;
  g.x = tbn_bn_gate1(v.x, sc.x, sh.x, d.x);
  g.y = tbn_bn_gate1(v.y, sc.y, sh.y, d.y);
  g.z = tbn_bn_gate1(v.z, sc.z, sh.z, d.z);
  g.w = tbn_bn_gate1(v.w, sc.w, sh.w, d.w);
  return g;
}
__device__ __forceinline__ float4 tbn_pos_gate4(const float4& z, const float4& d) {
  return make_float4(z.x > 0.f ? d.x : 0.f, z.y > 0.f ? d.y : 0.f, z.z > 0.f ? d.z : 0.f, z.w > 0.f ? d.w : 0.f);
}
__device__ __forceinline__ void tbn_bn_sums4(float4& s1, float4& s2, const float4& g, const float4& v, const float4& mu,
                                             const float4& rs4) {
  s1.x += g.x; s1.y += g.y; s1.z += g.z; s1.w += g.w;
  s2.x = fmaf(g.x, (v.x - mu.x) * rs4.x, s2.x);
  s2.y = fmaf(g.y, (v.y - mu.y) * rs4.y, s2.y);
  s2.z = fmaf(g.z, (v.z - mu.z) * rs4.z, s2.z);
  s2.w = fmaf(g.w, (v.w - mu.w) * rs4.w, s2.w);
}
__device__ __forceinline__ float4 tbn_bn_dy4(const float4& ca, const float4& cb, const float4& cc, const float4& g,
                                             const float4& v) {
  float4 o;
  o.x = tbn_bn_dy1(ca.x, cb.x, cc.x, g.x, v.x);
  o.y = tbn_bn_dy1(ca.y, cb.y, cc.y, g.y, v.y);
  o.z = tbn_bn_dy1(ca.z, cb.z, cc.z, g.z, v.z);
  o.w = tbn_bn_dy1(ca.w, cb.w, cc.w, g.w, v.w);
  return o;
}
// dy with the mask recomputed from y, element by element (gate then dy: as tbn_bn_dy4(.., tbn_bn_gate4(..), ..) the four
// gates come first, which moved bn_bwd_apply_kernel<true>)
__device__ __forceinline__ float4 tbn_bn_gated_dy4(const float4& ca, const float4& cb, const float4& cc, const float4& v,
                                                   const float4& sc, const float4& sh, const float4& d) {
  float4 o;
  o.x = tbn_bn_dy1(ca.x, cb.x, cc.x, tbn_bn_gate1(v.x, sc.x, sh.x, d.x), v.x);
  o.y = tbn_bn_dy1(ca.y, cb.y, cc.y, tbn_bn_gate1(v.y, sc.y, sh.y, d.y), v.y);
  o.z = tbn_bn_dy1(ca.z, cb.z, cc.z, tbn_bn_gate1(v.z, sc.z, sh.z, d.z), v.z);
  o.w = tbn_bn_dy1(ca.w, cb.w, cc.w, tbn_bn_gate1(v.w, sc.w, sh.w, d.w), v.w);
  return o;
}

// declares sg = index of the column range (of n <= 3 in s[], ascending col_begin) that holds channel c.  A macro: as a
// function it moved the code of the kernels that use it (profiles/bn_pool_refactor.md)
#define TBN_SEG_OF(sg, s, n, c)                   \
  int sg = 0;                                     \
  if ((n) > 1 && (c) >= (s)[1].col_begin) sg = 1; \
  if ((n) > 2 && (c) >= (s)[2].col_begin) sg = 2

// row lane rs stores the sums of its quad cg (of G) to red[2 * 2048]
__device__ __forceinline__ void tbn_bn_red_put(float* red, int rs, int G, int cg, const float4 s1, const float4 s2) {
  *reinterpret_cast<float4*>(&red[(rs * G + cg) * 4]) = s1;
  *reinterpret_cast<float4*>(&red[2048 + (rs * G + cg) * 4]) = s2;
}
// after the barrier: the RP row lanes of each of the Cs channels of the workgroup's column slice (origin c0), added in
// lane order, to the partial row pair `part` (rows of pitch pld).  A macro: as a function it moved
// bn_bwd_reduce_multi_kernel and bn_res_bwd_reduce_kernel (profiles/bn_pool_refactor.md)
#define TBN_BN_RED_FOLD(red, RP, Cs, partial, part, pld, c0)                  \
  for (int cc = threadIdx.x; cc < (Cs); cc += 256) {                          \
    float a = 0.f, b = 0.f;                                                   \
    for (int r = 0; r < (RP); ++r) {                                          \
      a += (red)[r * (Cs) + cc];                                              \
      b += (red)[2048 + r * (Cs) + cc];                                       \
    }                                                                         \
    (partial)[((size_t)(part) * 2 + 0) * (pld) + (c0) + cc] = a;              \
    (partial)[((size_t)(part) * 2 + 1) * (pld) + (c0) + cc] = b;              \
  }

// forward finalize of channel c (uses s1, s2, P, c of the kernel); running_mean / conv_bias may be null.  The statistics
// are those of the bias-free conv output, the reference's BN sees conv + bias: hence mean_b.  A macro: as a function it
// moved bn_finalize_multi_kernel, whose arguments are fields of a descriptor (profiles/bn_pool_refactor.md)
#define TBN_BN_FWD_FINALIZE(gamma, beta, conv_bias, running_mean, running_var, momentum, eps, save_mean, save_rstd, scale, \
                            shift)                                                                                         \
  do {                                                                                                                     \
    const double mean = s1 / P;                                                                                            \
    double var = s2 / P - mean * mean;                                                                                     \
    if (var < 0.0) var = 0.0;                                                                                              \
    const float rstd = (float)(1.0 / sqrt(var + (double)(eps)));                                                           \
    const float sc = (gamma)[c] * rstd;                                                                                    \
    (save_mean)[c] = (float)mean;                                                                                          \
    (save_rstd)[c] = rstd;                                                                                                 \
    (scale)[c] = sc;                                                                                                       \
    (shift)[c] = fmaf(-(float)mean, sc, (beta)[c]);                                                                        \
    if ((running_mean) != nullptr) {                                                                                       \
      const double unb = P > 1 ? var * ((double)P / (double)(P - 1)) : var;                                                \
      const float mean_b = (float)mean + ((conv_bias) != nullptr ? (conv_bias)[c] : 0.f);                                  \
      (running_mean)[c] = (1.f - (momentum)) * (running_mean)[c] + (momentum) * mean_b;                                    \
      (running_var)[c] = (1.f - (momentum)) * (running_var)[c] + (momentum) * (float)unb;                                  \
    }                                                                                                                      \
  } while (0)

// backward finalize of channel c (uses s1, s2, P, C, c of the kernel): the three coef rows (pitch C) and the parameter
// gradients, each of which may be null; a per-channel constant added before a batch-stat BN has exactly zero gradient.
// A macro: as a function it moved the code of both kernels that use it (profiles/bn_pool_refactor.md)
#define TBN_BN_BWD_FINALIZE(scale, mean, rstd, coef, dgamma, dbeta, dbias)   \
  do {                                                                       \
    const double sc = (scale)[c], rs = (rstd)[c], mu = (mean)[c];            \
    const double bb = -sc * rs * (s2 / P);                                   \
    (coef)[c] = (float)sc;                                                   \
    (coef)[C + c] = (float)bb;                                               \
    (coef)[2 * C + c] = (float)(-sc * (s1 / P) - bb * mu);                   \
    if (dgamma) (dgamma)[c] = (float)s2;                                     \
    if (dbeta) (dbeta)[c] = (float)s1;                                       \
    if (dbias) (dbias)[c] = 0.f;                                             \
  } while (0)

// Channels per finalize workgroup (a build-time knob: -DTBN_FIN_CH=4 | 8 | 16).  The finalize kernels sit on the
// conv -> BN -> conv dependency chain and are pure latency (a step's ~190 of them cost 1.16 ms of step time at ~6 us
// each, DESIGN.md finding 14): round 2 went from 8 channels x 32 row slots with scalar loads to 16 channels x 64 slots
// with 16-B loads (9 -> 3 us for 588 rows, -0.97 ms per step).  Round 4 measured the next step of the same idea -- ONE
// channel quad per workgroup and 256 row slots: 4x the workgroups, one round of loads instead of three for 588 rows --
// and it bought nothing (same-box A/B, three alternations: 36.05 vs 35.98 ms; config 2 12.31 vs 12.23; config 3 50.53 vs
// 50.42; profiles/r04_ab_finalize_channels.txt): what a finalize costs now is its launch boundary on the chain, not the
// rows a thread walks.  16 stays.
#ifndef TBN_FIN_CH
#define TBN_FIN_CH 16
#endif

// Sums partial[(i*2 + s) * pld + c] over i < nparts for the CH channels [c0, c0 + CH) and s in {0, 1}.
// 256 threads = CH/4 float4 channel quads x S = 1024/CH row slots: a thread walks rows slot, slot + S, ... with four
// independent 16-B loads in flight per statistic, then the S slot sums are added in a fixed two-level order (groups of 8
// slots, then the groups): the result does not depend on scheduling (deterministic).
// Returns the two sums of channel c0 + tid in threads tid < CH (others: zeros); `red` = 2048 doubles of LDS.
template <int CH>
__device__ __forceinline__ void tbn_sum_partials(const float* __restrict__ partial, int pld, int nparts, int c0, int C,
                                                 double* red, double* out_s1, double* out_s2) {
  constexpr int Q = CH / 4, S = 256 / Q, V = Q * 8, G = S / 8;
  static_assert(CH == 4 || CH == 8 || CH == 16, "finalize: 4, 8 or 16 channels per workgroup");
  const int tid = threadIdx.x, cq = tid % Q, slot = tid / Q;
  const int c = c0 + cq * 4;
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
  if (c < C) {
    const float* p = partial + c;
    for (int i = slot; i < nparts; i += 4 * S) {
      float4 u[4], v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int r = i + S * k;
        const bool ok = r < nparts;
        const size_t rr = (size_t)(ok ? r : i);          // an in-range row: the load is issued either way
        u[k] = *reinterpret_cast<const float4*>(p + (rr * 2 + 0) * pld);
        v[k] = *reinterpret_cast<const float4*>(p + (rr * 2 + 1) * pld);
        if (!ok) u[k] = v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a0 += (double)u[k].x; a1 += (double)u[k].y; a2 += (double)u[k].z; a3 += (double)u[k].w;
        b0 += (double)v[k].x; b1 += (double)v[k].y; b2 += (double)v[k].z; b3 += (double)v[k].w;
      }
    }
  }
  double* r = red + slot * V + cq * 8;                   // per slot: per quad a0..a3 b0..b3
  r[0] = a0; r[1] = a1; r[2] = a2; r[3] = a3;
  r[4] = b0; r[5] = b1; r[6] = b2; r[7] = b3;
  __syncthreads();
  const int vi = tid % V, g = tid / V;                   // level 1: value vi of slot group g (8 slots), V * G = 256 threads
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += red[(g * 8 + k) * V + vi];
  __syncthreads();
  red[g * V + vi] = s;
  __syncthreads();
  double t = 0.0;
  if (tid < V) {                                         // level 2: the G group sums of value tid
#pragma unroll 8
    for (int gg = 0; gg < G; ++gg) t += red[gg * V + tid];
  }
  __syncthreads();
  if (tid < V) red[tid] = t;
  __syncthreads();
  // channel j of the workgroup = quad j / 4, component j % 4: S1 at value (j/4)*8 + j%4, S2 four further
  *out_s1 = (tid < CH) ? red[(tid >> 2) * 8 + (tid & 3)] : 0.0;
  *out_s2 = (tid < CH) ? red[(tid >> 2) * 8 + 4 + (tid & 3)] : 0.0;
}
