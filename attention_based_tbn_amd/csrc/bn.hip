// BatchNorm2d (+ReLU) for NHWC fp32 activations on gfx950: HBM-bound streaming kernels.
//
// Reference semantics: every conv of the backbone is followed by nn.BatchNorm2d(C, affine=True)
// (eps 1e-5, momentum 0.1) + ReLU(inplace) (reference core/models/bn_inception_audio.py:24-31 ...).
// Training keeps the modules in .train() (core/tools/train.py:68) so *batch statistics* are used
// and running stats are updated even for the "partialbn"-frozen layers (core/models/model.py:164-176
// only freezes the affine parameters); eval (train.py:146, test.py:67) uses the running stats.
//
// Channel is the fastest dim, so a wave reads 16 B / lane fully coalesced and every lane owns 4
// fixed channels: per-channel reductions are register accumulations + one fixed-order LDS pass,
// written as per-workgroup partials and summed in fp64 by a finalize kernel (deterministic).
#include "tbn_common.h"
#include "tbn_kernels.h"
#include "tbn_bn_dev.h"
#include "tbn_pool_dev.h"

// ---------------------------------------------------------------- forward statistics (standalone)
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ y, int ld, int P, int C, int pch,
                                                       float* __restrict__ partial) {
  __shared__ float red[2 * 2048];
  const int G = C >> 2, RP = 256 / G;
  const int tid = threadIdx.x, cg = tid % G, rs = tid / G;
  const int p0 = blockIdx.x * pch, p1 = min(P, p0 + pch);
  float4 s1 = make_float4(0, 0, 0, 0), s2 = s1;
  if (rs < RP)
    for (int p = p0 + rs; p < p1; p += RP) {
      const float4 v = *reinterpret_cast<const float4*>(y + (size_t)p * ld + cg * 4);
      s1.x += v.x; s1.y += v.y; s1.z += v.z; s1.w += v.w;
      s2.x = fmaf(v.x, v.x, s2.x); s2.y = fmaf(v.y, v.y, s2.y); s2.z = fmaf(v.z, v.z, s2.z); s2.w = fmaf(v.w, v.w, s2.w);
    }
  if (rs < RP) tbn_bn_red_put(red, rs, G, cg, s1, s2);
  __syncthreads();
  TBN_BN_RED_FOLD(red, RP, C, partial, blockIdx.x, C, 0)
}

int tbn_bn_stats_parts(int P, int C) { return tbn_bn_reduce_parts(P, C); }

int tbn_launch_bn_stats(const float* y, int ld, int P, int C, float* partial, int* nparts, hipStream_t st) {
  TBN_REQUIRE(P >= 1 && C >= 4 && C % 4 == 0 && C <= 1024 && ld % 4 == 0 && ld >= C,
              "bn_stats: P >= 1, C a multiple of 4 in 4..1024, pitch a multiple of 4 and at least C");
  const int pch = tbn_bn_reduce_chunk(P, C), parts = cdiv(P, pch);
  TBN_KLAUNCH(bn_stats_kernel, dim3(parts), dim3(256), 0, st, y, ld, P, C, pch, partial);
  TBN_CHECK_LAUNCH("bn_stats");
  if (nparts) *nparts = parts;
  return TBN_OK;
}

// ---------------------------------------------------------------- finalize: partials -> mean/rstd/scale/shift
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ partial, int nparts, int P, int C,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          const float* __restrict__ conv_bias, float* running_mean,
                                                          float* running_var, float momentum, float eps,
                                                          float* save_mean, float* save_rstd, float* scale,
                                                          float* shift) {
  // 16 channels per workgroup, fixed summation order (tbn_bn_dev.h)
  __shared__ double red[64 * 32];
  const int tid = threadIdx.x;
  const int c = blockIdx.x * TBN_FIN_CH + tid;
  double s1, s2;
  tbn_sum_partials<TBN_FIN_CH>(partial, C, nparts, blockIdx.x * TBN_FIN_CH, C, red, &s1, &s2);
  if (tid < TBN_FIN_CH && c < C)
    TBN_BN_FWD_FINALIZE(gamma, beta, conv_bias, running_mean, running_var, momentum, eps, save_mean, save_rstd, scale,
                        shift);
}

int tbn_launch_bn_finalize(const float* partial, int nparts, int P, int C, const float* gamma, const float* beta,
                           const float* conv_bias, float* running_mean, float* running_var, float momentum, float eps,
                           float* save_mean, float* save_rstd, float* scale, float* shift, hipStream_t st) {
  TBN_KLAUNCH(bn_finalize_kernel, dim3(cdiv(C, TBN_FIN_CH)), dim3(256), 0, st, partial, nparts, P, C, gamma, beta,
                     conv_bias, running_mean, running_var, momentum, eps, save_mean, save_rstd, scale, shift);
  TBN_CHECK_LAUNCH("bn_finalize");
  return TBN_OK;
}

// ---------------------------------------------------------------- apply: z = relu(y*scale+shift) -> concat slices
struct Seg3 {
  Seg s[3];
  int n;
};
struct CSeg3 {
  CSeg s[3];
  int n;
};

__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ y, int P, int C,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift, Seg3 segs, FastDiv divg) {
  const int G = C >> 2;
  const uint32_t total = (uint32_t)P * G;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const int p = (int)fdiv(i, divg), c = (int)(i - (uint32_t)p * (uint32_t)G) * 4;
    const float4 v = *reinterpret_cast<const float4*>(y + (size_t)p * C + c);
    const float4 sc = *reinterpret_cast<const float4*>(scale + c);
    const float4 sh = *reinterpret_cast<const float4*>(shift + c);
    TBN_SEG_OF(sg, segs.s, segs.n, c);
    *reinterpret_cast<float4*>(segs.s[sg].ptr + (size_t)p * segs.s[sg].ld + (c - segs.s[sg].col_begin)) = tbn_bn_relu4(v, sc, sh);
  }
}

int tbn_launch_bn_apply(const float* y, int P, int C, const float* scale, const float* shift, const Seg* segs,
                        int nseg, hipStream_t st) {
  TBN_REQUIRE(C % 4 == 0 && nseg >= 1 && nseg <= 3, "bn_apply: bad C/nseg");
  TBN_REQUIRE(tbn_segs_x4(segs, nseg), "bn_apply: segment pitch/offset must be x4");
  Seg3 s3;
  s3.n = nseg;
  for (int i = 0; i < nseg; ++i) s3.s[i] = segs[i];
  TBN_REQUIRE((size_t)P * (C / 4) < (1ull << 31), "bn_apply: too many elements per call");
  TBN_KLAUNCH(bn_apply_kernel, dim3(ew_grid((size_t)P * C / 4, 4096)), dim3(256), 0, st, y, P, C, scale, shift, s3,
                     make_fastdiv((uint32_t)(C / 4)));
  TBN_CHECK_LAUNCH("bn_apply");
  return TBN_OK;
}

// ---------------------------------------------------------------- eval fold: running stats -> scale/shift
// scale = gamma / sqrt(var + eps);  shift = beta + (conv_bias - mean) * scale   (the conv epilogue
// then computes relu(acc * scale + shift) on the bias-free accumulator)
__global__ void bn_fold_kernel(const float* gamma, const float* beta, const float* mean, const float* var,
                               const float* bias, float eps, float* scale, float* shift, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    const float sc = gamma[c] / sqrtf(var[c] + eps);
    scale[c] = sc;
    shift[c] = fmaf((bias != nullptr ? bias[c] : 0.f) - mean[c], sc, beta[c]);
  }
}

int tbn_launch_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, const float* bias,
                       float eps, float* scale, float* shift, int C, hipStream_t st) {
  TBN_KLAUNCH(bn_fold_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, gamma, beta, mean, var, bias, eps, scale,
                     shift, C);
  TBN_CHECK_LAUNCH("bn_fold");
  return TBN_OK;
}

// ---------------------------------------------------------------- apply + 3x3 max pool in one pass
// For a conv whose BN-ReLU output is consumed ONLY by a max pool (the stem: conv1 -> pool1, conv2_3x3 -> pool2):
// z = relu(y*scale+shift) is formed in registers and pooled at once; z itself is never written (the backward
// recomputes the ReLU mask from y anyway).  Same comparison order as maxpool_fwd_kernel on a stored z (first
// maximum in scan order, NaN propagates), so values and arg-max are identical to the two-pass form.
__global__ __launch_bounds__(256) void bn_apply_maxpool_kernel(const float* __restrict__ y, int N, int H, int W, int C,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift,
                                                               float* __restrict__ out, int out_ld,
                                                               unsigned char* __restrict__ argmax, int OH, int OW,
                                                               int stride, int pad, PixDecode dec) {
  const int G = C >> 2;
  const uint32_t total = (uint32_t)N * OH * OW * G;
  for (uint32_t i = tbn_xcd_block_id() * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    int g, ox, oy, n;
    uint32_t opix;
    pix_decode(dec, i, g, ox, oy, n, opix);
    const int y0 = oy * stride - pad, x0 = ox * stride - pad;
    const float4 sc = *reinterpret_cast<const float4*>(scale + g * 4);
    const float4 sh = *reinterpret_cast<const float4*>(shift + g * 4);
    // z >= 0 or NaN: the first in-bounds tap always takes, the start index 0 is never kept
    TBN_MAX3X3(best, b, y, C, n, H, W, y0, x0, g * 4, 0, z, float4 z;
               z.x = tbn_bn_relu1(v.x, sc.x, sh.x); z.y = tbn_bn_relu1(v.y, sc.y, sh.y);
               z.z = tbn_bn_relu1(v.z, sc.z, sh.z); z.w = tbn_bn_relu1(v.w, sc.w, sh.w););
    *reinterpret_cast<float4*>(out + (size_t)opix * out_ld + g * 4) = best;
    *reinterpret_cast<uint32_t*>(argmax + (size_t)opix * C + g * 4) = tbn_argmax_word(bx, by, bz, bw);
  }
}

int tbn_launch_bn_apply_maxpool(const float* y, int N, int H, int W, int C, const float* scale, const float* shift,
                                float* out, int out_ld, unsigned char* argmax, int OH, int OW, int stride, int pad,
                                hipStream_t st) {
  TBN_REQUIRE(C % 4 == 0 && out_ld % 4 == 0 && argmax != nullptr, "bn_apply_maxpool: bad C / pitch / argmax");
  TBN_REQUIRE((size_t)N * H * W * (C / 4) < (1ull << 31), "bn_apply_maxpool: too many elements per call");
  TBN_KLAUNCH(bn_apply_maxpool_kernel, dim3(ew_grid((size_t)N * OH * OW * (C / 4), 8192)), dim3(256), 0, st, y, N, H, W, C, scale,
                     shift, out, out_ld, argmax, OH, OW, stride, pad, make_pixdecode(C / 4, OW, OH));
  TBN_CHECK_LAUNCH("bn_apply_maxpool");
  return TBN_OK;
}

// Gradient of a max pool's INPUT formed on the fly from the pooled gradient and the stored arg-max (tbn_pool_gather, the
// gather of maxpool_bwd_kernel): used by the BN-backward kernels of a conv fused with its pool, so dz is never materialised.
struct PoolGrad {
  const float* dout;            // gradient of the pooled tensor (N, OH, OW, C) with pitch dout_ld
  const unsigned char* argmax;  // (N, OH, OW, C) uint8 window index
  int dout_ld, H, W, OH, OW, C, stride, pad;
  FastDiv div_w, div_h;
};
__device__ __forceinline__ float4 pooled_grad(const PoolGrad& q, int p, int c) {
  const uint32_t row = fdiv((uint32_t)p, q.div_w);        // n*H + iy
  const int ix = p - (int)row * q.W;
  const uint32_t n = fdiv(row, q.div_h);
  const int iy = (int)row - (int)n * q.H;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q.stride == 2 && q.pad == 0) {
    TBN_POOL_GATHER_S2(acc, q.dout, q.dout_ld, q.argmax, q.C, q.OH, q.OW, (int)n, iy, ix, c);
    return acc;
  }
  TBN_POOL_GATHER_LOOPS(acc, q.dout, q.dout_ld, q.argmax, q.C, q.OH, q.OW, q.stride, q.pad, (int)n, iy, ix, c);
  return acc;
}

// ---------------------------------------------------------------- backward
// g = dz * [y*scale+shift > 0];  xhat = (y-mean)*rstd;  S1 = sum g, S2 = sum g*xhat
template <bool POOLED>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(CSeg3 dz, PoolGrad pg, const float* __restrict__ y, int P,
                                                            int C, int pch, const float* __restrict__ scale,
                                                            const float* __restrict__ shift,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ rstd,
                                                            float* __restrict__ partial) {
  __shared__ float red[2 * 2048];
  const int G = C >> 2, RP = 256 / G;
  const int tid = threadIdx.x, cg = tid % G, rs = tid / G, c = cg * 4;
  const int p0 = blockIdx.x * pch, p1 = min(P, p0 + pch);
  float4 s1 = make_float4(0, 0, 0, 0), s2 = s1;
  if (rs < RP) {
    TBN_SEG_OF(sg, dz.s, dz.n, c);
    const float* dzp = POOLED ? nullptr : dz.s[sg].ptr + (c - dz.s[sg].col_begin);
    const int dld = dz.s[sg].ld;
    const float4 sc = *reinterpret_cast<const float4*>(scale + c);
    const float4 sh = *reinterpret_cast<const float4*>(shift + c);
    const float4 mu = *reinterpret_cast<const float4*>(mean + c);
    const float4 rs4 = *reinterpret_cast<const float4*>(rstd + c);
    for (int p = p0 + rs; p < p1; p += RP) {
      const float4 v = *reinterpret_cast<const float4*>(y + (size_t)p * C + c);
      const float4 d = POOLED ? pooled_grad(pg, p, c) : *reinterpret_cast<const float4*>(dzp + (size_t)p * dld);
      tbn_bn_sums4(s1, s2, tbn_bn_gate4(v, sc, sh, d), v, mu, rs4);
    }
    tbn_bn_red_put(red, rs, G, cg, s1, s2);
  }
  __syncthreads();
  TBN_BN_RED_FOLD(red, RP, C, partial, blockIdx.x, C, 0)
}

int tbn_bn_bwd_parts(int P, int C) { return tbn_bn_stats_parts(P, C); }

static int fill_cseg3(CSeg3* o, const CSeg* s, int n) {
  o->n = n;
  for (int i = 0; i < n; ++i) o->s[i] = s[i];
  return tbn_segs_x4(s, n) ? 0 : -1;
}

int tbn_launch_bn_bwd_reduce(const CSeg* dz, int nseg, const float* y, int P, int C, const float* scale,
                             const float* shift, const float* mean, const float* rstd, float* partial,
                             hipStream_t st) {
  TBN_REQUIRE(C % 4 == 0 && C <= 1024 && nseg >= 1 && nseg <= 3, "bn_bwd_reduce: bad C/nseg");
  CSeg3 s3;
  TBN_REQUIRE(fill_cseg3(&s3, dz, nseg) == 0, "bn_bwd_reduce: segment pitch/offset must be x4");
  const int pch = tbn_bn_reduce_chunk(P, C), parts = cdiv(P, pch);
  PoolGrad none = {};
  TBN_KLAUNCH(bn_bwd_reduce_kernel<false>, dim3(parts), dim3(256), 0, st, s3, none, y, P, C, pch, scale, shift,
                     mean, rstd, partial);
  TBN_CHECK_LAUNCH("bn_bwd_reduce");
  return TBN_OK;
}

static PoolGrad make_poolgrad(const float* dout, int dout_ld, const unsigned char* argmax, int H, int W, int OH, int OW,
                              int C, int stride, int pad) {
  PoolGrad q;
  q.dout = dout; q.argmax = argmax; q.dout_ld = dout_ld;
  q.H = H; q.W = W; q.OH = OH; q.OW = OW; q.C = C; q.stride = stride; q.pad = pad;
  q.div_w = make_fastdiv((uint32_t)W);
  q.div_h = make_fastdiv((uint32_t)H);
  return q;
}

// ---------------------------------------------------------------- fused-pool backward on 2x2 input blocks
// 3x3 / stride 2 / pad 0 (the stem pools: the only fused ones).  pooled_grad() above evaluates four candidate windows
// for every input pixel; taken as a 2x2 block (even-even, even-odd, odd-even, odd-odd pixel) the four pixels share the
// SAME four windows -- (by, bx), (by, bx-1), (by-1, bx), (by-1, bx-1) -- and only 9 (pixel, window) pairs exist:
// one arg-max word + one gradient quad per window are loaded once per block instead of four per pixel (4x fewer
// loads, ~2x fewer VALU instructions on the two largest tensors of the network).  Same per-pixel summation order.
__global__ __launch_bounds__(256) void bn_bwd_reduce_pooled2x2_kernel(PoolBlk pb, const float* __restrict__ y, int NQ,
                                                                       int C, int qch, const float* __restrict__ scale,
                                                                       const float* __restrict__ shift,
                                                                       const float* __restrict__ mean,
                                                                       const float* __restrict__ rstd,
                                                                       float* __restrict__ partial) {
  __shared__ float red[2 * 2048];
  const int G = C >> 2, RP = 256 / G;
  const int tid = threadIdx.x, cg = tid % G, rs = tid / G, c = cg * 4;
  const int q0 = blockIdx.x * qch, q1 = min(NQ, q0 + qch);
  float4 s1 = make_float4(0, 0, 0, 0), s2 = s1;
  if (rs < RP) {
    const float4 sc = *reinterpret_cast<const float4*>(scale + c);
    const float4 sh = *reinterpret_cast<const float4*>(shift + c);
    const float4 mu = *reinterpret_cast<const float4*>(mean + c);
    const float4 rs4 = *reinterpret_cast<const float4*>(rstd + c);
    for (int q = q0 + rs; q < q1; q += RP) {
      TBN_BLK_DECODE(pb, q, n, by, bx);
      float4 g[4];
      pooled_grad_2x2(pb, n, by, bx, c, g);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int iy = 2 * by + (i >> 1), ix = 2 * bx + (i & 1);
        if (iy < pb.H && ix < pb.W) {
          const float4 v = *reinterpret_cast<const float4*>(y + ((size_t)(n * pb.H + iy) * pb.W + ix) * C + c);
          tbn_bn_sums4(s1, s2, tbn_bn_gate4(v, sc, sh, g[i]), v, mu, rs4);
        }
      }
    }
    tbn_bn_red_put(red, rs, G, cg, s1, s2);
  }
  __syncthreads();
  TBN_BN_RED_FOLD(red, RP, C, partial, blockIdx.x, C, 0)
}

__global__ __launch_bounds__(256) void bn_bwd_apply_pooled2x2_kernel(PoolBlk pb, const float* y, int NQ, int C,
                                                                      const float* __restrict__ scale,
                                                                      const float* __restrict__ shift,
                                                                      const float* __restrict__ coef, float* dy,
                                                                      FastDiv divg) {
  const int G = C >> 2;
  const uint32_t total = (uint32_t)NQ * G;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t q = fdiv(i, divg);
    const int c = (int)(i - q * (uint32_t)G) * 4;
    TBN_BLK_DECODE(pb, q, n, by, bx);
    float4 g[4];
    pooled_grad_2x2(pb, n, by, bx, c, g);
    const float4 sc = *reinterpret_cast<const float4*>(scale + c);
    const float4 sh = *reinterpret_cast<const float4*>(shift + c);
    const float4 ca = *reinterpret_cast<const float4*>(coef + c);
    const float4 cb = *reinterpret_cast<const float4*>(coef + C + c);
    const float4 cc = *reinterpret_cast<const float4*>(coef + 2 * C + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int iy = 2 * by + (k >> 1), ix = 2 * bx + (k & 1);
      if (iy < pb.H && ix < pb.W) {
        const size_t off = ((size_t)(n * pb.H + iy) * pb.W + ix) * C + c;
        const float4 v = tbn_ld4<(TBN_BN_NT & 8) != 0>(y + off);
        *reinterpret_cast<float4*>(dy + off) = tbn_bn_gated_dy4(ca, cb, cc, v, sc, sh, g[k]);
      }
    }
  }
}

// number of partial rows the pooled reduce writes (the engine sizes the finalize by it)
int tbn_bn_bwd_pooled_parts(int N, int H, int W, int C, int stride, int pad) {
  if (stride == 2 && pad == 0) return tbn_bn_reduce_parts(N * ((H + 1) / 2) * ((W + 1) / 2), C);
  return tbn_bn_reduce_parts(N * H * W, C);
}

// BN-backward reduce / apply of a conv fused with its max pool: dz = gather(dpooled, argmax) on the fly
int tbn_launch_bn_bwd_reduce_pooled(const float* dpooled, int dpooled_ld, const unsigned char* argmax, int N, int H,
                                    int W, int OH, int OW, int stride, int pad, const float* y, int C,
                                    const float* scale, const float* shift, const float* mean, const float* rstd,
                                    float* partial, hipStream_t st) {
  TBN_REQUIRE(C % 4 == 0 && C <= 1024 && dpooled_ld % 4 == 0, "bn_bwd_reduce_pooled: bad C / pitch");
  TBN_REQUIRE((long)N * H * W < (1l << 31), "bn_bwd_reduce_pooled: too many pixels");
  if (stride == 2 && pad == 0) {
    const int NQ = N * ((H + 1) / 2) * ((W + 1) / 2);
    const int qch = tbn_bn_reduce_chunk(NQ, C), parts = cdiv(NQ, qch);
    TBN_KLAUNCH(bn_bwd_reduce_pooled2x2_kernel, dim3(parts), dim3(256), 0, st,
                       make_poolblk(dpooled, dpooled_ld, argmax, H, W, OH, OW, C), y, NQ, C, qch, scale, shift, mean, rstd,
                       partial);
    TBN_CHECK_LAUNCH("bn_bwd_reduce_pooled2x2");
    return TBN_OK;
  }
  const int P = N * H * W;
  CSeg3 s3 = {};
  s3.n = 1;
  const int pch = tbn_bn_reduce_chunk(P, C), parts = cdiv(P, pch);
  TBN_KLAUNCH(bn_bwd_reduce_kernel<true>, dim3(parts), dim3(256), 0, st, s3,
                     make_poolgrad(dpooled, dpooled_ld, argmax, H, W, OH, OW, C, stride, pad), y, P, C, pch, scale,
                     shift, mean, rstd, partial);
  TBN_CHECK_LAUNCH("bn_bwd_reduce_pooled");
  return TBN_OK;
}

// coef[0][c]=a, coef[1][c]=b, coef[2][c]=cst with dy = a*g + b*y + cst
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int nparts, int P,
                                                              int C, const float* __restrict__ scale,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, float* coef,
                                                              float* dgamma, float* dbeta, float* dbias) {
  __shared__ double red[64 * 32];
  const int tid = threadIdx.x;
  const int c = blockIdx.x * TBN_FIN_CH + tid;
  double s1, s2;
  tbn_sum_partials<TBN_FIN_CH>(partial, C, nparts, blockIdx.x * TBN_FIN_CH, C, red, &s1, &s2);
  if (tid < TBN_FIN_CH && c < C) TBN_BN_BWD_FINALIZE(scale, mean, rstd, coef, dgamma, dbeta, dbias);
}

int tbn_launch_bn_bwd_finalize(const float* partial, int nparts, int P, int C, const float* scale, const float* mean,
                               const float* rstd, float* coef, float* dgamma, float* dbeta, float* dbias,
                               hipStream_t st) {
  TBN_KLAUNCH(bn_bwd_finalize_kernel, dim3(cdiv(C, TBN_FIN_CH)), dim3(256), 0, st, partial, nparts, P, C, scale, mean,
                     rstd, coef, dgamma, dbeta, dbias);
  TBN_CHECK_LAUNCH("bn_bwd_finalize");
  return TBN_OK;
}

// y and dy may alias (the engine converts y to dy in place): no __restrict__ on them
template <bool POOLED>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(CSeg3 dz, PoolGrad pg, const float* y, int P, int C,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift,
                                                           const float* __restrict__ coef, float* dy, FastDiv divg) {
  const int G = C >> 2;
  const uint32_t total = (uint32_t)P * G;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const int p = (int)fdiv(i, divg), c = (int)(i - (uint32_t)p * (uint32_t)G) * 4;
    TBN_SEG_OF(sg, dz.s, dz.n, c);
    const float4 d = POOLED ? pooled_grad(pg, p, c)
                            : *reinterpret_cast<const float4*>(dz.s[sg].ptr + (size_t)p * dz.s[sg].ld +
                                                               (c - dz.s[sg].col_begin));
    const float4 v = *reinterpret_cast<const float4*>(y + (size_t)p * C + c);
    const float4 sc = *reinterpret_cast<const float4*>(scale + c);
    const float4 sh = *reinterpret_cast<const float4*>(shift + c);
    const float4 ca = *reinterpret_cast<const float4*>(coef + c);
    const float4 cb = *reinterpret_cast<const float4*>(coef + C + c);
    const float4 cc = *reinterpret_cast<const float4*>(coef + 2 * C + c);
    *reinterpret_cast<float4*>(dy + (size_t)p * C + c) = tbn_bn_gated_dy4(ca, cb, cc, v, sc, sh, d);
  }
}

int tbn_launch_bn_bwd_apply(const CSeg* dz, int nseg, const float* y, int P, int C, const float* scale,
                            const float* shift, const float* coef, float* dy, hipStream_t st) {
  CSeg3 s3;
  TBN_REQUIRE(C % 4 == 0 && nseg >= 1 && nseg <= 3 && fill_cseg3(&s3, dz, nseg) == 0, "bn_bwd_apply: bad segments");
  PoolGrad none = {};
  TBN_REQUIRE((size_t)P * (C / 4) < (1ull << 31), "bn_bwd_apply: too many elements per call");
  TBN_KLAUNCH(bn_bwd_apply_kernel<false>, dim3(ew_grid((size_t)P * C / 4, 4096)), dim3(256), 0, st, s3, none, y, P, C,
                     scale, shift, coef, dy, make_fastdiv((uint32_t)(C / 4)));
  TBN_CHECK_LAUNCH("bn_bwd_apply");
  return TBN_OK;
}

int tbn_launch_bn_bwd_apply_pooled(const float* dpooled, int dpooled_ld, const unsigned char* argmax, int N, int H, int W,
                                   int OH, int OW, int stride, int pad, const float* y, int C, const float* scale,
                                   const float* shift, const float* coef, float* dy, hipStream_t st) {
  TBN_REQUIRE(C % 4 == 0 && dpooled_ld % 4 == 0, "bn_bwd_apply_pooled: bad C / pitch");
  if (stride == 2 && pad == 0) {
    const int NQ = N * ((H + 1) / 2) * ((W + 1) / 2);
    TBN_REQUIRE((size_t)NQ * (C / 4) < (1ull << 31), "bn_bwd_apply_pooled: too many elements per call");
    TBN_KLAUNCH(bn_bwd_apply_pooled2x2_kernel, dim3(ew_grid((size_t)NQ * C / 4, 4096)), dim3(256), 0, st,
                       make_poolblk(dpooled, dpooled_ld, argmax, H, W, OH, OW, C), y, NQ, C, scale, shift, coef, dy,
                       make_fastdiv((uint32_t)(C / 4)));
    TBN_CHECK_LAUNCH("bn_bwd_apply_pooled2x2");
    return TBN_OK;
  }
  const int P = N * H * W;
  CSeg3 s3 = {};
  s3.n = 1;
  TBN_KLAUNCH(bn_bwd_apply_kernel<true>, dim3(ew_grid((size_t)P * C / 4, 4096)), dim3(256), 0, st, s3,
                     make_poolgrad(dpooled, dpooled_ld, argmax, H, W, OH, OW, C, stride, pad), y, P, C, scale, shift,
                     coef, dy, make_fastdiv((uint32_t)(C / 4)));
  TBN_CHECK_LAUNCH("bn_bwd_apply_pooled");
  return TBN_OK;
}
