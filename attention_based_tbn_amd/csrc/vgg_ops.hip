// The three operators a VGG needs beside the 3x3 convolutions and the Linear layers (include/tbn_hip.h: tbn_conv3_first_*,
// tbn_maxpool2_*, tbn_adaptive_avgpool7_*), fp32.
//
// Reference ops (core/models/vgg.py:15-41, torchvision's vgg11 / vgg16 with and without BatchNorm):
//   features[0] = Conv2d(cin, 64, 3, padding 1) from the NCHW frames, cin = 3 (RGB), 10 (Flow), 1 (Audio)
//   MaxPool2d(2, 2)                             five times
//   AdaptiveAvgPool2d((7, 7)) + flatten         in front of the classifier
//
// First convolution: 9 cin multiply-adds per output value (27 / 90 / 9) and 256 B written per pixel -- a streaming kernel of
// plain fp32 FMAs in the shape of audio_stem.hip, no MFMA.  A workgroup takes F3_STRIP output rows of ONE frame and walks
// them in tiles of F3_ROWS rows x F3_XT pixels: the F3_ROWS + 2 input rows of every channel are staged in LDS with coalesced
// row loads (reads outside the image become zeros THERE, so every global read is bounds-checked in one place), the weights
// sit in LDS as [tap][ci][64] for the whole workgroup.  A lane owns 4 consecutive output channels of 4 consecutive pixels:
// per (filter row, input channel) it reads its 6 input values (shared by the 16 lanes of a pixel group: broadcast) and three
// float4 of weights and issues 48 FMAs, in the fixed order filter row -> input channel -> filter column.  The 16 lanes of a
// pixel store its 256 B as one contiguous run.
// The weight gradient walks the same tiles: a lane owns 4 output channels x 9 taps of ONE input channel (36 accumulators),
// the 16 lane groups are (input channel slot) x (pixel slot), a pixel slot walks the tile in runs of 4 consecutive pixels (four
// dy loads in flight, the 6 staged inputs of a filter row shared); pixel slots are combined through LDS in fixed order, ONE
// [64][3][3][cin] partial per workgroup is written, and a second launch sums the workgroups in fixed order in fp64 (the
// convention of tbn_sum_partials).  No atomics anywhere in this file.
#include "tbn_common.h"
#include "tbn_hip.h"

#define F3_STRIP 8                   // output rows of a frame per workgroup
#define F3_ROWS 2                    // output rows per staged tile
#define F3_XT 64                     // output pixels of a row per tile
#define F3_XP 68                     // LDS pitch of a staged row: F3_XT + 2 columns, rounded up to x4
#define F3_WGRAD_MAX_WG 1024         // workgroups (= partials) of the weight gradient

struct F3Geom {
  int N, C, H, W;
  int spf;                           // strips per frame
  int strips;                        // N * spf
};

// stages input rows oy0 - 1 .. oy0 + F3_ROWS of every channel of frame n, columns ox0 - 1 + (0 .. F3_XP - 1):
// tile[(t * C + ci) * F3_XP + cx]
__device__ __forceinline__ void f3_stage(const float* __restrict__ x, const F3Geom& g, int n, int oy0, int ox0,
                                         float* __restrict__ tile) {
  const int total = (F3_ROWS + 2) * g.C * F3_XP;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int lr = i / F3_XP, cx = i - lr * F3_XP;
    const int t = lr / g.C, ci = lr - t * g.C;
    const int iy = oy0 - 1 + t, ix = ox0 - 1 + cx;
    float v = 0.f;
    if ((unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W)
      v = x[(((size_t)n * g.C + ci) * g.H + iy) * g.W + ix];
    tile[i] = v;
  }
}

template <int EPI>   // 0: + bias (RELU by flag), 1: raw + statistics partial row per workgroup, 2: relu(acc * scale + shift)
__global__ __launch_bounds__(256) void conv3_first_fwd_kernel(const float* __restrict__ x, const float* __restrict__ weight,
                                                              const float* __restrict__ bias, float* __restrict__ out,
                                                              int out_ld, F3Geom g, int relu,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ shift,
                                                              float* __restrict__ stat_partial) {
  extern __shared__ float4 f3_lds4[];
  float* wl = reinterpret_cast<float*>(f3_lds4);      // [9 * C][64]
  float* tile = wl + 9 * g.C * 64;                    // [(F3_ROWS + 2) * C][F3_XP]; the statistics combine reuses it
  const int cl = threadIdx.x & 15, slot = threadIdx.x >> 4;
  const int K = 9 * g.C;
  // weight [co][tap][ci] -> wl[(tap * C + ci) * 64 + co]: consecutive lanes take consecutive co (LDS writes without
  // conflicts; the strided global reads stay in cache, the tensor is at most 36 KB)
  for (int i = threadIdx.x; i < K * 64; i += 256) {
    const int k = i >> 6, co = i & 63;
    wl[i] = weight[(size_t)co * K + k];
  }
  float e0[4], e1[4];     // epilogue 0: bias | 0;  epilogue 2: scale | shift
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    e0[j] = EPI == 0 ? (bias != nullptr ? bias[cl * 4 + j] : 0.f) : (EPI == 2 ? scale[cl * 4 + j] : 0.f);
    e1[j] = EPI == 2 ? shift[cl * 4 + j] : 0.f;
  }
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  const int n = blockIdx.x / g.spf, strip = blockIdx.x - n * g.spf;
  const int oyb = strip * F3_STRIP;
  const int oye = min(oyb + F3_STRIP, g.H);
  for (int oy0 = oyb; oy0 < oye; oy0 += F3_ROWS) {
    for (int ox0 = 0; ox0 < g.W; ox0 += F3_XT) {
      __syncthreads();                 // the previous tile has been read
      f3_stage(x, g, n, oy0, ox0, tile);
      __syncthreads();                 // (also orders the weight staging before its first use)
#pragma unroll 1
      for (int j = 0; j < F3_ROWS; ++j) {
        const int oy = oy0 + j;
        if (oy >= oye) break;          // uniform over the workgroup
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) acc[i][jj] = 0.f;
        for (int r = 0; r < 3; ++r) {
#pragma unroll 2
          for (int ci = 0; ci < g.C; ++ci) {
            const float* row = tile + ((j + r) * g.C + ci) * F3_XP + slot * 4;
            const float4 a = *reinterpret_cast<const float4*>(row);
            const float2 b = *reinterpret_cast<const float2*>(row + 4);
            const float in[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
#pragma unroll
            for (int s = 0; s < 3; ++s) {
              const float4 wv = *reinterpret_cast<const float4*>(wl + ((r * 3 + s) * g.C + ci) * 64 + cl * 4);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                acc[i][0] = fmaf(in[i + s], wv.x, acc[i][0]);
                acc[i][1] = fmaf(in[i + s], wv.y, acc[i][1]);
                acc[i][2] = fmaf(in[i + s], wv.z, acc[i][2]);
                acc[i][3] = fmaf(in[i + s], wv.w, acc[i][3]);
              }
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ox = ox0 + slot * 4 + i;
          if (ox >= g.W) continue;
          float v[4];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            float t = acc[i][jj];
            if (EPI == 0) {
              t += e0[jj];
              if (relu) t = fmaxf(t, 0.f);
            } else if (EPI == 1) {
              s1[jj] += t;
              s2[jj] = fmaf(t, t, s2[jj]);
            } else {
              t = fmaxf(fmaf(t, e0[jj], e1[jj]), 0.f);
            }
            v[jj] = t;
          }
          *reinterpret_cast<float4*>(out + (((size_t)n * g.H + oy) * g.W + ox) * out_ld + cl * 4) =
              make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
  }
  if (EPI == 1) {
    __syncthreads();                   // the last tile has been read: its memory becomes red[16 slots][16 cl][8]
    float* red = tile;                 // 2048 floats: the launch sizes the tile region to at least that
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      red[(slot * 16 + cl) * 8 + jj] = s1[jj];
      red[(slot * 16 + cl) * 8 + 4 + jj] = s2[jj];
    }
    __syncthreads();
    if (threadIdx.x < 128) {           // (sum | sum of squares) x 64 channels, the 16 pixel slots in fixed order
      const int which = threadIdx.x >> 6, ch = threadIdx.x & 63;
      float s = 0.f;
#pragma unroll
      for (int pp = 0; pp < 16; ++pp) s += red[(pp * 16 + (ch >> 2)) * 8 + which * 4 + (ch & 3)];
      stat_partial[((size_t)blockIdx.x * 2 + which) * 64 + ch] = s;
    }
  }
}

// lane groups of the weight gradient: CS input-channel slots (the power of two >= C) x PS = 16 / CS pixel slots
__global__ __launch_bounds__(256) void conv3_first_wgrad_kernel(const float* __restrict__ dy, int dy_ld,
                                                                const float* __restrict__ x, F3Geom g, int cs_log2,
                                                                float* __restrict__ partial) {
  extern __shared__ float4 f3_lds4[];
  float* tile = reinterpret_cast<float*>(f3_lds4);          // [(F3_ROWS + 2) * C][F3_XP]
  float* red = tile + (F3_ROWS + 2) * g.C * F3_XP;          // [PS][64 * 9 * C]
  const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int CS = 1 << cs_log2, PS = 16 >> cs_log2;
  const int ci = grp & (CS - 1), ps = grp >> cs_log2;
  const bool live = ci < g.C;
  const int K = 9 * g.C;
  float acc[4][9];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[j][t] = 0.f;
  for (int sidx = blockIdx.x; sidx < g.strips; sidx += gridDim.x) {
    const int n = sidx / g.spf, strip = sidx - n * g.spf;
    const int oyb = strip * F3_STRIP;
    const int oye = min(oyb + F3_STRIP, g.H);
    for (int oy0 = oyb; oy0 < oye; oy0 += F3_ROWS) {
      for (int ox0 = 0; ox0 < g.W; ox0 += F3_XT) {
        __syncthreads();               // the previous tile has been read
        f3_stage(x, g, n, oy0, ox0, tile);
        __syncthreads();
        if (!live) continue;           // (the barriers above are reached by every thread in every iteration)
        // a pixel slot takes runs of 4 consecutive pixels of a row: their four dy loads are in flight together and the 6
        // input values of a filter row serve all 12 (pixel, column) pairs.  A pixel outside the map is skipped, not
        // multiplied by zero, so a non-finite frame value only reaches the taps that really touch it.
        for (int u = ps; u < F3_ROWS * (F3_XT / 4); u += PS) {
          const int j = u / (F3_XT / 4), xo = (u - j * (F3_XT / 4)) * 4;
          const int oy = oy0 + j, ox = ox0 + xo;
          if (oy >= oye || ox >= g.W) continue;
          const int nv = min(4, g.W - ox);
          const float* dp = dy + (((size_t)n * g.H + oy) * g.W + ox) * dy_ld + cl * 4;
          float4 d[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            d[i] = i < nv ? *reinterpret_cast<const float4*>(dp + (size_t)i * dy_ld) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const float* row = tile + ((j + r) * g.C + ci) * F3_XP + xo;
            const float4 a = *reinterpret_cast<const float4*>(row);
            const float2 b = *reinterpret_cast<const float2*>(row + 4);
            const float xin[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (i < nv) {
                const float dd[4] = {d[i].x, d[i].y, d[i].z, d[i].w};
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                  for (int jj = 0; jj < 4; ++jj) acc[jj][r * 3 + s] = fmaf(dd[jj], xin[i + s], acc[jj][r * 3 + s]);
              }
            }
          }
        }
      }
    }
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int t = 0; t < 9; ++t) red[(size_t)ps * 64 * K + (cl * 4 + jj) * K + t * g.C + ci] = acc[jj][t];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * K; i += 256) {
    float s = 0.f;
    for (int pp = 0; pp < PS; ++pp) s += red[(size_t)pp * 64 * K + i];
    partial[(size_t)blockIdx.x * 64 * K + i] = s;
  }
}

// dweight[i] = sum over the workgroups' partials in fp64: a block takes 64 elements, its 4 thread groups take the partial
// rows round robin and are combined through LDS -- every order is fixed
__global__ __launch_bounds__(256) void conv3_first_wgrad_sum_kernel(const float* __restrict__ partial, int nparts,
                                                                    int count, float* __restrict__ dweight) {
  __shared__ double red[4][64];
  const int e = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + e;
  double s = 0.0;
  if (i < count)
    for (int b = grp; b < nparts; b += 4) s += (double)partial[(size_t)b * count + i];
  red[grp][e] = s;
  __syncthreads();
  if (grp == 0 && i < count) dweight[i] = (float)((red[0][e] + red[1][e]) + (red[2][e] + red[3][e]));
}

static bool f3_geom(int n, int cin, int h, int w, F3Geom* g) {
  if (n < 1 || h < 1 || w < 1 || cin < 1 || cin > 16) return false;
  if ((size_t)n * h * w >= (1ull << 31) / 16) return false;          // n * cin * h * w and n * strips stay below 2^31
  g->N = n;
  g->C = cin;
  g->H = h;
  g->W = w;
  g->spf = cdiv(h, F3_STRIP);
  g->strips = n * g->spf;
  return true;
}

static size_t f3_tile_floats(int cin) { return (size_t)(F3_ROWS + 2) * cin * F3_XP; }

// ---------------------------------------------------------------------------------------------- MaxPool2d(2, 2)
// one thread per (output pixel, 4 channels); ties keep the first maximum in scan order and a NaN wins, as maxpool_fwd_kernel
__global__ __launch_bounds__(256) void maxpool2_fwd_kernel(const float* __restrict__ in, int in_ld, float* __restrict__ out,
                                                           int out_ld, uint8_t* __restrict__ argmax, int H, int W, int C,
                                                           int OH, int OW, uint32_t total) {
  const int G = C >> 2;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t opix = i / (uint32_t)G;
    const int gq = (int)(i - opix * (uint32_t)G);
    const uint32_t orow = opix / (uint32_t)OW;
    const int ox = (int)(opix - orow * (uint32_t)OW);
    const int n = (int)(orow / (uint32_t)OH), oy = (int)(orow - (uint32_t)n * (uint32_t)OH);
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    int bx = 0, by = 0, bz = 0, bw = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int iy = 2 * oy + (k >> 1), ix = 2 * ox + (k & 1);
      const float4 v = *reinterpret_cast<const float4*>(in + (((size_t)n * H + iy) * W + ix) * in_ld + gq * 4);
      if (v.x > best.x || v.x != v.x) { best.x = v.x; bx = k; }
      if (v.y > best.y || v.y != v.y) { best.y = v.y; by = k; }
      if (v.z > best.z || v.z != v.z) { best.z = v.z; bz = k; }
      if (v.w > best.w || v.w != v.w) { best.w = v.w; bw = k; }
    }
    *reinterpret_cast<float4*>(out + (size_t)opix * out_ld + gq * 4) = best;
    if (argmax != nullptr)
      *reinterpret_cast<uint32_t*>(argmax + (size_t)opix * C + gq * 4) =
          (uint32_t)bx | ((uint32_t)by << 8) | ((uint32_t)bz << 16) | ((uint32_t)bw << 24);
  }
}

// one thread per (INPUT pixel, 4 channels): every element of din is written -- dout where the element is its window's
// argmax (and, with z, where z > 0), zero elsewhere and in a dropped trailing row / column
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float* __restrict__ dout, int dout_ld,
                                                           const uint8_t* __restrict__ argmax,
                                                           const float* __restrict__ z, int z_ld, float* __restrict__ din,
                                                           int din_ld, int H, int W, int C, int OH, int OW, int accumulate,
                                                           uint32_t total) {
  const int G = C >> 2;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t pix = i / (uint32_t)G;
    const int gq = (int)(i - pix * (uint32_t)G);
    const uint32_t row = pix / (uint32_t)W;
    const int ix = (int)(pix - row * (uint32_t)W);
    const int n = (int)(row / (uint32_t)H), iy = (int)(row - (uint32_t)n * (uint32_t)H);
    const int oy = iy >> 1, ox = ix >> 1;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (oy < OH && ox < OW) {
      const size_t opix = ((size_t)n * OH + oy) * OW + ox;
      const uint32_t k = (uint32_t)((iy & 1) * 2 + (ix & 1));
      const uint32_t a = *reinterpret_cast<const uint32_t*>(argmax + opix * C + gq * 4);
      const float4 d = *reinterpret_cast<const float4*>(dout + opix * dout_ld + gq * 4);
      v.x = (a & 255u) == k ? d.x : 0.f;
      v.y = ((a >> 8) & 255u) == k ? d.y : 0.f;
      v.z = ((a >> 16) & 255u) == k ? d.z : 0.f;
      v.w = (a >> 24) == k ? d.w : 0.f;
    }
    if (z != nullptr) {
      const float4 zz = *reinterpret_cast<const float4*>(z + (size_t)pix * z_ld + gq * 4);
      v.x = zz.x > 0.f ? v.x : 0.f;
      v.y = zz.y > 0.f ? v.y : 0.f;
      v.z = zz.z > 0.f ? v.z : 0.f;
      v.w = zz.w > 0.f ? v.w : 0.f;
    }
    float4* dst = reinterpret_cast<float4*>(din + (size_t)pix * din_ld + gq * 4);
    if (accumulate) {
      const float4 o = *dst;
      v.x += o.x;
      v.y += o.y;
      v.z += o.z;
      v.w += o.w;
    }
    *dst = v;
  }
}

// ---------------------------------------------------------------------------------------------- AdaptiveAvgPool2d((7, 7))
// PyTorch's windows: bin i of an axis of length L covers [floor(i L / 7), ceil((i + 1) L / 7))
__device__ __forceinline__ int ap_start(int i, int L) { return (i * L) / 7; }
__device__ __forceinline__ int ap_end(int i, int L) { return ((i + 1) * L + 6) / 7; }

#define AP_CT 64                     // channels per workgroup: their 64 * 49 outputs are ONE contiguous run of a row of out

// a workgroup takes AP_CT channels of one frame: lanes run along the channels (coalesced NHWC reads), the 49 means of a
// channel go through LDS and leave as the contiguous run out[n][c0 * 49 .. (c0 + cw) * 49)
__global__ __launch_bounds__(256) void adaptive_avgpool7_fwd_kernel(const float* __restrict__ in, int in_ld,
                                                                    float* __restrict__ out, int H, int W, int C,
                                                                    int ctiles) {
  __shared__ float sm[AP_CT * 49];
  const int n = blockIdx.x / ctiles, c0 = (blockIdx.x - n * ctiles) * AP_CT;
  const int cw = min(AP_CT, C - c0);
  const int chl = threadIdx.x & 63, bg = threadIdx.x >> 6;
  if (chl < cw) {
    for (int b = bg; b < 49; b += 4) {
      const int oy = b / 7, ox = b - oy * 7;
      const int y0 = ap_start(oy, H), y1 = ap_end(oy, H), x0 = ap_start(ox, W), x1 = ap_end(ox, W);
      float s = 0.f;
      for (int y = y0; y < y1; ++y)
        for (int xx = x0; xx < x1; ++xx) s += in[(((size_t)n * H + y) * W + xx) * in_ld + c0 + chl];
      sm[chl * 49 + b] = s / (float)((y1 - y0) * (x1 - x0));
    }
  }
  __syncthreads();
  float* dst = out + ((size_t)n * C + c0) * 49;
  for (int i = threadIdx.x; i < cw * 49; i += 256) dst[i] = sm[i];
}

// the adjoint: dout[n][c0 * 49 ..) enters LDS as one contiguous run, already divided by its window's area; every input
// element then sums the bins whose window contains it (a contiguous range of bins per axis), in fp64, in fixed order
__global__ __launch_bounds__(256) void adaptive_avgpool7_bwd_kernel(const float* __restrict__ dout, float* __restrict__ din,
                                                                    int din_ld, int H, int W, int C, int ctiles,
                                                                    int accumulate) {
  __shared__ float sm[AP_CT * 49];
  const int n = blockIdx.x / ctiles, c0 = (blockIdx.x - n * ctiles) * AP_CT;
  const int cw = min(AP_CT, C - c0);
  const float* src = dout + ((size_t)n * C + c0) * 49;
  for (int i = threadIdx.x; i < cw * 49; i += 256) {
    const int b = i % 49;
    const int oy = b / 7, ox = b - oy * 7;
    const int area = (ap_end(oy, H) - ap_start(oy, H)) * (ap_end(ox, W) - ap_start(ox, W));
    sm[i] = src[i] / (float)area;
  }
  __syncthreads();
  const int chl = threadIdx.x & 63, pg = threadIdx.x >> 6;
  if (chl >= cw) return;
  for (int pix = pg; pix < H * W; pix += 4) {
    const int y = pix / W, xx = pix - y * W;
    int ylo = 7, yhi = -1, xlo = 7, xhi = -1;
#pragma unroll
    for (int b = 0; b < 7; ++b) {
      if (ap_start(b, H) <= y && y < ap_end(b, H)) { ylo = min(ylo, b); yhi = max(yhi, b); }
      if (ap_start(b, W) <= xx && xx < ap_end(b, W)) { xlo = min(xlo, b); xhi = max(xhi, b); }
    }
    double s = 0.0;
    for (int oy = ylo; oy <= yhi; ++oy)
      for (int ox = xlo; ox <= xhi; ++ox) s += (double)sm[chl * 49 + oy * 7 + ox];
    float* dst = din + (((size_t)n * H + y) * W + xx) * din_ld + c0 + chl;
    *dst = accumulate ? (float)((double)*dst + s) : (float)s;
  }
}

static bool pool_args(int n, int h, int w, int c) {
  return n >= 1 && h >= 1 && w >= 1 && c >= 4 && c % 4 == 0 && (size_t)n * h * w * (size_t)(c / 4) < (1ull << 31);
}

extern "C" {

int tbn_conv3_first_stat_rows(int n, int cin, int h, int w) {
  F3Geom g;
  return f3_geom(n, cin, h, w, &g) ? g.strips : 0;
}

int tbn_conv3_first_fwd(const float* x, const float* weight, const float* bias, float* out, int out_ld, int n, int h, int w,
                        int cin, int cout, int epilogue, int flags, const float* scale, const float* shift,
                        float* stat_partial, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  F3Geom g;
  TBN_REQUIRE(x && weight && out, "conv3_first_fwd: null pointer");
  TBN_REQUIRE(cin >= 1 && cin <= 16, "conv3_first_fwd: cin must be in 1..16 (got %d)", cin);
  TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, cout == 64, "conv3_first_fwd: cout must be 64 (got %d)", cout);
  TBN_REQUIRE(f3_geom(n, cin, h, w, &g), "conv3_first_fwd: n, h, w must be >= 1 with n * h * w < 2^27 (got %d, %d, %d)", n,
              h, w);
  TBN_REQUIRE(out_ld >= 64 && out_ld % 4 == 0, "conv3_first_fwd: out_ld must be a multiple of 4 and >= 64 (got %d)",
              out_ld);
  TBN_REQUIRE(((uintptr_t)out & 15) == 0, "conv3_first_fwd: out must be 16-B aligned");
  TBN_REQUIRE((size_t)n * h * w * (size_t)out_ld < (1ull << 40), "conv3_first_fwd: output too large");
  TBN_REQUIRE(epilogue >= 0 && epilogue <= 2, "conv3_first_fwd: epilogue must be 0, 1 or 2 (got %d)", epilogue);
  TBN_REQUIRE((flags & ~2) == 0 && (epilogue == 0 || flags == 0),
              "conv3_first_fwd: flags takes 2 (ReLU) with epilogue 0 only (got %d)", flags);
  TBN_REQUIRE(epilogue != 1 || stat_partial, "conv3_first_fwd: epilogue 1 needs stat_partial");
  TBN_REQUIRE(epilogue != 2 || (scale && shift), "conv3_first_fwd: epilogue 2 needs scale and shift");
  const dim3 grid(g.strips);
  // weights + staged rows; the statistics combine of epilogue 1 reuses the staged rows and needs 2048 floats of them
  size_t tile = f3_tile_floats(cin);
  if (tile < 2048) tile = 2048;
  const size_t lds = ((size_t)9 * cin * 64 + tile) * sizeof(float);
  if (epilogue == 0) {
    TBN_KLAUNCH(conv3_first_fwd_kernel<0>, grid, dim3(256), lds, st, x, weight, bias, out, out_ld, g, (flags & 2) ? 1 : 0,
                scale, shift, stat_partial);
  } else if (epilogue == 1) {
    TBN_KLAUNCH(conv3_first_fwd_kernel<1>, grid, dim3(256), lds, st, x, weight, bias, out, out_ld, g, 0, scale, shift,
                stat_partial);
  } else {
    TBN_KLAUNCH(conv3_first_fwd_kernel<2>, grid, dim3(256), lds, st, x, weight, bias, out, out_ld, g, 0, scale, shift,
                stat_partial);
  }
  TBN_CHECK_LAUNCH("conv3_first_fwd");
  return TBN_OK;
}

static int f3_wgrad_wgs(const F3Geom& g) { return g.strips < F3_WGRAD_MAX_WG ? g.strips : F3_WGRAD_MAX_WG; }

size_t tbn_conv3_first_wgrad_workspace_floats(int n, int cin, int h, int w) {
  F3Geom g;
  return f3_geom(n, cin, h, w, &g) ? (size_t)f3_wgrad_wgs(g) * 64 * 9 * cin : 0;
}

int tbn_conv3_first_wgrad(const float* dy, int dy_ld, const float* x, float* dweight, int n, int h, int w, int cin, int cout,
                          float* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  F3Geom g;
  TBN_REQUIRE(dy && x && dweight && workspace, "conv3_first_wgrad: null pointer");
  TBN_REQUIRE(cin >= 1 && cin <= 16, "conv3_first_wgrad: cin must be in 1..16 (got %d)", cin);
  TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, cout == 64, "conv3_first_wgrad: cout must be 64 (got %d)", cout);
  TBN_REQUIRE(f3_geom(n, cin, h, w, &g), "conv3_first_wgrad: n, h, w must be >= 1 with n * h * w < 2^27 (got %d, %d, %d)",
              n, h, w);
  TBN_REQUIRE(dy_ld >= 64 && dy_ld % 4 == 0, "conv3_first_wgrad: dy_ld must be a multiple of 4 and >= 64 (got %d)", dy_ld);
  TBN_REQUIRE(((uintptr_t)dy & 15) == 0, "conv3_first_wgrad: dy must be 16-B aligned");
  TBN_REQUIRE((size_t)n * h * w * (size_t)dy_ld < (1ull << 40), "conv3_first_wgrad: dy too large");
  int cs_log2 = 0;
  while ((1 << cs_log2) < cin) ++cs_log2;
  const int wgs = f3_wgrad_wgs(g);
  const int count = 64 * 9 * cin;
  const size_t lds = (f3_tile_floats(cin) + (size_t)(16 >> cs_log2) * count) * sizeof(float);
  TBN_KLAUNCH(conv3_first_wgrad_kernel, dim3(wgs), dim3(256), lds, st, dy, dy_ld, x, g, cs_log2, workspace);
  TBN_CHECK_LAUNCH("conv3_first_wgrad");
  TBN_KLAUNCH(conv3_first_wgrad_sum_kernel, dim3(cdiv(count, 64)), dim3(256), 0, st, (const float*)workspace, wgs, count,
              dweight);
  TBN_CHECK_LAUNCH("conv3_first_wgrad_sum");
  return TBN_OK;
}

int tbn_maxpool2_fwd(const float* in, int in_ld, float* out, int out_ld, uint8_t* argmax, int n, int h, int w, int c,
                     void* stream) {
  TBN_REQUIRE(in && out, "maxpool2_fwd: null pointer");
  TBN_REQUIRE(pool_args(n, h, w, c), "maxpool2_fwd: n, h, w >= 1, c a multiple of 4, n * h * w * c / 4 < 2^31 (got %d, %d, "
              "%d, %d)", n, h, w, c);
  TBN_REQUIRE(h >= 2 && w >= 2, "maxpool2_fwd: a 2x2 / stride 2 window needs h, w >= 2 (got %d, %d)", h, w);
  TBN_REQUIRE(in_ld >= c && in_ld % 4 == 0 && out_ld >= c && out_ld % 4 == 0,
              "maxpool2_fwd: pitches must be multiples of 4 and >= c (got %d, %d for c = %d)", in_ld, out_ld, c);
  TBN_REQUIRE((((uintptr_t)in | (uintptr_t)out) & 15) == 0 && ((uintptr_t)argmax & 3) == 0,
              "maxpool2_fwd: in / out must be 16-B aligned, argmax 4-B aligned");
  const int oh = h / 2, ow = w / 2;
  const size_t total = (size_t)n * oh * ow * (c / 4);
  TBN_KLAUNCH(maxpool2_fwd_kernel, dim3(ew_grid(total, 8192)), dim3(256), 0, (hipStream_t)stream, in, in_ld, out, out_ld,
              argmax, h, w, c, oh, ow, (uint32_t)total);
  TBN_CHECK_LAUNCH("maxpool2_fwd");
  return TBN_OK;
}

int tbn_maxpool2_bwd(const float* dout, int dout_ld, const uint8_t* argmax, const float* z, int z_ld, float* din, int din_ld,
                     int n, int h, int w, int c, int accumulate, void* stream) {
  TBN_REQUIRE(dout && argmax && din, "maxpool2_bwd: null pointer");
  TBN_REQUIRE(pool_args(n, h, w, c), "maxpool2_bwd: n, h, w >= 1, c a multiple of 4, n * h * w * c / 4 < 2^31 (got %d, %d, "
              "%d, %d)", n, h, w, c);
  TBN_REQUIRE(h >= 2 && w >= 2, "maxpool2_bwd: a 2x2 / stride 2 window needs h, w >= 2 (got %d, %d)", h, w);
  TBN_REQUIRE(dout_ld >= c && dout_ld % 4 == 0 && din_ld >= c && din_ld % 4 == 0,
              "maxpool2_bwd: pitches must be multiples of 4 and >= c (got %d, %d for c = %d)", dout_ld, din_ld, c);
  TBN_REQUIRE(z == nullptr || (z_ld >= c && z_ld % 4 == 0), "maxpool2_bwd: z_ld must be a multiple of 4 and >= c (got %d)",
              z_ld);
  TBN_REQUIRE((((uintptr_t)dout | (uintptr_t)din | (uintptr_t)z) & 15) == 0 && ((uintptr_t)argmax & 3) == 0,
              "maxpool2_bwd: dout / din / z must be 16-B aligned, argmax 4-B aligned");
  const size_t total = (size_t)n * h * w * (c / 4);
  TBN_KLAUNCH(maxpool2_bwd_kernel, dim3(ew_grid(total, 8192)), dim3(256), 0, (hipStream_t)stream, dout, dout_ld, argmax, z,
              z_ld, din, din_ld, h, w, c, h / 2, w / 2, accumulate ? 1 : 0, (uint32_t)total);
  TBN_CHECK_LAUNCH("maxpool2_bwd");
  return TBN_OK;
}

int tbn_adaptive_avgpool7_fwd(const float* in, int in_ld, float* out, int n, int h, int w, int c, void* stream) {
  TBN_REQUIRE(in && out, "adaptive_avgpool7_fwd: null pointer");
  TBN_REQUIRE(pool_args(n, h, w, c), "adaptive_avgpool7_fwd: n, h, w >= 1, c a multiple of 4, n * h * w * c / 4 < 2^31 (got "
              "%d, %d, %d, %d)", n, h, w, c);
  TBN_REQUIRE(h < (1 << 20) && w < (1 << 20), "adaptive_avgpool7_fwd: h, w must be below 2^20 (got %d, %d)", h, w);
  TBN_REQUIRE(in_ld >= c && in_ld % 4 == 0, "adaptive_avgpool7_fwd: in_ld must be a multiple of 4 and >= c (got %d)", in_ld);
  const int ctiles = cdiv(c, AP_CT);
  TBN_REQUIRE((size_t)n * ctiles < (1ull << 31), "adaptive_avgpool7_fwd: too many workgroups");
  TBN_KLAUNCH(adaptive_avgpool7_fwd_kernel, dim3(n * ctiles), dim3(256), 0, (hipStream_t)stream, in, in_ld, out, h, w, c,
              ctiles);
  TBN_CHECK_LAUNCH("adaptive_avgpool7_fwd");
  return TBN_OK;
}

int tbn_adaptive_avgpool7_bwd(const float* dout, float* din, int din_ld, int n, int h, int w, int c, int accumulate,
                              void* stream) {
  TBN_REQUIRE(dout && din, "adaptive_avgpool7_bwd: null pointer");
  TBN_REQUIRE(pool_args(n, h, w, c), "adaptive_avgpool7_bwd: n, h, w >= 1, c a multiple of 4, n * h * w * c / 4 < 2^31 (got "
              "%d, %d, %d, %d)", n, h, w, c);
  TBN_REQUIRE(h < (1 << 20) && w < (1 << 20), "adaptive_avgpool7_bwd: h, w must be below 2^20 (got %d, %d)", h, w);
  TBN_REQUIRE(din_ld >= c && din_ld % 4 == 0, "adaptive_avgpool7_bwd: din_ld must be a multiple of 4 and >= c (got %d)",
              din_ld);
  const int ctiles = cdiv(c, AP_CT);
  TBN_REQUIRE((size_t)n * ctiles < (1ull << 31), "adaptive_avgpool7_bwd: too many workgroups");
  TBN_KLAUNCH(adaptive_avgpool7_bwd_kernel, dim3(n * ctiles), dim3(256), 0, (hipStream_t)stream, dout, din, din_ld, h, w, c,
              ctiles, accumulate ? 1 : 0);
  TBN_CHECK_LAUNCH("adaptive_avgpool7_bwd");
  return TBN_OK;
}

}  // extern "C"
