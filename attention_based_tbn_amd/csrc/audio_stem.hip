// The separable audio stem of BNInception_Audio (include/tbn_hip.h: tbn_audio_stem_*), fp32, NCHW spectrogram in, NHWC out.
//
// Reference ops (core/models/bn_inception_audio.py:11-20, 408-416): conv1_1x3_s2 = Conv2d(1, 32, (3, 1), stride 2, padding
// (1, 0)) -- three taps along frequency -- and conv1_3x1_s2 = Conv2d(1, 32, (1, 3), stride 2, padding (0, 1)) -- three taps
// along time -- on the same one-channel input, concatenated to 64 channels.
//
// 6 multiply-adds per output value and 256 B written per output pixel for ~16 B read: a streaming kernel, not a GEMM (no
// MFMA).  A workgroup takes AS_STRIP consecutive output rows of the flattened (frame, row) axis -- a strip may cross a frame
// boundary, every row finds its own frame -- and walks them in chunks of AS_XT output pixels: the three input rows of each
// output row are staged in LDS with coalesced row loads (reads outside the image become zeros THERE, so every global read
// is bounds-checked in one place), then a lane owns 4 consecutive channels of a pixel and the 16 lanes of a pixel move its
// 256 B as one contiguous run (a wave: 4 consecutive pixels, 1 KB).  All 16 lanes of a pixel read the same LDS words
// (broadcast), the two branches differ only in WHICH three words, picked by index -- no divergence.  Plain fp32 FMAs in tap
// order 0, 1, 2: reproducible.
// The weight gradient walks the same tiles, reads dy exactly once with the same lane mapping, keeps 4 channels x 3 taps per
// lane in registers, combines the 16 pixel lanes through LDS in fixed order and writes ONE [64][3] partial per workgroup; a
// second launch sums the workgroups in fixed order in fp64 (the convention of tbn_sum_partials).  No atomics.
#include "tbn_common.h"
#include "tbn_hip.h"

#define AS_STRIP 4                   // output rows per tile
#define AS_XT 64                     // output pixels of a row per tile
#define AS_XW (2 * AS_XT + 1)        // staged input columns 2 ox0 - 1 .. 2 (ox0 + AS_XT - 1) + 1
#define AS_XP 132                    // LDS pitch of a staged row
#define AS_WGRAD_MAX_WG 1024         // workgroups (= partials) of the weight gradient

struct AsGeom {
  int N, H, W, OH, OW;
  int rows;                          // N * OH
};

// stages input rows 2 oy - 1 .. 2 oy + 1 of the AS_STRIP output rows from r0 on, columns 2 ox0 - 1 + (0 .. AS_XW - 1)
__device__ __forceinline__ void as_stage(const float* __restrict__ x, const AsGeom& g, int r0, int ox0,
                                         float (*tile)[AS_XP]) {
  for (int i = threadIdx.x; i < AS_STRIP * 3 * AS_XP; i += 256) {
    const int lr = i / AS_XP, cx = i - lr * AS_XP;
    const int j = lr / 3, t = lr - j * 3;
    const int r = r0 + j;
    float v = 0.f;
    if (r < g.rows && cx < AS_XW) {
      const int n = r / g.OH, oy = r - n * g.OH;
      const int iy = 2 * oy - 1 + t, ix = 2 * ox0 - 1 + cx;
      if ((unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W) v = x[((size_t)n * g.H + iy) * g.W + ix];
    }
    tile[lr][cx] = v;
  }
}

// the three input values of pixel (row j of the tile, xo) for this lane's branch: frequency taps (same column, three rows)
// for channels < 32, time taps (middle row, three columns) for channels >= 32
__device__ __forceinline__ void as_taps(float (*tile)[AS_XP], int j, int xo, bool time_branch, float& a, float& b,
                                        float& c) {
  const int col = 2 * xo + 1;
  a = time_branch ? tile[3 * j + 1][col - 1] : tile[3 * j][col];
  b = tile[3 * j + 1][col];
  c = time_branch ? tile[3 * j + 1][col + 1] : tile[3 * j + 2][col];
}

template <int EPI>   // 0: + bias (RELU by flag), 1: raw + statistics partial row per workgroup, 2: relu(acc * scale + shift)
__global__ __launch_bounds__(256) void audio_stem_fwd_kernel(const float* __restrict__ x, const float* __restrict__ weight,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             int out_ld, AsGeom g, int relu,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift,
                                                             float* __restrict__ stat_partial) {
  __shared__ float tile[AS_STRIP * 3][AS_XP];
  __shared__ float red[EPI == 1 ? 16 : 1][16][8];
  const int cl = threadIdx.x & 15, p = threadIdx.x >> 4;
  const bool tb = cl >= 8;
  float wt[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < 3; ++t) wt[j][t] = weight[(cl * 4 + j) * 3 + t];
  float e0[4], e1[4];     // epilogue 0: bias | 0;  epilogue 2: scale | shift
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    e0[j] = EPI == 0 ? (bias != nullptr ? bias[cl * 4 + j] : 0.f) : (EPI == 2 ? scale[cl * 4 + j] : 0.f);
    e1[j] = EPI == 2 ? shift[cl * 4 + j] : 0.f;
  }
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  const int r0 = blockIdx.x * AS_STRIP;
  for (int ox0 = 0; ox0 < g.OW; ox0 += AS_XT) {
    if (ox0 > 0) __syncthreads();      // the previous tile has been read
    as_stage(x, g, r0, ox0, tile);
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < AS_STRIP * AS_XT / 16; ++k) {
      const int q = k * 16 + p;
      const int j = q / AS_XT, xo = q - j * AS_XT;
      const int r = r0 + j, ox = ox0 + xo;
      if (r >= g.rows || ox >= g.OW) continue;
      float a, b, c;
      as_taps(tile, j, xo, tb, a, b, c);
      float v[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        float acc = wt[jj][0] * a;
        acc = fmaf(wt[jj][1], b, acc);
        acc = fmaf(wt[jj][2], c, acc);
        if (EPI == 0) {
          acc += e0[jj];
          if (relu) acc = fmaxf(acc, 0.f);
        } else if (EPI == 1) {
          s1[jj] += acc;
          s2[jj] = fmaf(acc, acc, s2[jj]);
        } else {
          acc = fmaxf(fmaf(acc, e0[jj], e1[jj]), 0.f);
        }
        v[jj] = acc;
      }
      *reinterpret_cast<float4*>(out + ((size_t)r * g.OW + ox) * out_ld + cl * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  if (EPI == 1) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      red[p][cl][jj] = s1[jj];
      red[p][cl][4 + jj] = s2[jj];
    }
    __syncthreads();
    if (threadIdx.x < 128) {           // (sum | sum of squares) x 64 channels, the 16 pixel lanes in fixed order
      const int which = threadIdx.x >> 6, ch = threadIdx.x & 63;
      float s = 0.f;
#pragma unroll
      for (int pp = 0; pp < 16; ++pp) s += red[pp][ch >> 2][which * 4 + (ch & 3)];
      stat_partial[((size_t)blockIdx.x * 2 + which) * 64 + ch] = s;
    }
  }
}

__global__ __launch_bounds__(256) void audio_stem_wgrad_kernel(const float* __restrict__ dy, int dy_ld,
                                                               const float* __restrict__ x, AsGeom g, int strips,
                                                               float* __restrict__ partial) {
  __shared__ float tile[AS_STRIP * 3][AS_XP];
  __shared__ float red[16][192];
  const int cl = threadIdx.x & 15, p = threadIdx.x >> 4;
  const bool tb = cl >= 8;
  float acc[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[j][t] = 0.f;
  for (int strip = blockIdx.x; strip < strips; strip += gridDim.x) {
    const int r0 = strip * AS_STRIP;
    for (int ox0 = 0; ox0 < g.OW; ox0 += AS_XT) {
      __syncthreads();                 // the previous tile has been read
      as_stage(x, g, r0, ox0, tile);
      __syncthreads();
#pragma unroll 4
      for (int k = 0; k < AS_STRIP * AS_XT / 16; ++k) {
        const int q = k * 16 + p;
        const int j = q / AS_XT, xo = q - j * AS_XT;
        const int r = r0 + j, ox = ox0 + xo;
        if (r >= g.rows || ox >= g.OW) continue;
        const float4 d = *reinterpret_cast<const float4*>(dy + ((size_t)r * g.OW + ox) * dy_ld + cl * 4);
        float xt[3];
        as_taps(tile, j, xo, tb, xt[0], xt[1], xt[2]);
        const float dd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
          for (int t = 0; t < 3; ++t) acc[jj][t] = fmaf(dd[jj], xt[t], acc[jj][t]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < 3; ++t) red[p][(cl * 4 + j) * 3 + t] = acc[j][t];
  __syncthreads();
  if (threadIdx.x < 192) {
    float s = 0.f;
#pragma unroll
    for (int pp = 0; pp < 16; ++pp) s += red[pp][threadIdx.x];
    partial[(size_t)blockIdx.x * 192 + threadIdx.x] = s;
  }
}

// dweight[i] = sum over the workgroups' partials in fp64: AS_SUM_GROUPS thread groups take the partial rows round robin, each
// in four interleaved chains, and are combined through LDS -- every order is fixed.  (One group of 192 threads walking 1024
// rows alone took 0.070 ms beside 0.099 ms for the partial kernel at 96 x 256 x 256: a latency chain, not bandwidth.)
#define AS_SUM_GROUPS 4
__global__ __launch_bounds__(192 * AS_SUM_GROUPS) void audio_stem_wgrad_sum_kernel(const float* __restrict__ partial,
                                                                                   int nparts,
                                                                                   float* __restrict__ dweight) {
  __shared__ double red[AS_SUM_GROUPS][192];
  constexpr int G = AS_SUM_GROUPS;
  static_assert(G == 4, "the final combine below is written for four groups");
  const int i = threadIdx.x % 192, grp = threadIdx.x / 192;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int b = grp;
  for (; b + 3 * G < nparts; b += 4 * G) {
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] += (double)partial[(size_t)(b + u * G) * 192 + i];
  }
  for (int u = 0; b < nparts; b += G, ++u) s[u] += (double)partial[(size_t)b * 192 + i];
  red[grp][i] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  if (grp == 0) dweight[i] = (float)((red[0][i] + red[1][i]) + (red[2][i] + red[3][i]));
}

static bool as_geom(int n, int h, int w, AsGeom* g) {
  if (n < 1 || h < 1 || w < 1 || (size_t)n * h * w >= (1ull << 31)) return false;
  g->N = n;
  g->H = h;
  g->W = w;
  g->OH = (h - 1) / 2 + 1;
  g->OW = (w - 1) / 2 + 1;
  g->rows = n * g->OH;
  return true;
}

extern "C" {

int tbn_audio_stem_stat_rows(int n, int h, int w) {
  AsGeom g;
  return as_geom(n, h, w, &g) ? cdiv(g.rows, AS_STRIP) : 0;
}

int tbn_audio_stem_fwd(const float* x, const float* weight, const float* bias, float* out, int out_ld, int n, int h, int w,
                       int epilogue, int flags, const float* scale, const float* shift, float* stat_partial, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  AsGeom g;
  TBN_REQUIRE(x && weight && out, "audio_stem_fwd: null pointer");
  TBN_REQUIRE(as_geom(n, h, w, &g), "audio_stem_fwd: n, h, w must be >= 1 with n * h * w < 2^31 (got %d, %d, %d)", n, h, w);
  TBN_REQUIRE(out_ld >= 64 && out_ld % 4 == 0, "audio_stem_fwd: out_ld must be a multiple of 4 and >= 64 (got %d)", out_ld);
  TBN_REQUIRE(((uintptr_t)out & 15) == 0, "audio_stem_fwd: out must be 16-B aligned");
  TBN_REQUIRE((size_t)g.rows * g.OW * (size_t)out_ld < (1ull << 40), "audio_stem_fwd: output too large");
  TBN_REQUIRE(epilogue >= 0 && epilogue <= 2, "audio_stem_fwd: epilogue must be 0, 1 or 2 (got %d)", epilogue);
  TBN_REQUIRE((flags & ~2) == 0 && (epilogue == 0 || flags == 0),
              "audio_stem_fwd: flags takes 2 (ReLU) with epilogue 0 only (got %d)", flags);
  TBN_REQUIRE(epilogue != 1 || stat_partial, "audio_stem_fwd: epilogue 1 needs stat_partial");
  TBN_REQUIRE(epilogue != 2 || (scale && shift), "audio_stem_fwd: epilogue 2 needs scale and shift");
  const dim3 grid(cdiv(g.rows, AS_STRIP));
  if (epilogue == 0) {
    TBN_KLAUNCH(audio_stem_fwd_kernel<0>, grid, dim3(256), 0, st, x, weight, bias, out, out_ld, g, (flags & 2) ? 1 : 0,
                scale, shift, stat_partial);
  } else if (epilogue == 1) {
    TBN_KLAUNCH(audio_stem_fwd_kernel<1>, grid, dim3(256), 0, st, x, weight, bias, out, out_ld, g, 0, scale, shift,
                stat_partial);
  } else {
    TBN_KLAUNCH(audio_stem_fwd_kernel<2>, grid, dim3(256), 0, st, x, weight, bias, out, out_ld, g, 0, scale, shift,
                stat_partial);
  }
  TBN_CHECK_LAUNCH("audio_stem_fwd");
  return TBN_OK;
}

static int as_wgrad_wgs(const AsGeom& g) {
  const int strips = cdiv(g.rows, AS_STRIP);
  return strips < AS_WGRAD_MAX_WG ? strips : AS_WGRAD_MAX_WG;
}

size_t tbn_audio_stem_wgrad_workspace_floats(int n, int h, int w) {
  AsGeom g;
  return as_geom(n, h, w, &g) ? (size_t)as_wgrad_wgs(g) * 192 : 0;
}

int tbn_audio_stem_wgrad(const float* dy, int dy_ld, const float* x, float* dweight, int n, int h, int w, float* workspace,
                         void* stream) {
  hipStream_t st = (hipStream_t)stream;
  AsGeom g;
  TBN_REQUIRE(dy && x && dweight && workspace, "audio_stem_wgrad: null pointer");
  TBN_REQUIRE(as_geom(n, h, w, &g), "audio_stem_wgrad: n, h, w must be >= 1 with n * h * w < 2^31 (got %d, %d, %d)", n, h,
              w);
  TBN_REQUIRE(dy_ld >= 64 && dy_ld % 4 == 0, "audio_stem_wgrad: dy_ld must be a multiple of 4 and >= 64 (got %d)", dy_ld);
  TBN_REQUIRE(((uintptr_t)dy & 15) == 0, "audio_stem_wgrad: dy must be 16-B aligned");
  TBN_REQUIRE((size_t)g.rows * g.OW * (size_t)dy_ld < (1ull << 40), "audio_stem_wgrad: dy too large");
  const int wgs = as_wgrad_wgs(g);
  TBN_KLAUNCH(audio_stem_wgrad_kernel, dim3(wgs), dim3(256), 0, st, dy, dy_ld, x, g, cdiv(g.rows, AS_STRIP), workspace);
  TBN_CHECK_LAUNCH("audio_stem_wgrad");
  TBN_KLAUNCH(audio_stem_wgrad_sum_kernel, dim3(1), dim3(192 * AS_SUM_GROUPS), 0, st, (const float*)workspace, wgs,
              dweight);
  TBN_CHECK_LAUNCH("audio_stem_wgrad_sum");
  return TBN_OK;
}

}  // extern "C"
