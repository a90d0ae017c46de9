// BatchNorm2d with an optional residual and an optional ReLU -- the join of a residual block -- for NHWC fp32
// activations on gfx950: HBM-bound streaming kernels.
//
// Reference semantics: torchvision's BasicBlock / Bottleneck end in  out = relu(bn(conv(x)) + identity)  and their
// downsample path is bn(conv1x1(x)) without a ReLU (the reference reaches them through core/models/resnet.py:15-24).
// The BN kernels of bn.hip / bn_multi.hip hard-wire z = relu(y*scale+shift) and recompute the ReLU mask from
// y*scale+shift > 0 in the backward pass, which is wrong once a residual is added; they also stop at 1024 channels and
// ResNet-50/101/152 join at 2048.
//
// Same conventions as bn.hip: p rows x c channels, every tensor with its own pitch (multiples of 4 floats, 16-B aligned
// pointers), each lane owns 4 fixed channels and moves float4, per-workgroup partials are summed in a fixed order in
// fp64 by a finalize step (deterministic).  The backward mask comes from the forward's STORED output z (z > 0), so it is
// bit-consistent with the forward by construction whatever was added before the ReLU.
//
// Bytes per element (fp32): forward apply 8 (y -> z) + 4 with a residual; backward reduce 8 (dz, y) + 4 with a ReLU (z);
// backward apply 12 (dz, y -> dy) + 4 with a ReLU (z) + 4 with a residual (dres; 8 when it accumulates).
#include "tbn_common.h"
#include "tbn_kernels.h"
#include "tbn_bn_dev.h"
#include "../../include/tbn_hip.h"

namespace {

constexpr int kSlice = 1024;   // channels per workgroup of the reduce: red[] below holds 2 x 2048 floats as in bn.hip

// rows per reduce workgroup: NOT tbn_bn_reduce_chunk -- not rounded to the row lanes, whose count differs between column
// slices of unequal width, so that all slices write the same partial rows
inline int res_chunk(int P) {
  const int pch = cdiv(P, 512);
  return pch < 64 ? 64 : pch;
}
inline int res_parts(int P) { return cdiv(P, res_chunk(P)); }
// column slices of at most kSlice channels, balanced in float4 quads
inline int res_slices(int C) { return cdiv(C, kSlice); }
inline int res_slice_width(int C) { return cdiv(C / 4, res_slices(C)) * 4; }

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// ---------------------------------------------------------------- finalize: partials (pitch pld) -> mean/rstd/scale/shift
__global__ __launch_bounds__(256) void bn_res_finalize_kernel(const float* __restrict__ partial, int pld, int nparts,
                                                              int P, int C, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* running_mean,
                                                              float* running_var, float momentum, float eps,
                                                              float* save_mean, float* save_rstd, float* scale,
                                                              float* shift) {
  __shared__ double red[64 * 32];
  const int tid = threadIdx.x;
  const int c = blockIdx.x * TBN_FIN_CH + tid;
  double s1, s2;
  tbn_sum_partials<TBN_FIN_CH>(partial, pld, nparts, blockIdx.x * TBN_FIN_CH, C, red, &s1, &s2);
  if (tid < TBN_FIN_CH && c < C)
    TBN_BN_FWD_FINALIZE(gamma, beta, (const float*)nullptr, running_mean, running_var, momentum, eps, save_mean,
                        save_rstd, scale, shift);
}

// ---------------------------------------------------------------- apply: z = act(y*scale + shift + res)
// z may be y itself (a lane reads its quad before it writes it): no __restrict__ on them
template <bool RES, bool RELU>
__global__ __launch_bounds__(256) void bn_res_apply_kernel(const float* y, int y_ld, int P, int C,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const float* res,
                                                           int res_ld, float* z, int z_ld, FastDiv divg) {
  const int G = C >> 2;
  const uint32_t total = (uint32_t)P * G;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t p = fdiv(i, divg);
    const int c = (int)(i - p * (uint32_t)G) * 4;
    const float4 v = tbn_ld4<(TBN_BN_NT & 1) != 0>(y + (size_t)p * y_ld + c);
    const float4 sc = *reinterpret_cast<const float4*>(scale + c);
    const float4 sh = *reinterpret_cast<const float4*>(shift + c);
    float4 o;
    o.x = fmaf(v.x, sc.x, sh.x);
    o.y = fmaf(v.y, sc.y, sh.y);
    o.z = fmaf(v.z, sc.z, sh.z);
    o.w = fmaf(v.w, sc.w, sh.w);
    if (RES) {
      const float4 r = *reinterpret_cast<const float4*>(res + (size_t)p * res_ld + c);
      o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
    }
    if (RELU) {
      o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
    }
    *reinterpret_cast<float4*>(z + (size_t)p * z_ld + c) = o;
  }
}

// ---------------------------------------------------------------- backward
// g = RELU ? (z > 0 ? dz : 0) : dz;  xhat = (y-mean)*rstd;  S1 = sum g, S2 = sum g*xhat over the rows of chunk
// blockIdx.x, for the channels of column slice blockIdx.y (at most 1024: the LDS of bn.hip's reduce, not more)
template <bool RELU>
__global__ __launch_bounds__(256) void bn_res_bwd_reduce_kernel(const float* __restrict__ dz, int dz_ld,
                                                                const float* __restrict__ z, int z_ld,
                                                                const float* __restrict__ y, int y_ld, int P, int C,
                                                                int cs, int pch, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd,
                                                                float* __restrict__ partial) {
  __shared__ float red[2 * 2048];
  const int c0 = blockIdx.y * cs, Cs = min(cs, C - c0);
  const int G = Cs >> 2, RP = 256 / G;
  const int tid = threadIdx.x, cg = tid % G, rs = tid / G, c = c0 + cg * 4;
  const int p0 = blockIdx.x * pch, p1 = min(P, p0 + pch);
  if (rs < RP) {
    float4 s1 = make_float4(0, 0, 0, 0), s2 = s1;
    const float4 mu = *reinterpret_cast<const float4*>(mean + c);
    const float4 rs4 = *reinterpret_cast<const float4*>(rstd + c);
    for (int p = p0 + rs; p < p1; p += RP) {
      const float4 v = *reinterpret_cast<const float4*>(y + (size_t)p * y_ld + c);
      float4 g = *reinterpret_cast<const float4*>(dz + (size_t)p * dz_ld + c);
      if (RELU) g = tbn_pos_gate4(*reinterpret_cast<const float4*>(z + (size_t)p * z_ld + c), g);
      tbn_bn_sums4(s1, s2, g, v, mu, rs4);
    }
    tbn_bn_red_put(red, rs, G, cg, s1, s2);
  }
  __syncthreads();
  TBN_BN_RED_FOLD(red, RP, Cs, partial, blockIdx.x, C, c0)
}

// dy = a*g + b*y + cst (coef rows a | b | cst of bn_bwd_finalize_kernel);  dres (+)= g.
// dy may be y itself, and dres may be dz itself (each lane reads its quad before it writes it): no __restrict__ on them
template <bool RELU, bool DRES, bool ACC>
__global__ __launch_bounds__(256) void bn_res_bwd_apply_kernel(const float* dz, int dz_ld, const float* z, int z_ld,
                                                               const float* y, int y_ld, int P, int C,
                                                               const float* __restrict__ coef, float* dy, int dy_ld,
                                                               float* dres, int dres_ld, FastDiv divg) {
  const int G = C >> 2;
  const uint32_t total = (uint32_t)P * G;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t p = fdiv(i, divg);
    const int c = (int)(i - p * (uint32_t)G) * 4;
    float4 g = tbn_ld4<(TBN_BN_NT & 2) != 0>(dz + (size_t)p * dz_ld + c);
    const float4 v = tbn_ld4<(TBN_BN_NT & 2) != 0>(y + (size_t)p * y_ld + c);
    if (RELU) g = tbn_pos_gate4(tbn_ld4<(TBN_BN_NT & 2) != 0>(z + (size_t)p * z_ld + c), g);
    const float4 ca = *reinterpret_cast<const float4*>(coef + c);
    const float4 cb = *reinterpret_cast<const float4*>(coef + C + c);
    const float4 cc = *reinterpret_cast<const float4*>(coef + 2 * C + c);
    if (DRES) {
      float* dr = dres + (size_t)p * dres_ld + c;
      float4 r = g;
      if (ACC) {
        const float4 old = *reinterpret_cast<const float4*>(dr);
        r.x += old.x; r.y += old.y; r.z += old.z; r.w += old.w;
      }
      *reinterpret_cast<float4*>(dr) = r;
    }
    *reinterpret_cast<float4*>(dy + (size_t)p * dy_ld + c) = tbn_bn_dy4(ca, cb, cc, g, v);
  }
}

// ---------------------------------------------------------------- C-ABI
static int check_shape(const char* who, int p, int c) {
  TBN_REQUIRE(p >= 1 && c >= 4 && c % 4 == 0 && c <= 2048, "%s: p >= 1 and c a multiple of 4 in 4..2048", who);
  TBN_REQUIRE((size_t)p * (c / 4) < (1ull << 31), "%s: too many elements per call", who);
  return TBN_OK;
}
static int check_tensor(const char* who, const char* name, const void* ptr, int ld, int c) {
  TBN_REQUIRE(ptr != nullptr, "%s: %s is a null pointer", who, name);
  TBN_REQUIRE(ld >= c && ld % 4 == 0 && aligned16(ptr), "%s: %s needs a pitch that is a multiple of 4 and at least c, and a 16-byte aligned pointer", who, name);
  return TBN_OK;
}

int tbn_bn_res_apply(const float* y, int y_ld, int p, int c, const float* scale, const float* shift, const float* res,
                     int res_ld, int relu, float* z, int z_ld, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "bn_res_apply";
  TBN_TRY(check_shape(who, p, c));
  TBN_TRY(check_tensor(who, "y", y, y_ld, c));
  TBN_TRY(check_tensor(who, "z", z, z_ld, c));
  if (res != nullptr) TBN_TRY(check_tensor(who, "res", res, res_ld, c));
  TBN_REQUIRE(scale && shift && aligned16(scale) && aligned16(shift), "%s: scale / shift must be 16-byte aligned device pointers", who);
  TBN_REQUIRE(relu == 0 || relu == 1, "%s: relu is 0 or 1", who);
  const dim3 grid(ew_grid((size_t)p * c / 4, 4096)), block(256);
  const FastDiv dg = make_fastdiv((uint32_t)(c / 4));
  tbn_prof_begin(res ? (relu ? "bn_res_apply_kernel<res,relu>" : "bn_res_apply_kernel<res>")
                     : (relu ? "bn_res_apply_kernel<relu>" : "bn_res_apply_kernel<>"),
                 0.0, st, (double)p * c * 4.0 * (res ? 3 : 2));
  if (res != nullptr && relu) TBN_LAUNCH((bn_res_apply_kernel<true, true>), grid, block, 0, st, y, y_ld, p, c, scale, shift, res, res_ld, z, z_ld, dg);
  else if (res != nullptr) TBN_LAUNCH((bn_res_apply_kernel<true, false>), grid, block, 0, st, y, y_ld, p, c, scale, shift, res, res_ld, z, z_ld, dg);
  else if (relu) TBN_LAUNCH((bn_res_apply_kernel<false, true>), grid, block, 0, st, y, y_ld, p, c, scale, shift, res, res_ld, z, z_ld, dg);
  else TBN_LAUNCH((bn_res_apply_kernel<false, false>), grid, block, 0, st, y, y_ld, p, c, scale, shift, res, res_ld, z, z_ld, dg);
  tbn_prof_end(st);
  TBN_CHECK_LAUNCH("bn_res_apply");
  return TBN_OK;
}

int tbn_bn_res_fwd(const float* y, int y_ld, int p, int c, const float* partial, int pld, int nparts, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                   float* save_mean, float* save_rstd, float* scale, float* shift, const float* res, int res_ld,
                   int relu, float* z, int z_ld, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "bn_res_fwd";
  TBN_TRY(check_shape(who, p, c));
  TBN_REQUIRE(partial && aligned16(partial) && pld >= c && pld % 4 == 0 && nparts >= 1,
              "%s: partial needs nparts >= 1, a pitch that is a multiple of 4 and at least c, and a 16-byte aligned pointer", who);
  TBN_REQUIRE(gamma && beta && save_mean && save_rstd && scale && shift, "%s: null per-channel pointer", who);
  TBN_REQUIRE(running_mean == nullptr || running_var != nullptr, "%s: running_mean without running_var", who);
  // validate the apply's arguments before anything is launched
  TBN_TRY(check_tensor(who, "y", y, y_ld, c));
  TBN_TRY(check_tensor(who, "z", z, z_ld, c));
  if (res != nullptr) TBN_TRY(check_tensor(who, "res", res, res_ld, c));
  TBN_REQUIRE(aligned16(scale) && aligned16(shift), "%s: scale / shift must be 16-byte aligned", who);
  TBN_REQUIRE(relu == 0 || relu == 1, "%s: relu is 0 or 1", who);
  TBN_KLAUNCH(bn_res_finalize_kernel, dim3(cdiv(c, TBN_FIN_CH)), dim3(256), 0, st, partial, pld, nparts, p, c, gamma,
              beta, running_mean, running_var, momentum, eps, save_mean, save_rstd, scale, shift);
  TBN_CHECK_LAUNCH("bn_res_finalize");
  return tbn_bn_res_apply(y, y_ld, p, c, scale, shift, res, res_ld, relu, z, z_ld, stream);
}

size_t tbn_bn_res_bwd_workspace_floats(int p, int c) {
  if (p < 1 || c < 4 || c > 2048 || c % 4 != 0) return 0;
  return (size_t)res_parts(p) * 2 * c + 3 * (size_t)c;
}

int tbn_bn_res_bwd(const float* dz, int dz_ld, const float* z, int z_ld, const float* y, int y_ld, int p, int c,
                   const float* save_mean, const float* save_rstd, const float* scale, int relu, float* dy, int dy_ld,
                   float* dres, int dres_ld, int accumulate, float* dgamma, float* dbeta, float* workspace,
                   void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* who = "bn_res_bwd";
  TBN_TRY(check_shape(who, p, c));
  TBN_TRY(check_tensor(who, "dz", dz, dz_ld, c));
  TBN_TRY(check_tensor(who, "y", y, y_ld, c));
  TBN_TRY(check_tensor(who, "dy", dy, dy_ld, c));
  TBN_REQUIRE(relu == 0 || relu == 1, "%s: relu is 0 or 1", who);
  if (relu) TBN_TRY(check_tensor(who, "z", z, z_ld, c));
  if (dres != nullptr) TBN_TRY(check_tensor(who, "dres", dres, dres_ld, c));
  TBN_REQUIRE(save_mean && save_rstd && scale && aligned16(save_mean) && aligned16(save_rstd),
              "%s: save_mean / save_rstd / scale must be (16-byte aligned) device pointers", who);
  TBN_REQUIRE(workspace && aligned16(workspace), "%s: workspace must be a 16-byte aligned device pointer", who);
  const int pch = res_chunk(p), parts = res_parts(p), cs = res_slice_width(c);
  float* coef = workspace + (size_t)parts * 2 * c;
  const double elems = (double)p * c * 4.0;
  tbn_prof_begin(relu ? "bn_res_bwd_reduce_kernel<relu>" : "bn_res_bwd_reduce_kernel<>", 0.0, st, elems * (relu ? 3 : 2));
  if (relu) TBN_LAUNCH(bn_res_bwd_reduce_kernel<true>, dim3(parts, res_slices(c)), dim3(256), 0, st, dz, dz_ld, z, z_ld, y, y_ld, p, c, cs, pch, save_mean, save_rstd, workspace);
  else TBN_LAUNCH(bn_res_bwd_reduce_kernel<false>, dim3(parts, res_slices(c)), dim3(256), 0, st, dz, dz_ld, z, z_ld, y, y_ld, p, c, cs, pch, save_mean, save_rstd, workspace);
  tbn_prof_end(st);
  TBN_CHECK_LAUNCH("bn_res_bwd_reduce");
  TBN_TRY(tbn_launch_bn_bwd_finalize(workspace, parts, p, c, scale, save_mean, save_rstd, coef, dgamma, dbeta, nullptr, st));
  const dim3 grid(ew_grid((size_t)p * c / 4, 4096)), block(256);
  const FastDiv dg = make_fastdiv((uint32_t)(c / 4));
  const int mode = (relu ? 4 : 0) | (dres != nullptr ? 2 : 0) | (dres != nullptr && accumulate ? 1 : 0);
  tbn_prof_begin(relu ? (dres ? "bn_res_bwd_apply_kernel<relu,dres>" : "bn_res_bwd_apply_kernel<relu>")
                      : (dres ? "bn_res_bwd_apply_kernel<dres>" : "bn_res_bwd_apply_kernel<>"),
                 0.0, st, elems * (3 + (relu ? 1 : 0) + (dres ? (accumulate ? 2 : 1) : 0)));
#define TBN_RES_BWD_APPLY(R, D, A)                                                                                     \
  TBN_LAUNCH((bn_res_bwd_apply_kernel<R, D, A>), grid, block, 0, st, dz, dz_ld, z, z_ld, y, y_ld, p, c, coef, dy, dy_ld, \
             dres, dres_ld, dg)
  switch (mode) {
    case 0: TBN_RES_BWD_APPLY(false, false, false); break;
    case 2: TBN_RES_BWD_APPLY(false, true, false); break;
    case 3: TBN_RES_BWD_APPLY(false, true, true); break;
    case 4: TBN_RES_BWD_APPLY(true, false, false); break;
    case 6: TBN_RES_BWD_APPLY(true, true, false); break;
    default: TBN_RES_BWD_APPLY(true, true, true); break;
  }
#undef TBN_RES_BWD_APPLY
  tbn_prof_end(st);
  TBN_CHECK_LAUNCH("bn_res_bwd_apply");
  return TBN_OK;
}
