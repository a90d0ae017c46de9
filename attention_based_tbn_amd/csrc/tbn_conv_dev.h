// Device code shared by the convolution kernels (conv_igemm.hip, conv_bf16x.hip): hardware-bounds-checked buffer
// loads / stores, the XCD tile map and the epilogue of a finished accumulator tile.
#pragma once
#include "tbn_common.h"
#include "tbn_kernels.h"

// Hardware-bounds-checked 16-B loads.  ROCm 7.2's clang lowers __builtin_amdgcn_raw_buffer_load_b128 to a
// ONE-dword load, so the LLVM intrinsic is bound directly (same idiom as composable_kernel).
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ f32x4 tbn_llvm_buffer_load_f32x4(i32x4 srsrc, int voffset, int soffset, int aux) __asm(
    "llvm.amdgcn.raw.buffer.load.v4f32");
#define TBN_OOB 0x80000000u  // byte offset beyond any buffer extent (< 2 GiB enforced) -> hardware returns 0

// 128-bit buffer descriptor from wave-uniform kernel arguments (base, extent in bytes)
__device__ __forceinline__ i32x4 make_rsrc(const void* ptr, unsigned bytes) {
  union {
    i32x4 v;
    struct {
      const void* p;
      unsigned range, cfg;
    } s;
  } u;
  u.s.p = ptr;
  u.s.range = bytes;
  u.s.cfg = 0x00020000u;
  i32x4 r;
  r.x = __builtin_amdgcn_readfirstlane(u.v.x);
  r.y = __builtin_amdgcn_readfirstlane(u.v.y);
  r.z = __builtin_amdgcn_readfirstlane(u.v.z);
  r.w = __builtin_amdgcn_readfirstlane(u.v.w);
  return r;
}

__device__ void tbn_llvm_buffer_store_f32(float data, i32x4 srsrc, int voffset, int soffset, int aux) __asm(
    "llvm.amdgcn.raw.buffer.store.f32");
__device__ float tbn_llvm_buffer_load_f32(i32x4 srsrc, int voffset, int soffset, int aux) __asm(
    "llvm.amdgcn.raw.buffer.load.f32");

__device__ __forceinline__ float4 buf_load4(i32x4 r, unsigned voff, unsigned soff = 0u) {
  const f32x4 v = tbn_llvm_buffer_load_f32x4(r, (int)voff, (int)soff, 0);
  return make_float4(v.x, v.y, v.z, v.w);
}

// XCD-aware bijective remap of a 1-D grid of `nb` workgroups: blocks b, b + 8, ... share an XCD (and its L2) -> they get
// consecutive logical ids, so each XCD owns one contiguous run of the ids
__device__ __forceinline__ int xcd_remap(const int bid, const int nb) {
  const int q8 = nb >> 3, r8 = nb & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
}
// ... for the tiles_m x tiles_n output tiles of a conv GEMM, N fastest: the tiles of an activation row panel share an XCD
__device__ __forceinline__ void xcd_tile(const int bid, const int tiles_m, const int tiles_n, int& tm, int& tn) {
  const int nid = xcd_remap(bid, tiles_m * tiles_n);
  tm = nid / tiles_n;
  tn = nid - tm * tiles_n;
}

// ---------------------------------------------------------------- epilogue (shared by the GEMM bodies)
// EPI 1 / 2 work on the bias-free accumulator (training: a per-channel constant cancels in the batch-stat
// BN; eval: the bias is folded into `shift`).  Rows >= M and columns >= Cout hold exact zeros, so the
// statistics need no masking.  Stores are buffer stores: the lane offset is computed once per 32x32
// sub-tile, the per-register row step rides in the scalar offset -> no VALU address math, no branches.
// Precondition: every wave has passed a barrier after its last LDS tile read (`lds` is reused for the partial sums).
// WM = waves stacked along M: 4 (the GEMM bodies whose waves own 32*MT rows each) or 1 (conv_sk4_body: ONE wave holds the
// finished (32*MT) x (32*NT) tile, the partial sums go straight to global memory, no barrier).
template <int MT, int NT, int EPI, bool RED, int WM = 4>
__device__ __forceinline__ void conv_epilogue(const ConvP& p, f32x16 (&acc)[MT][NT], float* lds, const int tm,
                                              const int m0, const int n0) {
  constexpr int BM = 32 * WM * MT, BN = 32 * NT;
  const int tid = threadIdx.x, lane = tid & 63, wave = WM == 1 ? 0 : (tid >> 6);
  const int lrow = lane & 31, lhalf = lane >> 5;
  float* red = lds;  // [2][4 waves][BN] for the BN-statistics partials (tiles are dead now)
  const int mrow0 = m0 + wave * 32 * MT + 4 * lhalf;  // + i*32 + 8*g + q  (accumulator register e = 4*g + q)
  const bool tile_full = (m0 + BM <= p.M);
  constexpr bool scatter = (EPI == 3);  // strided data-gradient phase
  constexpr bool SUMS = (EPI == 1) || RED;   // (the K loop ends with a barrier: `red` may overlay the tiles)
  // VALU diet of the epilogue (round 3): the static instruction count of a <1,1> data-gradient tile with the reduce was
  // ~650 VALU (~450 of them here) against 16 MFMAs per K-step -- 2.2 VALU per MFMA over an 18-step tile, 6.8 over the
  // 6 steps of the short-K 1x1 groups -- because block-uniform run-time cases (ragged last M tile, accumulate, ReLU,
  // bias) were evaluated per element with selects.  A full tile without those takes the LEAN loop: per element one
  // store (+ 2 VALU for the statistics, + 6 for the reduce); everything else keeps the general loop.
  // (round 4: an accumulating data gradient -- the 1x1 groups of 3c / 4e / 5b, whose block input also receives a max
  //  pool's gradient -- takes the lean loop too, with its 16 old values loaded up front like the reduce's y values: these
  //  were the slowest data gradients of a backbone, 72-92 TF/s, on the ~450-VALU general loop because of that one flag)
  const bool lean = tile_full && !scatter && (EPI != 0 || ((p.flags & CONV_FLAG_RELU) == 0 && p.bias == nullptr));
  const bool accum = (EPI == 0) && (p.flags & CONV_FLAG_ACCUM) != 0;   // block-uniform
  // strided data-gradient phase: output pixel of each tile row, decoded ONCE per row into LDS (was: two magic-number
  // divisions per ELEMENT, ~25 VALU x 16 elements x NT sub-tiles per lane)
  unsigned* opix_tab = reinterpret_cast<unsigned*>(lds + 2 * 4 * BN);
  if (scatter) {
    if (tid < BM) {
      const int m = m0 + tid;
      const uint32_t n = fdiv((uint32_t)m, p.div_ohw);
      const uint32_t rem = (uint32_t)m - n * p.div_ohw.d;
      const uint32_t a = fdiv(rem, p.div_ow);
      const uint32_t b = rem - a * p.div_ow.d;
      const unsigned opix = (unsigned)(((int)n * p.OH + ((int)a * p.out_sy + p.out_oy)) * p.OW + ((int)b * p.out_sx + p.out_ox));
      opix_tab[tid] = m < p.M ? opix : 0xffffffffu;
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int colb = n0 + j * 32;
    if (colb >= p.Cout) continue;  // block-uniform
    const int col = colb + lrow;
    const bool col_ok = col < p.Cout;
    int sg = 0;
    if (p.nseg > 1 && colb >= p.seg[1].col_begin) sg = 1;
    if (p.nseg > 2 && colb >= p.seg[2].col_begin) sg = 2;
    if (p.nseg > 3 && colb >= p.seg[3].col_begin) sg = 3;
    const int old = p.seg[sg].ld;
    const i32x4 o_rsrc = make_rsrc(p.seg[sg].ptr, p.seg_bytes[sg]);
    const unsigned col_off = (unsigned)(col - p.seg[sg].col_begin) * 4u;
    const float bias = (EPI == 0 || EPI == 3) ? ((p.bias != nullptr && col_ok) ? p.bias[col] : 0.f) : 0.f;
    float sc = 1.f, sh = 0.f;
    bool raw = false;
    if (EPI == 2) {
      raw = (p.raw_seg1 == sg + 1);   // block-uniform
      if (col_ok && !raw) {
        sc = p.scale[col];
        sh = p.shift[col];
      }
    }
    // fused BN-backward reduce: the producer layer of these 32 columns (block-uniform, segments start on x32 columns)
    int rs = 0, lc = 0;
    bool red_on = false;
    i32x4 y_rsrc = o_rsrc;
    unsigned ycol_off = 0u;
    int yld = 0;
    float b_sc = 0.f, b_sh = 0.f, b_mu = 0.f, b_rs = 0.f;
    if (RED) {
      if (p.nred > 1 && colb >= p.red[1].col_begin) rs = 1;
      if (p.nred > 2 && colb >= p.red[2].col_begin) rs = 2;
      if (p.nred > 3 && colb >= p.red[3].col_begin) rs = 3;
      red_on = p.red[rs].y != nullptr && colb < p.red[rs].col_begin + p.red[rs].C;
      if (red_on) {
        y_rsrc = make_rsrc(p.red[rs].y, p.red[rs].y_bytes);
        yld = p.red[rs].y_ld;
        lc = col - p.red[rs].col_begin;
        ycol_off = (unsigned)lc * 4u;
        if (lc < p.red[rs].C) {
          const float* stp = p.red[rs].stats + p.red[rs].c_off + lc;
          b_mu = stp[0];
          b_rs = stp[p.red_chan];
          b_sc = stp[2 * p.red_chan];
          b_sh = stp[3 * p.red_chan];
        }
      }
    }
    float s1 = 0.f, s2 = 0.f;
    if (lean) {
      // columns without a BN layer behind them (or beyond it) keep b_sc = b_sh = 0: fma(y, 0, 0) > 0 is false -> g = 0
      const float b_nmr = -b_mu * b_rs;       // xhat = fma(y, rstd, -mean * rstd)
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const unsigned vbase = col_ok ? (unsigned)(mrow0 + i * 32) * (unsigned)old * 4u + col_off : TBN_OOB;
        const unsigned ybase = (RED && red_on && col_ok) ? (unsigned)(mrow0 + i * 32) * (unsigned)yld * 4u + ycol_off : TBN_OOB;
        float yv[16], ov[16];
        if (EPI == 0 && accum) {
#pragma unroll
          for (int e = 0; e < 16; ++e)
            ov[e] = tbn_llvm_buffer_load_f32(o_rsrc, (int)vbase, (int)((unsigned)((8 * (e >> 2) + (e & 3)) * old) * 4u), 0);
        }
        if (RED) {
#pragma unroll
          for (int e = 0; e < 16; ++e)
            yv[e] = tbn_llvm_buffer_load_f32(y_rsrc, (int)ybase, (int)((unsigned)((8 * (e >> 2) + (e & 3)) * yld) * 4u), 0);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int dm = 8 * (e >> 2) + (e & 3);
          float v = acc[i][j][e];
          if (EPI == 0 && accum) v += ov[e];
          if (EPI == 1) {
            s1 += v;
            s2 = fmaf(v, v, s2);
          } else if (EPI == 2) {
            if (!raw) v = fmaxf(fmaf(v, sc, sh), 0.f);
          }
          tbn_llvm_buffer_store_f32(v, o_rsrc, (int)vbase, (int)((unsigned)(dm * old) * 4u), 0);
          if (RED) {
            const float g = fmaf(yv[e], b_sc, b_sh) > 0.f ? v : 0.f;
            s1 += g;
            s2 = fmaf(g, fmaf(yv[e], b_rs, b_nmr), s2);
          }
        }
      }
    } else {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const unsigned vbase = col_ok ? (unsigned)(mrow0 + i * 32) * (unsigned)old * 4u + col_off : TBN_OOB;
      const unsigned ybase = (RED && red_on && col_ok) ? (unsigned)(mrow0 + i * 32) * (unsigned)yld * 4u + ycol_off : TBN_OOB;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int dm = 8 * (e >> 2) + (e & 3);
        float v = acc[i][j][e];
        if (EPI == 1) {
          s1 += v;
          s2 = fmaf(v, v, s2);
        } else if (EPI == 2) {
          if (!raw) v = fmaxf(fmaf(v, sc, sh), 0.f);
        } else {
          v += bias;
        }
        unsigned voff = vbase, soff = (unsigned)(dm * old) * 4u;
        unsigned yvoff = ybase, ysoff = (unsigned)(dm * yld) * 4u;
        if (scatter) {
          const unsigned opix = opix_tab[wave * 32 * MT + i * 32 + 4 * lhalf + dm];   // 0xffffffff: row >= M
          const bool ok = opix != 0xffffffffu && col_ok;
          voff = ok ? __umul24(opix, (unsigned)old * 4u) + col_off : TBN_OOB;
          soff = 0u;
          if (RED) {
            yvoff = (ok && red_on) ? __umul24(opix, (unsigned)yld * 4u) + ycol_off : TBN_OOB;
            ysoff = 0u;
          }
        } else if (!tile_full) {
          const int m = mrow0 + i * 32 + dm;
          voff = (m < p.M) ? vbase : TBN_OOB;  // the scalar offset is not bounds-checked: mask the row here
          if (RED) yvoff = (m < p.M) ? ybase : TBN_OOB;
        }
        if (EPI == 0 || EPI == 3) {
          if (p.flags & CONV_FLAG_ACCUM) v += tbn_llvm_buffer_load_f32(o_rsrc, (int)voff, (int)soff, 0);
          if (p.flags & CONV_FLAG_RELU) v = fmaxf(v, 0.f);
        }
        tbn_llvm_buffer_store_f32(v, o_rsrc, (int)voff, (int)soff, 0);
        if (RED) {
          // rows >= M / masked lanes: v may hold junk only where the store was masked too -> mask g the same way
          const float yv = tbn_llvm_buffer_load_f32(y_rsrc, (int)yvoff, (int)ysoff, 0);
          const float g = (yvoff != TBN_OOB && fmaf(yv, b_sc, b_sh) > 0.f) ? v : 0.f;
          s1 += g;
          s2 = fmaf(g, (yv - b_mu) * b_rs, s2);
        }
      }
    }
    }
    if (SUMS) {
      s1 += __shfl_xor(s1, 32);
      s2 += __shfl_xor(s2, 32);
      if (WM == 1) {   // the wave holds the whole tile: its column sums ARE the tile's partial row
        if (lhalf == 0 && col_ok) {
          if (EPI == 1) {
            p.stat_partial[((size_t)tm * 2 + 0) * p.Cout + col] = s1;
            p.stat_partial[((size_t)tm * 2 + 1) * p.Cout + col] = s2;
          } else if (red_on && lc < p.red[rs].C) {
            float* part = p.red[rs].partial + (size_t)(p.red_row0 + tm) * 2 * p.red[rs].C;
            part[lc] = s1;
            part[p.red[rs].C + lc] = s2;
          }
        }
      } else if (lhalf == 0) {
        red[(0 * 4 + wave) * BN + j * 32 + lrow] = s1;
        red[(1 * 4 + wave) * BN + j * 32 + lrow] = s2;
      }
    }
  }
  if (SUMS && WM != 1) {
    __syncthreads();
    if (tid < BN && n0 + tid < p.Cout) {
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        t1 += red[(0 * 4 + w) * BN + tid];
        t2 += red[(1 * 4 + w) * BN + tid];
      }
      if (EPI == 1) {
        p.stat_partial[((size_t)tm * 2 + 0) * p.Cout + n0 + tid] = t1;
        p.stat_partial[((size_t)tm * 2 + 1) * p.Cout + n0 + tid] = t2;
      } else {
        const int col = n0 + tid;
        int rs = 0;
        if (p.nred > 1 && col >= p.red[1].col_begin) rs = 1;
        if (p.nred > 2 && col >= p.red[2].col_begin) rs = 2;
        if (p.nred > 3 && col >= p.red[3].col_begin) rs = 3;
        const int lc = col - p.red[rs].col_begin;
        if (p.red[rs].y != nullptr && lc < p.red[rs].C) {
          float* part = p.red[rs].partial + (size_t)(p.red_row0 + tm) * 2 * p.red[rs].C;
          part[lc] = t1;
          part[p.red[rs].C + lc] = t2;
        }
      }
    }
  }
}
