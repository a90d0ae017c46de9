// Clip summary for the attention visualiser (gfx950): what the prediction table and the figure read off a batch.
//
//   core/tools/vis.py:73-84    out[head].max(dim=1) ; (-(w * log(w + 1e-6)).sum(1)).mean() per clip
//   core/tools/vis.py:153-154  out[head].softmax(dim=1).topk(5, 1, largest=True, sorted=True)
//
// The reference walks the dataset at batch size 1 and reads five scalars per clip back to the host.  Here ONE launch
// per batch writes the k best classes of every head, their softmax probabilities and the clip's attention entropy at the
// batch's offset into device rings, and the host copies each ring once after the loop.
//
// One wave per clip, four clips per workgroup, as metric_update_kernel; the wave walks the heads.  No LDS, no atomics;
// lane 0 stores.  Every sum runs in a fixed order (a lane's strided terms in index order, then the xor-shuffle tree),
// so the results are bit-reproducible from run to run.
#include <cmath>

#include "tbn_common.h"
#include "../../include/tbn_hip.h"

// (value descending, class index ascending): does (v, c) come before (bv, bi)?  NaN never does.  The order of
// tbn_topk_correct / tbn_metric_update (train_ops.hip), restated.
__device__ __forceinline__ bool score_before(float v, int c, float bv, int bi) { return v > bv || (v == bv && c < bi); }

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

struct SummaryArgs {
  tbn_summary_head head[4];
  int num_heads, batch, k;
  const float* weights;
  int weights_ld, segments, T;
};

__global__ __launch_bounds__(256) void clip_summary_kernel(SummaryArgs a, int* __restrict__ top_idx,
                                                           float* __restrict__ top_prob, float* __restrict__ entropy) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.batch) return;
  for (int h = 0; h < a.num_heads; ++h) {
    const int C = a.head[h].classes;
    const float* row = a.head[h].scores + (size_t)b * a.head[h].scores_ld;
    // softmax normaliser: the largest score that is not NaN, then sum exp(v - max) over EVERY entry, so a NaN or +inf
    // entry (inf - inf) makes the sum NaN and with it every probability of the row, as torch.softmax does
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) {
      const float v = row[c];
      if (v > mx) mx = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(mx, o);
      if (ov > mx) mx = ov;
    }
    float sum = 0.0f;
    for (int c = lane; c < C; c += 64) sum += expf(row[c] - mx);
    sum = wave_sum(sum);
    // k rounds of wavefront arg-max: the best element strictly after (prev_v, prev_i)
    float prev_v = INFINITY;
    int prev_i = -1;
    const size_t slot0 = ((size_t)b * a.num_heads + h) * a.k;
    for (int j = 0; j < a.k; ++j) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int c = lane; c < C; c += 64) {
        const float v = row[c];
        const bool after = (v < prev_v) || (v == prev_v && c > prev_i);
        if (after && score_before(v, c, bv, bi)) {
          bv = v;
          bi = c;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (score_before(ov, oi, bv, bi)) {
          bv = ov;
          bi = oi;
        }
      }
      if (lane == 0) {
        const bool ranked = bi < C;   // false once the row has run out of classes that are not NaN
        top_idx[slot0 + j] = ranked ? bi : -1;
        top_prob[slot0 + j] = ranked ? expf(bv - mx) / sum : NAN;
      }
      prev_v = bv;
      prev_i = bi;
    }
  }
  if (a.weights != nullptr) {
    float total = 0.0f;
    for (int s = 0; s < a.segments; ++s) {
      const float* w = a.weights + ((size_t)b * a.segments + s) * a.weights_ld;
      float acc = 0.0f;
      for (int t = lane; t < a.T; t += 64) {
        const float v = w[t];
        acc += v * logf(v + 1e-6f);
      }
      total += -wave_sum(acc);
    }
    if (lane == 0) entropy[b] = total / (float)a.segments;
  }
}

extern "C" int tbn_clip_summary(const tbn_summary_head* heads, int num_heads, int batch, int k, const float* weights,
                                int weights_ld, int segments, int T, int* top_idx, float* top_prob, float* entropy,
                                void* stream) {
  TBN_REQUIRE(heads != nullptr && top_idx != nullptr && top_prob != nullptr, "clip_summary: null argument");
  TBN_REQUIRE(num_heads >= 1 && num_heads <= 4, "clip_summary: num_heads %d outside 1..4", num_heads);
  TBN_REQUIRE(k >= 1 && k <= 8, "clip_summary: k %d outside 1..8", k);
  TBN_REQUIRE(batch >= 0, "clip_summary: batch %d", batch);
  TBN_REQUIRE((weights == nullptr) == (entropy == nullptr),
              "clip_summary: weights and entropy go together (one of them is null)");
  SummaryArgs a = {};
  a.num_heads = num_heads, a.batch = batch, a.k = k;
  for (int h = 0; h < num_heads; ++h) {
    TBN_REQUIRE(heads[h].scores != nullptr, "clip_summary: null argument in head %d", h);
    TBN_REQUIRE(heads[h].classes >= 1 && heads[h].scores_ld >= heads[h].classes,
                "clip_summary: bad shape of head %d (C=%d, ld=%d)", h, heads[h].classes, heads[h].scores_ld);
    TBN_REQUIRE(k <= heads[h].classes, "clip_summary: k=%d outside 1..%d of head %d", k, heads[h].classes, h);
    a.head[h] = heads[h];
  }
  TBN_REQUIRE(segments >= 1, "clip_summary: segments %d", segments);
  if (weights != nullptr) {
    TBN_REQUIRE(T >= 1 && weights_ld >= T, "clip_summary: bad shape of the weights (T=%d, ld=%d)", T, weights_ld);
    a.weights = weights, a.weights_ld = weights_ld, a.segments = segments, a.T = T;
  }
  if (batch == 0) return TBN_OK;
  TBN_KLAUNCH(clip_summary_kernel, dim3(cdiv(batch, 4)), dim3(256), 0, (hipStream_t)stream, a, top_idx, top_prob,
              entropy);
  TBN_CHECK_LAUNCH("clip_summary");
  return TBN_OK;
}
