// Huffman decoding of baseline JPEG scans on the device (opt-in: decode_jpegs(entropy="device")): packed records from
// tbn_jpeg_scan_pack in, the quantised coefficients tbn_jpeg_reconstruct (jpeg.hip) takes out.  The algorithm, the
// record layout and the decoder core are in tbn_jpeg_sync.h, which scripts/jpeg_sync_check.cpp runs serially on the
// CPU under the sanitizers; this file is the parallel schedule round that core.
//
// One workgroup of 1024 threads per image, one launch, phases separated by workgroup barriers:
//   0  record check; Huffman tables -> LDS; the scan -> LDS when it is at most kStreamLdsBytes
//   1  subsequence size S (the caller's, or 1024; grown in steps of 32 until the lanes fit) and the lane -> interval map
//   2  relaxation rounds until no entry changes (hard bound: the lane count); idle lanes wait at the barriers
//   3  scan of the block counts, validation -> status
//   4  write pass: every lane decodes its subsequence once more and stores the non-zero coefficients (DC: difference)
//   5  DC differences -> DC values: a segmented scan over MCU chunks, reset at every restart interval
// Every barrier is reached by all 1024 threads: the only early exits are workgroup-uniform (a value read from LDS after
// a barrier).  A corrupt stream costs a status bit, never an address outside the image's coefficients.
#include "tbn_common.h"
#include "tbn_jpeg_sync.h"
#include "../../include/tbn_hip.h"

using namespace tbn_jpeg;

// ---------------------------------------------------------------- host entries (no HIP call in them) ------------------
extern "C" size_t tbn_jpeg_scan_pack_bytes(size_t file_size, int n_intervals) {
  return tbn_jpeg_host_scan_pack_bytes(file_size, n_intervals > 0 ? (size_t)n_intervals : 0);
}

extern "C" int tbn_jpeg_scan_pack(const unsigned char* data, size_t size, const tbn_jpeg_geometry* expect, void* record,
                                  size_t record_bytes, int max_intervals, uint16_t* quant, int* n_intervals, size_t* used) {
  char err[256];
  const int rc = tbn_jpeg_host_scan_pack(data, size, expect, record, record_bytes, max_intervals, quant, n_intervals, used,
                                         err, sizeof(err));
  if (rc) tbn_set_error("%s", err);
  return rc;
}

// ---------------------------------------------------------------- device stage ----------------------------------------
constexpr int kEntThreads = TBN_JPEG_SYNC_MAX_LANES;
constexpr uint32_t kStreamLdsBytes = 48 * 1024;     // with the tables and the lane arrays: 71 KiB, two workgroups per CU
constexpr int kEntArr = kEntThreads + 8;

struct EntP {
  SyncGeom g;
  uint32_t s_req;            // 0: TBN_JPEG_SYNC_DEFAULT_BITS
  unsigned long long packed_bytes;
  int n_img;
};

struct EntShared {
  DevTables tab;
  SyncGeom g;
  uint32_t w[4][kEntArr];    // phases 2-3: exit p, exit bz, block counts, lanes per interval (scanned); phase 5: the DC scan
  uint32_t stream[kStreamLdsBytes / 4];
  PackedHeader hdr;
  uint32_t acc, bad, max_bits, status;
  uint32_t changed[2];
  uint8_t natural[64];
  uint8_t slots[16];         // table slot of each block of the MCU: DC, AC
};

__constant__ uint8_t c_zigzag_to_natural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// sum of v over the workgroup; three barriers, reached by every thread
__device__ __forceinline__ uint32_t ent_block_sum(uint32_t v, uint32_t* acc) {
  if (threadIdx.x == 0) *acc = 0;
  __syncthreads();
  if (v) atomicAdd(acc, v);
  __syncthreads();
  const uint32_t r = *acc;
  __syncthreads();
  return r;
}

// inclusive scan of a[0, kEntThreads) in place (Hillis-Steele: 10 steps, two barriers each), closed by a barrier
__device__ __forceinline__ void ent_block_scan(uint32_t* a) {
  const int t = threadIdx.x;
  __syncthreads();
#pragma unroll 1
  for (int off = 1; off < kEntThreads; off <<= 1) {
    const uint32_t x = t >= off ? a[t - off] : 0u;
    __syncthreads();
    a[t] += x;
    __syncthreads();
  }
}

__device__ __forceinline__ int ent_sat_add(int a, int b) {     // |a| <= 2^30, |b| <= 2^30
  return min(max(a + b, -(1 << 30)), 1 << 30);
}

template <bool kLds>
__device__ __forceinline__ void ent_image(EntShared& sh, const EntP& p, const unsigned char* __restrict__ rec,
                                          int16_t* __restrict__ coef, int* __restrict__ status_out,
                                          int* __restrict__ info_out, uint32_t* __restrict__ ws_out) {
  const int t = threadIdx.x;
  const uint32_t n_int = sh.hdr.n_intervals, ri = sh.hdr.restart_interval, nwords = (sh.hdr.scan_bytes + 3) / 4;
  const uint32_t* __restrict__ iv = reinterpret_cast<const uint32_t*>(rec + kPackedIntervalsOff);
  const uint32_t* gwords = reinterpret_cast<const uint32_t*>(rec + sh.hdr.scan_off);
  const uint32_t* words = gwords;
  if (kLds) {
    for (uint32_t i = t; i < nwords; i += kEntThreads) sh.stream[i] = sync_bswap(gwords[i]);     // nwords <= kStreamLdsBytes / 4
    words = sh.stream;
  }
  // ---- phase 1: S and the lane -> interval map
  const uint32_t my_bits = (uint32_t)t < n_int ? iv[2 * t + 1] : 0u;
  uint32_t S = p.s_req ? p.s_req : (uint32_t)TBN_JPEG_SYNC_DEFAULT_BITS;
  uint32_t lanes = ent_block_sum(sync_interval_lanes(my_bits, S), &sh.acc);       // also closes the LDS loads above
  if (lanes > (uint32_t)kEntThreads) {        // the smallest multiple of 32 at which the lanes fit: lanes(32 hi) <= n_int
    uint32_t lo = S / 32, hi = max((sh.max_bits + 31) / 32, lo + 1);
#pragma unroll 1
    while (hi - lo > 1) {                     // workgroup-uniform: lo, hi and the sums are the same in every thread
      const uint32_t mid = lo + (hi - lo) / 2;
      if (ent_block_sum(sync_interval_lanes(my_bits, 32 * mid), &sh.acc) > (uint32_t)kEntThreads) lo = mid; else hi = mid;
    }
    S = 32 * hi;
    lanes = ent_block_sum(sync_interval_lanes(my_bits, S), &sh.acc);
  }
  uint32_t* lane_incl = sh.w[3];              // lane_incl[i]: lanes of intervals 0..i
  lane_incl[t] = sync_interval_lanes(my_bits, S);
  ent_block_scan(lane_incl);
  const bool live = (uint32_t)t < lanes;      // lanes <= kEntThreads here
  uint32_t sub_end = 0, int_end = 0, first_block = 0, block_limit = 0, my_int = 0, my_first_lane = 0;
  SyncState entry = {0, 0}, guess = {0, 0};
  bool is_first = true;
  if (live) {
    uint32_t lo = 0, hi = n_int - 1;          // the smallest i with lane_incl[i] > t: it exists because t < lanes
    while (lo < hi) {
      const uint32_t mid = (lo + hi) / 2;
      if (lane_incl[mid] > (uint32_t)t) hi = mid; else lo = mid + 1;
    }
    my_int = lo;
    my_first_lane = lo ? lane_incl[lo - 1] : 0u;
    const uint32_t k = (uint32_t)t - my_first_lane, start = iv[2 * lo], len = iv[2 * lo + 1];   // start + len <= 8 scan_bytes < 2^31
    int_end = start + len;
    const unsigned long long nominal = (unsigned long long)start + (unsigned long long)(k + 1) * S;
    sub_end = nominal < int_end ? (uint32_t)nominal : int_end;
    entry.p = start + k * S;                  // k S < len
    guess.p = sub_end;
    is_first = k == 0;
  }
  // ---- phase 2: relaxation
  uint32_t* exit_p = sh.w[0];
  uint32_t* exit_bz = sh.w[1];
  uint32_t* counts = sh.w[2];
  counts[t] = 0;
  if (t < 2) sh.changed[t] = 0;
  bool dirty = live;
  uint32_t ev = 0, rounds = 0;
  SyncNoSink none;
#pragma unroll 1
  for (uint32_t r = 1; r <= lanes; ++r) {     // lanes, sh.changed: workgroup-uniform, so is the trip count
    if (dirty) {
      SyncState st = entry;
      uint32_t n;
      ev = sync_decode<kLds>(&sh.tab, words, nwords, sub_end, int_end, sh.g.bpm, sh.slots, guess, &st, &n, none);
      exit_p[t] = st.p;
      exit_bz[t] = st.bz;
      counts[t] = n;
    }
    __syncthreads();                          // the exits are written; every read of changed[(r + 1) & 1] is behind us
    if (t == 0) sh.changed[(r + 1) & 1] = 0;
    dirty = false;
    if (live && !is_first) {
      const uint32_t pp = exit_p[t - 1], bz = exit_bz[t - 1];
      if (pp != entry.p || bz != entry.bz) {
        entry.p = pp;
        entry.bz = bz;
        dirty = true;
        sh.changed[r & 1] = 1;
      }
    }
    __syncthreads();
    rounds = r;
    if (!sh.changed[r & 1]) break;            // uniform
  }
  // ---- phase 3: block bases and validation
  ent_block_scan(counts);                     // counts[l]: blocks completed by lanes 0..l
  if (live) {
    if (ev & TBN_JPEG_EV_CODE) atomicOr(&sh.status, (uint32_t)TBN_JPEG_ST_CODE);
    if (ev & TBN_JPEG_EV_RUN) atomicOr(&sh.status, (uint32_t)TBN_JPEG_ST_RUN);
    const uint32_t before_int = my_first_lane ? counts[my_first_lane - 1] : 0u, before_me = t ? counts[t - 1] : 0u;
    const uint32_t base = (uint32_t)((unsigned long long)my_int * ri * (uint32_t)sh.g.bpm);
    first_block = base + (before_me - before_int);
    block_limit = base + sync_interval_blocks(sh.g, ri, my_int);
  }
  if ((uint32_t)t < n_int) {
    const uint32_t first = t ? lane_incl[t - 1] : 0u, end = lane_incl[t];      // first <= end <= lanes
    const bool has = end > first;
    const uint32_t blocks = has ? counts[end - 1] - (first ? counts[first - 1] : 0u) : 0u;
    SyncState last = {0, 0};
    if (has) { last.p = exit_p[end - 1]; last.bz = exit_bz[end - 1]; }
    const uint32_t st = sync_interval_status(blocks, sync_interval_blocks(sh.g, ri, (uint32_t)t), has, last, iv[2 * t] + iv[2 * t + 1]);
    if (st) atomicOr(&sh.status, st);
  }
  __syncthreads();
  if (sh.status == 0) {                       // uniform; nothing writes sh.status until the next barrier
    // ---- phase 4: the write pass
    if (live) {
      SyncCoefSink sink = {coef, &sh.g, sh.natural, first_block, block_limit, 0xFFFFFFFFu, 0u, false};
      SyncState st = entry;
      uint32_t n;
      sync_decode<kLds>(&sh.tab, words, nwords, sub_end, int_end, sh.g.bpm, sh.slots, guess, &st, &n, sink);
    }
    __threadfence_block();
    __syncthreads();                          // the differences are in memory, sh.w is free
    // ---- phase 5: DC differences -> values.  Thread t owns MCUs [m0, m1); (flag, sums) compose as a segmented scan
    const uint32_t total = sh.g.total_mcus, chunk = (total + kEntThreads - 1) / kEntThreads;
    const uint32_t m0 = min((uint32_t)t * chunk, total), m1 = min(m0 + chunk, total);
    const int bpm = sh.g.bpm;
    int sum[3] = {0, 0, 0};
    uint32_t flag = 0;
    for (uint32_t m = m0; m < m1; ++m) {
      if (ri && m % ri == 0) { flag = 1; sum[0] = sum[1] = sum[2] = 0; }
      for (int b = 0; b < bpm; ++b) {
        uint32_t off;
        if (sync_block_offset(sh.g, m * (uint32_t)bpm + (uint32_t)b, &off)) {
          const int c = sh.g.comp[b];
          const int v = ent_sat_add(c == 0 ? sum[0] : (c == 1 ? sum[1] : sum[2]), coef[off]);
          if (c == 0) sum[0] = v; else if (c == 1) sum[1] = v; else sum[2] = v;
        }
      }
    }
    sh.w[0][t] = flag;
    sh.w[1][t] = (uint32_t)sum[0];
    sh.w[2][t] = (uint32_t)sum[1];
    sh.w[3][t] = (uint32_t)sum[2];
    __syncthreads();
#pragma unroll 1
    for (int off = 1; off < kEntThreads; off <<= 1) {
      uint32_t f = 0;
      int s0 = 0, s1 = 0, s2 = 0;
      if (t >= off) { f = sh.w[0][t - off]; s0 = (int)sh.w[1][t - off]; s1 = (int)sh.w[2][t - off]; s2 = (int)sh.w[3][t - off]; }
      __syncthreads();
      if (t >= off) {
        if (!sh.w[0][t]) {                    // no reset inside the right part: the left part's sums carry over
          sh.w[1][t] = (uint32_t)ent_sat_add(s0, (int)sh.w[1][t]);
          sh.w[2][t] = (uint32_t)ent_sat_add(s1, (int)sh.w[2][t]);
          sh.w[3][t] = (uint32_t)ent_sat_add(s2, (int)sh.w[3][t]);
        }
        sh.w[0][t] |= f;
      }
      __syncthreads();
    }
    int pred[3] = {0, 0, 0};
    if (t) { pred[0] = (int)sh.w[1][t - 1]; pred[1] = (int)sh.w[2][t - 1]; pred[2] = (int)sh.w[3][t - 1]; }
    bool dc_bad = false;
    for (uint32_t m = m0; m < m1; ++m) {
      if (ri && m % ri == 0) pred[0] = pred[1] = pred[2] = 0;
      for (int b = 0; b < bpm; ++b) {
        uint32_t off;
        if (sync_block_offset(sh.g, m * (uint32_t)bpm + (uint32_t)b, &off)) {
          const int c = sh.g.comp[b];
          const int v = ent_sat_add(c == 0 ? pred[0] : (c == 1 ? pred[1] : pred[2]), coef[off]);
          if (c == 0) pred[0] = v; else if (c == 1) pred[1] = v; else pred[2] = v;
          dc_bad |= v < -32768 || v > 32767;
          coef[off] = (int16_t)v;
        }
      }
    }
    if (dc_bad) atomicOr(&sh.status, (uint32_t)TBN_JPEG_ST_DC);
    __syncthreads();
  }
  if (t == 0) {
    *status_out = (int)sh.status;
    info_out[0] = (int)lanes;
    info_out[1] = (int)rounds;
    ws_out[0] = S; ws_out[1] = lanes; ws_out[2] = rounds; ws_out[3] = kLds ? 1u : 0u;
  }
}

__global__ __launch_bounds__(kEntThreads) void jpeg_entropy_kernel(EntP p, const unsigned char* __restrict__ packed,
                                                                   const uint32_t* __restrict__ offsets,
                                                                   int16_t* __restrict__ coef, int* __restrict__ status,
                                                                   int* __restrict__ info, uint32_t* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) EntShared sh;
  const int t = threadIdx.x, img = blockIdx.x;
  const uint32_t off = offsets[img];
  // ---- phase 0: the record.  Thread 0 judges it; everyone reads the verdict after the barrier
  if (t == 0) {
    uint32_t bad = 0;
    sh.status = 0;
    sh.max_bits = 0;
    sh.acc = 0;
    if (off == TBN_JPEG_SYNC_NO_RECORD) {
      bad = TBN_JPEG_ST_SKIPPED;
    } else if ((off & 15u) || (unsigned long long)off + kPackedIntervalsOff > p.packed_bytes) {
      bad = TBN_JPEG_ST_RECORD;
    } else {
      const PackedHeader h = *reinterpret_cast<const PackedHeader*>(packed + off);
      const unsigned long long scan_end = (unsigned long long)h.scan_off + (((unsigned long long)h.scan_bytes + 15ull) & ~15ull);
      if (h.magic != TBN_JPEG_SYNC_MAGIC || h.n_intervals < 1 || h.n_intervals > (uint32_t)kEntThreads ||
          h.intervals_off != kPackedIntervalsOff || (h.scan_off & 15u) ||
          h.scan_off < kPackedIntervalsOff + 8ull * h.n_intervals || (unsigned long long)off + scan_end > p.packed_bytes ||
          h.scan_bytes >= (1u << 28))
        bad = TBN_JPEG_ST_RECORD;
      sh.hdr = h;
    }
    sh.bad = bad;
    sh.g = p.g;
  }
  if (t < 64) sh.natural[t] = c_zigzag_to_natural[t];
  __syncthreads();
  int* info_out = info + 2 * (size_t)img;
  uint32_t* ws_out = ws + 4 * (size_t)img;
  if (sh.bad) {                               // uniform
    if (t == 0) {
      status[img] = (int)sh.bad;
      info_out[0] = info_out[1] = 0;
      ws_out[0] = ws_out[1] = ws_out[2] = ws_out[3] = 0;
    }
    return;
  }
  const unsigned char* rec = packed + off;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(rec + kPackedTablesOff);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&sh.tab);
    for (uint32_t i = t; i < sizeof(DevTables) / 4; i += kEntThreads) dst[i] = src[i];
    if ((uint32_t)t < sh.hdr.n_intervals) {
      const uint32_t* iv = reinterpret_cast<const uint32_t*>(rec + kPackedIntervalsOff);
      const uint32_t start = iv[2 * t], len = iv[2 * t + 1];
      if ((unsigned long long)start + len > 8ull * sh.hdr.scan_bytes) atomicOr(&sh.bad, (uint32_t)TBN_JPEG_ST_RECORD);
      atomicMax(&sh.max_bits, len);
    }
  }
  __syncthreads();
  if (sh.bad) {                               // uniform
    if (t == 0) {
      status[img] = (int)sh.bad;
      info_out[0] = info_out[1] = 0;
      ws_out[0] = ws_out[1] = ws_out[2] = ws_out[3] = 0;
    }
    return;
  }
  if (t == 0) sync_block_slots(&sh.tab, sh.g, sh.slots);       // read after the barriers of ent_image's first sum
  int16_t* my_coef = coef + (size_t)img * p.g.coef_count;
  if (sh.hdr.scan_bytes <= kStreamLdsBytes)   // uniform
    ent_image<true>(sh, p, rec, my_coef, status + img, info_out, ws_out);
  else
    ent_image<false>(sh, p, rec, my_coef, status + img, info_out, ws_out);
}

static int entropy_params(const char* fn, const tbn_jpeg_geometry* g, int n_img, EntP* p) {
  TBN_REQUIRE(g != nullptr, "%s: null geometry", fn);
  TBN_REQUIRE(n_img >= 0, "%s: n_img %d", fn, n_img);
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
  const int mx = (g->width + 8 * hs - 1) / (8 * hs), my = (g->height + 8 * vs - 1) / (8 * vs);
  size_t coef = 0;
  for (int c = 0; c < g->components; ++c) {
    TBN_REQUIRE(g->blocks_w[c] == mx * g->hsamp[c] && g->blocks_h[c] == my * g->vsamp[c],
                "%s: block extents %dx%d of component %d do not belong to a %dx%d image", fn, g->blocks_w[c], g->blocks_h[c], c,
                g->width, g->height);
    coef += (size_t)64 * g->blocks_w[c] * g->blocks_h[c];
  }
  TBN_REQUIRE(coef == g->coef_count, "%s: coef_count %zu does not belong to this geometry (%zu)", fn, g->coef_count, coef);
  TBN_REQUIRE(coef < ((size_t)1 << 31), "%s: a %dx%d image is too large", fn, g->width, g->height);
  memset(p, 0, sizeof(*p));
  sync_geom(g, &p->g);
  p->n_img = n_img;
  return TBN_OK;
}

extern "C" size_t tbn_jpeg_entropy_workspace_bytes(const tbn_jpeg_geometry* geometry, int n_img) {
  EntP p;
  if (entropy_params("jpeg_entropy_workspace_bytes", geometry, n_img, &p) != TBN_OK) return 0;
  return (size_t)16 * (size_t)(n_img > 0 ? n_img : 1);
}

extern "C" int tbn_jpeg_entropy_decode_dev(const void* packed_dev, size_t packed_bytes, const uint32_t* offsets_dev, int n_img,
                                           const tbn_jpeg_geometry* geometry, int subseq_bits, int16_t* coef_dev,
                                           int* status_dev, int* info_dev, void* workspace, void* stream) {
  const char* fn = "jpeg_entropy_decode_dev";
  EntP p;
  const int rc = entropy_params(fn, geometry, n_img, &p);
  if (rc != TBN_OK) return rc;
  TBN_REQUIRE(subseq_bits == 0 || (subseq_bits >= 64 && subseq_bits % 32 == 0 && subseq_bits <= (1 << 24)),
              "%s: subseq_bits %d is not 0 or a multiple of 32 in [64, 2^24]", fn, subseq_bits);
  if (n_img == 0) return TBN_OK;
  TBN_REQUIRE(packed_dev != nullptr && offsets_dev != nullptr && coef_dev != nullptr && status_dev != nullptr &&
                  info_dev != nullptr && workspace != nullptr, "%s: null argument", fn);
  TBN_REQUIRE(((uintptr_t)packed_dev & 15) == 0 && ((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)offsets_dev & 3) == 0 &&
                  ((uintptr_t)status_dev & 3) == 0 && ((uintptr_t)info_dev & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
              "%s: packed and coef must be 16-byte aligned, the others 4-byte aligned", fn);
  TBN_REQUIRE(packed_bytes < ((size_t)1 << 32), "%s: %zu packed bytes are too many for one launch", fn, packed_bytes);
  p.s_req = (uint32_t)subseq_bits;
  p.packed_bytes = packed_bytes;
  hipStream_t st = (hipStream_t)stream;
  // the lanes store the non-zero coefficients only
  const hipError_t e = hipMemsetAsync(coef_dev, 0, (size_t)n_img * geometry->coef_count * sizeof(int16_t), st);
  TBN_REQUIRE_OR(TBN_ERR_LAUNCH, e == hipSuccess, "%s: hipMemsetAsync failed: %s", fn, hipGetErrorString(e));
  TBN_KLAUNCH(jpeg_entropy_kernel, dim3((unsigned)n_img), dim3(kEntThreads), 0, st, p, (const unsigned char*)packed_dev,
              offsets_dev, coef_dev, status_dev, info_dev, (uint32_t*)workspace);
  TBN_CHECK_LAUNCH(fn);
  return TBN_OK;
}
