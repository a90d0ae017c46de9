// Log-power STFT spectrogram on gfx950 (replaces the CPU librosa call of reference
// core/dataset/dataset.py:461-495: librosa.stft(n_fft=511, hop=120, win_length=240, "hann",
// center=True, pad_mode="constant") followed by log(|X|^2 + 1e-6)).
//
// Only 239 of the 511 window taps are non-zero (periodic Hann(240), centred), so a frame's 256
// bins are a dense 256 x 240 real DFT: X[k] = sum_j hann[j] * y[120 t - 120 + j] * e^{-2 pi i (j+135) k / 511}.
// That is a [bins x taps] x [taps x frames] contraction -> fp32 MFMA (32x32x2), 2 * 2 * 256 * 240 FLOP per frame.
//
// Workgroup = 4 waves = 64 frames of one segment x 128 bins (wave = 32 bins; blockIdx.z picks the half of the bins); re and
// im of 2 frame tiles = 4 accumulators per wave.  Config 4's 96 segments x 4 frame blocks x 2 = 768 workgroups = 3 per CU.
// (An 8-wave form that stages the frames once for all 256 bins is 1.5 % faster when its grid happens to fill the CUs evenly
// and 25 % slower when it does not; a persistent form that overlaps the stores of one unit with the MFMAs of the next
// measured the same as this one -- both removed, round 3.)
//   * frames (B operand): hop = 120, 240 taps -> consecutive frames overlap by half.  The RAW samples of the 64
//     frames (65 hop rows of 120) are staged ONCE per workgroup in LDS with rows padded to 124 floats: frame f, tap j
//     lives at (f + j / 120) * 124 + j % 120, no im2col copy, and a lane's four consecutive taps are one conflict-free
//     ds_read_b128 (lane stride 496 B -> 16 distinct 16-B slots per 16-lane group).  The 65 rows are one contiguous
//     span of the waveform: staged with 16-B buffer loads (1950 of them per workgroup, 8 per thread) whose hardware
//     range check supplies the zero padding in front of the first and behind the last sample;
//   * twiddles (A operand): the window is folded into the table, stored [cos | -sin][tap / 8][bin][tap % 8]: the
//     fragment of 8 taps x 32 bins is ONE fully coalesced 1-KB load per wave (the table is 480 KB, shared by every
//     workgroup: L2 resident), prefetched two 8-tap groups ahead (stft_groups below); each load feeds 8 MFMAs;
//   * k is permuted identically for A and B (lane half h holds taps 4h..4h+3 of the group) so one 16-B fragment
//     feeds four MFMAs; accumulators put frames on lanes -> the (256, W) freq-major rows are written 128 B contiguous;
//   * log(|X|^2 + eps) with the hardware logarithm (v_log_f32, 1 ulp): 3 VALU instructions per output instead of the
//     ~20 of logf's software path (32 outputs per lane: the epilogue was 8 % of the kernel).
//
// The rest of the audio data layer lives here too (reference dataset.py:421-575): the audio window cut inside the launch
// (tbn_stft_windows: a table of window addresses instead of a staged batch), the log-mel representation (the same kernel
// writing |X|^2 + mel_db_kernel) and the "loud" attention prior (attn_prior_loud_kernel).
//
// Everything above is the geometry of data.audio.sampling_rate = 24000: window 240, hop 120.  The reference derives both from
// the rate (dataset.py:483-484: 10 ms and 5 ms, rounded); at any other rate stft_rate_kernel below does the same contraction
// with window, hop and tap-group count at run time (tbn_stft_rate_windows), feeding the same epilogue, mel and prior kernels.
// The 24 kHz kernel is untouched and stays the path of (240, 120).
#include <cmath>
#include <cstring>

#include "tbn_kernels.h"
#include "../../include/tbn_hip.h"

#define STFT_TAPS 240
#define STFT_KG 30     // groups of 8 taps
#define STFT_BINS 256
#define STFT_FR 64     // frames per workgroup
#define STFT_PITCH 124 // LDS floats per hop row of 120 samples

typedef int stft_i32x4 __attribute__((ext_vector_type(4)));
__device__ f32x4 stft_buffer_load_f32x4(stft_i32x4 srsrc, int voffset, int soffset, int aux) __asm(
    "llvm.amdgcn.raw.buffer.load.v4f32");
__device__ void stft_buffer_store_f32(float v, stft_i32x4 srsrc, int voffset, int soffset, int aux) __asm(
    "llvm.amdgcn.raw.buffer.store.f32");

// One tap group (8 taps) = 16 MFMAs of a wave.  The loop runs D groups per trip on D-slot register rings, so no slot
// is copied: group kg multiplies slot kg % D while the twiddle fragments of groups kg + 1 .. kg + D - 1 and the frame
// taps of group kg + 1 are in flight into the other slots.  The twiddle address is a scalar base (advanced per group, wrapping to
// group 0 behind the last one: a persistent workgroup's ring runs on into its next unit) plus one per-lane offset, and
// there is no branch in the trip: with a conditional prefetch the compiler's wait-count pass fell back to vmcnt(0) right
// behind the loads it had just issued (the L2 latency sat in front of every group).
struct StftAcc {
  f32x16 re0, im0, re1, im1;
};
template <int D>
struct StftRing {
  float4 c[D], s[D];   // twiddle fragments (cos | -sin) of D consecutive tap groups
};

__device__ __forceinline__ float4 stft_tw_load(const float* tw, unsigned k_byte, unsigned lane_byte) {
  return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(tw) + k_byte + lane_byte);
}

// groups [KB, KE) of the K loop (KB, KE multiples of D); fr_off = LDS float index of (frame lrow, tap 8 * KB + 4 * lhalf);
// fa / fb [KB % 2] hold the frame taps of group KB on entry
template <int D, int KB, int KE>
__device__ __forceinline__ void stft_groups(const float* __restrict__ frc, int fr_off, const float* __restrict__ tw,
                                            unsigned lane_byte, StftRing<D>& tr, float4 (&fa)[D], float4 (&fb)[D], StftAcc& a) {
  static_assert(KB % D == 0 && KE % D == 0 && STFT_KG % D == 0, "ring depth must divide the group ranges");
  constexpr unsigned kGroupBytes = STFT_BINS * 8 * 4, kPartBytes = STFT_KG * kGroupBytes;
#pragma unroll 1
  for (int kg = KB; kg < KE; kg += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int k = kg + j;
      const unsigned kn = (unsigned)(k + D - 1 < STFT_KG ? k + D - 1 : k + D - 1 - STFT_KG) * kGroupBytes;
      tr.c[(j + D - 1) % D] = stft_tw_load(tw, kn, lane_byte);
      tr.s[(j + D - 1) % D] = stft_tw_load(tw, kn + kPartBytes, lane_byte);
      // taps of the next group: + 8 floats, + 12 where tap 120 opens the next hop row; the last group re-reads itself
      fr_off += k + 1 == STFT_KG ? 0 : (k + 1 == 15 ? 12 : 8);
      fa[(j + 1) % D] = *reinterpret_cast<const float4*>(&frc[fr_off]);
      fb[(j + 1) % D] = *reinterpret_cast<const float4*>(&frc[fr_off + 32 * STFT_PITCH]);
      __builtin_amdgcn_sched_barrier(0);
      const float4 c = tr.c[j], s = tr.s[j], f0 = fa[j], f1 = fb[j];
#define STFT_STEP(q)                                                            \
      a.re0 = __builtin_amdgcn_mfma_f32_32x32x2f32(c.q, f0.q, a.re0, 0, 0, 0);   \
      a.im0 = __builtin_amdgcn_mfma_f32_32x32x2f32(s.q, f0.q, a.im0, 0, 0, 0);   \
      a.re1 = __builtin_amdgcn_mfma_f32_32x32x2f32(c.q, f1.q, a.re1, 0, 0, 0);   \
      a.im1 = __builtin_amdgcn_mfma_f32_32x32x2f32(s.q, f1.q, a.im1, 0, 0, 0);
      STFT_STEP(x) STFT_STEP(y) STFT_STEP(z) STFT_STEP(w)
#undef STFT_STEP
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int D>
__device__ __forceinline__ void stft_ring_start(const float* __restrict__ tw, unsigned lane_byte, StftRing<D>& tr) {
  constexpr unsigned kGroupBytes = STFT_BINS * 8 * 4, kPartBytes = STFT_KG * kGroupBytes;
#pragma unroll
  for (int d = 0; d + 1 < D; ++d) {
    tr.c[d] = stft_tw_load(tw, d * kGroupBytes, lane_byte);
    tr.s[d] = stft_tw_load(tw, d * kGroupBytes + kPartBytes, lane_byte);
  }
}

// log(|X|^2 + eps) of a wave's 32 bins x 64 frames -> (256, W) freq-major rows of the segment, 128 B contiguous per store;
// |X|^2 + eps >= 1e-6 is a normal number: v_log_f32 (log2, 1 ulp) * ln 2.  Raw-buffer stores: frames >= W get an offset
// outside the segment's 256 x W floats and are dropped by the range check (no branch per store, 32-bit offsets).
// POWER (the log-mel path, dataset.py:496-506): the plain power re^2 + im^2 instead, no log / exp round trip.
template <bool POWER>
__device__ __forceinline__ void stft_store(float* __restrict__ o, int W, int b0, int t0, int lrow, int lhalf, float eps,
                                           const StftAcc& a) {
  const float ln2 = 0.6931471805599453f;
  union {
    stft_i32x4 v;
    struct {
      void* p;
      unsigned range, cfg;
    } d;
  } u;
  u.d.p = o;
  u.d.range = (unsigned)(STFT_BINS * W) * 4u;
  u.d.cfg = 0x00020000u;
  stft_i32x4 rs;
  rs.x = __builtin_amdgcn_readfirstlane(u.v.x);
  rs.y = __builtin_amdgcn_readfirstlane(u.v.y);
  rs.z = __builtin_amdgcn_readfirstlane(u.v.z);
  rs.w = __builtin_amdgcn_readfirstlane(u.v.w);
  const int ta = t0 + lrow, tb = ta + 32;
  const int row = (b0 + 4 * lhalf) * W;
  const int oa = ta < W ? (row + ta) * 4 : (int)0x80000000, ob = tb < W ? (row + tb) * 4 : (int)0x80000000;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int soff = (8 * (e >> 2) + (e & 3)) * W * 4;   // the bin row of accumulator element e (wave-uniform)
    if (POWER) {
      stft_buffer_store_f32(fmaf(a.re0[e], a.re0[e], a.im0[e] * a.im0[e]), rs, oa + soff, 0, 0);
      stft_buffer_store_f32(fmaf(a.re1[e], a.re1[e], a.im1[e] * a.im1[e]), rs, ob + soff, 0, 0);
      continue;
    }
    stft_buffer_store_f32(__builtin_amdgcn_logf(fmaf(a.re0[e], a.re0[e], fmaf(a.im0[e], a.im0[e], eps))) * ln2, rs, oa + soff, 0, 0);
    stft_buffer_store_f32(__builtin_amdgcn_logf(fmaf(a.re1[e], a.re1[e], fmaf(a.im1[e], a.im1[e], eps))) * ln2, rs, ob + soff, 0, 0);
  }
}

// a segment's samples as a raw buffer: offsets in front of sample 0 (negative -> huge unsigned) and behind sample len - 1
// are out of range, per dword -> zeros (librosa's centre padding, reference dataset.py:487-489).  The base is row `seg` of a
// contiguous (nseg, len) batch, or -- `windows` non-null -- entry `seg` of a table of window addresses into untrimmed clips
// (the trim of dataset.py:439-451 as a pointer): the range is the WINDOW's len samples either way, so the padding in front
// of and behind a window is zeros, never the clip's neighbouring audio (librosa pads the trimmed sample).  A window's
// address is only 4-byte aligned; offsets are still multiples of 16 B relative to it, and a multi-dword buffer load needs
// dword alignment only (its range check is per dword, relative to the base) -- a 16-B group that straddles a cache line is
// two requests, nothing else.
__device__ __forceinline__ stft_i32x4 stft_segment_buffer(const float* wave, const float* const* windows, int seg, int len) {
  union {
    stft_i32x4 v;
    struct {
      const void* p;
      unsigned range, cfg;
    } d;
  } u;
  u.d.p = windows ? windows[seg] : wave + (size_t)seg * len;
  u.d.range = (unsigned)len * 4u;
  u.d.cfg = 0x00020000u;
  stft_i32x4 rs;
  rs.x = __builtin_amdgcn_readfirstlane(u.v.x);
  rs.y = __builtin_amdgcn_readfirstlane(u.v.y);
  rs.z = __builtin_amdgcn_readfirstlane(u.v.z);
  rs.w = __builtin_amdgcn_readfirstlane(u.v.w);
  return rs;
}

template <bool POWER>
__global__ __launch_bounds__(256) void stft_logpower_kernel(const float* __restrict__ wave, const float* const* __restrict__ windows,
                                                            int len, int W, const float* __restrict__ tw,
                                                            float* __restrict__ spec, float eps) {
  __shared__ __attribute__((aligned(16))) float fr[(STFT_FR + 1) * STFT_PITCH];
  const int seg = blockIdx.y, t0 = blockIdx.x * STFT_FR;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lrow = lane & 31, lhalf = lane >> 5;
  const int b0 = blockIdx.z * 128 + wv * 32;
  const unsigned lane_byte = (unsigned)((b0 + lrow) * 2 + lhalf) * 16u;   // [part][kg][b0 + lrow][4 * lhalf]
  StftRing<3> tr;
  stft_ring_start(tw, lane_byte, tr);
  {
    const stft_i32x4 rs = stft_segment_buffer(wave, windows, seg, len);
    const int g0 = (t0 - 1) * 120;     // first staged sample (a multiple of 4: a 16-B group never straddles sample 0)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i4 = tid + 256 * q;    // 16-B group of the 65 x 120 span (30 groups per hop row)
      if (i4 < (STFT_FR + 1) * 30) {
        const int r = (i4 * 2185) >> 16, c4 = i4 - r * 30;   // i4 / 30 for i4 < 2048
        const f32x4 v = stft_buffer_load_f32x4(rs, (g0 + i4 * 4) * 4, 0, 0);
        *reinterpret_cast<float4*>(&fr[r * STFT_PITCH + c4 * 4]) = make_float4(v.x, v.y, v.z, v.w);
      }
    }
  }
  StftAcc a;
#pragma unroll
  for (int e = 0; e < 16; ++e) a.re0[e] = a.im0[e] = a.re1[e] = a.im1[e] = 0.f;
  __syncthreads();
  const int off = lrow * STFT_PITCH + 4 * lhalf;
  float4 fa[3], fb[3];
  fa[0] = *reinterpret_cast<const float4*>(&fr[off]);
  fb[0] = *reinterpret_cast<const float4*>(&fr[off + 32 * STFT_PITCH]);
  stft_groups<3, 0, STFT_KG>(fr, off, tw, lane_byte, tr, fa, fb, a);
  stft_store<POWER>(spec + (size_t)seg * STFT_BINS * W, W, b0, t0, lrow, lhalf, eps, a);
}

// ---- the STFT at any sampling rate (reference dataset.py:483-495: win = round(10 ms * rate), hop = round(5 ms * rate)) ----
// The same contraction, [256 bins x 8 * KG taps] . [taps x frames], with the geometry at run time: tap j of frame t reads
// sample t * hop - win / 2 + j, KG = ceil(win / 8) tap groups (up to 64; the table's taps from `win` to 8 * KG are exact
// zeros), the same workgroup (64 frames x 128 bins, 4 waves), twiddle layout, k permutation and epilogue as above.  What
// the 24 kHz kernel takes from its constants is decided here per launch:
//   * the staged span, (64 - 1) * hop + 8 * KG samples from s0 = t0 * hop - win / 2 (up to 128 KB: dynamic LDS), is loaded
//     in 16-B groups that start at multiples of 4 SAMPLES, whatever s0 is: a group is then wholly in front of sample 0
//     (out of range as a whole: zeros, which is right) or wholly behind it -- one that straddled sample 0 would lose its
//     real samples.  Sample s goes to LDS position x = s - s0, so frame f starts at f * hop whatever s0 mod 4 is: one
//     ds_write_b128 per group when s0 is a multiple of 4 and hop % 4 == 0, four ds_write_b32 otherwise.  Every position
//     of the span is written (zeros in front of the first and behind the last sample), so no fragment read meets a word
//     that was never staged (0 * NaN);
//   * ALIGNED (hop % 4 == 0: 8, 16, 24, 32, 44.1, 48 kHz): a lane's 4 taps are one 16-B aligned ds_read_b128.  Each hop
//     row gets `pad` = 4 floats behind it when hop / 4 is even -- position x lives at x + pad * (x / hop) -- so the lane
//     stride hop + pad is an odd number of 16-B slots (16 distinct slots per 16-lane group; hop 120 -> the 124 above);
//   * any other hop (22.05 kHz: 110, 11.025 kHz: 55): frames start off the 16-B grid, where a ds_read_b128 is replayed
//     at 64 cycles per instruction -- four ds_read_b32 per fragment instead, on the unpadded span (8 per tap group and
//     wave against its 16 MFMAs = 1024 MFMA cycles);
//   * a 3-slot twiddle ring like the one above, with the prefetch index clamped to the last group instead of wrapping,
//     whole trips of 3 groups without a branch and the 0 .. 2 groups left over behind them.
#define STFT_RATE_D 3

template <bool ALIGNED>
__device__ __forceinline__ int stft_rate_pos(int x, int pad, unsigned rcp) {   // rcp = floor(2^32 / hop) + 1: x / hop is
  return ALIGNED ? x + pad * (int)__umulhi((unsigned)x, rcp) : x;              // exact for x * hop < 2^32
}

template <bool ALIGNED>
__device__ __forceinline__ float4 stft_rate_taps(const float* __restrict__ fr, int i) {
  if (ALIGNED) return *reinterpret_cast<const float4*>(&fr[i]);
  return make_float4(fr[i], fr[i + 1], fr[i + 2], fr[i + 3]);
}

template <bool POWER, bool ALIGNED>
__global__ __launch_bounds__(256) void stft_rate_kernel(const float* __restrict__ wave, const float* const* __restrict__ windows,
                                                        int len, int W, int half, int hop, int KG, int pad, unsigned rcp,
                                                        const float* __restrict__ tw, float* __restrict__ spec, float eps) {
  extern __shared__ __attribute__((aligned(16))) float fr_dyn[];
  constexpr int D = STFT_RATE_D;
  constexpr unsigned kGroupBytes = STFT_BINS * 8 * 4;
  const int seg = blockIdx.y, t0 = blockIdx.x * STFT_FR;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lrow = lane & 31, lhalf = lane >> 5;
  const int b0 = blockIdx.z * 128 + wv * 32;
  const unsigned lane_byte = (unsigned)((b0 + lrow) * 2 + lhalf) * 16u;   // [part][kg][b0 + lrow][4 * lhalf]
  const unsigned part_bytes = (unsigned)KG * kGroupBytes;
  StftRing<D> tr;
#pragma unroll
  for (int d = 0; d + 1 < D; ++d) {
    const unsigned kn = (unsigned)min(d, KG - 1) * kGroupBytes;
    tr.c[d] = stft_tw_load(tw, kn, lane_byte);
    tr.s[d] = stft_tw_load(tw, kn + part_bytes, lane_byte);
  }
  const int span = (STFT_FR - 1) * hop + 8 * KG;
  {
    const stft_i32x4 rs = stft_segment_buffer(wave, windows, seg, len);
    const int s0 = t0 * hop - half;        // first staged sample; a0 <= s0: the multiple of 4 its 16-B group starts at
    const int a0 = s0 & ~3, d0 = s0 - a0;
    const int ngroups = (d0 + span + 3) >> 2;
    const bool whole = ALIGNED && d0 == 0; // then span % 4 == 0 too, and no group straddles a hop row
    // four loads in flight per thread; a group behind the span is loaded (the range check makes that safe) and dropped
#pragma unroll 1
    for (int i0 = tid; i0 < ngroups; i0 += 4 * 256) {
      f32x4 v[4];
      // unsigned byte offset: in front of sample 0 it is >= 2^31, out of range like everything behind sample len - 1
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = stft_buffer_load_f32x4(rs, (int)((unsigned)(a0 + 4 * (i0 + 256 * q)) * 4u), 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int x = 4 * (i0 + 256 * q) - d0;
        if (whole) {
          if (x < span)
            *reinterpret_cast<float4*>(&fr_dyn[stft_rate_pos<ALIGNED>(x, pad, rcp)]) = make_float4(v[q].x, v[q].y, v[q].z, v[q].w);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (x + e >= 0 && x + e < span) fr_dyn[stft_rate_pos<ALIGNED>(x + e, pad, rcp)] = v[q][e];
        }
      }
    }
  }
  StftAcc a;
#pragma unroll
  for (int e = 0; e < 16; ++e) a.re0[e] = a.im0[e] = a.re1[e] = a.im1[e] = 0.f;
  __syncthreads();
  // frame lrow (and lrow + 32), tap j at position lrow * hop + j: base + j + pad * (j / hop)
  const int base = lrow * (hop + pad), second = 32 * (hop + pad), j0 = 4 * lhalf;
  float4 fa[D], fb[D];
  fa[0] = stft_rate_taps<ALIGNED>(fr_dyn, base + j0);
  fb[0] = stft_rate_taps<ALIGNED>(fr_dyn, base + second + j0);
  // group k from ring slot j = k % D: prefetch the twiddles of group k + D - 1 and the taps of group k + 1 (both clamped to
  // the last group: a re-read, no branch), then the 16 MFMAs
#define STFT_RATE_GROUP(j, k)                                                                \
  {                                                                                          \
    const unsigned kn = (unsigned)min((k) + D - 1, KG - 1) * kGroupBytes;                     \
    tr.c[((j) + D - 1) % D] = stft_tw_load(tw, kn, lane_byte);                                \
    tr.s[((j) + D - 1) % D] = stft_tw_load(tw, kn + part_bytes, lane_byte);                   \
    const int jn = 8 * min((k) + 1, KG - 1) + j0;                                             \
    const int fo = base + stft_rate_pos<ALIGNED>(jn, pad, rcp);                               \
    fa[((j) + 1) % D] = stft_rate_taps<ALIGNED>(fr_dyn, fo);                                  \
    fb[((j) + 1) % D] = stft_rate_taps<ALIGNED>(fr_dyn, fo + second);                         \
    __builtin_amdgcn_sched_barrier(0);                                                       \
    const float4 c = tr.c[j], s = tr.s[j], f0 = fa[j], f1 = fb[j];                            \
    STFT_RATE_STEP(x) STFT_RATE_STEP(y) STFT_RATE_STEP(z) STFT_RATE_STEP(w)                   \
    __builtin_amdgcn_sched_barrier(0);                                                       \
  }
#define STFT_RATE_STEP(q)                                                     \
  a.re0 = __builtin_amdgcn_mfma_f32_32x32x2f32(c.q, f0.q, a.re0, 0, 0, 0);     \
  a.im0 = __builtin_amdgcn_mfma_f32_32x32x2f32(s.q, f0.q, a.im0, 0, 0, 0);     \
  a.re1 = __builtin_amdgcn_mfma_f32_32x32x2f32(c.q, f1.q, a.re1, 0, 0, 0);     \
  a.im1 = __builtin_amdgcn_mfma_f32_32x32x2f32(s.q, f1.q, a.im1, 0, 0, 0);
  int kg = 0;
#pragma unroll 1
  for (; kg + D <= KG; kg += D) {
    STFT_RATE_GROUP(0, kg)
    STFT_RATE_GROUP(1, kg + 1)
    STFT_RATE_GROUP(2, kg + 2)
  }
  if (kg < KG) STFT_RATE_GROUP(0, kg)
  if (kg + 1 < KG) STFT_RATE_GROUP(1, kg + 1)
#undef STFT_RATE_STEP
#undef STFT_RATE_GROUP
  static_assert(D == 3, "the trips above are written out for a ring of 3");
  stft_store<POWER>(spec + (size_t)seg * STFT_BINS * W, W, b0, t0, lrow, lhalf, eps, a);
}

// ---- log-mel (spec_type "logms", reference dataset.py:496-506: librosa melspectrogram + power_to_db(ref = np.max)) ----
// One workgroup per segment: mel = basis (128 x 256) . power (256 x W), then 10 log10(max(amin, mel)) - 10 log10(max(amin,
// max mel)), floored at -80 dB.  A Slaney mel filter is a triangle over a handful of neighbouring bins (about 500 non-zeros
// in the 128 x 256 basis), so each output sums only its filter's [first, last] non-zero bin span, found here from the
// caller's basis: 2 x ~500 x W FLOP per segment instead of the dense GEMM's 2 x 32768 x W -- VALU work, no MFMA needed.
// Pass 1 leaves the mel power in `out` and reduces the segment maximum (each thread its own items in index order, then a
// shuffle tree and 8 wave values read in order: no float atomics, and max is exact, so the same input gives the same bits);
// pass 2 has each thread turn exactly the elements it wrote itself into dB.  The dB maximum of a segment is 0 by
// construction (its largest element and `ref` go through the same log10f and the same rounded product: no fused
// multiply-subtract in the conversion, fp contract off), so the top_db clip is max(db, -80) and silence is exactly 0 dB.
#define MEL_N 128
#define MEL_THREADS 512
#define MEL_G 8   // mels per work item: item = (group of 8 filters, frame), frames fastest -> coalesced power / out rows

__global__ __launch_bounds__(MEL_THREADS) void mel_db_kernel(const float* __restrict__ power, const float* __restrict__ basis,
                                                              int W, float* __restrict__ out) {
  __shared__ int lo[MEL_N], hi[MEL_N];
  __shared__ float wmax[MEL_THREADS / 64];
  const int tid = threadIdx.x;
  const float* __restrict__ P = power + (size_t)blockIdx.x * STFT_BINS * W;
  float* O = out + (size_t)blockIdx.x * MEL_N * W;
  if (tid < MEL_N) {
    int l = STFT_BINS, h = 0;
    for (int k = 0; k < STFT_BINS; ++k)
      if (basis[tid * STFT_BINS + k] != 0.f) {
        l = min(l, k);
        h = k + 1;
      }
    lo[tid] = l;
    hi[tid] = h;
  }
  __syncthreads();
  const int items = (MEL_N / MEL_G) * W;
  float mx = -INFINITY;
  for (int item = tid; item < items; item += MEL_THREADS) {
    const int mg = item / W, t = item - mg * W;
#pragma unroll 1
    for (int j = 0; j < MEL_G; ++j) {
      const int m = mg * MEL_G + j;
      float acc = 0.f;
      for (int k = lo[m]; k < hi[m]; ++k) acc = fmaf(basis[m * STFT_BINS + k], P[k * W + t], acc);
      O[m * W + t] = acc;
      mx = fmaxf(mx, acc);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  if ((tid & 63) == 0) wmax[tid >> 6] = mx;
  __syncthreads();
  float ref = wmax[0];
#pragma unroll
  for (int w = 1; w < MEL_THREADS / 64; ++w) ref = fmaxf(ref, wmax[w]);
  {
#pragma clang fp contract(off)
    const float amin = 1e-10f;
    const float ref_db = 10.0f * log10f(fmaxf(amin, ref));
    for (int item = tid; item < items; item += MEL_THREADS) {
      const int mg = item / W, t = item - mg * W;
#pragma unroll 1
      for (int j = 0; j < MEL_G; ++j) {
        const int i = (mg * MEL_G + j) * W + t;
        const float db = 10.0f * log10f(fmaxf(amin, O[i]));
        O[i] = fmaxf(db - ref_db, -80.0f);
      }
    }
  }
}

// ---- the "loud" attention prior (reference dataset.py:534-575, `_get_attn_weights`) ----
// One wave per segment.  Column maxima over all F rows of the nblk * T frames that lie in full blocks of T (lanes on
// consecutive frames: coalesced rows) -> LDS; block maxima and their arg-max, ties to the HIGHEST block index; then the
// reference's selection among the T host-computed Gaussian values and their minimum -- no arithmetic on them.
#define PRIOR_MAX_W 4096

__global__ __launch_bounds__(64) void attn_prior_loud_kernel(const float* __restrict__ spec, int F, int W, int T,
                                                             const float* __restrict__ gauss, float* __restrict__ out) {
  __shared__ float col[PRIOR_MAX_W];
  const int lane = threadIdx.x;
  const float* __restrict__ S = spec + (size_t)blockIdx.x * F * W;
  const int nblk = W / T, ncol = nblk * T;
  for (int c = lane; c < ncol; c += 64) {
    float m0 = -INFINITY, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
    int r = 0;
    for (; r + 4 <= F; r += 4) {
      m0 = fmaxf(m0, S[(r + 0) * W + c]);
      m1 = fmaxf(m1, S[(r + 1) * W + c]);
      m2 = fmaxf(m2, S[(r + 2) * W + c]);
      m3 = fmaxf(m3, S[(r + 3) * W + c]);
    }
    for (; r < F; ++r) m0 = fmaxf(m0, S[r * W + c]);
    col[c] = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
  }
  __syncthreads();
  float best = -INFINITY;
  int loc = -1;
  for (int b = lane; b < nblk; b += 64) {
    float v = col[b * T];
    for (int i = 1; i < T; ++i) v = fmaxf(v, col[b * T + i]);
    if (loc < 0 || v >= best) {
      best = v;
      loc = b;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off);
    const int ol = __shfl_xor(loc, off);
    if (ol >= 0 && (loc < 0 || ov > best || (ov == best && ol > loc))) {
      best = ov;
      loc = ol;
    }
  }
  float gmin = gauss[0];
  for (int i = 1; i < T; ++i) gmin = fminf(gmin, gauss[i]);
  const int mean = T / 2;
  const bool roll = loc <= T && (loc < mean - 2 || loc > mean + 2);
  for (int i = lane; i < T; i += 64) {
    float v = gauss[i];
    if (roll) {
      v = gauss[(((i - (loc - mean)) % T) + T) % T];            // np.roll(wts, loc - mean)
      if (loc - 4 > 0 && i < loc - 4) v = gmin;                  // wts[:loc - 4] = min
      if (loc + 4 < T && i >= loc + 4) v = gmin;                 // wts[loc + 4:] = min
    }
    out[(size_t)blockIdx.x * T + i] = v;
  }
}

// the one STFT launch behind tbn_stft_logpower and tbn_stft_windows; `what` names the entry in error messages
template <bool POWER>
static int stft_launch(const char* what, const float* wave, const float* const* windows, int nseg, int len,
                       const float* twiddle, float* spec, float eps, bool profile, hipStream_t st) {
  const int W = 1 + (len - 1) / 120;
  // 32-bit byte offsets inside a segment's samples and inside its 256 x W spectrogram
  TBN_REQUIRE(nseg <= 65535 && (size_t)len * 4 < (1ull << 31) && (size_t)STFT_BINS * W * 4 < (1ull << 31),
              "%s: too many segments / too long a waveform per call", what);
  const dim3 grid(cdiv(W, STFT_FR), nseg, 2);
  if (profile) {
    tbn_prof_begin(POWER ? "stft_logpower_kernel<power>" : "stft_logpower_kernel<log>",
                   4.0 * STFT_BINS * STFT_TAPS * (double)W * nseg, st);
    TBN_LAUNCH(stft_logpower_kernel<POWER>, grid, dim3(256), 0, st, wave, windows, len, W, twiddle, spec, eps);
    tbn_prof_end(st);
  } else {
    TBN_KLAUNCH(stft_logpower_kernel<POWER>, grid, dim3(256), 0, st, wave, windows, len, W, twiddle, spec, eps);
  }
  TBN_CHECK_LAUNCH(what);
  return TBN_OK;
}

// the accepted geometry of the rate kernel (librosa refuses win_length > n_fft = 511; tap groups of 8 need win >= 8)
static inline bool stft_rate_geometry_ok(int win, int hop) { return win >= 8 && win <= 511 && hop >= 1 && hop <= win; }

template <bool POWER, bool ALIGNED>
static int stft_rate_launch_as(const float* wave, const float* const* windows, int nseg, int len, int W, int win, int hop,
                               const float* twiddle, float* spec, float eps, hipStream_t st) {
  const int KG = cdiv(win, 8), pad = ALIGNED && (hop / 4) % 2 == 0 ? 4 : 0;
  const unsigned rcp = ALIGNED ? (unsigned)((1ull << 32) / (unsigned)hop) + 1u : 0u;
  // LDS floats: the last position of the span + 1 (stft_rate_pos), whole 16-B groups
  const int span = (STFT_FR - 1) * hop + 8 * KG;
  const size_t lds = (size_t)((span + pad * ((span - 1) / hop) + 3) & ~3) * sizeof(float);
  TBN_REQUIRE(lds <= TBN_DYN_LDS_MAX, "stft_rate_windows: window %d / hop %d needs %zu bytes of LDS", win, hop, lds);
  static size_t allowed = TBN_DYN_LDS_DEFAULT;
  const int rc = tbn_raise_dyn_lds((const void*)stft_rate_kernel<POWER, ALIGNED>, lds, allowed, "stft_rate_windows");
  if (rc != TBN_OK) return rc;
  const dim3 grid(cdiv(W, STFT_FR), nseg, 2);
  tbn_prof_begin(POWER ? "stft_rate_kernel<power>" : "stft_rate_kernel<log>", 4.0 * STFT_BINS * win * (double)W * nseg, st);
  TBN_LAUNCH((stft_rate_kernel<POWER, ALIGNED>), grid, dim3(256), lds, st, wave, windows, len, W, win / 2, hop, KG, pad, rcp,
             twiddle, spec, eps);
  tbn_prof_end(st);
  TBN_CHECK_LAUNCH("stft_rate_windows");
  return TBN_OK;
}

template <bool POWER>
static int stft_rate_launch(const float* wave, const float* const* windows, int nseg, int len, int win, int hop,
                            const float* twiddle, float* spec, float eps, hipStream_t st) {
  const int W = 1 + (len - 1) / hop;
  // 32-bit byte offsets inside a segment's samples and inside its 256 x W spectrogram
  TBN_REQUIRE(nseg <= 65535 && (size_t)len * 4 < (1ull << 31) && (size_t)STFT_BINS * W * 4 < (1ull << 31),
              "stft_rate_windows: too many segments / too long a waveform per call");
  return hop % 4 == 0 ? stft_rate_launch_as<POWER, true>(wave, windows, nseg, len, W, win, hop, twiddle, spec, eps, st)
                      : stft_rate_launch_as<POWER, false>(wave, windows, nseg, len, W, win, hop, twiddle, spec, eps, st);
}

extern "C" {

size_t tbn_stft_rate_twiddle_floats(int win) {
  return win >= 8 && win <= 511 ? (size_t)2 * cdiv(win, 8) * STFT_BINS * 8 : 0;
}

int tbn_stft_rate_make_twiddle(int win, float* host) {
  TBN_REQUIRE(host != nullptr, "stft_rate_make_twiddle: null buffer");
  TBN_REQUIRE(win >= 8 && win <= 511, "stft_rate_make_twiddle: window %d outside 8 .. 511 (n_fft = 511)", win);
  const double pi = 3.14159265358979323846;
  const int lpad = (511 - win) / 2;
  const size_t part = (size_t)cdiv(win, 8) * STFT_BINS * 8;
  memset(host, 0, 2 * part * sizeof(float));     // the taps win .. 8 * ceil(win / 8) - 1
  for (int j = 0; j < win; ++j) {
    const double h = 0.5 - 0.5 * cos(2.0 * pi * j / (double)win);
    for (int k = 0; k < STFT_BINS; ++k) {
      const long m = ((long)(j + lpad) * k) % 511;  // exact phase reduction
      const double a = 2.0 * pi * (double)m / 511.0;
      const size_t idx = ((size_t)(j / 8) * STFT_BINS + k) * 8 + (j % 8);
      host[idx] = (float)(h * cos(a));
      host[part + idx] = (float)(-h * sin(a));
    }
  }
  return TBN_OK;
}

int tbn_stft_rate_windows(const float* const* window_ptrs, const float* wave, int nseg, int len, int win, int hop,
                          const float* twiddle, float* out, float eps, int mode, const float* mel_basis, float* power,
                          void* stream) {
  TBN_REQUIRE((window_ptrs != nullptr) != (wave != nullptr),
              "stft_rate_windows: give a window table or a contiguous batch, not both");
  TBN_REQUIRE(twiddle && out && nseg > 0 && len > 0, "stft_rate_windows: bad argument");
  TBN_REQUIRE(stft_rate_geometry_ok(win, hop), "stft_rate_windows: window %d / hop %d outside 8 <= window <= 511, 1 <= hop <= window",
              win, hop);
  TBN_REQUIRE(mode == TBN_STFT_LOGPOWER || mode == TBN_STFT_LOGMEL, "stft_rate_windows: unknown mode %d", mode);
  hipStream_t st = (hipStream_t)stream;
  if (mode == TBN_STFT_LOGPOWER) return stft_rate_launch<false>(wave, window_ptrs, nseg, len, win, hop, twiddle, out, eps, st);
  TBN_REQUIRE(mel_basis && power && power != out, "stft_rate_windows: the log-mel mode needs the mel basis and a power workspace");
  const int W = 1 + (len - 1) / hop;
  const int rc = stft_rate_launch<true>(wave, window_ptrs, nseg, len, win, hop, twiddle, power, 0.f, st);
  if (rc != TBN_OK) return rc;
  tbn_prof_begin("mel_db_kernel", 0.0, st);
  TBN_LAUNCH(mel_db_kernel, dim3(nseg), dim3(MEL_THREADS), 0, st, (const float*)power, mel_basis, W, out);
  tbn_prof_end(st);
  TBN_CHECK_LAUNCH("stft_rate_windows (mel)");
  return TBN_OK;
}

size_t tbn_stft_twiddle_floats(void) { return (size_t)2 * STFT_KG * STFT_BINS * 8; }

int tbn_stft_make_twiddle(float* host) {
  TBN_REQUIRE(host != nullptr, "stft_make_twiddle: null buffer");
  const double pi = 3.14159265358979323846;
  const size_t part = (size_t)STFT_KG * STFT_BINS * 8;
  for (int j = 0; j < STFT_TAPS; ++j) {
    const double h = 0.5 - 0.5 * cos(2.0 * pi * j / 240.0);
    for (int k = 0; k < STFT_BINS; ++k) {
      const long m = ((long)(j + 135) * k) % 511;  // exact phase reduction
      const double a = 2.0 * pi * (double)m / 511.0;
      const size_t idx = ((size_t)(j / 8) * STFT_BINS + k) * 8 + (j % 8);
      host[idx] = (float)(h * cos(a));
      host[part + idx] = (float)(-h * sin(a));
    }
  }
  return TBN_OK;
}

int tbn_stft_logpower(const float* wave, int nseg, int len, const float* twiddle, float* spec, float eps,
                      void* stream) {
  TBN_REQUIRE(wave && twiddle && spec && nseg > 0 && len > 0, "stft_logpower: bad argument");
  return stft_launch<false>("stft_logpower", wave, nullptr, nseg, len, twiddle, spec, eps, false, (hipStream_t)stream);
}

int tbn_stft_windows(const float* const* window_ptrs, const float* wave, int nseg, int len, const float* twiddle,
                     float* out, float eps, int mode, const float* mel_basis, float* power, void* stream) {
  TBN_REQUIRE((window_ptrs != nullptr) != (wave != nullptr), "stft_windows: give a window table or a contiguous batch, not both");
  TBN_REQUIRE(twiddle && out && nseg > 0 && len > 0, "stft_windows: bad argument");
  TBN_REQUIRE(mode == TBN_STFT_LOGPOWER || mode == TBN_STFT_LOGMEL, "stft_windows: unknown mode %d", mode);
  hipStream_t st = (hipStream_t)stream;
  if (mode == TBN_STFT_LOGPOWER)
    return stft_launch<false>("stft_windows", wave, window_ptrs, nseg, len, twiddle, out, eps, true, st);
  TBN_REQUIRE(mel_basis && power && power != out, "stft_windows: the log-mel mode needs the mel basis and a power workspace");
  const int W = 1 + (len - 1) / 120;
  const int rc = stft_launch<true>("stft_windows", wave, window_ptrs, nseg, len, twiddle, power, 0.f, true, st);
  if (rc != TBN_OK) return rc;
  tbn_prof_begin("mel_db_kernel", 0.0, st);
  TBN_LAUNCH(mel_db_kernel, dim3(nseg), dim3(MEL_THREADS), 0, st, (const float*)power, mel_basis, W, out);
  tbn_prof_end(st);
  TBN_CHECK_LAUNCH("stft_windows (mel)");
  return TBN_OK;
}

int tbn_attn_prior_loud(const float* spec, int nseg, int F, int W, int T, const float* gauss, float* out, void* stream) {
  TBN_REQUIRE(spec && gauss && out && nseg > 0 && F > 0 && T > 0, "attn_prior_loud: bad argument");
  TBN_REQUIRE(W >= T, "attn_prior_loud: no full block of %d frames in a spectrogram %d frames wide", T, W);
  TBN_REQUIRE(W <= PRIOR_MAX_W && (size_t)F * W < (1ull << 31), "attn_prior_loud: spectrogram %d x %d too large", F, W);
  hipStream_t st = (hipStream_t)stream;
  tbn_prof_begin("attn_prior_loud_kernel", 0.0, st);
  TBN_LAUNCH(attn_prior_loud_kernel, dim3(nseg), dim3(64), 0, st, spec, F, W, T, gauss, out);
  tbn_prof_end(st);
  TBN_CHECK_LAUNCH("attn_prior_loud");
  return TBN_OK;
}

}  // extern "C"
