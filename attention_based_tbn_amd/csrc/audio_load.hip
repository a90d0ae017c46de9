// Audio files at any rate and sample format -> the mono float32 waveform at the target rate, on gfx950 (replaces the
// librosa.load(path, sr=data.audio.sampling_rate, mono=True) call of reference core/dataset/dataset.py:401-414 and
// preprocessing/create_audio_pickle.py:47-49: libsndfile's sample decode, librosa.to_mono, resampy's `kaiser_best`
// windowed-sinc resampler, librosa's fix_length).
//
// The raw interleaved PCM bytes of the file's data chunk go to the device as they are; ONE launch decodes, downmixes,
// filters and zeroes the padded tail sample.
//
//   decode     u8 (b - 128) / 128, s16 / 32768, s24 / 8388608, s32 / 2147483648, f32 as is (what libsndfile hands
//              librosa as float32); little endian;
//   downmix    float32 sum of the channels in channel order, divided by the channel count; one channel as is;
//   resample   output t sits at input position t * sr_orig / sr_new = n + fr (exact integer arithmetic, 64 bit: no drifting
//              time register).  resampy walks a left wing over x[n - i] and a right wing over x[n + 1 + i] through an
//              interpolated table of 32769 filter samples; the weights depend on t only through r = t mod L,
//              L = sr_new / gcd, so they are a POLYPHASE BANK of L rows of 2W weights (W = ceil(32769 / step)), built once
//              per ratio on the host in float64 (audio_bank_build below) and rounded to float32.  Tap k of the bank multiplies
//              x[n - W + 1 + k]: k < W is left-wing tap W - 1 - k, k >= W is right-wing tap k - W; shorter wings are zeros.
//
// Kernel: one workgroup of 256 threads per tile of AUDIO_TILE = 1024 consecutive outputs.  The tile's input span
// ((AUDIO_TILE - 1) * sr_orig / sr_new + 2 + 2W frames at most) is decoded and downmixed ONCE into LDS as float32, zeros
// outside the clip (resampy drops those taps); each thread owns four outputs 256 apart (four independent accumulators) and
// walks the 2W taps in tap order: a fixed summation order, the same bits every run.  The bank is laid out [tap][L]:
// neighbouring lanes (consecutive t, consecutive r) read neighbouring weights; with L = 1 the weight of a tap is
// wave-uniform and comes through the scalar cache, one load per four multiply-adds.  PCM reads are per sample at the
// sample's own width (s24 frames are 3, 6, 9 ... bytes: three byte loads per sample); a tile re-reads only the 2W frames of
// its halo.  With sr_orig == sr_new nothing is filtered: a plain decode / downmix kernel, one thread per frame.
#include <cmath>
#include <cstring>
#include <vector>

#include "tbn_kernels.h"
#include "../../include/tbn_hip.h"

#define AUDIO_TILE 1024
#define AUDIO_THREADS 256
#define AUDIO_PER_THREAD (AUDIO_TILE / AUDIO_THREADS)
#define AUDIO_MAX_CHANNELS 8
#define AUDIO_LDS_BYTES 65536       // the span of one tile must fit: a down-sampling ratio of about 12 at most
#define AUDIO_BANK_MAX_BYTES (64ull << 20)

// resampy 0.2.2 `kaiser_best`, quoted from memory and NOT verified against the library: kept in one place
#define RS_NUM_ZEROS 64
#define RS_NUM_TABLE 512
#define RS_ROLLOFF 0.9475937167399596
#define RS_BETA 14.769656459379492
#define RS_NWIN (RS_NUM_ZEROS * RS_NUM_TABLE + 1)     // 32769 samples of the right half of the filter

// one frame of interleaved PCM -> its mono float32 sample
template <int FORMAT>
__device__ __forceinline__ float audio_sample(const unsigned char* __restrict__ p) {
  if (FORMAT == TBN_AUDIO_U8) return (float)((int)p[0] - 128) * (1.0f / 128.0f);
  if (FORMAT == TBN_AUDIO_S16) return (float)*reinterpret_cast<const short*>(p) * (1.0f / 32768.0f);
  if (FORMAT == TBN_AUDIO_S24) {
    const int v = (int)p[0] | ((int)p[1] << 8) | ((int)(signed char)p[2] << 16);
    return (float)v * (1.0f / 8388608.0f);
  }
  if (FORMAT == TBN_AUDIO_S32) return (float)*reinterpret_cast<const int*>(p) * (1.0f / 2147483648.0f);
  return *reinterpret_cast<const float*>(p);
}

template <int FORMAT>
__device__ __forceinline__ float audio_frame(const unsigned char* __restrict__ pcm, long long frame, int channels) {
  constexpr int width = FORMAT == TBN_AUDIO_U8 ? 1 : FORMAT == TBN_AUDIO_S16 ? 2 : FORMAT == TBN_AUDIO_S24 ? 3 : 4;
  const unsigned char* p = pcm + (size_t)frame * (size_t)(channels * width);
  float s = audio_sample<FORMAT>(p);
  if (channels == 1) return s;
  for (int c = 1; c < channels; ++c) s += audio_sample<FORMAT>(p + c * width);
  return s / (float)channels;
}

template <int FORMAT>
__global__ __launch_bounds__(AUDIO_THREADS) void audio_decode_kernel(const unsigned char* __restrict__ pcm, long long frames,
                                                                     int channels, float* __restrict__ out) {
  const long long f = (long long)blockIdx.x * AUDIO_THREADS + threadIdx.x;
  if (f < frames) out[f] = audio_frame<FORMAT>(pcm, f, channels);
}

// UNIFORM: L == 1, the weight of tap k is bank[k] for every output
template <int FORMAT, bool UNIFORM>
__global__ __launch_bounds__(AUDIO_THREADS) void audio_load_kernel(const unsigned char* __restrict__ pcm, long long frames,
                                                                   int channels, long long sr_orig, long long sr_new, int W,
                                                                   int L, int span, const float* __restrict__ bank,
                                                                   float* __restrict__ out, long long n_out, long long out_len) {
  extern __shared__ __attribute__((aligned(16))) float xs[];   // span floats: frames base .. base + span - 1 of the mono signal
  const int tid = threadIdx.x;
  const long long t0 = (long long)blockIdx.x * AUDIO_TILE;
  const long long n0 = (t0 * sr_orig) / sr_new;
  const long long base = n0 - W + 1;
  for (int i = tid; i < span; i += AUDIO_THREADS) {
    const long long f = base + i;
    xs[i] = (f >= 0 && f < frames) ? audio_frame<FORMAT>(pcm, f, channels) : 0.f;
  }
  int li[AUDIO_PER_THREAD], r[AUDIO_PER_THREAD];
#pragma unroll
  for (int j = 0; j < AUDIO_PER_THREAD; ++j) {
    const long long t = t0 + tid + j * AUDIO_THREADS;
    // outputs past n_out (the padded tail, and the rest of the last tile) filter nothing: they read the start of the span
    const bool live = t < n_out;
    li[j] = live ? (int)((t * sr_orig) / sr_new - n0) : 0;     // <= (AUDIO_TILE - 1) * sr_orig / sr_new + 1 = span - 2W - 1
    r[j] = live && !UNIFORM ? (int)(t % L) : 0;
  }
  __syncthreads();
  float acc[AUDIO_PER_THREAD];
#pragma unroll
  for (int j = 0; j < AUDIO_PER_THREAD; ++j) acc[j] = 0.f;
  const int taps = 2 * W;
  if (UNIFORM) {
#pragma unroll 4
    for (int k = 0; k < taps; ++k) {
      const float w = bank[k];
#pragma unroll
      for (int j = 0; j < AUDIO_PER_THREAD; ++j) acc[j] = fmaf(w, xs[li[j] + k], acc[j]);
    }
  } else {
#pragma unroll 2
    for (int k = 0; k < taps; ++k) {
      const float* __restrict__ row = bank + (size_t)k * L;
#pragma unroll
      for (int j = 0; j < AUDIO_PER_THREAD; ++j) acc[j] = fmaf(row[r[j]], xs[li[j] + k], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < AUDIO_PER_THREAD; ++j) {
    const long long t = t0 + tid + j * AUDIO_THREADS;
    if (t < out_len) out[t] = t < n_out ? acc[j] : 0.f;        // librosa's fix_length: at most one sample, exactly 0
  }
}

// ---------------------------------------------------------------------------------------------- host: geometry and bank
static long long audio_gcd(long long a, long long b) {
  while (b) {
    const long long c = a % b;
    a = b;
    b = c;
  }
  return a;
}

struct AudioGeometry {
  int W, L, step;
  double scale, ratio;
  size_t floats;
};

// false: a rate is not positive; W / L / floats may be huge (the caller refuses the bank size)
static bool audio_geometry(int sr_orig, int sr_new, AudioGeometry* g) {
  if (sr_orig <= 0 || sr_new <= 0) return false;
  g->ratio = (double)sr_new / (double)sr_orig;
  g->scale = g->ratio < 1.0 ? g->ratio : 1.0;
  g->step = (int)(g->scale * RS_NUM_TABLE);       // truncated: resampy's own quirk (44100 -> 24000: 278, not 278.6)
  if (g->step < 1) {
    g->W = 0;
    g->L = 0;
    g->floats = ~(size_t)0;
    return true;
  }
  g->W = (RS_NWIN + g->step - 1) / g->step;
  g->L = (int)(sr_new / audio_gcd(sr_orig, sr_new));
  g->floats = (size_t)2 * g->W * (size_t)g->L;
  return true;
}

// modified Bessel function of the first kind, order 0, by its power series (all terms positive: no cancellation)
static double audio_bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < sum * 1e-18) break;
  }
  return sum;
}

static void audio_bank_build(int sr_orig, int sr_new, const AudioGeometry& g, float* bank) {
#pragma clang fp contract(off)
  const double pi = 3.14159265358979323846;
  const int n = RS_NUM_ZEROS * RS_NUM_TABLE;
  std::vector<double> win(RS_NWIN), delta(RS_NWIN);
  const double i0_beta = audio_bessel_i0(RS_BETA);
  for (int j = 0; j <= n; ++j) {
    const double a = (double)j / (double)n;
    const double kaiser = audio_bessel_i0(RS_BETA * sqrt(1.0 - a * a)) / i0_beta;
    const double u = RS_ROLLOFF * ((double)j / RS_NUM_TABLE);
    const double sinc = j == 0 ? 1.0 : sin(pi * u) / (pi * u);
    win[j] = kaiser * RS_ROLLOFF * sinc;
    if (g.ratio < 1.0) win[j] *= g.ratio;
  }
  for (int j = 0; j < n; ++j) delta[j] = win[j + 1] - win[j];
  delta[n] = 0.0;
  const int W = g.W, L = g.L;
  memset(bank, 0, g.floats * sizeof(float));
  for (int r = 0; r < L; ++r) {
    const long long pos = (long long)r * sr_orig;
    const double fr = (double)(pos % sr_new) / (double)sr_new;
    for (int wing = 0; wing < 2; ++wing) {
      const double frac = wing == 0 ? g.scale * fr : g.scale - g.scale * fr;
      const double idx = frac * RS_NUM_TABLE;
      const int off = (int)idx;
      const double eta = idx - off;
      const int count = (RS_NWIN - off) / g.step;
      for (int i = 0; i < count; ++i) {
        const double w = win[off + i * g.step] + eta * delta[off + i * g.step];
        const int k = wing == 0 ? W - 1 - i : W + i;
        bank[(size_t)k * L + r] = (float)w;
      }
    }
  }
}

template <int FORMAT>
static void audio_launch(const unsigned char* pcm, long long frames, int channels, int sr_orig, int sr_new,
                         const AudioGeometry& g, int span, const float* bank, float* out, long long n_out, long long out_len,
                         hipStream_t st) {
  if (sr_orig == sr_new) {
    tbn_prof_begin("audio_decode_kernel", 0.0, st, (double)frames * 4.0);
    TBN_LAUNCH(audio_decode_kernel<FORMAT>, dim3((unsigned)((frames + AUDIO_THREADS - 1) / AUDIO_THREADS)), dim3(AUDIO_THREADS),
               0, st, pcm, frames, channels, out);
    tbn_prof_end(st);
    return;
  }
  const dim3 grid((unsigned)((out_len + AUDIO_TILE - 1) / AUDIO_TILE));
  const size_t lds = (size_t)span * sizeof(float);
  tbn_prof_begin(g.L == 1 ? "audio_load_kernel<uniform>" : "audio_load_kernel<phases>", 4.0 * g.W * (double)n_out, st);
  if (g.L == 1)
    TBN_LAUNCH((audio_load_kernel<FORMAT, true>), grid, dim3(AUDIO_THREADS), lds, st, pcm, frames, channels, (long long)sr_orig,
               (long long)sr_new, g.W, g.L, span, bank, out, n_out, out_len);
  else
    TBN_LAUNCH((audio_load_kernel<FORMAT, false>), grid, dim3(AUDIO_THREADS), lds, st, pcm, frames, channels, (long long)sr_orig,
               (long long)sr_new, g.W, g.L, span, bank, out, n_out, out_len);
  tbn_prof_end(st);
}

extern "C" {

int tbn_audio_tile(void) { return AUDIO_TILE; }

int tbn_audio_bank_geometry(int sr_orig, int sr_new, int* taps, int* phases, size_t* floats) {
  TBN_REQUIRE(taps && phases && floats, "audio_bank_geometry: null out");
  AudioGeometry g;
  TBN_REQUIRE(audio_geometry(sr_orig, sr_new, &g), "audio_bank_geometry: sampling rates %d -> %d must be positive", sr_orig,
              sr_new);
  if (sr_orig == sr_new) {      // nothing is filtered: no bank
    *taps = 0;
    *phases = 0;
    *floats = 0;
    return TBN_OK;
  }
  TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, g.step >= 1 && g.floats * sizeof(float) <= AUDIO_BANK_MAX_BYTES,
                 "audio_bank_geometry: the polyphase bank of %d -> %d Hz (%d phases of %d taps) would pass 64 MiB", sr_orig,
                 sr_new, g.L, 2 * g.W);
  *taps = 2 * g.W;
  *phases = g.L;
  *floats = g.floats;
  return TBN_OK;
}

int tbn_audio_make_bank(int sr_orig, int sr_new, float* host_buffer, size_t floats) {
  int taps, phases;
  size_t need;
  const int rc = tbn_audio_bank_geometry(sr_orig, sr_new, &taps, &phases, &need);
  if (rc != TBN_OK) return rc;
  TBN_REQUIRE(need > 0, "audio_make_bank: %d -> %d Hz needs no bank", sr_orig, sr_new);
  TBN_REQUIRE(host_buffer != nullptr && floats == need, "audio_make_bank: the buffer holds %zu floats, the bank of %d -> %d Hz has %zu",
              floats, sr_orig, sr_new, need);
  AudioGeometry g;
  audio_geometry(sr_orig, sr_new, &g);
  audio_bank_build(sr_orig, sr_new, g, host_buffer);
  return TBN_OK;
}

int tbn_audio_load(const void* pcm, size_t pcm_bytes, long long frames, int channels, int format, int sr_orig, int sr_new,
                   const float* bank, float* out, long long out_len, void* stream) {
  TBN_REQUIRE(format >= TBN_AUDIO_U8 && format <= TBN_AUDIO_F32, "audio_load: unknown sample format code %d", format);
  TBN_REQUIRE(channels >= 1 && channels <= AUDIO_MAX_CHANNELS, "audio_load: %d channels, 1..%d are read", channels,
              AUDIO_MAX_CHANNELS);
  TBN_REQUIRE(sr_orig > 0 && sr_new > 0, "audio_load: sampling rates %d -> %d must be positive", sr_orig, sr_new);
  TBN_REQUIRE(frames > 0, "audio_load: %lld frames", frames);
  // frames * sr_new, t * sr_orig (t < out_len) and the byte offsets of the frames stay inside int64
  const long long big = sr_orig > sr_new ? sr_orig : sr_new;
  TBN_REQUIRE(frames <= (0x7fffffffffffffffLL / big) - 2 && frames <= 0x7fffffffffffffffLL / (4 * AUDIO_MAX_CHANNELS),
              "audio_load: %lld frames at %d -> %d Hz overflow 64-bit positions", frames, sr_orig, sr_new);
  const int width = format == TBN_AUDIO_U8 ? 1 : format == TBN_AUDIO_S16 ? 2 : format == TBN_AUDIO_S24 ? 3 : 4;
  TBN_REQUIRE(pcm_bytes == (size_t)frames * (size_t)(channels * width),
              "audio_load: %zu bytes of PCM, but %lld frames of %d channels x %d bytes are %zu", pcm_bytes, frames, channels, width,
              (size_t)frames * (size_t)(channels * width));
  const long long n_out = (frames * sr_new) / sr_orig;
  const long long want = n_out + ((frames * sr_new) % sr_orig != 0);
  TBN_REQUIRE(out_len == want, "audio_load: out_len %lld, but %lld frames at %d -> %d Hz give ceil(frames * sr_new / sr_orig) = %lld",
              out_len, frames, sr_orig, sr_new, want);
  TBN_REQUIRE(pcm != nullptr && out != nullptr, "audio_load: null pointer");
  TBN_REQUIRE(((uintptr_t)pcm & 3) == 0 && ((uintptr_t)out & 3) == 0, "audio_load: pcm and out must be 4-byte aligned");
  AudioGeometry g;
  audio_geometry(sr_orig, sr_new, &g);
  int span = 0;
  if (sr_orig != sr_new) {
    TBN_REQUIRE(bank != nullptr, "audio_load: %d -> %d Hz resamples, which needs the bank of tbn_audio_make_bank", sr_orig, sr_new);
    TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, g.step >= 1 && g.floats * sizeof(float) <= AUDIO_BANK_MAX_BYTES,
                   "audio_load: the polyphase bank of %d -> %d Hz would pass 64 MiB", sr_orig, sr_new);
    const long long s = ((long long)(AUDIO_TILE - 1) * sr_orig) / sr_new + 2 + 2LL * g.W;
    TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, s * (long long)sizeof(float) <= AUDIO_LDS_BYTES,
                   "audio_load: %d -> %d Hz: one tile of %d outputs spans %lld input frames, more than the %d the kernel stages",
                   sr_orig, sr_new, AUDIO_TILE, s, AUDIO_LDS_BYTES / 4);
    TBN_REQUIRE((out_len + AUDIO_TILE - 1) / AUDIO_TILE <= 0x7fffffffLL, "audio_load: %lld outputs are too many tiles", out_len);
    span = (int)s;
  } else {
    TBN_REQUIRE((frames + AUDIO_THREADS - 1) / AUDIO_THREADS <= 0x7fffffffLL, "audio_load: %lld frames are too many blocks", frames);
  }
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* p = (const unsigned char*)pcm;
  switch (format) {
    case TBN_AUDIO_U8: audio_launch<TBN_AUDIO_U8>(p, frames, channels, sr_orig, sr_new, g, span, bank, out, n_out, out_len, st); break;
    case TBN_AUDIO_S16: audio_launch<TBN_AUDIO_S16>(p, frames, channels, sr_orig, sr_new, g, span, bank, out, n_out, out_len, st); break;
    case TBN_AUDIO_S24: audio_launch<TBN_AUDIO_S24>(p, frames, channels, sr_orig, sr_new, g, span, bank, out, n_out, out_len, st); break;
    case TBN_AUDIO_S32: audio_launch<TBN_AUDIO_S32>(p, frames, channels, sr_orig, sr_new, g, span, bank, out, n_out, out_len, st); break;
    default: audio_launch<TBN_AUDIO_F32>(p, frames, channels, sr_orig, sr_new, g, span, bank, out, n_out, out_len, st); break;
  }
  TBN_CHECK_LAUNCH("audio_load");
  return TBN_OK;
}

}  // extern "C"
