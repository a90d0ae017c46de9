// C-ABI glue: error reporting and the single-operator entry points of include/tbn_hip.h.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tbn_common.h"
#include "tbn_kernels.h"
#include "../../include/tbn_hip.h"

static thread_local char g_err[512] = "";

void tbn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#if TBN_EXPERIMENT
int tbn_env_int(const char* name, int def, int lo, int hi) {
  const char* e = getenv(name);
  if (e == nullptr || *e == 0) return def;
  char* end = nullptr;
  const long v = strtol(e, &end, 10);
  if (end == e || *end != 0 || v < lo || v > hi) {
    fprintf(stderr, "[tbn] experiment knob %s=%s ignored (expected an integer in [%d, %d]); using %d\n", name, e, lo, hi, def);
    return def;
  }
  if ((int)v != def) fprintf(stderr, "[tbn] experiment knob %s=%ld active (default %d): not the shipped configuration\n", name, v, def);
  return (int)v;
}
#endif

static void conv_geom(ConvP* p, int n, int h, int w, int cin, int cout, int k, int stride, int pad) {
  memset(p, 0, sizeof(*p));
  p->N = n;
  p->H = h;
  p->W = w;
  p->OH = (h + 2 * pad - k) / stride + 1;
  p->OW = (w + 2 * pad - k) / stride + 1;
  p->Cin = cin;
  p->Cout = cout;
  p->R = p->S = k;
  p->stride = stride;
  p->pad = pad;
  p->up = 1;
  p->M = n * p->OH * p->OW;
  p->K = k * k * cin;
}

// ------------------------------------------------------------------ in-process conv-GEMM profiler
#include <map>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>
namespace {
struct ProfRec {
  int name;
  double flops, bytes;
  hipEvent_t a, b;
  bool used;      // a launch took the events (hipExtLaunchKernelGGL wrote the kernel's begin / end timestamps into them)
};
struct ProfAgg {
  long launches = 0;
  double ms = 0, flops = 0, bytes = 0;
};
std::mutex g_prof_mu;
bool g_prof_on = false;
bool g_prof_layers = false;   // enable(2): key = "kernel | layer label"
std::string g_prof_label;
thread_local const char* g_prof_prefix = nullptr;   // "linear: " while a head Linear entry point launches (bench.py keeps
                                                    // the BN-Inception conv stage and the head GEMMs apart)
std::vector<std::string> g_prof_names;
std::vector<ProfRec> g_prof_recs;
std::vector<hipEvent_t> g_prof_pool;
std::map<std::string, ProfAgg> g_prof_agg;
std::vector<std::string> g_prof_keys;
int g_prof_open = -1;

hipEvent_t prof_event() {
  if (!g_prof_pool.empty()) {
    hipEvent_t e = g_prof_pool.back();
    g_prof_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);   // a failed create leaves nullptr: the record / elapsed calls below then report 0 ms
  return e;
}
void prof_collect() {
  for (auto& r : g_prof_recs) {
    if (r.used) {
      (void)hipEventSynchronize(r.b);
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, r.a, r.b);
      ProfAgg& a = g_prof_agg[g_prof_names[r.name]];
      a.launches += 1;
      a.ms += ms;
      a.flops += r.flops;
      a.bytes += r.bytes;
    }
    g_prof_pool.push_back(r.a);
    g_prof_pool.push_back(r.b);
  }
  g_prof_recs.clear();
  g_prof_keys.clear();
  for (auto& kv : g_prof_agg) g_prof_keys.push_back(kv.first);
}
}  // namespace

void tbn_prof_begin(const char* kernel, double flops, hipStream_t st, double bytes) {
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  std::string key = g_prof_prefix ? std::string(g_prof_prefix) + kernel : std::string(kernel);
  if (g_prof_layers) key += " | " + g_prof_label;
  kernel = key.c_str();
  int idx = -1;
  for (size_t i = 0; i < g_prof_names.size(); ++i)
    if (g_prof_names[i] == kernel) idx = (int)i;
  if (idx < 0) {
    g_prof_names.push_back(kernel);
    idx = (int)g_prof_names.size() - 1;
  }
  ProfRec r;
  r.name = idx;
  r.flops = flops;
  r.bytes = bytes;
  r.a = prof_event();
  r.b = prof_event();
  r.used = false;
  (void)st;
  g_prof_recs.push_back(r);
  g_prof_open = (int)g_prof_recs.size() - 1;
}
bool tbn_prof_enabled() { return g_prof_on; }

// ---- kernel timeline
namespace {
struct TlRec {
  std::string name;
  void* stream;
  hipEvent_t a, b;
};
std::mutex g_tl_mu;
std::atomic<bool> g_tl_on{false};   // read by every launch, from every host thread that drives a backbone stream
std::vector<TlRec> g_tl;
void tl_free_events() {             // caller holds g_tl_mu
  for (auto& r : g_tl) {
    if (r.a) (void)hipEventDestroy(r.a);
    if (r.b) (void)hipEventDestroy(r.b);
  }
  g_tl.clear();
}
}  // namespace
// A launch takes the timeline path only outside stream captures: an event-carrying dispatch inside hipStreamBeginCapture
// invalidates the capture (TrainStep / scripts/graph_experiment.py capture whole steps) -- such launches are simply not
// on the timeline (round-5 advisor).
bool tbn_tl_on(hipStream_t st) {
  if (!g_tl_on.load(std::memory_order_relaxed)) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return cs == hipStreamCaptureStatusNone;
}
void tbn_tl_events(const char* name, hipStream_t st, hipEvent_t* start, hipEvent_t* stop) {
  std::lock_guard<std::mutex> lk(g_tl_mu);
  TlRec r;
  r.name = name;
  r.stream = (void*)st;
  r.a = r.b = nullptr;
  (void)hipEventCreate(&r.a);
  (void)hipEventCreate(&r.b);
  *start = r.a;
  *stop = r.b;
  g_tl.push_back(r);
}
// enable(1) starts a fresh recording; enable(0) stops it and keeps the records for tbn_timeline_dump, which frees them
// (their events included) once written -- a disabled, dumped timeline holds no events
extern "C" int tbn_timeline_enable(int on) {
  std::lock_guard<std::mutex> lk(g_tl_mu);
  if (on) {
    (void)hipDeviceSynchronize();   // no launch of an earlier recording may still carry the events freed here
    tl_free_events();
  }
  g_tl_on.store(on != 0, std::memory_order_relaxed);
  return TBN_OK;
}
extern "C" int tbn_timeline_dump(const char* path) {
  TBN_REQUIRE(path != nullptr, "timeline_dump: null path");
  (void)hipDeviceSynchronize();
  std::lock_guard<std::mutex> lk(g_tl_mu);
  FILE* f = fopen(path, "w");
  TBN_REQUIRE(f != nullptr, "timeline_dump: cannot open %s", path);
  fprintf(f, "Kernel_Name,Queue_Id,Start_Timestamp,End_Timestamp\n");
  if (!g_tl.empty()) {
    // common clock: nanoseconds after the first recorded launch began (kernels of other streams may have begun earlier)
    const hipEvent_t ref = g_tl[0].a;
    for (auto& r : g_tl) {
      float a = 0.f, d = 0.f;
      if (hipEventElapsedTime(&a, ref, r.a) != hipSuccess || hipEventElapsedTime(&d, r.a, r.b) != hipSuccess) {
        (void)hipGetLastError();
        continue;
      }
      std::string nm = r.name;
      for (auto& ch : nm)
        if (ch == ',' || ch == '"') ch = ';';
      const long long s0 = (long long)((double)a * 1e6) + 1000000000ll;
      fprintf(f, "%s,%p,%lld,%lld\n", nm.c_str(), r.stream, s0, s0 + (long long)((double)d * 1e6));
    }
  }
  fclose(f);
  if (!g_tl_on.load(std::memory_order_relaxed)) tl_free_events();   // device is idle (synchronised above), recording is off
  return TBN_OK;
}
bool tbn_prof_launch_events(hipEvent_t* start, hipEvent_t* stop) {
  if (!g_prof_on) return false;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (g_prof_open < 0 || g_prof_recs[g_prof_open].used || !g_prof_recs[g_prof_open].a || !g_prof_recs[g_prof_open].b)
    return false;
  g_prof_recs[g_prof_open].used = true;
  *start = g_prof_recs[g_prof_open].a;
  *stop = g_prof_recs[g_prof_open].b;
  return true;
}
void tbn_prof_label(const char* label) {
  if (!g_prof_on || !g_prof_layers) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_label = label;
}
void tbn_prof_end(hipStream_t st) {
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  (void)st;
  g_prof_open = -1;
}

// Box calibration (bench.py `box.mfma_calibration`): a pure v_mfma_f32_32x32x2_f32 loop, operands in registers, no memory
// traffic -- what THIS device sustains on the instruction the roofline is priced in (157.3 TFLOP/s nominal; boxes of one
// pool differ by a few per cent in the clock they hold).  Four rotating accumulators: a dependent MFMA is only free right
// behind its producer or >= 4 MFMAs later (hardware finding 2).
__global__ __launch_bounds__(256) void mfma_burst_kernel(float* sink, int iters) {
  f32x16 a0, a1, a2, a3;
#pragma unroll
  for (int e = 0; e < 16; ++e) a0[e] = a1[e] = a2[e] = a3[e] = 0.f;
  const float x = 1e-3f * (float)(threadIdx.x & 63) + 0.5f, y = 1.0f - 1e-3f * (float)(threadIdx.x >> 6);
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(y, x, a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, x, a2, 0, 0, 0);
      a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(y, y, a3, 0, 0, 0);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) s += (a0[e] + a1[e]) + (a2[e] + a3[e]);
  if (s == -1.2345f) sink[0] = s;   // never true (all terms are positive): keeps the loop alive without a store
}

extern "C" {

int tbn_version(void) { return 102 | (TBN_EXPERIMENT ? 0x10000 : 0); }

int tbn_capabilities(void) { return TBN_CAP_CONV_BF16X | TBN_CAP_CONV_BF16X_PLANES | TBN_CAP_FRAMES_CROPS | TBN_CAP_ATTN_GENERAL | TBN_CAP_ATTN_REG | TBN_CAP_AUDIO_LAYER | TBN_CAP_STEM_OPS | TBN_CAP_BN_BATCH_OPS; }

int tbn_diag_mfma_burst(float* sink, int workgroups, int iters, double* flops, void* stream) {
  TBN_REQUIRE(sink != nullptr && workgroups > 0 && workgroups <= 65536 && iters > 0, "diag_mfma_burst: bad argument");
  hipLaunchKernelGGL(mfma_burst_kernel, dim3(workgroups), dim3(256), 0, (hipStream_t)stream, sink, iters);
  TBN_CHECK_LAUNCH("mfma_burst");
  if (flops) *flops = (double)workgroups * 4.0 * (double)iters * 16.0 * 4096.0;   // 2 * 32 * 32 * 2 per MFMA
  return TBN_OK;
}

int tbn_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
  g_prof_layers = on == 2;
  return TBN_OK;
}
int tbn_profile_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  prof_collect();
  g_prof_agg.clear();
  g_prof_keys.clear();
  return TBN_OK;
}
int tbn_profile_num_entries(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  prof_collect();
  return (int)g_prof_keys.size();
}
int tbn_profile_entry(int i, char* name, int name_len, long* launches, double* total_ms, double* total_flops) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  TBN_REQUIRE(i >= 0 && i < (int)g_prof_keys.size() && name && name_len > 0, "profile_entry: bad index");
  const ProfAgg& a = g_prof_agg[g_prof_keys[i]];
  snprintf(name, name_len, "%s", g_prof_keys[i].c_str());
  if (launches) *launches = a.launches;
  if (total_ms) *total_ms = a.ms;
  if (total_flops) *total_flops = a.flops;
  return TBN_OK;
}
int tbn_profile_entry_bytes(int i, double* total_alg_bytes) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  TBN_REQUIRE(i >= 0 && i < (int)g_prof_keys.size() && total_alg_bytes, "profile_entry_bytes: bad index");
  *total_alg_bytes = g_prof_agg[g_prof_keys[i]].bytes;
  return TBN_OK;
}
const char* tbn_last_error(void) { return g_err; }

// the input pitch rule of every conv C-ABI entry (host only, ahead of any launch): every family forms its input offsets from
// the pitch and reads `channels` floats per pixel in float4 steps
static int conv_in_ld_ok(const char* who, int in_ld, int channels) {
  if (channels % 32 != 0) return TBN_OK;   // no kernel takes it: the launcher's channel rule refuses the launch in its own words
  TBN_REQUIRE(in_ld >= channels && in_ld % 4 == 0, "%s: in_ld %d (at least the %d input channels, a multiple of 4)", who, in_ld,
              channels);
  return TBN_OK;
}

int tbn_conv2d_stat_tiles(int n, int h, int w, int cin, int cout, int ksize, int stride, int pad) {
  ConvP p;
  conv_geom(&p, n, h, w, cin, cout, ksize, stride, pad);
  int mt, nt;
  tbn_conv_pick_tile(p.M, p.Cout, p.K, &mt, &nt);
  return cdiv(p.M, 128 * mt);
}

int tbn_conv2d_fwd(const float* in, int in_ld, const float* weight, const float* bias, float* out, int out_ld,
                   int n, int h, int w, int cin, int cout, int ksize, int stride, int pad, int epilogue, int flags,
                   const float* scale, const float* shift, float* stat_partial, void* stream) {
  TBN_REQUIRE(in && weight && out, "conv2d_fwd: null pointer");
  TBN_REQUIRE(epilogue >= 0 && epilogue <= 2, "conv2d_fwd: bad epilogue");
  TBN_REQUIRE(epilogue != CONV_EPI_STATS || stat_partial, "conv2d_fwd: stats epilogue needs stat_partial");
  TBN_REQUIRE(epilogue != CONV_EPI_EVAL || (scale && shift), "conv2d_fwd: eval epilogue needs scale/shift");
  // the split-K tile kernel writes one statistics row per 32*mt output rows, tbn_conv2d_stat_tiles() counts 128-row tiles:
  // only the explicit-tile entry point (tbn_conv2d_fwd_tile / tbn_conv_launch) may combine the two
  TBN_REQUIRE(!(epilogue == CONV_EPI_STATS && (flags & CONV_FLAG_SK4)),
              "conv2d_fwd: the split-K tile variant with the statistics epilogue needs an explicit tile (tbn_conv2d_fwd_tile)");
  TBN_TRY(conv_in_ld_ok("conv2d_fwd", in_ld, cin));
  ConvP p;
  conv_geom(&p, n, h, w, cin, cout, ksize, stride, pad);
  p.in = in;
  p.in_ld = in_ld;
  p.wt = weight;
  p.bias = bias;
  p.scale = scale;
  p.shift = shift;
  p.stat_partial = stat_partial;
  p.mode = epilogue;
  p.flags = flags;
  p.nseg = 1;
  p.seg[0].ptr = out;
  p.seg[0].ld = out_ld;
  p.seg[0].col_begin = 0;
  return tbn_launch_conv(p, 0, 0, 0, (hipStream_t)stream);
}

// test / tuning aid: forward conv with an explicit (mt, nt) tile (0,0 = heuristic)
int tbn_conv2d_fwd_tile(const float* in, int in_ld, const float* weight, const float* bias, float* out, int out_ld,
                        int n, int h, int w, int cin, int cout, int ksize, int stride, int pad, int epilogue, int flags,
                        float* stat_partial, int mt, int nt, void* stream) {
  TBN_TRY(conv_in_ld_ok("conv2d_fwd_tile", in_ld, cin));
  ConvP p;
  conv_geom(&p, n, h, w, cin, cout, ksize, stride, pad);
  p.in = in;
  p.in_ld = in_ld;
  p.wt = weight;
  p.bias = bias;
  p.stat_partial = stat_partial;
  p.mode = epilogue;
  p.flags = flags;
  p.nseg = 1;
  p.seg[0].ptr = out;
  p.seg[0].ld = out_ld;
  p.seg[0].col_begin = 0;
  return tbn_launch_conv(p, 0, mt, nt, (hipStream_t)stream);
}

int tbn_conv2d_dgrad(const float* dout, int dout_ld, const float* weight, float* din, int din_ld, int n, int h, int w,
                     int cin, int cout, int ksize, int stride, int pad, int accumulate, float* workspace,
                     void* stream) {
  TBN_REQUIRE(dout && weight && din && workspace, "conv2d_dgrad: null pointer");
  TBN_TRY(conv_in_ld_ok("conv2d_dgrad", dout_ld, cout));
  hipStream_t st = (hipStream_t)stream;
  TBN_TRY(tbn_launch_weight_flip_transpose(weight, workspace, cout, ksize * ksize, cin, st));
  const int oh = (h + 2 * pad - ksize) / stride + 1, ow = (w + 2 * pad - ksize) / stride + 1;
  ConvP p;
  memset(&p, 0, sizeof(p));
  p.in = dout;
  p.in_ld = dout_ld;
  p.wt = workspace;
  p.N = n;
  p.H = oh;
  p.W = ow;
  p.OH = h;
  p.OW = w;
  p.Cin = cout;
  p.Cout = cin;
  p.R = p.S = ksize;
  p.stride = 1;
  p.pad = ksize - 1 - pad;
  p.up = stride;
  p.M = n * h * w;
  p.K = ksize * ksize * cout;
  p.mode = CONV_EPI_PLAIN;
  p.flags = accumulate ? CONV_FLAG_ACCUM : 0;
  p.nseg = 1;
  p.seg[0].ptr = din;
  p.seg[0].ld = din_ld;
  p.seg[0].col_begin = 0;
  return tbn_launch_conv(p, 0, 0, 0, st);
}

// ---- descriptor form (test / tuning aid): every variant / tile / epilogue the engine can launch
static int desc_to_convp(const tbn_conv_desc* d, float* workspace, hipStream_t st, ConvP* pp) {
  ConvP& p = *pp;
  TBN_REQUIRE(d && d->in && d->weight && d->out, "conv_launch: null pointer");
  TBN_TRY(conv_in_ld_ok("conv_launch", d->in_ld, d->dgrad ? d->cout : d->cin));
  if (!d->dgrad) {
    TBN_REQUIRE(d->epilogue >= 0 && d->epilogue <= 2, "conv_launch: bad epilogue");
    TBN_REQUIRE(d->epilogue != CONV_EPI_STATS || d->stat_partial, "conv_launch: stats epilogue needs stat_partial");
    TBN_REQUIRE(d->epilogue != CONV_EPI_EVAL || (d->scale && d->shift), "conv_launch: eval epilogue needs scale/shift");
    TBN_REQUIRE(d->nred == 0, "conv_launch: the fused BN-backward reduce belongs to a data gradient");
    conv_geom(&p, d->n, d->h, d->w, d->cin, d->cout, d->ksize, d->stride, d->pad);
    p.in = d->in;
    p.in_ld = d->in_ld;
    p.wt = d->weight;
    p.bias = d->bias;
    p.scale = d->scale;
    p.shift = d->shift;
    p.stat_partial = d->stat_partial;
    p.mode = d->epilogue;
  } else {
    if (d->flags & (CONV_FLAG_BF16X6 | CONV_FLAG_BF16X3 | CONV_FLAG_BF16X_PLANES)) {
      tbn_set_error("conv_launch: the bf16x kernels (flags 32 / 64) compute forward convolutions only, not dgrad = 1");
      return TBN_ERR_UNSUPPORTED;
    }
    TBN_REQUIRE(workspace != nullptr, "conv_launch: a data gradient needs the flipped-weight workspace");
    TBN_REQUIRE(d->epilogue == 0 && d->nred >= 0 && d->nred <= TBN_CONV_MAXSEG, "conv_launch: data gradient: epilogue 0, nred <= 4");
    TBN_TRY(tbn_launch_weight_flip_transpose(d->weight, workspace, d->cout, d->ksize * d->ksize, d->cin, st));
    const int oh = (d->h + 2 * d->pad - d->ksize) / d->stride + 1, ow = (d->w + 2 * d->pad - d->ksize) / d->stride + 1;
    memset(&p, 0, sizeof(p));
    p.in = d->in;
    p.in_ld = d->in_ld;
    p.wt = workspace;
    p.N = d->n;
    p.H = oh;
    p.W = ow;
    p.OH = d->h;
    p.OW = d->w;
    p.Cin = d->cout;
    p.Cout = d->cin;
    p.R = p.S = d->ksize;
    p.stride = 1;
    p.pad = d->ksize - 1 - d->pad;
    p.up = d->stride;
    p.M = d->n * d->h * d->w;
    p.K = d->ksize * d->ksize * d->cout;
    p.mode = CONV_EPI_PLAIN;
    p.nred = d->nred;
    p.red_chan = d->red_stats_stride;
    for (int i = 0; i < d->nred; ++i) {
      TBN_REQUIRE(d->red[i].partial && d->red_stats, "conv_launch: reduce segment %d incomplete", i);
      p.red[i].y = d->red[i].y;
      p.red[i].y_ld = d->red[i].y_ld;
      p.red[i].partial = d->red[i].partial;
      p.red[i].stats = d->red_stats;
      p.red[i].col_begin = d->red[i].col_begin;
      p.red[i].C = d->red[i].channels;
      p.red[i].c_off = d->red[i].stat_offset;
    }
  }
  p.flags = d->flags & ~CONV_FLAG_DESC_OUT2;
  p.stages = d->stages;
  p.nseg = 1;
  p.seg[0].ptr = d->out;
  p.seg[0].ld = d->out_ld;
  p.seg[0].col_begin = 0;
  // the out2* fields were appended to the struct: they are only read under flag 256, which a caller built against the
  // shorter struct never sets
  if (d->flags & CONV_FLAG_DESC_OUT2) {   // forward: the columns from out2_col_begin on go to a second destination
    TBN_REQUIRE(d->out2 != nullptr && !d->dgrad && d->epilogue != CONV_EPI_STATS && d->out2_col_begin > 0 && d->out2_col_begin < d->cout,
                "conv_launch: a second output segment belongs to a forward launch with epilogue 0 / 2 and starts inside (0, cout)");
    p.nseg = 2;
    p.seg[1].ptr = d->out2;
    p.seg[1].ld = d->out2_ld;
    p.seg[1].col_begin = d->out2_col_begin;
    if (d->out2_raw && d->epilogue == CONV_EPI_EVAL) p.raw_seg1 = 2;
  }
  return TBN_OK;
}

// a weight tensor [cout][ksize][ksize][cin] a split-bf16 kernel can read (the shape rule at the layer's stride 1 and
// same-size padding) and a plane count
static bool planes_args_ok(int cout, int ksize, int cin, int np) {
  return cout > 0 && cin > 0 && bf16x_layer_kind(ksize, 1, ksize / 2, cin) != BF16X_LAYER_NONE && (np == 6 || np == 3);
}

size_t tbn_conv_weight_planes_bytes(int cout, int ksize, int cin, int np) {
  if (!planes_args_ok(cout, ksize, cin, np)) return 0;
  return tbn_bf16x_planes_bytes((size_t)cout * ksize * ksize * cin, np);
}

int tbn_conv_split_weights(const float* weight, int cout, int ksize, int cin, int np, void* planes, void* stream) {
  TBN_REQUIRE(weight && planes, "conv_split_weights: null pointer");
  TBN_REQUIRE(planes_args_ok(cout, ksize, cin, np),
              "conv_split_weights: bf16x weight planes need ksize 1 | 3, cin a multiple of 32 and np 6 | 3 (got ksize %d, cin %d, np %d)",
              ksize, cin, np);
  TBN_REQUIRE((((uintptr_t)weight | (uintptr_t)planes) & 15) == 0, "conv_split_weights: pointers must be 16-B aligned");
  static thread_local SplitTab tab;
  tab.n = 0;
  split_tab_push(tab, 0, 0, (size_t)cout * ksize * ksize * cin);
  return tbn_launch_bf16x_split(weight, planes, tab, np, (hipStream_t)stream);
}

int tbn_conv_partial_rows(const tbn_conv_desc* d, int mt, int pair) {
  if (!d || mt < 1) return 0;
  const int rows = ((d->flags & CONV_FLAG_SK4) && !pair ? 32 : 128) * mt;
  if (d->dgrad) return tbn_conv_red_rows(d->n, d->h, d->w, d->stride, d->ksize, d->pad, rows);
  const int oh = (d->h + 2 * d->pad - d->ksize) / d->stride + 1, ow = (d->w + 2 * d->pad - d->ksize) / d->stride + 1;
  return cdiv(d->n * oh * ow, rows);
}

int tbn_conv_launch(const tbn_conv_desc* d, int mt, int nt, float* workspace, void* stream) {
  ConvP p;
  TBN_TRY(desc_to_convp(d, workspace, (hipStream_t)stream, &p));
  // partial-sum epilogues write one row per M tile: the caller sized the buffers for an explicit tile
  TBN_REQUIRE(((d->dgrad ? d->nred == 0 : d->epilogue != CONV_EPI_STATS)) || (mt >= 1 && nt >= 1),
              "conv_launch: partial-sum epilogues need an explicit tile");
  return tbn_launch_conv(p, 0, mt, nt, (hipStream_t)stream);
}

int tbn_conv_launch_pair(const tbn_conv_desc* a, const tbn_conv_desc* b, int variant, int mt, int nt,
                         float* workspace_a, float* workspace_b, void* stream) {
  ConvP pa, pb;
  TBN_TRY(desc_to_convp(a, workspace_a, (hipStream_t)stream, &pa));
  TBN_TRY(desc_to_convp(b, workspace_b, (hipStream_t)stream, &pb));
  return tbn_launch_conv_pair(pa, pb, variant, mt, nt, (hipStream_t)stream);
}

static void wgrad_geom(WgradP* wp, int n, int h, int w, int cin, int cout, int k, int stride, int pad) {
  memset(wp, 0, sizeof(*wp));
  wp->N = n;
  wp->H = h;
  wp->W = w;
  wp->OH = (h + 2 * pad - k) / stride + 1;
  wp->OW = (w + 2 * pad - k) / stride + 1;
  wp->Cin = cin;
  wp->Cout = cout;
  wp->R = wp->S = k;
  wp->taps = k * k;
  wp->stride = stride;
  wp->pad = pad;
  wp->M = n * wp->OH * wp->OW;
}

size_t tbn_conv2d_wgrad_workspace_floats(int n, int h, int w, int cin, int cout, int ksize, int stride, int pad) {
  WgradP wp;
  wgrad_geom(&wp, n, h, w, cin, cout, ksize, stride, pad);
  return tbn_wgrad_workspace_floats(wp.M, cout, cin, ksize * ksize);
}

int tbn_conv2d_wgrad(const float* dout, int dout_ld, const float* in, int in_ld, float* dweight, int n, int h, int w,
                     int cin, int cout, int ksize, int stride, int pad, float* workspace, void* stream) {
  TBN_REQUIRE(dout && in && dweight, "conv2d_wgrad: null pointer");
  WgradP wp;
  wgrad_geom(&wp, n, h, w, cin, cout, ksize, stride, pad);
  wp.dy = dout;
  wp.dy_ld = dout_ld;
  wp.x = in;
  wp.x_ld = in_ld;
  return tbn_launch_wgrad(wp, 0, dweight, workspace, (hipStream_t)stream);
}

// the checks the two explicit-tile entries share (host only); `who` prefixes the message
static int wgrad_tile_args_ok(const char* who, int n, int h, int w, int cin, int cout, int ksize, int stride, int pad, int mt,
                              int nt) {
  TBN_REQUIRE(tbn_wgrad_tile_ok(mt, nt), "%s: tile %dx%d (mt 1 | 2 | 3 | 5, nt 1..3 without 5x3, or 0x0)", who, mt, nt);
  TBN_REQUIRE(n >= 1 && h >= 1 && w >= 1 && ksize >= 1 && stride >= 1 && pad >= 0 && h + 2 * pad >= ksize && w + 2 * pad >= ksize,
              "%s: bad shape (%d frames of %dx%d, filter %d / stride %d / pad %d)", who, n, h, w, ksize, stride, pad);
  TBN_REQUIRE(cin >= 4 && cout >= 4 && cin % 4 == 0 && cout % 4 == 0, "%s: cin %d / cout %d must be multiples of 4", who, cin, cout);
  return TBN_OK;
}

int tbn_conv2d_wgrad_tile(const float* dout, int dout_ld, const float* in, int in_ld, float* dweight, int n, int h, int w,
                          int cin, int cout, int ksize, int stride, int pad, int mt, int nt, float* workspace, void* stream) {
  TBN_REQUIRE(dout && in && dweight, "conv2d_wgrad_tile: null pointer");
  TBN_TRY(wgrad_tile_args_ok("conv2d_wgrad_tile", n, h, w, cin, cout, ksize, stride, pad, mt, nt));
  TBN_REQUIRE(dout_ld >= cout && dout_ld % 4 == 0, "conv2d_wgrad_tile: dout_ld %d (at least cout, a multiple of 4)", dout_ld);
  TBN_REQUIRE(in_ld >= cin && in_ld % 4 == 0, "conv2d_wgrad_tile: in_ld %d (at least cin, a multiple of 4)", in_ld);
  WgradP wp;
  wgrad_geom(&wp, n, h, w, cin, cout, ksize, stride, pad);
  wp.dy = dout;
  wp.dy_ld = dout_ld;
  wp.x = in;
  wp.x_ld = in_ld;
  wp.mt = mt;
  wp.nt = nt;
  return tbn_launch_wgrad(wp, 0, dweight, workspace, (hipStream_t)stream);
}

long long tbn_conv2d_wgrad_plan(int n, int h, int w, int cin, int cout, int ksize, int stride, int pad, int mt, int nt, int* out8) {
  TBN_REQUIRE(out8 != nullptr, "conv2d_wgrad_plan: null out");
  TBN_TRY(wgrad_tile_args_ok("conv2d_wgrad_plan", n, h, w, cin, cout, ksize, stride, pad, mt, nt));
  WgradP wp;
  wgrad_geom(&wp, n, h, w, cin, cout, ksize, stride, pad);
  wp.mt = mt;
  wp.nt = nt;
  const WgradLaunchPlan q = tbn_wgrad_launch_plan(wp, 0);
  const int v[8] = {q.mt, q.nt, q.mode, q.splits, q.rows_per_split, q.tiles_co, q.tiles_ci, q.reduce};
  memcpy(out8, v, sizeof(v));
  return (long long)q.ws_floats;
}

// ---- the 7x7 / stride 2 / pad 3 stem on its own (test / tuning aid): the launches the engine issues for conv1_7x7_s2, built
// from stem_geom (tbn_kernels.h) as build_graph / fill_fwd / fill_wgrad build them from the plan
// workspace regions (float offsets, 256-B aligned like the engine's): bordered image | packed weights | packed dW | split-K slabs
struct StemWs {
  size_t image, wpack, dwpack, wsplit, total;
};
static StemWs stem_ws(const StemGeom& g, int n, int cout) {
  StemWs s;
  size_t off = 0;
  auto take = [&](size_t f) {
    const size_t o = off;
    off += (f + 63) / 64 * 64;
    return o;
  };
  s.image = take((size_t)n * g.H * g.W * g.cp);
  s.wpack = take((size_t)cout * g.K);
  s.dwpack = take((size_t)cout * g.rows * g.kw);
  s.wsplit = take(tbn_wgrad_workspace_floats(n * g.OH * g.OW, cout, g.rows * g.kw, 1));
  s.total = off;
  return s;
}
// the argument checks the stem entries share; `who` prefixes the message
static int stem_args_ok(const char* who, int n, int h, int w, int cin, int cout, int layout, const void* workspace) {
  TBN_REQUIRE(cin >= 1 && cin <= 16, "%s: cin %d outside 1..16", who, cin);
  TBN_REQUIRE(layout >= STEM_LAYOUT_RULE && layout <= STEM_LAYOUT_ROWS, "%s: layout %d (0 = the rule, 1 = space-to-depth, 2 = row runs)",
              who, layout);
  TBN_REQUIRE(n >= 1 && h >= 1 && w >= 1 && h <= (1 << 15) && w <= (1 << 15), "%s: bad shape (%d frames of %dx%d)", who, n, h, w);
  TBN_REQUIRE(cout >= 32 && cout % 32 == 0, "%s: cout %d must be a multiple of 32", who, cout);
  const StemGeom g = stem_geom(cin, h, w, layout);
  TBN_REQUIRE((size_t)n * g.H * g.W * g.cp * sizeof(float) < (1ull << 31), "%s: the bordered image of %d frames exceeds 2 GiB", who, n);
  TBN_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-B aligned", who);
  return TBN_OK;
}
static int stem_repack(const StemGeom& g, const float* x_nchw, float* image, int n, int cin, int h, int w, hipStream_t st) {
  if (g.mode == 1) return tbn_launch_nchw_to_nhwc_pad(x_nchw, image, n, cin, h, w, g.H, g.W, st);
  return tbn_launch_nchw_to_s2d_pad(x_nchw, image, n, cin, h, w, st);
}

int tbn_stem_geometry(int cin, int h, int w, int layout, int* out8) {
  TBN_REQUIRE(out8 != nullptr, "stem_geometry: null out");
  TBN_TRY(stem_args_ok("stem_geometry", 1, h, w, cin, 32, layout, nullptr));
  const StemGeom g = stem_geom(cin, h, w, layout);
  const int v[8] = {g.mode == 1 ? STEM_LAYOUT_ROWS : STEM_LAYOUT_S2D, g.H, g.W, g.cp, g.kw, g.K, g.rows * g.kw, g.H * g.W * g.cp};
  memcpy(out8, v, sizeof(v));
  return TBN_OK;
}

size_t tbn_stem_workspace_floats(int cin, int h, int w, int layout, int n, int cout) {
  if (stem_args_ok("stem_workspace_floats", n, h, w, cin, cout, layout, nullptr) != TBN_OK) return 0;
  return stem_ws(stem_geom(cin, h, w, layout), n, cout).total;
}

int tbn_stem_conv_fwd(const float* x_nchw, const float* weight, const float* bias, float* out, int out_ld, int n, int h, int w,
                      int cin, int cout, int layout, int epilogue, const float* scale, const float* shift, float* stat_partial,
                      int mt, int nt, int stages, float* workspace, void* stream) {
  TBN_REQUIRE(x_nchw && weight && out && workspace, "stem_conv_fwd: null pointer");
  TBN_REQUIRE(epilogue >= 0 && epilogue <= 2, "stem_conv_fwd: bad epilogue");
  TBN_REQUIRE(epilogue != CONV_EPI_STATS || stat_partial, "stem_conv_fwd: stats epilogue needs stat_partial");
  TBN_REQUIRE(epilogue != CONV_EPI_EVAL || (scale && shift), "stem_conv_fwd: eval epilogue needs scale/shift");
  TBN_TRY(stem_args_ok("stem_conv_fwd", n, h, w, cin, cout, layout, workspace));
  TBN_REQUIRE(out_ld >= cout, "stem_conv_fwd: out_ld %d below cout %d", out_ld, cout);
  TBN_REQUIRE((mt == 0 && nt == 0) || (mt >= 1 && mt <= 2 && nt >= 1 && nt <= 4), "stem_conv_fwd: tile %dx%d (mt 1..2, nt 1..4, or 0x0)", mt, nt);
  TBN_REQUIRE(stages >= 0 && stages <= 2, "stem_conv_fwd: stages %d (0 = default, 1, 2)", stages);
  hipStream_t st = (hipStream_t)stream;
  const StemGeom g = stem_geom(cin, h, w, layout);
  const StemWs ws = stem_ws(g, n, cout);
  float* image = workspace + ws.image;
  float* wpack = workspace + ws.wpack;
  TBN_TRY(stem_repack(g, x_nchw, image, n, cin, h, w, st));
  if (g.mode == 1)
    TBN_TRY(tbn_launch_pack_stem_weight_rows(weight, wpack, cout, cin, g.kw, g.K, st));
  else
    TBN_TRY(tbn_launch_pack_stem_weight_s2d(weight, wpack, cout, cin, st));
  ConvP p;
  memset(&p, 0, sizeof(p));
  p.in = image;
  p.wt = wpack;
  p.bias = bias;
  p.scale = scale;
  p.shift = shift;
  p.stat_partial = stat_partial;
  p.N = n;
  p.H = g.H;
  p.W = g.W;
  p.OH = g.OH;
  p.OW = g.OW;
  p.Cin = g.kw;
  p.Cout = cout;
  p.R = g.rows;
  p.S = 1;
  p.stride = g.stride;
  p.pad = g.pad;
  p.up = 1;
  p.M = n * g.OH * g.OW;
  p.K = g.K;
  p.cp = p.in_ld = g.cp;
  p.alg_flops = 2.0 * p.M * (double)cout * 49 * cin;
  p.mode = epilogue;
  p.stages = stages;
  p.nseg = 1;
  p.seg[0].ptr = out;
  p.seg[0].ld = out_ld;
  p.seg[0].col_begin = 0;
  return tbn_launch_conv(p, 1, mt, nt, st);
}

int tbn_stem_conv_wgrad(const float* dy, int dy_ld, const float* x_nchw, float* dweight, int n, int h, int w, int cin, int cout,
                        int layout, int mt, int nt, float* workspace, void* stream) {
  TBN_REQUIRE(dy && x_nchw && dweight && workspace, "stem_conv_wgrad: null pointer");
  TBN_TRY(stem_args_ok("stem_conv_wgrad", n, h, w, cin, cout, layout, workspace));
  TBN_REQUIRE(dy_ld >= cout && dy_ld % 4 == 0, "stem_conv_wgrad: dy_ld %d (at least cout, a multiple of 4)", dy_ld);
  TBN_REQUIRE(tbn_wgrad_tile_ok(mt, nt),
              "stem_conv_wgrad: tile %dx%d (mt 1 | 2 | 3 | 5, nt 1..3 without 5x3, or 0x0)", mt, nt);
  hipStream_t st = (hipStream_t)stream;
  const StemGeom g = stem_geom(cin, h, w, layout);
  const StemWs ws = stem_ws(g, n, cout);
  float* image = workspace + ws.image;
  float* dwpack = workspace + ws.dwpack;
  TBN_TRY(stem_repack(g, x_nchw, image, n, cin, h, w, st));
  WgradP wp;
  memset(&wp, 0, sizeof(wp));
  wp.dy = dy;
  wp.dy_ld = dy_ld;
  wp.x = image;
  wp.N = n;
  wp.H = g.H;
  wp.W = g.W;
  wp.OH = g.OH;
  wp.OW = g.OW;
  wp.Cin = g.rows * g.kw;
  wp.Cout = cout;
  wp.R = g.rows;
  wp.S = 1;
  wp.taps = 1;
  wp.stride = g.stride;
  wp.pad = g.pad;
  wp.M = n * g.OH * g.OW;
  wp.cp = wp.x_ld = g.cp;
  wp.rl = g.kw;
  wp.mt = mt;
  wp.nt = nt;
  wp.alg_flops = 2.0 * wp.M * (double)cout * 49 * cin;
  TBN_TRY(tbn_launch_wgrad(wp, 1, dwpack, workspace + ws.wsplit, st));
  if (g.mode == 1) return tbn_launch_unpack_stem_wgrad_rows(dwpack, dweight, cout, cin, g.kw, st);
  return tbn_launch_unpack_stem_wgrad_s2d(dwpack, dweight, cout, cin, st);
}

// ---- linear = 1x1 conv over an (m,1,1,k) "image"
namespace {
struct ProfPrefix {   // profiler entries of the launches made inside the scope carry the prefix
  explicit ProfPrefix(const char* p) { g_prof_prefix = p; }
  ~ProfPrefix() { g_prof_prefix = nullptr; }
};
}  // namespace

int tbn_linear_fwd(const float* x, int x_ld, const float* w, const float* bias, float* out, int out_ld, int m, int k,
                   int n, int relu, void* stream) {
  ProfPrefix scope("linear: ");
  return tbn_conv2d_fwd(x, x_ld, w, bias, out, out_ld, m, 1, 1, k, n, 1, 1, 0, CONV_EPI_PLAIN,
                        relu ? CONV_FLAG_RELU : 0, nullptr, nullptr, nullptr, stream);
}

int tbn_linear_dgrad(const float* dy, int dy_ld, const float* w, float* dx, int dx_ld, int m, int k, int n,
                     int accumulate, float* workspace, void* stream) {
  ProfPrefix scope("linear: ");
  return tbn_conv2d_dgrad(dy, dy_ld, w, dx, dx_ld, m, 1, 1, k, n, 1, 1, 0, accumulate, workspace, stream);
}

size_t tbn_linear_wgrad_workspace_floats(int m, int k, int n) { return tbn_wgrad_workspace_floats(m, n, k, 1); }

int tbn_linear_wgrad(const float* dy, int dy_ld, const float* x, int x_ld, float* dw, float* dbias, int m, int k,
                     int n, float* workspace, void* stream) {
  ProfPrefix scope("linear: ");
  TBN_TRY(tbn_conv2d_wgrad(dy, dy_ld, x, x_ld, dw, m, 1, 1, k, n, 1, 1, 0, workspace, stream));
  if (dbias) TBN_TRY(tbn_colsum(dy, dy_ld, dbias, m, n, stream));
  return TBN_OK;
}

// ---- standalone training BN + ReLU
size_t tbn_bn_workspace_floats(int p, int c) { return (size_t)tbn_bn_stats_parts(p, c) * 2 * c + 3 * (size_t)c; }

int tbn_bn_relu_train_fwd(const float* y, int p, int c, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, float momentum, float eps, float* save_mean, float* save_rstd,
                          float* scale, float* shift, float* z, int z_ld, float* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int parts = 0;
  TBN_TRY(tbn_launch_bn_stats(y, c, p, c, workspace, &parts, st));
  TBN_TRY(tbn_launch_bn_finalize(workspace, parts, p, c, gamma, beta, nullptr, running_mean, running_var, momentum, eps,
                                 save_mean, save_rstd, scale, shift, st));
  Seg s;
  s.ptr = z;
  s.ld = z_ld;
  s.col_begin = 0;
  return tbn_launch_bn_apply(y, p, c, scale, shift, &s, 1, st);
}

int tbn_bn_relu_train_bwd(const float* dz, int dz_ld, const float* y, int p, int c, const float* save_mean,
                          const float* save_rstd, const float* scale, const float* shift, float* dy, float* dgamma,
                          float* dbeta, float* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  CSeg s;
  s.ptr = dz;
  s.ld = dz_ld;
  s.col_begin = 0;
  const int parts = tbn_bn_bwd_parts(p, c);
  float* coef = workspace + (size_t)parts * 2 * c;
  TBN_TRY(tbn_launch_bn_bwd_reduce(&s, 1, y, p, c, scale, shift, save_mean, save_rstd, workspace, st));
  TBN_TRY(tbn_launch_bn_bwd_finalize(workspace, parts, p, c, scale, save_mean, save_rstd, coef, dgamma, dbeta, nullptr,
                                     st));
  return tbn_launch_bn_bwd_apply(&s, 1, y, p, c, scale, shift, coef, dy, st);
}

// ---- the engine's batched training BN on its own (bn_multi.hip): descriptors in, the launchers' own rules decide
int tbn_bn_stats_partials(const float* y, int y_ld, int p, int c, float* partial, int* nparts, void* stream) {
  TBN_REQUIRE(y && partial && nparts, "bn_stats_partials: null pointer");
  return tbn_launch_bn_stats(y, y_ld, p, c, partial, nparts, (hipStream_t)stream);
}

size_t tbn_bn_bwd_partial_floats(int p, int c) {
  if (p < 1 || c < 4 || c > 1024 || c % 4 != 0) return 0;
  return (size_t)tbn_bn_bwd_parts(p, c) * 2 * c;
}

int tbn_bn_fwd_batch(const tbn_bn_fwd_desc* members, int n, float momentum, float eps, void* stream) {
  TBN_REQUIRE(members != nullptr, "bn_fwd_batch: null pointer");
  static thread_local BnFwdBatch b;
  memset(&b, 0, sizeof(b));
  b.n = n;                       // outside 1..TBN_BN_MAXL: nothing is copied and the launcher refuses
  b.momentum = momentum;
  b.eps = eps;
  for (int i = 0; i < n && n <= TBN_BN_MAXL; ++i) {
    const tbn_bn_fwd_desc& d = members[i];
    TBN_REQUIRE(d.y && d.partial && d.gamma && d.beta && d.save_mean && d.save_rstd && d.scale && d.shift,
                "bn_fwd_batch: null pointer in member %d", i);
    TBN_REQUIRE(d.running_mean == nullptr || d.running_var != nullptr, "bn_fwd_batch: member %d has running_mean without running_var", i);
    BnFwdLayer& L = b.l[i];
    L.y = d.y; L.y_ld = d.y_ld; L.P = d.p; L.C = d.c;
    L.partial = d.partial; L.pld = d.pld; L.nparts = d.nparts;
    L.gamma = d.gamma; L.beta = d.beta; L.conv_bias = d.conv_bias;
    L.running_mean = d.running_mean; L.running_var = d.running_var;
    L.save_mean = d.save_mean; L.save_rstd = d.save_rstd; L.scale = d.scale; L.shift = d.shift;
    L.nseg = d.nseg;
    for (int s = 0; s < 3 && s < d.nseg; ++s) {
      TBN_REQUIRE(d.seg[s].ptr != nullptr, "bn_fwd_batch: null pointer in segment %d of member %d", s, i);
      L.seg[s].ptr = d.seg[s].ptr; L.seg[s].ld = d.seg[s].ld; L.seg[s].col_begin = d.seg[s].col_begin;
    }
  }
  return tbn_launch_bn_fwd_multi(b, (hipStream_t)stream);
}

int tbn_bn_bwd_batch(const tbn_bn_bwd_desc* members, int n, void* stream) {
  TBN_REQUIRE(members != nullptr, "bn_bwd_batch: null pointer");
  static thread_local BnBwdBatch b;
  memset(&b, 0, sizeof(b));
  b.n = n;
  for (int i = 0; i < n && n <= TBN_BN_MAXL; ++i) {
    const tbn_bn_bwd_desc& d = members[i];
    TBN_REQUIRE(d.y && d.dy && d.scale && d.shift && d.mean && d.rstd && d.partial && d.coef,
                "bn_bwd_batch: null pointer in member %d", i);
    BnBwdLayer& L = b.l[i];
    L.nseg = d.nseg;
    for (int s = 0; s < 3 && s < d.nseg; ++s) {
      TBN_REQUIRE(d.dz[s].ptr != nullptr, "bn_bwd_batch: null pointer in segment %d of member %d", s, i);
      L.dz[s].ptr = d.dz[s].ptr; L.dz[s].ld = d.dz[s].ld; L.dz[s].col_begin = d.dz[s].col_begin;
    }
    L.y = d.y; L.dy = d.dy; L.y_ld = d.y_ld; L.P = d.p; L.C = d.c;
    L.scale = d.scale; L.shift = d.shift; L.mean = d.mean; L.rstd = d.rstd;
    L.partial = d.partial; L.ext_parts = d.ext_parts; L.coef = d.coef;
    L.dgamma = d.dgamma; L.dbeta = d.dbeta; L.dbias = d.dbias;
  }
  return tbn_launch_bn_bwd_multi(b, (hipStream_t)stream);
}

// ---- training BN + ReLU + max pool in one pass (the fused stem form of the engine)
int tbn_bn_relu_maxpool_train_fwd(const float* y, int n, int h, int w, int c, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                                  float* save_rstd, float* scale, float* shift, float* pooled, int pooled_ld,
                                  uint8_t* argmax, int oh, int ow, int stride, int pad, float* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  TBN_REQUIRE(y && pooled && argmax && workspace, "bn_relu_maxpool_train_fwd: null pointer");
  const int p = n * h * w;
  int parts = 0;
  TBN_TRY(tbn_launch_bn_stats(y, c, p, c, workspace, &parts, st));
  TBN_TRY(tbn_launch_bn_finalize(workspace, parts, p, c, gamma, beta, nullptr, running_mean, running_var, momentum, eps,
                                 save_mean, save_rstd, scale, shift, st));
  return tbn_launch_bn_apply_maxpool(y, n, h, w, c, scale, shift, pooled, pooled_ld, argmax, oh, ow, stride, pad, st);
}

int tbn_bn_relu_maxpool_train_bwd(const float* dpooled, int dpooled_ld, const uint8_t* argmax, const float* y, int n, int h,
                                  int w, int c, int oh, int ow, int stride, int pad, const float* save_mean,
                                  const float* save_rstd, const float* scale, const float* shift, float* dy,
                                  float* dgamma, float* dbeta, float* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  TBN_REQUIRE(dpooled && argmax && y && dy && workspace, "bn_relu_maxpool_train_bwd: null pointer");
  const int p = n * h * w;
  const int parts = tbn_bn_bwd_pooled_parts(n, h, w, c, stride, pad);
  TBN_REQUIRE(parts <= tbn_bn_bwd_parts(p, c), "bn_relu_maxpool_train_bwd: workspace sized by tbn_bn_workspace_floats is too small");
  float* coef = workspace + (size_t)tbn_bn_bwd_parts(p, c) * 2 * c;
  TBN_TRY(tbn_launch_bn_bwd_reduce_pooled(dpooled, dpooled_ld, argmax, n, h, w, oh, ow, stride, pad, y, c, scale, shift,
                                          save_mean, save_rstd, workspace, st));
  TBN_TRY(tbn_launch_bn_bwd_finalize(workspace, parts, p, c, scale, save_mean, save_rstd, coef, dgamma, dbeta, nullptr, st));
  return tbn_launch_bn_bwd_apply_pooled(dpooled, dpooled_ld, argmax, n, h, w, oh, ow, stride, pad, y, c, scale, shift, coef,
                                        dy, st);
}

// ---- pooling
int tbn_maxpool3_fwd(const float* in, int in_ld, float* out, int out_ld, uint8_t* argmax, int n, int h, int w, int c,
                     int oh, int ow, int stride, int pad, void* stream) {
  return tbn_launch_maxpool_fwd(in, in_ld, out, out_ld, argmax, n, h, w, c, oh, ow, stride, pad, (hipStream_t)stream);
}
int tbn_maxpool3_bwd(const float* dout, int dout_ld, const uint8_t* argmax, float* din, int din_ld, int n, int h,
                     int w, int c, int oh, int ow, int stride, int pad, int accumulate, void* stream) {
  return tbn_launch_maxpool_bwd(dout, dout_ld, argmax, din, din_ld, n, h, w, c, oh, ow, stride, pad, accumulate,
                                (hipStream_t)stream);
}
int tbn_avgpool3_fwd(const float* in, int in_ld, float* out, int out_ld, int n, int h, int w, int c, int accumulate,
                     void* stream) {
  return tbn_launch_avgpool3_fwd(in, in_ld, out, out_ld, n, h, w, c, accumulate, (hipStream_t)stream);
}
int tbn_spatial_mean_fwd(const float* in, int in_ld, float* out, int out_ld, int n, int h, int w, int c,
                         int freq_only, void* stream) {
  return tbn_launch_spatial_mean_fwd(in, in_ld, out, out_ld, n, h, w, c, freq_only, (hipStream_t)stream);
}
int tbn_spatial_mean_bwd(const float* dout, int dout_ld, float* din, int din_ld, int n, int h, int w, int c,
                         int freq_only, void* stream) {
  return tbn_launch_spatial_mean_bwd(dout, dout_ld, din, din_ld, n, h, w, c, freq_only, (hipStream_t)stream);
}

}  // extern "C"
