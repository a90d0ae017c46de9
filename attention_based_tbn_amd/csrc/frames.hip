// On-device input pipeline for the visual modalities: the step right before the hot path.
//
// Reference (host, per sample, NumPy + cv2):  core/utils/create_dataloader.py:19-81 composes
//   train:  MultiScaleCrop (crop box -> cv2.resize INTER_LINEAR to the input size)  ->  RandomHorizontalFlip
//   test :  Rescale (cv2.resize, smaller edge to test_scale_size)  ->  CenterCrop
//   both :  Stack (Flow: `length` single-channel images become the channels of one sample)  ->  ToTensor
//           (uint8 HWC -> float CHW, / 255)  ->  Normalize ((x - mean) / std)       core/dataset/transform.py:9-543
// Here the random decisions stay on the host (same NumPy draws), the pixels are touched ONCE: a single kernel reads
// the uint8 frames, resizes / crops / flips on the fly and writes the normalised fp32 NCHW tensor the model takes.
//
// Resize arithmetic = OpenCV's 8-bit INTER_LINEAR (imgproc/resize.cpp: 11-bit fixed-point weights, cvRound,
//   horizontal pass in int, vertical pass ((b0*(S0>>4))>>16 + (b1*(S1>>4))>>16 + 2) >> 2).  cv2 is NOT in the build
//   image, so that part is restated from the published algorithm ("parity unpinned"); crop / flip / stack /
//   ToTensor / Normalize are pinned bit-exactly to the reference classes.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "tbn_common.h"
#include "../../include/tbn_hip.h"

struct FramesP {
  const unsigned char* src;
  float* out;
  int n_img, H, W, C;            // source frames (n_img, H, W, C) uint8
  int bx, by, bw, bh;            // box of the source that is resized
  int rw, rh;                    // size the box is resized to (== bw, bh: no interpolation)
  int ow, oh;                    // crop window size = output size
  int n_crops, mirror;           // windows per image; 0 as given, 1 mirrored, 2 window then mirror, 3 mirror then window
  int stack, div255;
  int n_stat;                    // entries of mean / std (repeated over the channels, as Normalize does)
  double scale_x, scale_y;
  int cx[TBN_FRAMES_MAX_CROPS], cy[TBN_FRAMES_MAX_CROPS];   // window origins inside the resized box
};

__device__ __forceinline__ int cv_round_to_short(float v) {
  // saturate_cast<short>(cvRound(v)): round half to even; v is in [0, 2048]
  return (int)__float2int_rn(v);
}

__device__ __forceinline__ void lin_coef(int d, double scale, int ssize, int* s0, int* a0, int* a1, bool clamp_frac) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (clamp_frac) {                    // x direction: the fraction is zeroed at the borders
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
  }
  *s0 = s;
  *a0 = cv_round_to_short((1.f - f) * 2048.f);
  *a1 = cv_round_to_short(f * 2048.f);
}

// What one workgroup needs to know: one output plane's source image and channel, the geometry and the plane's place in
// `out`.  Uniform over the workgroup: the single-geometry entries fill it from the launch arguments (FramesP), the
// batch entry from its clip's row of the table in device memory (a scalar load), so neither "resize or not" nor the
// flip diverges inside a workgroup.
struct FramePlane {
  const unsigned char* base;     // the plane's source image, at its channel
  float* out;                    // the plane (oh x ow)
  int W, C;                      // source row pitch = W * C bytes
  int bx, by, bw, bh, rw, rh, ow, oh;
  int cx, cy, flip;
  int c;                         // output channel of the sample: selects mean / std
  int div255, n_stat;
  double scale_x, scale_y;
};

// One workgroup = kRows output rows of ONE output plane (sample n, channel c).  A thread owns the columns x = tid,
// tid + 256, ...: their horizontal source positions / weights are computed once and reused for every row; the rows'
// vertical coefficients are computed once per workgroup (LDS).  Per output element that leaves four byte loads, the
// fixed-point blend, one table look-up (ToTensor / Normalize) and one coalesced store -- the first version decoded
// the flat index (64-bit div / mod chain) and both coefficient pairs (double precision) per ELEMENT and ran at
// 1.0-1.35 TB/s of algorithmic bytes.
constexpr int kFrameRows = 32;
constexpr int kFrameCols = 4;     // columns per thread: output widths up to 1024
__device__ __forceinline__ void frames_plane_rows(const FramePlane& q, int rt, const float* __restrict__ mean,
                                                  const float* __restrict__ stdv) {
  __shared__ int ysrc0[kFrameRows], ysrc1[kFrameRows], yw0[kFrameRows], yw1[kFrameRows];
  const int y_begin = rt * kFrameRows, y_end = min(q.oh, y_begin + kFrameRows);
  const bool resize = (q.rw != q.bw) || (q.rh != q.bh);
  const int tid = threadIdx.x;
  if (tid < y_end - y_begin) {
    const int yr = q.cy + y_begin + tid;              // position in the resized box
    if (resize) {
      int sy, ay0, ay1;
      lin_coef(yr, q.scale_y, q.bh, &sy, &ay0, &ay1, false);
      ysrc0[tid] = q.by + min(max(sy, 0), q.bh - 1);     // rows are clamped
      ysrc1[tid] = q.by + min(max(sy + 1, 0), q.bh - 1);
      yw0[tid] = ay0;
      yw1[tid] = ay1;
    } else {
      ysrc0[tid] = ysrc1[tid] = q.by + yr;
      yw0[tid] = yw1[tid] = 0;
    }
  }
  int xs0[kFrameCols], xs1[kFrameCols], xa0[kFrameCols], xa1[kFrameCols];
#pragma unroll
  for (int k = 0; k < kFrameCols; ++k) {
    const int x = tid + 256 * k;
    xs0[k] = xs1[k] = xa0[k] = xa1[k] = 0;
    if (x < q.ow) {
      const int xr = q.cx + (q.flip ? q.ow - 1 - x : x);
      if (resize) {
        int sx, ax0, ax1;
        lin_coef(xr, q.scale_x, q.bw, &sx, &ax0, &ax1, true);
        xs0[k] = (q.bx + sx) * q.C;
        xs1[k] = (q.bx + min(sx + 1, q.bw - 1)) * q.C;   // weight 0 when clamped
        xa0[k] = ax0;
        xa1[k] = ax1;
      } else {
        xs0[k] = (q.bx + xr) * q.C;
      }
    }
  }
  // ToTensor / Normalize see only 256 different inputs per plane: their exact (correctly rounded, as torch) divisions
  // are done once per workgroup, the pixel loop looks the result up
  __shared__ float lut[256];
  {
    float f = (float)tid;
    if (q.div255) f = f / 255.f;
    if (q.n_stat > 0) f = (f - mean[q.c % q.n_stat]) / stdv[q.c % q.n_stat];
    lut[tid] = f;
  }
  const unsigned char* __restrict__ base = q.base;
  float* __restrict__ out = q.out + (size_t)y_begin * q.ow;
  __syncthreads();
  for (int y = 0; y < y_end - y_begin; ++y) {
    const unsigned char* r0 = base + (size_t)ysrc0[y] * q.W * q.C;
    const unsigned char* r1 = base + (size_t)ysrc1[y] * q.W * q.C;
    const int ay0 = yw0[y], ay1 = yw1[y];
#pragma unroll
    for (int k = 0; k < kFrameCols; ++k) {
      const int x = tid + 256 * k;
      if (x >= q.ow) break;
      int v;
      if (!resize) {
        v = r0[xs0[k]];
      } else {
        const int h0 = (int)r0[xs0[k]] * xa0[k] + (int)r0[xs1[k]] * xa1[k];
        const int h1 = (int)r1[xs0[k]] * xa0[k] + (int)r1[xs1[k]] * xa1[k];
        v = (((ay0 * (h0 >> 4)) >> 16) + ((ay1 * (h1 >> 4)) >> 16) + 2) >> 2;
        v = min(max(v, 0), 255);
      }
      out[(size_t)y * q.ow + x] = lut[v];
    }
  }
}

// Single geometry.  The plane's stack slot u = c / C is entry j = n * stack + u of the flat list FixedCrop emits
// (transform.py:153-177: windows outermost, then the images, then plain / mirrored), which Stack cuts into runs of
// `stack` (transform.py:454-459): j -> (window, image, mirrored).  With one window and no pairs j is the image itself,
// the single-window entry.
__global__ __launch_bounds__(256) void frames_to_tensor_kernel(FramesP p, const float* __restrict__ mean,
                                                               const float* __restrict__ stdv) {
  const int co = p.C * p.stack;                       // output channels per sample
  const int row_tiles = (p.oh + kFrameRows - 1) / kFrameRows;
  const int plane = blockIdx.x / row_tiles, rt = blockIdx.x - plane * row_tiles;
  const int n = plane / co, c = plane - n * co;
  const int j = n * p.stack + c / p.C, ch = c % p.C;
  const int pair = p.mirror >= 2 ? 2 : 1;
  const int second = j % pair, t = j / pair;
  const int img = t % p.n_img, win = t / p.n_img;                  // win < n_crops: planes cover exactly the list
  FramePlane q;
  q.base = p.src + (size_t)img * p.H * p.W * p.C + ch;
  q.out = p.out + (size_t)plane * p.oh * p.ow;
  q.W = p.W; q.C = p.C;
  q.bx = p.bx; q.by = p.by; q.bw = p.bw; q.bh = p.bh; q.rw = p.rw; q.rh = p.rh; q.ow = p.ow; q.oh = p.oh;
  q.cx = p.cx[win]; q.cy = p.cy[win];
  q.flip = p.mirror == 1 || (p.mirror == 2 && second) || (p.mirror == 3 && !second);
  q.c = c; q.div255 = p.div255; q.n_stat = p.n_stat;
  q.scale_x = p.scale_x; q.scale_y = p.scale_y;
  frames_plane_rows(q, rt, mean, stdv);
}

// A batch of clips, one geometry each.  The workgroups of clip k are consecutive; a workgroup reads its clip's row of
// the table (uniform address: a scalar load) and does what frames_to_tensor_kernel does for that geometry, image
// first_img + j of `src`, sample out_row + n of `out`.  The two scale factors are the host's expression in the same
// IEEE double operations (a correctly rounded division twice), so the bits are those of the single-geometry launch.
struct FramesBatchP {
  const unsigned char* src;
  float* out;
  const tbn_frames_clip* clips;
  int H, W, C, ow, oh, stack, div255, n_stat;
  int planes_per_clip;           // imgs_per_clip / stack * C * stack
};

__global__ __launch_bounds__(256) void frames_to_tensor_batch_kernel(FramesBatchP p, const float* __restrict__ mean,
                                                                     const float* __restrict__ stdv) {
  const int co = p.C * p.stack;
  const int row_tiles = (p.oh + kFrameRows - 1) / kFrameRows;
  const int plane_all = blockIdx.x / row_tiles, rt = blockIdx.x - plane_all * row_tiles;
  const int clip = plane_all / p.planes_per_clip, plane = plane_all - clip * p.planes_per_clip;
  const tbn_frames_clip k = p.clips[clip];
  const int n = plane / co, c = plane - n * co;
  const int img = k.first_img + n * p.stack + c / p.C, ch = c % p.C;
  FramePlane q;
  q.base = p.src + (size_t)img * p.H * p.W * p.C + ch;
  q.out = p.out + ((size_t)(k.out_row + n) * co + c) * p.oh * p.ow;
  q.W = p.W; q.C = p.C;
  q.bx = k.box_x; q.by = k.box_y; q.bw = k.box_w; q.bh = k.box_h; q.rw = k.resized_w; q.rh = k.resized_h;
  q.ow = p.ow; q.oh = p.oh;
  q.cx = k.crop_x; q.cy = k.crop_y; q.flip = k.flip != 0;
  q.c = c; q.div255 = p.div255; q.n_stat = p.n_stat;
  q.scale_x = 1.0 / ((double)k.resized_w / (double)k.box_w);
  q.scale_y = 1.0 / ((double)k.resized_h / (double)k.box_h);
  frames_plane_rows(q, rt, mean, stdv);
}

// One geometry against its frame: the kernels read `frames` unchecked, so the source box must lie inside the frame and
// every window inside the resized box.  `who` names the entry (and, for a batch, the clip) in the messages.
static int frames_check_geometry(const char* who, int height, int width, int box_x, int box_y, int box_w, int box_h,
                                 int resized_w, int resized_h, const int* crop_x, const int* crop_y, int n_crops,
                                 int out_w, int out_h) {
  TBN_REQUIRE(box_x >= 0 && box_y >= 0 && box_w > 0 && box_h > 0 && box_x <= width - box_w && box_y <= height - box_h,
              "%s: source box (%d,%d,%d,%d) outside the %dx%d frame", who, box_x, box_y, box_w, box_h, width, height);
  TBN_REQUIRE(resized_w > 0 && resized_h > 0 && out_w > 0 && out_h > 0, "%s: empty resized box %dx%d or window %dx%d",
              who, resized_w, resized_h, out_w, out_h);
  for (int i = 0; i < n_crops; ++i)
    TBN_REQUIRE(crop_x[i] >= 0 && crop_y[i] >= 0 && crop_x[i] <= resized_w - out_w && crop_y[i] <= resized_h - out_h,
                "%s: crop window (%d,%d,%d,%d) outside the resized %dx%d box", who, crop_x[i], crop_y[i], out_w, out_h,
                resized_w, resized_h);
  return TBN_OK;
}

// the two single-geometry entries: `fn` names the entry in the messages
static int frames_launch(const char* fn, const unsigned char* frames, int n_img, int height, int width, int channels,
                         int box_x, int box_y, int box_w, int box_h, int resized_w, int resized_h, const int* crop_x,
                         const int* crop_y, int n_crops, int out_w, int out_h, int mirror, int stack, const float* mean,
                         const float* std_dev, int n_stat, int div255, float* out, void* stream) {
  TBN_REQUIRE(frames != nullptr && out != nullptr && crop_x != nullptr && crop_y != nullptr, "%s: null argument", fn);
  TBN_REQUIRE(n_crops >= 1 && n_crops <= TBN_FRAMES_MAX_CROPS, "%s: %d crop windows, 1..%d supported", fn, n_crops,
              TBN_FRAMES_MAX_CROPS);
  TBN_REQUIRE(mirror >= 0 && mirror <= 3, "%s: mirror mode %d is not one of 0..3", fn, mirror);
  const long long entries = (long long)n_img * n_crops * (mirror >= 2 ? 2 : 1);    // FixedCrop's flat list
  TBN_REQUIRE(n_img >= 0 && height > 0 && width > 0 && channels >= 1 && channels <= 4 && stack >= 1 &&
                  entries % stack == 0,
              "%s: bad frame stack (n=%d, %dx%dx%d, stack %d, %lld crops)", fn, n_img, height, width, channels, stack,
              entries);
  if (int rc = frames_check_geometry(fn, height, width, box_x, box_y, box_w, box_h, resized_w, resized_h, crop_x, crop_y,
                                     n_crops, out_w, out_h))
    return rc;
  TBN_REQUIRE(n_stat == 0 || (mean != nullptr && std_dev != nullptr), "%s: mean/std missing", fn);
  if (n_img == 0) return TBN_OK;
  FramesP p;
  p.src = frames; p.out = out;
  p.n_img = n_img; p.H = height; p.W = width; p.C = channels;
  p.bx = box_x; p.by = box_y; p.bw = box_w; p.bh = box_h;
  p.rw = resized_w; p.rh = resized_h;
  p.ow = out_w; p.oh = out_h;
  p.n_crops = n_crops; p.mirror = mirror;
  for (int i = 0; i < TBN_FRAMES_MAX_CROPS; ++i) {
    p.cx[i] = i < n_crops ? crop_x[i] : 0;
    p.cy[i] = i < n_crops ? crop_y[i] : 0;
  }
  p.stack = stack; p.div255 = div255 ? 1 : 0; p.n_stat = n_stat;
  // resize.cpp: inv_scale = dsize / ssize (double); scale = 1. / inv_scale
  p.scale_x = 1.0 / ((double)resized_w / (double)box_w);
  p.scale_y = 1.0 / ((double)resized_h / (double)box_h);
  TBN_REQUIRE(out_w <= 256 * kFrameCols, "%s: output width %d > %d", fn, out_w, 256 * kFrameCols);
  const size_t planes = (size_t)entries * channels;              // (entries / stack) samples x (channels * stack)
  const size_t g = planes * (size_t)((out_h + kFrameRows - 1) / kFrameRows);
  TBN_REQUIRE(g < (1ull << 31), "%s: too many output planes", fn);
  TBN_KLAUNCH(frames_to_tensor_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, p, mean, std_dev);
  TBN_CHECK_LAUNCH(fn);
  return TBN_OK;
}

extern "C" int tbn_frames_to_tensor(const unsigned char* frames, int n_img, int height, int width, int channels,
                                    int box_x, int box_y, int box_w, int box_h, int resized_w, int resized_h,
                                    int crop_x, int crop_y, int out_w, int out_h, int flip, int stack,
                                    const float* mean, const float* std_dev, int n_stat, int div255, float* out,
                                    void* stream) {
  return frames_launch("frames_to_tensor", frames, n_img, height, width, channels, box_x, box_y, box_w, box_h,
                       resized_w, resized_h, &crop_x, &crop_y, 1, out_w, out_h, flip ? 1 : 0, stack, mean, std_dev,
                       n_stat, div255, out, stream);
}

extern "C" int tbn_frames_to_tensor_crops(const unsigned char* frames, int n_img, int height, int width, int channels,
                                          int box_x, int box_y, int box_w, int box_h, int resized_w, int resized_h,
                                          const int* crop_x, const int* crop_y, int n_crops, int out_w, int out_h,
                                          int mirror, int stack, const float* mean, const float* std_dev, int n_stat,
                                          int div255, float* out, void* stream) {
  return frames_launch("frames_to_tensor_crops", frames, n_img, height, width, channels, box_x, box_y, box_w, box_h,
                       resized_w, resized_h, crop_x, crop_y, n_crops, out_w, out_h, mirror, stack, mean, std_dev, n_stat,
                       div255, out, stream);
}

extern "C" int tbn_frames_to_tensor_batch(const unsigned char* frames, int n_img, int height, int width, int channels,
                                          const tbn_frames_clip* clips_host, const tbn_frames_clip* clips_dev,
                                          int n_clips, int imgs_per_clip, int out_w, int out_h, int stack,
                                          const float* mean, const float* std_dev, int n_stat, int div255, float* out,
                                          int out_rows, void* stream) {
  const char* fn = "frames_to_tensor_batch";
  TBN_REQUIRE(n_clips >= 0, "%s: %d clips", fn, n_clips);
  if (n_clips == 0) return TBN_OK;
  TBN_REQUIRE(frames != nullptr && out != nullptr && clips_host != nullptr && clips_dev != nullptr, "%s: null argument",
              fn);
  TBN_REQUIRE(n_img >= 0 && height > 0 && width > 0 && channels >= 1 && channels <= 4 && stack >= 1 && out_rows >= 0,
              "%s: bad frame stack (n=%d, %dx%dx%d, stack %d, %d output rows)", fn, n_img, height, width, channels,
              stack, out_rows);
  TBN_REQUIRE(imgs_per_clip > 0 && imgs_per_clip % stack == 0,
              "%s: clip 0: %d images per clip is not a positive multiple of the stack length %d", fn, imgs_per_clip,
              stack);
  TBN_REQUIRE(n_stat == 0 || (mean != nullptr && std_dev != nullptr), "%s: mean/std missing", fn);
  TBN_REQUIRE(out_w <= 256 * kFrameCols, "%s: output width %d > %d", fn, out_w, 256 * kFrameCols);
  const int rows_per_clip = imgs_per_clip / stack;
  std::vector<std::pair<int, int>> rows((size_t)n_clips);        // (first output row, clip)
  char who[64];
  for (int i = 0; i < n_clips; ++i) {
    const tbn_frames_clip& k = clips_host[i];
    snprintf(who, sizeof(who), "%s: clip %d", fn, i);
    TBN_REQUIRE(k.first_img >= 0 && k.first_img <= n_img - imgs_per_clip,
                "%s: images %d..%d outside the %d frames", who, k.first_img, k.first_img + imgs_per_clip - 1, n_img);
    if (int rc = frames_check_geometry(who, height, width, k.box_x, k.box_y, k.box_w, k.box_h, k.resized_w, k.resized_h,
                                       &k.crop_x, &k.crop_y, 1, out_w, out_h))
      return rc;
    TBN_REQUIRE(k.out_row >= 0 && k.out_row <= out_rows - rows_per_clip,
                "%s: output rows %d..%d outside the %d rows of out", who, k.out_row, k.out_row + rows_per_clip - 1,
                out_rows);
    rows[(size_t)i] = {k.out_row, i};
  }
  std::sort(rows.begin(), rows.end());
  for (int i = 1; i < n_clips; ++i)
    TBN_REQUIRE(rows[i].first - rows[i - 1].first >= rows_per_clip,
                "%s: clip %d and clip %d write overlapping output rows (%d and %d, %d rows each)", fn,
                std::min(rows[i - 1].second, rows[i].second), std::max(rows[i - 1].second, rows[i].second),
                rows[i - 1].first, rows[i].first, rows_per_clip);
  FramesBatchP p;
  p.src = frames; p.out = out; p.clips = clips_dev;
  p.H = height; p.W = width; p.C = channels; p.ow = out_w; p.oh = out_h;
  p.stack = stack; p.div255 = div255 ? 1 : 0; p.n_stat = n_stat;
  const size_t planes = (size_t)imgs_per_clip * channels;        // (imgs_per_clip / stack) samples x (channels * stack)
  const size_t g = (size_t)n_clips * planes * (size_t)((out_h + kFrameRows - 1) / kFrameRows);
  TBN_REQUIRE(g < (1ull << 31), "%s: too many output planes", fn);
  p.planes_per_clip = (int)planes;
  TBN_KLAUNCH(frames_to_tensor_batch_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, p, mean, std_dev);
  TBN_CHECK_LAUNCH(fn);
  return TBN_OK;
}
