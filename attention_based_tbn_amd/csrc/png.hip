// PNG frames on the device: the step in front of tbn_frames_to_tensor for frames extracted as PNG.  Replaces cv2.imread of
// reference core/dataset/dataset.py:305 (RGB) and :360, :365 (Flow) when data.rgb.file_ext / data.flow.file_ext is "png".
// The container is host work (csrc/tbn_png_host.h); here are the three kernels and their host twins.
//
// png_inflate_kernel, 64 threads (one wavefront) per image: the RFC 1951 decoder core of csrc/tbn_inflate.h with the IO policy
// of csrc/tbn_inflate_dev.h, exactly as inflate_kernel of csrc/inflate.hip runs it, over the image's deflate data (the zlib
// stream without its 2-byte header and 4-byte trailer) into the image's raw_bytes of the workspace.
//
// png_adler_kernel, 256 threads per image: Adler-32 is combinable, so every thread sums one piece of the inflated bytes from
// (a, b) = (1, 0) and thread 0 folds the 256 pieces in order (tbn_png_core.h: adler_fold); a mismatch turns status 0 into 20.
//
// png_unfilter_kernel, 64 threads (one wavefront) per image: scanline unfiltering fused with the conversion into frame bytes.
// Pixel (y, x) needs (y, x - 1), (y - 1, x) and (y - 1, x - 1), and Average and Paeth are not associative along a row, so
// the parallelism inside an image is the skewed wavefront: in a band of 64 rows lane l takes row r0 + l and runs one pixel
// behind lane l - 1.  At step t lane l reconstructs pixel x = t - l: `a` is its own previous pixel (a register), `b` is what
// lane l - 1 made one step earlier (one cross-lane move), `c` is the `b` of the step before.  Lane 0's `b` is the previous
// band's last reconstructed row, kept in LDS (two buffers, read one and write the other: the frame bytes cannot serve,
// palette and alpha conversion change them).  The five predictors are selects on the lane's filter type.
// Each lane walks its row, so its reads and writes are strided by the row length; they are staged: every kStepTile steps all
// lanes together load, row by row, the dwords that cover the pixels each row is about to take into an LDS tile, and store
// the finished frame bytes of each row from a second tile, so that global accesses run along rows.
// Every address depends on the geometry alone: corrupt bytes cost a status (21, 22) or garbage pixels, never a fault.
#include "tbn_common.h"
#include "tbn_inflate.h"
#include "tbn_inflate_dev.h"
#include "tbn_png_core.h"
#include "tbn_png_host.h"
#include "../../include/tbn_hip.h"

using namespace tbn_inflate;
using namespace tbn_png;

static_assert(sizeof(tbn_png_image) == 24, "the image row is 24 bytes");
static_assert(TBN_PNG_MAX_ROW_BYTES >= 4096 * 4, "a row of 4096 RGBA pixels stays on chip");

namespace {

constexpr int kUnfThreads = 64;                        // one wavefront: the cross-lane move and wave_sync rely on it
constexpr int kInPitchDw = kStepTile + 2;              // dwords of one row of the input tile: 3 + 64 * 4 + 3 bytes at most
constexpr int kOutPitch = kStepTile * 3;               // bytes of one row of the output tile
static_assert(kBandRows == kUnfThreads && kStepTile == 64, "one lane per row of a band; the staging loops assume 64 steps");

__device__ __forceinline__ void wave_sync() {          // as DevIO::sync: the workgroup is one wavefront
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the aligned dword at byte offset `off` of raw[0, total); bytes at or behind `total` read as zero and are not read
__device__ __forceinline__ uint32_t load_dword(const uint8_t* raw, size_t off, size_t total) {
  if (off + 4 <= total) return *(const uint32_t*)(raw + off);
  uint32_t v = 0;
  for (uint32_t k = 0; k < 4; ++k)
    if (off + k < total) v |= (uint32_t)raw[off + k] << (8 * k);
  return v;
}

// where image i's palette slot lies: (n_img, TBN_PNG_PALETTE_BYTES) behind `pal_base`, or at images[i].palette_off of it
__host__ __device__ __forceinline__ const uint8_t* palette_of(const uint8_t* pal_base, const tbn_png_image* images, int i) {
  return images ? pal_base + images[i].palette_off : pal_base + (size_t)i * TBN_PNG_PALETTE_BYTES;
}

template <int BPP, int MODE>
__global__ __launch_bounds__(kUnfThreads) void png_unfilter_kernel(const uint8_t* __restrict__ raw, size_t raw_total, uint32_t raw_bytes,
                                                                   const uint8_t* __restrict__ pal_base,
                                                                   const tbn_png_image* __restrict__ images, int W, int H, int oc,
                                                                   uint8_t* __restrict__ frames, int* __restrict__ status, int keep) {
  __shared__ uint32_t tile_in[kBandRows * kInPitchDw];
  __shared__ uint8_t tile_out[kBandRows * kOutPitch];
  __shared__ uint32_t prev_dw[2][TBN_PNG_MAX_ROW_BYTES / 4];
  __shared__ uint8_t pal[768];
  const int img = blockIdx.x, ln = threadIdx.x;
  if (keep && status[img] != 0) return;            // one value for the wavefront: the image is the host stage's
  uint32_t entries = 0;
  if (MODE == kModePalette) {
    const uint8_t* p = palette_of(pal_base, images, img);
    for (int i = ln; i < 768; i += kUnfThreads) pal[i] = p[i];
    entries = (uint32_t)p[768] | ((uint32_t)p[769] << 8);
    entries = entries > 256u ? 256u : entries;
  }
  const uint32_t row_bytes = (uint32_t)W * BPP, stride = 1u + row_bytes;
  for (uint32_t i = (uint32_t)ln; i < (row_bytes + 3u) / 4u; i += kUnfThreads) prev_dw[0][i] = 0;   // row -1 is zero
  const size_t img_base = (size_t)img * raw_bytes;
  const uint8_t* in_bytes = (const uint8_t*)tile_in;
  bool bad_filter = false, bad_index = false;
  int band = 0;
  for (int r0 = 0; r0 < H; r0 += kBandRows, ++band) {
    const uint8_t* prev_rd = (const uint8_t*)prev_dw[band & 1];
    uint8_t* prev_wr = (uint8_t*)prev_dw[(band + 1) & 1];
    const int rows = H - r0 < kBandRows ? H - r0 : kBandRows;
    const bool row_on = ln < rows;
    uint32_t ft = row_on ? raw[img_base + (size_t)(r0 + ln) * stride] : 0u;
    if (ft > 4u) {
      bad_filter = true;
      ft = 0;
    }
    uint32_t cur = 0, b_before = 0;
    const int t_end = W + rows - 1;
    for (int t0 = 0; t0 < t_end; t0 += kStepTile) {
      wave_sync();
      for (int rr = 0; rr < rows; ++rr) {            // rr, xs, xe: one value for the wavefront
        const int xs = t0 - rr > 0 ? t0 - rr : 0, xe = t0 - rr + kStepTile < W ? t0 - rr + kStepTile : W;
        if (xs >= xe) continue;
        const size_t gs = img_base + (size_t)(r0 + rr) * stride + 1u + (size_t)xs * BPP, al = gs & ~(size_t)3;
        const int ndw = (int)((gs - al) + (size_t)(xe - xs) * BPP + 3u) / 4;      // <= 65
        for (int i = ln; i < ndw; i += kUnfThreads) tile_in[rr * kInPitchDw + i] = load_dword(raw, al + 4u * (size_t)i, raw_total);
      }
      wave_sync();
      const int my_xs = t0 - ln > 0 ? t0 - ln : 0;
      const uint32_t my_off = (uint32_t)((img_base + (size_t)(r0 + ln) * stride + 1u + (size_t)my_xs * BPP) & 3u);
      for (int s = 0; s < kStepTile; ++s) {
        const int x = t0 + s - ln;
        const uint32_t up = (uint32_t)__shfl_up((int)cur, 1, kUnfThreads);       // lane l - 1's pixel x, made one step ago
        const bool on = row_on && x >= 0 && x < W;
        uint32_t b = up;
        if (ln == 0) {
          b = 0;
          if (on)
            for (int k = 0; k < BPP; ++k) b |= (uint32_t)prev_rd[x * BPP + k] << (8 * k);
        }
        if (on) {
          const uint32_t a = x > 0 ? cur : 0u, c = x > 0 ? b_before : 0u;
          const uint32_t at = (uint32_t)ln * (kInPitchDw * 4) + my_off + (uint32_t)(x - my_xs) * BPP;
          uint32_t px = 0;
          for (int k = 0; k < BPP; ++k) {
            const uint32_t v = in_bytes[at + k] + predict(ft, (a >> (8 * k)) & 255u, (b >> (8 * k)) & 255u, (c >> (8 * k)) & 255u);
            px |= (v & 255u) << (8 * k);
          }
          cur = px;
          if (ln == kBandRows - 1)
            for (int k = 0; k < BPP; ++k) prev_wr[x * BPP + k] = (uint8_t)(px >> (8 * k));
          const uint32_t o = convert<MODE>(px, pal, entries, &bad_index);
          for (int k = 0; k < oc; ++k) tile_out[ln * kOutPitch + (x - my_xs) * oc + k] = (uint8_t)(o >> (8 * k));
        }
        b_before = b;
      }
      wave_sync();
      for (int rr = 0; rr < rows; ++rr) {
        const int xs = t0 - rr > 0 ? t0 - rr : 0, xe = t0 - rr + kStepTile < W ? t0 - rr + kStepTile : W;
        if (xs >= xe) continue;
        const size_t go = (((size_t)img * H + (size_t)(r0 + rr)) * W + (size_t)xs) * oc;
        const int nb = (xe - xs) * oc;                                            // <= 192
        for (int j = ln; j < nb; j += kUnfThreads) frames[go + j] = tile_out[rr * kOutPitch + j];
      }
    }
  }
  const bool any_filter = __ballot(bad_filter) != 0, any_index = __ballot(bad_index) != 0;
  if (ln == 0) status[img] = any_filter ? TBN_PNG_ST_FILTER : (any_index ? TBN_PNG_ST_PALETTE : 0);
}

// true when image row `im` may be read as it says
__host__ __device__ __forceinline__ bool image_ok(const tbn_png_image& im, size_t in_bytes, int colour_type) {
  return (im.in_off & 3u) == 0 && im.in_len < (1u << 31) && im.in_off <= in_bytes && im.in_len <= in_bytes - im.in_off &&
         (colour_type != 3 || (im.palette_off <= in_bytes && TBN_PNG_PALETTE_BYTES <= in_bytes - im.palette_off));
}

__global__ __launch_bounds__(kInfThreads) void png_inflate_kernel(const uint8_t* __restrict__ in, size_t in_bytes,
                                                                  const tbn_png_image* __restrict__ images, uint32_t raw_bytes,
                                                                  int colour_type, uint8_t* __restrict__ out, int* __restrict__ status,
                                                                  int* __restrict__ info) {
  __shared__ Tables tables;
  __shared__ uint32_t ring[2 * kChunk / 4];
  __shared__ uint8_t win[kWin];
  const int i = blockIdx.x, ln = threadIdx.x;
  const tbn_png_image im = images[i];
  int st = TBN_INF_ROW;
  uint32_t produced = 0;
  if (image_ok(im, in_bytes, colour_type)) {       // depends on the row alone: workgroup-uniform
    DevIO io{in + im.in_off, im.in_len, out + (size_t)i * raw_bytes, win, ring, kNoBase, ln};
    st = inflate_stream(io, tables, im.in_len, raw_bytes, &produced);
  }
  if (ln == 0) {
    status[i] = st;
    info[i] = (int)produced;
  }
}

__global__ __launch_bounds__((int)kAdlerPieces) void png_adler_kernel(const tbn_png_image* __restrict__ images,
                                                                      const uint8_t* __restrict__ out, uint32_t raw_bytes,
                                                                      int* __restrict__ status) {
  __shared__ uint32_t pa[kAdlerPieces], pb[kAdlerPieces];
  const int i = blockIdx.x, t = threadIdx.x;
  if (status[i] != TBN_INF_OK) return;             // one value for the workgroup: the inflate launch has completed
  const uint32_t piece = adler_piece_len(raw_bytes);
  const uint64_t lo = (uint64_t)t * piece, hi = lo + piece;
  adler_piece(out + (size_t)i * raw_bytes, (uint32_t)(lo < raw_bytes ? lo : raw_bytes), (uint32_t)(hi < raw_bytes ? hi : raw_bytes),
              &pa[t], &pb[t]);
  __syncthreads();
  if (t == 0 && adler_fold_all(pa, pb, raw_bytes) != images[i].adler) status[i] = TBN_PNG_ST_ADLER;
}

int check_geometry(const char* fn, const tbn_png_geometry* g, int n_img, int oc) {
  TBN_REQUIRE(g != nullptr, "%s: null geometry", fn);
  TBN_REQUIRE(n_img >= 0, "%s: n_img %d is negative", fn, n_img);
  const int ct = g->colour_type;
  const int bpp = ct == 0 ? 1 : ct == 2 ? 3 : ct == 3 ? 1 : ct == 4 ? 2 : ct == 6 ? 4 : 0;
  TBN_REQUIRE(bpp != 0 && g->bpp == bpp, "%s: colour type %d with %d bytes per pixel is not a PNG geometry", fn, ct, g->bpp);
  TBN_REQUIRE(g->width >= 1 && g->height >= 1, "%s: invalid image size %dx%d", fn, g->width, g->height);
  TBN_REQUIRE_OR(TBN_ERR_UNSUPPORTED, (uint64_t)g->width * bpp <= TBN_PNG_MAX_ROW_BYTES,
                 "%s: a scanline of %d pixels x %d bytes is not supported (at most %d bytes)", fn, g->width, bpp, TBN_PNG_MAX_ROW_BYTES);
  const uint64_t raw = (uint64_t)g->height * (1u + (uint64_t)g->width * bpp);
  TBN_REQUIRE(raw == g->raw_bytes && raw < (1ull << 31), "%s: raw_bytes %zu is not height * (1 + width * bpp) below 2^31", fn, g->raw_bytes);
  TBN_REQUIRE(oc == 3 || (oc == 1 && (ct == 0 || ct == 4)),
              "%s: out_channels %d with colour type %d (3, or 1 for the gray types 0 and 4: colour read as gray is not supported)", fn, oc, ct);
  return TBN_OK;
}

int launch_unfilter(const char* fn, const uint8_t* raw, const uint8_t* pal_base, const tbn_png_image* images, int n_img,
                    const tbn_png_geometry* g, int oc, uint8_t* frames, int* status, int keep, hipStream_t st) {
  return dispatch_mode(g->colour_type, [&](auto bpp, auto mode) {
    TBN_KLAUNCH((png_unfilter_kernel<decltype(bpp)::value, decltype(mode)::value>), dim3((unsigned)n_img), dim3(kUnfThreads), 0, st, raw,
                (size_t)n_img * g->raw_bytes, (uint32_t)g->raw_bytes, pal_base, images, g->width, g->height, oc, frames, status, keep);
    TBN_CHECK_LAUNCH(fn);
    return TBN_OK;
  });
}

}  // namespace

// ---- the container (host) ----------------------------------------------------------------------------------------------
extern "C" int tbn_png_parse(const unsigned char* data, size_t size, tbn_png_geometry* out) {
  char err[256] = "";
  const int rc = tbn_png::parse(data, size, out, err, sizeof(err));
  if (rc) tbn_set_error("%s", err);
  return rc;
}

extern "C" int tbn_png_parse_header(const unsigned char* data, size_t size, tbn_png_geometry* out) {
  char err[256] = "";
  const int rc = tbn_png::parse_header(data, size, out, err, sizeof(err));
  if (rc) tbn_set_error("%s", err);
  return rc;
}

extern "C" size_t tbn_png_gather_bytes(size_t idat_bytes) { return tbn_png::gather_bytes(idat_bytes); }

extern "C" int tbn_png_gather(const unsigned char* data, size_t size, const tbn_png_geometry* expect, unsigned char* zstream,
                              unsigned char* palette_bgr, uint32_t* deflate_begin, uint32_t* deflate_end, uint32_t* adler) {
  char err[256] = "";
  const int rc = tbn_png::gather(data, size, expect, zstream, palette_bgr, deflate_begin, deflate_end, adler, err, sizeof(err));
  if (rc) tbn_set_error("%s", err);
  return rc;
}

extern "C" int tbn_png_limits(int* band_rows, int* step_tile, int* max_row_bytes) {
  TBN_REQUIRE(band_rows && step_tile && max_row_bytes, "png_limits: null argument");
  *band_rows = kBandRows;
  *step_tile = kStepTile;
  *max_row_bytes = TBN_PNG_MAX_ROW_BYTES;
  return TBN_OK;
}

// ---- the device half -----------------------------------------------------------------------------------------------------
extern "C" int tbn_png_unfilter(const unsigned char* raw_dev, const unsigned char* palette_dev, int n_img,
                                const tbn_png_geometry* geometry, int out_channels, unsigned char* frames_dev, int* status_dev,
                                void* stream) {
  const char* fn = "png_unfilter";
  TBN_TRY(check_geometry(fn, geometry, n_img, out_channels));
  if (n_img == 0) return TBN_OK;
  TBN_REQUIRE(raw_dev != nullptr && frames_dev != nullptr && status_dev != nullptr, "%s: null argument", fn);
  TBN_REQUIRE(geometry->colour_type != 3 || palette_dev != nullptr, "%s: colour type 3 needs the palettes", fn);
  TBN_REQUIRE(((uintptr_t)raw_dev & 3) == 0 && ((uintptr_t)status_dev & 3) == 0, "%s: raw_dev and status_dev must be 4-byte aligned", fn);
  return launch_unfilter(fn, raw_dev, palette_dev, nullptr, n_img, geometry, out_channels, frames_dev, status_dev, 0, (hipStream_t)stream);
}

extern "C" size_t tbn_png_workspace_bytes(const tbn_png_geometry* geometry, int n_img) {
  if (check_geometry("png_workspace_bytes", geometry, n_img, 3) != TBN_OK) return 0;
  return align_up((size_t)(n_img > 0 ? n_img : 1) * geometry->raw_bytes, 16);
}

static int check_decode_args(const char* fn, const void* in, const tbn_png_image* images, const void* frames, const void* ws,
                             const int* status, const int* info) {
  TBN_REQUIRE(in != nullptr && images != nullptr && frames != nullptr && ws != nullptr && status != nullptr && info != nullptr,
              "%s: null argument", fn);
  TBN_REQUIRE(((uintptr_t)in & 3) == 0 && ((uintptr_t)images & 7) == 0 && ((uintptr_t)ws & 3) == 0 && ((uintptr_t)status & 3) == 0 &&
                  ((uintptr_t)info & 3) == 0,
              "%s: `in`, the workspace, status and info must be 4-byte aligned, the image table 8-byte aligned", fn);
  return TBN_OK;
}

extern "C" int tbn_png_decode(const void* in_dev, size_t in_bytes, const tbn_png_image* images_dev, int n_img,
                              const tbn_png_geometry* geometry, int out_channels, unsigned char* frames_dev, void* workspace,
                              int* status_dev, int* info_dev, void* stream) {
  const char* fn = "png_decode";
  TBN_TRY(check_geometry(fn, geometry, n_img, out_channels));
  if (n_img == 0) return TBN_OK;
  TBN_TRY(check_decode_args(fn, in_dev, images_dev, frames_dev, workspace, status_dev, info_dev));
  hipStream_t st = (hipStream_t)stream;
  TBN_KLAUNCH(png_inflate_kernel, dim3((unsigned)n_img), dim3(kInfThreads), 0, st, (const uint8_t*)in_dev, in_bytes, images_dev,
              (uint32_t)geometry->raw_bytes, geometry->colour_type, (uint8_t*)workspace, status_dev, info_dev);
  TBN_CHECK_LAUNCH(fn);
  TBN_KLAUNCH(png_adler_kernel, dim3((unsigned)n_img), dim3(kAdlerPieces), 0, st, images_dev, (const uint8_t*)workspace,
              (uint32_t)geometry->raw_bytes, status_dev);
  TBN_CHECK_LAUNCH(fn);
  return launch_unfilter(fn, (const uint8_t*)workspace, (const uint8_t*)in_dev, images_dev, n_img, geometry, out_channels, frames_dev,
                         status_dev, 1, st);
}

// ---- the host twins: no GPU call, all pointers host memory ---------------------------------------------------------------
extern "C" int tbn_png_unfilter_host(const unsigned char* raw, const unsigned char* palette, int n_img, const tbn_png_geometry* geometry,
                                     int out_channels, unsigned char* frames, int* status) {
  const char* fn = "png_unfilter_host";
  TBN_TRY(check_geometry(fn, geometry, n_img, out_channels));
  if (n_img == 0) return TBN_OK;
  TBN_REQUIRE(raw != nullptr && frames != nullptr && status != nullptr, "%s: null argument", fn);
  TBN_REQUIRE(geometry->colour_type != 3 || palette != nullptr, "%s: colour type 3 needs the palettes", fn);
  const size_t frame_bytes = (size_t)geometry->height * geometry->width * out_channels;
  for (int i = 0; i < n_img; ++i)
    status[i] = unfilter_host(geometry->colour_type, raw + (size_t)i * geometry->raw_bytes, palette_of(palette, nullptr, i),
                              geometry->width, geometry->height, out_channels, frames + i * frame_bytes);
  return TBN_OK;
}

extern "C" int tbn_png_decode_host(const void* in, size_t in_bytes, const tbn_png_image* images, int n_img,
                                   const tbn_png_geometry* geometry, int out_channels, unsigned char* frames, void* workspace,
                                   int* status, int* info) {
  const char* fn = "png_decode_host";
  TBN_TRY(check_geometry(fn, geometry, n_img, out_channels));
  if (n_img == 0) return TBN_OK;
  TBN_TRY(check_decode_args(fn, in, images, frames, workspace, status, info));
  const uint32_t raw_bytes = (uint32_t)geometry->raw_bytes;
  const size_t frame_bytes = (size_t)geometry->height * geometry->width * out_channels;
  for (int i = 0; i < n_img; ++i) {
    const tbn_png_image& im = images[i];
    uint8_t* raw = (uint8_t*)workspace + (size_t)i * raw_bytes;
    int st = TBN_INF_ROW;
    uint32_t produced = 0;
    if (image_ok(im, in_bytes, geometry->colour_type))
      st = decode_image_host((const uint8_t*)in + im.in_off, im.in_len, im.adler, palette_of((const uint8_t*)in, images, i),
                             geometry->colour_type, geometry->width, geometry->height, out_channels, raw, frames + i * frame_bytes,
                             &produced);
    status[i] = st;
    info[i] = (int)produced;
  }
  return TBN_OK;
}
