// Memory and equality check of the PNG host code (attention_based_tbn_amd/csrc/tbn_png_host.h: the container parser, the
// gather and the host twins of the kernels in csrc/png.hip; tbn_png_core.h and tbn_inflate.h, which the kernels are built
// from as well) as a plain executable.  Nothing of HIP is involved.
//
//   python -m tests.png_util --dump /tmp/png_cases
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iattention_based_tbn_amd/csrc
//       scripts/png_check.cpp -o /tmp/png_check                                        (one command line)
//   /tmp/png_check /tmp/png_cases/*.png
//
// Per NAME.png (with NAME.bgr beside it: the written pixels as B, G, R frame bytes): the file in a heap block of EXACTLY
// its length is parsed and gathered into a block of EXACTLY tbn_png::gather_bytes(), and decoded into scanline and frame
// blocks of EXACTLY their sizes, so that a read or write past any of them is a report.  The result must be status 0 and
// NAME.bgr's bytes.  Then every truncation of the file (every length of files up to 4 KiB, 300 seeded lengths of larger
// ones) must be refused by the parser; every truncation of the gathered deflate data (same rule) must end in a non-zero
// status; and seeded single-byte corruptions of the container (120), of the zlib stream (200) and of the inflated
// scanlines (120) must each end -- refused, with a status, or with status 0; status 0 is then checked against a textbook
// byte-by-byte Adler-32 of the inflated scanlines: it means "these bytes carry the file's Adler-32", and Adler-32 being weak
// on periodic data a damaged stream can really do that (the seeded runs meet one such collision, which zlib accepts too).
// `--pick NAME` prints, for the file whose path contains NAME, seeded corruptions of its ZLIB STREAM by outcome: the first
// the decoder core refuses mid-stream and the first that inflates to the full size and fails only the Adler-32 (the damaged
// inputs of tests/test_png_gpu.py), as (offset in the zlib stream, new value).  Exit status 0 and "ok" = clean.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "tbn_png_host.h"

using namespace tbn_png;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {    // xorshift64*: seeded, no library state
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

static bool read_file(const std::string& path, std::vector<uint8_t>* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  out->resize((size_t)n);
  const bool ok = n == 0 || fread(out->data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  return ok;
}

// an exact-size heap copy: the sanitizer's red zones begin at its last byte
struct Exact {
  uint8_t* p;
  size_t n;
  Exact(const uint8_t* src, size_t len) : p((uint8_t*)malloc(len ? len : 1)), n(len) {
    if (src && len) memcpy(p, src, len);
  }
  explicit Exact(size_t len) : Exact(nullptr, len) { memset(p, 0xA5, len ? len : 1); }
  ~Exact() { free(p); }
  Exact(const Exact&) = delete;
};

struct Gathered {
  tbn_png_geometry geo;
  std::vector<uint8_t> z;      // gather_bytes() long
  uint8_t palette[TBN_PNG_PALETTE_BYTES];
  uint32_t begin, end, adler;
};

// parse + gather of `n` file bytes -> 0 or the refusal's code
static int gather_file(const uint8_t* file, size_t n, Gathered* g) {
  char err[256];
  Exact f(file, n);
  int rc = parse(f.p, f.n, &g->geo, err, sizeof(err));
  if (rc) return rc;
  Exact z(gather_bytes(g->geo.idat_bytes));
  Exact pal((size_t)TBN_PNG_PALETTE_BYTES);
  rc = gather(f.p, f.n, &g->geo, z.p, pal.p, &g->begin, &g->end, &g->adler, err, sizeof(err));
  if (rc) return rc;
  g->z.assign(z.p, z.p + z.n);
  memcpy(g->palette, pal.p, TBN_PNG_PALETTE_BYTES);
  return 0;
}

// the deflate data [begin, begin + len) of `z` -> status; the frame when `frame` is given
static int decode(const Gathered& g, const std::vector<uint8_t>& z, uint32_t len, std::vector<uint8_t>* frame) {
  Exact in(z.data() + g.begin, len);                 // exactly the deflate data: nothing behind it may be read
  Exact pal(g.palette, TBN_PNG_PALETTE_BYTES);
  Exact raw(g.geo.raw_bytes);
  const size_t fb = (size_t)g.geo.width * g.geo.height * 3;
  Exact out(fb);
  uint32_t produced = 0;
  const int st = decode_image_host(in.p, len, g.adler, pal.p, g.geo.colour_type, g.geo.width, g.geo.height, 3, raw.p, out.p, &produced);
  if (produced > g.geo.raw_bytes) {
    printf("produced %u of %zu\n", produced, g.geo.raw_bytes);
    exit(1);
  }
  if (st == 0) {     // the chunked Adler-32 said yes: so must the textbook one
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < raw.n; ++i) {
      a = (a + raw.p[i]) % 65521u;
      b = (b + a) % 65521u;
    }
    if (((b << 16) | a) != g.adler) {
      printf("status 0 with Adler-32 %08x, the stream says %08x\n", (b << 16) | a, g.adler);
      exit(1);
    }
  }
  if (frame) frame->assign(out.p, out.p + fb);
  return st;
}

static int fail(const std::string& path, const char* what, long a = 0, long b = 0) {
  printf("FAIL %s: %s (%ld, %ld)\n", path.c_str(), what, a, b);
  return 1;
}

static int check_file(const std::string& path, bool pick) {
  std::vector<uint8_t> file, want;
  if (!read_file(path, &file)) return fail(path, "cannot read");
  if (!read_file(path.substr(0, path.size() - 4) + ".bgr", &want)) return fail(path, "no .bgr beside it");
  Gathered g;
  if (gather_file(file.data(), file.size(), &g) != 0) return fail(path, "the good file is refused");
  const uint32_t dlen = g.end - g.begin;
  std::vector<uint8_t> frame;
  if (decode(g, g.z, dlen, &frame) != 0) return fail(path, "the good file has a status");
  if (frame != want) return fail(path, "the frame differs from the written pixels");
  if (pick) {
    bool have_mid = false, have_adler = false;
    for (int k = 0; k < 4000 && !(have_mid && have_adler); ++k) {
      std::vector<uint8_t> z = g.z;
      const uint32_t at = rnd(dlen), v = rnd(256);
      if (z[g.begin + at] == v) continue;
      z[g.begin + at] = (uint8_t)v;
      const int st = decode(g, z, dlen, nullptr);
      if (st >= 1 && st <= 9 && !have_mid) {
        printf("refused mid-stream: offset %u value %u status %d\n", g.begin - TBN_PNG_ZSTREAM_LEAD + at, v, st);
        have_mid = true;
      }
      if (st == TBN_PNG_ST_ADLER && !have_adler) {
        printf("adler only: offset %u value %u status %d\n", g.begin - TBN_PNG_ZSTREAM_LEAD + at, v, st);
        have_adler = true;
      }
    }
    return 0;
  }
  // truncations of the file: never a success
  const bool all = file.size() <= 4096;
  for (size_t k = 0; k < (all ? file.size() : 300); ++k) {
    const size_t n = all ? k : rnd((uint32_t)file.size());
    Gathered t;
    if (gather_file(file.data(), n, &t) == 0) return fail(path, "a truncated file is accepted", (long)n);
  }
  // truncations of the deflate data: never status 0
  const bool all_d = dlen <= 4096;
  for (uint32_t k = 0; k < (all_d ? dlen : 300); ++k) {
    const uint32_t n = all_d ? k : rnd(dlen);
    if (decode(g, g.z, n, nullptr) == 0) return fail(path, "truncated deflate data decode with status 0", (long)n);
  }
  // corruptions of the container
  for (int k = 0; k < 120; ++k) {
    std::vector<uint8_t> f = file;
    f[rnd((uint32_t)f.size())] = (uint8_t)rnd(256);
    Gathered t;
    if (gather_file(f.data(), f.size(), &t) != 0) continue;
    if (t.geo.raw_bytes > (1u << 24)) continue;     // a corrupted size that is still a valid header: nothing to decode
    decode(t, t.z, t.end - t.begin, nullptr);
  }
  // corruptions of the deflate data
  for (int k = 0; k < 200; ++k) {
    std::vector<uint8_t> z = g.z;
    const uint32_t at = rnd(dlen);
    z[g.begin + at] = (uint8_t)rnd(256);
    decode(g, z, dlen, nullptr);
  }
  // corruptions of the inflated scanlines: any status, any pixels, no report
  {
    Exact in(g.z.data() + g.begin, dlen);
    std::vector<uint8_t> raw(g.geo.raw_bytes), out((size_t)g.geo.width * g.geo.height * 3);
    tbn_inflate::Tables t;
    tbn_inflate::HostIO io{in.p, dlen, raw.data()};
    uint32_t produced = 0;
    if (tbn_inflate::inflate_stream(io, t, dlen, (uint32_t)raw.size(), &produced) != 0) return fail(path, "inflate");
    for (int k = 0; k < 120; ++k) {
      Exact r(raw.data(), raw.size());
      r.p[rnd((uint32_t)r.n)] = (uint8_t)rnd(256);
      if (k % 3 == 0) r.p[(size_t)rnd((uint32_t)g.geo.height) * (1 + (size_t)g.geo.width * g.geo.bpp)] = (uint8_t)(5 + rnd(251));
      Exact pal(g.palette, TBN_PNG_PALETTE_BYTES);
      Exact o(out.size());
      const int st = unfilter_host(g.geo.colour_type, r.p, pal.p, g.geo.width, g.geo.height, 3, o.p);
      if (st != 0 && st != TBN_PNG_ST_FILTER && st != TBN_PNG_ST_PALETTE) return fail(path, "unfilter status", st);
      if (k % 3 == 0 && st != TBN_PNG_ST_FILTER) return fail(path, "a filter byte above 4 is not status 21", st);
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  std::string pick;
  std::vector<std::string> paths;
  for (int i = 1; i < argc; ++i) {
    if (std::string(argv[i]) == "--pick" && i + 1 < argc) pick = argv[++i];
    else paths.push_back(argv[i]);
  }
  if (paths.empty()) {
    printf("usage: png_check [--pick NAME] FILE.png ...\n");
    return 2;
  }
  int bad = 0, n = 0;
  for (const std::string& p : paths) {
    if (!pick.empty() && p.find(pick) == std::string::npos) continue;
    bad += check_file(p, !pick.empty());
    ++n;
  }
  if (bad) return 1;
  if (pick.empty()) printf("ok: %d files\n", n);
  return 0;
}
