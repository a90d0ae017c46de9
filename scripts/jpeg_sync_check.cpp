// Memory and equality check of the self-synchronising JPEG entropy decoder (attention_based_tbn_amd/csrc/tbn_jpeg_sync.h:
// the host pack stage and the decoder core the kernel in csrc/jpeg_entropy.hip is built from) as a plain executable.
// The relaxation runs serially here, lanes in a loop, phase by phase as the kernel runs them.  Nothing of HIP is involved.
//
//   python scripts/make_jpeg_golden.py --dump /tmp/jpeg_cases
//   python scripts/make_jpeg_sync_golden.py --dump /tmp/jpeg_cases
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iattention_based_tbn_amd/csrc
//       scripts/jpeg_sync_check.cpp -o /tmp/jpeg_sync_check                            (one command line)
//   /tmp/jpeg_sync_check /tmp/jpeg_cases/*.jpg
//
// Per file, at subsequence sizes auto, 64 and 96, from the scan's bytes as packed and from pre-swapped dwords (the
// kernel's LDS copy): pack into a record of EXACTLY the declared capacity, decode from a
// heap copy of EXACTLY the bytes used into a coefficient buffer of EXACTLY coef_count elements, and compare with
// tbn_jpeg_host_entropy_decode: equal coefficients whenever the status is 0 and the host stage accepts; where the host
// stage refuses, a refusal by the pack stage, a non-zero status, or the documented strictness gap (stray bytes between
// the last block and the next marker).  Then every truncation (every offset of files up to 4 KiB, 400 seeded offsets
// of larger ones: the pack stage must refuse each) and 200 seeded single-byte corruptions of the scan.  A file of more
// than 1024 intervals must come back unpacked.  `--pick NAME` prints, for the file whose path contains NAME, the first
// seeded corruption the host stage accepts and the first it refuses with "invalid Huffman code" (the two cases of
// tests/test_jpeg_sync_gpu.py).  Exit status 0 and "ok" = clean.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "tbn_jpeg_sync.h"

using namespace tbn_jpeg;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {    // xorshift64*: seeded, no library state
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

struct Aligned {     // a heap block of exactly n bytes, 16-byte aligned
  unsigned char* p;
  explicit Aligned(size_t n) : p((unsigned char*)aligned_alloc(16, n ? n : 16)) {}    // n is a multiple of 16 here
  ~Aligned() { free(p); }
  Aligned(const Aligned&) = delete;
  Aligned& operator=(const Aligned&) = delete;
};

// The kernel's phases, serially.  coef[coef_count] must be zero on entry.  Returns the status bits.
// kSwapped: decode from a copy of the scan whose dwords are swapped beforehand, as the kernel's LDS copy is
template <bool kSwapped>
static uint32_t sync_image(const unsigned char* rec, size_t rec_bytes, const tbn_jpeg_geometry& geo, uint32_t s_req,
                           int16_t* coef, uint32_t* lanes_out, uint32_t* rounds_out) {
  *lanes_out = *rounds_out = 0;
  if (rec_bytes < kPackedIntervalsOff) return TBN_JPEG_ST_RECORD;
  PackedHeader h;
  memcpy(&h, rec, sizeof(h));
  const uint64_t scan_end = (uint64_t)h.scan_off + ((h.scan_bytes + 15ull) & ~15ull);
  if (h.magic != TBN_JPEG_SYNC_MAGIC || h.n_intervals < 1 || h.n_intervals > TBN_JPEG_SYNC_MAX_LANES ||
      h.intervals_off != kPackedIntervalsOff || (h.scan_off & 15) || h.scan_off < h.intervals_off + 8ull * h.n_intervals ||
      scan_end > rec_bytes || h.scan_bytes >= (1u << 28))
    return TBN_JPEG_ST_RECORD;
  const DevTables* tab = (const DevTables*)(rec + kPackedTablesOff);
  const uint32_t* iv = (const uint32_t*)(rec + h.intervals_off);
  const uint32_t nwords = (h.scan_bytes + 3) / 4, n_int = h.n_intervals, total_bits = 8 * h.scan_bytes;
  const uint32_t* words = (const uint32_t*)(rec + h.scan_off);
  std::vector<uint32_t> swapped(kSwapped ? nwords : 0);      // exactly nwords: a read past it is a report
  if (kSwapped) {
    for (uint32_t i = 0; i < nwords; ++i) swapped[i] = sync_bswap(words[i]);
    words = swapped.data();
  }
  uint32_t max_bits = 0;
  for (uint32_t i = 0; i < n_int; ++i) {
    if ((uint64_t)iv[2 * i] + iv[2 * i + 1] > total_bits) return TBN_JPEG_ST_RECORD;
    max_bits = std::max(max_bits, iv[2 * i + 1]);
  }
  SyncGeom g;
  sync_geom(&geo, &g);
  uint8_t slots[16];
  sync_block_slots(tab, g, slots);
  auto lanes_at = [&](uint32_t S) {
    uint64_t n = 0;
    for (uint32_t i = 0; i < n_int; ++i) n += sync_interval_lanes(iv[2 * i + 1], S);
    return n;
  };
  uint32_t S = s_req ? s_req : TBN_JPEG_SYNC_DEFAULT_BITS;
  if (lanes_at(S) > TBN_JPEG_SYNC_MAX_LANES) {        // the smallest multiple of 32 at which the lanes fit
    uint32_t lo = S / 32, hi = std::max((max_bits + 31) / 32, lo + 1);     // lanes_at(32 lo) too many, lanes_at(32 hi) <= n_int
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (lanes_at(32 * mid) > TBN_JPEG_SYNC_MAX_LANES) lo = mid; else hi = mid;
    }
    S = 32 * hi;
  }
  const uint32_t lanes = (uint32_t)lanes_at(S);
  std::vector<uint32_t> first(n_int + 1, 0);
  for (uint32_t i = 0; i < n_int; ++i) first[i + 1] = first[i] + sync_interval_lanes(iv[2 * i + 1], S);
  std::vector<uint32_t> lane_int(lanes), sub_end(lanes), int_end(lanes), cnt(lanes, 0), ev(lanes, 0);
  std::vector<SyncState> entry(lanes), exit_(lanes), guess(lanes);
  std::vector<char> dirty(lanes, 1), is_first(lanes, 0);
  for (uint32_t i = 0; i < n_int; ++i)
    for (uint32_t l = first[i]; l < first[i + 1]; ++l) {
      const uint32_t k = l - first[i], start = iv[2 * i], end = start + iv[2 * i + 1];
      lane_int[l] = i;
      int_end[l] = end;
      sub_end[l] = (uint32_t)std::min<uint64_t>((uint64_t)start + (uint64_t)(k + 1) * S, end);
      entry[l] = SyncState{start + k * S, 0};
      guess[l] = SyncState{sub_end[l], 0};
      is_first[l] = k == 0;
    }
  SyncNoSink none;
  uint32_t rounds = 0;
  for (uint32_t r = 1; r <= lanes; ++r) {             // the hard bound: lane k is right after k rounds
    for (uint32_t l = 0; l < lanes; ++l)
      if (dirty[l]) {
        SyncState st = entry[l];
        ev[l] = sync_decode<kSwapped>(tab, words, nwords, sub_end[l], int_end[l], g.bpm, slots, guess[l], &st, &cnt[l], none);
        exit_[l] = st;
      }
    bool any = false;
    for (uint32_t l = 0; l < lanes; ++l) {
      dirty[l] = 0;
      if (!is_first[l] && (exit_[l - 1].p != entry[l].p || exit_[l - 1].bz != entry[l].bz)) {
        entry[l] = exit_[l - 1];
        dirty[l] = 1;
        any = true;
      }
    }
    rounds = r;
    if (!any) break;
  }
  *lanes_out = lanes;
  *rounds_out = rounds;
  // exclusive scan of the block counts, validation
  std::vector<uint32_t> incl(lanes + 1, 0);
  for (uint32_t l = 0; l < lanes; ++l) incl[l + 1] = incl[l] + cnt[l];
  uint32_t status = 0;
  for (uint32_t l = 0; l < lanes; ++l) {
    if (ev[l] & TBN_JPEG_EV_CODE) status |= TBN_JPEG_ST_CODE;
    if (ev[l] & TBN_JPEG_EV_RUN) status |= TBN_JPEG_ST_RUN;
  }
  for (uint32_t i = 0; i < n_int; ++i) {
    const bool has = first[i + 1] > first[i];
    status |= sync_interval_status(incl[first[i + 1]] - incl[first[i]], sync_interval_blocks(g, h.restart_interval, i), has,
                                   has ? exit_[first[i + 1] - 1] : SyncState{0, 0}, iv[2 * i] + iv[2 * i + 1]);
  }
  if (status) return status;
  // the write pass
  for (uint32_t l = 0; l < lanes; ++l) {
    const uint32_t i = lane_int[l];
    const uint32_t base = (uint32_t)((uint64_t)i * h.restart_interval * g.bpm);
    SyncCoefSink sink{coef, &g, kZigzagToNatural, base + (incl[l] - incl[first[i]]),
                      base + sync_interval_blocks(g, h.restart_interval, i), 0xFFFFFFFFu, 0, false};
    SyncState st = entry[l];
    uint32_t n;
    sync_decode<kSwapped>(tab, words, nwords, sub_end[l], int_end[l], g.bpm, slots, guess[l], &st, &n, sink);
  }
  // DC differences -> DC values, per component in scan order, reset at every restart interval
  int pred[3] = {0, 0, 0};
  for (uint32_t mcu = 0; mcu < g.total_mcus; ++mcu) {
    if (h.restart_interval && mcu % h.restart_interval == 0) pred[0] = pred[1] = pred[2] = 0;
    for (int b = 0; b < g.bpm; ++b) {
      uint32_t off;
      if (!sync_block_offset(g, mcu * g.bpm + b, &off)) return status | TBN_JPEG_ST_BLOCKS;
      const int c = g.comp[b];
      pred[c] += coef[off];
      if (pred[c] < -32768 || pred[c] > 32767) return status | TBN_JPEG_ST_DC;
      coef[off] = (int16_t)pred[c];
    }
  }
  return status;
}

struct Outcome {
  int host_rc, pack_rc;
  bool packed;                 // false: more intervals than the lane limit
  uint32_t status[3];
  char host_err[256];
};

static const uint32_t kSizes[3] = {0, 64, 96};
static long n_equal = 0, n_routed = 0, n_gap = 0, n_calls = 0;

// pack + decode at the three sizes + compare with the host stage; false (with a message) on a violation
static bool check(const std::vector<unsigned char>& d, const tbn_jpeg_geometry& g, const char* what, Outcome* out) {
  std::vector<unsigned char> in(d);       // exact-size heap copy: a read past the end is a report
  std::vector<int16_t> want(g.coef_count);
  std::vector<uint16_t> wantq((size_t)g.components * 64), quant((size_t)g.components * 64);
  out->host_err[0] = 0;
  out->host_rc = tbn_jpeg_host_entropy_decode(in.data(), in.size(), &g, want.data(), wantq.data(), out->host_err, 256);
  tbn_jpeg_geometry pg;
  char err[256] = "";
  long long n_int = 1;
  if (tbn_jpeg_host_parse(in.data(), in.size(), &pg, err, sizeof(err)) == 0) {
    const long long mcus = (long long)(pg.blocks_w[0] / pg.hsamp[0]) * (pg.blocks_h[0] / pg.vsamp[0]);
    if (pg.restart_interval) n_int = (mcus + pg.restart_interval - 1) / pg.restart_interval;
  }
  const bool too_many = n_int > TBN_JPEG_SYNC_MAX_LANES;
  const size_t cap = tbn_jpeg_host_scan_pack_bytes(in.size(), too_many ? 1 : (size_t)n_int);
  Aligned rec(cap);
  int got_int = -1;
  size_t used = 0;
  out->pack_rc = tbn_jpeg_host_scan_pack(in.data(), in.size(), &g, rec.p, cap, TBN_JPEG_SYNC_MAX_LANES, quant.data(), &got_int,
                                         &used, err, sizeof(err));
  ++n_calls;
  out->packed = used != 0;
  if (out->pack_rc != 0) {
    if (!err[0] || used != 0) { fprintf(stderr, "%s: pack refusal without a message\n", what); return false; }
    if (out->host_rc == 0) { fprintf(stderr, "%s: the pack stage refuses (%s) what the host stage decodes\n", what, err); return false; }
    return true;
  }
  if (got_int != n_int || (too_many && used != 0)) {
    fprintf(stderr, "%s: interval count %d, expected %lld (used %zu)\n", what, got_int, n_int, used);
    return false;
  }
  if (too_many) return true;
  if (used > cap || used % 16) { fprintf(stderr, "%s: used %zu of %zu\n", what, used, cap); return false; }
  if (out->host_rc == 0 && quant != wantq) { fprintf(stderr, "%s: quantisation tables differ\n", what); return false; }
  Aligned exact(used);
  memcpy(exact.p, rec.p, used);
  for (int k = 0; k < 3; ++k) {
    std::vector<int16_t> coef(g.coef_count, 0);
    uint32_t lanes, rounds;
    const uint32_t st = sync_image<false>(exact.p, used, g, kSizes[k], coef.data(), &lanes, &rounds);
    {
      std::vector<int16_t> coef2(g.coef_count, 0);
      uint32_t lanes2, rounds2;
      const uint32_t st2 = sync_image<true>(exact.p, used, g, kSizes[k], coef2.data(), &lanes2, &rounds2);
      if (st2 != st || lanes2 != lanes || rounds2 != rounds || coef2 != coef) {
        fprintf(stderr, "%s: the two word forms disagree at S=%u\n", what, kSizes[k]);
        return false;
      }
    }
    n_calls += 2;
    out->status[k] = st;
    if (st == 0 && (rounds < 1 || rounds > lanes)) { fprintf(stderr, "%s: %u rounds with %u lanes\n", what, rounds, lanes); return false; }
    if (st == 0 && out->host_rc == 0) {
      if (coef != want) { fprintf(stderr, "%s: coefficients differ at S=%u\n", what, kSizes[k]); return false; }
      ++n_equal;
    } else if (st != 0 && out->host_rc == 0) {
      ++n_routed;                              // the host stage takes it: allowed, but never for an undamaged file
    } else if (st == 0) {
      const std::string m(out->host_err);     // the strictness gap: only the judgement of what follows the last block
      if (m.find("stray data where RST") == std::string::npos && m.find("no EOI marker") == std::string::npos &&
          m.find("where EOI is expected") == std::string::npos && m.find("more than one scan") == std::string::npos) {
        fprintf(stderr, "%s: status 0 at S=%u where the host stage refuses: %s\n", what, kSizes[k], out->host_err);
        return false;
      }
      ++n_gap;
    }
  }
  return true;
}

int main(int argc, char** argv) {
  std::string pick;
  std::vector<const char*> files;
  for (int a = 1; a < argc; ++a) {
    if (std::string(argv[a]) == "--pick" && a + 1 < argc) pick = argv[++a];
    else files.push_back(argv[a]);
  }
  if (files.empty()) {
    fprintf(stderr, "usage: %s [--pick NAME] FILE.jpg ...\n", argv[0]);
    return 2;
  }
  long decoded = 0, refused = 0, unpacked = 0;
  for (const char* path : files) {
    FILE* f = fopen(path, "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", path);
      return 2;
    }
    std::vector<unsigned char> d;
    unsigned char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + n);
    fclose(f);
    const bool must_refuse = std::string(path).find("refuse_") != std::string::npos;
    tbn_jpeg_geometry g;
    char err[256] = "";
    Outcome o;
    if (tbn_jpeg_host_parse(d.data(), d.size(), &g, err, sizeof(err)) != 0) {
      if (!must_refuse) { fprintf(stderr, "%s: parse failed: %s\n", path, err); return 1; }
      tbn_jpeg_geometry any;
      memset(&any, 0, sizeof(any));
      any.width = any.height = 16; any.components = 1; any.hsamp[0] = any.vsamp[0] = 1;
      any.blocks_w[0] = any.blocks_h[0] = 2; any.coef_count = 256;
      if (!check(d, any, path, &o) || o.pack_rc == 0) { fprintf(stderr, "%s: should have been refused\n", path); return 1; }
      ++refused;
      continue;
    }
    if (!check(d, g, path, &o)) return 1;
    if (o.host_rc != 0 || o.pack_rc != 0) { fprintf(stderr, "%s: refused: %s\n", path, o.host_err); return 1; }
    if (!o.packed) {
      ++unpacked;
      continue;
    }
    if (o.status[0] || o.status[1] || o.status[2]) {
      fprintf(stderr, "%s: status %u %u %u on an undamaged file\n", path, o.status[0], o.status[1], o.status[2]);
      return 1;
    }
    ++decoded;
    const int cuts = d.size() <= 4096 ? (int)d.size() : 400;
    for (int i = 0; i < cuts; ++i) {
      const size_t cut = d.size() <= 4096 ? (size_t)i : rnd((uint32_t)d.size());
      std::vector<unsigned char> t(d.begin(), d.begin() + cut);
      if (!check(t, g, path, &o)) return 1;
      if (o.pack_rc == 0) { fprintf(stderr, "%s: truncation at %zu was packed\n", path, cut); return 1; }
    }
    size_t scan = 0;
    for (size_t i = 2; i + 3 < d.size(); ++i)
      if (d[i] == 0xFF && d[i + 1] == 0xDA) {
        scan = i + 2 + ((size_t)d[i + 2] << 8 | d[i + 3]);
        break;
      }
    const bool picking = !pick.empty() && std::string(path).find(pick) != std::string::npos;
    bool have_accept = false, have_refuse = false;
    for (int i = 0; i < 200 && scan && scan < d.size(); ++i) {
      std::vector<unsigned char> c(d);
      const size_t at = scan + rnd((uint32_t)(d.size() - scan));
      const unsigned char v = (unsigned char)rnd(256);
      c[at] = v;
      char what[512];
      snprintf(what, sizeof(what), "%s with byte %zu = %u", path, at, (unsigned)v);
      if (!check(c, g, what, &o)) return 1;
      if (picking && v != d[at] && o.pack_rc == 0) {
        if (!have_accept && o.host_rc == 0 && !o.status[0] && !o.status[1]) {
          printf("pick accepted: byte %zu = %u (was %u)\n", at, (unsigned)v, (unsigned)d[at]);
          have_accept = true;
        }
        if (!have_refuse && o.host_rc != 0 && std::string(o.host_err).find("invalid Huffman code") != std::string::npos &&
            o.status[0] && o.status[1]) {
          printf("pick refused: byte %zu = %u (was %u): status %u / %u, host: %s\n", at, (unsigned)v, (unsigned)d[at],
                 o.status[0], o.status[1], o.host_err);
          have_refuse = true;
        }
      }
    }
  }
  printf("ok: %ld files decoded at 3 sizes, %ld refused, %ld left to the host stage; %ld calls, %ld equal decodes, "
         "%ld damaged streams routed to the host stage, %ld in the strictness gap\n",
         decoded, refused, unpacked, n_calls, n_equal, n_routed, n_gap);
  return 0;
}
