"""Writes tests/golden/inflate_cases.npz: the raw deflate streams (RFC 1951, no zlib or gzip wrapper) the inflate decoder
(csrc/tbn_inflate.h, csrc/inflate.hip) is tested on.  Bytes only: the expected output of a good stream is
zlib.decompress(stream, -15) at test time.

    python scripts/make_inflate_golden.py
    python scripts/make_inflate_golden.py --dump DIR    # DIR/NAME.deflate and DIR/NAME.out for scripts/inflate_check.cpp

A different zlib build may cut blocks elsewhere, so the bytes are committed and not re-made per run.  What each case is
FOR is a property of its block structure, so a small block walker (an inflate in Python that counts block types, the
largest distance and length, overlapping matches and matches that reach into an earlier block) asserts that structure
here, when the file is written, and the counts are stored beside the bytes (`structure`, JSON).  Streams zlib never
emits -- distances 32 507 .. 32 768, and every refusal -- are assembled by hand with a bit writer; keys starting with
`bad_` are refused by zlib.decompress."""
import io
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "inflate_cases.npz")

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


# ---------------------------------------------------------------------------------------------- the block walker
class _Bits(object):
    def __init__(self, data):
        self.v = int.from_bytes(data, "little")
        self.pos = 0
        self.n = 8 * len(data)

    def get(self, n):
        assert self.pos + n <= self.n, "stream ends early"
        r = (self.v >> self.pos) & ((1 << n) - 1)
        self.pos += n
        return r


def _codes(lens):
    """{(length, code): symbol} of a canonical Huffman code"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 16, 0
    for l in range(1, 16):
        c = (c + count[l - 1]) << 1
        nxt[l] = c
    table = {}
    for s, l in enumerate(lens):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def _sym(b, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | b.get(1)
        if (l, code) in table:
            return table[(l, code)]
    raise AssertionError("no such code")


def walk(stream):
    """-> (output bytes, structure dict) of a well-formed raw deflate stream"""
    b = _Bits(stream)
    out = bytearray()
    st = dict(stored=0, fixed=0, dynamic=0, matches=0, overlapping=0, cross_block=0, max_dist=0, max_len=0, literals=0,
              repeat_into_dist=0, empty_stored=0)
    while True:
        final, kind = b.get(1), b.get(2)
        start = len(out)
        if kind == 0:
            b.pos = (b.pos + 7) & ~7
            n, inv = b.get(16), b.get(16)
            assert n == (~inv & 0xFFFF)
            out += stream[b.pos // 8:b.pos // 8 + n]
            b.pos += 8 * n
            st["stored"] += 1
            st["empty_stored"] += n == 0
        else:
            assert kind in (1, 2)
            if kind == 1:
                lit = _codes([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
                dist = _codes([5] * 32)
                st["fixed"] += 1
            else:
                nl, nd, ncl = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
                cl = [0] * 19
                for i in range(ncl):
                    cl[CL_ORDER[i]] = b.get(3)
                clt, lens = _codes(cl), []
                while len(lens) < nl + nd:
                    s = _sym(b, clt)
                    before = len(lens)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + b.get(2))
                    elif s == 17:
                        lens += [0] * (3 + b.get(3))
                    else:
                        lens += [0] * (11 + b.get(7))
                    st["repeat_into_dist"] += before < nl < len(lens)
                assert len(lens) == nl + nd
                lit, dist = _codes(lens[:nl]), _codes(lens[nl:])
                st["dynamic"] += 1
            while True:
                s = _sym(b, lit)
                if s < 256:
                    out.append(s)
                    st["literals"] += 1
                elif s == 256:
                    break
                else:
                    n = LBASE[s - 257] + b.get(LEXT[s - 257])
                    d = _sym(b, dist)
                    d = DBASE[d] + b.get(DEXT[d])
                    assert d <= len(out)
                    st["matches"] += 1
                    st["overlapping"] += d < n
                    st["cross_block"] += len(out) - d < start
                    st["max_dist"], st["max_len"] = max(st["max_dist"], d), max(st["max_len"], n)
                    for _ in range(n):
                        out.append(out[-d])
        if final:
            break
    return bytes(out), {k: int(v) for k, v in st.items()}


# ---------------------------------------------------------------------------------------------- the bit writer
class Writer(object):
    def __init__(self):
        self.v, self.n = 0, 0

    def bits(self, value, n):          # n bits, least significant first (header fields, extra bits)
        self.v |= (value & ((1 << n) - 1)) << self.n
        self.n += n

    def code(self, value, n):          # a Huffman code: most significant bit first
        for i in range(n - 1, -1, -1):
            self.bits((value >> i) & 1, 1)

    def align(self):
        self.n = (self.n + 7) & ~7

    def fixed_sym(self, s):            # literal/length symbol of the fixed code
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def fixed_match(self, length, dist):
        ls = max(i for i in range(29) if LBASE[i] <= length)
        if length == 258:
            ls = 28
        self.fixed_sym(257 + ls)
        self.bits(length - LBASE[ls], LEXT[ls])
        ds = max(i for i in range(30) if DBASE[i] <= dist)
        self.code(ds, 5)
        self.bits(dist - DBASE[ds], DEXT[ds])

    def done(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def _deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, flush=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(flush) + c.compress(data[flush_at:]) + c.flush()


def _dynamic_header(w, cl_lens, final=1, nl=257, nd=1):
    """block header of a dynamic block with HLIT = nl, HDIST = nd and the given code-length code lengths {symbol: length}"""
    w.bits(final, 1)
    w.bits(2, 2)
    w.bits(nl - 257, 5)
    w.bits(nd - 1, 5)
    last = max(CL_ORDER.index(s) for s in cl_lens)
    w.bits(max(last + 1, 4) - 4, 4)
    for i in range(max(last + 1, 4)):
        w.bits(cl_lens.get(CL_ORDER[i], 0), 3)


def good_cases():
    rng = np.random.RandomState(1951)
    cases, want = {}, {}

    def add(name, stream, **structure):
        cases[name], want[name] = stream, structure

    add("stored_two_blocks", _deflate(rng.randint(0, 256, 70000).astype(np.uint8).tobytes(), 0), stored=("==", 2))
    add("incompressible_level6", _deflate(rng.randint(0, 256, 40000).astype(np.uint8).tobytes()), stored=(">=", 1),
        dynamic=("==", 0), fixed=("==", 0))
    add("fixed_with_matches", _deflate(rng.randint(0, 4, 3000).astype(np.uint8).tobytes(), 6, zlib.Z_FIXED), fixed=("==", 1),
        dynamic=("==", 0), matches=(">=", 100), overlapping=(">=", 1))
    add("zeros_distance_1", _deflate(bytes(5000)), dynamic=("==", 1), max_dist=("==", 1), max_len=("==", 258),
        overlapping=(">=", 10))
    runs = np.repeat(rng.randint(0, 256, 400), rng.randint(1, 20, 400)).astype(np.uint8).tobytes()[:4000]
    assert len(runs) == 4000
    add("rle", _deflate(runs, 6, zlib.Z_RLE), dynamic=("==", 1), max_dist=("==", 1), overlapping=(">=", 10))
    add("huffman_only", _deflate(runs, 6, zlib.Z_HUFFMAN_ONLY), dynamic=("==", 1), matches=("==", 0), literals=("==", 4000))
    add("dynamic_blocks_deep_window", _deflate(rng.randint(0, 8, 300000).astype(np.uint8).tobytes()), dynamic=(">=", 2),
        max_dist=(">=", 32000), cross_block=(">=", 100))
    y, x, c = np.mgrid[0:64, 0:96, 0:10]
    field = 128 + 60 * np.sin(x / 17.0 + c) * np.cos(y / 11.0 - 0.3 * c) + rng.randint(-1, 2, x.shape)
    flow = np.clip(field, 0, 255).astype(np.uint8).tobytes()
    add("flow_like", _deflate(flow), dynamic=(">=", 2), max_dist=(">=", 30000), cross_block=(">=", 10))
    add("flow_like_sync_flush", _deflate(flow, flush_at=20000, flush=zlib.Z_SYNC_FLUSH), dynamic=(">=", 2),
        empty_stored=("==", 1), cross_block=(">=", 10))
    add("flow_like_full_flush", _deflate(flow, flush_at=20000, flush=zlib.Z_FULL_FLUSH), dynamic=(">=", 2),
        empty_stored=("==", 1))
    add("empty", _deflate(b""), fixed=("==", 1), literals=("==", 0))
    # distances zlib never emits (its window is 32 768 minus the look-ahead) and exact corner pairs
    w = Writer()
    w.bits(0, 1)
    w.bits(1, 2)
    for v in rng.randint(0, 256, 32768):
        w.fixed_sym(int(v))
    w.fixed_sym(256)
    w.bits(1, 1)
    w.bits(1, 2)
    for length, dist in ((258, 32768), (3, 32768), (258, 1), (200, 7)):
        w.fixed_match(length, dist)
    w.fixed_sym(256)
    add("hand_far_distances", w.done(), fixed=("==", 2), max_dist=("==", 32768), max_len=("==", 258), matches=("==", 4),
        cross_block=("==", 2), overlapping=("==", 2))
    # zlib sends the two sets of lengths separately; the format makes them one sequence.  Literal lengths: 97, 254, 255 and
    # 256 have 2 bits; distance lengths 2, 2, 1.  The repeat of length 2 starts at symbol 255 and ends at distance 1.
    w = Writer()
    _dynamic_header(w, {1: 2, 2: 2, 16: 2, 18: 2}, nl=257, nd=3)      # canonical: 1 = 00, 2 = 01, 16 = 10, 18 = 11
    w.code(3, 2)
    w.bits(97 - 11, 7)                # symbols 0 .. 96: zeros
    w.code(1, 2)                      # 97: length 2
    w.code(3, 2)
    w.bits(138 - 11, 7)               # 98 .. 235
    w.code(3, 2)
    w.bits(18 - 11, 7)                # 236 .. 253
    w.code(1, 2)                      # 254: length 2
    w.code(2, 2)
    w.bits(4 - 3, 2)                  # repeat it 4 times: 255, 256, distance 0, distance 1
    w.code(0, 2)                      # distance 2: length 1
    for code in (0, 1, 2, 3):         # canonical: 97 = 00, 254 = 01, 255 = 10, end of block = 11
        w.code(code, 2)
    add("hand_repeat_into_distances", w.done(), dynamic=("==", 1), repeat_into_dist=("==", 1), literals=("==", 3))
    # a whole flow pickle member as np.savez_compressed writes it: the 128-byte .npy header, then (40, 56, 4) uint8
    y, x, c = np.mgrid[0:40, 0:56, 0:4]
    pickle = (120 + 50 * np.sin(x / 9.0 + c) * np.cos(y / 7.0) + rng.randint(-1, 2, x.shape)).astype(np.uint8)
    member = io.BytesIO()
    np.lib.format.write_array(member, pickle, version=(1, 0))
    assert len(member.getvalue()) == 128 + 40 * 56 * 4
    add("pickle_40x56x4", _deflate(member.getvalue()), dynamic=(">=", 1), matches=(">=", 10))
    return cases, want


def bad_cases():
    """streams zlib refuses, one per refusal of the decoder that a stream can carry by itself"""
    bad = {}
    bad["bad_block_type"] = bytes([0x07])
    bad["bad_stored_len"] = bytes([0x01, 0x05, 0x00, 0x00, 0x00]) + b"hello"
    w = Writer()                      # the code-length code itself: four codes of length 1
    _dynamic_header(w, {16: 1, 17: 1, 18: 1, 0: 1})
    w.bits(0, 32)
    bad["bad_oversubscribed_code_lengths"] = w.done()
    w = Writer()                      # the code-length code itself: one code of length 1 (incomplete)
    _dynamic_header(w, {0: 1})
    w.bits(0, 32)
    bad["bad_incomplete_code_lengths"] = w.done()
    w = Writer()                      # 258 literal/length + distance codes of length 1
    _dynamic_header(w, {1: 1, 18: 1})         # canonical: symbol 1 = code 0, symbol 18 = code 1
    for _ in range(258):
        w.code(0, 1)
    w.bits(0, 32)
    bad["bad_oversubscribed_literals"] = w.done()
    w = Writer()                      # two literal/length codes of length 2: incomplete, more than a single code
    _dynamic_header(w, {0: 2, 2: 2, 18: 1})   # canonical: 18 = 0, 0 = 10, 2 = 11
    w.code(3, 2)                      # symbol 0: length 2
    w.code(0, 1)
    w.bits(138 - 11, 7)               # 138 zeros: symbols 1 .. 138
    w.code(0, 1)
    w.bits(117 - 11, 7)               # 117 zeros: symbols 139 .. 255
    w.code(3, 2)                      # symbol 256: length 2
    w.code(2, 2)                      # the distance code: length 0
    w.bits(0, 32)
    bad["bad_incomplete_literals"] = w.done()
    w = Writer()                      # repeat the previous length, with nothing before it
    _dynamic_header(w, {1: 1, 16: 1})
    w.code(1, 1)
    w.bits(0, 2)
    w.bits(0, 32)
    bad["bad_repeat_without_previous"] = w.done()
    w = Writer()                      # a repeat that runs past HLIT + HDIST
    _dynamic_header(w, {1: 1, 18: 1})
    w.code(1, 1)
    w.bits(127, 7)
    w.code(1, 1)
    w.bits(127, 7)
    w.bits(0, 32)
    bad["bad_repeat_past_the_end"] = w.done()
    w = Writer()
    w.bits(1, 1)
    w.bits(1, 2)
    w.fixed_sym(286)
    w.bits(0, 16)
    bad["bad_literal_length_symbol_286"] = w.done()
    w = Writer()
    w.bits(1, 1)
    w.bits(1, 2)
    w.fixed_sym(65)
    w.fixed_sym(257)
    w.code(30, 5)
    w.bits(0, 16)
    bad["bad_distance_symbol_30"] = w.done()
    w = Writer()                      # all 258 lengths zero: no end-of-block code
    _dynamic_header(w, {1: 1, 18: 1})
    w.code(1, 1)
    w.bits(138 - 11, 7)
    w.code(1, 1)
    w.bits(120 - 11, 7)
    w.bits(0, 32)
    bad["bad_no_end_of_block"] = w.done()
    w = Writer()                      # literal A, then a match (3, 2): one byte further back than there is
    w.bits(1, 1)
    w.bits(1, 2)
    w.fixed_sym(65)
    w.fixed_match(3, 2)
    w.fixed_sym(256)
    bad["bad_distance_too_far_back"] = w.done()
    return bad


def build():
    cases, want = good_cases()
    structure = {}
    for name, stream in cases.items():
        expect = zlib.decompress(stream, -15)
        got, st = walk(stream)
        assert got == expect, name
        for key, (op, value) in want[name].items():
            assert (st[key] == value) if op == "==" else (st[key] >= value), (name, key, st[key], op, value)
        structure[name] = dict(st, stream_bytes=len(stream), output_bytes=len(expect))
        print(name, structure[name])
    assert any(s["repeat_into_dist"] for s in structure.values()), "no repeat runs from the literal lengths into the distances"
    far = cases["hand_far_distances"]
    assert len(zlib.decompress(far, -15)) == 32768 + 258 + 3 + 258 + 200
    bad = bad_cases()
    for name, stream in bad.items():
        try:
            zlib.decompress(stream, -15)
        except zlib.error as e:
            structure[name] = dict(zlib=str(e), stream_bytes=len(stream))
            print(name, e)
        else:
            raise AssertionError(name + ": zlib accepts it")
    assert "too far back" in structure["bad_distance_too_far_back"]["zlib"]
    cases.update(bad)
    return cases, structure


def main():
    cases, structure = build()
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        os.makedirs(sys.argv[2], exist_ok=True)
        for name, stream in cases.items():
            with open(os.path.join(sys.argv[2], name + ".deflate"), "wb") as f:
                f.write(stream)
            if not name.startswith("bad_"):
                with open(os.path.join(sys.argv[2], name + ".out"), "wb") as f:
                    f.write(zlib.decompress(stream, -15))
        return
    arrays = {k: np.frombuffer(v, np.uint8) for k, v in cases.items()}
    arrays["structure"] = np.frombuffer(json.dumps(structure, sort_keys=True).encode(), np.uint8)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
