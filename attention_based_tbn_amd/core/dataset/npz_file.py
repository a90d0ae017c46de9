"""Flow pickles on the device: the `flow` member of the reference's frame_XXXXXXXXXX.npz stacks
(preprocessing/create_epic_flow_pickle.py: np.savez_compressed(out_file, flow=img); read by np.load in
core/dataset/dataset.py:336-352).

The host keeps what is small and irregular -- the zip directory and the 128-byte .npy header (`npz_member`); the
device does what is large: `load_npz_arrays` packs the members' compressed bytes of a whole batch into one pinned buffer,
copies it once, and `tbn_inflate_batch` (csrc/inflate.hip) inflates every member and checks its CRC-32 in one call.  One
small copy back of the status vector is the only synchronisation.  A member the record or the status sends to the host
(anything np.load reads that this path does not: another dtype, Fortran order, a damaged stream, ...) is read by the
host code into its slot, so a batch may mix both and error wording stays the host path's; those members are counted.

Writing is the mirror image (`save_npz_arrays`, `write_npz_files`; the np.savez_compressed call of
preprocessing/create_epic_flow_pickle.py:203): the device lays out header and array per member, `tbn_deflate_batch`
(csrc/deflate.hip) compresses all of them and computes their CRC-32 in one call, and the host writes the zip container
around each stream (`npy_header`, `npz_container`).

The streams this project writes are chunks of 32 KB compressed independently and joined on byte boundaries
(csrc/tbn_deflate.h).  With `chunk_index=True` the writer records where each chunk's bytes end, as a zip extra field of
the member's CENTRAL-DIRECTORY entry (header ID 0x4354; np.load and zipfile skip it, the local header and the stream are
the same bytes as without it), and `load_npz_arrays` inflates such a member with one wavefront per chunk
(`tbn_inflate_chunks`) instead of one per member.  Files without the field, np.savez_compressed's among them, take the
whole-member path; the CRC-32 of the whole member is checked either way, so a wrong index costs a status (and the host
path for that member), never wrong bytes."""
import ast
import ctypes
import io
import os
import struct
import zipfile
import zlib
from collections import namedtuple

import numpy as np
import torch

from ..._lib import InflateChunk, InflateMember, TbnHipError, call, ptr, stream_ptr

NpzMember = namedtuple("NpzMember", "method data_offset data_length size crc header_length shape host reason")
NpzMember.__doc__ = """What `npz_member` reports: `method` 0 (stored) or 8 (deflate); the member's compressed bytes are
blob[data_offset : data_offset + data_length]; `size`: its inflated size (the .npy header and the array); `crc`: the
directory's CRC-32; `header_length`: bytes of the .npy header in front of the array; `shape`: (H, W, C).  `host` True:
the member takes the host path (np.load), `reason` says why and the other fields are None where they are unknown."""

STATUS_SKIPPED = 11        # include/tbn_hip.h: the row carried the skip marker
_ALIGN = 16
_PREFIX = 4096             # inflated bytes looked at for the .npy header
_counts = {"members": 0, "fallbacks": 0, "chunked": 0}
CHUNK_INDEX_ID = 0x4354    # the zip extra field that holds a member's chunk index
CHUNK_INDEX_VERSION = 1


def fallback_count():
    """members `load_npz_arrays` has sent through the host path so far (of `member_count()` in all)"""
    return _counts["fallbacks"]


def member_count():
    return _counts["members"]


def chunked_count():
    """members `load_npz_arrays` has inflated chunk by chunk so far (their chunk index held: status 0)"""
    return _counts["chunked"]


def _chunk_bytes():
    from ..._lib import lib
    return int(lib().tbn_deflate_chunk())


def npz_chunk_index(blob, name="flow"):
    """The chunk index of member `name` (.npy is appended) of the .npz file `blob`: the list of compressed end offsets
    of its chunks inside the member's stream, or None.  None unless the central-directory entry carries extra field
    0x4354 with version 1, the chunk size of this library (`tbn_deflate_chunk()`), method 8,
    n_chunks == max(1, ceil(size / chunk)), strictly increasing ends and a last end equal to compress_size.  A malformed
    field -- or file -- is no error here: it means "no index" (`npz_member` is the one that judges the file)."""
    try:
        end = blob.rfind(b"PK\x05\x06")
        if end < 0 or end + 22 > len(blob):
            return None
        entries, cd_size, at = struct.unpack_from("<HII", blob, end + 10)
        stop = at + cd_size
        fname = (name + ".npy").encode("ascii")
        for _ in range(entries):
            if at + 46 > stop or stop > end or blob[at:at + 4] != b"PK\x01\x02":
                return None
            method, = struct.unpack_from("<H", blob, at + 10)
            csize, size, name_len, extra_len, comment_len = struct.unpack_from("<IIHHH", blob, at + 20)
            if at + 46 + name_len + extra_len + comment_len > stop:
                return None
            if blob[at + 46:at + 46 + name_len] == fname:
                break
            at += 46 + name_len + extra_len + comment_len
        else:
            return None
        extra = memoryview(blob)[at + 46 + name_len:at + 46 + name_len + extra_len]
        pos = 0
        while pos + 4 <= len(extra):
            fid, flen = struct.unpack_from("<HH", extra, pos)
            if fid == CHUNK_INDEX_ID:
                break
            pos += 4 + flen
        else:
            return None
        if flen < 12 or pos + 4 + flen > len(extra):
            return None
        version, reserved, chunk, n_chunks = struct.unpack_from("<HHII", extra, pos + 4)
        if version != CHUNK_INDEX_VERSION or method != zipfile.ZIP_DEFLATED or chunk != _chunk_bytes():
            return None
        if n_chunks != max(1, -(-size // chunk)) or flen != 12 + 4 * n_chunks:
            return None
        ends = np.frombuffer(extra, "<u4", n_chunks, pos + 16)
        if int(ends[-1]) != csize or int(ends[0]) == 0 or (n_chunks > 1 and not (ends[1:] > ends[:-1]).all()):
            return None
        return ends.tolist()
    except (struct.error, ValueError, UnicodeEncodeError):
        return None


def _host(reason, **known):
    fields = dict(method=None, data_offset=None, data_length=None, size=None, crc=None, header_length=None, shape=None)
    fields.update(known)
    return NpzMember(host=True, reason=reason, **fields)


def npz_member(blob, name="flow"):
    """The record of member `name` (.npy is appended) of the .npz file `blob` (bytes).  Touches no GPU and inflates at
    most the first 4096 bytes.  Sizes, method, CRC and the local header's offset come from the zip CENTRAL DIRECTORY: the
    local header holds 0xFFFFFFFF or zeros there when the writer used zip64 extras (numpy >= 2.2 writes a 20-byte one in
    every local header) or a data descriptor (a non-seekable stream); only its name and extra lengths are read.
    Raises `zipfile.BadZipFile` on bytes that are not a zip file (or one cut short); everything else np.load might
    still read, and everything it would refuse with its own message, comes back with `host=True`."""
    zf = zipfile.ZipFile(io.BytesIO(blob))
    try:
        info = zf.getinfo(name + ".npy")
    except KeyError:
        return _host(f"no member {name}.npy")
    known = dict(method=info.compress_type, size=info.file_size, crc=info.CRC, data_length=info.compress_size)
    if info.flag_bits & 0x1:
        return _host("the member is encrypted", **known)
    if info.compress_type not in (zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED):
        return _host(f"compression method {info.compress_type}", **known)
    if info.file_size >= 1 << 31 or info.compress_size >= 1 << 31:
        return _host("a member of 2 GiB or more", **known)
    at = info.header_offset
    if at + 30 > len(blob) or blob[at:at + 4] != b"PK\x03\x04":
        raise zipfile.BadZipFile(f"no local file header at offset {at}")
    name_len, extra_len = struct.unpack_from("<HH", blob, at + 26)
    start = at + 30 + name_len + extra_len
    if start + info.compress_size > len(blob):
        raise zipfile.BadZipFile("the member's data runs past the end of the file")
    known["data_offset"] = start
    data = memoryview(blob)[start:start + info.compress_size]
    if info.compress_type == zipfile.ZIP_DEFLATED:
        try:
            head = zlib.decompressobj(-15).decompress(data, _PREFIX)
        except zlib.error as e:
            return _host(f"the .npy header does not inflate: {e}", **known)
    else:
        head = bytes(data[:_PREFIX])
    if len(head) < 10 or head[:6] != b"\x93NUMPY":
        return _host("no .npy magic", **known)
    if (head[6], head[7]) != (1, 0):
        return _host(f".npy header version {head[6]}.{head[7]}", **known)
    header_length = 10 + struct.unpack_from("<H", head, 8)[0]
    if header_length > len(head):
        return _host("the .npy header is cut short", **known)
    try:
        fields = ast.literal_eval(head[10:header_length].decode("latin1"))
        descr, fortran, shape = fields["descr"], fields["fortran_order"], tuple(fields["shape"])
    except Exception as e:
        return _host(f"the .npy header does not parse: {e}", **known)
    known["header_length"] = header_length
    if descr not in ("|u1", "u1"):
        return _host(f"dtype {descr!r}", **known)
    if fortran:
        return _host("Fortran order", **known)
    if len(shape) != 3 or not all(isinstance(v, int) and v >= 0 for v in shape):
        return _host(f"shape {shape}", **known)
    known["shape"] = shape
    if info.file_size != header_length + shape[0] * shape[1] * shape[2]:
        return _host("the member's size is not its header plus H * W * C", **known)
    return NpzMember(host=False, reason=None, **known)


def read_npz_host(blob, name="flow"):
    """the host path of one member: np.load, with np.load's exceptions"""
    with np.load(io.BytesIO(blob)) as z:
        return np.asarray(z[name])


def load_npz_arrays(blobs, name="flow", device="cuda", *, records=None, planes=False, host_read=None, chunked="auto"):
    """Member `name` of every .npz file in `blobs` (bytes each), all of ONE shape (H, W, C) uint8, inflated on `device`
    by one `tbn_inflate_batch` call on the current stream -> (tensor, statuses).

    chunked    "auto": a member whose file carries a chunk index (`npz_chunk_index`) is inflated one wavefront per chunk
               by the call's one `tbn_inflate_chunks`; the others go through `tbn_inflate_batch` as before.  Still one
               pinned upload (compressed bytes and every table) and one small copy back.  False: every member takes the
               whole-member path (the A/B arm; what a library without the chunk reader does with the same files).

    tensor     uint8 (n, H, W, C) in stream layout (a view into the staging buffer), or with `planes=True` the
               de-interleaved (n * C, H, W, 1) the dataset wants (image c of file i is channel c of its array): one
               permute(...).contiguous() pass on the device.
    statuses   per member, 0: inflated and CRC-checked on the device; otherwise the status of tbn_inflate_batch or
               tbn_inflate_chunks (include/tbn_hip.h; 11: the record said "host") -- that member was read by `host_read(i)` (default: np.load of
               blobs[i]; returns uint8 (H, W, C)) into its slot, and counted (`fallback_count()`).  What the host path
               raises for it propagates.
    records    the `npz_member` records when the caller has them already."""
    n = len(blobs)
    if n == 0:
        raise ValueError("load_npz_arrays: no files")
    if chunked not in ("auto", False):
        raise ValueError(f"load_npz_arrays: chunked={chunked!r}, expected 'auto' or False")
    device = torch.device(device)
    if device.type != "cuda":
        raise TbnHipError(f"load_npz_arrays: device {device} is not a GPU; there is no host version of this path "
                          "(np.load is the host path)")
    if records is None:
        records = [npz_member(b, name) for b in blobs]
    if host_read is None:
        def host_read(i):
            return read_npz_host(blobs[i], name)
    # the host members first: the shape may have to come from them, and what they raise should come before any launch
    host_arrays = {}
    for i, r in enumerate(records):
        if r.host:
            arr = np.asarray(host_read(i))
            if arr.dtype != np.uint8 or arr.ndim != 3:
                raise TbnHipError(f"load_npz_arrays: file {i}: {name!r} is {arr.dtype} {arr.shape}, expected uint8 (H, W, C)")
            host_arrays[i] = arr
    shapes = set(tuple(host_arrays[i].shape) if r.host else r.shape for i, r in enumerate(records))
    if len(shapes) != 1:
        raise TbnHipError(f"load_npz_arrays: the files of one call must share a shape, got {sorted(shapes)}")
    H, W, Cn = shapes.pop()
    payload = H * W * Cn
    dev_rows = [r for r in records if not r.host]
    header = dev_rows[0].header_length if dev_rows else 0
    if any(r.header_length != header for r in dev_rows):
        header = None                       # headers of several lengths: the arrays are gathered one by one below
    slot = -(-(max([r.size for r in dev_rows] + [payload])) // _ALIGN) * _ALIGN

    # which members carry a chunk index: they are inflated chunk by chunk, the others whole
    indexes = {}
    if chunked == "auto":
        for i, r in enumerate(records):
            if not r.host and r.method == zipfile.ZIP_DEFLATED:
                ends = npz_chunk_index(blobs[i], name)
                if ends is not None:
                    indexes[i] = ends
    whole = any(not r.host and i not in indexes for i, r in enumerate(records)) or not indexes

    table = (InflateMember * n)()
    total = 0
    for i, r in enumerate(records):
        row = table[i]
        row.out_off, row.skip = i * slot, int(r.host or i in indexes)
        if not r.host:
            row.in_off, row.in_len, row.out_len, row.crc, row.method = total, r.data_length, r.size, r.crc, r.method
            total += -(-r.data_length // _ALIGN) * _ALIGN
    in_bytes = max(total, _ALIGN)
    parts = [np.frombuffer(table, np.uint8)]                # behind the compressed bytes: every table, 8-byte aligned
    n_chunks = 0
    if indexes:
        # the chunk reader's tables: the member table again with the OTHER rows skipped, the chunk rows, chunk_begin
        ctable = (InflateMember * n)()
        ctypes.memmove(ctable, table, ctypes.sizeof(table))
        chunk = _chunk_bytes()
        begin = np.zeros(n + 2, np.uint32)                  # n + 1 entries and 4 bytes of padding
        for i in range(n):
            ctable[i].skip = int(i not in indexes)
            begin[i + 1] = begin[i] + len(indexes.get(i, ()))
        n_chunks = int(begin[n])
        crows = (InflateChunk * n_chunks)()
        for i, ends in indexes.items():
            m, first, prev = ctable[i], int(begin[i]), 0
            for k, end in enumerate(ends):
                row = crows[first + k]
                row.in_off, row.in_len, row.out_off = m.in_off + prev, end - prev, m.out_off + k * chunk
                row.out_len, row.member, row.last = min(chunk, m.out_len - k * chunk), i, int(k + 1 == len(ends))
                prev = end
        parts += [np.frombuffer(ctable, np.uint8), np.frombuffer(crows, np.uint8), begin.view(np.uint8)]
    offsets = np.cumsum([in_bytes] + [p.size for p in parts])
    staging = torch.empty(int(offsets[-1]), dtype=torch.uint8, pin_memory=True)         # ONE pinned buffer, ONE copy
    flat = staging.numpy()
    for i, r in enumerate(records):
        if not r.host:
            at = table[i].in_off
            flat[at:at + r.data_length] = np.frombuffer(blobs[i], np.uint8, r.data_length, r.data_offset)
    for at, p in zip(offsets, parts):
        flat[at:at + p.size] = p
    dev = staging.to(device, non_blocking=True)
    out = torch.empty(n * slot, dtype=torch.uint8, device=device)
    # status[n], info[n] of the whole-member call; then status[n], info[n], chunk_status[2 * n_chunks] of the chunk reader
    status = torch.empty(4 * n + 2 * n_chunks, dtype=torch.int32, device=device)
    base = ptr(dev)
    if whole:
        call("tbn_inflate_batch", base, in_bytes, base + int(offsets[0]), n, ptr(out), n * slot, ptr(status), ptr(status) + 4 * n,
             stream_ptr())
    if indexes:
        call("tbn_inflate_chunks", base, in_bytes, base + int(offsets[1]), n, base + int(offsets[2]), base + int(offsets[3]),
             n_chunks, ptr(out), n * slot, ptr(status) + 8 * n, ptr(status) + 12 * n, ptr(status) + 16 * n, stream_ptr())
    rows = out.view(n, slot)
    if header is not None:
        arrays = rows[:, header:header + payload].view(n, H, W, Cn)
    else:
        arrays = torch.stack([rows[i, (r.header_length or 0):(r.header_length or 0) + payload] for i, r in enumerate(records)]
                             ).view(n, H, W, Cn)
    both = status[:3 * n].tolist()                                          # one small copy back: the only synchronisation
    statuses = [both[2 * n + i] if i in indexes else both[i] if whole else STATUS_SKIPPED for i in range(n)]
    _counts["members"] += n
    _counts["chunked"] += sum(1 for i in indexes if statuses[i] == 0)
    for i, s in enumerate(statuses):
        if s != 0:
            arr = host_arrays[i] if i in host_arrays else np.asarray(host_read(i))
            if arr.dtype != np.uint8 or tuple(arr.shape) != (H, W, Cn):
                raise TbnHipError(f"load_npz_arrays: file {i}: {name!r} is {arr.dtype} {arr.shape}, expected uint8 {(H, W, Cn)}")
            arrays[i].copy_(torch.from_numpy(np.ascontiguousarray(arr)), non_blocking=False)
            _counts["fallbacks"] += 1
    if planes:
        arrays = arrays.permute(0, 3, 1, 2).contiguous().view(n * Cn, H, W, 1)
    return arrays, statuses


# ---- writing: the other half of a flow pickle's life (reference preprocessing/create_epic_flow_pickle.py:203) ------------
STATUS_DEFLATE_SKIPPED = 3     # include/tbn_hip.h, tbn_deflate_batch: the row carried the skip marker
_ZIP_DATE, _ZIP_TIME = (0 << 9) | (1 << 5) | 1, 0       # 1980-01-01 00:00:00: the files depend on their content alone


def npy_header(shape):
    """The exact bytes np.save writes in front of a C-order uint8 array of `shape`: format version 1.0, the dict
    padded with spaces (numpy's 21-digit room for a growing first axis, then up to a multiple of 64) and a newline."""
    shape = tuple(int(v) for v in shape)
    text = "{'descr': '|u1', 'fortran_order': False, 'shape': %s, }" % repr(shape)
    if shape:
        text += " " * (21 - len(repr(shape[0])))
    used = 10 + len(text) + 1
    pad = 64 - used % 64
    body = text.encode("latin1") + b" " * pad + b"\n"
    if len(body) >= 1 << 16:
        raise ValueError(f"npy_header: shape {shape} does not fit a version 1.0 header")
    return b"\x93NUMPY\x01\x00" + struct.pack("<H", len(body)) + body


def npz_container(name, stream, crc, size, chunk_ends=None):
    """One complete .npz file (bytes) around ONE member `name`.npy whose raw deflate stream, CRC-32 and inflated size
    are given: local header, the stream, central directory, end record; method 8, a fixed timestamp, no zip64.

    `chunk_ends` (the compressed end offset of every chunk of a stream written by tbn_deflate_batch_indexed; the last
    equals len(stream)) goes into the CENTRAL-DIRECTORY entry as extra field 0x4354, little endian: u16 ID, u16 data size
    12 + 4 n, u16 version 1, u16 reserved 0, u32 raw bytes per chunk, u32 n, u32 end[n].  Everything in front of the
    central directory is the same bytes as without it; an index too long for an extra field (65 535 bytes) is left out."""
    fname = (name + ".npy").encode("ascii")
    if size >= 1 << 31 or len(stream) >= 1 << 31:
        raise ValueError("npz_container: a member of 2 GiB or more needs zip64, which this writer does not do")
    fields = (20, 0, 8, _ZIP_TIME, _ZIP_DATE, crc & 0xFFFFFFFF, len(stream), size, len(fname), 0)
    local = struct.pack("<4sHHHHHIIIHH", b"PK\x03\x04", *fields) + fname
    extra = b""
    if chunk_ends is not None and 4 + 12 + 4 * len(chunk_ends) <= 0xFFFF:
        ends = np.asarray(chunk_ends, "<u4")
        extra = struct.pack("<HHHHII", CHUNK_INDEX_ID, 12 + 4 * ends.size, CHUNK_INDEX_VERSION, 0, _chunk_bytes(), ends.size)
        extra += ends.tobytes()
    cfields = fields[:-1] + (len(extra),)
    central = struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\x01\x02", 20, *cfields, 0, 0, 0, 0, 0) + fname + extra
    end = struct.pack("<4sHHHHIIH", b"PK\x05\x06", 0, 0, 1, 1, len(central), len(local) + len(stream), 0)
    return b"".join((local, bytes(stream), central, end))


def save_npz_arrays(arrays, name="flow", *, deflate="device", chunk_index=False):
    """`arrays`: uint8 (n, H, W, C) on the device -> n `bytes`, each a complete .npz file with the one member `name`
    (what np.savez_compressed(file, **{name: array}) holds; np.load and `load_npz_arrays` read it).

    deflate="device"  the .npy header and the array are laid out per slot on the device, ONE `tbn_deflate_batch` call on
                      the current stream compresses every member and computes its CRC-32 (csrc/deflate.hip), one small
                      copy brings lengths, CRCs and statuses back, one copy the streams, packed.  The host only writes
                      the zip container around each stream.
    deflate="host"    zlib level 6 on the host, in the same container: the A/B and fallback path.
    chunk_index=True  (deflate="device" only) `tbn_deflate_batch_indexed` also reports where every chunk of a stream
                      ends, and the files carry that chunk index (`npz_container`): `load_npz_arrays` then inflates
                      them one wavefront per chunk.  The streams are the same bytes; with False so are the files."""
    if deflate not in ("device", "host"):
        raise ValueError(f"save_npz_arrays: deflate={deflate!r}, expected 'device' or 'host'")
    if chunk_index and deflate == "host":
        raise ValueError("save_npz_arrays: chunk_index=True needs deflate='device': a zlib stream has no chunks")
    if not isinstance(arrays, torch.Tensor) or arrays.dtype != torch.uint8 or arrays.dim() != 4:
        raise TbnHipError("save_npz_arrays: expected a uint8 tensor (n, H, W, C)")
    n, H, W, Cn = arrays.shape
    if n == 0:
        return []
    header = npy_header((H, W, Cn))
    size = len(header) + H * W * Cn
    if size >= 1 << 31:
        raise ValueError(f"save_npz_arrays: a member of {size} bytes: 2 GiB or more is refused (no zip64)")
    if deflate == "host":
        out = []
        for a in arrays.contiguous().cpu().numpy():
            raw = header + a.tobytes()
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            out.append(npz_container(name, c.compress(raw) + c.flush(), zlib.crc32(raw), size))
        return out
    if arrays.device.type != "cuda":
        raise TbnHipError(f"save_npz_arrays: device {arrays.device} is not a GPU (deflate='host' is the host path)")
    from ..._lib import DeflateMember, lib
    L = lib()
    device = arrays.device
    stride = -(-size // _ALIGN) * _ALIGN
    cap = -(-int(L.tbn_deflate_bound(size)) // _ALIGN) * _ALIGN
    table = (DeflateMember * n)()
    for i in range(n):
        row = table[i]
        row.in_off, row.in_len, row.out_off, row.out_cap = i * stride, size, i * cap, cap
    workspace_bytes = int(L.tbn_deflate_workspace_bytes(ctypes.addressof(table), n))
    small = torch.empty(len(header) + ctypes.sizeof(table), dtype=torch.uint8, pin_memory=True)   # header + table: one copy
    flat = small.numpy()
    flat[:len(header)] = np.frombuffer(header, np.uint8)
    flat[len(header):] = np.frombuffer(table, np.uint8)
    small_dev = small.to(device, non_blocking=True)
    raw = torch.empty((n, stride), dtype=torch.uint8, device=device)
    raw[:, :len(header)] = small_dev[:len(header)]
    raw[:, len(header):size] = arrays.reshape(n, -1)
    table_dev = small_dev[len(header):].clone()               # its own allocation: 8-byte aligned
    out = torch.empty((n, cap), dtype=torch.uint8, device=device)
    meta = torch.empty(3 * n, dtype=torch.int32, device=device)            # out_len[n], crc[n], status[n]
    workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=device)
    args = (ptr(raw), n * stride, ptr(table_dev), n, ptr(out), n * cap, ptr(meta), ptr(meta) + 4 * n, ptr(meta) + 8 * n,
            ptr(workspace), stream_ptr())
    if chunk_index:
        per = max(1, -(-size // _chunk_bytes()))                            # chunks per member: all of one size
        meta = torch.empty((3 + per) * n, dtype=torch.int32, device=device)             # ..., then chunk_end[n * per]
        call("tbn_deflate_batch_indexed", *args[:6], ptr(meta), ptr(meta) + 4 * n, ptr(meta) + 8 * n, *args[9:],
             ptr(meta) + 12 * n)
    else:
        call("tbn_deflate_batch", *args)
    host = meta.cpu().numpy()                                               # the first synchronisation
    lengths, crcs, statuses = host[:n].view(np.uint32), host[n:2 * n].view(np.uint32), host[2 * n:3 * n]
    if statuses.any():
        raise TbnHipError(f"save_npz_arrays: tbn_deflate_batch statuses {statuses.tolist()}")
    index = host[3 * n:].view(np.uint32).reshape(n, -1) if chunk_index else [None] * n
    packed = torch.cat([out[i, :int(lengths[i])] for i in range(n)]).cpu().numpy()      # the streams: one copy
    ends = np.cumsum(lengths.astype(np.int64))
    return [npz_container(name, packed[int(e) - int(l):int(e)].tobytes(), int(c), size, chunk_ends=ix)
            for e, l, c, ix in zip(ends, lengths, crcs, index)]


def write_npz_files(paths, arrays, name="flow", *, deflate="device", chunk_index=False):
    """`save_npz_arrays`, then file i goes to paths[i]: written under a temporary name beside it and renamed, so a
    reader (or an interrupted run) never sees half a file.  -> bytes written per file."""
    if len(paths) != arrays.shape[0]:
        raise ValueError(f"write_npz_files: {len(paths)} paths for {arrays.shape[0]} arrays")
    sizes = []
    for path, blob in zip(paths, save_npz_arrays(arrays, name, deflate=deflate, chunk_index=chunk_index)):
        tmp = f"{path}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(blob)
        os.replace(tmp, path)
        sizes.append(len(blob))
    return sizes
