"""Shared cases of the Snap format (tests/golden/snap_vectors.json), run by test_snap_golden.py (the generator),
test_emu_snap.py (the product sources on the CPU emulator) and test_gpu_snap.py (the HIP library).

The decoder below is written from the framing format's description (stream identifier, chunk types 0x00 / 0x01,
24-bit lengths, masked CRC-32C) and the raw Snappy format (varint length, literal and copy elements); it shares
nothing with the product or with the generator's encoder."""
import hashlib
import importlib.util
import json
import os
import struct

import numpy as np

from gzp_amd import _native, par

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "snap_vectors.json")
IDENT = bytes.fromhex("ff060000734e61507059")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def generator():
    """tests/golden/make_snap_golden.py as a module (make_input, snappy_raw, frame_stream, load_snappy)."""
    spec = importlib.util.spec_from_file_location("make_snap_golden", os.path.join(HERE, "golden", "make_snap_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


# ---------------------------------------------------------------- decoder
def _crc32c(b):
    c = 0xFFFFFFFF
    for x in b:
        c ^= x
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
    return c ^ 0xFFFFFFFF


def _crc32c_np(b):
    """The same, over a numpy table (long chunks)."""
    t = _CRC_T
    c = 0xFFFFFFFF
    for x in bytes(b):
        c = int(t[(c ^ x) & 0xFF]) ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def _table():
    t = np.zeros(256, dtype=np.uint64)
    for i in range(256):
        r = i
        for _ in range(8):
            r = (r >> 1) ^ (0x82F63B78 if r & 1 else 0)
        t[i] = r
    return t


_CRC_T = _table()


def crc32c(b):
    return _crc32c_np(b)


def unmask(m):
    r = (m - 0xA282EAD8) & 0xFFFFFFFF
    return ((r >> 17) | (r << 15)) & 0xFFFFFFFF


def raw_decode(b):
    """A raw Snappy buffer -> its bytes."""
    pos, n, shift = 0, 0, 0
    while True:
        x = b[pos]
        pos += 1
        n |= (x & 0x7F) << shift
        shift += 7
        if x < 0x80:
            break
    out = bytearray()
    while pos < len(b):
        tag = b[pos]
        pos += 1
        t = tag & 3
        if t == 0:
            m = tag >> 2
            if m >= 60:
                k = m - 59
                m = int.from_bytes(b[pos:pos + k], "little")
                pos += k
            out += b[pos:pos + m + 1]
            pos += m + 1
            continue
        if t == 1:
            ln = 4 + ((tag >> 2) & 7)
            o = ((tag >> 5) << 8) | b[pos]
            pos += 1
        elif t == 2:
            ln = 1 + (tag >> 2)
            o = int.from_bytes(b[pos:pos + 2], "little")
            pos += 2
        else:
            ln = 1 + (tag >> 2)
            o = int.from_bytes(b[pos:pos + 4], "little")
            pos += 4
        assert 0 < o <= len(out), "copy offset %d before the start" % o
        start = len(out) - o
        if o >= ln:
            out += out[start:start + ln]
        else:
            for i in range(ln):
                out.append(out[start + i])
    assert len(out) == n, (len(out), n)
    return bytes(out)


def decode_frames(s, check_crc=True):
    """A Snappy frame stream (any number of stream identifiers) -> (bytes, number of chunks)."""
    s = bytes(s)
    pos, out, chunks = 0, bytearray(), 0
    while pos < len(s):
        t = s[pos]
        ln = int.from_bytes(s[pos + 1:pos + 4], "little")
        body = s[pos + 4:pos + 4 + ln]
        assert len(body) == ln, "truncated chunk"
        pos += 4 + ln
        if t == 0xFF:
            assert s[pos - 4 - ln:pos] == IDENT
            continue
        assert t in (0, 1), "chunk type %#x" % t
        crc = struct.unpack("<I", body[:4])[0]
        data = raw_decode(body[4:]) if t == 0 else body[4:]
        assert len(data) <= 65536
        if check_crc:
            assert unmask(crc) == crc32c(data), "CRC-32C of chunk %d" % chunks
        out += data
        chunks += 1
    return bytes(out), chunks


# ---------------------------------------------------------------- the product
def check_digest(got, want, what):
    assert len(got) == want["size"], "%s: %d bytes, want %d" % (what, len(got), want["size"])
    if "hex" in want:
        assert got.hex() == want["hex"], what
    assert sha(got) == want["sha256"], what


def raw_body_matches(framed, chunk, want, what):
    """A one-chunk buffer's frame against a raw vector: the body where it is compressed, the stored decision where
    it is not."""
    n = len(chunk)
    if n == 0:
        assert framed == b"", what
        return
    assert framed[:10] == IDENT, what
    t = framed[10]
    body = framed[18:]
    assert int.from_bytes(framed[11:14], "little") == len(body) + 4, what
    assert unmask(struct.unpack("<I", framed[14:18])[0]) == crc32c(chunk), what
    if want["size"] >= n - n // 8:
        assert t == 1 and body == bytes(chunk), what + ": stored"
    else:
        assert t == 0, what + ": compressed"
        check_digest(body, want, what)


def run_raw(lib, vectors, gen, modes=("host", "encode"), max_slab=65536):
    with _native.Context(format=_native.FORMAT_SNAP, buffer_size=65536, lib=lib, max_slab_bytes=max_slab) as c:
        for v in vectors:
            a = gen.make_input(v["spec"])[:65536]
            for mode in modes:
                got = c.compress_slab(a, True) if mode == "host" else c.encode_block(a, False)
                raw_body_matches(got, a.tobytes(), v, "%s %s" % (mode, v["spec"]))


def run_framed(lib, vectors, gen, slab_modes=(_native.SLAB_LAST, _native.SLAB_FLUSH)):
    """Every framed vector through gzpx_compress_slab (LAST and FLUSH: the same bytes; FULL_BLOCKS where the stream is
    a whole number of buffers, followed by an empty final piece), block sizes summing to the stream."""
    by_bs = {}
    for v in vectors:
        by_bs.setdefault(v["spec"][3], []).append(v)
    for bs, vs in sorted(by_bs.items()):
        big = max(v["spec"][1] for v in vs)
        with _native.Context(format=_native.FORMAT_SNAP, buffer_size=bs, lib=lib, max_slab_bytes=max(big, 1)) as c:
            for v in vs:
                a = gen.make_input(v["spec"][:3])
                what = "bs %d %s" % (bs, v["spec"])
                for mode in slab_modes:
                    got, sizes = c.compress_slab(a, mode, return_block_sizes=True)
                    check_digest(got, v, what)
                    assert int(sizes.sum()) == len(got), what
                    assert len(sizes) == c.n_blocks(a.size), what
                if a.size and a.size % bs == 0:
                    got = c.compress_slab(a, _native.SLAB_FULL_BLOCKS)
                    check_digest(got, v, what + " FULL_BLOCKS")


def run_encode_block(lib, vectors, gen):
    """FormatSpec::encode buffer by buffer (is_last ignored) concatenated = the framed vector."""
    by_bs = {}
    for v in vectors:
        by_bs.setdefault(v["spec"][3], []).append(v)
    for bs, vs in sorted(by_bs.items()):
        with _native.Context(format=_native.FORMAT_SNAP, buffer_size=bs, lib=lib, max_slab_bytes=bs) as c:
            for v in vs:
                a = gen.make_input(v["spec"][:3])
                pieces = [a[i:i + bs] for i in range(0, a.size, bs)]
                if a.size % bs == 0:
                    pieces.append(a[:0])
                out = b"".join(c.encode_block(p, k % 2 == 0) for k, p in enumerate(pieces))
                check_digest(out, v, "encode_block bs %d %s" % (bs, v["spec"]))


class _Sink:
    def __init__(self):
        self.parts = []

    def write(self, b):
        self.parts.append(bytes(b))

    def value(self):
        return b"".join(self.parts)


def run_twin(lib, vectors, gen, seed=5, batch_blocks=3):
    """ParCompressBuilder(par.Snap): ragged write sizes, a flush in the middle (the buffer so far goes out short: it is
    compared with the framing of those pieces), finish.  Without the flush the stream is the framed vector."""
    rng = np.random.default_rng(seed)
    for v in vectors:
        bs = v["spec"][3]
        a = gen.make_input(v["spec"][:3]).tobytes()
        sink = _Sink()
        w = par.ParCompressBuilder(par.Snap, lib=lib).buffer_size(bs).num_threads(2).batch_blocks(batch_blocks) \
            .compression_level(par.Compression(99)).from_writer(sink)
        pos = 0
        while pos < len(a):
            k = int(rng.integers(1, max(2, 3 * bs // 2)))
            w.write(a[pos:pos + k])
            pos += k
        w.finish()
        check_digest(sink.value(), v, "twin %s" % v["spec"])


def run_twin_flush(lib, gen, raw, cases, seed=7):
    """flush() sends the buffer it holds, short (src/par/compress.rs flush -> flush_last(false)); the stream is the
    concatenation of the framing of the pieces as they were cut."""
    rng = np.random.default_rng(seed)
    for cls, n, s, bs in cases:
        a = gen.make_input([cls, n, s]).tobytes()
        sink = _Sink()
        w = par.ParCompressBuilder(par.Snap, lib=lib).buffer_size(bs).num_threads(1).batch_blocks(2).from_writer(sink)
        cut = int(rng.integers(1, n))
        w.write(a[:cut])
        w.flush()
        w.write(a[cut:])
        w.finish()
        want = b"".join(gen.frame_buffer(a[i:min(i + bs, cut)], raw) for i in range(0, cut, bs))
        rest = a[cut:]
        want += gen.frame_stream(rest, bs, raw) if rest else b""
        got = sink.value()
        assert decode_frames(got)[0] == a
        assert got == want, (cls, n, bs, cut)
