"""Generate tests/golden/snap_vectors.json -- the known-answer vectors of gzp's Snap format.

Run in the build container only (needs the snappy binary of the image, /opt/conda/lib/libsnappy.so.1.1.8):

    python tests/golden/make_snap_golden.py

gzp's Snap writer is snap::read::FrameEncoder over every buffer_size piece (src/snap.rs:38-83); the snap crate is
Rust and cannot be built here, so the raw Snappy bodies come from the C++ snappy 1.1.8 binary, which the crate ports.
The framing is restated below in plain Python, independently of the product:

  * a non-empty buffer: the stream identifier ff 06 00 00 "sNaPpY", then per 64 KiB chunk a 4-byte header (type,
    24-bit LE length = 4 + body), the masked CRC-32C of the uncompressed chunk (LE), the body: the raw encoding
    (type 0x00), or the chunk itself (type 0x01) when the encoding is >= n - n/8 bytes;
  * an empty buffer encodes to nothing (gzp sends one when the stream is empty or a multiple of buffer_size).

Inputs are regenerated from their spec (make_input); outputs are stored as SHA-256 + size (+ hex up to 1 KiB).
This module is also imported by the tests for make_input, the restated compressor (snappy_raw) and the framing.
"""
import hashlib
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from gzp_amd import synth  # noqa: E402

SNAPPY_SO = os.environ.get("SNAPPY_SO", "/opt/conda/lib/libsnappy.so.1.1.8")
OUT = os.path.join(HERE, "snap_vectors.json")
CHUNK = 65536
IDENT = bytes.fromhex("ff060000734e61507059")
FULL_N, FULL_SEED, FULL_BS = 576_716_800, 20250927, 131072  # bench.py's headline slab, gzp's default buffer


def load_snappy(path=SNAPPY_SO):
    """The binary's raw compressor, or None where the library is not on this machine."""
    import ctypes
    if not os.path.exists(path):
        return None
    L = ctypes.CDLL(path)
    L.snappy_compress.restype = ctypes.c_int
    L.snappy_compress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t)]

    def raw(b):
        b = bytes(b)
        cap = 32 + len(b) + len(b) // 6
        out = ctypes.create_string_buffer(cap)
        n = ctypes.c_size_t(cap)
        assert L.snappy_compress(b, len(b), out, ctypes.byref(n)) == 0
        return out.raw[:n.value]
    return raw


# ---------------------------------------------------------------- inputs
def make_input(spec):
    """spec = [kind, n, seed, *args]: a synth class, or one of the shapes that reach a given rule."""
    kind, n, seed = spec[0], spec[1], spec[2]
    if kind in synth.CLASSES:
        return synth.make(kind, n, seed)
    rnd = np.frombuffer(synth.splitmix64(seed, (n + 7) // 8 + 8).tobytes(), dtype=np.uint8)
    if kind == "period":  # runs of period p: overlapping copies
        p = spec[3]
        return np.resize(rnd[:p], n).astype(np.uint8)
    if kind == "echo":  # random bytes with a[d : d + l] = a[s : s + l]: one copy of offset d - s and length >= l
        s, d, l = spec[3], spec[4], spec[5]
        a = rnd[:n].copy()
        a[d:d + l] = a[s:s + l]
        return a
    if kind == "literal":  # a literal run of exactly m bytes, then a run of zeros
        m = spec[3]
        a = np.zeros(n, dtype=np.uint8)
        a[:m] = rnd[:m] | 1
        return a
    raise ValueError(kind)


def probe_offsets(count=400):
    offs, skip = [0], 32
    while len(offs) < count:
        offs.append(offs[-1] + (skip >> 5))
        skip += skip >> 5
    return offs


def echo_specs():
    """Copies at offsets around 2047 / 2048 and lengths around 11 / 12 in random data: the copy's source and
    destination are both probe positions of the first literal scan (1 + offs[i], 1 + offs[j]), so the scan finds it."""
    offs = probe_offsets()
    specs = []
    for want in (2046, 2047, 2048, 2049):
        pair = next((1 + offs[i], 1 + offs[j]) for i in range(8, 200) for j in range(i + 1, 300)
                    if offs[j] - offs[i] == want)
        for l in (4, 11, 12, 13, 64, 67, 68, 69, 131):
            specs.append(["echo", 16384, 100 + l, pair[0], pair[1], l])
    return specs


# ---------------------------------------------------------------- the restated compressor (snappy 1.1.8's loop)
def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _literal(s):
    m = len(s) - 1
    if m < 60:
        return bytes([m << 2]) + s
    k = (m.bit_length() + 7) // 8
    return bytes([(59 + k) << 2]) + m.to_bytes(k, "little") + s


def _copy64(o, l):
    if l < 12 and o < 2048:
        return bytes([1 | ((l - 4) << 2) | ((o >> 8) << 5), o & 0xFF])
    return bytes([2 | ((l - 1) << 2), o & 0xFF, o >> 8])


def _copy(o, l):
    out = b""
    while l >= 68:
        out += _copy64(o, 64)
        l -= 64
    if l > 64:
        out += _copy64(o, 60)
        l -= 60
    return out + _copy64(o, l)


def snappy_raw(c):
    """The raw Snappy encoding of one chunk (len(c) <= 65536), step for step as snappy 1.1.8 compresses it."""
    c = bytes(c)
    n = len(c)
    out = bytearray(_varint(n))
    size = 256
    while size < 16384 and size < n:
        size <<= 1
    shift = 32 - (size.bit_length() - 1)
    table = [0] * size

    def ld(p):
        return int.from_bytes(c[p:p + 4], "little")

    def hsh(p):
        return ((ld(p) * 0x1E35A7BD) & 0xFFFFFFFF) >> shift
    emit = 0
    if n >= 15:
        limit = n - 15
        ip = 1
        nh = hsh(1)
        while True:
            skip, nxt = 32, ip
            while True:
                ip, h = nxt, nh
                step = skip >> 5
                skip += step
                nxt = ip + step
                if nxt > limit:
                    break
                nh = hsh(nxt)
                cand = table[h]
                table[h] = ip
                if ld(ip) == ld(cand):
                    break
            if nxt > limit:
                break
            out += _literal(c[emit:ip])
            tail = False
            while True:
                m = 4
                while ip + m < n and c[cand + m] == c[ip + m]:
                    m += 1
                out += _copy(ip - cand, m)
                ip += m
                emit = ip
                if ip >= limit:
                    tail = True
                    break
                table[hsh(ip - 1)] = ip - 1
                h = hsh(ip)
                cand = table[h]
                table[h] = ip
                if ld(ip) != ld(cand):
                    break
            if tail:
                break
            ip += 1
            nh = hsh(ip)
    if emit < n:
        out += _literal(c[emit:])
    return bytes(out)


# ---------------------------------------------------------------- CRC-32C and the framing
def _crc32c_table():
    t = np.zeros(256, dtype=np.uint32)
    for i in range(256):
        r = i
        for _ in range(8):
            r = (r >> 1) ^ (0x82F63B78 if r & 1 else 0)
        t[i] = r
    return t


CRC32C_TABLE = _crc32c_table()


def crc32c_rows(rows):
    """CRC-32C of every row of a (k, m) uint8 array: one numpy step per byte position, all rows at once."""
    cols = np.ascontiguousarray(np.asarray(rows, dtype=np.uint8).T)  # (one contiguous row per byte position)
    crc = np.full(cols.shape[1], 0xFFFFFFFF, dtype=np.uint32)
    for i in range(cols.shape[0]):
        crc = CRC32C_TABLE[(crc ^ cols[i]) & 0xFF] ^ (crc >> np.uint32(8))
    return crc ^ np.uint32(0xFFFFFFFF)


def crc32c(b):
    return int(crc32c_rows(np.frombuffer(bytes(b), dtype=np.uint8)[None, :])[0]) if len(b) else 0


def mask(c):
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def frame_chunk(chunk, body, crc):
    """One chunk's frame from its raw encoding and its (unmasked) CRC-32C."""
    n = len(chunk)
    if len(body) >= n - n // 8:
        t, body = 1, bytes(chunk)
    else:
        t = 0
    return bytes([t]) + (len(body) + 4).to_bytes(3, "little") + struct.pack("<I", mask(crc)) + body


def frame_buffer(buf, raw):
    """FrameEncoder over one buffer: nothing for an empty one."""
    buf = bytes(buf)
    if not buf:
        return b""
    out = [IDENT]
    for k in range(0, len(buf), CHUNK):
        ch = buf[k:k + CHUNK]
        out.append(frame_chunk(ch, raw(ch), crc32c(ch)))
    return b"".join(out)


def frame_stream(data, bs, raw):
    """ParCompress<Snap>: the stream cut into buffer_size pieces, the last one short or empty (flush_last)."""
    data = bytes(data)
    pieces = [data[i:i + bs] for i in range(0, len(data), bs)]
    if len(data) % bs == 0:
        pieces.append(b"")
    return b"".join(frame_buffer(p, raw) for p in pieces)


def digest(b):
    d = {"sha256": hashlib.sha256(b).hexdigest(), "size": len(b)}
    if len(b) <= 1024:
        d["hex"] = b.hex()
    return d


# ---------------------------------------------------------------- the vector sets
RAW_SIZES = [0, 1, 14, 15, 16, 17, 255, 256, 257, 4095, 4096, 65535, 65536]


def raw_specs():
    specs = []
    for cls in sorted(synth.CLASSES):
        for n in RAW_SIZES:
            specs.append([cls, n, 11])
    for p in (1, 2, 3):
        for n in (20, 100, 4096, 65536):
            specs.append(["period", n, 21 + p, p])
    specs += echo_specs()
    for m in (59, 60, 61, 62, 256, 257, 65535, 65536):
        specs.append(["literal", 65536, 31, m])
    specs.append(["period", 65536, 40, 4])  # the first probe matches position 0 through the zeroed table
    specs.append(["text", 70000, 41])  # (cut to 65,536 by the test: a chunk of a longer stream)
    return specs


def framed_specs():
    out = []
    for bs in (32768, 65536, 65537, 131072, 1 << 20):
        for n in sorted({0, 1, bs - 1, bs, bs + 1, 65535, 65536, 65537, 2 * bs + 12345, 3 * bs}):
            for cls, seed in (("text", 51), ("random", 52), ("mixed", 53)):
                if bs == 1 << 20 and n > 2 * bs and cls != "text":
                    continue
                out.append([cls, n, seed, bs])
    return out


def main():
    raw = load_snappy()
    if raw is None:
        sys.exit("no snappy binary at %s" % SNAPPY_SO)
    res = {"generator": "tests/golden/make_snap_golden.py", "snappy": os.path.basename(SNAPPY_SO),
           "ident_hex": IDENT.hex(), "raw": [], "framed": []}
    for spec in raw_specs():
        a = make_input(spec)[:CHUNK].tobytes()
        body = raw(a)
        assert body == snappy_raw(a), spec  # the restatement is the binary's loop
        res["raw"].append({"spec": spec, **digest(body)})
    for spec in framed_specs():
        a = make_input(spec[:3]).tobytes()
        res["framed"].append({"spec": spec, **digest(frame_stream(a, spec[3], raw))})
    # the full-size digest: libsnappy over every chunk, CRC-32C vectorised across the chunks
    a = synth.text_slab(FULL_N, seed=FULL_SEED)
    assert FULL_N % FULL_BS == 0 and FULL_BS % CHUNK == 0
    crcs = crc32c_rows(a.reshape(-1, CHUNK))
    h = hashlib.sha256()
    size = 0
    per = FULL_BS // CHUNK
    for b in range(FULL_N // FULL_BS):
        h.update(IDENT)
        size += len(IDENT)
        for k in range(per):
            i = b * per + k
            ch = a[i * CHUNK:(i + 1) * CHUNK].tobytes()
            f = frame_chunk(ch, raw(ch), int(crcs[i]))
            h.update(f)
            size += len(f)
    res["fullsize"] = {"n": FULL_N, "seed": FULL_SEED, "buffer_size": FULL_BS, "sha256": h.hexdigest(), "size": size}
    with open(OUT, "w") as f:
        json.dump(res, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("%s: %d raw, %d framed vectors; full size %d -> %d" % (OUT, len(res["raw"]), len(res["framed"]), FULL_N, size))


if __name__ == "__main__":
    main()
