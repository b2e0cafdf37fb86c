"""The compressor's CRC kernel (k_crc32) on blocks that start off a dword boundary, written once and run twice: through
the emulated library on CPU (tests/test_emu_crc.py, where a device pointer is a host pointer) and through the real HIP
library on the MI355X (tests/test_gpu_crc.py).

Every other caller of compress_slab_device hands over an aligned tensor, so the byte alignment that the 256-byte
segment takes out of its loads, and its rule about the dword behind the input's end, are met here alone on the
compress side: level 1 from `base + mis` for mis in 0..3, lengths around the segment (256), around buffer_size (a
block's end that is the slab's end, and one that is not) and around the routine's 64 KiB chunk.  The yardstick is
zlib.crc32 of every member's chunk, compared exactly, with the member's ISIZE."""
import struct
import zlib

import numpy as np

import scan_cases
from checksum_cases import put_aligned
from gzp_amd import _native

BGZF, MGZIP = _native.FORMAT_BGZF, _native.FORMAT_MGZIP
SHAPES = {
    "bgzf": (BGZF, 32771, (0, 1, 3, 4, 5, 255, 256, 257, 511, 513, 32771, 32772, 70000)),
    "mgzip": (MGZIP, 131075, (65535, 65536, 65537, 65791, 65793, 131075, 131333)),  # across crc32_direct's 64 KiB chunk
}
MISALIGNMENTS = (0, 1, 2, 3)


def trailers(fmt, stream):
    """(CRC-32, ISIZE) of every member of a stream, walked by BSIZE (BGZF) / the member size (Mgzip)."""
    out, pos = [], 0
    while pos < len(stream):
        assert stream[pos:pos + 4] == b"\x1f\x8b\x08\x04", pos
        if fmt == BGZF:
            size = struct.unpack_from("<H", stream, pos + 16)[0] + 1
        else:
            size = struct.unpack_from("<I", stream, pos + 16)[0]
        assert size >= 26 and pos + size <= len(stream), (pos, size)
        out.append(struct.unpack_from("<II", stream, pos + size - 8))
        pos += size
    return out


def misaligned_blocks(lib, shape):
    """Returns how many members were checked."""
    fmt, buffer_size, lengths = SHAPES[shape]
    blob = np.random.RandomState(23).randint(0, 256, max(lengths), dtype=np.uint8).tobytes()
    mem = scan_cases.Mem(lib)
    checked = 0
    with _native.Context(format=fmt, level=1, buffer_size=buffer_size, max_slab_bytes=max(lengths), lib=lib) as ctx:
        cap = ctx.slab_bound(max(lengths))
        h_out, d_out = mem.empty(cap)
        for mis in MISALIGNMENTS:
            for n in lengths:
                # (a copy of its own per length: the input's last byte is the allocation's last but one)
                h_in, d_in = put_aligned(mem, blob[:n], mis)
                assert d_in % 4 == mis
                out_len, nb = ctx.compress_slab_device(d_in, n, d_out, cap, True)
                got = trailers(fmt, mem.get(h_out, out_len))
                chunks = [blob[b:min(b + buffer_size, n)] for b in range(0, n, buffer_size)] or [b""]
                want = [(zlib.crc32(c), len(c)) for c in chunks]
                assert nb == len(want), (shape, mis, n, nb)
                # BGZF ends with its end-of-file marker, an empty member
                assert got == want + ([(0, 0)] if fmt == BGZF else []), (shape, mis, n, got, want)
                checked += len(got)
                del h_in
    return checked
