"""Grow-on-demand scratch on real device memory: ONE compress context and ONE DContext live through calls whose sizes go
small, large, small, larger, so that every group of allocations the contexts own (gzp_amd/csrc/gzpx_own.h) is released
and allocated again at least twice with uses of the old arrays in between.  No failure is injected here (the CPU
emulator does that, tests/test_emu_ownership.py); every result is compared with the oracle or with the input."""
import zlib

import numpy as np
import pytest

from gzp_amd import _native, synth
from scan_cases import BGZF, Mem, member

pytestmark = pytest.mark.gpu

BS = 65280
CHUNK = 4500  # bytes per member of the streams that are inflated (the tables grow with the members, not the bytes)


def _stream(text, n_members):
    plain = text[:n_members * CHUNK].tobytes()
    return plain, b"".join(member(BGZF, plain[i:i + CHUNK], 1) for i in range(0, len(plain), CHUNK))


def test_contexts_outlive_two_rounds_of_growth(hip_lib, oracle):
    text = synth.text_slab(200 * BS, base_bytes=2_000_000, seed=31)
    mem = Mem(hip_lib)
    # (batches of 16 blocks: the slabs below are 1, 4, 1 and 13 batches, so the per-batch result records grow as well)
    with _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=BS, lib=hip_lib, max_slab_bytes=16 * BS) as c, \
            _native.DContext(format=_native.FORMAT_BGZF, lib=hip_lib) as d:
        for n in (100, 64 * BS, 100, 200 * BS):
            want = oracle.compress_stream(text[:n], oracle.FMT_BGZF, 1, oracle.COMPAT_1_24, BS)
            assert c.compress_slab(text[:n], True) == want, "slab of %d bytes" % n
        for n_members in (1, 300, 1, 2000):
            plain, s = _stream(text, n_members)
            what = "%d members" % n_members
            assert d.decompress(s) == plain, what
            keep, ptr = mem.put(s, shift=3)
            out, p_out = mem.empty(len(plain) + 64)
            assert d.decompress_stream_device(ptr, len(s), p_out, len(plain) + 64) == (len(plain), n_members, len(s)), what
            assert mem.get(out, len(plain)) == plain, what
            offs, sizes, used = d.scan_blocks(s)
            got = d.scan_blocks_device(ptr, len(s))
            assert (got[0].tolist(), got[1].tolist(), got[2]) == (offs.tolist(), sizes.tolist(), used), what
        # (plain, s, ptr, out: the 2000-member stream)
        with d.build_index_device(ptr, len(s)) as ix:
            assert (ix.n_members, ix.consumed, ix.inflated_len) == (2000, len(s), len(plain))
            one = [(len(plain) // 3, len(plain) // 3 + 999)]
            many = [((i * 104729) % (len(plain) - 4096), (i * 104729) % (len(plain) - 4096) + 4096) for i in range(500)]
            for ranges in (one, many, one):
                want = b"".join(plain[b:e] for b, e in ranges)
                m, o = d.read_ranges_device(ix, ptr, len(s), ranges, p_out, len(want))
                assert m == len(want) and mem.get(out, m) == want, "%d ranges" % len(ranges)
                assert o.tolist() == np.cumsum([0] + [e - b for b, e in ranges]).tolist()
        for n in (3, 400):
            parts = [plain[i * 9000:i * 9000 + 1 + (i * 977) % 9000] for i in range(n)]
            zs = [zlib.compress(p, 1) for p in parts]
            total = sum(len(p) for p in parts)
            t = [mem.put(b"".join(zs)), mem.put(np.cumsum([0] + [len(z) for z in zs[:-1]]).astype(np.uint64).view(np.uint8)),
                 mem.put(np.array([len(z) for z in zs], dtype=np.uint32).view(np.uint8)),
                 mem.put(np.array([len(p) for p in parts], dtype=np.uint32).view(np.uint8))]
            got = d.inflate_batch_device(_native.WRAP_ZLIB, t[0][1], sum(len(z) for z in zs), t[1][1], t[2][1], t[3][1], n,
                                         p_out, total)
            assert got == (total, 0) and mem.get(out, total) == b"".join(parts), "batch of %d" % n
