"""Member discovery on the MI355X: the shared bodies of tests/scan_cases.py through the real library, and the
full-size streams of tests/test_gpu_fullsize.py compressed on the device and never copied to the host before the call
under test."""
import numpy as np
import pytest
import torch

import scan_cases
from gzp_amd import _native, synth

pytestmark = pytest.mark.gpu


def test_well_formed_streams(hip_lib, oracle):
    scan_cases.well_formed(hip_lib, oracle)


def test_foreign_members(hip_lib):
    scan_cases.foreign_members(hip_lib)


def test_truncation(hip_lib):
    scan_cases.truncation(hip_lib)


def test_max_blocks(hip_lib, oracle):
    scan_cases.max_blocks(hip_lib, oracle)


def test_invalid_headers(hip_lib):
    scan_cases.invalid_headers(hip_lib)


def test_impostors(hip_lib, oracle):
    scan_cases.impostors(hip_lib, oracle)


def test_stream_decompress(hip_lib, oracle):
    scan_cases.stream_decompress(hip_lib, oracle, scale=4)


def test_index(hip_lib, oracle):
    scan_cases.index(hip_lib, oracle, scale=4)


def _device_compress(lib, fmt, level, bs, d_in, n):
    with _native.Context(format=fmt, level=level, buffer_size=bs, lib=lib, max_slab_bytes=n) as ctx:
        cap = ctx.slab_bound(n)
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        out_len, _ = ctx.compress_slab_device(d_in.data_ptr(), n, d_out.data_ptr(), cap, True)
    return d_out, out_len


def _full_size(lib, fmt, level, bs, d_in, n):
    d_comp, comp_len = _device_compress(lib, fmt, level, bs, d_in, n)
    d_back = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    with _native.DContext(format=fmt, lib=lib) as d:
        # the calls under test: nothing of the stream has been on the host
        got, nb, consumed = d.decompress_stream_device(d_comp.data_ptr(), comp_len, d_back.data_ptr(), n + 64)
        assert (got, consumed) == (n, comp_len)
        assert torch.equal(d_back[:n], d_in[:n])
        offs, sizes, used = d.scan_blocks_device(d_comp.data_ptr(), comp_len)
        assert d.last_scan_ms() > 0.0
        idx, iused, total = d.index_device(d_comp.data_ptr(), comp_len)
        # afterwards, as the check: the host's walk of the same bytes
        comp = d_comp[:comp_len].cpu().numpy()
        ho, hs, hu = d.scan_blocks(comp)
    assert nb == ho.size and used == hu == comp_len
    assert np.array_equal(offs, ho) and np.array_equal(sizes, hs)
    assert iused == comp_len and total == n and np.array_equal(idx[:, 0], ho)
    ends = ho.astype(np.int64) + hs.astype(np.int64)
    isize = np.stack([comp[e - 4:e] for e in ends]).copy().view("<u4").ravel().astype(np.uint64)
    assert np.array_equal(idx[:, 1], np.concatenate([[0], np.cumsum(isize)[:-1]]).astype(np.uint64))
    return d_comp, comp_len, ho, hs


def test_config1_550mib_bgzf_stream_device(hip_lib):
    """configs[1]: the 550 MiB text slab in 64 KiB BGZF blocks, level 1.  Then the same stream 21 times back to back
    (a concatenation of BGZF streams is a BGZF stream; 4.4 GB of compressed bytes, above 2^32: the offsets need their
    64 bits), scanned on the device and compared with the host's walk of the bytes copied back."""
    n = 576_716_800
    d_in = torch.from_numpy(synth.text_slab(n, seed=20250927)).cuda()
    d_comp, comp_len, ho, hs = _full_size(hip_lib, _native.FORMAT_BGZF, 1, 65280, d_in, n)
    assert ho.size == -(-n // 65280) + 1 and int(hs[-1]) == 28
    del d_in
    reps = (1 << 32) // comp_len + 2
    d_big = d_comp[:comp_len].repeat(reps)
    big_len = reps * comp_len
    assert big_len > (1 << 32)
    with _native.DContext(format=_native.FORMAT_BGZF, lib=hip_lib) as d:
        nb, used = d.scan_blocks_device(d_big.data_ptr(), big_len, want_tables=False)
        assert (nb, used) == (reps * ho.size, big_len)
        offs, sizes, used = d.scan_blocks_device(d_big.data_ptr(), big_len)
        cut = big_len - 1000  # the last member (an EOF marker) and the one before it are cut off
        o2, s2, u2 = d.scan_blocks_device(d_big.data_ptr(), cut)
        big = d_big.cpu().numpy()
        bo, bs_, bu = d.scan_blocks(big)
        co, cs, cu = d.scan_blocks(big[:cut])
    assert bu == big_len == used and int(bo[-1]) > (1 << 32)
    assert np.array_equal(offs, bo) and np.array_equal(sizes, bs_)
    assert u2 == cu and np.array_equal(o2, co) and np.array_equal(s2, cs) and co.size == bo.size - 2


def test_config2_mgzip_1mib_blocks_stream_device(hip_lib):
    """configs[2]'s shape: Mgzip, 1 MiB blocks, level 3, 1 GiB of ASCII noise (members of about 0.85 MiB: several
    waves inflate each, which the scan path decides from consumed / n_blocks)."""
    n = 1 << 30
    d_in = torch.from_numpy(synth.make("ascii", n, 4242)).cuda()
    d_comp, comp_len, ho, hs = _full_size(hip_lib, _native.FORMAT_MGZIP, 3, 1 << 20, d_in, n)
    assert ho.size == n >> 20
