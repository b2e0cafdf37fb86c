"""Random-access reads by range on the MI355X: the shared bodies of tests/range_cases.py through the real library, and
full-size streams compressed on the device (as tests/test_gpu_scan_device.py does), read by thousands of ranges and
compared on the device with slices of the slab they were made from."""
import numpy as np
import pytest
import torch

import range_cases
from gzp_amd import _native, synth

pytestmark = pytest.mark.gpu


def test_index(hip_lib, oracle):
    range_cases.index(hip_lib, oracle)


def test_empty_stream(hip_lib):
    range_cases.empty_stream(hip_lib)


def test_ranges(hip_lib, oracle):
    range_cases.ranges(hip_lib, oracle)


def test_virtual_offsets(hip_lib, oracle):
    range_cases.virtual(hip_lib, oracle)


def test_errors(hip_lib):
    range_cases.errors(hip_lib)


def test_only_needed_members_are_touched(hip_lib):
    range_cases.touched(hip_lib)


def test_members_around_the_several_waves_size(hip_lib):
    range_cases.big_members(hip_lib)


# ---------------------------------------------------------------------------------------------------- full size
def _device_compress(lib, fmt, level, bs, d_in, n):
    with _native.Context(format=fmt, level=level, buffer_size=bs, lib=lib, max_slab_bytes=n) as ctx:
        cap = ctx.slab_bound(n)
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        out_len, _ = ctx.compress_slab_device(d_in.data_ptr(), n, d_out.data_ptr(), cap, True)
    return d_out, out_len


def _random_ranges(seed, total, count, max_len, cap):
    """`count` ranges at uniformly random places, lengths log-uniform in [1, max_len]; where the running total of the
    lengths would pass `cap`, a length is cut to what is left of it (the ranges behind that point are empty)."""
    rng = np.random.default_rng(seed)
    lens = np.minimum(np.exp(rng.uniform(0.0, np.log(max_len), count)).astype(np.int64), min(max_len, total))
    room = cap - (np.cumsum(lens) - lens)
    lens = np.clip(np.minimum(lens, room), 0, None)
    begins = (rng.random(count) * (total - lens + 1)).astype(np.int64)
    return np.stack([begins, begins + lens], axis=1).astype(np.uint64)


def _expected(d_plain, period, ranges):
    """The ranges' bytes of the stream whose inflated form is d_plain[:period] over and over: one indexed gather."""
    b = torch.from_numpy(ranges[:, 0].astype(np.int64)).cuda()
    lens = torch.from_numpy((ranges[:, 1] - ranges[:, 0]).astype(np.int64)).cuda()
    out_off = torch.cumsum(lens, 0) - lens
    idx = torch.repeat_interleave(b - out_off, lens)
    idx += torch.arange(idx.numel(), device="cuda")
    idx %= period
    return d_plain[idx]


def _union_size(entries, ranges):
    """Members a read must touch, by the rule of include/gzpx.h, on the host."""
    ustart = entries[:, 1].astype(np.int64)
    r = ranges[ranges[:, 1] > ranges[:, 0]].astype(np.int64)
    first = np.searchsorted(ustart, r[:, 0], side="right") - 1
    last = np.searchsorted(ustart, r[:, 1], side="left") - 1
    diff = np.zeros(ustart.size + 1, dtype=np.int64)
    np.add.at(diff, first, 1)
    np.add.at(diff, last + 1, -1)
    return int((np.cumsum(diff)[:-1] > 0).sum())


def _read_and_check(d, ix, d_comp, comp_len, d_plain, period, ranges, what):
    total = int((ranges[:, 1] - ranges[:, 0]).sum())
    d_out = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    out_len, offs = d.read_ranges_device(ix, d_comp.data_ptr(), comp_len, ranges, d_out.data_ptr() + 1, total)
    lens = (ranges[:, 1] - ranges[:, 0]).astype(np.uint64)
    assert out_len == total and np.array_equal(offs, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)), what
    assert torch.equal(d_out[1:1 + total], _expected(d_plain, period, ranges)), what
    assert bool((d_out[1 + total:] == 0xEE).all()) and int(d_out[0]) == 0xEE, what
    assert d.last_ranges_members() == _union_size(ix.entries(), ranges), what
    ms = d.last_ranges_ms()
    assert all(t > 0.0 for t in ms) or total == 0, (what, ms)


def test_config1_550mib_bgzf_ranges(hip_lib):
    """configs[1]: the 550 MiB text slab in 64 KiB BGZF blocks, level 1.  20,000 ranges with log-uniform lengths between
    1 byte and 1 MiB (seed fixed, 512 MiB of output at most), one range over the whole stream in a call of its own, the
    first 2,000 again through the other inflate route.  Then the same stream 21 times back to back (above 2^32
    compressed bytes) with a handful of ranges on both sides of the 4 GiB line."""
    n = 576_716_800
    d_in = torch.from_numpy(synth.text_slab(n, seed=20250927)).cuda()
    d_comp, comp_len = _device_compress(hip_lib, _native.FORMAT_BGZF, 1, 65280, d_in, n)
    ranges = _random_ranges(20260101, n, 20000, 1 << 20, 512 << 20)
    assert int((ranges[:, 1] - ranges[:, 0]).sum()) == 512 << 20
    with _native.DContext(format=_native.FORMAT_BGZF, lib=hip_lib) as d:
        with d.build_index_device(d_comp.data_ptr(), comp_len) as ix:
            assert (ix.n_members, ix.consumed, ix.inflated_len) == (-(-n // 65280) + 1, comp_len, n)
            _read_and_check(d, ix, d_comp, comp_len, d_in, n, ranges, "20,000 ranges")
            _read_and_check(d, ix, d_comp, comp_len, d_in, n, np.array([[0, n]], dtype=np.uint64), "whole stream")
            assert d.last_ranges_members() == ix.n_members - 1  # (all but the EOF marker)
            d.set_route(_native.INFLATE_WAVE)
            _read_and_check(d, ix, d_comp, comp_len, d_in, n, ranges[:2000], "2,000 ranges, k_inflate")
            d.set_route(_native.INFLATE_SEG)
            # the same slices as virtual offsets
            e = ix.entries()
            r = ranges[:5000].astype(np.int64)
            m0 = np.searchsorted(e[:, 1].astype(np.int64), r[:, 0], side="right") - 1
            m1 = np.searchsorted(e[:, 1].astype(np.int64), r[:, 1], side="right") - 1
            vr = np.stack([(e[m0, 0] << np.uint64(16)) | (r[:, 0] - e[m0, 1].astype(np.int64)).astype(np.uint64),
                           (e[m1, 0] << np.uint64(16)) | (r[:, 1] - e[m1, 1].astype(np.int64)).astype(np.uint64)], axis=1)
            total = int((r[:, 1] - r[:, 0]).sum())
            d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
            out_len, offs = d.read_ranges_device(ix, d_comp.data_ptr(), comp_len, vr, d_out.data_ptr(), total, "virtual")
            assert out_len == total and torch.equal(d_out[:total], _expected(d_in, n, ranges[:5000]))
            del d_out
        reps = (1 << 32) // comp_len + 2
        d_big = d_comp[:comp_len].repeat(reps)
        big_len = reps * comp_len
        assert big_len > (1 << 32)
        with d.build_index_device(d_big.data_ptr(), big_len) as ix:
            assert (ix.consumed, ix.inflated_len) == (big_len, reps * n)
            e = ix.entries()
            k = int(np.searchsorted(e[:, 0], np.uint64(1 << 32)))  # the first member that starts behind the line
            u = int(e[k, 1])
            t = reps * n
            rs = np.array([(u - (3 << 20), u - (2 << 20)), (u - 100, u + 100), (u - 1, u + 1), (u + (5 << 20), u + (6 << 20) + 17),
                           (0, 1000), (t - 1000, t), (u - 65280, u), (u, u + 65281), (t - n - 5, t - n + 5)], dtype=np.uint64)
            _read_and_check(d, ix, d_big, big_len, d_in, n, rs, "above 2^32")
            assert int(e[k, 0]) >= (1 << 32) > int(e[k - 1, 0])


def test_mgzip_1mib_members_ranges(hip_lib):
    """Mgzip with 1 MiB members (several waves inflate each): 256 MiB of ASCII noise at level 3, 300 ranges of up to
    4 MiB, and the whole stream."""
    n = 256 << 20
    d_in = torch.from_numpy(synth.make("ascii", n, 4242)).cuda()
    d_comp, comp_len = _device_compress(hip_lib, _native.FORMAT_MGZIP, 3, 1 << 20, d_in, n)
    ranges = _random_ranges(20260102, n, 300, 4 << 20, 1 << 40)
    with _native.DContext(format=_native.FORMAT_MGZIP, lib=hip_lib) as d:
        with d.build_index_device(d_comp.data_ptr(), comp_len) as ix:
            assert (ix.n_members, ix.consumed, ix.inflated_len) == (n >> 20, comp_len, n)
            _read_and_check(d, ix, d_comp, comp_len, d_in, n, ranges, "300 ranges")
            _read_and_check(d, ix, d_comp, comp_len, d_in, n, np.array([[0, n]], dtype=np.uint64), "whole stream")
            assert d.last_ranges_members() == ix.n_members
