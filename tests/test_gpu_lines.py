"""Reads by line on the MI355X: the shared bodies of tests/line_cases.py through the real library, and a FASTQ stream
compressed on the device, read by thousands of record ranges and compared on the device with slices of the slab it was
made from."""
import numpy as np
import pytest
import torch

import line_cases
from gzp_amd import _native, synth
from test_gpu_ranges import _device_compress, _expected, _union_size

pytestmark = pytest.mark.gpu
T = _native.LINES_TILE


def test_table(hip_lib, oracle):
    line_cases.table(hip_lib, oracle)


def test_offsets(hip_lib, oracle):
    line_cases.offsets(hip_lib, oracle)


def test_reads(hip_lib, oracle):
    line_cases.reads(hip_lib, oracle)


def test_errors(hip_lib, oracle):
    line_cases.errors(hip_lib, oracle)


def test_only_needed_members_are_touched(hip_lib):
    line_cases.touched(hip_lib)


# ---------------------------------------------------------------------------------------------------- more than one batch
def test_fastq_8mib_records(hip_lib):
    """8 MiB of FASTQ in 64 KiB BGZF blocks, level 1, compressed on the device: 129 members, 512 tiles.  The table with the
    default batch and with batches of 1 MiB; 2,000 ranges of 1 to 500 records (four lines each, seed fixed) plus the whole
    stream, through both inflate routes, compared on the device with slices of the input."""
    n = 8 << 20
    host = synth.make("fastq", n, 20260103)
    d_in = torch.from_numpy(host).cuda()
    d_comp, comp_len = _device_compress(hip_lib, _native.FORMAT_BGZF, 1, 65280, d_in, n)
    pos = np.flatnonzero(host == 10).astype(np.int64)
    D = int(pos.size)
    L = D if host[-1] == 10 else D + 1
    start = np.concatenate([[0], pos + 1, [n] if L > D else []]).astype(np.int64)
    P = np.concatenate([[0], np.cumsum(np.bincount(pos // T, minlength=n // T))]).astype(np.int64)
    rng = np.random.default_rng(20260104)
    records = L // 4
    count = rng.integers(1, 501, 2000)
    first = (rng.random(2000) * (records - count + 1)).astype(np.int64)
    lr = np.stack([4 * first, 4 * (first + count)], axis=1)
    lr = np.concatenate([lr, [[0, L]]]).astype(np.int64)
    br = np.stack([start[lr[:, 0]], start[lr[:, 1]]], axis=1).astype(np.uint64)
    tile = lambda k: np.searchsorted(P[1:], k, side="left")  # (1 <= k <= D)
    cover = np.stack([np.where(lr[:, 0] == 0, 0, T * tile(np.maximum(lr[:, 0], 1))),
                      np.where(lr[:, 1] > D, n, np.minimum(T * (tile(np.minimum(lr[:, 1], D)) + 1), n))], axis=1).astype(np.uint64)
    total = int((br[:, 1] - br[:, 0]).sum())
    with _native.DContext(format=_native.FORMAT_BGZF, lib=hip_lib) as d, d.build_index_device(d_comp.data_ptr(), comp_len) as ix:
        assert (ix.n_members, ix.inflated_len) == (-(-n // 65280) + 1, n)
        for route in (_native.INFLATE_SEG, _native.INFLATE_WAVE):
            for batch in (0, 1 << 20):
                d.set_route(route)
                d.set_lines_batch(batch)
                with d.build_lines_device(ix, d_comp.data_ptr(), comp_len) as lt:
                    assert (lt.n_delims, lt.n_lines) == (D, L) and np.array_equal(lt.prefix(), P.astype(np.uint64)), (route, batch)
                    d_out = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
                    out_len, offs, got_br = d.read_lines_device(ix, lt, d_comp.data_ptr(), comp_len, lr, d_out.data_ptr() + 1, total)
                    assert out_len == total and np.array_equal(got_br, br), (route, batch)
                    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(br[:, 1] - br[:, 0])]).astype(np.uint64))
                    assert torch.equal(d_out[1:1 + total], _expected(d_in, n, br)), (route, batch)
                    assert bool((d_out[1 + total:] == 0xEE).all()) and int(d_out[0]) == 0xEE
                    assert d.last_lines_members() == _union_size(ix.entries(), cover)
                    assert all(t > 0.0 for t in d.last_lines_ms())
                    # the records alone: the members behind the last cover stay untouched
                    out_len, offs, got_br = d.read_lines_device(ix, lt, d_comp.data_ptr(), comp_len, lr[:50], d_out.data_ptr(), total)
                    assert np.array_equal(got_br, br[:50]) and torch.equal(d_out[:out_len], _expected(d_in, n, br[:50]))
                    assert d.last_lines_members() == _union_size(ix.entries(), cover[:50]) < ix.n_members - 1
                    ks = np.arange(0, L + 1, max(L // 8, 1))  # where a sharder's eight parts start
                    assert np.array_equal(d.line_offsets_device(ix, lt, d_comp.data_ptr(), comp_len, ks), start[ks].astype(np.uint64))
