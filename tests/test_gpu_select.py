"""The selection of lines by content and the read by table on the MI355X: the shared bodies of tests/select_cases.py
through the real library -- the run of lost_updates here is the one that decides whether the bitmap update is atomic --
and a FASTQ stream compressed on the device, its records selected and read through both inflate routes and compared with
the host's computation on the slab it was made from."""
import numpy as np
import pytest
import torch

import find_cases
import select_cases
from gzp_amd import _native, synth
from test_gpu_ranges import _device_compress

pytestmark = pytest.mark.gpu


def test_edge_sets(hip_lib):
    select_cases.edge_sets(hip_lib)


def test_scan_step(hip_lib):
    select_cases.scan_step(hip_lib)


def test_records(hip_lib):
    select_cases.records(hip_lib)


def test_attribution_every_split(hip_lib):
    select_cases.attribution_every_split(hip_lib)


def test_attribution_tiny_members(hip_lib):
    select_cases.attribution_tiny_members(hip_lib)


def test_attribution_delimiters(hip_lib):
    select_cases.attribution_delimiters(hip_lib)


def test_lost_updates(hip_lib):
    select_cases.lost_updates(hip_lib)


def test_capacity(hip_lib):
    select_cases.capacity(hip_lib)


def test_errors(hip_lib):
    select_cases.errors(hip_lib)


def test_damaged_member(hip_lib):
    select_cases.damaged(hip_lib)


def test_table_reads(hip_lib, oracle):
    select_cases.table_reads(hip_lib, oracle)


def test_table_errors(hip_lib, oracle):
    select_cases.table_errors(hip_lib, oracle)


def test_close_the_loop(hip_lib):
    select_cases.close_the_loop(hip_lib)


# ---------------------------------------------------------------------------------------------------- more than one batch
def test_fastq_8mib(hip_lib):
    """8 MiB of FASTQ in 64 KiB BGZF blocks, level 1, compressed on the device: 129 members.  Records of four lines; a
    12-byte prefix of a read name (plain and inverted), "@" (every record), a 200-byte slice of the input and a pattern that
    is absent (plain and inverted), with the default batch and with batches of 1 MiB, through both inflate routes.  The
    runs, the counts and the bytes that read_lines_table_device returns for the table where select left it, against the
    host's computation on the input."""
    n, g = 8 << 20, 4
    host = synth.make("fastq", n, 20260103)
    plain = host.tobytes()
    d_in = torch.from_numpy(host).cuda()
    d_comp, comp_len = _device_compress(hip_lib, _native.FORMAT_BGZF, 1, 65280, d_in, n)
    nl = np.flatnonzero(host == 10)
    L = nl.size + (0 if host[-1] == 10 else 1)
    R = -(-L // g)
    start = np.concatenate([[0], nl + 1, [n] if L > nl.size else []]).astype(np.int64)
    second = plain.index(b"\n@", 3 << 20) + 1  # a record in the middle of the stream
    cases = ((plain[second:second + 12], False), (plain[second:second + 12], True), (b"@", False), (plain[5000000:5000200], False),
             (b"no such read", False), (b"no such read", True))
    want = []
    for pat, invert in cases:
        hits = find_cases.host_hits(plain, pat)
        sel = np.zeros(R, dtype=bool)
        sel[np.unique(np.searchsorted(nl, hits, side="left") // g)] = True
        if invert:
            sel = ~sel
        edge = np.diff(np.concatenate([[0], sel.astype(np.int8), [0]]))
        runs = np.stack([g * np.flatnonzero(edge == 1), np.minimum(g * np.flatnonzero(edge == -1), L)], axis=1).astype(np.int64)
        data = b"".join(plain[start[a]:start[b]] for a, b in runs.tolist())
        want.append((runs, int(sel.sum()), hits.size, data))
    assert want[0][1] >= 1 and want[1][1] == R - want[0][1] and want[2][1] == R and want[2][3] == plain and want[3][2] >= 1
    assert want[4][0].size == 0 and want[4][1:3] == (0, 0) and want[5][0].tolist() == [[0, L]] and want[5][1] == R
    cap_runs = -(-R // 2)
    with _native.DContext(format=_native.FORMAT_BGZF, lib=hip_lib) as d, d.build_index_device(d_comp.data_ptr(), comp_len) as ix, \
            d.build_lines_device(ix, d_comp.data_ptr(), comp_len) as lt:
        assert (ix.n_members, ix.inflated_len, lt.n_lines) == (-(-n // 65280) + 1, n, L)
        for route in (_native.INFLATE_SEG, _native.INFLATE_WAVE):
            for batch in (0, 1 << 20):
                d.set_route(route)
                d.set_lines_batch(batch)
                for (pat, invert), (runs, records, hits, data) in zip(cases, want):
                    what = (route, batch, pat[:12], invert)
                    k = runs.shape[0]
                    assert d.select_lines_device(ix, lt, d_comp.data_ptr(), comp_len, pat, g, invert) == (k, records, hits), what
                    d_runs = torch.full((cap_runs + 4, 2), -2, dtype=torch.int64, device="cuda")
                    got = d.select_lines_device(ix, lt, d_comp.data_ptr(), comp_len, pat, g, invert, d_runs.data_ptr(), cap_runs)
                    assert got == (k, records, hits), what
                    assert all(t >= 0.0 for t in d.last_select_ms()) and d.last_select_ms()[1] > 0.0
                    table = d_runs.cpu().numpy()
                    assert np.array_equal(table[:k], runs) and bool(np.all(table[k:] == -2)), what
                    d_out = torch.full((len(data) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
                    out_len = d.read_lines_table_device(ix, lt, d_comp.data_ptr(), comp_len, d_runs.data_ptr(), k, d_out.data_ptr(),
                                                        len(data))
                    assert out_len == len(data), what
                    assert d_out.cpu().numpy().tobytes() == data + b"\xEE" * 64, what
