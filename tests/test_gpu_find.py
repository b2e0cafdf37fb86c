"""The search on the MI355X: the shared bodies of tests/find_cases.py through the real library, and a FASTQ stream
compressed on the device, searched through both inflate routes and compared with the host's search of the slab it was made
from."""
import numpy as np
import pytest
import torch

import find_cases
from gzp_amd import _native, synth
from test_gpu_ranges import _device_compress

pytestmark = pytest.mark.gpu


def test_hits_planted(hip_lib):
    find_cases.hits_planted(hip_lib)


def test_hits_small_members(hip_lib):
    find_cases.hits_small_members(hip_lib)


def test_hits_newline(hip_lib, oracle):
    find_cases.hits_newline(hip_lib, oracle)


def test_hits_special_bytes(hip_lib):
    find_cases.hits_special_bytes(hip_lib)


def test_hits_overlaps(hip_lib):
    find_cases.hits_overlaps(hip_lib)


def test_hits_edges(hip_lib):
    find_cases.hits_edges(hip_lib)


def test_batches_tiny_members(hip_lib):
    find_cases.batches_tiny_members(hip_lib)


def test_batches_every_split(hip_lib):
    find_cases.batches_every_split(hip_lib)


def test_lines(hip_lib):
    find_cases.lines(hip_lib)


def test_lines_close_the_loop(hip_lib):
    find_cases.lines_close_the_loop(hip_lib)


def test_capacity(hip_lib):
    find_cases.capacity(hip_lib)


def test_errors(hip_lib):
    find_cases.errors(hip_lib)


def test_damaged_member(hip_lib):
    find_cases.damaged(hip_lib)


# ---------------------------------------------------------------------------------------------------- more than one batch
def test_fastq_8mib(hip_lib):
    """8 MiB of FASTQ in 64 KiB BGZF blocks, level 1, compressed on the device: 129 members.  "@" (every record and more), a
    12-byte prefix of a read name, "\\n+\\n" and a 200-byte slice of the input, with the default batch and with batches of
    1 MiB, through both inflate routes; positions and lines against the host's search of the input."""
    n = 8 << 20
    host = synth.make("fastq", n, 20260103)
    plain = host.tobytes()
    d_in = torch.from_numpy(host).cuda()
    d_comp, comp_len = _device_compress(hip_lib, _native.FORMAT_BGZF, 1, 65280, d_in, n)
    second = plain.index(b"\n@", 3 << 20) + 1  # a record in the middle of the stream
    patterns = (b"@", plain[second:second + 12], b"\n+\n", plain[5000000:5000200])
    nl = np.flatnonzero(host == 10)
    want = []
    for pat in patterns:
        hits = find_cases.host_hits(plain, pat)
        want.append((hits, np.searchsorted(nl, hits, side="left")))
    assert want[0][0].size > nl.size // 4 and want[1][0].size >= 1 and want[2][0].size >= nl.size // 4 - 1 and 5000000 in want[3][0]
    with _native.DContext(format=_native.FORMAT_BGZF, lib=hip_lib) as d, d.build_index_device(d_comp.data_ptr(), comp_len) as ix:
        assert (ix.n_members, ix.inflated_len) == (-(-n // 65280) + 1, n)
        for route in (_native.INFLATE_SEG, _native.INFLATE_WAVE):
            for batch in (0, 1 << 20):
                d.set_route(route)
                d.set_lines_batch(batch)
                for pat, (hits, lines) in zip(patterns, want):
                    k = hits.size
                    assert d.find_device(ix, d_comp.data_ptr(), comp_len, pat) == k, (route, batch, pat[:12])
                    d_pos = torch.full((k + 4,), -2, dtype=torch.int64, device="cuda")
                    d_lines = torch.full((k + 4,), -2, dtype=torch.int64, device="cuda")
                    assert d.find_device(ix, d_comp.data_ptr(), comp_len, pat, 10, d_pos.data_ptr(), d_lines.data_ptr(), k) == k
                    assert np.array_equal(d_pos.cpu().numpy(), np.concatenate([hits, [-2] * 4])), (route, batch, pat[:12])
                    assert np.array_equal(d_lines.cpu().numpy(), np.concatenate([lines, [-2] * 4])), (route, batch, pat[:12])
                    assert all(t >= 0.0 for t in d.last_find_ms()) and d.last_find_ms()[1] > 0.0
