"""The search for a set of patterns on the MI355X: the shared bodies of tests/findset_cases.py through the real library,
and a FASTQ stream compressed on the device, searched for sets through both inflate routes and compared with the host's
merge of its single-pattern searches of the slab the stream was made from."""
import numpy as np
import pytest
import torch

import find_cases
import findset_cases
from gzp_amd import _native, synth
from test_gpu_ranges import _device_compress

pytestmark = pytest.mark.gpu


def test_one_pattern(hip_lib):
    findset_cases.one_pattern(hip_lib)


def test_mixed_lengths(hip_lib):
    findset_cases.mixed_lengths(hip_lib)


def test_same_position(hip_lib):
    findset_cases.same_position(hip_lib)


def test_buckets(hip_lib):
    findset_cases.buckets(hip_lib)


def test_order_every_split(hip_lib):
    findset_cases.order_every_split(hip_lib)


def test_waiting_carry(hip_lib):
    findset_cases.waiting_carry(hip_lib)


def test_dense_overlaps(hip_lib):
    findset_cases.dense_overlaps(hip_lib)


def test_special_bytes(hip_lib):
    findset_cases.special_bytes(hip_lib)


def test_lines(hip_lib):
    findset_cases.lines(hip_lib)


def test_lines_close_the_loop(hip_lib):
    findset_cases.lines_close_the_loop(hip_lib)


def test_capacity(hip_lib):
    findset_cases.capacity(hip_lib)


def test_errors(hip_lib):
    findset_cases.errors(hip_lib)


def test_damaged_member(hip_lib):
    findset_cases.damaged(hip_lib)


def test_selection(hip_lib):
    findset_cases.selection(hip_lib)


def test_selection_errors(hip_lib):
    findset_cases.selection_errors(hip_lib)


def test_selection_damaged_member(hip_lib):
    findset_cases.selection_damaged(hip_lib)


# ---------------------------------------------------------------------------------------------------- more than one batch
def test_fastq_8mib(hip_lib):
    """8 MiB of FASTQ in 64 KiB BGZF blocks, level 1, compressed on the device: 129 members.  Two sets: the four patterns
    of tests/test_gpu_find.py::test_fastq_8mib ("@", a 12-byte prefix of a read name, "\\n+\\n" and a 200-byte slice) in one
    set, and 16 eight-byte slices of reads (the barcode case: a 4-byte window of ACGT passes the filter nearly everywhere).
    The default batch and batches of 1 MiB, both inflate routes; positions, ids, lines and counts against the host's merge
    of its single-pattern searches of the input."""
    n = 8 << 20
    host = synth.make("fastq", n, 20260103)
    plain = host.tobytes()
    d_in = torch.from_numpy(host).cuda()
    d_comp, comp_len = _device_compress(hip_lib, _native.FORMAT_BGZF, 1, 65280, d_in, n)
    second = plain.index(b"\n@", 3 << 20) + 1  # a record in the middle of the stream
    read = lambda at: plain.index(b"\n", plain.index(b"\n@", at) + 1) + 1  # the first base of the read behind `at`
    mixed = [b"@", plain[second:second + 12], b"\n+\n", plain[5000000:5000200]]
    barcodes = [plain[read(j * (n // 17)) + 3 * j:][:8] for j in range(16)]
    assert all(set(b) <= set(b"ACGTN") for b in barcodes)
    nl = np.flatnonzero(host == 10)
    want = []
    for patterns in (mixed, barcodes):
        per = [find_cases.host_hits(plain, p) for p in patterns]
        pos = np.concatenate(per)
        ids = np.concatenate([np.full(h.size, k, np.int64) for k, h in enumerate(per)])
        order = np.lexsort((ids, pos))
        pos, ids = pos[order], ids[order]
        want.append((patterns, pos, ids, np.searchsorted(nl, pos, side="left"), np.array([h.size for h in per])))
    assert want[0][4][0] > nl.size // 4 and want[0][4][1] >= 1 and 5000000 in want[0][1] and bool(np.all(want[1][4] >= 1))
    with _native.DContext(format=_native.FORMAT_BGZF, lib=hip_lib) as d, d.build_index_device(d_comp.data_ptr(), comp_len) as ix:
        assert (ix.n_members, ix.inflated_len) == (-(-n // 65280) + 1, n)
        for route in (_native.INFLATE_SEG, _native.INFLATE_WAVE):
            for batch in (0, 1 << 20):
                d.set_route(route)
                d.set_lines_batch(batch)
                for patterns, pos, ids, lines, counts in want:
                    k, what = pos.size, (route, batch, len(patterns))
                    d_counts = torch.full((len(patterns) + 4,), -2, dtype=torch.int64, device="cuda")
                    assert d.find_set_device(ix, d_comp.data_ptr(), comp_len, patterns, d_counts_ptr=d_counts.data_ptr()) == k, what
                    assert np.array_equal(d_counts.cpu().numpy(), np.concatenate([counts, [-2] * 4])), what
                    d_pos = torch.full((k + 4,), -2, dtype=torch.int64, device="cuda")
                    d_ids = torch.full((k + 4,), -2, dtype=torch.int32, device="cuda")
                    d_lines = torch.full((k + 4,), -2, dtype=torch.int64, device="cuda")
                    assert d.find_set_device(ix, d_comp.data_ptr(), comp_len, patterns, 10, d_pos.data_ptr(), d_ids.data_ptr(),
                                             d_lines.data_ptr(), k) == k, what
                    assert np.array_equal(d_pos.cpu().numpy(), np.concatenate([pos, [-2] * 4])), what
                    assert np.array_equal(d_ids.cpu().numpy(), np.concatenate([ids, [-2] * 4])), what
                    assert np.array_equal(d_lines.cpu().numpy(), np.concatenate([lines, [-2] * 4])), what
                    assert all(t >= 0.0 for t in d.last_find_set_ms()) and d.last_find_set_ms()[1] > 0.0
