"""The fields of lines on the MI355X: the shared bodies of tests/field_cases.py through the real library, and a TSV of
8 MiB compressed on the device -- more pieces than one wave of workgroups, carries that run through many pieces -- read
through both inflate routes and compared with split and join on the host's copy."""
import numpy as np
import pytest
import torch

import field_cases
from field_cases import END, NL, TAB
from gzp_amd import _native
from test_gpu_ranges import _device_compress

pytestmark = pytest.mark.gpu


def test_rule(hip_lib):
    field_cases.rule(hip_lib)


def test_edges_of_the_walk(hip_lib):
    field_cases.edges(hip_lib)


def test_ranges(hip_lib):
    field_cases.ranges(hip_lib)


def test_close_the_loop(hip_lib):
    field_cases.close_the_loop(hip_lib)


def test_capacity(hip_lib):
    field_cases.capacity(hip_lib)


def test_errors(hip_lib):
    field_cases.errors(hip_lib)


def test_damaged_member(hip_lib):
    field_cases.damaged(hip_lib)


# ---------------------------------------------------------------------------------------------------- more than one wave of pieces
def _tsv(n, seed):
    """About n bytes: rows of 12 random decimal fields, every 500th row with 3,000 of them (about 20 KiB: its carry runs
    through a piece that holds no line delimiter)."""
    rng = np.random.default_rng(seed)
    rows, size, k = [], 0, 0
    while size < n:
        width = 3000 if k % 500 == 499 else 12
        row = b"\t".join(b"%d" % v for v in rng.integers(0, 10 ** 6, width).tolist()) + b"\n"
        rows.append(row)
        size += len(row)
        k += 1
    return rows


def test_tsv_8mib(hip_lib):
    """8 MiB of TSV in 64 KiB BGZF blocks, level 1, compressed on the device.  -f1-8, field 2,500 alone, everything and the
    complement of field 0; over all lines as one range and over 1,000 random ranges; both routes."""
    rows = _tsv(8 << 20, 20260111)
    plain = b"".join(rows)
    n, L = len(plain), len(rows)
    host = np.frombuffer(plain, dtype=np.uint8)
    d_in = torch.from_numpy(host.copy()).cuda()
    d_comp, comp_len = _device_compress(hip_lib, _native.FORMAT_BGZF, 1, 65280, d_in, n)
    rng = np.random.default_rng(5)
    begins = rng.integers(0, L, 1000)
    random_ranges = np.stack([begins, np.minimum(begins + rng.integers(0, 40, 1000), L)], axis=1).astype(np.uint64)
    range_sets = (np.array([[0, L]], dtype=np.uint64), random_ranges)
    cases = (([(0, 8)], False), ([(2500, 2501)], False), ([(0, END)], False), ([(0, 1)], True))
    want = []
    for fields, comp in cases:
        sel = field_cases.in_set(fields, comp)
        lines = [field_cases.cut_line(r, NL, TAB, sel) for r in rows]
        cum = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.int64)
        want.append((lines, cum))
    assert b"".join(want[2][0]) == plain and sum(1 for x in want[1][0] if len(x) > 1) == L // 500
    with _native.DContext(format=_native.FORMAT_BGZF, lib=hip_lib) as d, d.build_index_device(d_comp.data_ptr(), comp_len) as ix, \
            d.build_lines_device(ix, d_comp.data_ptr(), comp_len) as lt:
        assert (ix.inflated_len, lt.n_lines) == (n, L)
        for route in (_native.INFLATE_SEG, _native.INFLATE_WAVE):
            d.set_route(route)
            for (fields, comp), (lines, cum) in zip(cases, want):
                for rs in range_sets:
                    what = (route, fields, comp, rs.shape[0])
                    data = b"".join(b"".join(lines[a:b]) for a, b in rs.tolist())
                    offs = np.concatenate([[0], np.cumsum(cum[rs[:, 1].astype(np.int64)] - cum[rs[:, 0].astype(np.int64)])])
                    d_out = torch.full((len(data) + 64 + 3,), 0xEE, dtype=torch.uint8, device="cuda")
                    d_rs = torch.from_numpy(rs.astype(np.int64)).cuda()
                    d_offs = torch.full((rs.shape[0] + 1 + 4,), -2, dtype=torch.int64, device="cuda")
                    out_len = d.read_fields_table_device(ix, lt, d_comp.data_ptr(), comp_len, d_rs.data_ptr(), rs.shape[0], TAB, fields,
                                                         d_out.data_ptr() + 3, len(data), comp, d_offs.data_ptr())
                    assert out_len == len(data), what
                    assert d_out[3:].cpu().numpy().tobytes() == data + b"\xEE" * 64, what
                    got_offs = d_offs.cpu().numpy()
                    assert np.array_equal(got_offs[:rs.shape[0] + 1], offs) and bool(np.all(got_offs[rs.shape[0] + 1:] == -2)), what
                    ms = d.last_fields_ms()
                    assert all(t >= 0.0 for t in ms) and (ms[2] > 0.0 or not data), (what, ms)
