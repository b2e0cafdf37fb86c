"""The selection of lines by their numbers on the MI355X: the shared bodies of tests/where_cases.py through the real
library, and test_gpu_columns.py's TSV of 8 MiB compressed on the device -- more pieces than one wave of workgroups,
rows that run through many pieces, bitmap words that two workgroups set -- through both inflate routes, runs and counts
compared with numpy on the host's copy."""
import numpy as np
import pytest
import torch

import where_cases
from column_cases import FLT, INT, TAB
from gzp_amd import _native
from test_gpu_ranges import _device_compress
from where_cases import GE, IS_OK, LT, NE

pytestmark = pytest.mark.gpu


def test_operators(hip_lib):
    where_cases.operators(hip_lib)


def test_most_terms(hip_lib):
    where_cases.most_terms(hip_lib)


def test_edges_of_the_walk(hip_lib):
    where_cases.edges(hip_lib)


def test_runs(hip_lib):
    where_cases.runs(hip_lib)


def test_scan_step(hip_lib):
    where_cases.scan_step(hip_lib)


def test_capacity(hip_lib):
    where_cases.capacity(hip_lib)


def test_errors(hip_lib):
    where_cases.errors(hip_lib)


def test_damaged_member(hip_lib):
    where_cases.damaged(hip_lib)


def test_close_the_loop(hip_lib):
    where_cases.close_the_loop(hip_lib)


# ---------------------------------------------------------------------------------------------------- more than one wave of pieces
def _tsv(n, seed):
    """test_gpu_columns.py's recipe.  About n bytes: rows of 12 fields, integers but for field 3, a float written with
    %.6g; every 500th row has 3,000 integer fields.  Returns (rows, column 0, column 3, column 11, whether field 2500
    exists)."""
    rng = np.random.default_rng(seed)
    rows, c0, c3, c11, wide, size, k = [], [], [], [], [], 0, 0
    while size < n:
        width = 3000 if k % 500 == 499 else 12
        ints = rng.integers(-10 ** 6, 10 ** 6, width).tolist()
        x = float(b"%.6g" % (rng.normal() * 10.0 ** int(rng.integers(-4, 5))))
        parts = [b"%d" % v for v in ints]
        parts[3] = b"%.6g" % x
        row = b"\t".join(parts) + b"\n"
        rows.append(row)
        c0.append(ints[0])
        c3.append(float(parts[3]))
        c11.append(ints[11])
        wide.append(width > 2500)
        size += len(row)
        k += 1
    return rows, np.array(c0), np.array(c3), np.array(c11), np.array(wide)


def _runs(rs, ok):
    """The runs of the selected lines `ok` inside every range by itself, as line ranges in row order."""
    out = []
    for a, b in rs.tolist():
        edge = np.diff(np.concatenate([[0], ok[a:b].astype(np.int8), [0]]))
        out += [(a + int(i0), a + int(i1)) for i0, i1 in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1))]
    return np.array(out, dtype=np.uint64).reshape(-1, 2)


def test_tsv_8mib(hip_lib):
    """8 MiB of TSV in 64 KiB BGZF blocks, level 1, compressed on the device.  c0 >= 0, c3 < 1.5 and c11 != 7 under ALL and
    under ANY, and field 2500 IS_OK; all lines as one range and 1,000 random ranges; both routes; against numpy."""
    rows, c0, c3, c11, wide = _tsv(8 << 20, 20260111)
    plain = b"".join(rows)
    n, L = len(plain), len(rows)
    three = [(0, INT, GE, 0), (3, FLT, LT, 1.5), (11, INT, NE, 7)]
    truths = [c0 >= 0, c3 < 1.5, c11 != 7]  # (every cell of the three columns is OK: test_gpu_columns.py checks the model on them)
    cases = [(three, False, np.all(truths, axis=0)), (three, True, np.any(truths, axis=0)), ([(2500, INT, IS_OK, 0)], False, wide)]
    assert 0.1 * L < int(cases[0][2].sum()) < 0.9 * L and int(wide.sum()) == L // 500
    d_in = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
    d_comp, comp_len = _device_compress(hip_lib, _native.FORMAT_BGZF, 1, 65280, d_in, n)
    rng = np.random.default_rng(5)
    begins = rng.integers(0, L, 1000)
    random_ranges = np.stack([begins, np.minimum(begins + rng.integers(0, 40, 1000), L)], axis=1).astype(np.uint64)
    with _native.DContext(format=_native.FORMAT_BGZF, lib=hip_lib) as d, d.build_index_device(d_comp.data_ptr(), comp_len) as ix, \
            d.build_lines_device(ix, d_comp.data_ptr(), comp_len) as lt:
        assert (ix.inflated_len, lt.n_lines) == (n, L)
        for route in (_native.INFLATE_SEG, _native.INFLATE_WAVE):
            d.set_route(route)
            for rs in (np.array([[0, L]], dtype=np.uint64), random_ranges):
                R = int((rs[:, 1] - rs[:, 0]).sum())
                d_rs = torch.from_numpy(rs.astype(np.int64)).cuda()
                for terms, any_, ok in cases:
                    for invert in (False, True):
                        what = (route, rs.shape[0], terms, any_, invert)
                        want = _runs(rs, ok != invert)
                        selected = sum(int((ok[a:b] != invert).sum()) for a, b in rs.tolist())
                        not_ok = sum(int((~wide[a:b]).sum()) for a, b in rs.tolist()) if terms[0][0] == 2500 else 0
                        cap = want.shape[0] + 3
                        d_runs = torch.full((2 * cap + 8,), -2, dtype=torch.int64, device="cuda")
                        for table in (False, True):
                            d_runs.fill_(-2)
                            if table:
                                got = d.where_lines_table_device(ix, lt, d_comp.data_ptr(), comp_len, d_rs.data_ptr(), rs.shape[0], TAB,
                                                                 terms, any_, invert, d_runs.data_ptr(), cap)
                            else:
                                got = d.where_lines_device(ix, lt, d_comp.data_ptr(), comp_len, rs, TAB, terms, any_, invert,
                                                           d_runs.data_ptr(), cap)
                            assert got == (want.shape[0], selected, R, not_ok), (what, table, got, (want.shape[0], selected, R, not_ok))
                            tb = d_runs.cpu().numpy()
                            assert np.array_equal(tb[:2 * want.shape[0]].view(np.uint64).reshape(-1, 2), want), (what, table)
                            assert bool(np.all(tb[2 * want.shape[0]:] == -2)), (what, table, "written behind n_runs")
                            ms = d.last_where_ms()
                            assert all(t > 0.0 for t in ms), (what, table, ms)
