"""The selection of lines by the text of their fields on the MI355X: the shared bodies of tests/where_text_cases.py through
the real library, and test_gpu_where.py's TSV of 8 MiB with two text columns, compressed on the device -- more pieces than
one wave of workgroups, rows that run through many pieces, bitmap words that two workgroups set -- through both inflate
routes and both forms, runs and counts compared with numpy on the host's copy."""
import numpy as np
import pytest
import torch

import where_text_cases
from column_cases import FLT, INT, TAB
from gzp_amd import _native
from test_gpu_ranges import _device_compress
from test_gpu_where import _runs
from where_cases import EQ, GE, IS_OK, LT
from where_text_cases import NOT_PREFIX, PREFIX, TEXT

pytestmark = pytest.mark.gpu


def test_operators(hip_lib):
    where_text_cases.operators(hip_lib)


def test_edges_of_the_walk(hip_lib):
    where_text_cases.edges(hip_lib)


def test_mixed(hip_lib):
    where_text_cases.mixed(hip_lib)


def test_most_terms(hip_lib):
    where_text_cases.most(hip_lib)


def test_equivalence(hip_lib):
    where_text_cases.equivalence(hip_lib)


def test_close_the_loop(hip_lib):
    where_text_cases.close_the_loop(hip_lib)


def test_capacity(hip_lib):
    where_text_cases.capacity(hip_lib)


def test_errors(hip_lib):
    where_text_cases.errors(hip_lib)


def test_damaged_member(hip_lib):
    where_text_cases.damaged(hip_lib)


# ---------------------------------------------------------------------------------------------------- more than one wave of pieces
CONTIGS = (b"chr1", b"chr2", b"chr7", b"chr10", b"chr17", b"chrX", b"chrUn_KI270742v1")
FILTERS = (b"PASS", b"PASS;SB", b"q10", b"LowQual", b".", b"q10;PASS")
C_WEIGHTS = (0.08, 0.08, 0.52, 0.08, 0.08, 0.08, 0.08)  # about half of the rows lie on chr7 ...
F_WEIGHTS = (0.40, 0.12, 0.16, 0.16, 0.10, 0.06)        # ... about half begin their filter with PASS, and half are negative:
C_FIELD, X_FIELD, F_FIELD = 1, 3, 6                     # the three terms pass about 14 % of the rows under ALL, 89 % under ANY


def _tsv(n, seed):
    """test_gpu_where.py's recipe with two text columns.  About n bytes: rows of 12 fields, integers but for field 1, a
    contig's name, field 3, a float written with %.6g, and field 6, a filter; every 500th row has 3,000 fields, the same
    three among them.  Returns (rows, the contig's index, column 3, the filter's index, whether field 2500 exists)."""
    rng = np.random.default_rng(seed)
    rows, ci, c3, fi, wide, size, k = [], [], [], [], [], 0, 0
    while size < n:
        width = 3000 if k % 500 == 499 else 12
        parts = [b"%d" % v for v in rng.integers(-10 ** 6, 10 ** 6, width).tolist()]
        c, f = int(rng.choice(len(CONTIGS), p=C_WEIGHTS)), int(rng.choice(len(FILTERS), p=F_WEIGHTS))
        parts[C_FIELD], parts[F_FIELD] = CONTIGS[c], FILTERS[f]
        parts[X_FIELD] = b"%.6g" % float(b"%.6g" % (rng.normal() * 10.0 ** int(rng.integers(-4, 5))))
        row = b"\t".join(parts) + b"\n"
        rows.append(row)
        ci.append(c)
        c3.append(float(parts[X_FIELD]))
        fi.append(f)
        wide.append(width > 2500)
        size += len(row)
        k += 1
    return rows, np.array(ci), np.array(c3), np.array(fi), np.array(wide)


def test_tsv_8mib(hip_lib):
    """8 MiB of TSV in 64 KiB BGZF blocks, level 1, compressed on the device.  $2 == "chr7", $7 PREFIX "PASS" and $4 < 0
    under ALL and under ANY -- the truth of the text terms from Python's own comparison on the columns' vocabularies -- and
    a term on field 2500 beside a text term; all lines as one range and 1,000 random ranges; both routes, both forms;
    against numpy."""
    rows, ci, c3, fi, wide = _tsv(8 << 20, 20260111)
    plain = b"".join(rows)
    n, L = len(plain), len(rows)
    is_c = np.array([c == b"chr7" for c in CONTIGS])[ci]
    is_c_set = np.array([c >= b"chr17" for c in CONTIGS])[ci]
    is_f = np.array([f.startswith(b"PASS") for f in FILTERS])[fi]
    three = [(C_FIELD, TEXT, EQ, b"chr7"), (X_FIELD, FLT, LT, 0.0), (F_FIELD, TEXT, PREFIX, b"PASS")]
    loose = [(C_FIELD, TEXT, GE, b"chr17"), (X_FIELD, FLT, LT, 0.0), (F_FIELD, TEXT, NOT_PREFIX, b"PASS")]
    cases = [(three, False, is_c & (c3 < 0.0) & is_f), (three, True, is_c | (c3 < 0.0) | is_f),
             (loose, False, is_c_set & (c3 < 0.0) & ~is_f), ([(F_FIELD, TEXT, EQ, b"q10"), (2500, INT, IS_OK, 0)], True, wide | (np.array(FILTERS)[fi] == b"q10"))]
    for terms, any_, ok in cases[:3]:
        assert 0.1 * L < int(ok.sum()) < 0.9 * L, (terms, any_, int(ok.sum()), L)  # between 10 % and 90 % of the rows pass
    assert int(wide.sum()) == L // 500
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
                        not_ok = sum(int((~wide[a:b]).sum()) for a, b in rs.tolist()) if terms[-1][0] == 2500 else 0
                        cap = want.shape[0] + 3
                        d_runs = torch.full((2 * cap + 8,), -2, dtype=torch.int64, device="cuda")
                        for table in (False, True):
                            d_runs.fill_(-2)
                            if table:
                                got = d.where_text_table_device(ix, lt, d_comp.data_ptr(), comp_len, d_rs.data_ptr(), rs.shape[0], TAB,
                                                                terms, any_, invert, d_runs.data_ptr(), cap)
                            else:
                                got = d.where_text_device(ix, lt, d_comp.data_ptr(), comp_len, rs, TAB, terms, any_, invert,
                                                          d_runs.data_ptr(), cap)
                            assert got == (want.shape[0], selected, R, not_ok), (what, table, got, (want.shape[0], selected, R, not_ok))
                            tb = d_runs.cpu().numpy()
                            assert np.array_equal(tb[:2 * want.shape[0]].view(np.uint64).reshape(-1, 2), want), (what, table)
                            assert bool(np.all(tb[2 * want.shape[0]:] == -2)), (what, table, "written behind n_runs")
                            ms = d.last_where_ms()
                            assert all(t > 0.0 for t in ms), (what, table, ms)
