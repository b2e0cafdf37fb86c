"""The numeric columns of lines on the MI355X: the shared bodies of tests/column_cases.py through the real library, and a
TSV of 8 MiB compressed on the device -- more pieces than one wave of workgroups, rows that run through many pieces --
read through both inflate routes and compared with numpy's conversion of the host's copy."""
import numpy as np
import pytest
import torch

import column_cases
from column_cases import FLT, INT, OK, MISSING, NAN, TAB
from gzp_amd import _native
from test_gpu_ranges import _device_compress

pytestmark = pytest.mark.gpu


def test_grammar(hip_lib):
    column_cases.grammar(hip_lib)


def test_edges_of_the_walk(hip_lib):
    column_cases.edges(hip_lib)


def test_ranges(hip_lib):
    column_cases.ranges(hip_lib)


def test_capacity(hip_lib):
    column_cases.capacity(hip_lib)


def test_errors(hip_lib):
    column_cases.errors(hip_lib)


def test_damaged_member(hip_lib):
    column_cases.damaged(hip_lib)


def test_close_the_loop(hip_lib):
    column_cases.close_the_loop(hip_lib)


# ---------------------------------------------------------------------------------------------------- more than one wave of pieces
def _tsv(n, seed):
    """About n bytes: rows of 12 fields, integers but for field 3, a float written with %.6g; every 500th row has 3,000
    integer fields.  Returns (rows, column 0, column 3 as float64, column 11, column 2500 where it exists)."""
    rng = np.random.default_rng(seed)
    rows, c0, c3, c11, c2500, size, k = [], [], [], [], [], 0, 0
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
        c2500.append(ints[2500] if width > 2500 else None)
        size += len(row)
        k += 1
    return rows, c0, c3, c11, c2500


def test_tsv_8mib(hip_lib):
    """8 MiB of TSV in 64 KiB BGZF blocks, level 1, compressed on the device.  Columns {0: int, 3: float, 11: int, 2500:
    int}; all lines as one range and 1,000 random ranges; both routes; against numpy."""
    rows, c0, c3, c11, c2500 = _tsv(8 << 20, 20260111)
    plain = b"".join(rows)
    n, L = len(plain), len(rows)
    # the model alone: no cell of this input is outside the exact range
    assert all(column_cases.model(r.split(b"\t")[3], FLT)[0] == OK for r in rows[::97])
    assert all(column_cases.model(b"%.6g" % v, FLT) == (OK, column_cases.bits_of(v)) for v in c3)
    cols = [(0, INT), (3, FLT), (11, INT), (2500, INT)]
    val = np.stack([np.array(c0, dtype=np.int64).view(np.uint64), np.array(c3, dtype=np.float64).view(np.uint64),
                    np.array(c11, dtype=np.int64).view(np.uint64),
                    np.array([0 if v is None else v for v in c2500], dtype=np.int64).view(np.uint64)])
    st = np.zeros((4, L), dtype=np.uint8)
    st[3] = [MISSING if v is None else OK for v in c2500]
    assert int((st[3] == OK).sum()) == L // 500 and NAN not in val[1].tolist()
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
                what = (route, rs.shape[0])
                idx = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in rs.tolist()])
                R = idx.size
                offs = np.concatenate([[0], np.cumsum(rs[:, 1].astype(np.int64) - rs[:, 0].astype(np.int64))])
                cap = R + 5
                d_val = torch.full((4 * cap + 8 + 3,), -1229782938247303442, dtype=torch.int64, device="cuda")  # 0xEE..EE
                d_st = torch.full((4 * cap + 64 + 3,), 0xEE, dtype=torch.uint8, device="cuda")
                d_rs = torch.from_numpy(rs.astype(np.int64)).cuda()
                d_offs = torch.full((rs.shape[0] + 1 + 4,), -2, dtype=torch.int64, device="cuda")
                d_bad = torch.full((4 + 4,), -2, dtype=torch.int64, device="cuda")
                n_rows, n_bad, _ = d.read_columns_table_device(ix, lt, d_comp.data_ptr(), comp_len, d_rs.data_ptr(), rs.shape[0], TAB, cols,
                                                               d_val.data_ptr() + 24, d_st.data_ptr() + 3, cap, d_bad.data_ptr(),
                                                               d_offs.data_ptr())
                assert n_rows == R and n_bad == int((st[:, idx] != OK).sum()), what
                got = d_val[3:3 + 4 * cap].cpu().numpy().view(np.uint64).reshape(4, cap)
                want_val = val[:, idx].copy()
                want_val[3][st[3, idx] != OK] = 0
                assert np.array_equal(got[:, :R], want_val) and bool(np.all(got[:, R:] == column_cases.UNTOUCHED)), what
                assert bool(np.all(d_val[3 + 4 * cap:].cpu().numpy() == -1229782938247303442)) and bool(np.all(d_val[:3].cpu().numpy() == -1229782938247303442)), what
                got_st = d_st[3:].cpu().numpy()
                assert np.array_equal(got_st[:4 * cap].reshape(4, cap)[:, :R], st[:, idx]), what
                assert bool(np.all(got_st[:4 * cap].reshape(4, cap)[:, R:] == 0xEE)) and bool(np.all(got_st[4 * cap:] == 0xEE)), what
                got_offs = d_offs.cpu().numpy()
                assert np.array_equal(got_offs[:rs.shape[0] + 1], offs) and bool(np.all(got_offs[rs.shape[0] + 1:] == -2)), what
                got_bad = d_bad.cpu().numpy()
                assert got_bad[:4].tolist() == (st[:, idx] != OK).sum(axis=1).tolist() and bool(np.all(got_bad[4:] == -2)), what
                ms = d.last_columns_ms()
                assert all(t > 0.0 for t in ms), (what, ms)
