"""The steps of the single-workgroup scans on the MI355X: the shared bodies of tests/step_cases.py through the real
library with every place of the step's end against the long line, and the three scans whose step the CPU emulator cannot
reach, since their inputs are tens of MiB, or tens of millions of rows, that it would walk a thread at a time:
  - k_ln_prefix (gzpx_lines.h), kLnThreads * kLnScanItems = 1,024 tiles a step, and
  - k_fd_scan (gzpx_find.h), kFdThreads * kFdScanItems = 4,096 pieces of one batch a step, on one stream of 66 MiB;
  - the grid-stride sweep of k_wh_runs_count / k_wh_runs_write (gzpx_where.h) over more than kWhRunGrid groups of
    kSlRunRecords rows, on 34 million rows made of a repeated range.
Every size is derived from the kernels' constants (step_cases.K) and asserted to cross its step; every output checked
lies behind it.  The yardstick is numpy and the host's search on the host's copy of the text."""
import os
import re

import numpy as np
import pytest
import torch

import find_cases
import step_cases
from column_cases import INT, TAB
from gzp_amd import _native
from step_cases import FD_STEP, FL_STEP, LN_STEP, K
from test_gpu_ranges import _device_compress
from test_gpu_where import _runs
from where_cases import LT

pytestmark = pytest.mark.gpu

NL = 10


def test_piece_steps(hip_lib):
    ks = tuple(range(FL_STEP - 7, FL_STEP + 2)) + (2 * FL_STEP - 3,)
    step_cases.piece_steps(hip_lib, ks, table_ks=ks, host_ks=ks)  # (both forms of the three calls at every k)
    step_cases.piece_steps(hip_lib, ks[::3], table_ks=ks[::6], mgzip_ks=ks[::3], host_ks=ks[::3])


def test_member_steps(hip_lib):
    step_cases.member_steps(hip_lib)


# ---------------------------------------------------------------------------------------------------- d. 66 MiB of text
T, P, PAD = K["kLnTile"], K["kFdPiece"], K["kFdPad"]
M1, M2, M3 = b"QZWJK@!", b"^~`QZWJ", b"qu"  # (M2 ends with what M1 starts with: the two overlap at the step's end)
TILE_EDGES = (LN_STEP - 1, LN_STEP, 2 * LN_STEP, 3 * LN_STEP, 4 * LN_STEP)
_api = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gzp_amd", "csrc", "gzpx_api.cpp")).read()
_m = re.search(r"constexpr size_t kLinesBatchDefault = \(size_t\)(\d+) << (\d+);", _api)
BATCH_DEFAULT = int(_m.group(1)) << int(_m.group(2))  # inflated bytes a batch of the search holds at most


def _block(rng, n):
    """n bytes of lines of 8..100 bytes: lower-case letters and digits, a tab every few bytes."""
    a = rng.integers(0, 36, n).astype(np.uint8)
    a = np.where(a < 26, a + ord("a"), a - 26 + ord("0")).astype(np.uint8)
    tabs = np.cumsum(rng.integers(2, 12, n // 6))
    a[tabs[tabs < n]] = TAB
    nls = np.cumsum(rng.integers(8, 101, n // 50))
    a[nls[nls < n]] = NL
    a[-1] = NL
    return a


class Text:
    pass


def _host_text():
    """FD_STEP pieces and 2 MiB: a block of 1 MiB tiled, every copy with its number in its first line; M1 and M2 3,000
    times each in slots of 32 bytes of their own, and around byte E, the end of piece FD_STEP - 1 of the search's
    staging (a byte p of the stream lies at kFdPad + p there): M1 ending in front of the straddling M2, M2 across E, M1
    on the first byte of piece FD_STEP; M2 in the last piece.  Lines start 10 bytes in front of and 5 bytes behind the
    tile edges of TILE_EDGES.  With the host's newline index."""
    n = FD_STEP * P + (2 << 20)
    assert (60 << 20) <= n <= (80 << 20) and n % (1 << 20) == 0
    rng = np.random.default_rng(20260401)
    data = np.tile(_block(rng, 1 << 20), n >> 20)
    copies = np.arange(n >> 20)
    for i in range(4):
        data[(copies << 20) + i] = ord("0") + copies // 10 ** (3 - i) % 10
    E = FD_STEP * P - PAD
    taken = {E // 32 - 1, E // 32, (n - 1) // 32, (n - 1) // 32 - 1, 0} | {(b * T + d) // 32 for b in TILE_EDGES for d in (-11, 4)}
    taken |= set((copies << 15).tolist())
    slots = rng.choice(n // 32, 6100, replace=False)
    slots = np.array([x for x in slots.tolist() if x not in taken][:6000], dtype=np.int64)
    at = slots * 32 + rng.integers(0, 32 - len(M1) + 1, 6000)
    plant = {M1: sorted(at[:3000].tolist() + [E - 10, E]), M2: sorted(at[3000:].tolist() + [E - 3, n - 20])}
    for m in (M2, M1):  # (M1 behind M2: the four bytes they share at E are the same)
        for p in plant[m]:
            data[p:p + len(m)] = np.frombuffer(m, dtype=np.uint8)
    for b in TILE_EDGES:
        data[b * T - 11] = data[b * T + 4] = NL
    x = Text()
    x.n, x.E, x.data, x.plant = n, E, data, plant
    x.plain = data.tobytes()
    x.nl = np.flatnonzero(data == NL)
    x.L = int(x.nl.size)  # (the last byte is a delimiter)
    x.start = np.concatenate([[0], x.nl + 1]).astype(np.int64)
    assert data[-1] == NL and x.plain[E - 10:E + 7] == M1 + M2[:3] + M1
    return x


@pytest.fixture(scope="module")
def text(hip_lib):
    """_host_text() compressed on the device, BGZF level 1 in blocks of 65,280 bytes, with its index and line table."""
    x = _host_text()
    x.d_in = torch.from_numpy(x.data).cuda()
    x.d_comp, x.comp_len = _device_compress(hip_lib, _native.FORMAT_BGZF, 1, 65280, x.d_in, x.n)
    x.ptr = x.d_comp.data_ptr()
    with _native.DContext(format=_native.FORMAT_BGZF, lib=hip_lib) as d, d.build_index_device(x.ptr, x.comp_len) as ix, \
            d.build_lines_device(ix, x.ptr, x.comp_len) as lt:
        x.d, x.ix, x.lt = d, ix, lt
        yield x


def _sizes(x):
    """What every test on the stream asserts first: the stream is the host's, one batch holds it, and that batch has more
    pieces than a step of k_fd_scan and more tiles than four steps of k_ln_prefix."""
    assert (x.ix.inflated_len, x.lt.n_lines) == (x.n, x.L)
    x.d.set_lines_batch(0)
    assert x.n <= BATCH_DEFAULT, "one batch by default"
    assert (PAD + x.n + P - 1) // P - PAD // P > FD_STEP and -(-x.n // T) > 4 * LN_STEP


def _hits(x, pattern):
    hits = find_cases.host_hits(x.plain, pattern)
    return hits, np.searchsorted(x.nl, hits, side="left")


def test_lines_66mib(text):
    """k_ln_prefix across four of its steps of 1,024 tiles: the table's prefix P of 4,225 entries against the host's
    count of the delimiters of every tile; then read_lines_device, whose search reads P: 200 ranges of 1..50 lines at
    random places and ranges whose first or last line starts within 64 bytes of the tile edges 1,023 T, 1,024 T,
    2,048 T, 3,072 T and 4,096 T; bytes, out_offsets and byte_ranges against the host's slices."""
    x = text
    _sizes(x)
    tiles = -(-x.n // T)
    want_p = np.concatenate([[0], np.cumsum(np.bincount(x.nl // T, minlength=tiles))])
    assert np.array_equal(x.lt.prefix().astype(np.int64), want_p) and x.lt.n_delims == x.L
    assert all(want_p[b] < want_p[b + 1] for b in (LN_STEP, 4 * LN_STEP))
    rng = np.random.default_rng(8)
    begins = rng.integers(0, x.L - 50, 200)
    rs = np.stack([begins, begins + rng.integers(1, 51, 200)], axis=1).tolist()
    for b in TILE_EDGES:
        for at in (b * T - 10, b * T + 5):
            k = int(np.searchsorted(x.start, at))
            assert int(x.start[k]) == at and abs(at - b * T) <= 64
            rs += [[k, k + 3], [k - 5, k + 1], [k, k + 1]]
    rs = np.array(rs, dtype=np.uint64)
    want_br = np.stack([x.start[rs[:, 0].astype(np.int64)], x.start[rs[:, 1].astype(np.int64)]], axis=1)
    want = b"".join(x.plain[b:e] for b, e in want_br.tolist())
    for route in (_native.INFLATE_SEG, _native.INFLATE_WAVE):
        x.d.set_route(route)
        d_out = torch.full((len(want) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        out_len, offs, br = x.d.read_lines_device(x.ix, x.lt, x.ptr, x.comp_len, rs, d_out.data_ptr(), len(want))
        assert out_len == len(want), route
        assert np.array_equal(br.astype(np.int64), want_br), (route, "byte_ranges")
        assert np.array_equal(offs.astype(np.int64), np.concatenate([[0], np.cumsum(want_br[:, 1] - want_br[:, 0])])), (route, "out_offsets")
        assert d_out.cpu().numpy().tobytes() == want + b"\xEE" * 64, (route, "bytes")
    x.d.set_route(_native.INFLATE_SEG)


def _find(x, pattern, hits, lines, cap):
    """One writing call with `cap` entries and 4 more behind them: the first min(cap, hits) positions and lines, the
    count returned or raised as .needed."""
    d_pos = torch.full((cap + 4,), -2, dtype=torch.int64, device="cuda")
    d_lines = torch.full((cap + 4,), -2, dtype=torch.int64, device="cuda")
    try:
        got = x.d.find_device(x.ix, x.ptr, x.comp_len, pattern, NL, d_pos.data_ptr(), d_lines.data_ptr(), cap)
        assert hits.size <= cap
    except _native.GzpxError as e:
        assert e.code == _native.ERR_INSUFFICIENT_SPACE and hits.size > cap
        got = e.needed
    k = min(cap, hits.size)
    assert got == hits.size, (pattern, got, hits.size)
    assert np.array_equal(d_pos.cpu().numpy(), np.concatenate([hits[:k], [-2] * (cap + 4 - k)])), (pattern, "positions")
    assert np.array_equal(d_lines.cpu().numpy(), np.concatenate([lines[:k], [-2] * (cap + 4 - k)])), (pattern, "lines")


def test_find_66mib(text):
    """k_fd_scan across its step of 4,096 pieces in one batch: the hits and the delimiters in front of piece 4,096 and
    of every piece behind it are the first step's totals.  The two markers -- among their places one that ends in piece
    4,095, one across the step's end, one on the first byte of piece 4,096, one in the last piece -- with positions and
    lines against the host's search; a one-byte pattern counted, and written with room for 4,096 hits.  The markers again
    in two batches of 48 MiB, neither of which crosses the step: the same hits."""
    x = text
    _sizes(x)
    for m in (M1, M2):
        hits, lines = _hits(x, m)
        assert hits.tolist() == x.plant[m] and hits.size >= 3000
        at = (PAD + hits) // P  # the piece of staging a hit starts in
        assert int((at >= FD_STEP).sum()) >= 50 and (m == M1 or int(at.max()) == (PAD + x.n - 1) // P)
        assert x.d.find_device(x.ix, x.ptr, x.comp_len, m) == hits.size
        _find(x, m, hits, lines, hits.size)
    assert (PAD + x.E - 1) // P == FD_STEP - 1 and (PAD + x.E) // P == FD_STEP
    assert {x.E - 10, x.E} <= set(x.plant[M1]) and x.E - 3 in x.plant[M2]
    one = np.flatnonzero(x.data == ord("q"))
    assert one.size > 1 << 20
    assert x.d.find_device(x.ix, x.ptr, x.comp_len, b"q") == one.size
    assert x.d.find_device(x.ix, x.ptr, x.comp_len, b"q", NL) == one.size
    _find(x, b"q", one, np.searchsorted(x.nl, one, side="left"), FD_STEP)
    x.d.set_lines_batch(48 << 20)
    for m in (M1, M2):
        hits, lines = _hits(x, m)
        _find(x, m, hits, lines, hits.size)
    x.d.set_lines_batch(0)


def test_find_set_66mib(text):
    """k_fd_scan behind k_fs_count, across the same step: the two markers and "qu" as a set; positions, ids, lines and
    the counts of every pattern against the host's merge of its single searches."""
    x = text
    _sizes(x)
    patterns = [M1, M2, M3]
    per = [find_cases.host_hits(x.plain, p) for p in patterns]
    pos = np.concatenate(per)
    ids = np.concatenate([np.full(h.size, k, np.int64) for k, h in enumerate(per)])
    order = np.lexsort((ids, pos))
    pos, ids = pos[order], ids[order]
    lines = np.searchsorted(x.nl, pos, side="left")
    counts = np.array([h.size for h in per])
    assert int(counts.min()) >= 1000 and int(((PAD + pos) // P >= FD_STEP).sum()) >= 100
    k = pos.size
    d_counts = torch.full((len(patterns) + 4,), -2, dtype=torch.int64, device="cuda")
    assert x.d.find_set_device(x.ix, x.ptr, x.comp_len, patterns, d_counts_ptr=d_counts.data_ptr()) == k
    assert np.array_equal(d_counts.cpu().numpy(), np.concatenate([counts, [-2] * 4]))
    d_pos = torch.full((k + 4,), -2, dtype=torch.int64, device="cuda")
    d_ids = torch.full((k + 4,), -2, dtype=torch.int32, device="cuda")
    d_lines = torch.full((k + 4,), -2, dtype=torch.int64, device="cuda")
    assert x.d.find_set_device(x.ix, x.ptr, x.comp_len, patterns, NL, d_pos.data_ptr(), d_ids.data_ptr(), d_lines.data_ptr(), k) == k
    assert np.array_equal(d_pos.cpu().numpy(), np.concatenate([pos, [-2] * 4])), "positions"
    assert np.array_equal(d_ids.cpu().numpy(), np.concatenate([ids, [-2] * 4])), "ids"
    assert np.array_equal(d_lines.cpu().numpy(), np.concatenate([lines, [-2] * 4])), "lines"


def test_select_66mib(text):
    """The marking pass of select_lines_device reads k_fd_scan's bases for the line of every hit: M1 with records of one
    and of four lines, plain and inverted; runs and counts by select_cases.host_select's rule, in numpy."""
    x = text
    _sizes(x)
    hits, lines = _hits(x, M1)
    assert int(((PAD + hits) // P >= FD_STEP).sum()) >= 50
    for g in (1, 4):
        R = -(-x.L // g)
        for invert in (False, True):
            sel = np.zeros(R, dtype=bool)
            sel[np.unique(lines // g)] = True
            if invert:
                sel = ~sel
            edge = np.diff(np.concatenate([[0], sel.astype(np.int8), [0]]))
            runs = np.stack([g * np.flatnonzero(edge == 1), np.minimum(g * np.flatnonzero(edge == -1), x.L)], axis=1).astype(np.int64)
            k = runs.shape[0]
            assert k >= 2500
            want = (k, int(sel.sum()), hits.size)
            assert x.d.select_lines_device(x.ix, x.lt, x.ptr, x.comp_len, M1, g, invert) == want, (g, invert)
            d_runs = torch.full((k + 4, 2), -2, dtype=torch.int64, device="cuda")
            assert x.d.select_lines_device(x.ix, x.lt, x.ptr, x.comp_len, M1, g, invert, d_runs.data_ptr(), k) == want, (g, invert)
            table = d_runs.cpu().numpy()
            assert np.array_equal(table[:k], runs) and bool(np.all(table[k:] == -2)), (g, invert)


# ---------------------------------------------------------------------------------------------------- e. where's sweep
def _digits(L):
    """L digits: a fixed mixing hash of the line number, modulo 10.  (The offset 45 is the first for which the lines on
    both sides of row kWhRunGrid * kSlRunRecords of test_where_grid_stride are below 2: a run is open across that row.)"""
    x = (np.arange(L, dtype=np.uint64) + np.uint64(45)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    return (x % np.uint64(10)).astype(np.uint8)


def test_where_grid_stride(hip_lib):
    """k_wh_runs_count and k_wh_runs_write sweep the groups of kSlRunRecords rows with a stride of their grid, kWhRunGrid
    workgroups at most: 2,000,000 lines of one digit, all of them as one range 17 times, are 34 million rows -- more
    than kWhRunGrid groups, so that the first workgroups take a second group, and more than 4,096 pieces and 256 steps
    of k_wh_runs_scan besides.  The term is digit < 2; runs, counts and the entries behind n_runs against numpy, host
    form and table form, plain and inverted.  In the plain pass a run is open across row kWhRunGrid * kSlRunRecords, where
    the second sweep starts (asserted from the model); inverted, that row and the one in front of it are not selected,
    and the runs behind it still take their ranks from the groups of both sweeps."""
    W, G = K["kSlRunRecords"], K["kWhRunGrid"]
    L = 2_000_000
    n = (G * W + 2 * W) // L + 1
    R = n * L
    assert R > G * W + 2 * W and n <= 40 and R <= 0xFFFFFFF0
    v = _digits(L)
    data = np.empty((L, 2), dtype=np.uint8)
    data[:, 0] = v + ord("0")
    data[:, 1] = NL
    data = data.reshape(-1)
    ok = v < 2
    rs = np.array([[0, L]] * n, dtype=np.uint64)
    assert n * (data.size // K["kFlPiece"]) > FL_STEP
    line = G * W % L  # row G * W of the call
    assert bool(ok[line - 1] and ok[line]) and 0 < line, "a run is open across the sweep's first stride"
    d_in = torch.from_numpy(data).cuda()
    d_comp, comp_len = _device_compress(hip_lib, _native.FORMAT_BGZF, 1, 65280, d_in, data.size)
    d_rs = torch.from_numpy(rs.astype(np.int64)).cuda()
    terms = [(0, INT, LT, 2)]
    with _native.DContext(format=_native.FORMAT_BGZF, lib=hip_lib) as d, d.build_index_device(d_comp.data_ptr(), comp_len) as ix, \
            d.build_lines_device(ix, d_comp.data_ptr(), comp_len) as lt:
        assert (ix.inflated_len, lt.n_lines) == (data.size, L)
        for invert in (False, True):
            want = np.tile(_runs(rs[:1], ok != invert), (n, 1))  # (every range is the same lines: so are its runs)
            assert np.array_equal(want[:3 * (want.shape[0] // n)], _runs(rs[:3], ok != invert))
            selected = n * int((ok != invert).sum())
            assert want.shape[0] >= R // W
            cap = want.shape[0] + 3
            d_runs = torch.full((2 * cap + 8,), -2, dtype=torch.int64, device="cuda")
            for table in (False, True):
                d_runs.fill_(-2)
                if table:
                    got = d.where_lines_table_device(ix, lt, d_comp.data_ptr(), comp_len, d_rs.data_ptr(), n, TAB, terms, False, invert,
                                                     d_runs.data_ptr(), cap)
                else:
                    got = d.where_lines_device(ix, lt, d_comp.data_ptr(), comp_len, rs, TAB, terms, False, invert, d_runs.data_ptr(), cap)
                assert got == (want.shape[0], selected, R, 0), (invert, table, got, (want.shape[0], selected, R, 0))
                tb = d_runs.cpu().numpy()
                assert np.array_equal(tb[:2 * want.shape[0]].view(np.uint64).reshape(-1, 2), want), (invert, table, "runs")
                assert bool(np.all(tb[2 * want.shape[0]:] == -2)), (invert, table, "written behind n_runs")
