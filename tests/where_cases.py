"""Selection of lines by their numbers (gzpx_where_lines_device, gzpx_where_lines_table_device), written once and run
twice: through the emulated library on CPU (tests/test_emu_where.py) and through the real HIP library on the MI355X
(tests/test_gpu_where.py).

The yardstick is never the library.  It is range_cases.Plain (zlib's inflate of every member, joined), the lines that
line_cases.Lines cuts, the cells of column_cases.Want (the Python model of the two grammars), the truth of a term by
include/gzpx.h's rules with numpy's integer and IEEE comparisons, and numpy's edge detection on the selected rows of
every range by itself.  Every comparison is exact.  The run table is pre-filled with 0xEE and has GUARD entries behind
runs_cap; entries behind n_runs and behind runs_cap must still be 0xEE.

Not covered: GZPX_ERR_INVALID_ARG for more than 0xFFFFFFF0 rows, which takes a stream of more than 2^32 lines."""
import ctypes
import struct

import numpy as np
import pytest

import column_cases
from column_cases import FLT, HAND, INT, OK, MISSING, EMPTY, INVALID, RANGE, NL, TAB, Want, edge_text, number_text
from field_cases import put_ranges
from gzp_amd import _native
from line_cases import Lines, Opened, cut
from range_cases import Plain, ROUTES
from scan_cases import BGZF, MGZIP, HDR, Mem
from select_cases import RUN_RECORDS, SCAN_STEP

GUARD = 4    # entries behind runs_cap that must stay as they were
FILL = 0xEE
UNTOUCHED = int.from_bytes(bytes([FILL]) * 8, "little")
FORMATS = (BGZF, MGZIP)
LT, LE, EQ, NE, GE, GT, IS_OK, NOT_OK = (_native.WHERE_LT, _native.WHERE_LE, _native.WHERE_EQ, _native.WHERE_NE, _native.WHERE_GE,
                                         _native.WHERE_GT, _native.WHERE_IS_OK, _native.WHERE_NOT_OK)
OPS = (LT, LE, EQ, NE, GE, GT, IS_OK, NOT_OK)
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


# ------------------------------------------------------------------------------------------------ the model
def columns_of(terms):
    """The distinct fields of the terms as a column list, ascending."""
    cols = []
    for field, kind, _, _ in terms:
        if not cols or cols[-1][0] != field:
            cols.append((field, kind))
    return cols


def term_truth(kind, op, value, st, val):
    """The truth of one term on arrays of cells (status bytes, 64-bit patterns)."""
    ok = st == OK
    if op == IS_OK:
        return ok
    if op == NOT_OK:
        return ~ok
    if kind == INT:
        x, v = val.view(np.int64), np.int64(value)
    else:
        x, v = val.view(np.float64), np.float64(value)
    with np.errstate(invalid="ignore"):
        cmp = {LT: x < v, LE: x <= v, EQ: x == v, NE: x != v, GE: x >= v, GT: x > v}[op]
    return ok & cmp  # (a comparison on a cell that is not OK is false, NE included)


_wants = {}


def want_of(ln, delim, fd, cols):
    key = (id(ln), delim, fd, tuple(cols))
    if key not in _wants:
        _wants[key] = (ln, Want(ln, delim, fd, cols))  # (ln kept: its id stays its own)
    return _wants[key][1]


def passes(ln, delim, fd, terms, any_):
    """bool[L]: the lines that pass, and the status bytes of the distinct fields."""
    cols = columns_of(terms)
    want = want_of(ln, delim, fd, cols)
    at = {f: c for c, (f, _) in enumerate(cols)}
    truths = [term_truth(kind, op, value, want.st[at[field]], np.ascontiguousarray(want.val[at[field]]))
              for field, kind, op, value in terms]
    return (np.any(truths, axis=0) if any_ else np.all(truths, axis=0)), want.st


def model(ln, delim, fd, ranges, terms, any_=False, invert=False):
    """(runs as line ranges in row order, selected rows, rows, cells that are not OK) by the rules of include/gzpx.h."""
    ok, st = passes(ln, delim, fd, terms, any_)
    runs, selected, rows, not_ok = [], 0, 0, 0
    for a, b in ranges:
        if a >= b:
            continue
        sel = ok[a:b] != invert
        edge = np.diff(np.concatenate([[0], sel.astype(np.int8), [0]]))
        runs += [(a + int(i0), a + int(i1)) for i0, i1 in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1))]
        selected += int(sel.sum())
        rows += b - a
        not_ok += int((st[:, a:b] != OK).sum())
    assert len(runs) <= (rows + len(ranges)) // 2
    return runs, selected, rows, not_ok


# ------------------------------------------------------------------------------------------------ the calls
def where(mem, o, ranges, fd, terms, any_=False, invert=False, cap=None, table=False):
    """One call.  cap None: count only.  Otherwise a table of `cap` entries and GUARD more behind them:
    ((n_runs, n_selected, n_rows, n_not_ok) or the GzpxError raised, the cap + GUARD entries as [begin, end] rows)."""
    n = len(ranges)
    keep, p, room = None, None, 0
    if cap is not None:
        room = (cap + GUARD) * 16
        keep, p = mem.put(bytes([FILL]) * room)
    try:
        if table:
            kr, rp = put_ranges(mem, ranges)
            got = o.d.where_lines_table_device(o.ix, o.lt, o.ptr, o.n, rp, n, fd, terms, any_, invert, p, cap or 0)
            if n:
                assert mem.get(kr, 16 * n) == np.array(ranges, dtype=np.uint64).tobytes(), "the range table was written"
        else:
            got = o.d.where_lines_device(o.ix, o.lt, o.ptr, o.n, ranges, fd, terms, any_, invert, p, cap or 0)
    except _native.GzpxError as e:
        got = e
    return got, (np.frombuffer(mem.get(keep, room), dtype=np.uint64).reshape(-1, 2).tolist() if cap is not None else None)


def check(mem, o, ln, ranges, fd, terms, any_, invert, what, table=False, count=False, delim=NL):
    """The runs into a table of exactly n_runs entries (count: the count-only call in front of it)."""
    runs, selected, rows, not_ok = model(ln, delim, fd, ranges, terms, any_, invert)
    if count:
        got, _ = where(mem, o, ranges, fd, terms, any_, invert, None, table)
        assert got == (len(runs), selected, rows, not_ok), (what, "count only", got, (len(runs), selected, rows, not_ok))
    got, tb = where(mem, o, ranges, fd, terms, any_, invert, len(runs), table)
    assert got == (len(runs), selected, rows, not_ok), (what, "counts", got, (len(runs), selected, rows, not_ok))
    wrong = [i for i, r in enumerate(runs) if tb[i] != list(r)]
    assert not wrong, (what, "runs", wrong[:5], tb[wrong[0]], runs[wrong[0]])
    assert tb[len(runs):] == [[UNTOUCHED, UNTOUCHED]] * GUARD, (what, "written behind runs_cap")
    ms = o.d.last_where_ms()
    assert all(t >= 0.0 for t in ms), (what, ms)
    return runs


# ------------------------------------------------------------------------------------------------ 1. operators
OP_FIELDS = [f for f in HAND if len(f) < 40] + [b"", b"nan", b"-nan", b"inf", b"-inf", b"-0.0", b"0.0", b"0", b"-0", b"1.5",
                                                      b"9223372036854775807", b"-9223372036854775808", b"42", b"1e22", b"0.1"]
INT_CONSTANTS = (0, 1, -1, 42, I64_MIN, I64_MAX, 123456789)
FLT_CONSTANTS = (0.0, -0.0, 1.5, float("inf"), float("-inf"), 1e22, 0.1, -2.5)


def operators(lib):
    """Column 1 holds hand-written fields of every status, field 3 does not exist.  Every op x both types x constants
    that equal cells, as a single term; then ALL and ANY with and without INVERT on sets of terms, two terms on one
    field among them."""
    mem = Mem(lib)
    text = b"".join(b"%d\t%s\t%d\n" % (i, f, i % 7) for i, f in enumerate(OP_FIELDS))
    for fmt in FORMATS:
        s = cut(fmt, text, [len(text) // 2])
        ln = Lines(Plain(fmt, s), NL)
        whole = [(0, ln.L)]
        with Opened(lib, mem, fmt, s, route=ROUTES[fmt == MGZIP]) as o:
            for kind, constants in ((INT, INT_CONSTANTS), (FLT, FLT_CONSTANTS)):
                st = want_of(ln, NL, TAB, [(1, kind)]).st[0]
                assert set(st.tolist()) == {OK, EMPTY, INVALID, RANGE}, (kind, set(st.tolist()))
                if (kind == INT) == (fmt == BGZF):  # (every op and constant: one type per format, to keep the emulator's run short)
                    for op in OPS:
                        for v in (constants if op < IS_OK else (0,)):
                            check(mem, o, ln, whole, TAB, [(1, kind, op, v)], False, False, ("one term", fmt, kind, op, v))
                # a comparison on a cell that is not OK is false, NE too; the status ops see it
                bad = np.flatnonzero(st != OK)
                for op in (LT, LE, EQ, NE, GE, GT):
                    ok, _ = passes(ln, NL, TAB, [(1, kind, op, 1)], False)
                    assert not ok[bad].any()
                # MISSING: from the lane that closes the line
                assert check(mem, o, ln, whole, TAB, [(3, kind, NOT_OK, 0)], False, False, ("missing", fmt, kind)) == [(0, ln.L)]
                assert check(mem, o, ln, whole, TAB, [(3, kind, NE, 5)], False, False, ("missing NE", fmt, kind)) == []
                pair = [(1, kind, GE, -1), (1, kind, LT, 100)]
                sets = [pair, [(0, INT, GE, 20), (1, kind, NE, 42), (2, INT, LE, 3)], [(1, kind, IS_OK, 0), (3, INT, IS_OK, 0)],
                        [(0, INT, LT, 30), (1, kind, NOT_OK, 0), (1, kind, EQ, 0), (3, FLT, EQ, 1.0)]]
                for terms in sets:
                    for any_ in (False, True):
                        for invert in (False, True):
                            check(mem, o, ln, whole, TAB, terms, any_, invert, ("sets", fmt, kind, terms, any_, invert), count=not any_)
            if fmt == BGZF:
                special(mem, o, ln)


def special(mem, o, ln):
    """-0.0 against 0.0, the cell "nan", the infinities, the ends of int64, and constants that equal their cells."""
    cells = [f for f in OP_FIELDS]
    whole = [(0, ln.L)]

    def lines_of(terms):
        return {k for a, b in check(mem, o, ln, whole, TAB, terms, False, False, ("special", terms)) for k in range(a, b)}

    def holding(*fields):
        return {k for k, f in enumerate(cells) if f in fields}

    zeros = {k for k, f in enumerate(cells) if column_cases.model(f, FLT)[0] == OK and float(f) == 0.0}
    assert holding(b"-0.0", b"0.0", b"0", b"-0") <= zeros
    assert lines_of([(1, FLT, EQ, -0.0)]) == zeros and lines_of([(1, FLT, EQ, 0.0)]) == zeros
    nans = {k for k, f in enumerate(cells) if column_cases.model(f, FLT) == (OK, column_cases.NAN)}
    assert holding(b"nan", b"-nan") <= nans
    for op in (LT, LE, EQ, GE, GT):
        assert not lines_of([(1, FLT, op, 0.0)]) & nans
    oks = {k for k, f in enumerate(cells) if column_cases.model(f, FLT)[0] == OK}
    assert nans <= lines_of([(1, FLT, NE, 0.0)]) == oks - zeros
    assert holding(b"inf", b"+inf", b"INF", b"Inf", b"Infinity", b"+INFINITY") == lines_of([(1, FLT, EQ, float("inf"))]) != set()
    assert lines_of([(1, FLT, LE, float("-inf"))]) == holding(b"-inf", b"-infinity") != set()
    assert lines_of([(1, FLT, LT, float("inf"))]) == oks - nans - lines_of([(1, FLT, EQ, float("inf"))])
    assert lines_of([(1, INT, LE, I64_MIN)]) == holding(b"-9223372036854775808", b"-" + b"0" * 30 + b"9223372036854775808") != set()
    assert lines_of([(1, INT, LT, I64_MIN)]) == set()
    top = lines_of([(1, INT, GE, I64_MAX)])
    assert top == lines_of([(1, INT, EQ, I64_MAX)]) >= holding(b"9223372036854775807", b"+9223372036854775807") and top
    assert lines_of([(1, INT, GT, I64_MAX)]) == set()
    assert lines_of([(1, INT, EQ, 42)]) == holding(b"42") and lines_of([(1, FLT, EQ, 1.5)]) == holding(b"1.5")


def most_terms(lib):
    """32 terms on 16 distinct fields of lines of 20 numbers, two a field; ALL and ANY, with and without INVERT."""
    mem = Mem(lib)
    rng = np.random.default_rng(77)
    rows = rng.integers(0, 100, (600, 20))
    text = b"".join(b"\t".join((b"%d" if j % 2 else b"%d.5") % v for j, v in enumerate(r)) + b"\n" for r in rows)
    text = text.replace(b"\t17\t", b"\t\t", 3)
    s = cut(BGZF, text, [20000])
    ln = Lines(Plain(BGZF, s), NL)
    terms = []
    for f in range(2, 18):
        kind = INT if f % 2 else FLT
        terms += [(f, kind, GE, 3 if kind == INT else 2.5), (f, kind, LT, 97 if kind == INT else 98.0)]
    assert len(terms) == _native.WHERE_MAX_TERMS and len(columns_of(terms)) == _native.COLUMNS_MAX
    with Opened(lib, mem, BGZF, s) as o:
        for any_ in (False, True):
            for invert in (False, True):
                runs = check(mem, o, ln, [(0, ln.L), (100, 300)], TAB, terms, any_, invert, ("32 terms", any_, invert), table=invert)
                assert any_ or invert or len(runs) > 20
        rare = [(f, k, EQ if op == GE else NE, v) for f, k, op, v in terms]  # ANY: one of 16 equalities, or any inequality
        check(mem, o, ln, [(0, ln.L)], TAB, rare[::2], True, False, "16 equalities")


# ------------------------------------------------------------------------------------------------ 2. the edges of the walk
EDGE_TERMS = (([(0, INT, LT, 50), (2, FLT, GE, 5.0)], False),  # a term column in front of a piece's edge and one behind it
              ([(2500, INT, IS_OK, 0)], False), ([(1, FLT, GT, 5000.0), (2500, INT, GE, 0)], True),
              ([(0, INT, NE, 77), (1, FLT, NOT_OK, 0), (2, FLT, LT, 9.5)], True), ([(2, FLT, NOT_OK, 0)], False))


def edges(lib):
    """column_cases.edge_text: rows that run through a piece's edge with term columns on both sides of it, fields opened by
    a piece's last byte, an unterminated last line, a line of 3,000 fields with a term on field 2500, lines with too few
    fields, ranges that start at every one of the first lines."""
    mem = Mem(lib)
    for i, prefix in enumerate((0, 5, 10, 15, 22, 31)):
        fmt, route = FORMATS[i % 2], ROUTES[(i // 2) % 2]
        text = edge_text(prefix, terminated=prefix % 3 != 1, long_line=prefix % 5 == 0)
        s = cut(fmt, text, [] if fmt == MGZIP else [20000, 40000])
        ln = Lines(Plain(fmt, s), NL)
        with Opened(lib, mem, fmt, s, NL, route, shift=prefix % 16) as o:
            first = 1 if prefix else 0
            sets = [[(0, ln.L)], [(first, ln.L)]] + ([[(k, ln.L) for k in range(1, 6)], [(ln.L - 1, ln.L)]] if prefix < 6 else [])
            for j, rs in enumerate(sets):
                for terms, any_ in EDGE_TERMS:
                    if prefix % 5 and terms[-1][0] == 2500 and not any_:
                        continue  # (no line has the field: covered by `missing` above)
                    check(mem, o, ln, rs, TAB, terms, any_, bool((i + j) % 2), ("edges", prefix, fmt, route, rs[:2], terms), table=j % 2 == 1)
    text = edge_text(13, 0x00, 0xFF, False)  # both delimiters as bytes that text does not hold
    s = cut(BGZF, text, [30000])
    ln = Lines(Plain(BGZF, s), 0xFF)
    with Opened(lib, mem, BGZF, s, 0xFF) as o:
        for terms, any_ in EDGE_TERMS:
            check(mem, o, ln, [(0, ln.L), (3, 9)], 0x00, terms, any_, False, ("edges, binary delimiters", terms), delim=0xFF)


# ------------------------------------------------------------------------------------------------ 3. runs
RUN_ROWS = (1, 7, 8, 9, 511, 512, 513, 1025)
ALL_F, NONE_F, ALT_F, CROSS_F, ODD_F = range(5)  # the fields of run_text


def run_text(R):
    """R lines of five 0/1 fields: all, none, alternating from row 0, rows [500, 520), alternating from row 1."""
    return b"".join(b"1\t0\t%d\t%d\t%d\n" % (1 - k % 2, 500 <= k < 520, k % 2) for k in range(R))


def runs(lib):
    mem = Mem(lib)
    for i, R in enumerate(RUN_ROWS):
        fmt, route = FORMATS[i % 2], ROUTES[(i // 2) % 2]
        text = run_text(R)
        s = cut(fmt, text, [len(text) // 3])
        ln = Lines(Plain(fmt, s), NL)
        assert ln.L == R
        with Opened(lib, mem, fmt, s, NL, route) as o:
            whole = [(0, R)]
            for f in (ALL_F, NONE_F, ALT_F, CROSS_F):
                for invert in (False, True):
                    got = check(mem, o, ln, whole, TAB, [(f, INT, EQ, 1)], False, invert, ("runs", R, f, invert), table=invert, count=f == ALT_F)
                    if f == ALT_F and not invert:
                        assert len(got) == (R + 1) // 2  # the bound, met exactly
                    if f == CROSS_F and not invert and R >= 520:
                        assert got == [(500, 520)]
            if R < 1025:
                continue
            sets = {"adjacent": [(0, 5), (5, 9)], "overlapping": [(0, 10), (5, 15)], "repeated": [(3, 9), (3, 9)],
                    "empty between": [(0, 4), (7, 7), (4, 8), (9, 9), (9, 9), (8, 12)], "at a byte": [(0, 8), (8, 20)],
                    "at 512 rows": [(0, 512), (512, 1025)], "at 512 rows, shifted": [(1, 513), (513, 1025), (0, 1025)],
                    "at 511 rows": [(500, 1011), (400, 600)], "descending": [(600, 1025), (300, 600), (0, 300)],
                    "single lines": [(k, k + 1) for k in range(100, 140)], "odd lines": [(k, k + 1) for k in range(1, 99, 2)]}
            assert model(ln, NL, TAB, sets["adjacent"], [(ALL_F, INT, EQ, 1)])[0] == [(0, 5), (5, 9)]  # two runs, not one
            for name, rs in sets.items():
                for f in (ALL_F, ALT_F, CROSS_F, ODD_F):
                    for table in (False, True):
                        got = check(mem, o, ln, rs, TAB, [(f, INT, EQ, 1)], False, False, ("runs", name, f, table), table=table)
                        if f == ALL_F:
                            assert got == [r for r in rs if r[0] < r[1]]
                check(mem, o, ln, rs, TAB, [(ALT_F, INT, EQ, 1), (CROSS_F, INT, EQ, 1)], True, True, ("runs", name, "ANY, INVERT"))
            # the bound with several ranges: n ranges of one row each, every row selected -- (R + n) / 2 = n runs
            got = check(mem, o, ln, sets["odd lines"], TAB, [(ODD_F, INT, EQ, 1)], False, False, "the bound, ranges")
            assert got == sets["odd lines"]


STEP_A, STEP_B, STEP_C, STEP_ALT, STEP_ALL = range(5)  # the fields of step_text


def step_runs(L):
    """select_cases.scan_step's runs for W = kSlRunRecords rows a group and S = W * kSlScanStep rows a step: per field runs
    across row S, ending at it, starting at it; the same at the group edge 5 W; the first and the last row; both sides of
    a byte of the bitmap."""
    W, S = RUN_RECORDS, RUN_RECORDS * SCAN_STEP
    return {STEP_A: [(0, 1), (3 * W - 1, 3 * W + 1), (S - 2, S + 3), (L - 1, L)],
            STEP_B: [(7, 8), (5 * W, 5 * W + 2), (S - 3, S), (S + W - 1, S + W), (S + 2 * W, S + 2 * W + 1)],
            STEP_C: [(8, 9), (5 * W - 2, 5 * W), (S, S + 2), (S + 3 * W - 64, S + 3 * W + 64)]}


def step_text(L):
    """L lines of five 0/1 fields: the three of step_runs, every 16th row from row 1 on, all."""
    a = np.full((L, 10), TAB, dtype=np.uint8)
    a[:, 9] = NL
    a[:, 0:9:2] = ord("0")
    for f, rs in step_runs(L).items():
        for b, e in rs:
            a[b:e, 2 * f] = ord("1")
    a[1::16, 2 * STEP_ALT] = ord("1")
    a[:, 2 * STEP_ALL] = ord("1")
    return a.tobytes()


def scan_step(lib, both_forms=True):
    """k_wh_runs_scan (gzpx_where.h) across its step of kSlScanStep groups of kSlRunRecords rows: about 135,000 lines, so
    that the ranks of the runs behind row S = 131,072 need the first step's total.  Runs across the step, ending at it and
    starting at it, one field each, all lines as one range; then sets of ranges whose starts -- the second bitmap, which
    breaks a run -- fall at rows S - 1, S, S + 1 and S + W, and one of a repeated range with more than two steps of
    rows: ALL (every 16th row: every group has 32 rising edges of its own) and ANY (the three fields' runs), plain and
    inverted, the host form and the table form (`both_forms` False, for the emulator: a set takes one form and one of the
    two formats, in turn)."""
    mem = Mem(lib)
    W, S = RUN_RECORDS, RUN_RECORDS * SCAN_STEP
    L = S + 4 * W + 37
    assert 130000 <= L <= 290000
    text = step_text(L)
    one = lambda f: [(f, INT, EQ, 1)]
    any_terms = one(STEP_A) + one(STEP_B) + one(STEP_C)
    all_terms = one(STEP_ALT) + one(STEP_ALL)
    sets = [[(0, L)], [(0, S - 1), (S - 1, L)], [(0, S), (S, L)], [(0, S + 1), (S + 1, L)], [(0, S + W), (S + W, L)], [(0, L // 3)] * 7]
    assert 7 * (L // 3) > 2 * S
    ln = None
    for fmt in FORMATS:
        s = cut(fmt, text, list(range(60000, len(text), 60000)))
        pl = Plain(fmt, s)
        assert pl.plain == text and len(s) <= 300000
        ln = ln or Lines(pl, NL)  # (the same lines in both formats: the model's cells are made once)
        assert ln.L == L
        for f, rs in step_runs(L).items():  # the model's own runs are the intended ones
            assert model(ln, NL, TAB, [(0, L)], one(f))[0] == rs
        assert len(model(ln, NL, TAB, [(0, L)], all_terms)[0]) == -(-(L - 1) // 16) > L // W
        assert model(ln, NL, TAB, sets[2], one(STEP_A))[0][2:4] == [(S - 2, S), (S, S + 3)]  # a range's start breaks a run
        with Opened(lib, mem, fmt, s, NL, ROUTES[fmt == MGZIP]) as o:
            for f in step_runs(L):
                for invert in (False, True):
                    check(mem, o, ln, [(0, L)], TAB, one(f), False, invert, ("scan step", fmt, f, invert), table=invert, count=not invert)
            for i, rs in enumerate(sets):
                if not both_forms and FORMATS[i % 2] != fmt:
                    continue
                for terms, any_ in ((all_terms, False), (any_terms, True)):
                    for invert in (False, True):
                        for table in ((False, True) if both_forms else (i in (1, 2, 5),)):
                            check(mem, o, ln, rs, TAB, terms, any_, invert, ("scan step", fmt, rs[:2], any_, invert, table), table=table)


# ------------------------------------------------------------------------------------------------ 4. capacity
def capacity(lib):
    mem = Mem(lib)
    text = number_text(30000, 5)
    for fmt in FORMATS:
        s = cut(fmt, text, [17000])
        ln = Lines(Plain(fmt, s), NL)
        rs = [(0, ln.L), (ln.L // 2, ln.L), (3, 3)]
        terms = [(0, INT, GE, 0), (1, FLT, LT, 1.0)]
        want_runs, selected, rows, not_ok = model(ln, NL, TAB, rs, terms, True)
        n = len(want_runs)
        totals = (n, selected, rows, not_ok)
        assert n > 50
        with Opened(lib, mem, fmt, s) as o:
            for table in (False, True):
                assert where(mem, o, rs, TAB, terms, True, False, None, table)[0] == totals  # d_runs == NULL counts
                for cap in (0, n - 1):
                    e, tb = where(mem, o, rs, TAB, terms, True, False, cap, table)
                    assert isinstance(e, _native.GzpxError) and (e.code, e.needed) == (_native.ERR_INSUFFICIENT_SPACE, n), (fmt, table, cap)
                    assert tb[:cap] == [list(r) for r in want_runs[:cap]], (fmt, table, cap, "the first runs_cap runs")
                    assert tb[cap:] == [[UNTOUCHED, UNTOUCHED]] * GUARD, (fmt, table, cap, "written behind runs_cap")
                    rc, counts = raw_where(lib, o, rs, TAB, terms_raw(terms), len(terms), _native.WHERE_ANY, cap=cap, runs=True, mem=mem)
                    assert (rc, counts) == (_native.ERR_INSUFFICIENT_SPACE, totals), (fmt, cap, "the totals always come back")
                got, tb = where(mem, o, rs, TAB, terms, True, False, n, table)
                assert got == totals and tb == [list(r) for r in want_runs] + [[UNTOUCHED, UNTOUCHED]] * GUARD
                got, tb = where(mem, o, rs, TAB, terms, True, False, n + 7, table)
                assert got == totals and tb[n:] == [[UNTOUCHED, UNTOUCHED]] * (7 + GUARD), "entries behind n_runs"


# ------------------------------------------------------------------------------------------------ 5. errors
def terms_raw(terms):
    return [tuple(int(x) for x in t) for t in _native.DContext.where_terms(terms).tolist()]


def raw_where(lib, o, ranges, fd, raw_terms, n_terms, flags, cap=0, runs=False, mem=None, d_runs=None):
    """The C call itself: (rc, (n_runs, n_selected, n_rows, n_not_ok)), the counts preset to 77."""
    r = np.ascontiguousarray(np.array(ranges, dtype=np.uint64).reshape(-1, 2))
    tm = np.zeros(max(len(raw_terms), 1), dtype=_native.WHERE_TERM_DTYPE)
    for i, t in enumerate(raw_terms):
        tm[i] = t
    if runs:
        _, d_runs = mem.put(bytes([FILL]) * 16 * (cap + GUARD))
    c = [ctypes.c_uint64(77) for _ in range(4)]
    bad, info = ctypes.c_size_t(77), _native.GzpxCheckInfo()
    rc = lib.L.gzpx_where_lines_device(o.d.h, o.ix.h, o.lt.h, o.ptr, o.n, r.ctypes.data, r.shape[0], fd, tm.ctypes.data, n_terms, flags,
                                       d_runs, cap, ctypes.byref(c[0]), ctypes.byref(c[1]), ctypes.byref(c[2]), ctypes.byref(c[3]),
                                       ctypes.byref(bad), ctypes.byref(info), None)
    return rc, tuple(x.value for x in c)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def errors(lib):
    mem = Mem(lib)
    text = number_text(20000, 6)
    INV = _native.ERR_INVALID_ARG
    for fmt in FORMATS:
        s = cut(fmt, text, [7000])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        L = ln.L
        with Opened(lib, mem, fmt, s) as o:
            whole = [(0, L)]
            kr, pr = mem.put(bytes([FILL]) * 16 * 64)
            many = [(k // 2, INT, GE if k % 2 else LE, k) for k in range(34)]
            rc, counts = raw_where(lib, o, whole, TAB, many[:32], 32, 0)
            assert rc == _native.OK and counts[2] == L and o.d.last_lines_members() == pl.n
            cases = (("0 terms", [(0, INT, LT, 0)], 0, 0, TAB), ("33 terms", many[:33], 33, 0, TAB),
                     ("descending fields", [(3, INT, LT, 0), (1, INT, LT, 0)], 2, 0, TAB),
                     ("two types on one field", [(2, INT, LT, 0), (2, FLT, LT, 0)], 2, 0, TAB),
                     ("17 distinct fields", [(k, INT, LT, 0) for k in range(17)], 17, 0, TAB),
                     ("an unknown op", [(0, INT, 8, 0)], 1, 0, TAB), ("an unknown type", [(0, 2, LT, 0)], 1, 0, TAB),
                     ("IS_OK with a value", [(0, INT, IS_OK, 1)], 1, 0, TAB), ("NOT_OK with a value", [(0, FLT, NOT_OK, bits(1.0))], 1, 0, TAB),
                     ("a NaN", [(0, FLT, LT, column_cases.NAN)], 1, 0, TAB), ("a negative NaN", [(0, FLT, NE, bits(float("nan")) | 1 << 63)], 1, 0, TAB),
                     ("a signalling NaN", [(0, FLT, GE, 0x7FF0000000000001)], 1, 0, TAB),
                     ("a flag bit beyond the two", [(0, INT, LT, 0)], 1, 4, TAB), ("all flag bits", [(0, INT, LT, 0)], 1, 0xFFFFFFFF, TAB),
                     ("field_delim == the table's delimiter", [(0, INT, LT, 0)], 1, 0, NL), ("field_delim > 255", [(0, INT, LT, 0)], 1, 0, 256))
            for what, raw, n_terms, flags, fd in cases:
                got = raw_where(lib, o, whole, fd, raw, n_terms, flags, cap=16, d_runs=pr)
                assert got == (INV, (0, 0, 0, 0)), (fmt, what, got)
                assert o.d.last_lines_members() == 0, (fmt, what)
                assert mem.get(kr, 16 * 64) == bytes([FILL]) * 16 * 64, (fmt, what)
                raw_where(lib, o, [(0, 1)], TAB, [(0, INT, LT, 0)], 1, 0)  # (something is inflated in between)
            assert raw_where(lib, o, [], TAB, [(0, 7, LT, 0)], 1, 0) == (INV, (0, 0, 0, 0)), "a bad term and no ranges"
            assert raw_where(lib, o, whole, TAB, [(0, INT, LT, 0)], 1, 0, cap=16, d_runs=pr + -pr % 8 + 4)[0] == INV, "d_runs not 8-byte aligned"
            assert o.d.last_lines_members() == 0
            # an infinity is a constant like any other
            assert raw_where(lib, o, whole, TAB, [(1, FLT, LT, bits(float("inf")))], 1, 0)[0] == _native.OK
            good = [(0, 2), (L - 2, L), (5, 5)]
            for what, r, at in (("b = L + 1", [(L - 1, L + 1)], 3), ("a > b", [(11, 10)], 3), ("first", None, 0)):
                rs = good + r + good if r else [(L + 5, L + 6)] + good
                for table in (False, True):
                    e, tb = where(mem, o, rs, TAB, [(0, INT, GE, 0)], False, False, 16, table)
                    assert isinstance(e, _native.GzpxError) and (e.code, e.range_index) == (INV, at), (fmt, what, table)
                    assert tb == [[UNTOUCHED, UNTOUCHED]] * (16 + GUARD) and o.d.last_lines_members() == 0
            for table in (False, True):  # no ranges, and ranges that are all empty
                assert where(mem, o, [], TAB, [(0, INT, GE, 0)], False, True, 4, table) == ((0, 0, 0, 0), [[UNTOUCHED, UNTOUCHED]] * (4 + GUARD))
                assert o.d.last_lines_members() == 0
                assert where(mem, o, [(5, 5), (L, L)], TAB, [(0, INT, GE, 0)], False, True, 4, table)[0] == (0, 0, 0, 0)
            assert o.d.last_where_ms() == (0.0, 0.0, 0.0)
            with _native.DContext(format=BGZF + MGZIP - fmt, lib=lib) as d2:
                with pytest.raises(_native.GzpxError) as e:
                    d2.where_lines_device(o.ix, o.lt, o.ptr, o.n, [(0, 1)], TAB, [(0, INT, GE, 0)])
                assert e.value.code == INV and e.value.range_index is None


# ------------------------------------------------------------------------------------------------ 6. a damaged member
def damaged(lib):
    """A damaged member that the ranges touch: the inflate's error class and the member's index in the stream, all counts
    0, the table untouched; the context serves on.  One that they do not touch is never seen."""
    mem = Mem(lib)
    terms = [(0, INT, GE, 0), (1, FLT, NOT_OK, 0)]
    for fmt in FORMATS:
        text = number_text(8 * 5000, 11)[:8 * 5000 - 1] + b"\n"
        s = cut(fmt, text, [5000 * i for i in range(1, 8)])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        mid = int(np.searchsorted(ln.start, 3 * 5000 + 2500))
        route = ROUTES[fmt == BGZF]
        with Opened(lib, mem, fmt, s, route=route) as o:  # (the table of the undamaged stream)
            for victim in (0, 3, 7):
                for what, at, code in (("crc", pl.off[victim] + pl.size[victim] - 8, _native.ERR_INVALID_CHECK),
                                       ("block type", pl.off[victim] + HDR[fmt], _native.ERR_BAD_DATA)):
                    m = bytearray(s)
                    if what == "crc":
                        m[at] ^= 0xFF
                    else:
                        m[at] |= 0x06  # BTYPE = 3, reserved
                    keep, ptr = mem.put(m)
                    with o.d.build_index_device(ptr, len(m)) as ix:  # (the members' extents are the same: the table serves)
                        bad = type("O", (), dict(d=o.d, ix=ix, lt=o.lt, ptr=ptr, n=len(m)))
                        e, tb = where(mem, bad, [(0, ln.L)], TAB, terms, True, False, 8)
                        assert isinstance(e, _native.GzpxError), (fmt, victim, what, e)
                        assert (e.code, e.block, e.needed) == (code, victim, None), (fmt, route, victim, what)
                        assert tb == [[UNTOUCHED, UNTOUCHED]] * (8 + GUARD)
                        rc, counts = raw_where(lib, bad, [(0, ln.L)], TAB, terms_raw(terms), 2, 0)
                        assert (rc, counts) == (code, (0, 0, 0, 0)), (fmt, victim, what, "the counts of a failing member")
                        if victim != 3 and what == "crc":  # a range that does not touch the member
                            check(mem, bad, ln, [(mid, mid + 3)], TAB, terms, True, False, (fmt, route, victim, what))
            check(mem, o, ln, [(0, ln.L)], TAB, terms, True, False, (fmt, route, "after the damage"))


# ------------------------------------------------------------------------------------------------ 7. closing the loop
def close_the_loop(lib):
    """grep | awk | cut on the device: select_lines_device, its table into where_lines_table_device, that table into
    read_lines_table_device and read_columns_table_device; against the same pipeline in Python."""
    mem = Mem(lib)
    text = number_text(30000, 8)
    pattern = b"qu"
    terms = [(0, INT, GE, -5 * 10 ** 8), (0, INT, LT, 5 * 10 ** 8), (1, FLT, NOT_OK, 0)]
    cols = [(0, INT), (1, FLT), (4, INT)]
    for fmt in FORMATS:
        s = cut(fmt, text, [40, 11000])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        all_lines = pl.plain.splitlines(keepends=True)
        assert len(all_lines) == ln.L
        want = want_of(ln, NL, TAB, cols)
        with Opened(lib, mem, fmt, s, route=ROUTES[fmt == MGZIP]) as o:
            for invert in (False, True):
                grep = [k for k, x in enumerate(all_lines) if (pattern in x) != invert]
                cap_g = -(-ln.L // 2)
                kg, pg = mem.put(bytes([FILL]) * 16 * cap_g)
                n_g, n_rec, _ = o.d.select_lines_device(o.ix, o.lt, o.ptr, o.n, pattern, 1, invert, pg, cap_g)
                assert n_g >= 2 and n_rec == len(grep)
                g_runs = np.frombuffer(mem.get(kg, 16 * n_g), dtype=np.uint64).reshape(-1, 2).tolist()
                runs_w, selected, rows, not_ok = model(ln, NL, TAB, [tuple(r) for r in g_runs], terms)
                keepers = [k for a, b in runs_w for k in range(a, b)]
                ok, _ = passes(ln, NL, TAB, terms, False)
                assert keepers == [k for k in grep if ok[k]] and rows == len(grep) and 0 < len(keepers) < len(grep)
                cap_w = (rows + n_g) // 2
                kw, pw = mem.put(bytes([FILL]) * 16 * (cap_w + GUARD))
                got = o.d.where_lines_table_device(o.ix, o.lt, o.ptr, o.n, pg, n_g, TAB, terms, False, False, pw, cap_w)
                assert got == (len(runs_w), selected, rows, not_ok), (fmt, invert, got)
                first = mem.get(kw, 16 * (cap_w + GUARD))
                tb = np.frombuffer(first, dtype=np.uint64).reshape(-1, 2).tolist()
                assert tb[:len(runs_w)] == [list(r) for r in runs_w] and tb[len(runs_w):] == [[UNTOUCHED, UNTOUCHED]] * (cap_w + GUARD - len(runs_w))
                # the host form of the call gives the same runs; a second call the same bytes
                got_h, tb_h = where(mem, o, [tuple(r) for r in g_runs], TAB, terms, False, False, len(runs_w))
                assert got_h == got and tb_h[:len(runs_w)] == tb[:len(runs_w)]
                assert o.d.where_lines_table_device(o.ix, o.lt, o.ptr, o.n, pg, n_g, TAB, terms, False, False, pw, cap_w) == got
                assert mem.get(kw, 16 * (cap_w + GUARD)) == first
                # ... | cut: the lines, and their numbers
                expect = b"".join(all_lines[k] for k in keepers)
                ko, po = mem.put(bytes([FILL]) * (len(expect) + 64))
                assert o.d.read_lines_table_device(o.ix, o.lt, o.ptr, o.n, pw, got[0], po, len(expect)) == len(expect)
                assert mem.get(ko, len(expect) + 64) == expect + bytes([FILL]) * 64, (fmt, invert)
                R = len(keepers)
                kv, pv = mem.put(bytes([FILL]) * (8 * 3 * R + 64), shift=8)
                ks, ps = mem.put(bytes([FILL]) * (3 * R + 64), shift=3)
                n_rows, n_bad, _ = o.d.read_columns_table_device(o.ix, o.lt, o.ptr, o.n, pw, got[0], TAB, cols, pv, ps, R)
                assert n_rows == R and n_bad == int((want.st[:, keepers] != OK).sum()), (fmt, invert)
                v = np.frombuffer(mem.get(kv, 8 * 3 * R + 8)[8:], dtype=np.uint8)
                st = np.frombuffer(mem.get(ks, 3 * R + 3)[3:], dtype=np.uint8)
                assert np.array_equal(v.view(np.uint64).reshape(3, R), want.val[:, keepers]), (fmt, invert)
                assert np.array_equal(st.reshape(3, R), want.st[:, keepers]), (fmt, invert)
