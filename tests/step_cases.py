"""The steps of the single-workgroup scans behind the text calls, written once and run twice: through the emulated
library on CPU (tests/test_emu_steps.py) and through the real HIP library on the MI355X (tests/test_gpu_steps.py).

A scan of one workgroup walks its items in steps and carries a total -- or, for the segmented scans of the pieces, a
count with a reset bit -- from one step into the next.  A broken carry leaves everything in front of the first step's end
right and everything behind it wrong, so every case here gives a scan more items than one step and checks what lies
behind the step.  The sizes come from the kernels' constants, read from the headers (K): a case asserts that its input
crosses the step it names, so a changed constant moves the case with it or fails it.

The yardstick is never the library: range_cases.Plain, line_cases.Lines and the Want models of field_cases,
column_cases and where_cases, as in the suites of the calls themselves.  Every comparison is exact.

The runs scan of where (k_wh_runs_scan) has its case beside the other run cases: where_cases.scan_step."""
import glob
import os
import re

import numpy as np

import column_cases
import field_cases
import line_cases
import range_cases
import where_cases
from column_cases import INT
from gzp_amd import _native
from line_cases import Lines, Opened, cut
from range_cases import Plain, ROUTES
from scan_cases import BGZF, MGZIP, Mem
from where_cases import GE, IS_OK

NL, TAB = 0x0A, 0x09

_src = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gzp_amd", "csrc",
                                                                     "gzpx_*.h"))))
K = {name: int(re.search(r"constexpr uint32_t %s = (\d+);" % name, _src).group(1))
     for name in ("kFlThreads", "kFlScanItems", "kFlPiece", "kLnThreads", "kLnScanItems", "kLnTile", "kFdThreads", "kFdScanItems",
                  "kFdPiece", "kFdPad", "kRrThreads", "kRrItems", "kWhRunGrid", "kSlRunRecords", "kSlScanStep")}
FL_STEP = K["kFlThreads"] * K["kFlScanItems"]  # pieces per step of k_fl_carry_scan, k_fl_scan and k_cl_rows_scan's second loop
LN_STEP = K["kLnThreads"] * K["kLnScanItems"]  # tiles per step of k_ln_prefix
FD_STEP = K["kFdThreads"] * K["kFdScanItems"]  # pieces of a batch per step of k_fd_scan
RR_STEP = K["kRrThreads"] * K["kRrItems"]      # members per step of k_rr_select
assert K["kFlPiece"] == K["kLnTile"] == K["kFdPiece"] == line_cases.T, "the cases below place bytes on one 16 KiB grid"


# ------------------------------------------------------------------------------------------------ a. pieces
PIECE_FIELDS = [(1, 2), (9000, 9002)]
PIECE_COLS = [(0, INT), (9000, INT)]
PIECE_TERMS = [(0, INT, GE, 25), (9000, INT, IS_OK, 0)]
LONG_AT, LONG_FIELDS = 50, 12000


def piece_text():
    """50 short numeric lines, one line of 12,000 tab-separated integers (about 60 KiB), 50 more short lines.  Field 0 lies
    on both sides of 25 in the short lines and is 30 in the long one, the only line that has a field 9000."""
    short = [b"%d\t%d\t%d\n" % (i * 37 % 50, 7 * i, i % 5) for i in range(2 * LONG_AT + 1)]
    long_line = b"\t".join([b"30"] + [b"%d" % (1000 + 7 * k % 9000) for k in range(1, LONG_FIELDS)]) + b"\n"
    return b"".join(short[:LONG_AT]) + long_line + b"".join(short[LONG_AT + 1:])


def pieces_of(ln, a, b):
    """The pieces of the line range [a, b) where staging holds the stream from its first byte on (fl_pieces)."""
    s, e = int(ln.start[a]), int(ln.start[b])
    return (e - 1) // K["kFlPiece"] - s // K["kFlPiece"] + 1


def piece_ranges(k):
    j = LONG_AT
    return [(0, 1)] * k + [(j - 3, j + 3)] + [(0, 2)] * 10


def piece_steps(lib, ks, table_ks, mgzip_ks=(), host_ks=None):
    """k_fl_carry_scan, k_fl_scan and the second loop of k_cl_rows_scan (gzpx_fields.h, gzpx_columns.h) across their step
    of kFlThreads * kFlScanItems = 4,096 pieces.  `k` one-line ranges, a piece each, stand in front of a range of six
    lines whose fourth is many pieces long, and ten ranges behind it: with k around the step the scans carry a field count
    of thousands (cin), the range's lines so far (rin) and an output base over the step's end -- behind the range's
    first piece, inside the long line, at its last piece -- and a range's first piece is the last of a step or the first
    of the next.  read_fields_device (the list and its complement), read_columns_device and where_lines_device (ALL,
    ANY) against their models for the k of `host_ks` (by default those not in `table_ks`), the table forms of the three
    calls for the k of `table_ks` -- a k in both takes both forms -- and the k of `mgzip_ks` as Mgzip through the other
    inflate route."""
    mem = Mem(lib)
    assert 1024 <= FL_STEP <= 16384
    text = piece_text()
    j = LONG_AT
    for fmt in (BGZF, MGZIP):
        mine = [k for k in ks if (k in mgzip_ks) == (fmt == MGZIP)]
        if not mine:
            continue
        s = cut(fmt, text, [len(text) // 3, 2 * len(text) // 3])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        # the construction itself
        long_line = pl.plain[int(ln.start[j]):int(ln.start[j + 1])]
        assert pl.n == 3 and ln.L == 2 * LONG_AT + 1 and len(s) <= 200000
        assert len(long_line) > 3 * K["kFlPiece"] and long_line.count(b"\t") + 1 == LONG_FIELDS > 9002
        assert int(ln.start[2]) <= K["kFlPiece"] and pieces_of(ln, 0, 1) == pieces_of(ln, 0, 2) == 1
        wide = pieces_of(ln, j - 3, j + 3)
        assert 4 <= wide <= 5 and int(ln.start[j]) < K["kFlPiece"] < int(ln.start[j + 1]) - 2 * K["kFlPiece"]
        wants_f = {c: field_cases.Want(ln, NL, TAB, PIECE_FIELDS, c) for c in (False, True)}
        want_c = column_cases.Want(ln, NL, TAB, PIECE_COLS)
        assert want_c.st[1].tolist().count(column_cases.OK) == 1 and want_c.st[1, j] == column_cases.OK
        with Opened(lib, mem, fmt, s, NL, ROUTES[fmt == MGZIP]) as o:
            for k in mine:
                rs = piece_ranges(k)
                # every cover starts at the stream's first byte and the members read are the stream's first ones: a byte
                # lies in staging where it lies in the stream, and the pieces in front of the six lines number exactly k
                need = pl.union([ln.cover(a, b) for a, b in rs])
                assert need == set(range(len(need))) and all(ln.cover(a, b)[0] == 0 for a, b in rs)
                assert sum(pieces_of(ln, a, b) for a, b in rs[:k]) == k
                assert k + wide + 10 > FL_STEP, "the pieces of the call cross the step"
                forms = [f for f, chosen in ((False, k not in table_ks if host_ks is None else k in host_ks), (True, k in table_ks)) if chosen]
                assert forms, k
                for table in forms:
                    what = ("piece steps", fmt, k, table)
                    for comp, want in wants_f.items():
                        if table:
                            data, offs = want.data(rs), want.offsets(rs)
                            got, got_offs = field_cases.read_table(mem, o, rs, TAB, PIECE_FIELDS, comp, len(data))
                            assert got_offs == offs + [field_cases.UNTOUCHED] * field_cases.GUARD_OFF, (what, comp, "d_out_offsets")
                            assert got == data, (what, comp, "bytes")
                            assert o.d.last_lines_members() == len(need), (what, comp, "members read")
                        else:
                            field_cases.check(mem, o, ln, want, rs, TAB, PIECE_FIELDS, comp, what + (comp,), query=False)
                    column_cases.check(mem, o, want_c, rs, TAB, what, table=table)
                    for any_ in (True, False):
                        runs = where_cases.check(mem, o, ln, rs, TAB, PIECE_TERMS, any_, False, what + (any_,), table=table)
                        if not any_:  # ALL: the long line alone, row k + 3 of the call
                            assert runs == [(j, j + 1)]


# ------------------------------------------------------------------------------------------------ c. members
def member_text(n_members, seed):
    """(text, cuts): n_members members of 20..40 bytes of lines of 0..11 letters."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(20, 41, n_members)
    n = int(sizes.sum())
    a = rng.integers(ord("a"), ord("z") + 1, n, dtype=np.uint8)
    at = np.cumsum(rng.integers(1, 13, n // 6 + 2))
    a[at[at < n]] = NL
    a[-1] = NL
    return a.tobytes(), np.cumsum(sizes)[:-1].tolist()


def member_steps(lib, light=False):
    """k_rr_select (gzpx_ranges.h) across its step of kRrThreads * kRrItems = 1,024 members: a BGZF stream of two steps
    and 50 members of 20..40 bytes, so that the coverage, the rank and the staging offset are each carried over two step
    ends.  Byte ranges (read_ranges_device) and line ranges (read_lines_device) that begin or end in the members around
    both step ends, in the first and in the last member, and one over everything; every range in a call of its own, and
    all of them in one call, where the members selected are sparse and a member's rank is not its index.  Both inflate
    routes; the members read against Plain.union.  (`light`, for the emulator, where a call costs 3 ms a member: the byte
    ranges through the first route; through the second every third line range in a call of its own and all of them in
    one; the call with all byte ranges through both.)"""
    mem = Mem(lib)
    M = RR_STEP
    assert 256 <= M <= 4096
    n_members = 2 * M + 50
    text, cuts = member_text(n_members, 31)
    s = cut(BGZF, text, cuts)
    pl = Plain(BGZF, s)
    ln = Lines(pl, NL)
    assert pl.n == n_members > 2 * M and 20 <= min(pl.isize) and max(pl.isize) <= 40 and len(s) <= 400000
    u, t = pl.ustart, pl.total
    around = (0, M - 1, M, M + 1, 2 * M - 1, 2 * M, 2 * M + 1, n_members - 1)
    byte_ranges = []
    for m in around:
        byte_ranges.append((u[m] + 3, u[m] + 9))                # inside member m
        if m:
            byte_ranges.append((u[m] - 4, u[m] + 4))            # begins in m - 1, ends in m
    byte_ranges += [(u[M - 1] + 2, u[M + 1] + 5), (u[2 * M - 2], u[2 * M] + 1), (u[M] + 1, u[2 * M] + 1), (u[n_members - 1], t)]
    for (b, e), m in zip(byte_ranges[:3], (0, M - 1, M - 1)):
        assert pl.union([(b, e)]) in ({m}, {m - 1, m})
    assert pl.union([byte_ranges[-4]]) == {M - 1, M, M + 1} and pl.union([byte_ranges[-2]]) == set(range(M, 2 * M + 1))
    sparse = byte_ranges[::-1]
    assert M < len(pl.union(sparse)) < n_members - 100 and {0, n_members - 1} <= pl.union(sparse)
    # line ranges with the same placement: the first line that starts in member m, with the line in front of it
    line_ranges = []
    for m in around:
        k = int(np.searchsorted(ln.start, u[m]))
        k = min(max(k, 1), ln.L - 1)
        line_ranges += [(k, k + 1), (k - 1, k + 1)]
    line_ranges += [(0, 1), (ln.L - 1, ln.L)]
    keep, ptr = mem.put(s, shift=5)
    for route in ROUTES:
        with _native.DContext(format=BGZF, lib=lib) as d, d.build_index_device(ptr, len(s)) as ix:
            d.set_route(route)
            assert (ix.n_members, ix.inflated_len) == (n_members, t)
            if not light or route == ROUTES[0]:
                for r in byte_ranges:
                    range_cases.check_read(mem, d, ix, pl, ptr, len(s), [r], ("member steps", route, r))
                range_cases.check_read(mem, d, ix, pl, ptr, len(s), sparse, ("member steps", route, "sparse"))
            range_cases.check_read(mem, d, ix, pl, ptr, len(s), byte_ranges + [(0, t)], ("member steps", route, "all"))
        if light and route == ROUTES[0]:
            continue
        with Opened(lib, mem, BGZF, s, NL, route) as o:
            line_cases.check_table(o, ln, ("member steps", route))
            for r in (line_ranges[::3] if light else line_ranges):
                line_cases.check_read(mem, o, ln, [r], ("member steps, lines", route, r))
            line_cases.check_read(mem, o, ln, line_ranges + [(0, ln.L)], ("member steps, lines", route, "all"))
