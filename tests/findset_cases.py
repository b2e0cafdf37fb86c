"""The search for a set of patterns (gzpx_find_set_device, gzpx_select_lines_set_device), written once and run twice:
through the emulated library on CPU (tests/test_emu_findset.py) and through the real HIP library on the MI355X
(tests/test_gpu_findset.py).

The yardstick is never the library.  It is range_cases.Plain (zlib's inflate of every member, joined); the hits are
find_cases.host_hits per pattern, merged by (p, k); the lines find_cases.host_lines of the merged positions; the counts
the per-pattern hit numbers; the selected records and runs come from those lines by integer division and numpy's edge
detection, as select_cases.host_select computes them for one pattern."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import find_cases
import line_cases
import select_cases
from find_cases import BATCHES, FILL, GUARD, LENGTHS, NL, T, TAB, host_hits, host_lines, letters, pattern_of
from gzp_amd import _native
from line_cases import Lines, cut, short_lines
from range_cases import Plain, ROUTES
from scan_cases import BGZF, MGZIP, HDR, Mem

MAXP, MAXB = _native.FINDSET_MAX_PATTERNS, _native.FINDSET_MAX_BYTES
INV = _native.ERR_INVALID_ARG
U64 = int.from_bytes(bytes([FILL]) * 8, "little")
U32 = int.from_bytes(bytes([FILL]) * 4, "little")

_dev = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gzp_amd", "csrc", "gzpx_device.h")).read()
HASH = int(re.search(r"window \* (0x[0-9A-Fa-f]+)u\) >> 16", _dev).group(1), 16)  # the filter's multiplier for q = 3, 4


# ------------------------------------------------------------------------------------------------ the yardstick
_per = {}


def per_pattern(pl, pattern):
    key = (id(pl), bytes(pattern))
    if key not in _per:
        _per[key] = (pl, host_hits(pl.plain, bytes(pattern)))  # (pl kept alive: its id stays its own)
    return _per[key][1]


def host_set(pl, patterns, delim=None):
    """(positions, ids, lines or None, counts): the hits of every pattern, merged by (p, k)."""
    per = [per_pattern(pl, p) for p in patterns]
    pos = np.concatenate(per) if per else np.zeros(0, np.int64)
    ids = np.concatenate([np.full(h.size, k, np.int64) for k, h in enumerate(per)])
    order = np.lexsort((ids, pos))
    pos, ids = pos[order], ids[order]
    lines = host_lines(pl.plain, delim, pos) if delim is not None else None
    return pos, ids, lines, np.array([h.size for h in per], dtype=np.int64)


def host_select_set(pl, ln, delim, patterns, g, invert):
    """select_cases.host_select with the set's hits."""
    pos, _, lines, _ = host_set(pl, patterns, delim)
    L = ln.L
    R = -(-L // g)
    sel = np.zeros(R, dtype=bool)
    sel[np.unique(lines // g)] = True
    if invert:
        sel = ~sel
    edge = np.diff(np.concatenate([[0], sel.astype(np.int8), [0]]))
    r0, r1 = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    return [(int(g * a), int(min(g * b, L))) for a, b in zip(r0, r1)], int(sel.sum()), int(pos.size)


# ------------------------------------------------------------------------------------------------ the call
class Opened(find_cases.Opened):
    def count(self, patterns, delim=None):
        """A count-only call: (n_hits, d_counts)."""
        k = len(patterns)
        kc, cp = self.mem.put(bytes([FILL]) * 8 * (k + GUARD))
        n = self.d.find_set_device(self.ix, self.ptr, self.n, patterns, delim, d_counts_ptr=cp)
        c = np.frombuffer(self.mem.get(kc, 8 * (k + GUARD)), dtype=np.uint64)
        assert c[k:].tolist() == [U64] * GUARD, "counts written behind n_patterns"
        return n, c[:k].astype(np.int64)

    def find_set(self, patterns, delim, cap, positions=True, ids=True, lines=True, counts=True):
        """One writing call with `cap` entries and GUARD more behind them in each array: (n_hits or the GzpxError raised,
        positions, ids, lines, counts; None for an array that was not given)."""
        k = len(patterns)
        put = lambda want, size: self.mem.put(bytes([FILL]) * size) if want else (None, None)
        kp, pp = put(positions, 8 * (cap + GUARD))
        ki, ip = put(ids, 4 * (cap + GUARD))
        kl, lp = put(lines, 8 * (cap + GUARD))
        kc, cp = put(counts, 8 * (k + GUARD))
        try:
            got = self.d.find_set_device(self.ix, self.ptr, self.n, patterns, delim, pp, ip, lp, cap, cp)
        except _native.GzpxError as e:
            got = e
        back = lambda key, size, dt: np.frombuffer(self.mem.get(key, size), dtype=dt) if key is not None else None
        return (got, back(kp, 8 * (cap + GUARD), np.uint64), back(ki, 4 * (cap + GUARD), np.uint32),
                back(kl, 8 * (cap + GUARD), np.uint64), back(kc, 8 * (k + GUARD), np.uint64))


def check(o, pl, patterns, delim, what):
    """Count only, then everything into arrays of exactly n_hits entries."""
    pos, ids, lines, counts = host_set(pl, patterns, delim)
    n, k = pos.size, len(patterns)
    got_n, got_c = o.count(patterns)
    assert got_n == n and got_c.tolist() == counts.tolist(), (what, "count only", got_n, n)
    got, p, i, l, c = o.find_set(patterns, delim, n, lines=delim is not None)
    assert got == n, (what, "n_hits", got, n)
    assert p[:n].tolist() == pos.tolist(), (what, "positions")
    assert i[:n].tolist() == ids.tolist(), (what, "ids")
    assert p[n:].tolist() == [U64] * GUARD and i[n:].tolist() == [U32] * GUARD, (what, "written behind hits_cap")
    if delim is not None:
        assert l[:n].tolist() == lines.tolist(), (what, "lines")
        assert l[n:].tolist() == [U64] * GUARD, (what, "lines written behind hits_cap")
    assert c[:k].tolist() == counts.tolist() and c[k:].tolist() == [U64] * GUARD, (what, "counts")
    assert all(t >= 0.0 for t in o.d.last_find_set_ms())
    return n


def check_batches(lib, mem, name, fmt, s, pl, cases, route=ROUTES[0], batches=BATCHES, shift=0):
    """cases: (patterns, delim) pairs; every one at every batch size."""
    with Opened(lib, mem, fmt, s, route, shift) as o:
        for batch in batches:
            o.d.set_lines_batch(batch)
            for patterns, delim in cases:
                check(o, pl, patterns, delim, (name, fmt, route, batch, [bytes(p[:12]) for p in patterns[:6]], delim))


# ------------------------------------------------------------------------------------------------ 1. K = 1
def one_pattern(lib):
    """A set of one is the search: find_cases.planted(m) for every length, positions the planted starts, ids all 0."""
    mem = Mem(lib)
    for i, m in enumerate(LENGTHS):
        text, pat, starts = find_cases.planted(m)
        fmt = (BGZF, MGZIP)[i % 2]
        s = cut(fmt, text, find_cases.PLANT_CUTS, eof=fmt == BGZF and m % 4 == 1)
        pl = Plain(fmt, s)
        pos, ids, _, counts = host_set(pl, [pat])
        assert set(starts) <= set(pos.tolist()) and (m == 1 or pos.tolist() == starts) and not ids.any() and counts[0] == pos.size
        check_batches(lib, mem, "one pattern m=%d" % m, fmt, s, pl, [([pat], None)], ROUTES[(i // 2) % 2], shift=i % 16)


# ------------------------------------------------------------------------------------------------ 2. mixed lengths
MIXED = ((4, 8, 0, 6, 2, 7, 1, 5, 3), (1, 2, 3, 4, 5, 16, 17, 255, 256))  # a fixed permutation: id order is not length order
FURTHER = ((17, 2, 5), (256, 3, 4), (16, 255, 4), (255, 17, 256))          # shortest 2, 3, 4, 17: q = 2, 3, 4, 4


def mixed_sets():
    yield [MIXED[1][j] for j in MIXED[0]]
    yield from (list(x) for x in FURTHER)


def mixed_lengths(lib):
    """Every pattern of a set planted as find_cases.planted plants one (every word offset, the pieces' edges of staging,
    the member cuts, 0 and n), in a text of its own that holds the other patterns of the set too."""
    mem = Mem(lib)
    i = 0
    for lengths in mixed_sets():
        patterns = [pattern_of(m, seed=k) for k, m in enumerate(lengths)]
        for k, m in enumerate(lengths):
            text, pat, starts = find_cases.planted(m, seed=k)
            assert pat == patterns[k]
            text = bytearray(text)
            for j, other in enumerate(patterns):  # (27,000 .. 30,000 is free of planted starts)
                if j != k:
                    text[27000 + 300 * j:27000 + 300 * j + len(other)] = other
            fmt = (BGZF, MGZIP)[i % 2]
            s = cut(fmt, bytes(text), find_cases.PLANT_CUTS, eof=fmt == BGZF and i % 4 == 0)
            pl = Plain(fmt, s)
            pos, ids, _, counts = host_set(pl, patterns)
            assert set(starts) <= set(pos[ids == k].tolist()) and bool(np.all(counts >= 1))
            check_batches(lib, mem, "mixed %s planted %d" % (lengths, m), fmt, s, pl, [(patterns, None)], ROUTES[(i // 2) % 2],
                          shift=i % 16)
            i += 1


# ------------------------------------------------------------------------------------------------ 3. ties
def same_position(lib):
    """Patterns that are equal to, prefixes of and near misses of one another: ties in ascending id, both copies of the
    duplicate, nothing for the near miss where the last byte differs."""
    mem = Mem(lib)
    patterns = [b"abcdefgh", b"abcd", b"a", b"abcdefgh", b"ab", b"abcdefgX"]
    text = bytearray(letters(3000, 31).replace(b"a", b"q"))
    for at, what in ((0, b"abcdefgh"), (100, b"abcdefgX"), (1000 - 3, b"abcdefgh"), (1500, b"abcdefgY"), (2000, b"abcdabcdefgX"),
                     (3000 - 8, b"abcdefgh")):
        text[at:at + len(what)] = what
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, bytes(text), [1000, 2003], eof=fmt == BGZF)
        pl = Plain(fmt, s)
        pos, ids, _, counts = host_set(pl, patterns)
        assert ids[pos == 0].tolist() == [0, 1, 2, 3, 4] and ids[pos == 100].tolist() == [1, 2, 4, 5]
        assert ids[pos == 1500].tolist() == [1, 2, 4] and counts[0] == counts[3] == 3
        check_batches(lib, mem, "same position", fmt, s, pl, [(patterns, None), (patterns[::-1], NL)], batches=(0, 1000, 1))


# ------------------------------------------------------------------------------------------------ 4. buckets
def gram_index(w):
    return ((int.from_bytes(w, "little") * HASH) & 0xFFFFFFFF) >> 16


def colliding_windows():
    """Two 4-byte strings of lower-case letters whose windows share a bit of the filter."""
    seen = {}
    for t in itertools.product(b"klmnopqrstuvwxyz", repeat=4):
        w = bytes(t)
        i = gram_index(w)
        if i in seen:
            return seen[i], w
        seen[i] = w
    raise AssertionError("no collision")


def buckets(lib):
    mem = Mem(lib)
    rng = np.random.default_rng(41)
    # 64 patterns of 40 bytes in one bucket: the same first 4 bytes, 32 differ in byte 5 and 32 in the last byte
    base = b"abcd" + bytes(rng.integers(ord("A"), ord("Z") + 1, 36, dtype=np.uint8))
    shared = []
    for j in range(32):
        shared.append(base[:4] + bytes([0x80 + j]) + base[5:])
        shared.append(base[:39] + bytes([0x80 + j]))
    text = bytearray(letters(64 * 50 + 200, 42))
    for j, p in enumerate(shared):
        text[50 * j + 7:50 * j + 47] = p
    text[64 * 50 + 10:64 * 50 + 50] = base[:39] + b"~"  # a near miss of all of them
    # 64 patterns that differ only in the first byte, and a window of the text that collides with one of them in the filter
    in_set, stranger = colliding_windows()
    assert in_set != stranger and gram_index(in_set) == gram_index(stranger)
    firsts = [bytes([64 + j]) + b"SUFFIXES" for j in range(63)] + [in_set + b"TAIL"]
    text2 = bytearray(letters(64 * 20 + 100, 43).replace(b"S", b"s"))
    for j, p in enumerate(firsts):
        text2[20 * j + 3:20 * j + 3 + len(p)] = p
    text2[64 * 20 + 20:64 * 20 + 28] = stranger + b"TAIL"
    # 256 patterns of 64 bytes: the limit of bytes exactly, each planted twice
    full = [bytes(rng.integers(0, 256, 64, dtype=np.uint8)) for _ in range(MAXP)]
    assert sum(len(p) for p in full) == MAXB and len(set(full)) == MAXP
    text3 = bytearray(letters(2 * MAXP * 70 + 64, 44))
    for j, p in enumerate(full + full[::-1]):
        text3[70 * j + (j % 5):70 * j + (j % 5) + 64] = p
    for name, t, patterns, cuts, batches in (("one bucket", text, shared, [1600], BATCHES), ("first bytes", text2, firsts, [640], BATCHES),
                                             ("256 x 64", text3, full, [T - 30, 2 * T + 1], (0, 20000))):
        for fmt in (BGZF, MGZIP):
            s = cut(fmt, bytes(t), cuts)
            pl = Plain(fmt, s)
            _, _, _, counts = host_set(pl, patterns)
            assert counts.tolist() == [2 if name == "256 x 64" else 1] * len(patterns), name
            check_batches(lib, mem, name, fmt, s, pl, [(patterns, None)], route=ROUTES[fmt == MGZIP], batches=batches)


# ------------------------------------------------------------------------------------------------ 5. order across batches
def order_every_split(lib):
    """find_cases.batches_every_split with a 17-byte pattern, the 1-byte pattern of its 9th byte and the 2-byte pattern
    of its 2nd and 3rd byte, which occurs one byte behind every planted start: the short hits end in a batch in front of
    the one in which the long hit ends that starts in front of them.  Ownership by the last byte gets this order wrong."""
    mem = Mem(lib)
    pat = pattern_of(17)
    text = bytearray(letters(18000, 13))
    starts = [1000 * k - k for k in range(1, 17)]
    for p in starts:
        text[p:p + 17] = pat
    patterns = [pat[8:9], pat, pat[1:3]]
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, bytes(text), list(range(1000, 18000, 1000)))
        pl = Plain(fmt, s)
        pos, ids, _, counts = host_set(pl, patterns)
        assert pos[ids == 1].tolist() == starts and pos[ids == 2].tolist() == [p + 1 for p in starts] and counts[0] >= 16
        check_batches(lib, mem, "every split", fmt, s, pl, [(patterns, None), (patterns, ord("e"))], batches=(1000, 1, 0),
                      route=ROUTES[1])


# ------------------------------------------------------------------------------------------------ 6. the waiting carry
def waiting_carry(lib):
    """A 256-byte pattern keeps the last 255 bytes waiting in the carry; the batches behind them are empty (the BGZF EOF
    member, three empty members), so the short patterns' hits in those bytes are found only if the last batch is searched
    without a byte of its own."""
    mem = Mem(lib)
    rng = np.random.default_rng(61)
    long_pat = bytes(rng.integers(ord("A"), ord("Z") + 1, 256, dtype=np.uint8))
    patterns = [long_pat, b"xy", b"z"]
    n = 1500
    text = bytearray(letters(n, 62))
    for at in (100, n - 300):  # (the second ends 44 bytes in front of n)
        text[at:at + 256] = long_pat
    for at in (n - 40, n - 20, n - 3):
        text[at:at + 2] = b"xy"
    text[n - 30] = text[n - 1] = ord("z")
    text = bytes(text)
    tiny = np.cumsum(np.random.default_rng(11).integers(1, 4, 1000))
    streams = [("EOF member", BGZF, cut(BGZF, text, [700], eof=True), (1,)),
               ("three empty members", MGZIP, cut(MGZIP, text, [700, n, n, n]), (1,)),
               ("three empty members", BGZF, cut(BGZF, text, [700, n, n, n]), (1, 0)),
               ("tiny members", MGZIP, cut(MGZIP, text[n - 340:], tiny[tiny < 340].tolist()), (1, 0)),
               ("tiny members + EOF", BGZF, cut(BGZF, text[n - 340:], tiny[tiny < 340].tolist(), eof=True), (1, 0)),
               ("n < M", BGZF, cut(BGZF, text[n - 100:], [50], eof=True), (1, 0)),
               ("n < M", MGZIP, cut(MGZIP, text[n - 100:], [30, 100]), (1, 0))]
    for i, (name, fmt, s, batches) in enumerate(streams):
        pl = Plain(fmt, s)
        pos, ids, _, counts = host_set(pl, patterns)
        assert pos[-1] == pl.total - 1 and ids[-1] == 2 and counts[1] >= 3 and counts[2] >= 2, name
        assert counts[0] == (0 if name == "n < M" else 1 if name.startswith("tiny") else 2), name
        assert name == "n < M" or pl.isize[-1] == 0 or max(pl.isize) <= 3
        check_batches(lib, mem, name, fmt, s, pl, [(patterns, None), (patterns, ord("z"))], route=ROUTES[i % 2], batches=batches)
    for fmt in (BGZF, MGZIP):  # every pattern longer than the stream: nothing is inflated
        s = cut(fmt, text[:100], [50])
        with Opened(lib, mem, fmt, s) as o:
            n_hits, counts = o.count([b"q" * 101, long_pat])
            assert n_hits == 0 and counts.tolist() == [0, 0] and o.d.last_find_set_ms() == (0.0, 0.0, 0.0)
            got, p, i, l, c = o.find_set([b"q" * 101, long_pat], NL, 2)
            assert got == 0 and p.tolist() == [U64] * (2 + GUARD) and c[:2].tolist() == [0, 0]
        with Opened(lib, mem, fmt, b"" if fmt == BGZF else cut(fmt, b"", [0])) as o:
            n_hits, counts = o.count([b"a", b"b"])
            assert n_hits == 0 and counts.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 7. dense overlaps
def dense_overlaps(lib):
    mem = Mem(lib)
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, b"A" * 40000, [9000, 25000])
        pl = Plain(fmt, s)
        patterns = [b"A", b"AAAA", b"A" * 256, b"AB", b"AAAAAB"]
        assert host_set(pl, patterns)[3].tolist() == [40000, 39997, 39745, 0, 0]
        check_batches(lib, mem, "40,000 x A", fmt, s, pl, [(patterns, None)], route=ROUTES[fmt == MGZIP], batches=(0, 20000))
    # 16 positions x 64 patterns in every word: the largest per-lane count of the packed prefix at K = 64
    s = cut(BGZF, b"A" * 4096, [1000])
    pl = Plain(BGZF, s)
    assert host_set(pl, [b"A"] * 64)[0].size == 262144
    check_batches(lib, mem, "4,096 x A, 64 copies", BGZF, s, pl, [([b"A"] * 64, None)], batches=(0,))


# ------------------------------------------------------------------------------------------------ 8. special bytes
def special_bytes(lib):
    """0x00, 0x7F, 0x80 and 0xFF as the first, the second and the q-th byte of patterns, q = 1, 2, 3 and 4, on random
    bytes."""
    mem = Mem(lib)
    for name, fmt, s, pl in line_cases.binary_streams():
        at = [pl.plain.find(bytes([b]), 8) for b in find_cases.SPECIAL]
        cut_out = lambda back, m: [pl.plain[p - back:p - back + m] for p in at]
        q4 = cut_out(0, 5) + cut_out(1, 5) + cut_out(3, 6)
        q3 = cut_out(0, 3) + cut_out(1, 4) + cut_out(2, 3)
        q2 = [bytes([b, b]) for b in find_cases.SPECIAL] + cut_out(1, 2) + cut_out(0, 7)
        q1 = [bytes([b]) for b in find_cases.SPECIAL] + cut_out(1, 3)
        for patterns in (q4, q3, q2[4:], q1):  # (a doubled byte need not occur)
            assert bool(np.all(host_set(pl, patterns)[3] >= 1))
        check_batches(lib, mem, name, fmt, s, pl, [(q4, None), (q3, 0x00), (q2, 0xFF), (q1, 0x80)], batches=(0, 20000, 1))


# ------------------------------------------------------------------------------------------------ 9. lines
def line_set(delim):
    d = bytes([delim])
    return [b"HIT", d + b"HIT", b"HIT" + d, d, d + d, b"a" + d + b"HIT" + d + b"b"]


def lines(lib):
    mem = Mem(lib)
    for delim in (NL, TAB):
        for terminated in (True, False):
            text, cross_at = find_cases.line_text(delim, terminated)
            patterns = line_set(delim)
            fmt = BGZF if terminated == (delim == NL) else MGZIP
            s = cut(fmt, text, [40, cross_at + 6, 6000], eof=fmt == BGZF and terminated)
            pl = Plain(fmt, s)
            pos, ids, hl, counts = host_set(pl, patterns, delim)
            ln = Lines(pl, delim)
            assert bool(np.all(counts >= 1)) and hl[ids == 0][0] == 0 and hl[ids == 0][-1] == ln.L - 1
            # the hit that starts in the carry of the member cut at cross_at + 6 (a batch boundary at batch 1), delimiters
            # in front of and behind its first byte
            assert cross_at + 3 in pos[ids == 5].tolist() and cross_at + 5 in pos[ids == 0].tolist()
            check_batches(lib, mem, "lines", fmt, s, pl, [(patterns, delim), (patterns[:3], NL + TAB - delim)],
                          route=ROUTES[delim == TAB], batches=(0, 20000, 1))


def lines_close_the_loop(lib):
    """find_set -> line_offsets_device: every hit lies in the line it was given."""
    mem = Mem(lib)
    text, cross_at = find_cases.line_text(NL, False)
    patterns = line_set(NL)
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, text, [40, cross_at + 6, 6000])
        with line_cases.Opened(lib, mem, fmt, s) as o:
            for batch in (0, 1):
                o.d.set_lines_batch(batch)
                n = o.d.find_set_device(o.ix, o.ptr, o.n, patterns)
                kp, pp = mem.put(b"\0" * 8 * n)
                kl, lp = mem.put(b"\0" * 8 * n)
                assert o.d.find_set_device(o.ix, o.ptr, o.n, patterns, NL, pp, None, lp, n) == n
                pos = np.frombuffer(mem.get(kp, 8 * n), dtype=np.uint64).astype(np.int64)
                ln = np.frombuffer(mem.get(kl, 8 * n), dtype=np.uint64).astype(np.int64)
                begin, end = o.offsets(ln).astype(np.int64), o.offsets(ln + 1).astype(np.int64)
                assert n > 20 and bool(np.all(begin <= pos)) and bool(np.all(pos < end))


# ------------------------------------------------------------------------------------------------ 10. capacity
def capacity(lib):
    mem = Mem(lib)
    text = find_cases.capacity_text()
    patterns = [b"HIT", b"qu", b"HIT\n", b"zz"]
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, text, [40, 5000])
        pl = Plain(fmt, s)
        pos, ids, lns, counts = host_set(pl, patterns, NL)
        n = pos.size
        assert n >= 8
        with Opened(lib, mem, fmt, s) as o:
            for batch in (0, 5000):
                o.d.set_lines_batch(batch)
                assert o.count(patterns, NL)[0] == n
                # (count only: hits_cap is ignored)
                assert o.d.find_set_device(o.ix, o.ptr, o.n, patterns, None, None, None, None, 3) == n
                # (piece_caps: at batch 0 they end the writing inside the second piece -- the workgroup's early return, the walk's
                # early out; at batch 5000 staging is laid out otherwise and they are two more values)
                for cap in [n, n + 3, n - 1, 1, 0] + find_cases.piece_caps(pos):
                    for subset in itertools.product((True, False), repeat=3):
                        if not any(subset):
                            continue
                        for with_counts in (True, False):
                            got, p, i, l, c = o.find_set(patterns, NL, cap, *subset, counts=with_counts)
                            what = (fmt, batch, cap, subset, with_counts)
                            if cap >= n:
                                assert got == n, what
                            else:
                                assert isinstance(got, _native.GzpxError), what
                                assert (got.code, got.needed) == (_native.ERR_INSUFFICIENT_SPACE, n), what
                            k = min(cap, n)
                            for arr, want, fill in ((p, pos, U64), (i, ids, U32), (l, lns, U64)):
                                if arr is not None:
                                    assert arr[:k].tolist() == want[:k].tolist(), what
                                    assert arr[k:].tolist() == [fill] * (cap + GUARD - k), (what, "written behind hits_cap")
                            if with_counts:
                                assert c.tolist() == counts.tolist() + [U64] * GUARD, what


# ------------------------------------------------------------------------------------------------ 11. errors
def raw_find_set(lib, o, blob, offsets, k, delim=-1, pos=None, ids=None, lines=None, cap=0, counts=None, n=None):
    off = (ctypes.c_uint32 * len(offsets))(*offsets)
    hits, info = ctypes.c_uint64(77), _native.GzpxCheckInfo()
    rc = lib.L.gzpx_find_set_device(o.d.h, o.ix.h, o.ptr, o.n if n is None else n, blob, off, k, delim, pos, ids, lines, cap, counts,
                                    ctypes.byref(hits), ctypes.byref(info), None)
    return rc, hits.value, info.block


def bad_sets():
    """(what, bytes, offsets, n_patterns) of every rule of the set that can be broken."""
    return [("n_patterns == 0", b"HIT", [0], 0),
            ("n_patterns == 257", b"ab" * 257, list(range(0, 516, 2)), 257),
            ("an empty pattern", b"HITqu", [0, 3, 3, 5], 3),
            ("a pattern of 257 bytes", b"HIT" + b"x" * 257, [0, 3, 260], 2),
            ("more bytes than the limit", b"x" * (MAXB + 128), list(range(0, MAXB + 129, 128)), MAXB // 128 + 1),
            ("offsets that decrease", b"HITqu", [0, 3, 2, 5], 3)]


def errors(lib):
    mem = Mem(lib)
    text, _ = find_cases.line_text(NL, True)
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, text, [40, 5000])
        with Opened(lib, mem, fmt, s) as o:
            keep, p = mem.put(bytes([FILL]) * 64)
            untouched = lambda: mem.get(keep, 64) == bytes([FILL]) * 64
            for what, blob, offsets, k in bad_sets():
                assert raw_find_set(lib, o, blob, offsets, k, NL, p, p, p, 2, p)[:2] == (INV, 0) and untouched(), (fmt, what)
            for what, got in (("delim 256", raw_find_set(lib, o, b"HIT", [0, 3], 1, 256, p, None, None, 2, p)),
                              ("delim -2", raw_find_set(lib, o, b"HIT", [0, 3], 1, -2, p, None, None, 2, p)),
                              ("d_lines without a delimiter", raw_find_set(lib, o, b"HIT", [0, 3], 1, -1, None, None, p, 2, p)),
                              ("fewer bytes than the index covers", raw_find_set(lib, o, b"HIT", [0, 3], 1, NL, p, p, p, 2, p, n=o.n - 1)),
                              ("no offsets", (lib.L.gzpx_find_set_device(o.d.h, o.ix.h, o.ptr, o.n, b"HIT", None, 1, -1, p, None, None, 2, p,
                                                                         ctypes.byref(ctypes.c_uint64(0)), None, None), 0))):
                assert got[:2] == (INV, 0) and untouched(), (fmt, what)
            with _native.DContext(format=BGZF + MGZIP - fmt, lib=lib) as d2:  # another context's index
                with pytest.raises(_native.GzpxError) as e:
                    d2.find_set_device(o.ix, o.ptr, o.n, [b"HIT"], d_counts_ptr=p)
                assert e.value.code == INV and e.value.needed is None and untouched()
            with pytest.raises(_native.GzpxError) as e:
                o.d.find_set_device(o.ix, o.ptr, o.n, [])
            assert e.value.code == INV
            # the limits themselves are served: a non-zero first offset, 256 patterns, 256 bytes, the delimiters 0 and 255
            assert raw_find_set(lib, o, b"..HIT", [2, 5], 1)[:2] == (_native.OK, per_pattern(Plain(fmt, s), b"HIT").size)
            assert o.count([b"HIT"] * MAXP)[0] == MAXP * o.count([b"HIT"])[0] > 0
            assert o.count([b"x" * 256, b"HIT"], 255)[0] == o.count([b"HIT"], 0)[0]


def damaged(lib):
    """A damaged member as find_cases.damaged: the inflate's error class, the member's index in the stream (two members a
    batch), n_hits = 0; the context serves on."""
    mem = Mem(lib)
    patterns = [b"e\n", b"qu", b"e"]
    for fmt in (BGZF, MGZIP):
        text = short_lines(8 * 10000, 11)
        s = cut(fmt, text, [10000 * i for i in range(1, 8)])
        pl = Plain(fmt, s)
        keep0, ptr0 = mem.put(s)
        for route in ROUTES:
            with _native.DContext(format=fmt, lib=lib) as d:
                d.set_route(route)
                d.set_lines_batch(22000)
                for victim in (0, 3, 7):
                    for what, at, code in (("crc", pl.off[victim] + pl.size[victim] - 8, _native.ERR_INVALID_CHECK),
                                           ("block type", pl.off[victim] + HDR[fmt], _native.ERR_BAD_DATA)):
                        m = bytearray(s)
                        if what == "crc":
                            m[at] ^= 0xFF
                        else:
                            m[at] |= 0x06  # BTYPE = 3, reserved
                        keep, ptr = mem.put(m)
                        kp, pp = mem.put(b"\0" * 8 * 64)
                        kc, cp = mem.put(b"\0" * 8 * 3)
                        with d.build_index_device(ptr, len(m)) as ix:
                            with pytest.raises(_native.GzpxError) as e:
                                d.find_set_device(ix, ptr, len(m), patterns, NL, pp, None, None, 64, cp)
                            assert (e.value.code, e.value.block, e.value.needed) == (code, victim, None), (fmt, route, victim, what)
                            bad = type("O", (), dict(d=d, ix=ix, ptr=ptr, n=len(m)))
                            assert raw_find_set(lib, bad, b"eqe", [0, 1, 2, 3], 3) == (code, 0, victim), (fmt, route, victim, what)
                with d.build_index_device(ptr0, len(s)) as ix0:  # the context serves on
                    assert d.find_set_device(ix0, ptr0, len(s), patterns) == host_set(pl, patterns)[0].size


# ------------------------------------------------------------------------------------------------ 12. selection by a set
class Selected(select_cases.Opened):
    def count(self, patterns, g=1, invert=False):
        return self.d.select_lines_set_device(self.ix, self.lt, self.ptr, self.n, patterns, g, invert)

    def select(self, patterns, g, invert, cap):
        room = (cap + GUARD) * 16
        keep, p = self.mem.put(bytes([FILL]) * room)
        self.table = keep  # (the table stays where it is for read_lines_table_device)
        try:
            got = self.d.select_lines_set_device(self.ix, self.lt, self.ptr, self.n, patterns, g, invert, p, cap)
        except _native.GzpxError as e:
            got = e
        return got, np.frombuffer(self.mem.get(keep, room), dtype=np.uint64).reshape(-1, 2).tolist(), p


def select_sets(delim):
    d = bytes([delim])
    forty = [b"HIT"] + [bytes([ord("a") + j % 26, ord("a") + (7 * j) % 26, ord("a") + (3 * j) % 26]) for j in range(39)]
    return [[b"HIT"], [b"HIT" + d, b"another", d + d], forty]


def selection(lib):
    """Sets of 1, 3 (one pattern holds the delimiter, one is two delimiters) and 40 patterns; group 1 and 4, plain and
    inverted; a table one entry short; the device table read by read_lines_table_device."""
    mem = Mem(lib)
    i = 0
    for delim in (NL, TAB):
        for terminated in (True, False):
            text, cross_at = find_cases.line_text(delim, terminated)
            fmt = BGZF if terminated == (delim == NL) else MGZIP
            s = cut(fmt, text, [40, cross_at + 6, 6000], eof=fmt == BGZF and terminated)
            pl = Plain(fmt, s)
            ln = Lines(pl, delim)
            all_lines = [pl.plain[int(ln.start[k]):int(ln.start[k + 1])] for k in range(ln.L)]
            with Selected(lib, mem, fmt, s, delim, ROUTES[i % 2]) as o:
                for batch in (0, 1):
                    o.d.set_lines_batch(batch)
                    for patterns in select_sets(delim):
                        for g in (1, 4):
                            for invert in (False, True):
                                what = (fmt, delim, terminated, batch, len(patterns), g, invert)
                                runs, records, hits = host_select_set(pl, ln, delim, patterns, g, invert)
                                if len(patterns) == 1:  # the host's result for the single pattern
                                    assert (runs, records, hits) == select_cases.host_select(pl, ln, delim, patterns[0], g, invert)
                                assert len(runs) >= 2, what
                                assert o.count(patterns, g, invert) == (len(runs), records, hits), (what, "count only")
                                got, table, _ = o.select(patterns, g, invert, len(runs) - 1)
                                assert isinstance(got, _native.GzpxError), what
                                assert (got.code, got.needed) == (_native.ERR_INSUFFICIENT_SPACE, len(runs)), what
                                assert table == [list(r) for r in runs[:-1]] + [[U64, U64]] * GUARD, (what, "one short")
                                got, table, rp = o.select(patterns, g, invert, len(runs))
                                assert got == (len(runs), records, hits), (what, got)
                                assert table == [list(r) for r in runs] + [[U64, U64]] * GUARD, (what, "runs")
                                assert all(t >= 0.0 for t in o.d.last_select_ms())
                                want = b"".join(b"".join(all_lines[a:b]) for a, b in runs)
                                keep, p = mem.put(bytes([FILL]) * (len(want) + 64), shift=5)
                                assert o.d.read_lines_table_device(o.ix, o.lt, o.ptr, o.n, rp, len(runs), p, len(want)) == len(want)
                                assert mem.get(keep, len(want) + 64 + 5)[5:] == want + bytes([FILL]) * 64, (what, "bytes")
            i += 1


def raw_select_set(lib, o, blob, offsets, k, g=1, flags=0, d_runs=None, cap=0, n=None):
    off = (ctypes.c_uint32 * len(offsets))(*offsets)
    runs, records, hits, info = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint64(77), _native.GzpxCheckInfo()
    rc = lib.L.gzpx_select_lines_set_device(o.d.h, o.ix.h, o.lt.h, o.ptr, o.n if n is None else n, blob, off, k, g, flags, d_runs, cap,
                                            ctypes.byref(runs), ctypes.byref(records), ctypes.byref(hits), ctypes.byref(info), None)
    return rc, runs.value, records.value, hits.value


def selection_errors(lib):
    mem = Mem(lib)
    text, _ = find_cases.line_text(NL, True)
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, text, [40, 5000])
        with Selected(lib, mem, fmt, s) as o:
            keep, p = mem.put(bytes([FILL]) * 64)
            cases = [(what, raw_select_set(lib, o, blob, offsets, k, 1, 0, p, 4)) for what, blob, offsets, k in bad_sets()]
            cases += [("group == 0", raw_select_set(lib, o, b"HIT", [0, 3], 1, 0, 0, p, 4)),
                      ("a flag that is not defined", raw_select_set(lib, o, b"HIT", [0, 3], 1, 1, 2, p, 4)),
                      ("a flag that is not defined, with INVERT", raw_select_set(lib, o, b"HIT", [0, 3], 1, 1, 0x80000001, p, 4)),
                      ("fewer bytes than the index covers", raw_select_set(lib, o, b"HIT", [0, 3], 1, 1, 0, p, 4, n=o.n - 1))]
            for what, got in cases:
                assert got == (INV, 0, 0, 0), (fmt, what, got)
                assert mem.get(keep, 64) == bytes([FILL]) * 64, (fmt, what)
            with _native.DContext(format=BGZF + MGZIP - fmt, lib=lib) as d2:
                with pytest.raises(_native.GzpxError) as e:
                    d2.select_lines_set_device(o.ix, o.lt, o.ptr, o.n, [b"HIT"])
                assert e.value.code == INV
        # every m_k > n: nothing is inflated; plain no run, inverted the one run {0, L}
        s2 = cut(fmt, b"ab\ncd", [1])
        with Selected(lib, mem, fmt, s2) as o:
            long_set = [b"x" * 6, b"y" * 256]
            assert o.count(long_set) == (0, 0, 0) and o.select(long_set, 1, False, 2)[:2] == ((0, 0, 0), [[U64] * 2] * (2 + GUARD))
            assert o.count(long_set, 1, True) == (1, 2, 0) and o.count(long_set, 5, True) == (1, 1, 0)
            got, table, _ = o.select(long_set, 1, True, 1)
            assert got == (1, 2, 0) and table == [[0, 2]] + [[U64] * 2] * GUARD
            assert o.d.last_select_ms() == (0.0, 0.0, 0.0)
            assert o.count([b"x" * 6, b"cd"]) == (1, 1, 1)  # one pattern fits: the stream is searched for it


def selection_damaged(lib):
    mem = Mem(lib)
    for fmt in (BGZF, MGZIP):
        text = short_lines(4 * 5000, 11)
        s = cut(fmt, text, [5000 * i for i in range(1, 4)])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        with Selected(lib, mem, fmt, s, route=ROUTES[fmt == MGZIP], batch=11000) as o:
            for victim in (0, 3):
                m = bytearray(s)
                m[pl.off[victim] + pl.size[victim] - 8] ^= 0xFF
                keep, ptr = mem.put(m)
                kr, rp = mem.put(b"\0" * 16 * 64)
                with o.d.build_index_device(ptr, len(m)) as ix:
                    with pytest.raises(_native.GzpxError) as e:
                        o.d.select_lines_set_device(ix, o.lt, ptr, len(m), [b"e\n", b"qu"], 2, False, rp, 64)
                    assert (e.value.code, e.value.block, e.value.needed) == (_native.ERR_INVALID_CHECK, victim, None), (fmt, victim)
            runs, records, hits = host_select_set(pl, ln, NL, [b"e\n", b"qu"], 2, False)
            assert o.count([b"e\n", b"qu"], 2) == (len(runs), records, hits)
