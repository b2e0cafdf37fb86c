"""k_mparse's step over positions that have no hash candidate, written once and run twice: through the emulated
library on CPU (tests/test_emu_l1_skip.py) and through the real HIP library on the MI355X (tests/test_gpu_l1_skip.py).

The check: BGZF, level 1, compat 1.24, the whole stream byte for byte against oracle.compress_stream -- once as the
library runs, once with Config.debug bit 3 (a search at every position, the walk without the step).  The inputs are
single blocks or slabs of at most three blocks, built so that candidate-less runs meet everything the walk knows of:
whole segments, the segment and pass boundaries, the positions near a block's end that are never searched, a corrected
entry that lands inside a run the guessed walk has marked, and the hand-back of long runs to the dense kernels.  Every
generator asserts the property it is there for, with the numpy restatement of the level-1 table in
tools/sim_mparse_skip.py (lz_hash15, position 0 filed under bucket 0)."""
import os
import sys

import numpy as np

from gzp_amd import _native, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import sim_mparse_skip as sim  # noqa: E402

BLOCK = 65280
SEG, HALF = 32, 32768
NO_STEP = 8  # Config.debug bit 3


# ------------------------------------------------------------------------------------------------ building blocks
def _used_buckets(a, lo, hi):
    """Buckets taken by the windows of `a` that do not touch [lo, hi) (+ bucket 0, where position 0 is filed)."""
    used = np.zeros(32768, dtype=bool)
    used[0] = True
    if len(a) >= 4:
        h = sim.lz_hash15(sim.windows(a)).astype(np.int64)
        q = np.arange(h.size)
        used[h[(q + 3 < lo) | (q >= hi)]] = True
    return used


def splice_unique(a, s, length, rng, lo=0x80, hi=0xF0):
    """Overwrite a[s : s + length] with bytes of [lo, hi) chosen by rejection so that every four-byte window that
    touches them has a bucket no other window of `a` has, and not bucket 0."""
    n = len(a)
    for _ in range(200):
        used = _used_buckets(a, s, s + length)
        ok = True
        for i in range(length):
            p = s + i
            # the windows whose last spliced byte is this one
            qs = [p - 3] if i < length - 1 else list(range(p - 3, p + 1))
            qs = [q for q in qs if q >= 0 and q + 4 <= n]
            for b in rng.permutation(np.arange(lo, hi)):
                a[p] = b
                hs = [int(sim.lz_hash15(int.from_bytes(a[q:q + 4].tobytes(), "little"))) for q in qs]
                if len(set(hs)) == len(hs) and not any(used[h] for h in hs):
                    used[hs] = True
                    break
            else:
                ok = False
                break
        if ok:
            return
    raise AssertionError("no candidate-less run of %d bytes at %d" % (length, s))


def candidate_less(a, lo, hi):
    """Positions [lo, hi) have no candidate (or are never searched)."""
    d0 = sim.d0_of(a)
    return not d0[max(lo, 0):min(hi, len(a))].any()


def unique_block(n, seed):
    """n bytes in which no 15-bit hash of four bytes occurs twice: every position is candidate-less."""
    rng = np.random.default_rng(seed)
    a = np.zeros(n, dtype=np.uint8)
    splice_unique(a, 0, n, rng, lo=0, hi=256)
    h = sim.buckets(a)
    assert np.unique(h).size == h.size and not (h[1:] == 0).any()
    assert candidate_less(a, 0, n)
    return a


def text(n, seed):
    a = synth.english_like(n, seed).copy()
    assert a.max() < 0x80
    return a


# ------------------------------------------------------------------------------------------------ the cases
def all_candidate_less():
    # 52: the shortest block that is parsed (passthrough is 51 at level 1)
    return [("candidate-less %d" % n, unique_block(n, 100 + n)) for n in (52, 4096, 20000)]


def runs_against_geometry():
    """Runs of 1, 31, 32, 33, 64 and 100 bytes starting at offsets 0, 1 and 31 of a segment, and one over the pass
    boundary at 32,768, in one block of text."""
    rng = np.random.default_rng(7)
    a = text(BLOCK, 21)
    spots = []
    k = 0
    for length in (1, 31, 32, 33, 64, 100):
        for off in (0, 1, 31):
            s = 2048 + 1024 * k + off
            assert s % SEG == off and s + length < 32700
            spots.append((s, length))
            k += 1
    spots.append((32760, 16))  # positions 32,760-32,775
    assert spots[-1][0] < HALF < spots[-1][0] + spots[-1][1]
    spots.append((40000, 70))  # ... and one in the second pass
    for s, length in spots:
        splice_unique(a, s, length, rng)
    for s, length in spots:  # every window that holds a spliced byte
        assert candidate_less(a, s - 3, s + length), (s, length)
    return [("runs against the segments", a)]


def runs_at_the_end():
    """A run whose last byte is at n - 6, n - 5, n - 4, n - 1: around the last searched position, n - 5."""
    out = []
    for back in (6, 5, 4, 1):
        rng = np.random.default_rng(30 + back)
        n = 40000 + back
        a = text(n, 40 + back)
        s = n - back - 39
        splice_unique(a, s, 40, rng)
        assert s + 40 - 1 == n - back and candidate_less(a, s - 3, n - back + 1)
        out.append(("run ends at n - %d" % back, a))
    return out


def merge_inside_a_run():
    """A phrase of 40-70 bytes a second time, so that its match crosses a segment boundary and ends at offset 1, 15, 31
    of the segment, with a candidate-less run directly behind: the last three positions of the phrase are part of the
    run (their windows reach into it), the guessed walk marks it from there or from the segment's start, and the
    corrected entry -- the match's end -- lands inside it.  Last: a run of ONE byte, the entry on its last position."""
    rng = np.random.default_rng(9)
    a = text(BLOCK, 55)
    marker = iter(range(0xF0, 0x100))  # bytes that occur once each: no match crosses them
    plan = []
    for k, (end_off, plen, rlen) in enumerate(((1, 40, 8), (15, 57, 23), (31, 70, 40), (15, 48, 1))):
        first = 3000 + 2000 * k
        a[first - 1] = next(marker)
        splice_unique(a, first, plen, rng)
        a[first + plen] = next(marker)
        end = SEG * (400 + 60 * k) + end_off  # where the second copy's match ends
        second = end - plen
        a[second - 1] = next(marker)
        a[second:end] = a[first:first + plen]
        if rlen == 1:  # ... and a candidate directly behind it: text that was seen before
            a[end + 1:end + 41] = a[200:240]
        splice_unique(a, end, rlen, rng)
        plan.append((second, end, plen, rlen))
    blk = sim.Block(a)
    starts, lens = blk.parse()
    tokens = dict(zip(starts, lens))
    for second, end, plen, rlen in plan:
        assert tokens.get(second) == plen, (second, plen, tokens.get(second))  # one match, the whole phrase
        assert second // SEG < end // SEG and end in tokens  # it crosses a boundary; the parse enters the segment at `end`
        assert candidate_less(a, end - 3, end + rlen)
        if rlen == 1:
            assert blk.d0[end + 1] != 0
    return [("merge inside a run", a)]


def block_lengths():
    out = [("text %d" % n, text(n, 60 + k)) for k, n in enumerate((53, 63, 64, 65, 32767, 32768, 32769, 65279, 65280))]
    out.append(("three blocks, the last of 52", text(2 * BLOCK + 52, 80)))
    out.append(("three blocks, the last of 51 (stored)", text(2 * BLOCK + 51, 81)))
    return out


def synth_classes():
    return [("class %s" % cls, synth.make(cls, 2 * BLOCK, 3)) for cls in sorted(synth.CLASSES)]


GROUPS = {
    "all_candidate_less": all_candidate_less,
    "runs_against_geometry": runs_against_geometry,
    "runs_at_the_end": runs_at_the_end,
    "merge_inside_a_run": merge_inside_a_run,
    "block_lengths": block_lengths,
    "synth_classes": synth_classes,
}


# ------------------------------------------------------------------------------------------------ the check
def check(lib, oracle, group):
    cases = GROUPS[group]()
    ctxs = [(flags, _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=BLOCK, compat=_native.COMPAT_1_24,
                                    max_slab_bytes=3 * BLOCK, lib=lib)) for flags in (0, NO_STEP)]
    try:
        for flags, ctx in ctxs:
            ctx.debug_set_flags(flags)
        for name, data in cases:
            assert 0 < data.size <= 3 * BLOCK
            want = oracle.compress_stream(data, oracle.FMT_BGZF, 1, oracle.COMPAT_1_24, BLOCK)
            for flags, ctx in ctxs:
                got = ctx.compress_slab(data, is_last=True)
                assert got == want, (name, "debug flags %d" % flags, len(got), len(want))
    finally:
        for _, ctx in ctxs:
            ctx.close()


def handed_back(lib):
    """The long runs of the `runs` and `zeros` classes still leave k_mparse for the dense kernels."""
    with _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=BLOCK, compat=_native.COMPAT_1_24,
                         max_slab_bytes=2 * BLOCK, lib=lib) as ctx:
        for cls in ("runs", "zeros"):
            ctx.compress_slab(synth.make(cls, 2 * BLOCK, 3), is_last=True)
            assert ctx.debug_redo_count() > 0, cls
