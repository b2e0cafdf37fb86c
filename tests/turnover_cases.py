"""k_mparse at the turn of a pass and of a block, written once and run twice: through the emulated library on CPU
(tests/test_emu_turnover.py) and through the real HIP library on the MI355X (tests/test_gpu_turnover.py).

The kernel keeps three things in flight across its phases -- the next pass's d0, the next block's bytes and the ticket for
the block after the next -- and waits for them at one place, in front of a pass's token stores.  Every way to the top of
a pass or of a block has to have gone through such a wait, and a block that does not get as far as its last pass's
token build (handed back, or stored-only) requests and waits late.  The shapes here are the ones that reach a pass
top or a block top by every one of those ways.

The check: BGZF, level 1, compat 1.24, the whole stream byte for byte against oracle.compress_stream -- once as the
library runs, once with Config.debug bit 3 (a search at every position).  Where a generator is built for a property it
asserts it, with the numpy restatement of the level-1 table in tools/sim_mparse_skip.py (buckets, d0_of, Block)."""
import numpy as np

import l1_skip_cases as skip
import scan_cases
from gzp_amd import _native, synth

sim = skip.sim
HALF = 32768
SINGLE, THREE, FULL = 32768, 32771, 65280  # buffer sizes: one pass; a second pass of three positions; two full passes
PASSTHROUGH = 51  # a block of at most this many bytes is stored, never parsed (level 1)
NO_STEP = 8  # Config.debug bit 3
FLAGS = (0, NO_STEP)
EMU_CUS = 3


def text(n, seed):
    return synth.english_like(n, seed).copy()


def blocks_on(on_gpu):
    """More than two blocks per workgroup, so that every workgroup draws tickets: 3 x 256 + 5 on the MI355X's 256 CUs,
    10 on the emulator's three."""
    return 3 * 256 + 5 if on_gpu else 3 * EMU_CUS + 1


# ------------------------------------------------------------------------------------------------ the cases: (name, data, buffer_size)
def single_pass(on_gpu):
    """Blocks of one pass: that pass is the last, the successor's d0 and the ticket are requested in it."""
    assert SINGLE <= HALF
    return [("%d blocks of %d" % (k, SINGLE), text(k * SINGLE, 400 + k), SINGLE) for k in (1, 2, 7)] + \
           [("4 blocks of %d and one of 9000" % SINGLE, text(4 * SINGLE + 9000, 410), SINGLE)]


def short_second_pass(on_gpu):
    """A second pass of three positions: a single segment, three literals or the tail of a match, and no search."""
    assert THREE - HALF == 3
    return [("%d blocks of %d" % (k, THREE), text(k * THREE, 420 + k), THREE) for k in (1, 2, 7)]


def two_passes(on_gpu):
    """Full blocks of two passes."""
    assert HALF < FULL <= 2 * HALF
    return [("%d blocks of %d" % (k, FULL), text(k * FULL, 430 + k), FULL) for k in (1, 2, 4)] + \
           [("2 blocks of %d and one of %d" % (FULL, HALF + 1), text(2 * FULL + HALF + 1, 440), FULL)]


def claimed(on_gpu):
    """Every workgroup takes more than two blocks: the third and every later one is a ticket's."""
    k = blocks_on(on_gpu)
    return [("%d blocks of %d" % (k, THREE), text(k * THREE, 450), THREE),
            ("%d blocks of %d" % (k // 2 + 2, FULL), text((k // 2 + 2) * FULL, 451), FULL)]


def stored_last(on_gpu):
    """The slab ends in a block that is stored, not parsed: alone, as a workgroup's first block, as its second, and as
    one it has drawn a ticket for."""
    out = [("one block of 40", text(40, 460), FULL), ("one block of %d" % PASSTHROUGH, text(PASSTHROUGH, 461), SINGLE)]
    k = blocks_on(on_gpu)
    for bs in (SINGLE, THREE, FULL):
        for blocks, tail in ((1, 1), (2, PASSTHROUGH), (k, 40)):
            assert tail <= PASSTHROUGH
            out.append(("%d blocks of %d and one of %d" % (blocks, bs, tail), text(blocks * bs + tail, 462 + blocks), bs))
    # ... and the shortest block that is parsed, behind the same
    out.append(("%d blocks of %d and one of %d" % (k, THREE, PASSTHROUGH + 1), text(k * THREE + PASSTHROUGH + 1, 470), THREE))
    return out


def _mixed(bs, blocks, seed):
    """Blocks of text with blocks between them that k_mparse hands back: zeros and byte runs (in their first pass) and,
    where a block has two passes, text whose second half is zeros (in its second)."""
    a = text(blocks * bs, seed)
    kinds = []
    for k in range(blocks):
        kind = ("text", "text", "zeros", "text", "late", "runs", "zeros", "text")[k % 8]
        lo = k * bs
        if kind == "zeros":
            a[lo:lo + bs] = 0
        elif kind == "runs":
            a[lo:lo + bs] = synth.byte_runs(bs, seed + k)
        elif kind == "late" and bs > HALF + 4096:
            a[lo + HALF + 2048:lo + bs] = 0
        kinds.append(kind)
    assert {"text", "zeros", "runs", "late"} <= set(kinds)
    return a


def handbacks_among_text(on_gpu):
    k = blocks_on(on_gpu)
    return [("%d mixed blocks of %d" % (k, THREE), _mixed(THREE, k, 480), THREE),
            ("%d mixed blocks of %d" % (k // 2 + 2, FULL), _mixed(FULL, k // 2 + 2, 481), FULL),
            ("8 mixed blocks of %d" % SINGLE, _mixed(SINGLE, 8, 482), SINGLE)]


def older_in_first_half(on_gpu=False):
    """The gather out of global memory: a token of the second pass whose newer candidate lies in the first half, so that
    the older one's distance is not in LDS.  A phrase at A, its first six bytes again at B (both in the first half) and
    the whole phrase at C in the second half: at C the newer candidate B matches six bytes and the older one, A, all
    of them."""
    rng = np.random.default_rng(490)
    a = text(FULL, 491)
    A, B, C, plen = 30000, 32000, 33000, 24
    for p in (A, B, C):  # bytes that occur once each: no match crosses into a phrase
        a[p - 1] = 0xF0 + (p // 1000) % 8
    skip.splice_unique(a, A, plen, rng)
    skip.splice_unique(a, B, plen, rng)
    a[B:B + 6] = a[A:A + 6]
    a[C:C + plen] = a[A:A + plen]
    a[C + plen] = 0xFF
    blk = sim.Block(a)
    starts, lens = blk.parse()
    tokens = dict(zip(starts, lens))
    d0 = blk.d0
    assert B < HALF <= C and d0[C] == C - B and d0[B] == B - A  # the newer candidate lies before the pass; the older one is A
    assert blk._extend(C, B, 258) == 6 and blk._extend(C, A, 258) == plen  # ... and wins
    assert tokens.get(C) == plen, tokens.get(C)  # the parse starts a token there
    # (text has such positions of its own, where the newer candidate wins or none does)
    second = [p for p in starts if p >= HALF and d0[p] and p - d0[p] < HALF and d0[p - d0[p]]]
    assert len(second) > 1 and C in second
    two_blocks = np.concatenate([a, a])  # ... and once more in a block that is not the slab's first
    return [("older candidate in the first half", a, FULL), ("older candidate in the first half, twice", two_blocks, FULL)]


GROUPS = {
    "single_pass": single_pass,
    "short_second_pass": short_second_pass,
    "two_passes": two_passes,
    "claimed": claimed,
    "stored_last": stored_last,
    "handbacks_among_text": handbacks_among_text,
    "older_in_first_half": older_in_first_half,
}


# ------------------------------------------------------------------------------------------------ the check
def check(lib, oracle, group):
    mem = scan_cases.Mem(lib)
    cases = GROUPS[group](mem.on_gpu)
    biggest = max(data.size for _, data, _ in cases)
    for bs in sorted({bs for _, _, bs in cases}):
        ctxs = [(flags, _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=bs, compat=_native.COMPAT_1_24,
                                        max_slab_bytes=biggest, lib=lib)) for flags in FLAGS]
        try:
            for flags, ctx in ctxs:
                ctx.debug_set_flags(flags)
            for name, data, case_bs in cases:
                if case_bs != bs:
                    continue
                want = oracle.compress_stream(data, oracle.FMT_BGZF, 1, oracle.COMPAT_1_24, bs)
                for flags, ctx in ctxs:
                    got = ctx.compress_slab(data, is_last=True)
                    assert got == want, (name, "debug flags %d" % flags, len(got), len(want))
                    if group == "handbacks_among_text":
                        assert ctx.debug_redo_count() > 0, (name, "nothing was handed back")
        finally:
            for _, ctx in ctxs:
                ctx.close()
