"""k_candidates' two bodies for an iteration -- the interior one without clamps and per-position tests, and the clamped
one -- written once and run twice: through the emulated library on CPU (tests/test_emu_cand.py, where a device pointer
is a host pointer) and through the real HIP library on the MI355X (tests/test_gpu_cand.py).

The check: BGZF, compat 1.24, the whole stream byte for byte against oracle.compress_stream, at level 1 (MODE 0) and at
level 3 (MODES 1-3), three times each: as the library runs, with Config.debug bit 7 (every iteration through the clamped
body) and with Config.debug bit 0 (the order-independent fallback on every block).

An iteration is 1,024 positions (16 steps of 64 lanes); it is interior when it is not the block's first and
base0 + 1040 <= n.  The shapes are the smallest at which each thing can go wrong: block lengths around that choice,
block bases and input pointers at every residue mod 4, slabs of more blocks than the device has CUs (a workgroup
carries its position base, its turn counter and a wave's first turn of the next block from block to block), and
contents whose equal buckets meet inside one atomic instruction.  Where a generator is built for such a property it
asserts it, with the numpy restatement of the level-1 table in tools/sim_mparse_skip.py (buckets, d0_of)."""
import os
import sys

import numpy as np

import scan_cases
from checksum_cases import put_aligned
from gzp_amd import _native, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import sim_mparse_skip as sim  # noqa: E402

BLOCK = 65280
ITER = 1024  # positions per iteration
MARGIN = 16  # an interior iteration has base0 + ITER + MARGIN <= n
CLAMP_ALL = 128  # Config.debug bit 7
FALLBACK = 1  # Config.debug bit 0
FLAGS = (0, CLAMP_ALL, FALLBACK)
LEVELS = (1, 3)


def interior_iterations(n):
    """The iterations of a block of n bytes that take the interior body."""
    return [it for it in range(1, -(-n // ITER)) if it * ITER + ITER + MARGIN <= n]


# ------------------------------------------------------------------------------------------------ contents
def text(n, seed):
    return synth.english_like(n, seed).copy()


def periodic(n, period, seed):
    unit = np.random.default_rng(seed).integers(0, 256, period, dtype=np.uint8)
    return np.tile(unit, -(-n // period))[:n].copy()


def shared_in_instruction(a, it):
    """Every atomic instruction (64 consecutive positions) of iteration `it` has lanes that share a bucket, and the
    predecessor of such a lane sits in the same instruction."""
    h, d0 = sim.buckets(a), sim.d0_of(a)
    for k in range(ITER // 64):
        lo = it * ITER + 64 * k
        grp = h[lo:lo + 64]
        if grp.size < 64 or np.unique(grp).size == 64:
            return False
        lanes = np.arange(64)
        if not ((d0[lo:lo + 64] > 0) & (d0[lo:lo + 64] <= lanes)).any():
            return False
    return True


# ------------------------------------------------------------------------------------------------ the cases
# (name, data, buffer_size, lead): lead None = a host slab; 0..3 = a device slab whose first byte lies that many
# bytes behind a 16-byte boundary
def block_lengths(on_gpu=False):
    """Single blocks around the choice of body: 52 is the shortest parsed block; around 1040 there is the margin but
    only a first iteration, which is never interior; 2064 = 1024 + 1040 is the shortest block with an interior
    iteration and 3 * 1024 + 16 the shortest with two."""
    lengths = (52, 1024, 1039, 1040, 1041, 2063, 2064, 2065, 3 * 1024 + 15, 3 * 1024 + 16, 3 * 1024 + 17, 65279, 65280)
    assert interior_iterations(1041) == [] and interior_iterations(2063) == [] and interior_iterations(2064) == [1]
    assert interior_iterations(3 * 1024 + 15) == [1] and interior_iterations(3 * 1024 + 16) == [1, 2]
    assert interior_iterations(65280) == list(range(1, 63))  # of a full block's 64, the first and the last are clamped
    return [("text %d" % n, text(n, 300 + k), BLOCK, None) for k, n in enumerate(lengths)]


def alignment(on_gpu=False):
    """Block bases at every residue mod 4 (buffer_size not divisible by four), and the input pointer advanced by 1-3."""
    out = []
    for bs, blocks in ((32771, 5), (65279, 5)):
        assert bs % 4 == 3 and len(interior_iterations(bs)) >= 2
        n = (blocks - 1) * bs + bs // 2 + 1500
        assert {(b * bs) % 4 for b in range(blocks)} == {0, 1, 2, 3}
        out.append(("text, buffer_size %d, %d blocks" % (bs, blocks), text(n, 320 + blocks), bs, None))
    for lead in (0, 1, 2, 3):
        out.append(("text, pointer + %d" % lead, text(BLOCK + 7000 + lead, 330 + lead), BLOCK, lead))
        out.append(("text, pointer + %d, buffer_size 32771" % lead, text(2 * 32771 + 3000, 340 + lead), 32771, lead))
    return out


def carry_over(on_gpu):
    """More blocks than the device has CUs, so that every workgroup walks several blocks without clearing the table:
    300 on the MI355X (256 CUs) and 10 in the emulator (three CUs, and a few hundred KB a second).
    buffer_size is 32771, close to the smallest the library takes (32768) and no multiple of four: 33 turns a block,
    so wave 0 takes three turns in a block and the others two, a fast wave starts the next block while the rest
    finish the old one, and the bases cycle through all four alignments along a workgroup's walk.  The slab cut gives every block but the last buffer_size bytes, so a block without
    turns (at most `passthrough` bytes: 51 at level 1, 43 at level 3) is always a slab's last: the second slab ends
    with one, which the workgroup that owns it has to step over, and the third with a block of one clamped iteration."""
    bs, blocks = 32771, 300 if on_gpu else 10
    assert len(interior_iterations(bs)) == 30 and -(-bs // ITER) == 33
    return [("%d blocks of %d" % (blocks, bs), text(blocks * bs, 350), bs, None),
            ("%d blocks of %d and one of 40" % (blocks, bs), text(blocks * bs + 40, 352), bs, None),
            ("%d blocks of %d and one of 1000" % (blocks, bs), text(blocks * bs + 1000, 353), bs, None)]


def lane_order(on_gpu=False):
    """Contents whose equal buckets meet inside one atomic instruction, or in the same lane of the next."""
    n = 5 * ITER + 100
    out = []
    a = np.zeros(n, dtype=np.uint8)
    assert shared_in_instruction(a, 1) and shared_in_instruction(a, 3)
    out.append(("zeros", a, BLOCK, None))
    for period in (2, 63, 64, 65):
        a = periodic(n, period, 360 + period)
        d0 = sim.d0_of(a)
        its = interior_iterations(n)
        assert its == [1, 2, 3, 4]
        # the predecessor is one period back: the same instruction (2, and lanes >= 63 of 63), the lane's own slot in
        # the instruction before (64), or its neighbour's (63, 65)
        assert (d0[ITER:4 * ITER] == period).all(), period
        if period == 2:
            assert shared_in_instruction(a, 1)
        out.append(("period %d" % period, a, BLOCK, None))
    # one bucket twice in one instruction of an interior iteration, in the middle of text: lanes 3 and 40 of step 5
    a = text(n, 370)
    first, second = 2 * ITER + 64 * 5 + 3, 2 * ITER + 64 * 5 + 40
    word = np.array([0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8], dtype=np.uint8)
    a[first:first + 8] = word
    a[second:second + 8] = word
    h, d0 = sim.buckets(a), sim.d0_of(a)
    assert 2 in interior_iterations(n) and first // 64 == second // 64
    assert h[first] == h[second] and d0[second] == second - first
    out.append(("a phrase twice in one instruction", a, BLOCK, None))
    out.append(("repeated phrases", synth.repeated_phrases(2 * BLOCK, 7).copy(), BLOCK, None))
    out.append(("english_like", text(BLOCK + 4 * ITER, 371), BLOCK, None))
    out.append(("random", np.random.default_rng(372).integers(0, 256, BLOCK + 4 * ITER, dtype=np.uint8), BLOCK, None))
    out.append(("byte runs", synth.byte_runs(2 * BLOCK, 4).copy(), BLOCK, None))
    return out


GROUPS = {
    "block_lengths": block_lengths,
    "alignment": alignment,
    "carry_over": carry_over,
    "lane_order": lane_order,
}


# ------------------------------------------------------------------------------------------------ the check
def check(lib, oracle, group):
    mem = scan_cases.Mem(lib)
    cases = GROUPS[group](mem.on_gpu)
    biggest = max(data.size for _, data, _, _ in cases)
    for level in LEVELS:
        for bs in sorted({bs for _, _, bs, _ in cases}):
            ctxs = [(flags, _native.Context(format=_native.FORMAT_BGZF, level=level, buffer_size=bs, compat=_native.COMPAT_1_24,
                                            max_slab_bytes=biggest, lib=lib)) for flags in FLAGS]
            try:
                for flags, ctx in ctxs:
                    ctx.debug_set_flags(flags)
                for name, data, case_bs, lead in cases:
                    if case_bs != bs:
                        continue
                    want = oracle.compress_stream(data, oracle.FMT_BGZF, level, oracle.COMPAT_1_24, bs)
                    if lead is not None:
                        h_in, d_in = put_aligned(mem, data.tobytes(), lead)
                        assert d_in % 4 == lead
                        cap = ctxs[0][1].slab_bound(data.size)
                        h_out, d_out = mem.empty(cap)
                    for flags, ctx in ctxs:
                        if lead is None:
                            got = ctx.compress_slab(data, is_last=True)
                        else:
                            out_len, _ = ctx.compress_slab_device(d_in, data.size, d_out, cap, True)
                            got = mem.get(h_out, out_len)
                        assert got == want, (name, "level %d" % level, "debug flags %d" % flags, len(got), len(want))
            finally:
                for _, ctx in ctxs:
                    ctx.close()
