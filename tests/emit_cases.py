"""k_emit's token loop and k_hist, written once and run twice: through the emulated library on CPU
(tests/test_emu_emit.py) and through the real HIP library on the MI355X (tests/test_gpu_emit.py).

The check: the whole stream byte for byte against oracle.compress_stream.  Every case is at most three blocks, or one
Mgzip block of at most 256 KiB.  The inputs are built for what the two token consumers can get wrong: token counts
around the workgroup step Q of k_emit's loop, sub-blocks that begin at a token index of every residue mod 4 (the loop
loads 16 bytes from an index rounded down), the longest codewords and the widest tokens through the 32-bit bit
accumulator, every alignment of a block in the output, the kinds of sub-block, the sliding stage, the token producers
of the other levels, and the framing.  Every generator asserts the property it is there for, worked out on the CPU from
the oracle's own stream (walk(), a DEFLATE header / token reader on tools/deflate_tokens.py) or its level-1 parse."""
import os
import re
import sys

import numpy as np

from gzp_amd import _native, synth

import l1_skip_cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import deflate_tokens as dt  # noqa: E402

BLOCK = 65280
BGZF_EOF = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00, 0x1b, 0x00, 0x03, 0x00,
                  0, 0, 0, 0, 0, 0, 0, 0])


def _constant(name):
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gzp_amd", "csrc", "gzpx_kernels.hip")
    with open(src) as f:
        m = re.search(r"constexpr uint32_t %s = (\d+);" % name, f.read())
    assert m, name
    return int(m.group(1))


Q = _constant("kEmitTpl") * _constant("kEmitThreads")  # tokens per workgroup step of k_emit's token loop (kEmitStep)
STAGE_BYTES = 4 * _constant("kStageWords")               # a framed block longer than this slides the stage


# ------------------------------------------------------------------------------------------------ reading the oracle
def walk(raw):
    """A raw DEFLATE stream -> ([(type, first token, tokens, litlen lengths, offset lengths)] per DEFLATE block,
    [(byte,) | (length, distance)])."""
    b, out, blocks = dt.Bits(raw), [], []
    while True:
        final, typ = b.get(1), b.get(2)
        ll = dl = None
        start = len(out)
        if typ == 0:
            b.pos = (b.pos + 7) & ~7
            n = b.get(16)
            b.get(16)
            b.pos += 8 * n
        else:
            if typ == 1:
                ll, dl = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
            else:
                hlit, hdist, hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[dt.ORDER[i]] = b.get(3)
                cd, lens = dt.decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = cd(b)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + b.get(2))
                    elif s == 17:
                        lens += [0] * (3 + b.get(3))
                    else:
                        lens += [0] * (11 + b.get(7))
                ll, dl = lens[:hlit], lens[hlit:]
            ld, dd = dt.decoder(ll), dt.decoder(dl)
            while True:
                s = ld(b)
                if s < 256:
                    out.append((s,))
                elif s == 256:
                    break
                else:
                    ln = dt.LBASE[s - 257] + b.get(dt.LEXT[s - 257])
                    ds = dd(b)
                    out.append((ln, dt.DBASE[ds] + b.get(dt.DEXT[ds])))
        blocks.append((typ, start, len(out) - start, ll, dl))
        if final:
            return blocks, out


def walk_first_member(oracle, data, level=1):
    """walk() of the first BGZF member of the oracle's stream for `data`."""
    stream = oracle.compress_stream(data, oracle.FMT_BGZF, level, oracle.COMPAT_1_24, BLOCK)
    return walk(stream[18:])


def text(n, seed):
    return synth.english_like(n, seed).copy()


# ------------------------------------------------------------------------------------------------ the cases
def all_literal(n, seed):
    """n bytes of [0x80, 0xC0) without a repeated hash (l1_skip_cases.splice_unique): n literals, and -- unlike
    unique_block's 256 symbols, which the oracle stores -- six-bit codes, so a Huffman-coded sub-block of n tokens."""
    a = np.zeros(n, dtype=np.uint8)
    l1_skip_cases.splice_unique(a, 0, n, np.random.default_rng(seed), lo=0x80, hi=0xC0)
    assert l1_skip_cases.candidate_less(a, 0, n)
    return a


def token_counts(oracle):
    """All-literal single blocks of Q - 1, Q, Q + 1, Q + 2 and 2Q + 3 tokens: a last step of 1, 2, 3 tokens and of a whole
    step less one, token counts of every residue mod 4.  (A hash table of 32,768 buckets has room for 2Q + 3 = 8,195.)"""
    out = []
    for k, n in enumerate((Q - 1, Q, Q + 1, Q + 2, 2 * Q + 3)):
        a = all_literal(n, 300 + k)
        blocks, toks = walk_first_member(oracle, a)
        assert len(blocks) == 1 and blocks[0][0] != 0 and len(toks) == n and all(len(t) == 1 for t in toks), n
        out.append(("%d literals" % n, a))
    assert {len(a) % 4 for _, a in out} == {0, 1, 2, 3}
    return out


def sub_block_residues(oracle):
    """One block of text each, chosen so that the second sub-block begins at a token index of residue 0, 1, 2 and 3."""
    out, seen = [], set()
    for seed in range(1, 40):
        a = text(BLOCK, seed)
        _, first = oracle.l1_tokens(a)
        if len(first) > 1 and int(first[1]) % 4 not in seen:
            seen.add(int(first[1]) % 4)
            blocks, _ = walk_first_member(oracle, a)
            assert len(blocks) >= 2 and blocks[1][0] != 0 and blocks[1][1] == int(first[1])
            out.append(("text seed %d, second sub-block at token %d" % (seed, int(first[1])), a))
        if len(seen) == 4:
            break
    assert seen == {0, 1, 2, 3}
    return out


def skewed(ratio, nsym, n, seed):
    w = ratio ** -np.arange(nsym, dtype=np.float64)
    return (np.random.default_rng(seed).choice(nsym, size=n, p=w / w.sum()) + 0x30).astype(np.uint8)


def long_codes(oracle):
    """Geometric symbol frequencies (ratio 1.5, 30 symbols): 14-bit litlen codes and 10-bit offset codes in the oracle's
    level-1 stream.  14 bits is the literal/length code's limit, and this input reaches it without the limit: built
    without one, its tree is exactly 14 deep, so make_code never takes its clamp here.  (Ratios 1.3-1.55 with 30-44
    symbols, seeds 1-3: none went deeper -- the matches take the frequent symbols' counts away.)  The inputs whose trees
    are deeper than the limits are in tests/huffman_limit_cases.py."""
    a = skewed(1.5, 30, BLOCK, 3)
    blocks, toks = walk_first_member(oracle, a)
    assert max(max(ll) for _, _, _, ll, _ in blocks if ll) >= 14
    assert max(max(dl) for _, _, _, _, dl in blocks if dl) >= 10
    return [("geometric frequencies", a)]


def widest_tokens(oracle):
    """The second half repeats the random first half at a distance of 32,640: length-258 matches with 13 extra offset
    bits, one after another.  And the `runs` class: length 258 at distance 1."""
    half = synth.make("random", BLOCK // 2, 11)
    a = np.concatenate([half, half])
    blocks, toks = walk_first_member(oracle, a)
    wide = [t for t in toks if len(t) == 2 and t[0] == 258 and t[1] > 24576]
    assert len(wide) >= 100 and any(typ != 0 for typ, *_ in blocks)
    r = synth.make("runs", 2 * BLOCK, 3)
    _, rt = walk_first_member(oracle, r)
    assert any(len(t) == 2 and t[0] == 258 and t[1] == 1 for t in rt)
    return [("second half repeats the first", a), ("class runs", r)]


def output_alignment(oracle):
    """Three-block slabs of text whose blocks begin at output offsets of every residue mod 4."""
    out, seen = [], set()
    for seed in range(1, 20):
        a = text(2 * BLOCK + 30000 + 7 * seed, 400 + seed)
        _, sizes = oracle.compress_stream(a, oracle.FMT_BGZF, 1, oracle.COMPAT_1_24, BLOCK, return_block_sizes=True)
        assert len(sizes) == 3
        offs = {0, int(sizes[0]) % 4, int(sizes[0] + sizes[1]) % 4}
        if not offs <= seen:
            seen |= offs
            out.append(("three blocks, offsets mod 4 %s" % sorted(offs), a))
        if len(seen) == 4:
            break
    assert seen == {0, 1, 2, 3}
    return out


def sub_block_kinds(oracle):
    out = []
    a = synth.make("random", BLOCK, 5)
    blocks, _ = walk_first_member(oracle, a)
    assert all(typ == 0 for typ, *_ in blocks)
    out.append(("random (stored)", a))
    for cls, n in (("ascii", 52), ("ascii", 100), ("repeats", 200), ("repeats", 300), ("period2", 300)):
        a = synth.make(cls, n, 3)
        blocks, _ = walk_first_member(oracle, a)
        assert [typ for typ, *_ in blocks] == [1], (cls, n)
        out.append(("%s %d (static)" % (cls, n), a))
    a = synth.make("mixed", 3 * BLOCK, 6)  # a random block, a block of text, a random block
    stream, sizes = oracle.compress_stream(a, oracle.FMT_BGZF, 1, oracle.COMPAT_1_24, BLOCK, return_block_sizes=True)
    kinds = [{typ for typ, *_ in walk(stream[int(sizes[:k].sum()) + 18:])[0]} for k in range(3)]
    assert kinds == [{0}, {2}, {0}]
    out.append(("mixed", a))
    # every other byte is one symbol, 200 others between: a window repeats only where two neighbours of theirs do, so
    # most of it stays literals and more than a third of the tokens are the same one
    a = np.full(BLOCK, 0x61, dtype=np.uint8)
    a[1::2] = 0x20 + np.random.default_rng(12).integers(0, 200, BLOCK // 2)
    a[1::2][a[1::2] == 0x61] = 0x1f
    blocks, toks = walk_first_member(oracle, a)
    assert all(typ == 2 for typ, *_ in blocks) and 3 * toks.count((0x61,)) > len(toks)
    out.append(("one dominant symbol", a))
    return out


GROUPS = {
    "token_counts": token_counts,
    "sub_block_residues": sub_block_residues,
    "long_codes": long_codes,
    "widest_tokens": widest_tokens,
    "output_alignment": output_alignment,
    "sub_block_kinds": sub_block_kinds,
}


# ------------------------------------------------------------------------------------------------ the checks
def check(lib, oracle, group):
    """BGZF, level 1: every case of the group, is_last true."""
    cases = GROUPS[group](oracle)
    with _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=BLOCK, compat=_native.COMPAT_1_24,
                         max_slab_bytes=3 * BLOCK, lib=lib) as ctx:
        for name, data in cases:
            assert 0 < data.size <= 3 * BLOCK
            want = oracle.compress_stream(data, oracle.FMT_BGZF, 1, oracle.COMPAT_1_24, BLOCK)
            got = ctx.compress_slab(data, is_last=True)
            assert got == want, (name, len(got), len(want))


SLIDES = [("random", 131072, 1), ("ascii", 131072, 1), ("random", 262144, 1), ("ascii", 262144, 1), ("text", 262144, 0)]


def check_window_slide(lib, oracle, cls, buffer_size, level):
    """Mgzip, one block of buffer_size bytes that does not fit the stage: stored bytes slide (random; everything at level
    0), coded tokens slide (printable noise)."""
    data = synth.make(cls, buffer_size, 9)
    want = oracle.compress_stream(data, oracle.FMT_MGZIP, level, oracle.COMPAT_1_24, buffer_size)
    assert len(want) > STAGE_BYTES + 64
    blocks, _ = walk(want[20:])
    assert all((typ == 0) == (cls != "ascii") for typ, *_ in blocks)
    with _native.Context(format=_native.FORMAT_MGZIP, level=level, buffer_size=buffer_size, compat=_native.COMPAT_1_24,
                         max_slab_bytes=buffer_size, lib=lib) as ctx:
        assert ctx.compress_slab(data, is_last=True) == want


def check_other_levels(lib, oracle, level):
    """The tokens of k_parse_hc (3) and k_parse_lazy (6, 9): a two-block text slab and a two-block mixed slab."""
    with _native.Context(format=_native.FORMAT_BGZF, level=level, buffer_size=BLOCK, compat=_native.COMPAT_1_24,
                         max_slab_bytes=2 * BLOCK, lib=lib) as ctx:
        for name, data in (("text", text(2 * BLOCK, 70 + level)), ("mixed", synth.make("mixed", 2 * BLOCK, 6))):
            want = oracle.compress_stream(data, oracle.FMT_BGZF, level, oracle.COMPAT_1_24, BLOCK)
            assert ctx.compress_slab(data, is_last=True) == want, (name, level)


def check_framing(lib, oracle):
    """BGZF with and without the end-of-file member behind the last block; Mgzip."""
    data = text(2 * BLOCK, 90)
    want = oracle.compress_stream(data, oracle.FMT_BGZF, 1, oracle.COMPAT_1_24, BLOCK)
    assert want.endswith(BGZF_EOF)
    with _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=BLOCK, compat=_native.COMPAT_1_24,
                         max_slab_bytes=2 * BLOCK, lib=lib) as ctx:
        assert ctx.compress_slab(data, is_last=True) == want
        assert ctx.compress_slab(data, is_last=False) == want[:-len(BGZF_EOF)]
    data = text(2 * BLOCK + 1234, 91)
    want = oracle.compress_stream(data, oracle.FMT_MGZIP, 1, oracle.COMPAT_1_24, BLOCK)
    with _native.Context(format=_native.FORMAT_MGZIP, level=1, buffer_size=BLOCK, compat=_native.COMPAT_1_24,
                         max_slab_bytes=3 * BLOCK, lib=lib) as ctx:
        assert ctx.compress_slab(data, is_last=True) == want
