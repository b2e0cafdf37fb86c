"""libdeflate's parsing rules that gzp_amd/csrc/gzpx_policy.h states once -- the minimum match length by alphabet size,
the short-scan rule, the recalculation of the lazy parsers -- written once and run twice: through the emulated library
on CPU (tests/test_emu_policy.py) and through the real HIP library on the MI355X (tests/test_gpu_policy.py).

Every case is one deflate_compress of a few thousand bytes, compared byte for byte with oracle.deflate_compress.  The
inputs sit on both sides of every threshold of choose_min_match_len's table (6, 8, 10, 16, 45 and 80 literals in use):
k symbols, and a dictionary of words over them that recur with one to three random symbols between, so that matches
of every length from 3 to 10 are on offer and a minimum match length that is off by one changes the parse.  (Uniform
random symbols without the dictionary do not notice a shifted table at k = 44 and k = 79.)  With the oracle's table
shifted by one either way, every k is noticed at levels 4, 6 and 9; levels 2 and 3 notice from k = 16 and k = 8 up --
below that their depth caps, 5 and 7, hide the table, as they should -- and level 10 at k = 6, 8, 9, 10, 15 and 44."""
import functools

import numpy as np

from gzp_amd import _native

ALPHABETS = (5, 6, 7, 8, 9, 10, 15, 16, 44, 45, 79, 80)
ALPHABET_LEVELS = (2, 3, 4, 6, 9, 10)
SHORT_LEVELS = (3, 6, 10)
RECALC_LEVELS = (5, 8)
SCAN = 4096  # calculate_min_match_len looks at the first 4096 bytes of a block


@functools.lru_cache(maxsize=None)
def recipe(k, n=6000):
    """The k symbols themselves, then word + 1..3 random symbols, repeated, cut at n bytes."""
    rng = np.random.default_rng(k)
    sym = rng.permutation(256)[:k].astype(np.uint8)
    words = [sym[rng.integers(0, k, int(rng.integers(3, 11)))] for _ in range(40)]
    parts, size = [sym], k
    while size < n:
        parts += [words[int(rng.integers(40))], sym[rng.integers(0, k, int(rng.integers(1, 4)))]]
        size += parts[-2].size + parts[-1].size
    a = np.ascontiguousarray(np.concatenate(parts)[:n])
    a.flags.writeable = False
    return a


def distinct(a):
    return int(np.unique(a[:SCAN]).size)


BOTH = (_native.COMPAT_1_24, _native.COMPAT_1_10)


def compats(level):
    """Levels 10-12 are libdeflate 1.10's parser whatever is asked for."""
    return (_native.COMPAT_1_10,) if level >= 10 else BOTH


def _same_stream(lib, oracle, level, compat, inputs):
    ocompat = {_native.COMPAT_1_10: oracle.COMPAT_1_10, _native.COMPAT_1_24: oracle.COMPAT_1_24}[compat]
    c = _native.Compressor(level, compat, lib=lib)
    try:
        for what, a in inputs:
            assert c.deflate_compress(a) == oracle.deflate_compress(a, level, ocompat), (what, level, compat)
    finally:
        c.close()


def min_len_by_alphabet(lib, oracle, level):
    inputs = []
    for k in ALPHABETS:
        a = recipe(k)
        assert a.size == 6000 and distinct(a) == k, (k, distinct(a))  # (a condition on the input, not on the library)
        inputs.append(("k = %d" % k, a))
    _same_stream(lib, oracle, level, compats(level)[0], inputs)


def short_scan(lib, oracle, level):
    """libdeflate >= 1.1x does not scan a block shorter than 512 bytes and uses 3; 1.10 scans it.  Five symbols: 9 (or
    the level's cap) against 3."""
    inputs = []
    for n in (511, 512):
        a = recipe(5)[:n]
        assert distinct(a) == 5
        inputs.append(("%d bytes" % n, a))
    for compat in BOTH:
        _same_stream(lib, oracle, level, compat, inputs)


def recalculation(lib, oracle, level):
    """Five symbols, then eighty: recalculate_min_match_len is first due at 10000 bytes, inside the first half, and then
    inside the second, where the answer is another."""
    a = np.concatenate([recipe(5, 12000), recipe(80, 12000)])
    assert distinct(a) == 5 and distinct(a[12000:]) == 80
    for compat in compats(level):
        _same_stream(lib, oracle, level, compat, [("5 then 80", a)])
