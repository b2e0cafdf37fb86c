"""DEFLATE's length and offset alphabets end to end (gzp_amd/csrc/gzpx_deflate.h), written once and run twice: through
the emulated library on CPU (tests/test_emu_alphabet.py) and through the real HIP library on the MI355X
(tests/test_gpu_alphabet.py).  Exact equality throughout; zlib and the oracle are the yardsticks.

Decode: crafted members (deflate_craft) of 32,768 seeded random literals and then one match of every length 3..258,
258 both as symbol 285 and as symbol 284 with extra 31, at distances that cycle through the lowest and the highest
distance of each of the 30 offset symbols (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, ..., 24,577, 32,768).  Once under the fixed
code and once under a dynamic code that gives all 29 length and all 30 offset symbols a codeword.  A BGZF member holds
at most 65,280 bytes here, so the BGZF form is two members, each with the literal prefix; the Mgzip form is one.  Both
routes of the inflater against zlib.decompress(raw, -15), and the same raw streams through the size query.

Encode: one input for which the oracle's stream at levels 1, 6 and 12 uses all 256 match lengths and all 30 offset
symbols -- asserted on the oracle's own stream first, read with tools/deflate_tokens.py -- then the library's stream
against the oracle's in both compat modes, and zlib inflates it to the input.  (At level 1 the lengths are the 255
from 4 on: libdeflate's level 1 hashes four bytes and never writes a match of three, and neither does the oracle.)"""
import bisect
import functools
import os
import sys
import zlib

import numpy as np

import deflate_craft as dc
import size_cases
from batch_cases import RAW, contexts
from gzp_amd import _native

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import deflate_tokens as dt  # noqa: E402

PREFIX = 32768
BGZF_MAX_OUT = 65280
# the lowest and the highest distance of every offset symbol (symbols 0..3 hold one distance each)
EDGE_DISTANCES = sorted({d for s in range(30) for d in (dc.DIST_BASE[s], dc.DIST_BASE[s] + (1 << dc.DIST_EXTRA[s]) - 1)})
assert len(EDGE_DISTANCES) == 56 and EDGE_DISTANCES[:10] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 12] and EDGE_DISTANCES[-2:] == [24577, 32768]
# (length, 258 as symbol 284 + 31): every length once, 258 twice
MATCHES = [(n, False) for n in range(3, 259)] + [(258, True)]
CODES = ("fixed", "dynamic")


# ------------------------------------------------------------------------------------------------ decode
def _prefix():
    return np.random.RandomState(41).randint(0, 256, PREFIX, dtype=np.uint8).tobytes()


def _match_tokens(first, count):
    """MATCHES[first : first + count] as tokens; the distances go on cycling where the member before stopped."""
    return [dc.match(n, EDGE_DISTANCES[k % len(EDGE_DISTANCES)], via)
            for k, (n, via) in enumerate(MATCHES[first:first + count], first)]


def _raw(code, tokens):
    w = dc.BitWriter()
    tokens = [("lits", _prefix())] + tokens + [("eob",)]
    if code == "fixed":
        dc.fixed(w, tokens, True)
    else:  # flat complete codes over 256 literals + end of block + 29 lengths, and over 30 offsets
        dc.dynamic(w, tokens, True, dc.balanced_lens(286), dc.balanced_lens(30))
    return w.getvalue()


@functools.lru_cache(maxsize=None)
def decode_streams(code, fmt):
    """[(raw DEFLATE stream, what zlib inflates it to)]: one member for Mgzip, as many as BGZF's output limit needs."""
    assert code in CODES
    cuts, first = [], 0
    while first < len(MATCHES):
        count, room = 0, (BGZF_MAX_OUT if fmt == dc.BGZF else 1 << 30) - PREFIX
        while first + count < len(MATCHES) and MATCHES[first + count][0] <= room:
            room -= MATCHES[first + count][0]
            count += 1
        cuts.append((first, count))
        first += count
    out = []
    for first, count in cuts:
        raw = _raw(code, _match_tokens(first, count))
        plain = zlib.decompress(raw, -15)
        assert len(plain) == PREFIX + sum(n for n, _ in MATCHES[first:first + count])
        out.append((raw, plain))
    assert len(out) == (2 if fmt == dc.BGZF else 1)
    return out


def check_decode(lib, code, fmt):
    streams = decode_streams(code, fmt)
    if code == "dynamic":  # every length and offset symbol has a codeword, and all members together use each of them
        used_l, used_d = set(), set()
        for raw, _ in streams:
            toks, blocks = dt.tokens(raw)
            assert [b[0] for b in blocks] == [2]
            used_l |= {t[2] for t in toks if t[1] == "M"}
            used_d |= {bisect.bisect_right(dc.DIST_BASE, t[3]) - 1 for t in toks if t[1] == "M"}
        assert used_l == set(range(3, 259)) and used_d == set(range(30))
    stream = b"".join(dc.wrap(fmt, raw, zlib.crc32(plain), len(plain)) for raw, plain in streams)
    want = b"".join(plain for _, plain in streams)
    for route in (_native.INFLATE_SEG, _native.INFLATE_WAVE):
        with _native.DContext(format=_native.FORMAT_BGZF if fmt == dc.BGZF else _native.FORMAT_MGZIP, lib=lib) as d:
            d.set_route(route)
            assert d.decompress(stream) == want, (code, fmt, route)
    members = [raw for raw, _ in streams]
    blob, offs = size_cases.layout(members)
    for route, d in contexts(lib):
        r = size_cases.call(lib, d, RAW, blob, offs, [len(m) for m in members])
        size_cases.check_all_good(r, [plain for _, plain in streams], members, (code, fmt, route))


# ------------------------------------------------------------------------------------------------ encode
LEVELS = (1, 6, 12)
# libdeflate's matchfinders look 32,767 bytes back, not 32,768: that is the far edge a compressor can reach.  After
# one turn through all the edges the lengths go on with those up to 1,025 (the first 37), which keeps the input small.
ENCODE_DISTANCES = EDGE_DISTANCES[:-1] + [32767]
ENCODE_NEAR = 37
# Level 1 keeps two positions per hash bucket, and of the candidates thousands of bytes back some are gone when their
# copy comes: the lengths that met the distances from 6,144 on in the first turn come once more, at near distances.
ENCODE_AGAIN = list(range(48, 59))
# Level 1 hashes four bytes (ht_matchfinder): the oracle writes no match of length 3 there
ENCODE_LENGTHS = {1: set(range(4, 259)), 6: set(range(3, 259)), 12: set(range(3, 259))}
@functools.lru_cache(maxsize=None)
def encode_input():
    """Random bytes, and in them for every length L = 3..258 a copy of the L bytes that lie an edge distance back,
    closed by a byte that breaks the match.  Length 3 + k takes distance ENCODE_DISTANCES[k] in the first turn: the
    short lengths go with the short distances (no parser takes a three-byte match from far away).  A copy's source is random bytes that
    no other copy has read and that are no copy themselves -- fresh bytes are put in front of a copy until that holds --
    so the wanted match is the only one a matchfinder meets, whatever its search depth."""
    rng = np.random.RandomState(43)
    out = bytearray(rng.randint(0, 256, 64, dtype=np.uint8).tobytes())
    fresh = [True] * len(out)  # a random byte that no copy has read
    for k, n in enumerate(list(range(3, 259)) + ENCODE_AGAIN):
        dist = ENCODE_DISTANCES[k] if k < len(ENCODE_DISTANCES) else ENCODE_DISTANCES[k % ENCODE_NEAR]
        src = min(n, dist)  # (a copy longer than its distance repeats the dist bytes in front of it)
        # (the source does not begin at byte 0, and the bytes in front of source and copy differ: the match is no longer)
        while (len(out) <= dist or not all(fresh[len(out) - dist:len(out) - dist + src])
               or out[-1] == out[-1 - dist]):
            out.append(int(rng.randint(0, 256)))
            fresh.append(True)
        at = len(out) - dist
        fresh[at:at + src] = [False] * src
        for _ in range(n):
            out.append(out[-dist])
        stop = int(rng.randint(0, 256))
        while stop == out[-dist] or stop == out[-1]:
            stop = (stop + 1) & 255
        out.append(stop)
        fresh += [False] * (n + 1)
    assert len(out) <= 256 * 1024
    return np.frombuffer(bytes(out), dtype=np.uint8)


def coverage(raw):
    """(match lengths, offset symbols) a raw DEFLATE stream uses."""
    toks, _ = dt.tokens(raw)
    return ({t[2] for t in toks if t[1] == "M"}, {bisect.bisect_right(dc.DIST_BASE, t[3]) - 1 for t in toks if t[1] == "M"})


@functools.lru_cache(maxsize=None)
def oracle_stream(oracle, level, ocompat):
    """The oracle's Mgzip member of the input, after the claim on its payload: every length the level can write
    (ENCODE_LENGTHS), all 30 offset symbols."""
    data = encode_input()
    want = oracle.compress_stream(data, oracle.FMT_MGZIP, level, ocompat, data.size)
    lengths, offsets = coverage(want[20:-8])
    assert lengths == ENCODE_LENGTHS[level], (level, sorted(ENCODE_LENGTHS[level] ^ lengths))
    assert offsets == set(range(30)), (level, sorted(set(range(30)) - offsets))
    return want


def check_encode(lib, oracle, level):
    data = encode_input()
    compat_pairs = [(_native.COMPAT_1_10, oracle.COMPAT_1_10), (_native.COMPAT_1_24, oracle.COMPAT_1_24)]
    for compat, ocompat in compat_pairs:
        want = oracle_stream(oracle, level, ocompat)
        with _native.Context(format=_native.FORMAT_MGZIP, level=level, buffer_size=data.size, compat=compat,
                             max_slab_bytes=data.size, lib=lib) as ctx:
            got = ctx.compress_slab(data, is_last=True)
        assert got == want, (level, compat, len(got), len(want))
        assert zlib.decompress(got[20:-8], -15) == data.tobytes(), (level, compat)
