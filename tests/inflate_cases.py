"""Inflate conformance: DEFLATE streams no compressor writes, and a differential run of a hostile encoder.  Written
once and run twice: through the emulated library on CPU (tests/test_emu_inflate_conformance.py) and through the real
HIP library on the MI355X (tests/test_gpu_inflate_conformance.py).

The yardstick is libdeflate_deflate_decompress of the system's libdeflate.so.0 (v1.10 behaviour), whose verdict on
every crafted stream -- return code and, for an accepted one, the bytes -- is recorded in
tests/golden/inflate_verdicts.json by tests/golden/make_inflate_verdicts.py.  The tests read the record, so a box
without the binary runs them all the same.  Where zlib accepts a stream too, its bytes must equal the record's.

Every crafted stream is built field by field with tests/deflate_craft.py: one stream per rule, and one per table
builder (litlen / offset / precode) or table level (root / second level) that decodes the rule."""
import ctypes
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import deflate_craft as dc
from deflate_craft import BitWriter, dynamic, fixed, lens_from, match, stored
from gzp_amd import _native, synth

VERDICTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inflate_verdicts.json")
ROUTES = {"seg": _native.INFLATE_SEG, "wave": _native.INFLATE_WAVE}
LD_OK, LD_BAD_DATA, LD_SHORT_OUTPUT, LD_INSUFFICIENT_SPACE = 0, 1, 2, 3
# kSegBigBytes (gzpx_inflate_seg.h): launch_inflate_members (gzpx_kernels.hip) takes the launch form of k_inflate_seg for
# large members (kSegBigW waves a member) when the compressed bytes the host hands it (InflateScratch.in_bytes) reach
# this much per member: the AVERAGE over the launch, so a one-member slab switches at this size.
SEG_BIG_BYTES = 131072


# ------------------------------------------------------------------------------------------------ the yardstick
def box_libdeflate():
    """decompress(raw, cap) -> (libdeflate's return code, the bytes it wrote) through the system's library, or None."""
    for path in ("libdeflate.so.0", "/lib/x86_64-linux-gnu/libdeflate.so.0", "/usr/lib/x86_64-linux-gnu/libdeflate.so.0",
                 "/usr/lib64/libdeflate.so.0"):
        try:
            L = ctypes.CDLL(path)
        except OSError:
            continue
        L.libdeflate_alloc_decompressor.restype = ctypes.c_void_p
        L.libdeflate_deflate_decompress.restype = ctypes.c_int
        L.libdeflate_deflate_decompress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p,
                                                    ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        d = L.libdeflate_alloc_decompressor()

        def decompress(raw, cap, L=L, d=d):
            out = ctypes.create_string_buffer(max(cap, 1))
            n = ctypes.c_size_t(0)
            rc = L.libdeflate_deflate_decompress(d, bytes(raw), len(raw), out, cap, ctypes.byref(n))
            return rc, out.raw[:n.value] if rc == LD_OK else b""
        return decompress
    return None


def load_verdicts():
    with open(VERDICTS) as f:
        return {v["case"]: v for v in json.load(f)["verdicts"]}


# ------------------------------------------------------------------------------------------------ crafted streams
class Case:
    """One crafted raw stream and the output size its member's footer claims (= the room libdeflate is given)."""

    def __init__(self, name, raw, isize, fmt=dc.BGZF):
        self.name, self.raw, self.isize, self.fmt = name, bytes(raw), isize, fmt


A, B = ord("a"), ord("b")
PAIR = [1, 1]  # a complete offset code nobody uses


def _dyn(tokens, litlen, dist=None, lead=False, **kw):
    """A single final dynamic block; litlen / dist as {symbol: length} or length lists.  lead: behind a fixed block that
    holds one 'a' (a framed member whose ISIZE is 0 is never inflated, so a case without output of its own needs one)."""
    w = BitWriter()
    if lead:
        fixed(w, [("lit", A), ("eob",)], False)
    ll = lens_from(litlen, 257) if isinstance(litlen, dict) else litlen
    dl = PAIR if dist is None else lens_from(dist, 1) if isinstance(dist, dict) else dist
    dynamic(w, tokens, True, ll, dl, **kw)
    return w.getvalue()


def _fix(tokens):
    w = BitWriter()
    fixed(w, tokens, True)
    return w.getvalue()


def _chain(first_sym, upto, step=1):
    """{symbol: length} of a code with one codeword of each length 1 .. upto: incomplete by 2^-upto."""
    return {first_sym + step * (l - 1): l for l in range(1, upto + 1)}


def _all_cases():
    c = []
    add = lambda name, raw, isize, fmt=dc.BGZF: c.append(Case(name, raw, isize, fmt))
    lit = lambda b: ("lit", b)
    EOB = ("eob",)
    aa = [lit(A), lit(A), EOB]
    aaaa = [lit(A), match(3, 1), EOB]  # 'a' and a match of three at distance 1

    # ---- code shape: litlen
    add("litlen_incomplete", _dyn(aa, {A: 1, 256: 2}), 2)
    # (lengths 1..12 on bytes 0..11 and 13 for the end-of-block code: codewords behind the 10-bit root)
    add("litlen_incomplete_long", _dyn([lit(0), lit(10), lit(11), EOB], {**_chain(0, 12), 256: 13}), 3)
    add("litlen_oversubscribed", _dyn([lit(A), EOB], {A: 1, B: 1, 256: 1}), 1)
    add("litlen_oversubscribed_long", _dyn([lit(0), EOB], {**_chain(0, 12), 256: 12, 255: 12, 254: 12}), 1)
    add("litlen_only_eob_bit0", _dyn([EOB], {256: 1}, lead=True), 1)
    add("litlen_only_eob_bit1", _dyn([("raw", 1, 1)], {256: 1}, lead=True), 1)
    add("litlen_only_eob_alone", _dyn([EOB], {256: 1}), 0)
    add("litlen_single_len2", _dyn([EOB], {256: 2}, lead=True), 1)
    add("litlen_single_len1_literal", _dyn([lit(A)] * 4 + [("raw", 0xFF, 8)] * 4, {A: 1}), 4)  # (no end-of-block code)
    # ---- code shape: offset
    add("offset_incomplete", _dyn(aaaa, {A: 1, 257: 2, 256: 2}, {0: 1, 1: 2}), 4)
    add("offset_incomplete_long", _dyn(aaaa, {A: 1, 257: 2, 256: 2}, _chain(0, 10)), 4)  # (codewords behind the 8-bit root)
    add("offset_oversubscribed", _dyn(aaaa, {A: 1, 257: 2, 256: 2}, {0: 1, 1: 1, 2: 1}), 4)
    add("offset_oversubscribed_long", _dyn(aaaa, {A: 1, 257: 2, 256: 2}, {**_chain(0, 10), 10: 10, 11: 10, 12: 10}), 4)
    add("offset_empty_unused", _dyn(aa, {A: 1, 256: 1}, [0]), 2)
    add("offset_empty_used_bit0", _dyn([lit(A), ("match", 257, 0, 0, 0), ("raw", 0, 1), EOB], {A: 1, 257: 2, 256: 2}, [0]), 4)
    add("offset_empty_used_bit1", _dyn([lit(A), ("match", 257, 0, 0, 0), ("raw", 1, 1), EOB], {A: 1, 257: 2, 256: 2}, [0]), 4)
    add("offset_empty_wide_used", _dyn([lit(A), ("match", 257, 0, 0, 0), ("raw", 1, 1), EOB], {A: 1, 257: 2, 256: 2}, [0] * 30), 4)
    abab = [lit(A), lit(B), lit(A), lit(B)]
    for bit in (0, 1):
        # (symbol 3 alone, one bit long: distance 4, whichever bit is sent)
        add("offset_single_len1_bit%d" % bit,
            _dyn(abab + [("match", 257, 0, 0, 0), ("raw", bit, 1), EOB], {A: 2, B: 2, 257: 2, 256: 2}, {3: 1}), 7)
    # (tokens name an offset symbol WITHOUT a codeword where the bit is sent raw: nothing but that bit is written)
    add("offset_single_len1_sym0_bit1", _dyn([lit(A), ("match", 257, 0, 1, 0), ("raw", 1, 1), EOB], {A: 1, 257: 2, 256: 2}, {0: 1}), 4)
    add("offset_single_len2", _dyn(aaaa, {A: 1, 257: 2, 256: 2}, {0: 2}), 4)
    add("offset_single_len2_unused", _dyn(aa, {A: 1, 256: 1}, {0: 2}), 2)
    # ---- code shape: precode (its lengths go by symbol: [16, 17, 18, 0, 8, ...] is the header's order, not this one's)
    good = lens_from({A: 1, 256: 1}, 257) + PAIR  # what the code-length symbols spell: lengths 0 and 1 only
    cl = dc.plain_cl_syms(good)
    pre = lambda d: lens_from(d, 19)
    add("precode_incomplete", _dyn(aa, {A: 1, 256: 1}, pre_lens=pre({0: 1, 1: 2}), cl_syms=cl), 2)
    add("precode_oversubscribed", _dyn(aa, {A: 1, 256: 1}, pre_lens=pre({0: 1, 1: 1, 2: 1}), cl_syms=cl), 2)
    add("precode_single_len2", _dyn(aa, {A: 1, 256: 1}, pre_lens=pre({0: 2}), cl_syms=[(0,)] * 259), 2)
    # a precode of one symbol spells one length 259 times; with symbol 0 that is the empty litlen code, which decodes
    # every bit as the literal 0: the zeros run until the output is full
    zeros = [("raw", 0, 16)] * 4
    add("precode_single_len1_bit0", _dyn(zeros, {}, [0, 0], pre_lens=pre({0: 1}), cl_syms=[(0,)] * 259), 4)
    add("precode_single_len1_bit1", _dyn(zeros, {}, [0, 0], pre_lens=pre({0: 1}), cl_syms=[("raw", 1, 1)] * 259), 4)
    add("precode_empty", _dyn(zeros, {}, [0, 0], pre_lens=[0] * 19, cl_syms=[("raw", 0, 1)] * 259), 4)
    add("precode_unused_codeword_sent", _dyn(aa, {A: 1, 256: 1}, pre_lens=pre({0: 1, 1: 2}), cl_syms=[("raw", 3, 2)] + cl[1:]), 2)

    # ---- the code-length header
    add("header_leading_16", _dyn(aa, {A: 1, 256: 1}, cl_syms=[(16, 0)] + cl[3:], pre_lens=pre({0: 1, 1: 2, 16: 2})), 2)
    # 16 across the boundary: lengths ..., [255] = 2, [256] = 2 | offsets 2 2 2 2
    ll = lens_from({A: 1, 255: 2, 256: 2}, 257)
    add("header_run16_crosses", _dyn(aa, ll, [2, 2, 2, 2], cl_syms=dc.plain_cl_syms(ll[:256]) + [(16, 2)]), 2)
    # 17 across: [257..259] = 0 | offsets 0 0 1 1
    ll = lens_from({A: 1, 256: 1}, 260)
    add("header_run17_crosses", _dyn(aa, ll, [0, 0, 1, 1], cl_syms=dc.plain_cl_syms(ll[:257]) + [(17, 2), (1,), (1,)]), 2)
    # 18 across: [257..269] = 0 | offsets 0 0 0 0 1 1
    ll = lens_from({A: 1, 256: 1}, 270)
    add("header_run18_crosses", _dyn(aa, ll, [0, 0, 0, 0, 1, 1], cl_syms=dc.plain_cl_syms(ll[:257]) + [(18, 6), (1,), (1,)]), 2)
    # the last run overruns the total: by one (17 of three zeros with two lengths left), by 137 (18 of 138, one left)
    ll = lens_from({A: 1, 256: 1}, 257)
    add("header_overrun_by_1", _dyn(aa, ll, [1, 1, 0, 0], cl_syms=dc.plain_cl_syms(ll + [1, 1]) + [(17, 0)]), 2)
    add("header_overrun_by_137", _dyn(aa, ll, [1, 1, 0], cl_syms=dc.plain_cl_syms(ll + [1, 1]) + [(18, 127)]), 2)
    add("header_overrun_by_137_of_320", _dyn(aa, lens_from({A: 1, 256: 1}, 288), [1, 1] + [0] * 30,
                                             cl_syms=dc.plain_cl_syms(lens_from({A: 1, 256: 1}, 288) + [1, 1] + [0] * 29) + [(18, 127)]), 2)
    add("header_overrun_16", _dyn(aa, ll, [2, 2, 2, 2], cl_syms=dc.plain_cl_syms(ll + [2]) + [(16, 3)]), 2)
    # HCLEN 4: only 16, 17, 18 and 0 can have a precode length, so every code length is zero (the empty litlen code)
    add("header_hclen_4", _dyn(zeros, {}, [0], hclen=4, pre_lens=pre({18: 1, 0: 1}), cl_syms=[(18, 127), (18, 109)]), 4)
    ll = lens_from({A: 1, 0: 15, 1: 15, 2: 14, 3: 13, 4: 12, 5: 11, 6: 10, 7: 9, 8: 8, 9: 7, 10: 6, 11: 5, 12: 4, 13: 3, 256: 2}, 257)
    add("header_hclen_19", _dyn([lit(0), lit(1), lit(A), lit(7), EOB], ll, hclen=19), 4)
    for n in (286, 287, 288):
        add("header_hlit_%d" % (n - 257), _dyn(aa, lens_from({A: 1, 256: 2, n - 1: 2}, n)), 2)
    for n in (30, 31, 32):
        add("header_hdist_%d" % n, _dyn(aaaa, {A: 1, 257: 2, 256: 2}, lens_from({0: 1, n - 1: 1}, n)), 4)
    # no end-of-block code in an otherwise complete code: libdeflate has no check of its own, so the block runs until
    # the output is full (many literals) or the input is spent (few)
    add("no_eob_output_fills", _dyn([lit(A)] * 40 + [("raw", 0, 16)] * 4, {A: 1, B: 1}), 8)
    add("no_eob_input_ends", _dyn([lit(A)] * 4, {A: 1, B: 1}), 4000)

    # ---- symbols
    for s in (286, 287):
        add("fixed_litlen_%d_sent" % s, _fix([lit(A), ("match", s, 0, 0, 0), EOB]), 259)
        add("dynamic_litlen_%d_sent" % s, _dyn([lit(A), ("match", s, 0, 0, 0), EOB], lens_from({A: 1, 256: 2, s: 2}, s + 1)), 259)
    for s in (30, 31):
        add("fixed_offset_%d_sent" % s, _fix([lit(A), ("match", 257, 0, s, 0), ("raw", 0, 14), EOB]), 4)
        add("dynamic_offset_%d_sent" % s, _dyn([lit(A), ("match", 257, 0, s, 0), ("raw", 0, 14), EOB], {A: 1, 257: 2, 256: 2},
                                               lens_from({0: 1, s: 1}, s + 1)), 4)
    add("litlen_unused_codeword_root", _dyn([lit(A), ("raw", 3, 2), EOB], {A: 1, 256: 2}), 1)
    # (the chain's free codeword is thirteen ones: behind the root table)
    add("litlen_unused_codeword_second_level", _dyn([lit(0), ("raw", (1 << 13) - 1, 13), EOB], {**_chain(0, 12), 256: 13}), 1)
    add("offset_unused_codeword_root", _dyn([lit(A), ("match", 257, 0, 0, 0), ("raw", 3, 2), EOB], {A: 1, 257: 2, 256: 2}, {0: 1, 1: 2}), 4)
    add("offset_unused_codeword_second_level",
        _dyn([lit(A), ("match", 257, 0, 0, 0), ("raw", (1 << 10) - 1, 10), EOB], {A: 1, 257: 2, 256: 2}, _chain(0, 10)), 4)
    w = BitWriter()
    fixed(w, [lit(A), EOB], False)
    w.bits(1, 1)
    w.bits(3, 2)
    w.bits(0, 29)
    add("block_type_3", w.getvalue(), 1)

    # ---- stored blocks
    def st(data, final=True, **kw):
        w = BitWriter()
        stored(w, data, final, **kw)
        return w

    add("stored_nlen_mismatch", st(b"abc", nlen=0xFFFC ^ 1).getvalue(), 3)
    add("stored_len_past_payload", st(b"abc", length=4).getvalue(), 4)
    add("stored_len_0", st(b"").getvalue(), 0)
    w = st(b"", final=False)
    fixed(w, aa, True)
    add("stored_len_0_then_fixed", w.getvalue(), 2)
    big = synth.make("text", 65535, 3).tobytes()
    add("stored_len_65535", st(big).getvalue(), 65535, dc.MGZIP)

    # ---- output accounting
    add("distance_one_before_start", _fix([lit(A), match(3, 2), EOB]), 4)
    add("distance_to_start", _fix([lit(A), lit(B), match(5, 2), EOB]), 7)
    add("over_isize_by_literal", _fix([lit(A)] * 5 + [EOB]), 4)
    add("over_isize_by_match", _fix([lit(A), match(4, 1), EOB]), 4)
    add("over_isize_by_stored", st(b"abcde").getvalue(), 4)
    add("over_isize_by_literal_dynamic", _dyn([lit(A)] * 5 + [EOB], {A: 1, 256: 1}), 4)
    add("over_isize_by_match_dynamic", _dyn([lit(A), match(4, 1), EOB], {A: 1, 258: 2, 256: 2}, {0: 1, 1: 1}), 4)
    add("short_of_isize", _fix([lit(A)] * 4 + [EOB]), 5)
    # 3 header bits + six 9-bit literals + 8-bit literals + the 7-bit end-of-block code: 64 + 8 k bits
    raw = _fix([lit(200)] * 6 + [lit(A)] * 3 + [EOB])
    assert len(raw) * 8 == 3 + 6 * 9 + 3 * 8 + 7
    add("final_block_ends_on_last_bit", raw, 9)
    # streams that end early; the all-zero codeword of every code below is the end-of-block code, so the zero padding a
    # decoder reads behind the end stops the block at once
    ll = lens_from({256: 1, 279: 8, **{A + i: l for i, l in enumerate((2, 3, 4, 5, 6, 7, 8))}}, 257)  # (279: lengths 99..114)
    text = bytes(A + (i * i + i // 3) % 7 for i in range(300))
    w = BitWriter()
    dynamic(w, [("lits", text), match(100, 7), EOB], True, ll, lens_from({4: 1, 5: 1}, 6))
    whole = w.getvalue()
    add("ends_whole", whole, 400)
    add("ends_inside_header", whole[:40], 400)  # (the header is 17 + 3 * 19 bits and 263 code lengths of 2 to 4 bits)
    w = BitWriter()
    dynamic(w, [("lits", text)], True, ll, lens_from({4: 1, 5: 1}, 6))
    if w.bitpos % 8 == 0:
        dc.emit(w, [lit(A)], dc.canonical(ll), dc.canonical([1, 1]))
    k = w.bitpos // 8 + 1  # the next literal has an 8-bit codeword, and this many bytes end inside it
    dc.emit(w, [lit(A + 6), lit(A + 6), EOB], dc.canonical(ll), dc.canonical([1, 1]))
    assert 0 < 8 * k - (w.bitpos - 8 - 8 - 1) < 8
    add("ends_inside_symbol", w.getvalue()[:k], 400)
    # a fixed block cut behind a length symbol: four of its five extra bits are there
    w = BitWriter()
    fixed(w, [lit(200)] + [lit(A)] * 7 + [("raw", int(dc.canonical(dc.FIXED_LITLEN)[0][284]), 8)], True)
    assert w.bitpos % 8 == 4
    add("ends_inside_extra_bits", w.getvalue(), 300)
    return c


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _all_cases()
        assert len({x.name for x in _CASES}) == len(_CASES)
    return _CASES


def case_names():
    return [x.name for x in cases()]


def record(decompress):
    """The verdict of `decompress` (box_libdeflate()'s) on every case, as the golden file holds it."""
    out = []
    for x in cases():
        rc, data = decompress(x.raw, x.isize)
        v = {"case": x.name, "sha256": hashlib.sha256(x.raw).hexdigest(), "isize": x.isize, "rc": rc}
        if rc == LD_OK:
            if len(data) > 512:  # (long outputs by their hash: the file stays small)
                v["out_sha256"] = hashlib.sha256(data).hexdigest()
                v["out_len"] = len(data)
            else:
                v["out_hex"] = data.hex()
        out.append(v)
    return out


# ------------------------------------------------------------------------------------------------ verdict checks
def _expect(v, x):
    """(error code or None, the bytes or None) a framed member must give: libdeflate's verdict, with the two rules of
    the framing around it -- a member whose ISIZE is 0 is not inflated at all (gzp's decompress skips the call), and an
    accepted stream that leaves its ISIZE short is BadData (test_error_classes: libdeflate's SHORT_OUTPUT)."""
    if x.isize == 0:
        return None, b""
    if v["rc"] == LD_BAD_DATA:
        return _native.ERR_BAD_DATA, None
    if v["rc"] == LD_INSUFFICIENT_SPACE:
        return _native.ERR_INSUFFICIENT_SPACE, None
    assert v["rc"] == LD_OK, v
    if v.get("out_len", len(v.get("out_hex", "")) // 2) < x.isize:
        return _native.ERR_BAD_DATA, None
    return None, _known_out(v, x)


def _same(v, got):
    if "out_hex" in v:
        return got == bytes.fromhex(v["out_hex"])
    return len(got) == v["out_len"] and hashlib.sha256(got).hexdigest() == v["out_sha256"]


def _known_out(v, x):
    """The bytes of an accepted case, for its member's CRC (the long ones are stored blocks: the case knows them)."""
    if "out_hex" in v:
        return bytes.fromhex(v["out_hex"])
    out = zlib.decompress(x.raw, -15)
    assert _same(v, out)
    return out


def check_record_matches_streams(verdicts):
    """The craft module still makes the streams the record was taken from, and zlib agrees wherever it accepts."""
    assert sorted(verdicts) == sorted(case_names())
    for x in cases():
        v = verdicts[x.name]
        assert v["sha256"] == hashlib.sha256(x.raw).hexdigest() and v["isize"] == x.isize, x.name
        try:
            z = zlib.decompressobj(-15).decompress(x.raw)
        except zlib.error:
            continue
        if v["rc"] == LD_OK:
            assert _same(v, z), (x.name, "zlib's bytes differ from libdeflate's")


def check_decompressor(lib, verdicts, name):
    """Decompressor.deflate_decompress: libdeflate's call, where fewer bytes than the room are fine."""
    x = next(c for c in cases() if c.name == name)
    v = verdicts[name]
    d = _native.Decompressor(lib=lib)
    try:
        if v["rc"] == LD_OK:
            assert _same(v, d.deflate_decompress(x.raw, x.isize)), name
        else:
            with pytest.raises(_native.GzpxError) as e:
                d.deflate_decompress(x.raw, x.isize)
            assert e.value.code == {LD_BAD_DATA: _native.ERR_BAD_DATA, LD_INSUFFICIENT_SPACE: _native.ERR_INSUFFICIENT_SPACE}[v["rc"]], name
    finally:
        d.close()


_NEIGHBOURS = {}


def _neighbours(fmt):
    if fmt not in _NEIGHBOURS:
        chunks = [synth.make(cls, n, 40 + i).tobytes() for i, (cls, n) in enumerate((("text", 3000), ("dna", 700), ("mixed", 5000), ("runs", 1200)))]
        _NEIGHBOURS[fmt] = [(ch, dc.wrap(fmt, dc.zlib_payload(ch, 6), zlib.crc32(ch), len(ch))) for ch in chunks]
    return _NEIGHBOURS[fmt]


def check_member(lib, verdicts, name, route):
    """The case as a framed member through DContext on one route: alone, then as the first, a middle and the last
    member of a stream of ordinary members -- the verdict, the failing member's index, the neighbours' bytes."""
    x = next(c for c in cases() if c.name == name)
    v = verdicts[name]
    code, out = _expect(v, x)
    out = out or b""
    member = dc.wrap(x.fmt, x.raw, zlib.crc32(out), x.isize)
    nb = _neighbours(x.fmt)
    with _native.DContext(format=_native.FORMAT_BGZF if x.fmt == dc.BGZF else _native.FORMAT_MGZIP, lib=lib) as d:
        d.set_route(ROUTES[route])
        for where in (None, 0, 2, 4):
            if where is None:
                members, plain, idx = [member], [out], 0
            else:
                members, plain = [m for _, m in nb], [p for p, _ in nb]
                members.insert(where, member)
                plain.insert(where, out)
                idx = where
            if code is None:
                assert d.decompress(b"".join(members)) == b"".join(plain), (name, route, where)
            else:
                with pytest.raises(_native.GzpxError) as e:
                    d.decompress(b"".join(members))
                assert (e.value.code, e.value.block) == (code, idx), (name, route, where, e.value.code, e.value.block)


# ------------------------------------------------------------------------------------------------ the differential run
GPU_MEMBERS, GPU_SEED = 200, 7300  # the GPU file's run (the emulator file checks its seeds' edges on the CPU too)
EDGE_SIZES = (0, 1, 2, 3, 258, 259, 32768, 32769, 65279, 65280)
BGZF_MAX_PAYLOAD = 65536 - 26


def hostile_bgzf(n_members, seed):
    """(streams, plain, stats): BGZF members of the hostile encoder over the synth classes, sizes 0 .. 65,280 drawn
    toward the edge sizes (the small ones more often: they cost nothing), several members per stream."""
    rng = np.random.default_rng(seed)
    classes = sorted(synth.CLASSES)
    stats = dict.fromkeys(dc.STAT_KEYS, 0)
    members, plain, raws = [], [], []
    for i in range(n_members):
        r = rng.random()
        if r < 0.55:
            n = int(rng.choice(EDGE_SIZES[:6]))
        elif r < 0.70:
            n = int(rng.choice(EDGE_SIZES[6:]))
        elif r < 0.95:
            n = int(rng.integers(0, 3000))
        else:
            n = int(rng.integers(0, 65281))
        a = synth.make(classes[i % len(classes)], n, seed + i).tobytes()
        raw, st = dc.encode(a, rng, max_payload=BGZF_MAX_PAYLOAD)
        for k in st:
            stats[k] += st[k]
        members.append(dc.bgzf_wrap(raw, zlib.crc32(a), len(a)))
        plain.append(a)
        raws.append(raw)
    streams = []
    i = 0
    while i < n_members:
        k = int(rng.integers(1, 24))
        streams.append((b"".join(members[i:i + k]), b"".join(plain[i:i + k])))
        i += k
    return streams, list(zip(raws, plain)), stats


def hostile_mgzip(seed):
    """Mgzip members whose size is SEG_BIG_BYTES - 1, SEG_BIG_BYTES and a little more, each its own slab (so the slab's
    average is the member's size): printable noise and text through the hostile encoder, brought to the exact size with
    garbage bytes behind the final block."""
    rng = np.random.default_rng(seed)
    out = []
    stats = dict.fromkeys(dc.STAT_KEYS, 0)
    for total in (SEG_BIG_BYTES - 1, SEG_BIG_BYTES, SEG_BIG_BYTES + 4097):
        a = (synth.make("ascii", 70000, seed + total).tobytes() + synth.make("text", 55000, seed + total).tobytes())  # (fits the size even stored)
        raw, st = dc.encode(a, rng, max_payload=total - 28)
        raw += rng.integers(0, 256, total - 28 - len(raw), dtype=np.uint8).tobytes()
        for k in st:
            stats[k] += st[k]
        out.append((dc.mgzip_wrap(raw, zlib.crc32(a), len(a)), a, raw))
    return out, stats


def check_stats(stats):
    """The lower bounds that keep the differential run from passing vacuously."""
    for k in dc.EDGE_KINDS + ("litlen15_used", "offset15_used", "stored_unaligned", "fixed_unaligned", "dynamic_unaligned",
                              "empty_stored"):
        assert stats[k] >= 1, (k, stats)


def check_hostile_bgzf(lib, route, streams, raws):
    ld = box_libdeflate()
    with _native.DContext(lib=lib) as d:
        d.set_route(ROUTES[route])
        for i, (s, plain) in enumerate(streams):
            assert d.decompress(s) == plain, (route, "stream", i)
    if ld:
        for i, (raw, plain) in enumerate(raws):
            assert ld(raw, len(plain)) == (LD_OK, plain), ("libdeflate", i)


def check_hostile_mgzip(lib, route, members):
    ld = box_libdeflate()
    sizes = [len(m) for m, _, _ in members]
    assert SEG_BIG_BYTES - 1 in sizes and SEG_BIG_BYTES in sizes, sizes  # the last member of the small launch form of k_inflate_seg, the first of the big one
    with _native.DContext(format=_native.FORMAT_MGZIP, lib=lib) as d:
        d.set_route(ROUTES[route])
        for m, plain, raw in members:
            assert d.decompress(m) == plain, (route, len(m))
            if ld:
                assert ld(raw, len(plain)) == (LD_OK, plain)
