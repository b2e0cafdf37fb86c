"""What the decode / copy pair (k_inflate_seg + k_lzcopy) hands back to k_inflate, and why.  Written once and run twice:
through the emulated library on CPU (tests/test_emu_handback.py) and through the real HIP library on the MI355X
(tests/test_gpu_handback.py).

A hand-back costs speed and nothing else -- k_inflate decodes the member again, the bytes are right either way -- so a
test that compares bytes cannot see the pair refuse a member it should take.  These tests look at the hand-back itself:
DContext.last_redo_count() (production kernels) and DContext.debug_handback() (the instrumented kernels' reason,
GZPX_HANDBACK_*).  Bytes and error classes stay tests/inflate_cases.py's business.

Every check decodes ONE member per launch, route seg, on a context whose first-block hint nobody has written:
k_inflate_seg keeps that hint in the context, any member of a launch whose first block is not its last writes it and
any such member reads it (tests/scan_cases.py), so with several unlike members in a launch, or a context with a past, a
hand-back can depend on the order the hardware took the members in.  One member on such a context is the same integer
arithmetic on the emulator and on the GPU.  A member that would touch the hint gets a context made for it; the others
share one (Contexts below says why that is the same thing).

No stream here is damaged at random: the crafted ones are built field by field (tests/inflate_cases.py), all others are
valid, and every expected outcome is written down before the run."""
import contextlib
import ctypes
import functools
import zlib

import numpy as np

import alphabet_cases
import deflate_craft as dc
import inflate_cases as ic
import scan_cases
from gzp_amd import _native, synth

N = _native
DECODES = N.HANDBACK_NONE
REASON_NAMES = {getattr(N, k): k for k in dir(N) if k.startswith("HANDBACK_")}

# ------------------------------------------------------------------------------------------------ a. crafted streams
# For each of the 78 streams of inflate_cases.cases(): DECODES, or the one reason the pair must hand it back for.  Written
# from what the stream is built to break and from DESIGN section 8 ("What the pair does not judge it hands back"), not
# from what the kernel reports:
#   * seg_header refuses block type 3, a code whose shape libdeflate refuses (over-subscribed; incomplete, except the
#     empty code and the single codeword of length 1), a header whose runs are wrong (16 with nothing before it, an unused
#     precode codeword), a litlen code without an end-of-block code, stored LEN / NLEN that disagree    -> HEADER
#   * a stored block past the payload or past ISIZE                                                      -> STORED
#   * the span's bytes overrun ISIZE, or its end-of-block code lies behind the payload                   -> SPAN_OVERRUN
#   * pass 3 on the true path: distance before the start -> DISTANCE, offset symbols 30 / 31 -> OFFSET_SYMBOL,
#     litlen symbols 286 / 287 (which seg_entry gives the "invalid" entry)                               -> CODEWORD
#   * behind the final block fewer bytes than ISIZE                                                      -> FINAL
_H, _S, _O = N.HANDBACK_HEADER, N.HANDBACK_STORED, N.HANDBACK_SPAN_OVERRUN
CRAFTED = {
    # code shape: litlen
    "litlen_incomplete": _H, "litlen_incomplete_long": _H, "litlen_oversubscribed": _H, "litlen_oversubscribed_long": _H,
    "litlen_only_eob_bit0": DECODES, "litlen_only_eob_bit1": DECODES,  # the single codeword of length 1: a code like any other
    "litlen_only_eob_alone": DECODES,  # (ISIZE 0: never inflated)
    "litlen_single_len2": _H,          # a single codeword of length 2 is incomplete
    "litlen_single_len1_literal": _H,  # no end-of-block code
    # code shape: offset
    "offset_incomplete": _H, "offset_incomplete_long": _H, "offset_oversubscribed": _H, "offset_oversubscribed_long": _H,
    "offset_empty_unused": DECODES, "offset_empty_used_bit0": DECODES, "offset_empty_used_bit1": DECODES,
    "offset_empty_wide_used": DECODES,  # the empty code decodes symbol 0 from every bit
    "offset_single_len1_bit0": DECODES, "offset_single_len1_bit1": DECODES, "offset_single_len1_sym0_bit1": DECODES,
    "offset_single_len2": _H, "offset_single_len2_unused": _H,
    # code shape: precode
    "precode_incomplete": _H, "precode_oversubscribed": _H, "precode_single_len2": _H,
    # (a precode that spells 259 zeros: the empty litlen code has no end-of-block code)
    "precode_single_len1_bit0": _H, "precode_single_len1_bit1": _H, "precode_empty": _H,
    "precode_unused_codeword_sent": _H,
    # the code-length header
    "header_leading_16": _H,
    "header_run16_crosses": DECODES, "header_run17_crosses": DECODES, "header_run18_crosses": DECODES,
    "header_overrun_by_1": DECODES, "header_overrun_by_137": DECODES, "header_overrun_by_137_of_320": DECODES,
    "header_overrun_16": DECODES,
    "header_hclen_4": _H,  # every code length zero: no end-of-block code
    "header_hclen_19": DECODES,
    "header_hlit_29": DECODES, "header_hlit_30": DECODES, "header_hlit_31": DECODES,  # (286 / 287 have codewords, none is sent)
    "header_hdist_30": DECODES, "header_hdist_31": DECODES, "header_hdist_32": DECODES,
    "no_eob_output_fills": _H, "no_eob_input_ends": _H,
    # symbols
    "fixed_litlen_286_sent": N.HANDBACK_CODEWORD, "dynamic_litlen_286_sent": N.HANDBACK_CODEWORD,
    "fixed_litlen_287_sent": N.HANDBACK_CODEWORD, "dynamic_litlen_287_sent": N.HANDBACK_CODEWORD,
    # An invalid codeword is one bit long and produces nothing, and the path walks on (gzpx_inflate_seg.h): behind the
    # first bit of offset symbol 30 / 31 the rest of its codeword and the 14 raw bits are decoded as literals -- fixed:
    # 1110 / 1111 and five zeros are a 9-bit literal; dynamic: every zero bit is an 'a' -- and ISIZE has no room for one.
    # The span's byte count is held against ISIZE in front of pass 3, which would have named the symbol.  (The first
    # draft of this table said OFFSET_SYMBOL; EXTRA below holds the streams that reach it.)
    "fixed_offset_30_sent": _O, "dynamic_offset_30_sent": _O, "fixed_offset_31_sent": _O, "dynamic_offset_31_sent": _O,
    # (the codes that leave a codeword unused are incomplete: the header is refused before the codeword is met)
    "litlen_unused_codeword_root": _H, "litlen_unused_codeword_second_level": _H,
    "offset_unused_codeword_root": _H, "offset_unused_codeword_second_level": _H,
    "block_type_3": _H,
    # stored blocks
    "stored_nlen_mismatch": _H, "stored_len_past_payload": _S,
    "stored_len_0": DECODES,  # (ISIZE 0: never inflated)
    "stored_len_0_then_fixed": DECODES, "stored_len_65535": DECODES,
    # output accounting
    "distance_one_before_start": N.HANDBACK_DISTANCE, "distance_to_start": DECODES,
    "over_isize_by_literal": _O, "over_isize_by_match": _O, "over_isize_by_stored": _S,
    "over_isize_by_literal_dynamic": _O, "over_isize_by_match_dynamic": _O,
    "short_of_isize": N.HANDBACK_FINAL,
    "final_block_ends_on_last_bit": DECODES,
    "ends_whole": DECODES,
    # 40 bytes hold the 74 bits in front of the code lengths and some eighty of the 263 lengths, all of them zero (the
    # literals below 'a'); the rest is read from the member's footer and the zeros behind it, so the end-of-block code
    # gets no length -- or the code no shape
    "ends_inside_header": _H,
    # the true path runs on into the member's footer; the end-of-block code of both streams is all zeros (one bit here,
    # seven in the fixed code) and ISIZE's upper bytes are zeros, so the block "ends" behind the payload
    "ends_inside_symbol": _O, "ends_inside_extra_bits": _O,
}
# Valid streams -- libdeflate's recorded verdict is OK with ISIZE filled -- that the pair hands back all the same:
VALID_BUT_HANDED_BACK = {
    "fixed_litlen_286_sent": "seg_entry gives litlen 286 the invalid entry (libdeflate decodes it as length 258): k_inflate's",
    "fixed_litlen_287_sent": "as 286",
    "dynamic_litlen_286_sent": "as the fixed code's 286, with a codeword of its own",
    "dynamic_litlen_287_sent": "as 286",
}
# the LAB_NOTES case (a bite check broke code_shape so that the single codeword of length 1 was refused, and no test
# failed): these must NOT be handed back
SINGLE_CODEWORD = ("litlen_only_eob_bit0", "litlen_only_eob_bit1", "offset_single_len1_bit0", "offset_single_len1_bit1",
                   "offset_single_len1_sym0_bit1", "offset_empty_used_bit0", "offset_empty_used_bit1", "offset_empty_wide_used")




def _offset_fits(sym):
    """'a', a match of three whose offset symbol is 30 / 31, and behind the ONE bit the pair takes for it a stream that
    goes on as if nothing were wrong: the codeword's other four bits (1110 / 1111) and five zeros are a 9-bit literal of
    the fixed code, then the end-of-block code.  Five bytes, and ISIZE says five: the span passes, pass 3 names the symbol."""
    w = dc.BitWriter()
    dc.fixed(w, [("lit", ic.A), ("match", 257, 0, sym, 0), ("raw", 0, 5), ("eob",)], True)
    return ic.Case("fixed_offset_%d_fits" % sym, w.getvalue(), 5)


# streams of this module's own, for the reasons none of the 78 reaches (libdeflate: an invalid offset symbol, BAD_DATA)
EXTRA = [_offset_fits(30), _offset_fits(31)]
CRAFTED.update({x.name: N.HANDBACK_OFFSET_SYMBOL for x in EXTRA})


def crafted_cases():
    return ic.cases() + EXTRA


def crafted_names():
    return [x.name for x in crafted_cases()]


def check_table(verdicts):
    """The table names every crafted stream, and agrees with libdeflate's recorded verdicts: OK with ISIZE filled <=>
    the pair decodes it, but for VALID_BUT_HANDED_BACK."""
    assert sorted(CRAFTED) == sorted(crafted_names()) and len(ic.cases()) == 78
    assert set(SINGLE_CODEWORD) <= set(CRAFTED) and all(CRAFTED[n] == DECODES for n in SINGLE_CODEWORD)
    for x in ic.cases():
        v = verdicts[x.name]
        filled = v["rc"] == ic.LD_OK and v.get("out_len", len(v.get("out_hex", "")) // 2) == x.isize
        if x.name in VALID_BUT_HANDED_BACK:
            assert filled and CRAFTED[x.name] != DECODES, x.name
        else:
            assert (CRAFTED[x.name] == DECODES) == (filled or x.isize == 0), (x.name, v["rc"], REASON_NAMES[CRAFTED[x.name]])


# ------------------------------------------------------------------------------------------------ one member, one context
def _fmt(fmt):
    return N.FORMAT_BGZF if fmt == dc.BGZF else N.FORMAT_MGZIP


class Contexts:
    """Where a member gets its context from.  A member whose first block is not its last gets a context of its own: it
    reads and writes the first-block hint.  A member whose first block is final does neither (seg_member: `hinted`), so
    all of those share one context per format, whose hint nobody ever writes: on the GPU a context's streams, pinned
    and device tables cost more than every launch made on it, and these tests make three thousand launches."""

    def __init__(self, lib):
        self.lib, self.shared, self.made = lib, {}, 0

    @contextlib.contextmanager
    def ctx(self, fmt, raw):
        if raw[0] & 1:  # BFINAL of the first block
            if fmt not in self.shared:
                self.shared[fmt] = N.DContext(format=_fmt(fmt), lib=self.lib)
                self.made += 1
            yield self.shared[fmt]
        else:
            self.made += 1
            with N.DContext(format=_fmt(fmt), lib=self.lib) as d:
                yield d

    def close(self):
        for d in self.shared.values():
            d.close()
        self.shared = {}


def _payload(fmt, member):
    return member[18 if fmt == dc.BGZF else 20:]


def framed(cx, fmt, member, debug):
    """(bytes or the GzpxError, reason, hand-backs) of one framed member alone in a launch."""
    with cx.ctx(fmt, _payload(fmt, member)) as d:
        d.set_route(N.INFLATE_SEG)
        d.debug_inflate(1 if debug else 0)
        try:
            out = d.decompress(member)
        except N.GzpxError as e:
            out = e
        return out, d.debug_handback(1)[0], d.last_redo_count()


def check_framed(cx, fmt, member, want, what, plain=None):
    """The instrumented kernels give the reason `want`; the production ones hand back, or not, accordingly."""
    out, reason, redo = framed(cx, fmt, member, True)
    assert REASON_NAMES[reason] == REASON_NAMES[want], (what, "instrumented")
    assert redo == (want != DECODES), (what, "instrumented", redo)
    if plain is not None:
        assert out == plain, (what, "bytes")
    out, reason, redo = framed(cx, fmt, member, False)
    assert reason == N.HANDBACK_NONE, (what, "the production kernels record no reason")
    assert redo == (want != DECODES), (what, "production", redo)
    if plain is not None:
        assert out == plain, (what, "bytes")


def _crafted_member(x, verdicts):
    v = verdicts.get(x.name, {"rc": ic.LD_BAD_DATA})
    out = ic._known_out(v, x) if v["rc"] == ic.LD_OK and x.isize else b""
    return dc.wrap(x.fmt, x.raw, zlib.crc32(out), x.isize)


def check_crafted(cx, verdicts, name):
    """a / b: the crafted stream as a framed member.  Among them the single-codeword members of SINGLE_CODEWORD
    (litlen_only_eob_bit0 / bit1, offset_single_len1_bit0 / bit1 / sym0_bit1, offset_empty_used_bit0 / bit1,
    offset_empty_wide_used), which a code_shape that refuses a single codeword of length 1 hands back: the gap
    docs/LAB_NOTES.md found is closed here."""
    x = next(c for c in crafted_cases() if c.name == name)
    check_framed(cx, x.fmt, _crafted_member(x, verdicts), CRAFTED[name], name)


# ------------------------------------------------------------------------------------------------ d. the raw wrapper
class _Result:
    pass


def _raw_call(cx, raw, cap, count):
    """One RAW member alone in a batch, instrumented: the count-only kernels
    (gzpx_inflate_batch_sizes_device, the exact size as the cap) or the writing ones (gzpx_inflate_batch_device, a slot
    of the exact size).  Both see the same bytes at the same alignment: one byte in front, sixteen zeros behind."""
    lib = cx.lib
    mem = scan_cases.Mem(lib)
    blob = b"\xa5" + bytes(raw) + bytes(16)
    keep = [mem.put(blob), mem.put(np.array([1, 0], dtype=np.uint64).view(np.uint8)),
            mem.put(np.array([len(raw), 0], dtype=np.uint32).view(np.uint8)), mem.put(np.array([cap, 0], dtype=np.uint32).view(np.uint8)),
            mem.put(np.zeros(2, dtype=np.uint32).view(np.uint8)), mem.put(np.zeros(cap + 16, dtype=np.uint8))]
    (_, d_in), (_, p_off), (_, p_size), (h_osz, p_osz), (h_used, p_used), (h_out, d_out) = keep
    r = _Result()
    total, n_failed, out_len = ctypes.c_uint64(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    info = N.GzpxCheckInfo()
    with cx.ctx(dc.BGZF, raw) as d:  # (any context serves, whatever format it was made for)
        d.set_route(N.INFLATE_SEG)
        d.debug_inflate(1)
        if count:
            r.rc = lib.L.gzpx_inflate_batch_sizes_device(d.h, N.WRAP_RAW, d_in, len(blob), p_off, p_size, 1, cap, p_osz, p_used, None,
                                                         ctypes.byref(total), ctypes.byref(n_failed), ctypes.byref(info), None)
            r.size = int(np.frombuffer(mem.get(h_osz, 4), dtype=np.uint32)[0])
            r.used = int(np.frombuffer(mem.get(h_used, 4), dtype=np.uint32)[0])
        else:
            r.rc = lib.L.gzpx_inflate_batch_device(d.h, N.WRAP_RAW, 0, d_in, len(blob), p_off, p_size, p_osz, 1, d_out, cap, None, None,
                                                   ctypes.byref(out_len), ctypes.byref(n_failed), ctypes.byref(info), None)
            r.out = mem.get(h_out, cap)
        r.reason, r.redo = d.debug_handback(1)[0], d.last_redo_count()
    del keep
    return r


def check_raw(cx, raw, cap, want, what, plain=None):
    """COUNT mode hands back the same member for the same reason as the writing launch.  The one allowance: the writing
    kernel's last check, fewer bytes than ISIZE, has no counterpart where the size is a cap and not a claim."""
    r = _raw_call(cx, raw, cap, False)
    assert REASON_NAMES[r.reason] == REASON_NAMES[want], (what, "writing")
    assert r.redo == (want != DECODES), (what, "writing", r.redo)
    if plain is not None:
        assert r.rc == N.OK and r.out == plain, (what, "bytes")
    want_count = DECODES if want == N.HANDBACK_FINAL else want
    r = _raw_call(cx, raw, cap, True)
    assert REASON_NAMES[r.reason] == REASON_NAMES[want_count], (what, "count-only")
    assert r.redo == (want_count != DECODES), (what, "count-only", r.redo)
    if plain is not None:
        # (the hostile encoder leaves garbage behind some final blocks: the stream's own length is tests/size_cases.py's)
        assert r.rc == N.OK and r.size == len(plain) and 0 < r.used <= len(raw), (what, "sizes", r.size, r.used)


def check_crafted_raw(cx, name):
    """d: the crafted stream in the RAW wrapper.  A member whose ISIZE is 0 has no counterpart (a framed one is never
    inflated; a cap of 0 means none).  The streams that end early are read into what lies behind them: a framed
    member's footer there, zeros here -- the all-zero codeword of those streams is the end-of-block code, so the block
    ends behind the payload here too."""
    x = next(c for c in crafted_cases() if c.name == name)
    assert x.isize > 0
    check_raw(cx, x.raw, x.isize, CRAFTED[name], name)


RAW_NAMES = [x.name for x in crafted_cases() if x.isize > 0]


# ------------------------------------------------------------------------------------------------ c. valid but hostile
HOSTILE_SEED, HOSTILE_MEMBERS = 7300, 120
HOSTILE_SIZES = (0, 1, 2, 3, 258, 259, 700, 3000, 9000, 20000)
# The members of hostile() that hit the re-synchronisation limit (kSegMaxFix pass-2 iterations).  A RECORD taken from the
# emulator, not a derivation: its job is to show that the GPU and the emulator agree and to make drift visible.  A
# deliberate change of kSegMaxFix or of the span rules updates it and says why.
HOSTILE_RESYNC = (8, 38, 67, 79, 89, 107, 109)
ZLIB_CLASSES = ("text", "dna", "fastq", "runs", "zeros", "random")
ZLIB_SIZES = (259, 3000, 5000, 20000, 60000)
ZLIB_STRATEGIES = (("huffman_only", zlib.Z_HUFFMAN_ONLY), ("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("default", zlib.Z_DEFAULT_STRATEGY))
ZLIB_LEVELS = (1, 9)
# ... of zlib_members(), by name: the same kind of record
ZLIB_RESYNC = ("runs_5000_huffman_only_1", "runs_5000_huffman_only_9", "zeros_60000_fixed_1")
# ... of alphabet_members(): none
ALPHABET_RESYNC = ()


@functools.lru_cache(maxsize=None)
def hostile():
    """[(name, raw, plain)]: the hostile encoder (deflate_craft.encode) over the synth classes and the edge sizes."""
    rng = np.random.default_rng(HOSTILE_SEED)
    classes = sorted(synth.CLASSES)
    out = []
    for i in range(HOSTILE_MEMBERS):
        a = synth.make(classes[i % len(classes)], HOSTILE_SIZES[i % len(HOSTILE_SIZES)], HOSTILE_SEED + i).tobytes()
        raw, _ = dc.encode(a, rng, max_payload=ic.BGZF_MAX_PAYLOAD)
        out.append((i, raw, a))
    return out


@functools.lru_cache(maxsize=None)
def zlib_members():
    """[(name, raw, plain)]: zlib at the strategies that make streams unlike a compressor's default."""
    out = []
    for ci, cls in enumerate(ZLIB_CLASSES):
        for n in ZLIB_SIZES:
            a = synth.make(cls, n, 900 + ci).tobytes()
            for sname, strategy in ZLIB_STRATEGIES:
                for level in ZLIB_LEVELS:
                    raw = dc.zlib_payload(a, level, strategy)
                    assert len(raw) <= ic.BGZF_MAX_PAYLOAD
                    out.append(("%s_%d_%s_%d" % (cls, n, sname, level), raw, a))
    assert len(out) == 240
    return out


@functools.lru_cache(maxsize=None)
def alphabet_members():
    """[(name, raw, plain)]: tests/alphabet_cases.py's decode members -- every length and offset symbol, distance 32,768."""
    return [("%s_%d" % (code, k), raw, plain) for code in alphabet_cases.CODES
            for k, (raw, plain) in enumerate(alphabet_cases.decode_streams(code, dc.BGZF))]


def check_valid(cx, members, record, fmt=dc.BGZF):
    """c: every member's bytes are its input's; a member is handed back for the re-synchronisation limit or not at all
    (k_lzcopy's reason among those that never appear); and the members that are, are the recorded ones."""
    got = []
    for name, raw, plain in members:
        member = dc.wrap(fmt, raw, zlib.crc32(plain), len(plain))
        out, reason, redo = framed(cx, fmt, member, True)
        assert out == plain, (name, "bytes")
        assert reason in (N.HANDBACK_NONE, N.HANDBACK_RESYNC), (name, REASON_NAMES[reason])
        assert redo == (reason != N.HANDBACK_NONE), (name, redo)
        out, _, redo_production = framed(cx, fmt, member, False)
        assert out == plain and redo_production == redo, (name, "production", redo_production)
        if reason:
            got.append(name)
    assert tuple(got) == tuple(record), got


def check_valid_raw(cx, members, record):
    """d: the same members in the RAW wrapper, count-only and writing."""
    for name, raw, plain in members:
        if len(plain) == 0:
            continue  # (a cap of 0 means none)
        check_raw(cx, raw, len(plain), N.HANDBACK_RESYNC if name in record else DECODES, name, plain)


# ------------------------------------------------------------------------------------------------ e. the W = 8 launch form
BIG_SEED = 7200
# ... of big_members(), by name: the same kind of record
# (the zeros: with eight waves a member the __syncthreads_or arm of the limit is the one that fires)
BIG_RESYNC = ("zeros_fixed_1MiB",)


@functools.lru_cache(maxsize=None)
def big_members():
    """[(name, Mgzip member, plain)]: inflate_cases.hostile_mgzip's three members around SEG_BIG_BYTES, and 1 MiB of
    zeros as zlib's Z_FIXED writes them (4,065 times the same 13 bits: a lane that starts inside that period decodes a
    parse of its own that never meets the true one), brought to SEG_BIG_BYTES with garbage behind the final block."""
    out = [("hostile_%d" % len(m), m, plain) for m, plain, _ in ic.hostile_mgzip(BIG_SEED)[0]]
    a = bytes(1 << 20)
    raw = dc.zlib_payload(a, 1, zlib.Z_FIXED)
    raw += np.random.default_rng(BIG_SEED).integers(0, 256, ic.SEG_BIG_BYTES - 28 - len(raw), dtype=np.uint8).tobytes()
    out.append(("zeros_fixed_1MiB", dc.mgzip_wrap(raw, zlib.crc32(a), len(a)), a))
    assert all(len(m) >= ic.SEG_BIG_BYTES for _, m, _ in out[1:]) and len(out[0][1]) == ic.SEG_BIG_BYTES - 1
    return out


def check_big(cx):
    """e: each member its own slab, so the slab's average is the member's size: the first in the W = 1 form, the others
    with eight waves a member."""
    got = []
    for name, member, plain in big_members():
        out, reason, redo = framed(cx, dc.MGZIP, member, True)
        assert out == plain, (name, "bytes")
        assert reason in (N.HANDBACK_NONE, N.HANDBACK_RESYNC), (name, REASON_NAMES[reason])
        assert redo == (reason != N.HANDBACK_NONE), (name, redo)
        out, _, redo_production = framed(cx, dc.MGZIP, member, False)
        assert out == plain and redo_production == redo, (name, "production", redo_production)
        if reason:
            got.append(name)
    assert tuple(got) == BIG_RESYNC, got
