"""The length limit of the Huffman codes -- make_code's sequential branch in k_huffman and its second copy, the
near-optimal parser's no_make_code_lens -- written once and run twice: through the emulated library on CPU
(tests/test_emu_huffman_limit.py) and through the real HIP library on the MI355X (tests/test_gpu_huffman_limit.py).

A code "takes the limit path" when libdeflate's tree for its histogram, built without a limit, has a leaf deeper than
the code's limit (literal/length 14, offset 15, precode 7).  Text never does that, so every input here is built for
it, and every case asserts the property on the CPU before the library is called: read() rebuilds the three histograms
of every DEFLATE block from the oracle's own stream, unlimited_depth() builds the tree in plain Python, and the longest
transmitted length has to be exactly the limit.

The checks are byte-exact: the framed stream against oracle.compress_stream, the raw stream against the SHA-256 that
tests/golden/make_huffman_limit_golden.py recorded from the libdeflate 1.10 binary, and the stream inflated again on
both routes of the GPU inflater (codes of 14 and 15 bits: the deepest second-level tables)."""
import functools
import hashlib
import json
import os
import sys

import numpy as np

from gzp_amd import _native, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import deflate_tokens as dt  # noqa: E402

BLOCK = 65280
MAXL = {"litlen": 14, "offset": 15, "precode": 7}


@functools.lru_cache(maxsize=None)
def vectors():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "huffman_limit_vectors.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ reading a stream
def _decode_table(lens):
    """(table, bits): table[the next `bits` bits of the stream] = symbol << 4 | length, -1 where no codeword begins."""
    bits = max(lens)
    tab = np.full(1 << max(bits, 1), -1, dtype=np.int32)
    code = 0
    for ln in range(1, bits + 1):
        for sym, l in enumerate(lens):
            if l == ln:
                rev = int(format(code, "0%db" % ln)[::-1], 2)
                tab[rev::1 << ln] = sym << 4 | ln
                code += 1
        code <<= 1
    return tab.tolist(), max(bits, 1)


def read(raw):
    """A raw DEFLATE stream -> one dict per block: type; for a coded block the histograms of the literal/length
    symbols (end-of-block included) and of the offset symbols, the numbers of literals and matches, and the two length
    arrays; for a dynamic block also the histogram of the precode symbols in its header and the precode's lengths.
    Reading stops behind the final block: a member's trailer, or further members, may follow."""
    b = np.frombuffer(bytes(raw) + bytes(8), dtype=np.uint8).astype(np.uint64)
    # word[k] = the 40 bits from byte k on: any field of up to 33 bits is one shift and one mask away
    word = (b[:-4] | b[1:-3] << np.uint64(8) | b[2:-2] << np.uint64(16) | b[3:-1] << np.uint64(24) | b[4:] << np.uint64(32)).tolist()
    pos = 0

    def get(n):
        nonlocal pos
        v = (word[pos >> 3] >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def sym(tab, bits):
        nonlocal pos
        e = tab[(word[pos >> 3] >> (pos & 7)) & ((1 << bits) - 1)]
        if e < 0:
            raise ValueError("no codeword at bit %d" % pos)
        pos += e & 15
        return e >> 4

    blocks = []
    while True:
        final, typ = get(1), get(2)
        blk = {"type": typ, "litlen_hist": None, "offset_hist": None, "precode_hist": None, "litlen_lens": None,
               "offset_lens": None, "precode_lens": None, "literals": 0, "matches": 0}
        if typ == 0:
            pos = (pos + 7) & ~7
            n = get(16)
            get(16)
            pos += 8 * n
            blk["literals"] = n
        else:
            if typ == 1:
                ll, dl = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
            else:
                hlit, hdist, hclen = get(5) + 257, get(5) + 1, get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[dt.ORDER[i]] = get(3)
                ptab, pbits = _decode_table(cl)
                lens, ph = [], [0] * 19
                while len(lens) < hlit + hdist:
                    s = sym(ptab, pbits)
                    ph[s] += 1
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + get(2))
                    elif s == 17:
                        lens += [0] * (3 + get(3))
                    else:
                        lens += [0] * (11 + get(7))
                assert len(lens) == hlit + hdist
                ll, dl = lens[:hlit], lens[hlit:]
                blk["precode_hist"], blk["precode_lens"] = ph, cl
            ltab, lbits = _decode_table(ll)
            dtab, dbits = _decode_table(dl)
            lh, dh = [0] * 288, [0] * 30
            while True:
                s = sym(ltab, lbits)
                lh[s] += 1
                if s == 256:
                    break
                if s > 256:
                    pos += dt.LEXT[s - 257]
                    d = sym(dtab, dbits)
                    dh[d] += 1
                    pos += dt.DEXT[d]
            blk["litlen_hist"], blk["offset_hist"], blk["litlen_lens"], blk["offset_lens"] = lh, dh, ll, dl
            blk["literals"], blk["matches"] = sum(lh[:256]), sum(lh[257:])
        blocks.append(blk)
        if final:
            assert (pos + 7) >> 3 <= len(raw), (pos, len(raw))
            return blocks


def unlimited_depth(freqs):
    """The deepest leaf of libdeflate's Huffman tree for `freqs`, built without a length limit: leaves sorted by
    (frequency, symbol), the two smallest nodes taken one at a time from two queues (sorted leaves, internal nodes
    in the order they were made), a leaf preferred where a leaf and an internal node tie."""
    leaves = sorted((f, s) for s, f in enumerate(freqs) if f)
    if len(leaves) < 2:
        return 1 if leaves else 0
    node_freq, node_parent, leaf_parent = [], [], [None] * len(leaves)
    i = b = 0
    for e in range(len(leaves) - 1):
        total = 0
        for _ in range(2):
            if i < len(leaves) and (b == len(node_freq) or leaves[i][0] <= node_freq[b]):
                total += leaves[i][0]
                leaf_parent[i] = e
                i += 1
            else:
                total += node_freq[b]
                node_parent[b] = e
                b += 1
        node_freq.append(total)
        node_parent.append(None)
    depth = [0] * len(node_freq)
    for k in range(len(node_freq) - 2, -1, -1):
        depth[k] = depth[node_parent[k]] + 1
    return max(depth[p] for p in leaf_parent) + 1


def limited(blk, code):
    """The block's code took the limit path."""
    return blk[code + "_hist"] is not None and unlimited_depth(blk[code + "_hist"]) > MAXL[code]


def assert_limited(blk, code, at_least=None):
    """The property of every case here: without a limit the tree is deeper than the limit, and the longest transmitted
    length is the limit itself.  Returns the unlimited depth."""
    assert blk["type"] == 2, blk["type"]
    d = unlimited_depth(blk[code + "_hist"])
    assert d > MAXL[code], (code, d)
    assert at_least is None or d >= at_least, (code, d, at_least)
    assert max(blk[code + "_lens"]) == MAXL[code], (code, max(blk[code + "_lens"]))
    return d


# ------------------------------------------------------------------------------------------------ literal/length inputs
def _fib(n):
    """1, 2, 3, 5, 8, ...: n terms."""
    out, a, b = [], 1, 2
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


FILLERS, FILLER_COUNT = range(0x80, 0xC0), 400
# The rare symbols 0x20.. carry 1, 2, 3, 5, ... and end-of-block the other 1 of the chain.  A term adds a level to the
# tree while the chain's sum stays below the fillers' count: with fillers at 400, eight terms give a tree of depth 15,
# one over the limit, and eleven or more give 18 (thirteen are used: 26,585 bytes).  A deeper tree needs heavier fillers,
# and 64 of them, so that three-byte windows stay unique: depth 21 takes 64 x 1,600 + 14 terms = 103,995 bytes, more
# than a BGZF block holds and more than level 1 puts into one DEFLATE block (65,535), so that input is an Mgzip block
# and reaches 21 at levels 2 and up; at level 1 its first DEFLATE block has depth 18 and its second 14.
LITLEN_INPUTS = {"litlen 15": (8, 400), "litlen 18": (13, 400), "litlen 21": (14, 1600)}


@functools.lru_cache(maxsize=None)
def litlen_input(chain, filler_count=FILLER_COUNT, seed=1):
    """Bytes with an exact histogram -- 64 fillers at 400 each and `chain` rare symbols with Fibonacci counts -- in
    which no three-byte window occurs twice: no parser of any level finds a match, so the stream is one block of
    literals and its literal/length histogram is the byte histogram plus one end-of-block.  Drawn symbol by symbol
    from the remaining counts; a draw that would repeat a window is rejected.  (A plain shuffle leaves a few chance
    matches, and they flatten the chain.)"""
    syms = np.concatenate([np.arange(0x20, 0x20 + chain), np.array(FILLERS)])
    counts = np.concatenate([np.array(_fib(chain)), np.full(len(FILLERS), filler_count)])
    for attempt in range(20):
        pool = np.random.default_rng([seed, chain, filler_count, attempt]).permutation(np.repeat(syms, counts)).tolist()
        n, seen, ok = len(pool), set(), True
        for p in range(2, n):
            head = pool[p - 2] << 16 | pool[p - 1] << 8
            j = p
            while j < n and (head | pool[j]) in seen:
                j += 1
            if j == n:  # the remaining symbols all repeat a window: draw the whole sequence again
                ok = False
                break
            pool[p], pool[j] = pool[j], pool[p]
            seen.add(head | pool[p])
        if ok:
            break
    assert ok
    a = np.array(pool, dtype=np.uint8)
    assert np.array_equal(np.bincount(a, minlength=256)[syms], counts)
    w = a[:-2].astype(np.uint32) << 16 | a[1:-1].astype(np.uint32) << 8 | a[2:]
    assert np.unique(w).size == w.size
    a.flags.writeable = False
    return a


# ------------------------------------------------------------------------------------------------ the offset input
UNIT = 7
FRESH_UNITS = 1171
LAST_CODE = 24  # the chain of the offset code: counts 1, 1, 2, 3, ... on the distance codes from `first_code` to this one


@functools.lru_cache(maxsize=None)
def offset_input(seed=3, fresh_units=FRESH_UNITS, lead=0, first_code=7):
    """Copies at chosen distance codes.  A unit is a six-byte window of bytes < 0x80 and one separator >= 0x80.  After
    `fresh_units` units of fresh windows, every further unit repeats the window of an earlier unit that is still the
    last occurrence of its window, 7 * (units back) bytes away -- a distance chosen to fall in the range of the wanted
    distance code.  Windows and separators are drawn by rejection so that no three-byte window occurs twice apart from
    the four inside each copy: the nearest occurrence is the only candidate of full length, six bytes, and nothing else
    matches anywhere.  Distance codes 7..24 get the counts 1, 1, 2, 3, ..., 2584: 6,764 copies and a tree of depth 17;
    that is what a block has room for (a chain one step longer needs 10,945 copies).  With `first_code` 8 the chain is
    one step shorter, 1, 1, 2, ..., 1597 on the codes 8..24, and the tree has depth 16, one over the limit.  1,171 fresh units are 8,197 bytes, more than the farthest wanted
    distance (6,144 bytes, 877 units) looks back.  `lead` copies at the farthest code come before the chain's, on top
    of its counts."""
    for attempt in range(20):
        try:
            a = _offset_units(np.random.default_rng([seed, fresh_units, lead, first_code, attempt]), fresh_units, lead, first_code)
            break
        except _DeadEnd:  # the last few copies found no live unit in their code's reach: draw everything again
            continue
    else:
        raise AssertionError("no sequence found")
    copies = a.size // UNIT - fresh_units
    w = a[:-2].astype(np.uint32) << 16 | a[1:-1].astype(np.uint32) << 8 | a[2:]
    assert np.unique(w).size == w.size - 4 * copies
    a.flags.writeable = False
    return a


class _DeadEnd(Exception):
    pass


def _offset_units(rng, fresh_units, lead, first_code):
    chain = range(first_code, LAST_CODE + 1)
    want = dict(zip(chain, [1] + _fib(len(chain) - 1)))
    ages = {}  # code -> (nearest, farthest) in units
    for c in chain:
        lo, hi = -(-dt.DBASE[c] // UNIT), (dt.DBASE[c + 1] - 1) // UNIT
        assert lo <= hi
        ages[c] = (lo, hi)
    total = fresh_units + lead + sum(want.values())
    assert total * UNIT <= BLOCK
    seen = set()
    out = []

    def unseen(keys):
        return len(set(keys)) == len(keys) and not any(k in seen for k in keys)

    def key(x, y, z):
        return x << 16 | y << 8 | z

    def append(win, fresh):
        if out:  # the separator behind the previous window, now that both of its neighbours are known
            for s in (rng.permutation(128) + 128).tolist():
                keys = [key(out[-2], out[-1], s), key(out[-1], s, win[0]), key(s, win[0], win[1])]
                if unseen(keys):
                    break
            else:
                raise AssertionError("no separator left")
            seen.update(keys)
            out.append(s)
        if fresh:
            seen.update(key(*win[k:k + 3]) for k in range(4))
        out.extend(win)

    live = np.zeros(total, dtype=bool)  # unit u holds the last occurrence of its window
    window = []
    for u in range(fresh_units):
        while True:
            win = rng.integers(0, 128, 6).tolist()
            if unseen([key(*win[k:k + 3]) for k in range(4)]):
                break
        append(win, True)
        window.append(win)
        live[u] = True
    for u in range(fresh_units, total):
        if u < fresh_units + lead:
            order = [LAST_CODE]  # a lead copy: the farthest code, not counted
        else:  # drawn from the remaining counts; the next draw where no live unit is in that code's reach
            codes = [c for c in chain if want[c]]
            left = np.array([want[c] for c in codes], dtype=np.float64)
            order = rng.choice(codes, size=len(codes), replace=False, p=left / left.sum()).tolist()
        for c in order:
            lo, hi = ages[c]
            cand = np.flatnonzero(live[max(u - hi, 0):u - lo + 1]) + max(u - hi, 0)
            if cand.size:
                break
        else:
            raise _DeadEnd
        src = int(cand[rng.integers(cand.size)])
        if u >= fresh_units + lead:
            want[c] -= 1
        live[src] = False
        live[u] = True
        append(window[src], False)
        window.append(window[src])
    assert not any(want.values())
    for s in (rng.permutation(128) + 128).tolist():
        if unseen([key(out[-2], out[-1], s)]):
            break
    out.append(s)
    a = np.array(out, dtype=np.uint8)
    assert a.size == total * UNIT
    return a


# ------------------------------------------------------------------------------------------------ the cases
OFFSET_LEAD = 300


def _one_literal_block(blocks, n):
    assert len(blocks) == 1 and blocks[0]["literals"] == n and blocks[0]["matches"] == 0


def claim_litlen(depth):
    def claim(data, blocks, level):
        _one_literal_block(blocks, data.size)
        assert assert_limited(blocks[0], "litlen") == depth
    return claim


def claim_litlen_21(data, blocks, level):
    """Levels 2 and up: one DEFLATE block, depth 21.  Level 1 ends a DEFLATE block after 65,535 bytes: the first has
    depth 18, the second stays within the limit -- two codes, one after the other out of the same HuffLds."""
    if level == 1:
        assert [b["literals"] for b in blocks] == [65535, data.size - 65535] and not any(b["matches"] for b in blocks)
        assert assert_limited(blocks[0], "litlen") == 18 and not limited(blocks[1], "litlen")
    else:
        _one_literal_block(blocks, data.size)
        assert assert_limited(blocks[0], "litlen") >= 21


def claim_offset(copies, depth):
    def claim(data, blocks, level):
        """Every copy is a match; the DEFLATE block that holds the chain (the only one at level 1, the last one where
        the block splitter cuts the literal prefix off) has an offset tree of the depth the chain was made for."""
        assert sum(b["matches"] for b in blocks) == copies
        assert len(blocks) == (1 if level == 1 else 2)
        assert assert_limited(blocks[-1], "offset") == depth
        assert not any(limited(b, "offset") for b in blocks[:-1])
    return claim


def claim_precode(data, blocks, level):
    hit = [b for b in blocks if limited(b, "precode")]
    assert hit
    for b in hit:
        assert assert_limited(b, "precode") == 8


# name -> (the input, its claim, the levels it is a limit case at)
INPUTS = {
    "litlen 15": (lambda: litlen_input(*LITLEN_INPUTS["litlen 15"]), claim_litlen(15), (1, 3, 6, 9)),
    "litlen 18": (lambda: litlen_input(*LITLEN_INPUTS["litlen 18"]), claim_litlen(18), (1, 3, 6, 9, 12)),
    "litlen 21": (lambda: litlen_input(*LITLEN_INPUTS["litlen 21"]), claim_litlen_21, (1, 3, 6, 9)),
    # Levels 2-9 end a DEFLATE block 194 copies after the literal prefix, and the chain that is left has depth 13 or 14:
    # the chain's margin is one count, so the largest counts must not lose a copy.  The `lead` variant makes 300 more
    # copies at the farthest code before the chain's: the cut falls among them, and k_huffman sees the whole chain at
    # levels 2-9 as well (measured at 2, 3, 6 and 9; 3 and 6 are run).  At levels 10 and 12 the chain also goes through
    # no_make_code_lens, whose lengths price the parse and are not transmitted: a wrong length shows there only where it
    # changes the tokens or leaves the arrays.
    "offset 16": (lambda: offset_input(first_code=8), claim_offset(4180, 16), (1, 10)),
    "offset 17": (lambda: offset_input(), claim_offset(6764, 17), (1, 10, 12)),
    "offset 17 lead": (lambda: offset_input(lead=OFFSET_LEAD), claim_offset(6764 + OFFSET_LEAD, 17), (3, 6)),
    # the two synth inputs of the suite whose precode happens to be limited, pinned so that they stay limit cases
    "precode mixed": (lambda: synth.make("mixed", BLOCK, 3), claim_precode, (1,)),
    "precode runs": (lambda: synth.make("runs", BLOCK, 3), claim_precode, (1,)),
}
ONE_BLOCK = [(name, level) for name, (_, _, levels) in INPUTS.items() for level in levels]


def compats(level):
    """Below level 10 both libdeflate generations; from 10 on the library runs 1.10's rules whatever it is asked for."""
    return (_native.COMPAT_1_10,) if level >= 10 else (_native.COMPAT_1_10, _native.COMPAT_1_24)


def vector(kind, **key):
    hit = [e for e in vectors()[kind] if all(e[k] == v for k, v in key.items())]
    assert len(hit) == 1, (kind, key)
    return hit[0]


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _inflates_back(lib, fmt, stream, data):
    for route in (_native.INFLATE_SEG, _native.INFLATE_WAVE):
        with _native.DContext(format=fmt, lib=lib) as d:
            d.set_route(route)
            assert d.decompress(stream) == data.tobytes(), route


# ------------------------------------------------------------------------------------------------ the checks
def check_one_block(lib, oracle, name, level):
    """One input, one level: the claim on the oracle's raw stream; then the library's Mgzip block and (where the input
    fits one) BGZF block against the oracle's, is_last true, in both compat modes below level 10; the raw stream of
    Compressor.deflate_compress against the libdeflate 1.10 binary's digest; both routes of the inflater."""
    make, claim, levels = INPUTS[name]
    assert level in levels
    data = make()
    ocompat = {_native.COMPAT_1_10: oracle.COMPAT_1_10, _native.COMPAT_1_24: oracle.COMPAT_1_24}
    formats = [("mgzip", _native.FORMAT_MGZIP, oracle.FMT_MGZIP, 20, max(data.size, BLOCK))]
    if data.size <= BLOCK:
        formats.insert(0, ("bgzf", _native.FORMAT_BGZF, oracle.FMT_BGZF, 18, BLOCK))
    for compat in compats(level):
        raw = oracle.deflate_compress(data, level, ocompat[compat])
        claim(data, read(raw), level)
        for fname, fmt, ofmt, hdr, bs in formats:
            want = oracle.compress_stream(data, ofmt, level, ocompat[compat], bs)
            assert want[hdr:hdr + len(raw)] == raw  # the block the claim was made on
            with _native.Context(format=fmt, level=level, buffer_size=bs, compat=compat, max_slab_bytes=bs, lib=lib) as ctx:
                got = ctx.compress_slab(data, is_last=True)
            assert got == want, (name, level, fname, compat, len(got), len(want))
            if compat == _native.COMPAT_1_10:
                assert _sha(got) == vector("streams", name=name, level=level, fmt=fname)["sha256"]
                _inflates_back(lib, fmt, got, data)
    c = _native.Compressor(level, _native.COMPAT_1_10, lib=lib)
    out = c.deflate_compress(data)
    c.close()
    e = vector("raw_deflate", name=name, level=level)
    assert (len(out), _sha(out)) == (e["size"], e["sha256"]), (name, level)


def check_oracle_vectors(oracle):
    """The oracle's own limit rule against the libdeflate 1.10 binary (tests/test_oracle_golden.py)."""
    for e in vectors()["raw_deflate"]:
        data = INPUTS[e["name"]][0]()
        assert (data.size, _sha(data.tobytes())) == (e["n"], e["input_sha256"]), e["name"]
        out = oracle.deflate_compress(data, e["level"], oracle.COMPAT_1_10)
        assert (len(out), _sha(out)) == (e["size"], e["sha256"]), (e["name"], e["level"])
    for e in vectors()["streams"]:
        data = INPUTS[e["name"]][0]()
        fmt = oracle.FMT_BGZF if e["fmt"] == "bgzf" else oracle.FMT_MGZIP
        out, sizes = oracle.compress_stream(data, fmt, e["level"], oracle.COMPAT_1_10, e["buffer_size"], True)
        assert _sha(out) == e["sha256"] and list(sizes) == e["block_sizes"], (e["name"], e["level"], e["fmt"])


# ------------------------------------------------------------------------------------------------ placements
def text(n, seed):
    return synth.english_like(n, seed).copy()


def _members(stream, sizes, hdr=18):
    """read() of every member of a framed stream."""
    at, out = 0, []
    for s in sizes:
        out.append(read(stream[at + hdr:at + int(s)]))
        at += int(s)
    return out


def placed_in_block():
    """The depth-18 input and then English-like text, one BGZF block.  Levels 2 and up end a DEFLATE block where the
    text begins: a limited sub-block (with the first matches of the text in it the tree has depth 15) and then an
    ordinary one, built by the same wave out of the same HuffLds.  Level 1 ends a DEFLATE block only after 8,192
    matches or 65,535 bytes, this block stays one sub-block, and its tree has depth 14 exactly: no limit case -- level
    1's limited code followed by an ordinary one is "litlen 21"."""
    a = litlen_input(*LITLEN_INPUTS["litlen 18"])
    return np.concatenate([a, text(BLOCK - a.size, 5)])


def placed_in_slab():
    """The same block between a block of text and a short one."""
    return np.concatenate([text(BLOCK, 6), placed_in_block(), text(30000, 7)])


PLACEMENTS = {"in a block of text": (placed_in_block, [True]), "middle block of three": (placed_in_slab, [False, True, False])}
PLACED = [(name, level) for name in PLACEMENTS for level in (3, 6)]


def check_placement(lib, oracle, name, level):
    make, where = PLACEMENTS[name]
    data = make()
    for compat, ocompat in ((_native.COMPAT_1_10, oracle.COMPAT_1_10), (_native.COMPAT_1_24, oracle.COMPAT_1_24)):
        want, sizes = oracle.compress_stream(data, oracle.FMT_BGZF, level, ocompat, BLOCK, return_block_sizes=True)
        members = _members(want, sizes)
        assert len(members) == len(where)
        for blocks, here in zip(members, where):
            hit = [limited(b, "litlen") for b in blocks]
            assert any(hit) == here
            if here:  # at least two dynamic sub-blocks, one limited and one not
                assert sum(b["type"] == 2 for b in blocks) >= 2 and not all(hit)
                for b, h in zip(blocks, hit):
                    if h:
                        assert_limited(b, "litlen")
        with _native.Context(format=_native.FORMAT_BGZF, level=level, buffer_size=BLOCK, compat=compat,
                             max_slab_bytes=3 * BLOCK, lib=lib) as ctx:
            got = ctx.compress_slab(data, is_last=True)
        assert got == want, (name, level, compat, len(got), len(want))
    _inflates_back(lib, _native.FORMAT_BGZF, got, data)
