"""A DEFLATE writer that makes every choice explicit (RFC 1951), for the inflate conformance tests.

Pure Python and numpy; no product code.  Three layers:

  BitWriter, canonical()        bits LSB first through an integer accumulator; canonical codewords of ANY length
                                vector (incomplete and over-subscribed ones included: the writer does not judge)
  stored / fixed / dynamic      block writers; a dynamic block takes HLIT / HDIST / HCLEN, the precode lengths and the
                                list of code-length symbols as given, so that runs may cross the litlen / offset
                                boundary or overrun it
  encode(data, rng)             a hostile but valid encoder: edge matches, random block types, random complete codes
                                of up to 15 bits, random header spellings; returns the stream and what it used

Tokens: ("lit", byte), ("lits", bytes), ("eob",), ("match", length symbol, extra, offset symbol, extra) -- see
match() -- and ("raw", value, nbits) for bits that are no codeword of the block's codes."""
import bisect
import struct
import zlib

import numpy as np

PRE_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
BGZF, MGZIP = 0, 1


# ------------------------------------------------------------------------------------------------ bits
class BitWriter:
    """Bits LSB first.  Whole bytes leave the integer accumulator for a bytearray as they fill, so the accumulator
    stays short; arrays of fields go in through numpy (fields())."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        if self.n >= 256:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def fields(self, values, nbits):
        """Many (value, nbits) fields at once (nbits <= 16 each), in order."""
        values = np.asarray(values, dtype=np.uint64)
        nbits = np.asarray(nbits, dtype=np.int64)
        if values.size == 0:
            return
        self._drain()
        pos = self.n + np.cumsum(nbits) - nbits
        total = int(self.n + nbits.sum())
        shifted = values << (pos & 7).astype(np.uint64)  # <= 23 bits
        byte = pos >> 3
        nbytes = (total + 7) // 8 + 3
        tmp = np.zeros(nbytes, dtype=np.int64)
        for k in range(3):  # (fields do not overlap, so sums of their bytes are ORs)
            tmp += np.bincount(byte + k, weights=((shifted >> np.uint64(8 * k)) & np.uint64(255)).astype(np.float64),
                               minlength=nbytes).astype(np.int64)
        tmp[0] += self.acc
        whole = total >> 3
        self.buf += tmp[:whole].astype(np.uint8).tobytes()
        self.acc = int(tmp[whole]) if total & 7 else 0
        self.n = total & 7

    def _drain(self):
        k = self.n >> 3
        if k:
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    @property
    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def align(self, fill=0):
        """Pad to a byte boundary with the low bits of `fill`."""
        pad = -self.n & 7
        self.bits(fill & ((1 << pad) - 1), pad)

    def raw_bytes(self, data):
        assert self.n & 7 == 0
        self._drain()
        self.buf += bytes(data)

    def getvalue(self):
        """The bytes so far; a last partial byte is padded with zero bits."""
        k = (self.n + 7) >> 3
        return bytes(self.buf) + (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")


def canonical(lens):
    """(codewords, lengths) as uint arrays: the canonical code of RFC 1951 3.2.2 for ANY length vector, each codeword
    bit-reversed (ready to be written LSB first).  An over-subscribed vector gives codewords that wrap around."""
    lens = np.asarray(lens, dtype=np.int64)
    count = np.bincount(lens, minlength=16)
    count[0] = 0
    nxt = np.zeros(17, dtype=np.int64)
    code = 0
    for l in range(1, 16):
        code = (code + int(count[l - 1])) << 1
        nxt[l] = code
    codes = np.zeros(lens.size, dtype=np.uint64)
    for s in np.nonzero(lens)[0]:
        l = int(lens[s])
        c = int(nxt[l]) & ((1 << l) - 1)
        nxt[l] += 1
        codes[s] = int(format(c, "0%db" % l)[::-1], 2)
    return codes, lens


def kraft(lens):
    """Sum of 2^(15 - len) over the used symbols: 1 << 15 for a complete code."""
    return sum(1 << (15 - l) for l in lens if l)


def balanced_lens(k):
    """Lengths of a complete code over k >= 2 symbols, as flat as possible (shorter codewords first)."""
    assert k >= 2
    m = (k - 1).bit_length()
    short = (1 << m) - k
    return [m - 1] * short + [m] * (k - short)


def random_complete_lens(k, maxlen, rng, deep=False):
    """Lengths of a random complete code over k >= 2 symbols, none longer than maxlen: leaves of a binary tree are
    split at random; `deep` prefers the deepest leaf that may still be split, which drives codewords to maxlen."""
    assert 2 <= k <= (1 << maxlen)
    leaves = [1, 1]
    while len(leaves) < k:
        can = [i for i, l in enumerate(leaves) if l < maxlen]
        if deep and rng.random() < 0.7:
            top = max(leaves[i] for i in can)
            can = [i for i in can if leaves[i] == top]
        i = can[int(rng.integers(len(can)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    return leaves


# ------------------------------------------------------------------------------------------------ tokens
def length_symbol(length, via_284=False):
    """(symbol, extra value) of a match length; 258 is symbol 285, or symbol 284 with extra 31 on request."""
    assert 3 <= length <= 258
    if length == 258:
        return (284, 31) if via_284 else (285, 0)
    s = bisect.bisect_right(LEN_BASE, length, 0, 28) - 1
    return 257 + s, length - LEN_BASE[s]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    s = bisect.bisect_right(DIST_BASE, dist) - 1
    return s, dist - DIST_BASE[s]


def match(length, dist, via_284=False):
    return ("match",) + length_symbol(length, via_284) + dist_symbol(dist)


def emit(w, tokens, litlen, dist):
    """Tokens through the codes litlen / dist (each as canonical() returns it)."""
    lc, ll = litlen
    dc, dl = dist
    for t in tokens:
        k = t[0]
        if k == "lit":
            w.bits(int(lc[t[1]]), int(ll[t[1]]))
        elif k == "lits":
            a = np.frombuffer(bytes(t[1]), dtype=np.uint8)
            w.fields(lc[a], ll[a])
        elif k == "eob":
            w.bits(int(lc[256]), int(ll[256]))
        elif k == "raw":
            w.bits(t[1], t[2])
        elif k == "match":
            _, ls, lx, ds, dx = t
            w.bits(int(lc[ls]), int(ll[ls]))
            if ls < 257 + 29:
                w.bits(lx, LEN_EXTRA[ls - 257])
            w.bits(int(dc[ds]), int(dl[ds]))
            if ds < 30:
                w.bits(dx, DIST_EXTRA[ds])
        else:
            raise ValueError(t)


# ------------------------------------------------------------------------------------------------ blocks
def stored(w, data, final, length=None, nlen=None, pad=0):
    """A stored block; LEN and NLEN may be given apart from the data that follows them."""
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align(pad)
    n = len(data) if length is None else length
    w.bits(n, 16)
    w.bits((n ^ 0xFFFF) if nlen is None else nlen, 16)
    w.raw_bytes(data)


def fixed(w, tokens, final):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    emit(w, tokens, canonical(FIXED_LITLEN), canonical(FIXED_DIST))


def plain_cl_syms(lens):
    """Every code length spelled out, no runs."""
    return [(int(l),) for l in lens]


def precode_for(cl_syms):
    """Lengths [19] of a flat complete precode over the symbols cl_syms uses (one more if it uses a single one)."""
    used = sorted({s[0] for s in cl_syms})
    if len(used) == 1:
        used = sorted(used + [(used[0] + 1) % 19])
    pre = [0] * 19
    for s, l in zip(used, balanced_lens(len(used))):
        pre[s] = l
    return pre


def dynamic(w, tokens, final, litlen_lens, dist_lens, hlit=None, hdist=None, hclen=None, pre_lens=None, cl_syms=None,
            code_litlen=None, code_dist=None):
    """A dynamic block.  litlen_lens / dist_lens are the codes the TOKENS are written with; the header says what
    cl_syms says -- by default the same lengths spelled out one by one, under a flat precode.  cl_syms entries:
    (length,), (16, extra), (17, extra), (18, extra).  hlit / hdist / hclen are the header's counts (257.., 1.., 4..)."""
    litlen_lens, dist_lens = list(litlen_lens), list(dist_lens)
    hlit = len(litlen_lens) if hlit is None else hlit
    hdist = len(dist_lens) if hdist is None else hdist
    if cl_syms is None:
        cl_syms = plain_cl_syms(litlen_lens + dist_lens)
    if pre_lens is None:
        pre_lens = precode_for(cl_syms)
    if hclen is None:
        hclen = max([4] + [i + 1 for i, s in enumerate(PRE_ORDER) if pre_lens[s]])
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for s in PRE_ORDER[:hclen]:
        w.bits(pre_lens[s], 3)
    pc, pl = canonical(pre_lens)
    for s in cl_syms:
        if s[0] == "raw":
            w.bits(s[1], s[2])
            continue
        w.bits(int(pc[s[0]]), int(pl[s[0]]))
        if s[0] >= 16:
            w.bits(s[1], (2, 3, 7)[s[0] - 16])
    pad = lambda v, n: list(v) + [0] * (n - len(v))
    emit(w, tokens, code_litlen or canonical(pad(litlen_lens, 288)), code_dist or canonical(pad(dist_lens, 32)))


def lens_from(d, floor):
    """A length list from {symbol: length}: as long as the highest symbol needs, and no shorter than `floor`."""
    n = max(floor, max(d) + 1 if d else 0)
    v = [0] * n
    for s, l in d.items():
        v[s] = l
    return v


# ------------------------------------------------------------------------------------------------ members
def bgzf_wrap(payload, crc, isize):
    """A BGZF member around a raw DEFLATE payload, with the footer fields as given."""
    assert len(payload) + 26 <= 65536
    hdr = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, ord("B"), ord("C"), 2, len(payload) + 25)
    return hdr + bytes(payload) + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def mgzip_wrap(payload, crc, isize):
    hdr = struct.pack("<BBBBIBBHBBHI", 31, 139, 8, 4, 0, 0, 255, 8, ord("I"), ord("G"), 4, len(payload) + 28)
    return hdr + bytes(payload) + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def wrap(fmt, payload, crc, isize):
    return (bgzf_wrap if fmt == BGZF else mgzip_wrap)(payload, crc, isize)


def zlib_payload(chunk, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(bytes(chunk)) + co.flush()


def bgzf_member(chunk, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """A BGZF member as zlib makes it."""
    chunk = bytes(chunk)
    return bgzf_wrap(zlib_payload(chunk, level, strategy), zlib.crc32(chunk), len(chunk))


# ------------------------------------------------------------------------------------------------ the hostile encoder
EDGE_KINDS = ("len3", "len258_sym285", "len258_sym284", "dist1_len258", "len_gt_dist", "dist32767", "dist32768",
              "dist_13_extra_bits", "match_to_last_byte")
STAT_KEYS = EDGE_KINDS + ("litlen15_used", "offset15_used", "stored_unaligned", "fixed_unaligned", "dynamic_unaligned",
                          "empty_stored", "blocks")


def _candidates(a):
    """Per position with three bytes left: the nearest earlier position with the same three bytes (or -1), and the
    farthest one that is still inside the window (or -1)."""
    n = a.size
    near = np.full(n, -1, dtype=np.int64)
    far = np.full(n, -1, dtype=np.int64)
    if n < 4:
        return near, far
    key = a[:-2].astype(np.int64) | (a[1:-1].astype(np.int64) << 8) | (a[2:].astype(np.int64) << 16)
    order = np.argsort(key, kind="stable")
    sk = key[order]
    same = np.zeros(order.size, dtype=bool)
    same[1:] = sk[1:] == sk[:-1]
    near[order[same]] = order[np.nonzero(same)[0] - 1]
    # the farthest inside the window: the first position of the same key that is >= i - 32768 (order is by key, then
    # by position, so a search for (key, i - 32768) in the sorted pairs finds it)
    pair = sk * (n + 1) + order
    j = np.searchsorted(pair, sk * (n + 1) + np.maximum(order - 32768, 0))
    cand = order[np.minimum(j, order.size - 1)]
    ok = (cand < order) & (key[cand] == sk)
    far[order[ok]] = cand[ok]
    return near, far


def _match_len(b, i, c, limit):
    """Length of the common prefix of b[i:] and b[c:], at most `limit` (the two may overlap)."""
    if b[i:i + limit] == b[c:c + limit]:
        return limit
    lo, hi = 0, limit  # b[i:i+lo] matches, b[i:i+hi] does not
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if b[i + lo:i + mid] == b[c + lo:c + mid]:
            lo = mid
        else:
            hi = mid
    return lo


def tokenize(data, rng, stats):
    """[(token, first byte, end byte)] pieces of `data` as literal runs and matches, edge matches preferred."""
    b = bytes(data)
    a = np.frombuffer(b, dtype=np.uint8)
    n = a.size
    near, far = _candidates(a)
    has = np.nonzero(near >= 0)[0].tolist()
    near, far = near.tolist(), far.tolist()
    draws = rng.random(4 * len(has) + 8).tolist()  # (four draws a candidate position, drawn at once)
    toks, i, lit_from = [], 0, 0
    for hp, h in enumerate(has):
        if h < i:
            continue
        i = h
        r0, r1, r2, r3 = draws[4 * hp:4 * hp + 4]
        cands = [near[i], far[i]]
        for d in (32768, 32767, 1):
            if i >= d and b[i:i + 3] == b[i - d:i - d + 3]:
                cands += [i - d, i - d]
        c = cands[int(r0 * len(cands))]
        dist = i - c
        if dist > 32768 or r1 < 0.05:
            continue
        length = _match_len(b, i, c, min(258, n - i))
        if length < 3:
            continue
        if r2 < 0.15 and i + length < n:
            length = 3
        elif r2 < 0.25 and i + length < n:
            length = 3 + int(r3 * (length - 2))
        via = length == 258 and r3 < 0.5
        if lit_from < i:
            toks.append((("lits", b[lit_from:i]), lit_from, i))
        toks.append((match(length, dist, via), i, i + length))
        stats["len3"] += length == 3
        stats["len258_sym285"] += length == 258 and not via
        stats["len258_sym284"] += length == 258 and via
        stats["dist1_len258"] += length == 258 and dist == 1
        stats["len_gt_dist"] += length > dist
        stats["dist32767"] += dist == 32767
        stats["dist32768"] += dist == 32768
        stats["dist_13_extra_bits"] += dist >= 24577
        stats["match_to_last_byte"] += i + length == n
        i += length
        lit_from = i
    if lit_from < n:
        toks.append((("lits", b[lit_from:]), lit_from, n))
    return toks


def _random_code(used, nsyms_max, floor, maxlen, rng, deep):
    """A random complete code over `used` plus a random set of unused symbols: (length list, its size)."""
    syms = set(used)
    universe = nsyms_max
    for _ in range(int(rng.integers(0, 6))):
        syms.add(int(rng.integers(universe)))
    while len(syms) < 2:
        syms.add(int(rng.integers(universe)))
    syms = sorted(syms)
    ls = random_complete_lens(len(syms), maxlen, rng, deep)
    rng.shuffle(ls)
    lens = [0] * max(floor, syms[-1] + 1)
    for s, l in zip(syms, ls):
        lens[s] = int(l)
    return lens


def _spell(lens, rng):
    """The code lengths as code-length symbols, every run spelled in one of its legal ways, chosen at random."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v = lens[i]
        r = 1
        while i + r < n and lens[i + r] == v:
            r += 1
        choice = rng.random()
        if v == 0 and r >= 11 and choice < 0.6:
            k = int(rng.integers(11, min(r, 138) + 1))
            out.append((18, k - 11))
        elif v == 0 and r >= 3 and choice < 0.8:
            k = int(rng.integers(3, min(r, 10) + 1))
            out.append((17, k - 3))
        elif i > 0 and lens[i - 1] == v and r >= 3 and choice < 0.8:
            k = int(rng.integers(3, min(r, 6) + 1))
            out.append((16, k - 3))
        else:
            k = 1
            out.append((v,))
        i += k
    return out


def _random_precode(cl_syms, rng):
    used = {s[0] for s in cl_syms}
    for _ in range(int(rng.integers(0, 4))):
        used.add(int(rng.integers(19)))
    while len(used) < 2:
        used.add(int(rng.integers(19)))
    used = sorted(used)
    ls = random_complete_lens(len(used), 7, rng, deep=rng.random() < 0.5)
    rng.shuffle(ls)
    pre = [0] * 19
    for s, l in zip(used, ls):
        pre[s] = int(l)
    return pre


def encode(data, rng, max_payload=None):
    """(raw DEFLATE stream, stats) for `data`: a valid stream that zlib inflates to `data`, made to look as little like
    a compressor's as it can.  stats counts what the stream holds (STAT_KEYS)."""
    data = bytes(data)
    stats = dict.fromkeys(STAT_KEYS, 0)
    pieces = tokenize(data, rng, stats)
    w = BitWriter()

    def room(after):
        """Payload bytes still free if everything from data[after:] on went into stored blocks (a BGZF member's cap)."""
        if max_payload is None:
            return 1 << 30
        rest = len(data) - after
        return max_payload - (w.bitpos // 8 + 1) - rest - 5 * (rest // 65535 + 1) - 32

    def empty_stored():
        if rng.random() < 0.3 and room(p_byte[0]) >= 5:
            stats["empty_stored"] += 1
            stats["stored_unaligned"] += (w.bitpos & 7) != 0
            stored(w, b"", False, pad=int(rng.integers(256)))

    p = 0
    p_byte = [0]  # first byte of data that no block holds yet
    while p < len(pieces):
        p_byte[0] = pieces[p][1]
        empty_stored()
        k = min(len(pieces) - p, int(rng.integers(1, 1 + max(1, min(len(pieces), int(rng.choice([3, 40, 400, 4000])))))))
        part = pieces[p:p + k]
        p += k
        first, end = part[0][1], part[-1][2]
        toks = [t for t, _, _ in part] + [("eob",)]
        kind = rng.choice(["stored", "fixed", "dynamic", "dynamic", "dynamic"])
        if kind == "stored" and end - first > 65535:
            kind = "dynamic"
        ll = dl = cl = pre = hclen = None
        if kind == "dynamic":
            used_l, used_d = {256}, set()
            for t in toks:
                if t[0] == "lits":
                    used_l.update(np.unique(np.frombuffer(t[1], dtype=np.uint8)).tolist())
                elif t[0] == "match":
                    used_l.add(t[1])
                    used_d.add(t[3])
            deep = rng.random() < 0.6
            ll = _random_code(used_l, int(rng.choice([286, 286, 287, 288])), 257, int(rng.choice([9, 12, 15, 15])), rng, deep)
            dl = _random_code(used_d, int(rng.choice([30, 30, 31, 32])), 1, int(rng.choice([5, 9, 12, 15, 15])), rng, deep)
            n15 = (sum(1 for s in used_l if ll[s] == 15), sum(1 for s in used_d if dl[s] == 15))
            # the header may announce more symbols than the last used one needs (trailing zeros: HLIT up to 288, HDIST up to 32)
            ll += [0] * int(rng.integers(0, 288 - len(ll) + 1)) if rng.random() < 0.3 else []
            dl += [0] * int(rng.integers(0, 32 - len(dl) + 1)) if rng.random() < 0.3 else []
            cl = _spell(ll + dl, rng)
            pre = _random_precode(cl, rng)
            hclen = max([4] + [i + 1 for i, s in enumerate(PRE_ORDER) if pre[s]])
            hclen = int(rng.integers(hclen, 20)) if rng.random() < 0.3 else hclen
        # under a member's cap a block must leave room for the rest; where it would not, everything left goes into one
        # stored block (which the cap always has room for)
        if max_payload is not None:
            if kind == "stored":
                cost = end - first + 6
            else:
                cl_l = np.array((ll + [0] * 288)[:288] if ll else FIXED_LITLEN)
                cl_d = dl + [0] * 32 if dl else FIXED_DIST
                bits = 80 + (sum(pre[s[0]] + (0, 2, 3, 7)[max(s[0] - 15, 0)] for s in cl) if cl else 0)
                for t in toks:
                    if t[0] == "lits":
                        bits += int(cl_l[np.frombuffer(t[1], dtype=np.uint8)].sum())
                    elif t[0] == "match":
                        bits += int(cl_l[t[1]]) + 5 + cl_d[t[3]] + 13
                cost = bits // 8 + 2
            if cost > room(end):
                part = pieces[p - k:]
                p = len(pieces)
                end = part[-1][2]
                kind = "stored"
        unaligned = (w.bitpos & 7) != 0
        stats["blocks"] += 1
        if kind == "stored":
            stats["stored_unaligned"] += unaligned
            for q in range(first, end, 65535):  # (more than one only where the cap forced the whole rest in)
                stored(w, data[q:min(q + 65535, end)], False, pad=int(rng.integers(256)))
        elif kind == "fixed":
            stats["fixed_unaligned"] += unaligned
            fixed(w, toks, False)
        else:
            stats["dynamic_unaligned"] += unaligned
            stats["litlen15_used"] += n15[0]
            stats["offset15_used"] += n15[1]
            dynamic(w, toks, False, ll, dl, hclen=hclen, pre_lens=pre, cl_syms=cl)
    p_byte[0] = len(data)
    empty_stored()
    # the final block: a zero-length stored one, or an end-of-block code alone
    if rng.random() < 0.5:
        stats["stored_unaligned"] += (w.bitpos & 7) != 0
        stored(w, b"", True, pad=int(rng.integers(256)))
    else:
        stats["fixed_unaligned"] += (w.bitpos & 7) != 0
        fixed(w, [("eob",)], True)
    # garbage behind the final block: the rest of its last byte, and sometimes bytes behind it
    w.align(int(rng.integers(256)))
    if rng.random() < 0.3:
        w.raw_bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8).tobytes())
    return w.getvalue(), stats
