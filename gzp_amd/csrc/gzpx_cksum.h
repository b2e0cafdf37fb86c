// gzpx_cksum.h -- checksums of a table of device-resident buffers (gzpx_checksum_batch_device): CRC-32, CRC-32C and
// Adler-32 of n entries of one input, tables in, sums out.  Included from gzpx_kernels.hip, namespace gzpx, behind
// gzpx_wrap.h (adler_workgroup, the status values of a report) and gzpx_wave.h (gzpx_crc.h: the CRC arithmetic; the scans).
//
// The work is cut into 64 KiB tiles counted from every entry's first byte, and the tiles of all entries form one flat
// index space, so that a table of one 2 GiB entry and a table of 30,000 small ones load the device alike:
//
//   k_cksum_plan     one workgroup: every entry against in_len, its tiles (0 for an empty or an invalid entry), and
//                    the 64-bit exclusive scan of the tiles -> prefix[n + 1]; the record's two counters are reset.
//   k_cksum_tiles    persistent workgroups; workgroup w takes the contiguous run of tiles ck_run_begin(w) ..
//                    ck_run_begin(w + 1), with the total read from prefix[n] on the device.  It finds the entry of its
//                    first tile by a 64-way search of the prefix and walks forward.  An entry that lies inside the run
//                    is stored once (part[e]); an entry that reaches across a run's edge leaves one carry per
//                    workgroup it touches: carry[2 w] where it came in over the front edge, carry[2 w + 1] where it
//                    leaves over the back edge.  Nothing is added up in memory, so there are no atomics on the sums.
//   k_cksum_finish   a lane per entry: part[e] or the fold of its carries (by the lane's wave), the seed, the comparison,
//                    the caller's tables, and the first failure / the count of failures into the record.
//   k_cksum_record   the first failing entry's status and two values into the record (kWrRec*) the host reads.
//
// What a tile gives (the linearity snap_crc32c_wave uses):
//   CRC: the shift register is linear over GF(2), so the register behind a run of tiles is the XOR of every tile's own
//   remainder times x^(8 * bytes behind the tile) mod P.  Inside a workgroup's run the register is simply carried from
//   tile to tile: the lane that owns a tile's first segment starts from the running value (for an entry's first tile:
//   the seed XOR all ones), the other lanes from zero, and a lane's register times x^(8 * bytes behind its segment in
//   the tile) XORs into the next running value.  Only where a run ends inside an entry is the value moved to the
//   entry's end, by x^(8 * bytes behind) -- once per workgroup at most.  The finish is the XOR of the terms and the
//   xor-out.
//   Adler-32: a tile gives (s1, s2) as adler_workgroup defines them; behind L more bytes the pair (A, B) has become
//   (A, B + L A), so terms add mod 65521 in any order, and the seed (a0, b0) comes in at the end as a0 + A,
//   b0 + n a0 + B.
#pragma once

constexpr uint32_t kCkCrc32 = 0, kCkAdler32 = 1, kCkCrc32c = 2;  // GZPX_CHECK_*
constexpr uint32_t kCkTile = 65536u;    // bytes per tile
constexpr uint32_t kCkThreads = 256u;   // a lane owns one 256-byte segment of a tile
constexpr uint32_t kCkSeg = kCkTile / kCkThreads;
constexpr uint32_t kCkWgPerCu = 6u;     // the persistent launch: workgroups per compute unit (77 VGPRs: six waves a SIMD)
constexpr uint32_t kCkPlanThreads = 1024u;
static_assert(kCkThreads == kAdlerThreads, "k_cksum_tiles calls adler_workgroup");

// ------------------------------------------------------------------------------------------
// the table
// ------------------------------------------------------------------------------------------
struct CkTable {
    const uint8_t *in;     // the input, in_len bytes: no byte of an entry that leaves it is read
    uint64_t in_len;
    const uint64_t *off;   // [n], or [n + 1] in the span form
    const uint32_t *size;  // [n], or null: entry i is [off[i], off[i + 1])
    uint32_t n;
};

// Entry i: where it starts, how long it is, and whether it lies inside the input (len = 0 if not).
__device__ __forceinline__ bool ck_entry(const CkTable &t, uint32_t i, uint64_t &off, uint64_t &len) {
    off = t.off[i];
    if (t.size) {
        len = t.size[i];
        if (off <= t.in_len && len <= t.in_len - off) return true;
    } else {
        const uint64_t end = t.off[i + 1];
        len = end - off;
        if (end >= off && end <= t.in_len) return true;
    }
    len = 0;
    return false;
}

__device__ __forceinline__ uint64_t ck_tiles(uint64_t len) { return (len >> 16) + ((len & 0xFFFFu) ? 1u : 0u); }

// The run of workgroup w out of g over `total` tiles: total / g tiles each, the first total % g workgroups one more.
__device__ __forceinline__ uint64_t ck_run_begin(uint64_t w, uint64_t total, uint64_t g) {
    const uint64_t q = total / g, r = total % g;
    return w * q + (w < r ? w : r);
}
// ... and the workgroup whose run holds tile t
__device__ __forceinline__ uint64_t ck_run_of(uint64_t t, uint64_t total, uint64_t g) {
    const uint64_t q = total / g, r = total % g;
    const uint64_t edge = r * (q + 1u);  // the first tile of the workgroups that take q
    return t < edge ? t / (q + 1u) : r + (t - edge) / q;
}

// The entry that holds tile t: the largest e in [lo, n) with prefix[e] <= t (prefix[lo] <= t < prefix[n]); an entry
// without tiles shares its prefix with its successor, so it is never the answer.  Every lane of a wave calls it with
// the same arguments and gets the same answer: 64 probes a round.
__device__ __forceinline__ uint32_t ck_find(const uint64_t *__restrict__ prefix, uint64_t lo, uint64_t n, uint64_t t) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t hi = n;
    while (hi - lo > 1u) {
        const uint64_t step = (hi - lo + 63u) >> 6;
        const uint64_t idx = lo + lane * step;
        const bool ok = idx < hi && prefix[idx] <= t;
        const uint32_t cnt = (uint32_t)__popcll(__ballot(ok));  // (the predicate is monotone; lane 0 holds)
        lo += (uint64_t)(cnt ? cnt - 1u : 0u) * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    return (uint32_t)lo;
}

// ------------------------------------------------------------------------------------------
// k_cksum_plan: k_scan's shape -- every lane owns a run of consecutive entries, two passes over them around one
// workgroup scan.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCkPlanThreads) void k_cksum_plan(CkTable t, uint64_t *__restrict__ prefix,
                                                              uint32_t *__restrict__ rec) {
    __shared__ uint64_t wsum[kCkPlanThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t per = ((uint64_t)t.n + kCkPlanThreads - 1) / kCkPlanThreads;
    const uint64_t i0 = tid * per < t.n ? tid * per : t.n, i1 = i0 + per < t.n ? i0 + per : t.n;
    uint64_t mine = 0;
    for (uint64_t i = i0; i < i1; i++) {
        uint64_t off, len;
        (void)ck_entry(t, (uint32_t)i, off, len);
        mine += ck_tiles(len);
    }
    uint64_t inc = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t v = __shfl_up(inc, d);
        if (lane >= (unsigned)d) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint64_t run = 0, total = 0;
    for (uint32_t w = 0; w < kCkPlanThreads / 64; w++) {
        const uint64_t v = wsum[w];
        if (w < wave) run += v;
        total += v;
    }
    run += inc - mine;
    for (uint64_t i = i0; i < i1; i++) {
        uint64_t off, len;
        (void)ck_entry(t, (uint32_t)i, off, len);
        prefix[i] = run;
        run += ck_tiles(len);
    }
    if (tid == 0) {
        prefix[t.n] = total;
        rec[kWrRecFirst] = 0xFFFFFFFFu;
        rec[kWrRecFailed] = 0;
    }
}

// ------------------------------------------------------------------------------------------
// One tile of a CRC.  crc32_direct's shape: lane t owns the 256-byte segment that ENDS 256 (255 - t) bytes in front of
// the tile's end, so only the first used segment is short; a whole segment is crc_seg256, a short one crc_bytes
// (gzpx_crc.h).  The registers are plain remainders -- no inversion in here -- and the lane whose segment starts the
// tile starts from `init`.  Returns the register behind the tile's last byte, in every lane.
// Reads: the dwords that hold bytes of p[0, len), and nothing else; `at_end` (the tile ends its entry) keeps the last
// segment's look-ahead load in front of the tile's end where the end is dword-aligned.
// ------------------------------------------------------------------------------------------
struct CkCrcLds {
    uint32_t table[4][256];
    uint32_t segpow[kCkThreads];  // x^(8 * 256 * (255 - t)): moves lane t's register to the tile's end
    uint32_t sq[64];
    uint32_t red[2][kCkThreads / 64];
};

template <uint32_t P>
__device__ __forceinline__ void ck_crc_setup(CkCrcLds &l, const CrcPow &pw, uint32_t tid) {
    if (tid < 64) l.sq[tid] = pw.sq[tid];
    crc_tables_fill<P>(l.table, tid, kCkThreads);  // (its barrier is the one behind sq[] too)
    l.segpow[tid] = crc_xpow8<P>(l.sq, (uint64_t)kCkSeg * (kCkThreads - 1u - tid));
    __syncthreads();
}

template <uint32_t P>
__device__ __forceinline__ uint32_t ck_crc_tile(CkCrcLds &l, const uint8_t *__restrict__ p, uint32_t len, uint32_t init,
                                                bool at_end, uint32_t tid, uint32_t parity) {
    const int32_t seg_end_i = (int32_t)len - (int32_t)kCkSeg * (int32_t)(kCkThreads - 1u - tid);
    uint32_t c = 0;
    if (seg_end_i > 0) {
        const uint32_t sb = seg_end_i > (int32_t)kCkSeg ? (uint32_t)seg_end_i - kCkSeg : 0u;
        const uint32_t n = (uint32_t)seg_end_i - sb;
        const uint8_t *s = p + sb;
        if (sb == 0) c = init;
        if (n == kCkSeg) c = crc_seg256(l.table, s, at_end && (uint32_t)seg_end_i == len, c);
        else c = crc_bytes(l.table, s, n, c);  // the short first segment of the tile
        c = crc_mulmod<P>(c, l.segpow[tid]);
    }
    for (int m = 32; m >= 1; m >>= 1) c ^= __shfl_xor(c, m);
    // (red[] alternates from tile to tile: a wave that is a tile ahead writes the other half, and it cannot be two
    // ahead without every wave having passed the barrier between)
    if ((tid & 63u) == 0) l.red[parity][tid >> 6] = c;
    __syncthreads();
    return l.red[parity][0] ^ l.red[parity][1] ^ l.red[parity][2] ^ l.red[parity][3];
}

// ------------------------------------------------------------------------------------------
// k_cksum_tiles
// ------------------------------------------------------------------------------------------
template <uint32_t KIND>
__global__ __launch_bounds__(kCkThreads) void k_cksum_tiles(CkTable t, const uint32_t *__restrict__ seeds,
                                                           const uint64_t *__restrict__ prefix, uint32_t *__restrict__ part,
                                                           uint32_t *__restrict__ carry, CrcPow pw) {
    constexpr bool kAdler = KIND == kCkAdler32;
    constexpr uint32_t P = KIND == kCkCrc32c ? kCrcPoly32c : kCrcPoly32;
    __shared__ typename std::conditional<kAdler, AdlerLds, CkCrcLds>::type l;
    const uint32_t tid = threadIdx.x;
    const uint64_t total = prefix[t.n], g = gridDim.x, w = blockIdx.x;
    const uint64_t t0 = ck_run_begin(w, total, g), t1 = ck_run_begin(w + 1u, total, g);
    if (t0 == t1) return;
    if constexpr (!kAdler) ck_crc_setup<P>(l, pw, tid);
    uint32_t e = ck_find(prefix, 0, t.n, t0);
    uint64_t pe = prefix[e], pn = prefix[e + 1u];
    uint32_t parity = 0;
    for (uint64_t tile = t0; tile < t1;) {
        uint64_t off, len;
        (void)ck_entry(t, e, off, len);  // (an entry with tiles is a valid one)
        const uint64_t stop = pn < t1 ? pn : t1;  // the entry's tiles in this run: [tile, stop)
        if (stop <= tile) break;                  // (never with a prefix k_cksum_plan made: the walk must not stall)
        const uint8_t *base = t.in + off;
        uint32_t a = 0, b = 0;  // CRC: the register in `a`.  Adler-32: (A, B) behind the last tile taken
        if constexpr (!kAdler)
            if (tile == pe) a = ~(seeds ? seeds[e] : 0u);
        for (; tile < stop; tile++) {
            const uint64_t pos = (tile - pe) << 16;
            const uint32_t n = len - pos < kCkTile ? (uint32_t)(len - pos) : kCkTile;
            if constexpr (kAdler) {
                uint32_t s1, s2;
                adler_workgroup(l, base + pos, n, tid, s1, s2);
                b = (uint32_t)((b + (uint64_t)n * a + s2) % kAdlerBase);
                a = (a + s1) % kAdlerBase;
            } else {
                a = ck_crc_tile<P>(l, base + pos, n, a, pos + n == len, tid, parity);
                parity ^= 1u;
            }
        }
        const uint64_t done = (stop - pe) << 16;  // bytes of the entry in front of the run's end
        if (done < len) {  // the run ends inside the entry: the value moves to the entry's end
            const uint64_t behind = len - done;
            if constexpr (kAdler) b = (uint32_t)((b + (behind % kAdlerBase) * a) % kAdlerBase);
            else a = crc_mulmod<P>(a, crc_xpow8<P>(l.sq, behind));
        }
        if (tid == 0) {
            const uint32_t v = kAdler ? (a | (b << 16)) : a;
            if (pe >= t0 && pn <= t1) part[e] = v;
            else carry[2u * w + (pe < t0 ? 0u : 1u)] = v;
        }
        if (tile < t1) {  // the next entry with tiles: nearly always the next entry
            e++;
            pe = pn;
            pn = prefix[e + 1u];
            if (pn == pe) {
                e = ck_find(prefix, e, t.n, tile);
                pn = prefix[e + 1u];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_cksum_finish, k_cksum_record
// ------------------------------------------------------------------------------------------
struct CkOut {
    const uint32_t *seeds;     // [n] or null
    const uint32_t *expected;  // [n] or null
    uint32_t *sums;            // [n] or null
    WrapResult *results;       // [n] or null
};

__global__ __launch_bounds__(256) void k_cksum_finish(uint32_t kind, CkTable t, CkOut o, const uint64_t *__restrict__ prefix,
                                                      uint32_t *__restrict__ part, const uint32_t *__restrict__ carry,
                                                      uint32_t g, uint32_t *__restrict__ rec) {
    __shared__ uint32_t first, failed;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        first = 0xFFFFFFFFu;
        failed = 0;
    }
    __syncthreads();
    const uint32_t lane = tid & 63u;
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + tid;
    const uint32_t i = (uint32_t)i64;
    const bool adler = kind == kCkAdler32;
    uint64_t off = 0, len = 0, w0 = 0, w1 = 0;
    bool valid = false, spans = false;
    uint32_t x = 0;         // CRC: the XOR of the entry's terms
    uint64_t a = 0, b = 0;  // Adler-32: their sums
    if (i64 < t.n) {
        valid = ck_entry(t, i, off, len);
        if (valid && len) {
            const uint64_t pe = prefix[i], pn = prefix[i + 1u], total = prefix[t.n];
            w0 = ck_run_of(pe, total, g);
            w1 = ck_run_of(pn - 1u, total, g);
            spans = w0 != w1;
            if (!spans) {
                x = part[i];
                a = x & 0xFFFFu;
                b = x >> 16;
            }
        }
    }
    // An entry that reaches across workgroups has one carry in each of them -- thousands for one long entry: the wave
    // folds them together, 64 carries a round, one such entry after the other.
    for (uint64_t todo = __ballot(spans); todo; todo &= todo - 1u) {
        const int src = __ffsll((long long)todo) - 1;
        const uint64_t s0 = __shfl(w0, src), s1 = __shfl(w1, src);
        uint32_t fx = 0;
        uint64_t fa = 0, fb = 0;
#pragma unroll 4
        for (uint64_t w = s0 + lane; w <= s1; w += 64u) {
            const uint32_t v = carry[2u * w + (w == s0 ? 1u : 0u)];
            fx ^= v;
            fa += v & 0xFFFFu;
            fb += v >> 16;
        }
        for (int m = 32; m >= 1; m >>= 1) {
            fx ^= __shfl_xor(fx, m);
            fa += __shfl_xor(fa, m);
            fb += __shfl_xor(fb, m);
        }
        if ((int)lane == src) {
            x = fx;
            a = fa;
            b = fb;
        }
    }
    if (i64 < t.n) {
        const uint32_t seed = o.seeds ? o.seeds[i] : (adler ? 1u : 0u);
        const uint32_t want = o.expected ? o.expected[i] : 0u;
        uint32_t sum = 0;
        if (valid && len == 0) {
            sum = seed;
        } else if (valid && adler) {
            const uint32_t a0 = seed & 0xFFFFu, b0 = seed >> 16;
            const uint32_t ra = (uint32_t)((a0 + a) % kAdlerBase);
            const uint32_t rb = (uint32_t)((b0 + (len % kAdlerBase) * a0 + b) % kAdlerBase);
            sum = ra | (rb << 16);
        } else if (valid) {
            sum = ~x;
        }
        const uint32_t status = !valid ? kWrInvalidArg : (o.expected && sum != want) ? kWrInvalidCheck : kWrOk;
        part[i] = sum;  // (k_cksum_record reads the first failing entry's here: the caller's tables are optional)
        if (o.sums) o.sums[i] = sum;
        if (o.results) o.results[i] = WrapResult{status, len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len, sum, want};
        if (status != kWrOk) {
            atomicMin(&first, i);
            atomicAdd(&failed, 1u);
        }
    }
    __syncthreads();
    if (tid == 0 && failed) {
        atomicMin(&rec[kWrRecFirst], first);
        atomicAdd(&rec[kWrRecFailed], failed);
    }
}

__global__ __launch_bounds__(64) void k_cksum_record(CkTable t, const uint32_t *__restrict__ expected,
                                                     const uint32_t *__restrict__ part, uint32_t *__restrict__ rec) {
    if (threadIdx.x != 0) return;
    const uint32_t i = rec[kWrRecFirst];
    uint32_t status = kWrOk, found = 0, want = 0;
    if (i != 0xFFFFFFFFu) {
        uint64_t off, len;
        status = ck_entry(t, i, off, len) ? kWrInvalidCheck : kWrInvalidArg;
        found = part[i];
        want = expected ? expected[i] : 0u;
    }
    rec[kWrRecStatus] = status;
    rec[kWrRecFound] = found;
    rec[kWrRecExpected] = want;
    rec[5] = 0;
    rec[kWrRecTotal] = 0;
    rec[kWrRecTotal + 1] = 0;
}
