// gzpx_lines.h -- reads by LINE of a BGZF / Mgzip stream in device memory: a table that says how many delimiter bytes
// every tile of kLnTile bytes of the INFLATED stream holds, and a search that turns line numbers into byte positions by
// inflating only the members that hold the boundaries' tiles.  Included from gzpx_kernels.hip behind gzpx_ranges.h,
// whose locate, select and gather run unchanged on the byte ranges made here.  (Definitions: include/gzpx.h.)
//
//   build   k_ln_count behind every batch of the inflate, one workgroup per (tile ∩ batch): the bytes of staging are
//           read once as aligned 16-byte words, four or five in flight per lane; per dword an exact equal-byte test and a
//           popcount, the bytes outside the tile at the two ragged ends masked; wave reduction, LDS, one atomic per
//           workgroup into the tile's counter (a tile that two batches share gets both parts; the batches are ordered
//           on one stream).  k_ln_prefix, one workgroup: counters -> P[tiles + 1] (u64), D, L, last-byte flag.
//   search  k_ln_tiles, one lane per boundary (or per line range: two boundaries): validation, the boundary's tile by
//           binary search in P (log2 loads), and the COVER -- the byte range of the inflated stream that has to be
//           there to place the boundaries -- written where k_rr_locate reads its ranges.  launch_ranges_select and
//           launch_inflate then run as for a read by byte range.
//           k_ln_find, one wave per boundary: its tile is walked in staging 1 KiB a step (64 lanes x 16 bytes): per
//           lane count, wave prefix, the lane that holds the k-th delimiter, the byte inside its word.  At most 17
//           steps whatever the size of the members (an Mgzip member may be 64 MiB: hence a table per tile).
//           k_ln_offsets, one workgroup: byte positions -> lengths -> out_offsets, and where every range starts in
//           staging, in the form k_rr_gather takes.
// No kernel's depth of dependent global loads grows with the number of members, ranges or lines.

constexpr uint32_t kLnNone = 0xFFFFFFFFu;  // a boundary that has no tile to walk
constexpr uint32_t kLnThreads = 256;
constexpr uint32_t kLnItems = 5;  // 16-byte words per lane of k_ln_count: 1024 in a tile, one more when it starts inside a word
constexpr uint32_t kLnScanItems = 4;  // tiles per thread and step of k_ln_prefix
static_assert(kLnItems * kLnThreads * 16u >= kLnTile + 16u, "a tile and a ragged word fit one pass");

// 0x80 in every byte of w that equals the splat's byte.  Exact for every delimiter, 0x00, 0x7F, 0x80 and 0xFF among
// them: the addition works on seven bits a byte, so no carry crosses into the next byte.
__device__ __forceinline__ uint32_t ln_marks(uint32_t w, uint32_t splat) {
    const uint32_t x = w ^ splat;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// the 0x80 bits of those bytes of the dword at address p that lie in [a0, a1)
__device__ __forceinline__ uint32_t ln_inside(uintptr_t p, uintptr_t a0, uintptr_t a1) {
    const uint32_t lo = p >= a0 ? 0u : (a0 - p >= 4u ? 4u : (uint32_t)(a0 - p));
    const uint32_t hi = p >= a1 ? 0u : (a1 - p >= 4u ? 4u : (uint32_t)(a1 - p));
    if (lo >= hi) return 0u;
    uint32_t m = 0x80808080u << (8u * lo);  // (lo < hi <= 4: a shift of 24 bits at most)
    if (hi < 4u) m &= (1u << (8u * hi)) - 1u;
    return m;
}

// the marks of the aligned word v read at address p, bytes outside [a0, a1) left out
__device__ __forceinline__ void ln_word(const uint4 &v, uint32_t splat, uintptr_t p, uintptr_t a0, uintptr_t a1,
                                        uint32_t (&m)[4]) {
    m[0] = ln_marks(v.x, splat);
    m[1] = ln_marks(v.y, splat);
    m[2] = ln_marks(v.z, splat);
    m[3] = ln_marks(v.w, splat);
    if (p < a0 || p + 16u > a1) {  // a ragged end: two words of a tile at most
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) m[q] &= ln_inside(p + 4u * q, a0, a1);
    }
}

// Staging holds the inflated bytes [base, base + len) of the stream (16 readable bytes behind them); workgroup x counts
// the delimiters of tile base / kLnTile + x inside it.  The one that sees the stream's last byte notes whether that is
// a delimiter.
__global__ __launch_bounds__(kLnThreads) void k_ln_count(const uint8_t *__restrict__ stage, uint64_t base, uint64_t len,
                                                         uint64_t total, uint32_t delim, uint32_t *cnt, uint32_t *rec) {
    __shared__ uint32_t wsum[kLnThreads / 64u];
    const uint32_t tid = threadIdx.x;
    const uint64_t t = base / kLnTile + blockIdx.x;
    uint64_t b = t * kLnTile, e = b + kLnTile;
    if (b < base) b = base;
    if (e > base + len) e = base + len;  // (b < e: the grid ends with the batch)
    const uintptr_t a0 = (uintptr_t)stage + (b - base), a1 = (uintptr_t)stage + (e - base);
    const uintptr_t w0 = a0 & ~(uintptr_t)15;
    const uint32_t n_words = (uint32_t)((a1 - w0 + 15u) / 16u);
    const uint32_t splat = delim * 0x01010101u;
    uint4 v[kLnItems];
#pragma unroll
    for (uint32_t u = 0; u < kLnItems; u++) {  // aligned words of staging, several loads in flight per lane
        const uint32_t k = u * kLnThreads + tid;
        v[u] = make_uint4(0, 0, 0, 0);
        if (k < n_words) v[u] = *(const uint4 *)(w0 + 16u * (uintptr_t)k);
    }
    uint32_t c = 0;
#pragma unroll
    for (uint32_t u = 0; u < kLnItems; u++) {
        const uint32_t k = u * kLnThreads + tid;
        if (k >= n_words) continue;
        uint32_t m[4];
        ln_word(v[u], splat, w0 + 16u * (uintptr_t)k, a0, a1, m);
        c += (uint32_t)(__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]));
    }
    c = wave_reduce_add(c);
    if ((tid & 63u) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0;
        for (uint32_t w = 0; w < kLnThreads / 64u; w++) s += wsum[w];
        if (s) atomicAdd(&cnt[t], s);
        if (e == total) rec[kLnRecLast] = stage[e - 1u - base] == (uint8_t)delim ? 1u : 0u;
    }
}

// One workgroup: P[t] = delimiters in tiles 0..t-1, P[tiles] = D; the record gets D, L and keeps the last-byte flag.
__global__ __launch_bounds__(kLnThreads) void k_ln_prefix(const uint32_t *__restrict__ cnt, uint32_t tiles, uint64_t total,
                                                          uint64_t *__restrict__ P, uint32_t *rec) {
    __shared__ uint64_t wsum[4];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0;  // every thread keeps its own copy (the scan returns the total)
    for (uint64_t base = 0; base < tiles; base += kLnThreads * kLnScanItems) {
        const uint64_t i0 = base + (uint64_t)tid * kLnScanItems;
        uint32_t c[kLnScanItems];
        uint64_t sum = 0, step;
#pragma unroll
        for (uint32_t j = 0; j < kLnScanItems; j++) {
            c[j] = i0 + j < tiles ? cnt[i0 + j] : 0u;
            sum += c[j];
        }
        uint64_t ex = carry + block_exclusive_scan256(sum, wsum, &step);
        carry += step;
#pragma unroll
        for (uint32_t j = 0; j < kLnScanItems; j++) {
            if (i0 + j < tiles) P[i0 + j] = ex;
            ex += c[j];
        }
    }
    if (tid == 0) {
        P[tiles] = carry;
        const uint32_t last = total ? rec[kLnRecLast] : 0u;
        const uint64_t lines = carry + (total && !last ? 1u : 0u);  // an unterminated last line counts
        rec[kLnRecLast] = last;
        rec[kLnRecD] = (uint32_t)carry;
        rec[kLnRecD + 1] = (uint32_t)(carry >> 32);
        rec[kLnRecL] = (uint32_t)lines;
        rec[kLnRecL + 1] = (uint32_t)(lines >> 32);
    }
}

// the tile of boundary k, 1 <= k <= D: the t with P[t] < k <= P[t + 1]  (P[tiles] = D >= k: there is one)
__device__ __forceinline__ uint32_t ln_tile_of(const LnTable &tb, uint64_t k) { return rr_bound<false>(tb.P + 1, 0, tb.tiles, k); }

__device__ __forceinline__ uint64_t ln_tile_end(const LnTable &tb, uint32_t t) {
    const uint64_t e = ((uint64_t)t + 1u) * kLnTile;
    return e < tb.total ? e : tb.total;
}

// per == 1: item r is the boundary bounds[r]; its cover is its tile.  per == 2: item r is the line range
// [bounds[2 r], bounds[2 r + 1]); its cover reaches from the tile of the first boundary to the tile of the second.  A
// boundary that needs no walk (0, above D, or of an empty range) gets kLnNone and its answer at once.  Invalid items
// get an empty cover, and the first of them is reduced with atomicMin.
__global__ __launch_bounds__(kLnThreads) void k_ln_tiles(LnTable tb, uint32_t n, uint32_t per, const uint64_t *__restrict__ bounds,
                                                         uint64_t *__restrict__ covers, uint32_t *__restrict__ btile,
                                                         uint64_t *__restrict__ bpos, uint32_t *rec) {
    const uint32_t r = blockIdx.x * kLnThreads + threadIdx.x;
    if (r >= n) return;
    uint64_t cb = 0, ce = 0;
    if (per == 1u) {
        const uint64_t k = bounds[r];
        uint32_t t = kLnNone;
        uint64_t pos = 0;
        if (k > tb.L) {
            atomicMin(&rec[kLnRecBad], r);
        } else if (k > tb.D) {
            pos = tb.total;
        } else if (k) {
            t = ln_tile_of(tb, k);
            cb = (uint64_t)t * kLnTile;
            ce = ln_tile_end(tb, t);
        }
        btile[r] = t;
        bpos[r] = pos;
    } else {
        const uint64_t a = bounds[2 * (uint64_t)r], b = bounds[2 * (uint64_t)r + 1];
        uint32_t ta = kLnNone, te = kLnNone;
        uint64_t pe = 0;
        if (a > b || b > tb.L) {
            atomicMin(&rec[kLnRecBad], r);
        } else if (a < b) {  // (a < L <= D + 1: a is 0 or has a tile.  An empty range reads nothing and is reported as {0, 0}.)
            if (a) {
                ta = ln_tile_of(tb, a);
                cb = (uint64_t)ta * kLnTile;
            }
            if (b > tb.D) {
                pe = ce = tb.total;
            } else {
                te = ln_tile_of(tb, b);
                ce = ln_tile_end(tb, te);
            }
        }
        btile[2 * (uint64_t)r] = ta;
        btile[2 * (uint64_t)r + 1] = te;
        bpos[2 * (uint64_t)r] = 0;
        bpos[2 * (uint64_t)r + 1] = pe;
    }
    covers[2 * (uint64_t)r] = cb;
    covers[2 * (uint64_t)r + 1] = ce;
}

// One wave per boundary i (item i / per).  src[item] is where the item's cover starts in staging (k_rr_select).  A
// boundary whose delimiter is not found -- the stream is not the one the table was built from -- gets its tile's end:
// every answer lies inside the boundary's tile, so nothing behind this kernel leaves the cover.
__global__ __launch_bounds__(kLnThreads) void k_ln_find(LnTable tb, uint32_t n_bounds, uint32_t per, uint32_t delim,
                                                        const uint64_t *__restrict__ bounds, const uint64_t *__restrict__ covers,
                                                        const uint64_t *__restrict__ src, const uint8_t *__restrict__ stage,
                                                        const uint32_t *__restrict__ btile, uint64_t *__restrict__ bpos) {
    const uint32_t i = blockIdx.x * (kLnThreads / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= n_bounds) return;  // (a whole wave)
    const uint32_t t = btile[i];
    if (t == kLnNone) return;
    const uint32_t item = i / per;
    const uint64_t need = bounds[i] - tb.P[t];  // the delimiter's rank inside the tile, from 1
    const uint64_t t_begin = (uint64_t)t * kLnTile, t_end = ln_tile_end(tb, t);
    const uintptr_t a0 = (uintptr_t)stage + src[item] + (t_begin - covers[2 * (uint64_t)item]), a1 = a0 + (t_end - t_begin);
    const uint32_t splat = delim * 0x01010101u;
    uint64_t seen = 0;
    for (uintptr_t row = a0 & ~(uintptr_t)15; row < a1; row += 1024u) {  // (the same in every lane)
        const uintptr_t p = row + 16u * lane;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p < a1) v = *(const uint4 *)p;
        uint32_t m[4];
        ln_word(v, splat, p, a0, a1, m);
        const uint32_t c = (uint32_t)(__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]));
        const uint32_t inc = wave_incl_add(c);
        const uint32_t step = rdlane(inc, 63);
        if (seen + step < need) {
            seen += step;
            continue;
        }
        const uint64_t want = need - seen;  // its rank in this step
        if (inc >= want && inc - c < want) {  // the one lane that holds it
            uint32_t j = (uint32_t)(want - (inc - c));
            uint32_t q = 0;
            while (j > (uint32_t)__popc(m[q])) j -= (uint32_t)__popc(m[q++]);  // (j <= c: q stays below 4)
            uint32_t mm = m[q];
            while (--j) mm &= mm - 1u;
            const uint32_t byte = 4u * q + ((uint32_t)__ffs((int)mm) - 1u) / 8u;
            bpos[i] = t_begin + (uint64_t)(p + byte - a0) + 1u;
        }
        return;
    }
    if (lane == 0) bpos[i] = t_end;
}

// One workgroup.  bpos holds (begin, end) of every range in bytes of the inflated stream; src[r] comes in as where the
// range's cover starts in staging and leaves as where its bytes start.
__global__ __launch_bounds__(kLnThreads) void k_ln_offsets(uint32_t n_ranges, const uint64_t *__restrict__ covers,
                                                           const uint64_t *__restrict__ bpos, uint64_t *__restrict__ src,
                                                           uint64_t *__restrict__ out_off, uint32_t *rec) {
    __shared__ uint64_t wsum[4];
    const uint32_t tid = threadIdx.x;
    uint64_t c_out = 0;
    for (uint64_t base = 0; base < n_ranges; base += kLnThreads) {
        const uint64_t r = base + tid;
        uint64_t begin = 0, end = 0;
        if (r < n_ranges) {
            begin = bpos[2 * r];
            end = bpos[2 * r + 1];
        }
        const uint64_t length = end > begin ? end - begin : 0u;
        uint64_t step;
        const uint64_t ex = c_out + block_exclusive_scan256(length, wsum, &step);
        c_out += step;
        if (r < n_ranges) {
            out_off[r] = ex;
            if (length) src[r] += begin - covers[2 * r];  // (the cover starts at or in front of the range)
        }
    }
    if (tid == 0) {
        out_off[n_ranges] = c_out;
        rec[kLnRecTotal] = (uint32_t)c_out;
        rec[kLnRecTotal + 1] = (uint32_t)(c_out >> 32);
    }
}
