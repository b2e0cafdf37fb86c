// gzpx_fields.h -- WHICH FIELDS of the lines of a BGZF / Mgzip stream in device memory: cut -f with -d on the line
// ranges that a line search has left in staging.  The output is the input with some bytes removed, in the same order:
// a stream compaction whose predicate depends on the byte and on how many field delimiters precede it in its line.
// Included from gzpx_kernels.hip behind gzpx_select.h; the marks are ln_word / fd_mask16 (gzpx_lines.h, gzpx_find.h),
// the searches rr_bound (gzpx_ranges.h).  (Definitions: include/gzpx.h.)
//
// Range r of the search lies at src[r] of staging, in_off[r + 1] - in_off[r] bytes long, and starts at a line start.  Its
// bytes are cut on the 16 KiB grid of staging into PIECES; the pieces of all ranges are numbered in one row, pfirst[r]
// the first of range r, and piece x finds its range by binary search.  The host launches fields_pieces() workgroups, a
// bound it knows without a round trip; those at and behind pfirst[n] leave at once.
//
//   k_fl_plan        one workgroup: the pieces of every range -> pfirst, by a scan.
//   k_fl_carry       one workgroup per piece: whether it holds a line delimiter, and the field delimiters behind its last
//                    one (in the whole piece if it holds none).
//   k_fl_carry_scan  one workgroup: a segmented scan of these over the pieces, restarted at every range's first piece ->
//                    cin[x], the field number of piece x's first byte.  A line many pieces long carries its count through
//                    pieces that hold no line delimiter at all; the sums are 64-bit.
//   k_fl_count       one workgroup per piece: the walk (below), the kept bytes counted.
//   k_fl_scan        one workgroup: the counts -> obase[x], where piece x's bytes go; out_offsets[r] = obase[pfirst[r]];
//                    the record.
//   k_fl_write       the walk again; a lane's kept bytes go to LDS at their rank in the piece, shifted by the output
//                    address's offset in its 16-byte word, and the workgroup stores LDS as aligned 16-byte words, bytes
//                    only in the two words that the piece shares with its neighbours.  Nothing is stored when the total
//                    exceeds out_cap.
// THE WALK.  256 lanes x one aligned 16-byte word a row, so lane order is byte order; the four rows of a piece are loaded
// together.  A lane's word is the pair (it holds a line delimiter, the field delimiters behind its last one), packed as
// bit 31 and a count below it; fl_join is the operator of the segmented sum, in which a line delimiter resets the count,
// and fl_scan its exclusive prefix over the rows, waves and lanes of the workgroup.  The prefix and cin give the field
// number k of the word's first byte, as a 64-bit value: nothing saturates.  fl_keep looks k up in the compiled list in LDS
// once (binary search over the changes in use), then advances at every field delimiter with a countdown to the next
// change, and returns the 16-bit mask of the bytes kept.
// No atomics: every placement comes from a scan, so the output is the same bit for bit from run to run.  No kernel reads
// further than the 16 bytes behind staging that the gather relies on.

constexpr uint32_t kFlThreads = 256;
constexpr uint32_t kFlItems = kFlPiece / (16u * kFlThreads);  // rows of a piece
constexpr uint32_t kFlScanItems = 16;                          // pieces per thread and step of the two scans
constexpr uint32_t kFlReset = 0x80000000u, kFlHead = 0x40000000u;
constexpr uint64_t kFlReset64 = 1ull << 63;
static_assert(kFlItems * kFlThreads * 16u == kFlPiece && kFlThreads == 256u, "a piece is a whole number of rows of four waves");

// what the kernels share of a call
struct FlArgs {
    const uint8_t *stage;
    const uint64_t *src;     // [n] where a range's bytes start in staging
    const uint64_t *in_off;  // [n + 1] the exclusive scan of the ranges' lengths
    const uint64_t *pfirst;  // [n + 1]
    uint32_t n;
    uint32_t delim, fdelim;
};

// the segmented sum: b behind a
__device__ __forceinline__ uint32_t fl_join(uint32_t a, uint32_t b) { return (b & kFlReset) ? b : a + b; }
__device__ __forceinline__ uint64_t fl_join64(uint64_t a, uint64_t b) { return (b & kFlReset64) ? b : a + b; }

// the pair of one word: fm its field delimiters, dm its line delimiters, a bit a byte
__device__ __forceinline__ uint32_t fl_elem(uint32_t fm, uint32_t dm) {
    if (!dm) return (uint32_t)__popc(fm);
    const uint32_t top = 31u - (uint32_t)__clz((int)dm);
    return kFlReset | (uint32_t)__popc(fm >> (top + 1u));
}

// Exclusive prefix of N values per thread under fl_join, in the order (row, wave, lane); *total: all of them joined.
// `wsum` is 4 N words of LDS.  Two barriers.  (Values without bit 31 are summed plainly.)
template <uint32_t N>
__device__ __forceinline__ void fl_scan(const uint32_t (&e)[N], uint32_t *wsum, uint32_t (&ex)[N], uint32_t *total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc[N], prev[N];
#pragma unroll
    for (uint32_t u = 0; u < N; u++) {
        inc[u] = e[u];
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t t = __shfl_up(inc[u], d);
            if (lane >= d) inc[u] = fl_join(t, inc[u]);
        }
        prev[u] = __shfl_up(inc[u], 1);
    }
    __syncthreads();  // protect wsum from the previous use
    if (lane == 63u) {
#pragma unroll
        for (uint32_t u = 0; u < N; u++) wsum[4u * u + wave] = inc[u];
    }
    __syncthreads();
    uint32_t run = 0;
#pragma unroll
    for (uint32_t u = 0; u < N; u++) {
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) {
            if (w == wave) ex[u] = lane ? fl_join(run, prev[u]) : run;
            run = fl_join(run, wsum[4u * u + w]);
        }
    }
    *total = run;
}

// the same for one 64-bit value per thread (bit 63 resets); `wsum` is 4 words of LDS
__device__ __forceinline__ uint64_t fl_scan64(uint64_t v, uint64_t *wsum, uint64_t *total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc = v;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t t = __shfl_up(inc, d);
        if (lane >= d) inc = fl_join64(t, inc);
    }
    const uint64_t prev = __shfl_up(inc, 1);
    __syncthreads();  // protect wsum from the previous use
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    uint64_t run = 0, ex = 0;
    for (uint32_t w = 0; w < 4u; w++) {
        if (w == wave) ex = lane ? fl_join64(run, prev) : run;
        run = fl_join64(run, wsum[w]);
    }
    *total = run;
    return ex;
}

// the pieces of a range of len > 0 bytes at s of staging
__device__ __forceinline__ uint64_t fl_pieces(uint64_t s, uint64_t len) { return (s + len - 1u) / kFlPiece - s / kFlPiece + 1u; }

// Piece x: its bytes [a0, a1) of staging, whether it is its range's first, the range and where that ends in staging.
// False: there is no such piece.
__device__ __forceinline__ bool fl_piece(const FlArgs &a, uint64_t x, uintptr_t &a0, uintptr_t &a1, bool &head, uint32_t &r,
                                         uintptr_t &end) {
    if (x >= a.pfirst[a.n]) return false;  // (the whole workgroup)
    r = rr_bound<true>(a.pfirst + 1, 0, a.n, x);  // the range with pfirst[r] <= x < pfirst[r + 1]
    const uint64_t j = x - a.pfirst[r];
    const uint64_t s = a.src[r], e = s + (a.in_off[r + 1u] - a.in_off[r]);
    const uint64_t cell = s / kFlPiece + j;
    const uint64_t b0 = cell * kFlPiece > s ? cell * kFlPiece : s;
    const uint64_t b1 = (cell + 1u) * kFlPiece < e ? (cell + 1u) * kFlPiece : e;  // (b0 < b1: the range touches the cell)
    a0 = (uintptr_t)a.stage + b0;
    a1 = (uintptr_t)a.stage + b1;
    end = (uintptr_t)a.stage + e;
    head = j == 0;
    return true;
}
__device__ __forceinline__ bool fl_piece(const FlArgs &a, uint64_t x, uintptr_t &a0, uintptr_t &a1, bool &head) {
    uint32_t r;
    uintptr_t end;
    return fl_piece(a, x, a0, a1, head, r, end);
}

// The rows of piece [a0, a1) for this lane: the aligned words (zero where the lane has none), the masks of the two
// delimiters and of the bytes inside the piece, and the pairs.
struct FlRows {
    uint4 v[kFlItems];
    uint32_t fm[kFlItems], dm[kFlItems], vm[kFlItems], e[kFlItems];
};
__device__ __forceinline__ void fl_rows(const FlArgs &a, uintptr_t a0, uintptr_t a1, FlRows &w) {
    const uintptr_t w0 = a0 & ~(uintptr_t)15;  // (a piece lies in one 16 KiB cell: at most kFlItems rows of words)
    const uint32_t sd = a.delim * 0x01010101u, sf = a.fdelim * 0x01010101u;
#pragma unroll
    for (uint32_t u = 0; u < kFlItems; u++) {  // aligned words of staging, several loads in flight per lane
        const uintptr_t p = w0 + 16u * (uintptr_t)(u * kFlThreads + threadIdx.x);
        w.v[u] = make_uint4(0, 0, 0, 0);
        if (p < a1) w.v[u] = *(const uint4 *)p;
    }
#pragma unroll
    for (uint32_t u = 0; u < kFlItems; u++) {
        const uintptr_t p = w0 + 16u * (uintptr_t)(u * kFlThreads + threadIdx.x);
        w.fm[u] = w.dm[u] = w.vm[u] = w.e[u] = 0;
        if (p >= a1) continue;
        uint32_t m[4];
        ln_word(w.v[u], sd, p, a0, a1, m);
        w.dm[u] = fd_mask16(m);
        ln_word(w.v[u], sf, p, a0, a1, m);
        w.fm[u] = fd_mask16(m);
        const uint32_t lo = p < a0 ? (uint32_t)(a0 - p) : 0u, hi = a1 - p < 16u ? (uint32_t)(a1 - p) : 16u;
        w.vm[u] = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
        w.e[u] = fl_elem(w.fm[u], w.dm[u]);
    }
}

// the compiled list in LDS, and what a line starts with
struct FlList {
    const uint64_t *b;  // LDS: the changes, ascending, UINT64_MAX behind them
    uint32_t n;         // changes in use
    uint32_t idx0, rem0;  // at field 0: the changes at or in front of it (0 or 1), and the fields up to the next
};
__device__ __forceinline__ uint32_t fl_clamp(uint64_t d) { return d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d; }

// the list from device memory into LDS (ends in a barrier)
__device__ __forceinline__ FlList fl_load(const FlSet *__restrict__ set, uint64_t *lds) {
    if (threadIdx.x < kFlBounds) lds[threadIdx.x] = set->b[threadIdx.x];
    __syncthreads();
    FlList l;
    l.b = lds;
    l.n = (uint32_t)set->n;
    l.idx0 = lds[0] == 0 ? 1u : 0u;
    l.rem0 = fl_clamp(lds[l.idx0]);
    return l;
}

// The bytes kept of a word whose first byte (the first inside the piece) has field number k: bit i, byte i.  A body
// byte of field j is kept iff j is in S; the delimiter in front of field j iff j is in S and is not its least member
// (the change that list index 0 -> 1 marks); a line delimiter always, and the count starts again behind it.
__device__ __forceinline__ uint32_t fl_keep(uint32_t fm, uint32_t dm, uint64_t k, const FlList &l) {
    uint32_t lo = 0, hi = l.n;  // the first change above k: b[n] = UINT64_MAX is
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (l.b[mid] <= k) lo = mid + 1u;
        else hi = mid;
    }
    uint32_t idx = lo, rem = fl_clamp(l.b[lo] - k);  // (rem >= 1; a word holds 16 delimiters at most: a clamped one never ends)
    bool in = (idx & 1u) != 0;
    uint32_t keep = 0, pos = 0;
    for (uint32_t marks = fm | dm; marks; marks &= marks - 1u) {
        const uint32_t bit = marks & (0u - marks);
        if (in) keep |= bit - (1u << pos);  // the bytes between the delimiters
        if (dm & bit) {
            keep |= bit;
            idx = l.idx0;
            in = idx != 0;
            rem = l.rem0;
        } else {
            bool least = false;
            if (--rem == 0) {
                least = idx == 0;
                idx++;
                in = !in;
                rem = fl_clamp(l.b[idx] - l.b[idx - 1u]);
            }
            if (in && !least) keep |= bit;
        }
        pos = (uint32_t)__ffs((int)bit);
    }
    if (in) keep |= 0x10000u - (1u << pos);
    return keep;
}

// The walk of piece [a0, a1), whose first byte has field number `cin`: keep[u] of every row.  Returns the lane's count.
__device__ __forceinline__ uint32_t fl_walk(const FlArgs &a, uintptr_t a0, uintptr_t a1, uint64_t cin, const FlList &l,
                                            uint32_t *wsum, FlRows &w, uint32_t (&keep)[kFlItems]) {
    fl_rows(a, a0, a1, w);
    uint32_t ex[kFlItems], total, c = 0;
    fl_scan<kFlItems>(w.e, wsum, ex, &total);
#pragma unroll
    for (uint32_t u = 0; u < kFlItems; u++) {
        keep[u] = 0;
        if (!w.vm[u]) continue;
        const uint64_t k = ((ex[u] & kFlReset) ? 0u : cin) + (ex[u] & ~kFlReset);
        keep[u] = fl_keep(w.fm[u], w.dm[u], k, l) & w.vm[u];
        c += (uint32_t)__popc(keep[u]);
    }
    return c;
}

// One workgroup: pfirst[r] = the pieces in front of range r, pfirst[n] = the pieces.
__global__ __launch_bounds__(kFlThreads) void k_fl_plan(uint32_t n, const uint64_t *__restrict__ src,
                                                        const uint64_t *__restrict__ in_off, uint64_t *__restrict__ pfirst,
                                                        uint64_t *rec) {
    __shared__ uint64_t wsum[4];
    uint64_t run = 0;  // every thread keeps its own copy
    for (uint64_t base = 0; base < n; base += kFlThreads) {
        const uint64_t r = base + threadIdx.x;
        uint64_t mine = 0, step;
        if (r < n) {
            const uint64_t len = in_off[r + 1u] - in_off[r];
            if (len) mine = fl_pieces(src[r], len);
        }
        const uint64_t ex = run + block_exclusive_scan256(mine, wsum, &step);
        run += step;
        if (r < n) pfirst[r] = ex;
    }
    if (threadIdx.x == 0) {
        pfirst[n] = run;
        rec[kFlRecPieces] = run;
    }
}

// Workgroup x: carry[x] of piece x.
__global__ __launch_bounds__(kFlThreads) void k_fl_carry(FlArgs a, uint32_t *__restrict__ carry) {
    __shared__ uint32_t wsum[4u * kFlItems];
    uintptr_t a0, a1;
    bool head;
    if (!fl_piece(a, blockIdx.x, a0, a1, head)) return;
    FlRows w;
    fl_rows(a, a0, a1, w);
    uint32_t ex[kFlItems], total;
    fl_scan<kFlItems>(w.e, wsum, ex, &total);
    if (threadIdx.x == 0) carry[blockIdx.x] = total | (head ? kFlReset | kFlHead : 0u);
}

// One workgroup: cin[x] = the field delimiters between the last line delimiter (or the range's start) in front of piece x
// and the piece.
__global__ __launch_bounds__(kFlThreads) void k_fl_carry_scan(const uint32_t *__restrict__ carry, const uint64_t *__restrict__ pfirst,
                                                              uint32_t n, uint64_t *__restrict__ cin) {
    __shared__ uint64_t wsum[4];
    const uint64_t n_pieces = pfirst[n];
    uint64_t run = 0;  // every thread keeps its own copy
    for (uint64_t i_base = 0; i_base < n_pieces; i_base += (uint64_t)kFlThreads * kFlScanItems) {
        const uint64_t i0 = i_base + (uint64_t)threadIdx.x * kFlScanItems;
        uint32_t c[kFlScanItems];
        uint64_t mine = 0, step;
#pragma unroll
        for (uint32_t j = 0; j < kFlScanItems; j++) {
            c[j] = i0 + j < n_pieces ? carry[i0 + j] : 0u;
            mine = fl_join64(mine, ((c[j] & kFlReset) ? kFlReset64 : 0u) | (c[j] & (kFlHead - 1u)));
        }
        uint64_t ex = fl_join64(run, fl_scan64(mine, wsum, &step));
        run = fl_join64(run, step);
#pragma unroll
        for (uint32_t j = 0; j < kFlScanItems; j++) {
            if (i0 + j < n_pieces) cin[i0 + j] = (c[j] & kFlHead) ? 0u : ex & ~kFlReset64;
            ex = fl_join64(ex, ((c[j] & kFlReset) ? kFlReset64 : 0u) | (c[j] & (kFlHead - 1u)));
        }
    }
}

// Workgroup x: cnt[x] = the bytes piece x keeps.
__global__ __launch_bounds__(kFlThreads) void k_fl_count(FlArgs a, const FlSet *__restrict__ set, const uint64_t *__restrict__ cin,
                                                         uint32_t *__restrict__ cnt) {
    __shared__ uint64_t list[kFlBounds];
    __shared__ uint32_t wsum[4u * kFlItems];
    uintptr_t a0, a1;
    bool head;
    if (!fl_piece(a, blockIdx.x, a0, a1, head)) return;
    const FlList l = fl_load(set, list);
    FlRows w;
    uint32_t keep[kFlItems];
    const uint32_t c = wave_reduce_add(fl_walk(a, a0, a1, cin[blockIdx.x], l, wsum, w, keep));
    __syncthreads();  // (the scan has read wsum)
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One workgroup: obase[x] = the kept bytes of the pieces in front of x, obase[pieces] = the total; out_off[r] =
// obase[pfirst[r]] for r <= n (an empty range has its successor's); the record.
__global__ __launch_bounds__(kFlThreads) void k_fl_scan(const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ pfirst,
                                                        uint32_t n, uint64_t *obase, uint64_t *__restrict__ out_off, uint64_t *rec) {
    __shared__ uint64_t wsum[4];
    const uint64_t n_pieces = pfirst[n];
    uint64_t run = 0;  // every thread keeps its own copy
    for (uint64_t i_base = 0; i_base < n_pieces; i_base += (uint64_t)kFlThreads * kFlScanItems) {
        const uint64_t i0 = i_base + (uint64_t)threadIdx.x * kFlScanItems;
        uint32_t c[kFlScanItems];
        uint64_t sum = 0, step;
#pragma unroll
        for (uint32_t j = 0; j < kFlScanItems; j++) {
            c[j] = i0 + j < n_pieces ? cnt[i0 + j] : 0u;
            sum += c[j];
        }
        uint64_t ex = run + block_exclusive_scan256(sum, wsum, &step);
        run += step;
#pragma unroll
        for (uint32_t j = 0; j < kFlScanItems; j++) {
            if (i0 + j < n_pieces) obase[i0 + j] = ex;
            ex += c[j];
        }
    }
    if (threadIdx.x == 0) {
        obase[n_pieces] = run;
        rec[kFlRecTotal] = run;
    }
    __syncthreads();  // obase is read below by other threads of this workgroup
    for (uint64_t r = threadIdx.x; r <= n; r += kFlThreads) out_off[r] = obase[pfirst[r]];
}

// Workgroup x stores the kept bytes of piece x at out[obase[x] ..].  A piece that keeps nothing is left at once, and
// every piece when the output does not fit.
__global__ __launch_bounds__(kFlThreads) void k_fl_write(FlArgs a, const FlSet *__restrict__ set, const uint64_t *__restrict__ cin,
                                                         const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ obase,
                                                         const uint64_t *__restrict__ rec, uint8_t *__restrict__ out,
                                                         uint64_t out_cap) {
    __shared__ uint64_t list[kFlBounds];
    __shared__ uint32_t wsum[4u * kFlItems];
    __shared__ uint4 obuf[kFlPiece / 16u + 1u];  // the piece's output, behind `lead` bytes
    uintptr_t a0, a1;
    bool head;
    if (!fl_piece(a, blockIdx.x, a0, a1, head)) return;
    const uint32_t kept = cnt[blockIdx.x];
    if (kept == 0 || rec[kFlRecTotal] > out_cap) return;  // (the whole workgroup)
    const FlList l = fl_load(set, list);
    FlRows w;
    uint32_t keep[kFlItems], c[kFlItems], at[kFlItems], total;
    fl_walk(a, a0, a1, cin[blockIdx.x], l, wsum, w, keep);
#pragma unroll
    for (uint32_t u = 0; u < kFlItems; u++) c[u] = (uint32_t)__popc(keep[u]);
    fl_scan<kFlItems>(c, wsum, at, &total);  // (plain sums: a word keeps 16 bytes at most)
    uint8_t *dst = out + obase[blockIdx.x];
    const uint32_t lead = (uint32_t)((uintptr_t)dst & 15u);
    uint8_t *ob = (uint8_t *)obuf;
#pragma unroll
    for (uint32_t u = 0; u < kFlItems; u++) {
        uint32_t o = lead + at[u];
        const uint32_t q[4] = {w.v[u].x, w.v[u].y, w.v[u].z, w.v[u].w};
#pragma unroll
        for (uint32_t i = 0; i < 16u; i++)
            if (keep[u] & (1u << i)) ob[o++] = (uint8_t)(q[i >> 2] >> (8u * (i & 3u)));
    }
    __syncthreads();
    // word i of LDS is the 16 bytes at the aligned address (dst - lead) + 16 i; the piece's bytes are [lead, lead + kept)
    const uint32_t end = lead + kept;
    for (uint32_t i = threadIdx.x; 16u * i < end; i += kFlThreads) {
        if (16u * i >= lead && 16u * i + 16u <= end) {
            *(uint4 *)(dst - lead + 16u * (uintptr_t)i) = obuf[i];
            continue;
        }
        const uint32_t b0 = 16u * i > lead ? 16u * i : lead, b1 = 16u * i + 16u < end ? 16u * i + 16u : end;
        for (uint32_t b = b0; b < b1; b++) dst[b - lead] = ob[b];  // a word shared with a neighbour piece, or the output's edge
    }
}
