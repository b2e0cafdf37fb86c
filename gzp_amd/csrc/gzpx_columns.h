// gzpx_columns.h -- NUMERIC COLUMNS of the lines of a BGZF / Mgzip stream in device memory: the last step of
// grep ... | cut -f ... | <numbers>.  One int64 / float64 cell and one status byte per (column, row), placed densely.
// Included from gzpx_kernels.hip behind gzpx_fields.h, whose pieces, rows of words and scans it uses as they are.
// (Definitions, the two grammars and the exact-conversion rule: include/gzpx.h.)
//
// Behind k_fl_plan, k_fl_carry and k_fl_carry_scan (pfirst, cin[x] = the field number of piece x's first byte):
//
//   k_cl_rows        one workgroup per piece: its line delimiters.
//   k_cl_rows_scan   one workgroup: rbase = the exclusive sum of the ranges' line counts -> row_off, the rows R into the
//                    record; a scan of the pieces' counts restarted at every range's first piece -> rin[x], the lines of
//                    its range in front of piece x.  The row of piece x's first byte is row_off[r] + rin[x].
//   k_cl_parse       cl_parse with the storing sink.  One workgroup per piece, fl_walk's geometry: 256 lanes x one aligned 16-byte word a row, the four
//                    rows loaded together; the segmented scan gives the field number of every word's first byte, a
//                    plain scan of the line delimiters its row.  The piece and the kClOverhang bytes behind it (clamped
//                    at the range's end) are staged in LDS, so the parser's byte steps are LDS reads.
//
// WHO STORES A CELL.  A field is OPENED by the byte in front of it -- a field delimiter, a line delimiter -- or by the
// range's first byte; the lane whose word holds the opener owns the field, looks its number up in the column list (16
// entries in LDS, binary search) and, if it is listed, parses at most 65 bytes forward, never behind the range's end.
// A field whose opener is a piece's last byte lies in the next piece of the same range, which is contiguous in staging
// and inside the overhang.  A line is CLOSED by its delimiter, or by the range's end when the last line is
// unterminated; the closing lane knows the line's F fields and stores MISSING for every column at or above F.  So every
// cell of rows [0, R) is stored exactly once, by ordinary vector stores, at a place that scans alone decide.  The two
// counts are integer atomicAdds of per-workgroup sums: the result is the same bit for bit from run to run.
// A row at or behind its range's row_off[r + 1] -- staging does not hold the stream the table was built from -- is
// not stored: nothing is written outside the rows the table promised.
//
// THE SINK.  What happens to a cell is a type parameter of the walk (cl_parse<Sink>): ClStore keeps it in the arrays,
// gzpx_where.h's sink tests it against the terms of its column and keeps nothing.  cl_int, cl_float, cl_open, cl_close
// and the walk itself are the same code for both, so a cell cannot be parsed differently by the two calls.
//
// TEXT COLUMNS.  A sink with kText set may list columns of type kClText (gzpx_where_text_device).  cl_open finds such a
// field's extent like any other, skips both parsers and hands the sink the bytes in LDS and their number, capped at
// kClMaxBytes + 1: 65 says "longer than 64", which is all a constant of at most 64 bytes has to know.  The cell is OK
// whatever it holds; cl_close stores MISSING for it like for the others.  Sinks without kText compile as they did.

constexpr uint32_t kClStageWords = kFlPiece / 16u + (kClOverhang + 15u) / 16u + 1u;
static_assert(kClOverhang >= kClMaxBytes + 1u, "a field opened by a piece's last byte is parsed from LDS");

// 10^0 .. 10^22: every one a double without rounding
__constant__ double kClPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                    1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
constexpr uint64_t kClNaN = 0x7FF8000000000000ull, kClInf = 0x7FF0000000000000ull, kClSign = 0x8000000000000000ull;
enum { kClOk = 0, kClMissing = 1, kClEmpty = 2, kClInvalid = 3, kClRange = 4 };  // GZPX_CELL_*

__device__ __forceinline__ bool cl_digit(uint32_t c) { return c - 48u < 10u; }

// [+-]?[0-9]+ in b[0, len), 1 <= len <= 64
__device__ __forceinline__ uint32_t cl_int(const uint8_t *b, uint32_t len, uint64_t *bits) {
    *bits = 0;
    uint32_t i = 0;
    const bool neg = b[0] == '-';
    if (neg || b[0] == '+') i = 1;
    if (i == len) return kClInvalid;
    uint64_t v = 0;
    uint32_t nd = 0;  // digits behind the leading zeros: 19 of them never overflow 64 bits
    for (; i < len; i++) {
        const uint32_t d = (uint32_t)b[i] - 48u;
        if (d >= 10u) return kClInvalid;
        if (nd || d) {
            if (nd < 19u) v = v * 10u + d;
            nd++;
        }
    }
    if (nd > 19u || v > (neg ? kClSign : kClSign - 1u)) return kClRange;
    *bits = neg ? 0u - v : v;
    return kClOk;
}

// the float grammar of gzpx.h in b[0, len), 1 <= len <= 64, and its rule of exact conversion
__device__ __forceinline__ uint32_t cl_float(const uint8_t *b, uint32_t len, uint64_t *bits) {
    *bits = kClNaN;
    uint32_t i = 0;
    const bool neg = b[0] == '-';
    if (neg || b[0] == '+') i = 1;
    const uint32_t rest = len - i;
    if (rest == 3u || rest == 8u) {
        const char *inf = "infinity";
        bool is_nan = rest == 3u, is_inf = true;
        for (uint32_t j = 0; j < rest; j++) {
            const uint32_t c = b[i + j] | 0x20u;
            is_inf = is_inf && c == (uint32_t)inf[j];
            is_nan = is_nan && c == (uint32_t)"nan"[j];
        }
        if (is_nan) return kClOk;
        if (is_inf) {
            *bits = kClInf | (neg ? kClSign : 0u);
            return kClOk;
        }
    }
    uint64_t w = 0;
    uint32_t nd = 0, z = 0, frac = 0;  // digits of w; zeros behind them not yet taken in; fraction digits
    bool any = false, big = false, dot = false;
    for (; i < len; i++) {
        const uint32_t d = (uint32_t)b[i] - 48u;
        if (d >= 10u) {
            if (b[i] != '.' || dot) break;
            dot = true;
            continue;
        }
        any = true;
        if (dot) frac++;
        if (d == 0u) {
            if (nd) z++;
            continue;
        }
        if (nd + z + 1u > 19u) {
            big = true;  // (nd stays above 0: the zeros behind still count)
        } else {
            for (uint32_t j = 0; j <= z; j++) w *= 10u;
            w += d;
        }
        nd += z + 1u;
        z = 0;
    }
    if (!any) return kClInvalid;
    int32_t ev = 0;
    if (i < len) {
        if ((b[i] | 0x20u) != 'e') return kClInvalid;
        i++;
        bool eneg = false;
        if (i < len && (b[i] == '-' || b[i] == '+')) eneg = b[i++] == '-';
        if (i == len) return kClInvalid;
        for (; i < len; i++) {
            if (!cl_digit(b[i])) return kClInvalid;
            ev = ev * 10 + (int32_t)(b[i] - 48u);
            if (ev > (1 << 20)) ev = 1 << 20;  // (far outside the table whatever the digit counts are)
        }
        if (eneg) ev = -ev;
    }
    if (nd == 0u) {  // w = 0
        *bits = neg ? kClSign : 0u;
        return kClOk;
    }
    const int32_t q = ev - (int32_t)frac + (int32_t)z;
    if (big || w > (1ull << 53) || q < -22 || q > 22) return kClRange;
    double v = (double)w;  // exact
    v = q >= 0 ? v * kClPow10[q] : v / kClPow10[-q];  // one IEEE operation on two exact operands
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
    *bits = u | (neg ? kClSign : 0u);
    return kClOk;
}

// what the walk's lanes share
struct ClWalk {
    const uint64_t *field;  // LDS: the columns' field numbers, ascending
    const uint32_t *type;   // LDS
    uint32_t *bad;          // LDS: cells that are not OK, per column
    uint32_t n;
    uint64_t lo, hi;        // the least and the greatest field number listed
    const uint8_t *lds;     // the staged bytes: lds[i] is the byte at address w0 + i
    uintptr_t w0, end;      // the range ends at address `end`
    uint32_t delim, fdelim;
    uint64_t row_end;       // the first row behind the range's
};

// the sink of gzpx_read_columns_device: the cell and its status byte into the arrays
struct ClStore {
    static constexpr bool kText = false;  // no column of type kClText (cols_compile)
    uint64_t *values;
    uint8_t *status;
    uint64_t rows_cap;
    // every piece leaves at once when an array is given and the rows do not fit
    __device__ __forceinline__ bool leaves(uint64_t rows) const { return (values || status) && rows > rows_cap; }
    __device__ __forceinline__ void operator()(const ClWalk &, uint32_t c, uint64_t row, uint64_t bits, uint32_t st, const uint8_t *,
                                               uint32_t) const {
        const uint64_t at = (uint64_t)c * rows_cap + row;
        if (values) values[at] = bits;
        if (status) status[at] = (uint8_t)st;
    }
};

// (b, len: the field's bytes in LDS and their number capped at kClMaxBytes + 1; null and 0 for MISSING)
template <class Sink>
__device__ __forceinline__ void cl_store(const ClWalk &k, const Sink &sink, uint32_t c, uint64_t row, uint64_t bits, uint32_t st,
                                         const uint8_t *b, uint32_t len) {
    if (row >= k.row_end) return;
    if (st != kClOk) atomicAdd(&k.bad[c], 1u);
    sink(k, c, row, bits, st, b, len);
}

// the field of number f that starts at address s, in row `row`
template <class Sink>
__device__ __forceinline__ void cl_open(const ClWalk &k, const Sink &sink, uint64_t f, uintptr_t s, uint64_t row) {
    if (f < k.lo || f > k.hi) return;
    uint32_t lo = 0, hi = k.n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (k.field[mid] < f) lo = mid + 1u;
        else hi = mid;
    }
    if (lo == k.n || k.field[lo] != f) return;
    const uint8_t *b = k.lds + (s - k.w0);
    const uint32_t room = k.end - s < kClMaxBytes + 1u ? (uint32_t)(k.end - s) : kClMaxBytes + 1u;
    uint32_t len = 0;
    while (len < room && b[len] != k.fdelim && b[len] != k.delim) len++;
    if constexpr (Sink::kText) {
        if (k.type[lo] == kClText) {  // the bytes are the value: any length, any byte
            cl_store(k, sink, lo, row, 0u, kClOk, b, len);
            return;
        }
    }
    const bool is_int = k.type[lo] == 0u;
    uint64_t bits = is_int ? 0u : kClNaN;
    uint32_t st;
    if (len == 0u) st = kClEmpty;
    else if (len > kClMaxBytes) st = kClInvalid;
    else st = is_int ? cl_int(b, len, &bits) : cl_float(b, len, &bits);
    if (st != kClOk) bits = is_int ? 0u : kClNaN;
    cl_store(k, sink, lo, row, bits, st, b, len);
}

// a line of F fields ends in row `row`
template <class Sink>
__device__ __forceinline__ void cl_close(const ClWalk &k, const Sink &sink, uint64_t F, uint64_t row) {
    if (F > k.hi) return;
    for (uint32_t c = k.n; c > 0u && k.field[c - 1u] >= F; c--)
        cl_store(k, sink, c - 1u, row, k.type[c - 1u] == 0u ? 0u : kClNaN, kClMissing, nullptr, 0u);
}

// Workgroup x: rcnt[x] = the line delimiters of piece x.
__global__ __launch_bounds__(kFlThreads) void k_cl_rows(FlArgs a, uint32_t *__restrict__ rcnt) {
    __shared__ uint32_t wsum[4];
    uintptr_t a0, a1;
    bool head;
    if (!fl_piece(a, blockIdx.x, a0, a1, head)) return;
    FlRows w;
    fl_rows(a, a0, a1, w);
    uint32_t c = 0;
#pragma unroll
    for (uint32_t u = 0; u < kFlItems; u++) c += (uint32_t)__popc(w.dm[u]);
    c = wave_reduce_add(c);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) rcnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One workgroup.  lines[2 r], lines[2 r + 1]: the line numbers of range r.  row_off[r] = the rows in front of range r,
// row_off[n] = R, also into the record; rin[x] = the line delimiters of piece x's range in front of the piece (carry[x]
// says which pieces are a range's first).
__global__ __launch_bounds__(kFlThreads) void k_cl_rows_scan(const uint64_t *__restrict__ lines, const uint32_t *__restrict__ carry,
                                                             const uint32_t *__restrict__ rcnt, const uint64_t *__restrict__ pfirst,
                                                             uint32_t n, uint64_t *__restrict__ rin, uint64_t *__restrict__ row_off,
                                                             uint64_t *rec) {
    __shared__ uint64_t wsum[4];
    uint64_t run = 0;  // every thread keeps its own copy
    for (uint64_t base = 0; base < n; base += kFlThreads) {
        const uint64_t r = base + threadIdx.x;
        uint64_t step;
        const uint64_t mine = r < n ? lines[2u * r + 1u] - lines[2u * r] : 0u;
        const uint64_t ex = run + block_exclusive_scan256(mine, wsum, &step);
        run += step;
        if (r < n) row_off[r] = ex;
    }
    if (threadIdx.x == 0) {
        row_off[n] = run;
        rec[kClRecRows] = run;
    }
    const uint64_t n_pieces = pfirst[n];
    run = 0;
    for (uint64_t i_base = 0; i_base < n_pieces; i_base += (uint64_t)kFlThreads * kFlScanItems) {
        const uint64_t i0 = i_base + (uint64_t)threadIdx.x * kFlScanItems;
        uint64_t e[kFlScanItems];
        uint64_t mine = 0, step;
#pragma unroll
        for (uint32_t j = 0; j < kFlScanItems; j++) {
            e[j] = i0 + j < n_pieces ? ((carry[i0 + j] & kFlHead) ? kFlReset64 : 0u) | rcnt[i0 + j] : 0u;
            mine = fl_join64(mine, e[j]);
        }
        uint64_t ex = fl_join64(run, fl_scan64(mine, wsum, &step));
        run = fl_join64(run, step);
#pragma unroll
        for (uint32_t j = 0; j < kFlScanItems; j++) {
            if (i0 + j < n_pieces) rin[i0 + j] = (e[j] & kFlReset64) ? 0u : ex & ~kFlReset64;
            ex = fl_join64(ex, e[j]);
        }
    }
}

// what a workgroup of the walk keeps in LDS
struct ClLds {
    uint64_t field[kClMaxCols];
    uint32_t type[kClMaxCols];
    uint32_t bad[kClMaxCols];
    uint32_t wsum[4u * kFlItems];
    uint4 buf[kClStageWords];
};

// Workgroup x: the cells of the fields that piece x's bytes open, and MISSING for the lines it closes, each handed to
// the sink.  Every piece leaves at once when the sink says so of the rows.  (Whatever the caller staged in LDS of its
// own is readable in the sink: the scans' barriers stand in front of the walk.)
template <class Sink>
__device__ __forceinline__ void cl_parse(const FlArgs &a, ClLds &l, const ClCols *__restrict__ cols, const uint64_t *__restrict__ cin,
                                         const uint64_t *__restrict__ rin, const uint64_t *__restrict__ row_off, uint64_t *rec,
                                         const Sink &sink) {
    uintptr_t a0, a1, end;
    bool head;
    uint32_t r;
    if (!fl_piece(a, blockIdx.x, a0, a1, head, r, end)) return;
    if (sink.leaves(rec[kClRecRows])) return;  // (the whole workgroup)
    if (threadIdx.x < kClMaxCols) {
        l.field[threadIdx.x] = cols->field[threadIdx.x];
        l.type[threadIdx.x] = cols->type[threadIdx.x];
        l.bad[threadIdx.x] = 0;
    }
    FlRows w;
    fl_rows(a, a0, a1, w);
    const uintptr_t w0 = a0 & ~(uintptr_t)15;
#pragma unroll
    for (uint32_t u = 0; u < kFlItems; u++) {
        const uint32_t i = u * kFlThreads + threadIdx.x;
        if (w0 + 16u * (uintptr_t)i < a1) l.buf[i] = w.v[u];
    }
    {  // the overhang: the words behind the piece's that hold a byte in front of min(end, a1 + kClOverhang)
        const uintptr_t lim = end - a1 < kClOverhang ? end : a1 + kClOverhang;
        const uint32_t first = (uint32_t)((a1 - w0 + 15u) / 16u), last = (uint32_t)((lim - w0 + 15u) / 16u);
        if (first + threadIdx.x < last) l.buf[first + threadIdx.x] = *(const uint4 *)(w0 + 16u * (uintptr_t)(first + threadIdx.x));
    }
    uint32_t ex[kFlItems], rx[kFlItems], dc[kFlItems], total;
    fl_scan<kFlItems>(w.e, l.wsum, ex, &total);  // (its barriers stand between the stores to LDS above and the reads below)
#pragma unroll
    for (uint32_t u = 0; u < kFlItems; u++) dc[u] = (uint32_t)__popc(w.dm[u]);
    fl_scan<kFlItems>(dc, l.wsum, rx, &total);  // (plain sums)
    ClWalk k;
    k.field = l.field;
    k.type = l.type;
    k.bad = l.bad;
    k.n = cols->n;
    k.lo = l.field[0];
    k.hi = l.field[k.n - 1u];
    k.lds = (const uint8_t *)l.buf;
    k.w0 = w0;
    k.end = end;
    k.delim = a.delim;
    k.fdelim = a.fdelim;
    k.row_end = row_off[r + 1u];
    const uint64_t cin_x = cin[blockIdx.x], row_x = row_off[r] + rin[blockIdx.x];
#pragma unroll
    for (uint32_t u = 0; u < kFlItems; u++) {
        if (!w.vm[u]) continue;
        const uintptr_t p = w0 + 16u * (uintptr_t)(u * kFlThreads + threadIdx.x);
        uint64_t f = ((ex[u] & kFlReset) ? 0u : cin_x) + (ex[u] & ~kFlReset);
        uint64_t row = row_x + rx[u];
        if (head && p <= a0) cl_open(k, sink, 0, a0, row);  // the range's first byte (vm: a0 < p + 16)
        for (uint32_t marks = w.fm[u] | w.dm[u]; marks; marks &= marks - 1u) {
            const uint32_t bit = marks & (0u - marks);
            const uintptr_t s = p + (uint32_t)__ffs((int)bit);  // the byte behind the mark
            if (w.dm[u] & bit) {
                cl_close(k, sink, f + 1u, row);
                row++;
                f = 0;
                if (s < end) cl_open(k, sink, 0, s, row);
            } else {
                f++;
                cl_open(k, sink, f, s, row);
            }
        }
        // the range's last byte, when it does not end its line
        if (a1 == end && end - p <= 16u && !((w.dm[u] >> (uint32_t)(end - 1u - p)) & 1u)) cl_close(k, sink, f + 1u, row);
    }
    __syncthreads();
    if (threadIdx.x < k.n && l.bad[threadIdx.x]) atomicAdd((unsigned long long *)&rec[kClRecCol + threadIdx.x], (unsigned long long)l.bad[threadIdx.x]);
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t c = 0; c < k.n; c++) sum += l.bad[c];
        if (sum) atomicAdd((unsigned long long *)&rec[kClRecNotOk], (unsigned long long)sum);
    }
}

// The walk with the storing sink: every cell of rows [0, R) into d_values / d_status.
__global__ __launch_bounds__(kFlThreads) void k_cl_parse(FlArgs a, const ClCols *__restrict__ cols, const uint64_t *__restrict__ cin,
                                                         const uint64_t *__restrict__ rin, const uint64_t *__restrict__ row_off,
                                                         uint64_t *rec, uint64_t *__restrict__ values, uint8_t *__restrict__ status,
                                                         uint64_t rows_cap) {
    __shared__ ClLds l;
    cl_parse(a, l, cols, cin, rin, row_off, rec, ClStore{values, status, rows_cap});
}
