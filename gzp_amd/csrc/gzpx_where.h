// gzpx_where.h -- WHICH lines of a BGZF / Mgzip stream in device memory hold numbers that pass a predicate: awk '$6 >= 30'
// between grep and cut.  The rows of a set of line ranges whose cells satisfy a conjunction (ANY: a disjunction) of
// comparisons, as a table of line ranges in device memory that the reads by line, field and column take where it lies.
// Included from gzpx_kernels.hip behind gzpx_columns.h, whose stages run as they are with the terms' distinct fields as
// the column list; no cell is stored.  (Definitions and the truth of a term: include/gzpx.h.)
// gzpx_where_text_device adds terms on the TEXT of a field -- awk '$1 == "chr7" && $7 == "PASS" && $6 >= 30' -- to the
// same walk: a third cell type whose value is the field's bytes where they are staged, and a pool of constants.
//
// Behind k_fl_plan .. k_cl_rows_scan (cin, rin, row_off, the rows R in the columns' record):
//
//   k_wh_parse<kText>  (false: terms on numbers alone, the code as it was; true: a term is on a TEXT column)
//                    cl_parse (gzpx_columns.h) with the sink WhSink: the lane that owns a cell -- the opener's, or for
//                    MISSING the lane that closes the line -- has it in registers, tests it against the terms of its
//                    column (staged in LDS once per workgroup, like the column list) and sets the row's bit in the row
//                    bitmap with at most one atomicOr, only when the cell DECIDES something: without ANY a cell that
//                    makes a term false rejects its row, with ANY a cell that makes a term true accepts it.  Lanes of
//                    two workgroups set bits of one word whenever a row runs through a piece boundary.  Rows at or
//                    behind row_off[r + 1] set no bit (cl_store), and nothing is set when R exceeds the bitmap.
//                    A TEXT cell is the field's bytes in LDS and their number capped at 65 (cl_open); the constants lie in
//                    a pool of at most 2 KiB staged in LDS behind the terms, and wh_text compares a byte at a time.
//   k_wh_starts      a lane a range: bit row_off[r] of a second bitmap for every range that is not empty.
//   k_wh_runs_count  the bitmap a byte a lane, 64 bytes a workgroup, read inverted when the bits mean "rejected" (XOR
//                    the caller's INVERT); sl_byte clears the bits at and behind R.  A run never leaves its range: the
//                    rising edges are w & (~(w << 1 | the msb in front) | starts), so a range's first row opens a run
//                    even when the row in front is selected.
//   k_wh_runs_scan   one workgroup: the counts -> the rank of every group's first rising edge; the record.
//   k_wh_runs_write  the bytes again; the falling edges are w & (~(w >> 1 | the lsb behind) | starts >> 1 | the starts'
//                    lsb behind): the row in front of a range's first closes its run.  Ranks as in gzpx_select.h: the
//                    j-th rising edge opens run j, a falling edge closes the run of the last rising edge at or in front
//                    of it.  An edge at row i finds its range -- the last r with row_off[r] <= i, which is not empty --
//                    by binary search in row_off and stores the LINE ranges[r].begin + (i - row_off[r]) (the falling
//                    edge one more), to ranks below runs_cap only.
//
// R is on the device only (the table form), so the runs kernels take it from the record: the host sizes the bitmaps and
// the grids by a bound it knows, and a workgroup sweeps the groups of kSlRunRecords rows below R that are its own.
// Bits set with atomicOr do not depend on order, scans place every run and the counts are integer sums: the result is
// the same bit for bit from run to run.  No kernel's depth of dependent global loads grows with the stream beyond that
// binary search (log2 of the ranges).

constexpr uint32_t kWhRunGrid = 65536;  // workgroups of the runs kernels, at most
static_assert(sizeof(WhTerms) % 4u == 0 && sizeof(WhTerms) / 4u <= kFlThreads, "staged a dword a lane");

// the truth of one term on a cell (include/gzpx.h): a comparison on a cell that is not OK is false, NE included
__device__ __forceinline__ bool wh_term(uint32_t op, uint64_t value, bool is_int, uint64_t bits, uint32_t st) {
    const bool ok = st == kClOk;
    if (op == kWhIsOk) return ok;
    if (op == kWhNotOk) return !ok;
    if (!ok) return false;
    bool lt, eq, gt;
    if (is_int) {
        const int64_t x = (int64_t)bits, y = (int64_t)value;
        lt = x < y;
        eq = x == y;
        gt = x > y;
    } else {
        double x, y;
        __builtin_memcpy(&x, &bits, 8);
        __builtin_memcpy(&y, &value, 8);
        lt = x < y;  // (IEEE: all three false for the cell "nan", -0.0 == 0.0)
        eq = x == y;
        gt = x > y;
    }
    switch (op) {
        case kWhLt: return lt;
        case kWhLe: return lt || eq;
        case kWhEq: return eq;
        case kWhNe: return !eq;
        case kWhGe: return gt || eq;
        default: return gt;
    }
}

// The truth of one term on a TEXT cell (include/gzpx.h): the field's bytes b[0, len) against the constant
// pool[value & 0xFFFFFFFF, + value >> 32), both in LDS, a byte at a time (neither is aligned).  len is capped at
// kClMaxBytes + 1 and the constant holds c <= kWhTextMax bytes, so min(len, c) bytes and then len against c decide
// every op exactly: a capped length still exceeds every c.  No byte behind b[min(len, c)) is read.
__device__ __forceinline__ bool wh_text(uint32_t op, uint64_t value, const uint8_t *pool, const uint8_t *b, uint32_t len, uint32_t st) {
    const bool ok = st == kClOk;
    if (op == kWhIsOk) return ok;
    if (op == kWhNotOk) return !ok;
    if (!ok) return false;  // MISSING: NE and NOT_PREFIX too
    const uint8_t *k = pool + (uint32_t)value;
    const uint32_t c = (uint32_t)(value >> 32), n = len < c ? len : c;
    uint32_t i = 0;
    while (i < n && b[i] == k[i]) i++;
    bool lt, gt;
    if (i < n) {
        lt = b[i] < k[i];  // (unsigned bytes)
        gt = !lt;
    } else {
        lt = len < c;  // the shorter first
        gt = len > c;
    }
    switch (op) {
        case kWhLt: return lt;
        case kWhLe: return !gt;
        case kWhEq: return !lt && !gt;
        case kWhNe: return lt || gt;
        case kWhGe: return !lt;
        case kWhGt: return gt;
        case kWhPrefix: return i == c;
        default: return i != c;  // kWhNotPrefix
    }
}

// the sink of gzpx_where_lines_device: the cell against the terms of its column.  kText: columns of type kClText may be
// among them, and `pool` holds their constants.
template <bool kTextColumns>
struct WhSink {
    static constexpr bool kText = kTextColumns;
    const WhTerms *t;     // LDS
    const uint8_t *pool;  // LDS (kText)
    uint32_t *bitmap;
    uint64_t cap;  // its bits
    __device__ __forceinline__ bool leaves(uint64_t rows) const { return rows > cap; }
    __device__ __forceinline__ void operator()(const ClWalk &k, uint32_t c, uint64_t row, uint64_t bits, uint32_t st, const uint8_t *b,
                                               uint32_t len) const {
        const bool is_int = k.type[c] == 0u, mark = t->any != 0u;
        bool is_text = false;
        if constexpr (kText) is_text = k.type[c] == kClText;
        bool decided = false;
        for (uint32_t i = t->first[c]; i < t->first[c + 1u] && !decided; i++)
            decided = (is_text ? wh_text(t->op[i], t->value[i], pool, b, len, st) : wh_term(t->op[i], t->value[i], is_int, bits, st)) == mark;
        if (decided) atomicOr(&bitmap[row >> 5], 1u << (row & 31u));
    }
};

// The walk with the testing sink: the rows that a cell decides into the row bitmap.  kText false is the parse of terms on
// numbers alone and reads the WhTerms at the head of `terms`; kText true stages the pool's bytes in use behind it.
template <bool kText>
__global__ __launch_bounds__(kFlThreads) void k_wh_parse(FlArgs a, const ClCols *__restrict__ cols, const WhTextTerms *__restrict__ terms,
                                                         const uint64_t *__restrict__ cin, const uint64_t *__restrict__ rin,
                                                         const uint64_t *__restrict__ row_off, uint64_t *rec, uint32_t *bitmap,
                                                         uint64_t cap) {
    __shared__ ClLds l;
    if constexpr (kText) {
        __shared__ WhTextTerms t;
        constexpr uint32_t head = (uint32_t)offsetof(WhTextTerms, pool) / 4u;
        static_assert(offsetof(WhTextTerms, pool) % 4u == 0 && head <= kFlThreads, "the head a dword a lane, the pool by a loop");
        if (threadIdx.x < head) ((uint32_t *)&t)[threadIdx.x] = ((const uint32_t *)terms)[threadIdx.x];
        const uint32_t words = ((terms->pool_len < kWhPoolMax ? terms->pool_len : kWhPoolMax) + 3u) / 4u;
        for (uint32_t i = threadIdx.x; i < words; i += kFlThreads) ((uint32_t *)t.pool)[i] = ((const uint32_t *)terms->pool)[i];
        cl_parse(a, l, cols, cin, rin, row_off, rec, WhSink<true>{&t.t, t.pool, bitmap, cap});
    } else {
        __shared__ WhTerms t;
        if (threadIdx.x < sizeof(WhTerms) / 4u) ((uint32_t *)&t)[threadIdx.x] = ((const uint32_t *)terms)[threadIdx.x];
        cl_parse(a, l, cols, cin, rin, row_off, rec, WhSink<false>{&t, nullptr, bitmap, cap});
    }
}

// Lane r: the first row of range r, if it has one.  (Ranges in front of it that are empty share its row_off; atomicOr:
// lanes of different workgroups set bits of one word.)
__global__ __launch_bounds__(kFlThreads) void k_wh_starts(const uint64_t *__restrict__ row_off, uint32_t n, uint64_t cap,
                                                          uint32_t *starts) {
    const uint64_t r = (uint64_t)blockIdx.x * kFlThreads + threadIdx.x;
    if (r >= n || row_off[n] > cap) return;
    const uint64_t i = row_off[r];
    if (row_off[r + 1u] > i) atomicOr(&starts[i >> 5], 1u << (i & 31u));
}

// the rows the runs kernels see: R, or none when the bitmaps do not hold them
__device__ __forceinline__ uint64_t wh_rows(const uint64_t *__restrict__ cl_rec, uint64_t cap) {
    const uint64_t n = cl_rec[kClRecRows];
    return n > cap ? 0u : n;
}

// the lane's byte k of the selected rows, of the starts, and its rising edges (every lane of the wave calls it)
__device__ __forceinline__ uint32_t wh_rises(const uint8_t *__restrict__ bitmap, const uint8_t *__restrict__ starts, uint64_t k,
                                             uint64_t n_rows, uint32_t invert, uint32_t &w, uint32_t &st) {
    w = sl_byte(bitmap, k, n_rows, invert);
    st = sl_byte(starts, k, n_rows, 0u);
    uint32_t front = __shfl_up(w, 1);  // the neighbour lane's byte; the wave's first lane loads it
    if ((threadIdx.x & 63u) == 0) front = k ? sl_byte(bitmap, k - 1u, n_rows, invert) : 0u;
    return w & (~((w << 1) | (front >> 7)) | st) & 0xFFu;
}

// Workgroup x, for every group g of kSlRunRecords rows that is its own: cnt[2 g] = rising edges, cnt[2 g + 1] = set bits.
__global__ __launch_bounds__(kSlRunThreads) void k_wh_runs_count(const uint8_t *__restrict__ bitmap, const uint8_t *__restrict__ starts,
                                                                 const uint64_t *__restrict__ cl_rec, uint64_t cap, uint32_t invert,
                                                                 uint32_t *__restrict__ cnt) {
    const uint64_t n_rows = wh_rows(cl_rec, cap), groups = (n_rows + kSlRunRecords - 1u) / kSlRunRecords;
    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        uint32_t w, st;
        const uint32_t rises = wh_rises(bitmap, starts, g * kSlRunThreads + threadIdx.x, n_rows, invert, w, st);
        const uint32_t cr = wave_reduce_add((uint32_t)__popc(rises)), cs = wave_reduce_add((uint32_t)__popc(w));
        if (threadIdx.x == 0) {
            cnt[2u * g] = cr;
            cnt[2u * g + 1u] = cs;
        }
    }
}

// One workgroup, kSlScanStep groups a step.  bases[g] = the rank of group g's first rising edge.  The record: runs,
// selected rows, and the rows and the cells that are not OK from the columns' record.  (Both sums stay below 2^32:
// R <= 0xFFFFFFF0.)
__global__ __launch_bounds__(kFdThreads) void k_wh_runs_scan(const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ cl_rec,
                                                             uint64_t cap, uint32_t *__restrict__ bases, uint64_t *rec) {
    static_assert(kSlScanStep == kFdThreads, "a thread takes one group's counts a step");
    __shared__ uint64_t wsum[4];
    const uint64_t n_rows = wh_rows(cl_rec, cap), groups = (n_rows + kSlRunRecords - 1u) / kSlRunRecords;
    uint64_t run = 0;  // rising edges << 32 | set bits; every thread keeps its own copy
    for (uint64_t base = 0; base < groups; base += kSlScanStep) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t mine = i < groups ? ((uint64_t)cnt[2u * i] << 32) | cnt[2u * i + 1u] : 0u;
        uint64_t step;
        const uint64_t ex = run + block_exclusive_scan256(mine, wsum, &step);
        run += step;
        if (i < groups) bases[i] = (uint32_t)(ex >> 32);
    }
    if (threadIdx.x == 0) {
        rec[kWhRecRuns] = run >> 32;
        rec[kWhRecSelected] = (uint32_t)run;
        rec[kWhRecRows] = cl_rec[kClRecRows];
        rec[kWhRecNotOk] = cl_rec[kClRecNotOk];
    }
}

// the line that is row i: lines[2 r] + (i - row_off[r]) for the last range r with row_off[r] <= i (n >= 1, row_off[0] = 0)
__device__ __forceinline__ uint64_t wh_line(const uint64_t *__restrict__ row_off, const uint64_t *__restrict__ lines, uint32_t n,
                                            uint64_t i) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (row_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lines[2u * (uint64_t)lo] + (i - row_off[lo]);
}

// Workgroup x writes the runs that begin or end in the groups that are its own: runs[2 j] = begin, runs[2 j + 1] = end
// of run j < cap, as line numbers.  A group without a set bit is passed over.
__global__ __launch_bounds__(kSlRunThreads) void k_wh_runs_write(const uint8_t *__restrict__ bitmap, const uint8_t *__restrict__ starts,
                                                                 const uint64_t *__restrict__ cl_rec, uint64_t cap, uint32_t invert,
                                                                 const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ bases,
                                                                 const uint64_t *__restrict__ row_off, const uint64_t *__restrict__ lines,
                                                                 uint32_t n_ranges, uint64_t *__restrict__ runs, uint64_t runs_cap) {
    const uint64_t n_rows = wh_rows(cl_rec, cap), groups = (n_rows + kSlRunRecords - 1u) / kSlRunRecords;
    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        if (cnt[2u * g + 1u] == 0) continue;  // (the whole workgroup)
        const uint64_t k = g * kSlRunThreads + threadIdx.x;
        uint32_t w, st;
        const uint32_t rises = wh_rises(bitmap, starts, k, n_rows, invert, w, st);
        uint32_t behind = __shfl_down(w, 1), st_behind = __shfl_down(st, 1);  // the neighbour lane's bytes; the wave's last lane loads them
        if ((threadIdx.x & 63u) == 63u) {
            behind = sl_byte(bitmap, k + 1u, n_rows, invert);
            st_behind = sl_byte(starts, k + 1u, n_rows, 0u);
        }
        const uint32_t falls = w & (~((w >> 1) | ((behind & 1u) << 7)) | (st >> 1) | ((st_behind & 1u) << 7));
        const uint32_t c = (uint32_t)__popc(rises);
        const uint64_t rank = (uint64_t)bases[g] + (wave_incl_add(c) - c);  // of the lane's first rising edge
        for (uint32_t e = rises; e; e &= e - 1u) {
            const uint32_t b = (uint32_t)__ffs((int)e) - 1u;
            const uint64_t j = rank + (uint32_t)__popc(rises & ((1u << b) - 1u));
            if (j < runs_cap) runs[2u * j] = wh_line(row_off, lines, n_ranges, 8u * k + b);
        }
        for (uint32_t e = falls; e; e &= e - 1u) {
            const uint32_t b = (uint32_t)__ffs((int)e) - 1u;
            const uint64_t j = rank + (uint32_t)__popc(rises & ((2u << b) - 1u)) - 1u;  // (a rising edge lies at or in front of it)
            if (j < runs_cap) runs[2u * j + 1u] = wh_line(row_off, lines, n_ranges, 8u * k + b) + 1u;
        }
    }
}
