// gzpx_select.h -- WHICH lines of a BGZF / Mgzip stream in device memory hold a byte string: the records (groups of g
// lines) in which at least one hit of the search lies, or the records in which none does, as a table of line ranges in
// device memory that gzpx_read_lines_table_device reads where it lies.  Included from gzpx_kernels.hip behind
// gzpx_find.h, whose counting pass, scan and carry run in front of the marking pass.  (Definitions: include/gzpx.h.)
//
//   k_sl_mark        behind k_fd_count + k_fd_scan of a batch, one workgroup per piece: sl_mark, the marking pass on
//                    the walk frame (fd_walk, gzpx_find.h), so every hit's line comes out by the writing pass's
//                    arithmetic, carry included.  Instead of storing it, the lane sets bit line / g of the record
//                    bitmap (R bits, zeroed per call) with atomicOr -- lanes of different workgroups set bits of one
//                    word -- and only when the record differs from that of its previous hit.
//   k_sl_runs_count  behind the last batch: the bitmap a byte a lane, 64 bytes a workgroup.  A byte is XORed with 0xFF
//                    under INVERT and loses the bits at and behind R; its rising edges are w & ~(w << 1 | the msb of the
//                    byte in front).  One count of edges and one of set bits per workgroup.
//   k_sl_runs_scan   one workgroup: the counts -> the rank of every workgroup's first rising edge; the record (runs,
//                    records, and the hits of find's record beside them).
//   k_sl_runs_write  the bytes again: the j-th rising edge, at record r, stores d_runs[j].begin = g r; a falling edge at
//                    record r closes the run that the last rising edge at or in front of r opened, so its rank is the
//                    number of rising edges up to r less one, and it stores d_runs[rank].end = min(g (r + 1), L).  No
//                    search, and stores to ranks below runs_cap only.
// No kernel's depth of dependent global loads grows with the stream.

constexpr uint32_t kSlRunThreads = 64;  // one wave: the counts of a workgroup need no LDS
static_assert(kSlRunThreads * 8u == kSlRunRecords, "a lane takes one byte of the bitmap");

// the record a line lies in
__device__ __forceinline__ uint64_t sl_record(uint64_t line, uint64_t g) {
    if (g == 1u) return line;
    if (((line | g) >> 32) == 0) return (uint32_t)line / (uint32_t)g;
    return line / g;
}

// The marking pass of piece x0 + i by workgroup i, for the matcher M: the records of its hits.  A piece without a hit is
// left at once, the matcher unloaded.  No rank is needed: the walk is not ranked, and its prefix carries the delimiters
// alone.  Delimiters are always marked.  (A line at or behind L -- the stream is not the one the line table was built
// from -- has no bit.)
template <class M>
__device__ __forceinline__ void sl_mark(const FdArgs &a, uint32_t x0, const typename M::Src *__restrict__ src, typename M::Lds &lds,
                                        uint64_t (&wsum)[4], const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ bases,
                                        uint32_t *bitmap, uint64_t g, uint64_t n_records) {
    if (cnt[2u * (uint64_t)blockIdx.x] == 0) return;  // (the whole workgroup)
    const M mt(a, src, lds);
    uint64_t last = ~(uint64_t)0;  // the record of the lane's previous hit
    fd_walk<false>(a, x0 + blockIdx.x, mt, true, 0, bases[2u * (uint64_t)blockIdx.x + 1u], 0, wsum,
            [&](uint64_t, uintptr_t, uint64_t line) {
                const uint64_t r = sl_record(line, g);
                if (r != last && r < n_records) atomicOr(&bitmap[r >> 5], 1u << (r & 31u));
                last = r;
            });
}

// Workgroup i marks the records of the hits of piece x0 + i.
__global__ __launch_bounds__(kFdThreads) void k_sl_mark(FdArgs a, uint32_t x0, const uint32_t *__restrict__ d_pat,
                                                        const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ bases,
                                                        uint32_t *bitmap, uint64_t g, uint64_t n_records) {
    __shared__ FdPattern::Lds pat;
    __shared__ uint64_t wsum[4];
    sl_mark<FdPattern>(a, x0, d_pat, pat, wsum, cnt, bases, bitmap, g, n_records);
}

// byte k of the bitmap as the runs see it: inverted where asked, the bits at and behind R cleared
__device__ __forceinline__ uint32_t sl_byte(const uint8_t *__restrict__ bitmap, uint64_t k, uint64_t n_records, uint32_t invert) {
    if (8u * k >= n_records) return 0u;
    uint32_t w = bitmap[k];
    if (invert) w ^= 0xFFu;
    const uint64_t left = n_records - 8u * k;
    if (left < 8u) w &= (1u << left) - 1u;
    return w;
}

// the lane's byte of workgroup x and its rising edges (every lane of the wave calls it)
__device__ __forceinline__ uint32_t sl_rises(const uint8_t *__restrict__ bitmap, uint64_t k, uint64_t n_records, uint32_t invert,
                                             uint32_t &w) {
    w = sl_byte(bitmap, k, n_records, invert);
    uint32_t front = __shfl_up(w, 1);  // the neighbour lane's byte; the wave's first lane loads it
    if ((threadIdx.x & 63u) == 0) front = k ? sl_byte(bitmap, k - 1u, n_records, invert) : 0u;
    return w & ~((w << 1) | (front >> 7)) & 0xFFu;
}

// Workgroup x: cnt[2 x] = rising edges, cnt[2 x + 1] = set bits of records [kSlRunRecords x, kSlRunRecords (x + 1)).
__global__ __launch_bounds__(kSlRunThreads) void k_sl_runs_count(const uint8_t *__restrict__ bitmap, uint64_t n_records,
                                                                 uint32_t invert, uint32_t *__restrict__ cnt) {
    uint32_t w;
    const uint32_t rises = sl_rises(bitmap, (uint64_t)blockIdx.x * kSlRunThreads + threadIdx.x, n_records, invert, w);
    const uint32_t cr = wave_reduce_add((uint32_t)__popc(rises)), cs = wave_reduce_add((uint32_t)__popc(w));
    if (threadIdx.x == 0) {
        cnt[2u * (uint64_t)blockIdx.x] = cr;
        cnt[2u * (uint64_t)blockIdx.x + 1u] = cs;
    }
}

// One workgroup, kSlScanStep workgroups of k_sl_runs_count a step.  bases[x] = the rank of workgroup x's first rising
// edge.  The record: [kSlRecRuns], [kSlRecRecords], and [kSlRecHits] from find's record.  (Both sums stay below 2^32:
// R <= 0xFFFFFFF0.)
__global__ __launch_bounds__(kFdThreads) void k_sl_runs_scan(const uint32_t *__restrict__ cnt, uint32_t n_groups,
                                                             uint32_t *__restrict__ bases, const uint64_t *__restrict__ find_rec,
                                                             uint64_t *rec) {
    static_assert(kSlScanStep == kFdThreads, "a thread takes one workgroup's counts a step");
    __shared__ uint64_t wsum[4];
    uint64_t run = 0;  // rising edges << 32 | set bits; every thread keeps its own copy
    for (uint64_t base = 0; base < n_groups; base += kSlScanStep) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t mine = i < n_groups ? ((uint64_t)cnt[2u * i] << 32) | cnt[2u * i + 1u] : 0u;
        uint64_t step;
        const uint64_t ex = run + block_exclusive_scan256(mine, wsum, &step);
        run += step;
        if (i < n_groups) bases[i] = (uint32_t)(ex >> 32);
    }
    if (threadIdx.x == 0) {
        rec[kSlRecRuns] = run >> 32;
        rec[kSlRecRecords] = (uint32_t)run;
        rec[kSlRecHits] = find_rec[kFdRecHits];
    }
}

// Workgroup x writes the runs that begin or end in its records: runs[2 j] = begin, runs[2 j + 1] = end of run j < cap.
// A workgroup without a set bit is left at once.
__global__ __launch_bounds__(kSlRunThreads) void k_sl_runs_write(const uint8_t *__restrict__ bitmap, uint64_t n_records,
                                                                 uint32_t invert, const uint32_t *__restrict__ cnt,
                                                                 const uint32_t *__restrict__ bases, uint64_t g, uint64_t n_lines,
                                                                 uint64_t *__restrict__ runs, uint64_t cap) {
    if (cnt[2u * (uint64_t)blockIdx.x + 1u] == 0) return;  // (the whole workgroup)
    const uint64_t k = (uint64_t)blockIdx.x * kSlRunThreads + threadIdx.x;
    uint32_t w;
    const uint32_t rises = sl_rises(bitmap, k, n_records, invert, w);
    uint32_t behind = __shfl_down(w, 1);  // the neighbour lane's byte; the wave's last lane loads it
    if ((threadIdx.x & 63u) == 63u) behind = sl_byte(bitmap, k + 1u, n_records, invert);
    const uint32_t falls = w & ~((w >> 1) | ((behind & 1u) << 7));
    const uint32_t c = (uint32_t)__popc(rises);
    const uint64_t rank = (uint64_t)bases[blockIdx.x] + (wave_incl_add(c) - c);  // of the lane's first rising edge
    for (uint32_t e = rises; e; e &= e - 1u) {
        const uint32_t b = (uint32_t)__ffs((int)e) - 1u;
        const uint64_t j = rank + (uint32_t)__popc(rises & ((1u << b) - 1u));
        if (j < cap) runs[2u * j] = g * (8u * k + b);
    }
    for (uint32_t e = falls; e; e &= e - 1u) {
        const uint32_t b = (uint32_t)__ffs((int)e) - 1u;
        const uint64_t j = rank + (uint32_t)__popc(rises & ((2u << b) - 1u)) - 1u;  // (a rising edge lies at or in front of it)
        const uint64_t r = 8u * k + b;
        if (j < cap) runs[2u * j + 1u] = r + 1u == n_records ? n_lines : g * (r + 1u);
    }
}
