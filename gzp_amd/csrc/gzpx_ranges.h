// gzpx_ranges.h -- random access by range: a batch of byte ranges of the inflated stream, read from a BGZF / Mgzip
// stream in device memory through an index that lies there too (RrIndex: member offsets, member sizes, exclusive
// prefix sum of ISIZE).  Included from gzpx_kernels.hip behind gzpx_wave.h (block_exclusive_scan256).
//
//   1. locate   k_rr_locate: one lane per range.  Virtual offsets are resolved to uncompressed ones (exact-match
//               binary search on the member offsets), then `first` = the last member whose uncompressed start is
//               <= begin and `last` = the last one whose start is < end, by binary search on the prefix table: log2 n
//               loads, every range on its own (the pattern of k_mscan_succ).  The first invalid range is reduced
//               with atomicMin.  The members of [first, last] are marked in a DIFFERENCE array (+1 at first, -1 at
//               last + 1): two atomics per range whatever its span -- a range over the whole stream costs what a
//               4-byte one does, no lane and no workgroup loops over members -- and the prefix sum that turns it
//               into marks is one more column of the scan that select runs anyway.
//   2. select   k_rr_select, one workgroup: coverage = scan of the differences, rank = scan of (coverage != 0),
//               staging offset = scan of the selected members' ISIZE; the compaction writes the selected members'
//               offsets and sizes (the table launch_inflate takes) and the map rank -> stream index.  Then the scan
//               of the range lengths gives out_offsets, and every range learns where its bytes start in staging:
//               selected members that are neighbours in the stream are neighbours in staging, so a range is ONE
//               contiguous run there, at staging(first) + begin - ustart[first].  The record (kRrRec*) is all the
//               host reads before it enqueues the inflate.
//   3. inflate  launch_inflate, unchanged, over the compacted table into the context's staging buffer.
//   4. gather   k_rr_gather: the OUTPUT is cut into tiles of kRrTile bytes (ranges run from a few bytes to
//               gigabytes), a tile finds its ranges by binary search in out_offsets; stores are aligned 16-byte
//               stores, the source -- misaligned against them in general -- is read as aligned 16-byte words and
//               shifted into place (v_alignbyte); bytes only at the ragged ends of a range.
// No kernel's depth of dependent global loads grows with the number of members or ranges (log2 for the searches).

constexpr uint32_t kRrNone = 0xFFFFFFFFu;
constexpr uint32_t kRrThreads = 256;
constexpr uint32_t kRrTile = 16384;            // output bytes per gather workgroup: four 16-byte words per lane
constexpr uint32_t kRrTileWords = kRrTile / 16u;
constexpr uint32_t kRrItems = 4;               // members per thread and step of k_rr_select

// first index in [lo, hi) with a[i] >= v (GT = false) / a[i] > v (GT = true)
template <bool GT>
__device__ __forceinline__ uint32_t rr_bound(const uint64_t *__restrict__ a, uint32_t lo, uint32_t hi, uint64_t v) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint64_t x = a[mid];
        if (GT ? x <= v : x < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// a BGZF virtual offset as an offset into the inflated stream; false where it names no position of the index
__device__ __forceinline__ bool rr_virtual(const RrIndex &ix, uint64_t v, uint64_t *u) {
    const uint64_t start = v >> 16, within = v & 0xFFFFu;
    const uint32_t m = rr_bound<false>(ix.off, 0, ix.n, start);
    if (m >= ix.n || ix.off[m] != start) return false;
    const uint64_t u0 = ix.ustart[m];
    if (within > ix.ustart[m + 1] - u0) return false;  // (== ISIZE: the position in front of the next member)
    *u = u0 + within;
    return true;
}

__global__ __launch_bounds__(kRrThreads) void k_rr_locate(RrIndex ix, uint32_t n_ranges, const uint64_t *__restrict__ ranges,
                                                          uint32_t virt, uint32_t *__restrict__ first,
                                                          uint64_t *__restrict__ len, uint64_t *__restrict__ src,
                                                          uint32_t *diff, uint32_t *rec) {
    const uint32_t r = blockIdx.x * kRrThreads + threadIdx.x;
    if (r >= n_ranges) return;
    const uint64_t b = ranges[2 * (uint64_t)r], e = ranges[2 * (uint64_t)r + 1];
    uint64_t ub = b, ue = e;
    bool ok = b <= e;  // (virtual offsets compare as positions do: member start first, then the offset inside)
    if (virt) ok = ok && rr_virtual(ix, b, &ub) && rr_virtual(ix, e, &ue);
    else ok = ok && e <= ix.ustart[ix.n];
    uint32_t f = 0;
    uint64_t length = 0, skip = 0;
    if (!ok) {
        atomicMin(&rec[kRrRecBad], r);
    } else if (ue > ub) {
        length = ue - ub;
        f = rr_bound<true>(ix.ustart, 0, ix.n, ub) - 1u;  // (ustart[0] = 0 <= ub: at least 1)
        const uint32_t l = rr_bound<false>(ix.ustart, 0, ix.n, ue) - 1u;  // (ue > 0 likewise)
        skip = ub - ix.ustart[f];
        atomicAdd(&diff[f], 1u);
        atomicAdd(&diff[l + 1u], 0xFFFFFFFFu);  // (l + 1 <= n: diff has n + 1 words)
    }
    first[r] = f;
    len[r] = length;
    src[r] = skip;
}

// One workgroup.  sel_off / sel_size: the compacted member table; map[rank] = stream index; soff[i] = where selected
// member i starts in staging.  src[r] comes in as begin - ustart[first] and leaves as the range's offset in staging.
__global__ __launch_bounds__(kRrThreads) void k_rr_select(RrIndex ix, uint32_t n_ranges, const uint32_t *__restrict__ diff,
                                                          uint64_t *__restrict__ sel_off, uint32_t *__restrict__ sel_size,
                                                          uint32_t *__restrict__ map, uint64_t *soff,
                                                          const uint32_t *__restrict__ first, const uint64_t *__restrict__ len,
                                                          uint64_t *__restrict__ src, uint64_t *__restrict__ out_off,
                                                          uint32_t *__restrict__ rec) {
    __shared__ uint64_t wsum[4];
    const uint32_t tid = threadIdx.x;
    uint64_t c_cov = 0, c_cnt = 0, c_sz = 0;  // the carries: every thread keeps its own copy (the scans return the totals)
    for (uint64_t base = 0; base < ix.n; base += kRrThreads * kRrItems) {
        const uint64_t i0 = base + (uint64_t)tid * kRrItems;
        uint32_t d[kRrItems];
        uint64_t dsum = 0, total;
#pragma unroll
        for (uint32_t j = 0; j < kRrItems; j++) {
            d[j] = i0 + j < ix.n ? diff[i0 + j] : 0u;
            dsum += d[j];
        }
        uint64_t cov = c_cov + block_exclusive_scan256(dsum, wsum, &total);
        c_cov += total;
        uint64_t isz[kRrItems];
        uint64_t cnt = 0, sz = 0;
#pragma unroll
        for (uint32_t j = 0; j < kRrItems; j++) {
            cov += d[j];  // (the -1 arrive as 2^32 - 1: only the low word counts)
            const bool sel = i0 + j < ix.n && (uint32_t)cov != 0;
            isz[j] = sel ? ix.ustart[i0 + j + 1] - ix.ustart[i0 + j] : ~0ull;
            cnt += sel ? 1u : 0u;
            sz += sel ? isz[j] : 0u;
        }
        uint64_t rank = c_cnt + block_exclusive_scan256(cnt, wsum, &total);
        c_cnt += total;
        uint64_t so = c_sz + block_exclusive_scan256(sz, wsum, &total);
        c_sz += total;
#pragma unroll
        for (uint32_t j = 0; j < kRrItems; j++) {
            if (isz[j] == ~0ull) continue;
            sel_off[rank] = ix.off[i0 + j];
            sel_size[rank] = ix.size[i0 + j];
            map[rank] = (uint32_t)(i0 + j);
            soff[i0 + j] = so;
            rank++;
            so += isz[j];
        }
    }
    __syncthreads();  // soff is read below by other threads of this workgroup
    uint64_t c_out = 0;
    for (uint64_t base = 0; base < n_ranges; base += kRrThreads) {
        const uint64_t r = base + tid;
        const uint64_t length = r < n_ranges ? len[r] : 0u;
        uint64_t total;
        const uint64_t ex = c_out + block_exclusive_scan256(length, wsum, &total);
        c_out += total;
        if (r < n_ranges) {
            out_off[r] = ex;
            if (length) src[r] += soff[first[r]];
        }
    }
    if (tid == 0) {
        out_off[n_ranges] = c_out;
        rec[kRrRecSelected] = (uint32_t)c_cnt;
        rec[kRrRecStage] = (uint32_t)c_sz;
        rec[kRrRecStage + 1] = (uint32_t)(c_sz >> 32);
        rec[kRrRecTotal] = (uint32_t)c_out;
        rec[kRrRecTotal + 1] = (uint32_t)(c_out >> 32);
    }
}

// bytes [mis, mis + 16) of the 32 that a (low) and b (high) hold
template <uint32_t Q>
__device__ __forceinline__ uint4 rr_shift_q(const uint32_t (&w)[8], uint32_t sh) {
    return make_uint4(__builtin_amdgcn_alignbyte(w[Q + 1], w[Q], sh), __builtin_amdgcn_alignbyte(w[Q + 2], w[Q + 1], sh),
                      __builtin_amdgcn_alignbyte(w[Q + 3], w[Q + 2], sh), __builtin_amdgcn_alignbyte(w[Q + 4], w[Q + 3], sh));
}
__device__ __forceinline__ uint4 rr_shift(uint4 a, uint4 b, uint32_t mis) {
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t sh = mis & 3u;
    switch (mis >> 2) {  // (the same in every lane of a tile that lies inside one range)
    case 0: return rr_shift_q<0>(w, sh);
    case 1: return rr_shift_q<1>(w, sh);
    case 2: return rr_shift_q<2>(w, sh);
    default: return rr_shift_q<3>(w, sh);
    }
}

// Word k of the output is the 16 bytes at the aligned address (out - lead) + 16 k, output bytes [16 k - lead, ..+16).
// `stage` holds 16 readable bytes behind the last one a range uses (the second aligned word of the last shift).
__global__ __launch_bounds__(kRrThreads) void k_rr_gather(const uint8_t *__restrict__ stage, const uint64_t *__restrict__ src,
                                                          const uint64_t *__restrict__ out_off, uint32_t n_ranges,
                                                          uint8_t *__restrict__ out, uint32_t lead, uint64_t total) {
    const uint64_t k0 = (uint64_t)blockIdx.x * kRrTileWords;
    // the ranges the tile's first and last byte lie in (never empty ones: theirs is the next range's offset)
    const uint64_t tb = k0 * 16u > lead ? k0 * 16u - lead : 0u;
    uint64_t te = (k0 + kRrTileWords) * 16u - lead;
    if (te > total) te = total;
    if (tb >= te) return;
    const uint32_t r0 = rr_bound<true>(out_off + 1, 0, n_ranges, tb);
    const uint32_t r1 = rr_bound<true>(out_off + 1, r0, n_ranges, te - 1u);
    uint4 a[4], b[4];
    uint32_t rr[4], mis[4];
    bool whole[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
        const uint64_t k = k0 + u * kRrThreads + threadIdx.x;
        const uint64_t o = k * 16u - lead;  // (wraps for k = 0 with a lead: then not `whole`)
        whole[u] = k * 16u >= lead && o + 16u <= total;
        rr[u] = r0;
        mis[u] = 0;
        if (whole[u]) {
            if (r0 != r1) rr[u] = rr_bound<true>(out_off + 1, r0, r1, o);
            whole[u] = o + 16u <= out_off[rr[u] + 1u];
        }
        if (whole[u]) {  // aligned words of the source, several loads in flight per lane
            const uint8_t *sp = stage + src[rr[u]] + (o - out_off[rr[u]]);
            mis[u] = (uint32_t)((uintptr_t)sp & 15u);
            const uint4 *sa = (const uint4 *)(sp - mis[u]);
            a[u] = sa[0];
            b[u] = sa[1];
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
        const uint64_t k = k0 + u * kRrThreads + threadIdx.x;
        if (whole[u]) {
            *(uint4 *)(out + (k * 16u - lead)) = rr_shift(a[u], b[u], mis[u]);
            continue;
        }
        // a word that a range's end, the output's start or its end cuts: byte by byte
        const uint64_t p0 = k * 16u > lead ? k * 16u - lead : 0u;
        uint64_t p1 = (k + 1u) * 16u - lead;
        if (p1 > total) p1 = total;
        if (p0 >= p1) continue;
        uint32_t r = r0 != r1 ? rr_bound<true>(out_off + 1, r0, r1, p0) : r0;
        uint64_t r_begin = out_off[r], r_end = out_off[r + 1u], r_src = src[r];
        for (uint64_t p = p0; p < p1; p++) {
            if (p >= r_end) {  // (at most 16 steps: the word's bytes)
                r = rr_bound<true>(out_off + 1, r + 1u, r1, p);
                r_begin = out_off[r];
                r_end = out_off[r + 1u];
                r_src = src[r];
            }
            out[p] = stage[r_src + (p - r_begin)];
        }
    }
}
