// gzpx_findset.h -- WHERE any of a SET of byte strings occurs in a BGZF / Mgzip stream in device memory: every pair
// (position, pattern id) at which a pattern of the set starts, ascending by position and at one position by id, the
// line of each, and how often every pattern occurs; and WHICH lines hold a hit of any of them.  Included from
// gzpx_kernels.hip behind gzpx_select.h: staging, the region, its pieces (fd_piece), the walk frame with the marking
// pass, k_fd_scan, k_fd_carry and the run kernels of the selection are shared with the single-pattern search.
// (Definitions: include/gzpx.h.)
//
// The set arrives compiled by the host (FsSet, gzpx_device.h) and is staged into LDS once per workgroup.  With
// q = min(shortest pattern, 4), the WINDOW of a position is its first q bytes as a little-endian number.
//   filter   a bitmap of 2^16 bits, indexed by the window itself (q <= 2) or by a multiplicative hash of it (q = 3, 4):
//            the host sets the bit of every pattern's first q bytes.  A clear bit: no pattern starts here.  The 16
//            windows of an aligned word come from the word and the first dword behind it (fd_next: the neighbour
//            lane's), shifted out with alignbyte.  (A window of 4 bytes at byte 15 of a word ends at byte 18: the
//            second dword behind the word is never needed.)
//   bucket   survivors look their window up in the sorted distinct windows of the set (binary search, 8 steps at most)
//            and compare the patterns listed for it, ids ascending, a dword at a time: the pattern's dwords from LDS
//            (every pattern starts on a dword there), the stream's by two aligned loads and alignbyte.
//
// OWNERSHIP BY START.  The single-pattern search gives a batch the hits that END in it; with patterns of different
// lengths that breaks the order (a 1-byte hit would be written before a longer one that starts in front of it and ends
// in the next batch).  Here a batch that is not the last owns the starts p of its region with p + M <= the region's
// end, M the longest pattern, for every pattern alike; the carry is the last min(M - 1, bytes seen) bytes, whose starts
// wait for the next batch; the last batch owns every start that is left, each pattern clipped by its own length against
// the region's end.  FdArgs::m is therefore M for a batch that is not the last and 1 for the last, and fd_piece cuts
// the allowed starts as it does for one pattern.
//
//   k_fs_count  one workgroup per piece, k_fd_count's geometry: four aligned 16-byte loads in flight per lane, filter,
//               bucket, compare.  cnt[2 i] hits (of all patterns), cnt[2 i + 1] delimiters: k_fd_count's layout, so
//               k_fd_scan runs behind it as it is.  Hits per pattern in LDS counters, flushed with one 64-bit atomicAdd
//               per non-zero counter: only this pass counts them, so they are totals however the writing is clipped.
//   k_fs_write  k_fd_write's walk, written out: 256 lanes x one word a step, a block prefix of (hits << 32 |
//               delimiters); a lane with hits walks its word again and stores positions[r], ids[r], lines[r] for
//               r < cap.  Not on the walk frame: there it measured 1 % slower where millions of hits are written.
//   k_fs_mark   the marking pass (sl_mark, gzpx_select.h) with FsAny, the matcher whose hit mask is "some pattern of
//               the set starts here": the compare stops at the first match of a position.
// No kernel's depth of dependent global loads grows with the stream.

static_assert(kFdThreads == kFsMaxPatterns, "a thread clears and flushes one pattern's counter");
static_assert((uint64_t)kFdThreads * 16u * kFsMaxPatterns < (1ull << 32),
              "a step's hits (at most 256 lanes x 16 positions x 256 patterns = 2^20) fit the packed prefix's upper half");
static_assert(sizeof(FsSet) + 4u * kFsMaxPatterns + 64u <= 40u * 1024u, "several workgroups share a CU's LDS");

// the compiled set from device memory into LDS: the header and what it says is in use of every table
__device__ __forceinline__ void fs_load_set(const FsSet *__restrict__ g, FsSet &s) {
    const uint32_t tid = threadIdx.x;
    const uint32_t n_ids = g->hdr[kFsHdrK], n_grams = g->hdr[kFsHdrGrams];
    const uint32_t n_bitmap = g->hdr[kFsHdrBitmapWords] / 4u, n_bytes = (g->hdr[kFsHdrByteWords] + 3u) / 4u;
    if (tid < kFsHdrWords) s.hdr[tid] = g->hdr[tid];
    const uint4 *gb = (const uint4 *)g->bitmap, *gy = (const uint4 *)g->bytes;
    uint4 *sb = (uint4 *)s.bitmap, *sy = (uint4 *)s.bytes;
    for (uint32_t i = tid; i < n_bitmap; i += kFdThreads) sb[i] = gb[i];
    for (uint32_t i = tid; i < n_bytes; i += kFdThreads) sy[i] = gy[i];
    if (tid < n_grams) s.keys[tid] = g->keys[tid];
    for (uint32_t i = tid; i <= n_grams; i += kFdThreads) s.bstart[i] = g->bstart[i];  // (one more entry than windows)
    if (tid < n_ids) {
        s.ids[tid] = g->ids[tid];
        s.meta[tid] = g->meta[tid];
    }
    __syncthreads();
}

// bit b: byte b of the word at address p is an allowed start, p + b in [a0, ah)
__device__ __forceinline__ uint32_t fs_allowed(uintptr_t p, uintptr_t a0, uintptr_t ah) {
    if (p >= a0 && p + 16u <= ah) return 0xFFFFu;
    const uint32_t lo = p >= a0 ? 0u : (a0 - p >= 16u ? 16u : (uint32_t)(a0 - p));
    const uint32_t hi = p >= ah ? 0u : (ah - p >= 16u ? 16u : (uint32_t)(ah - p));
    if (lo >= hi) return 0u;
    return ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// bit b: the filter passes the window at byte b of the word v; `next`: the dword behind the word
__device__ __forceinline__ uint32_t fs_candidates(const FsSet &s, const uint4 &v, uint32_t next, uint32_t q, uint32_t qmask) {
    const uint32_t d[5] = {v.x, v.y, v.z, v.w, next};
    uint32_t c = 0;
#pragma unroll
    for (uint32_t b = 0; b < 16u; b++) {
        const uint32_t w = __builtin_amdgcn_alignbyte(d[b / 4u + 1u], d[b / 4u], b & 3u) & qmask;
        const uint32_t i = fs_gram_index(w, q);
        c |= ((s.bitmap[i >> 5] >> (i & 31u)) & 1u) << b;
    }
    return c;
}

// the m bytes at `at` against a pattern's dwords in LDS (the tail of its last dword is zero)
__device__ __forceinline__ bool fs_equal(const uint8_t *at, const uint32_t *pat, uint32_t m) {
    for (uint32_t j = 0; j < m; j += 4u) {
        uint32_t x = load_le32_global(at + j) ^ pat[j >> 2];  // (8 bytes from the aligned dword in front of at + j: readable)
        if (m - j < 4u) x &= (1u << (8u * (m - j))) - 1u;
        if (x) return false;
    }
    return true;
}

// The patterns that start at `at` (a survivor of the filter), ids ascending: emit(id) for each that ends at or in front
// of `end`, the region's end; kFirst: the first one only.
template <bool kFirst, class Emit>
__device__ __forceinline__ void fs_position(const FsSet &s, const uint8_t *at, uintptr_t end, uint32_t qmask, Emit &&emit) {
    const uint32_t w = load_le32_global(at) & qmask, n_grams = s.hdr[kFsHdrGrams];
    uint32_t lo = 0, hi = n_grams;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s.keys[mid] < w) lo = mid + 1u;
        else hi = mid;
    }
    if (lo == n_grams || s.keys[lo] != w) return;  // (the hash of another window)
    for (uint32_t j = s.bstart[lo], j1 = s.bstart[lo + 1u]; j < j1; j++) {
        const uint32_t id = s.ids[j], meta = s.meta[id], m = meta & 0xFFFFu;
        if ((uintptr_t)at + m > end || !fs_equal(at, &s.bytes[meta >> 16], m)) continue;
        emit(id);
        if (kFirst) return;
    }
}

// emit(b, id) for every hit (p + b, id) of the aligned word v read at address p whose start lies in [a0, ah), in
// ascending b and at one b in ascending id
template <bool kFirst, class Emit>
__device__ __forceinline__ void fs_word(const FsSet &s, const uint4 &v, uint32_t next, uintptr_t p, uintptr_t a0, uintptr_t ah,
                                        uintptr_t end, uint32_t q, uint32_t qmask, Emit &&emit) {
    for (uint32_t c = fs_candidates(s, v, next, q, qmask) & fs_allowed(p, a0, ah); c; c &= c - 1u) {
        const uint32_t b = (uint32_t)__ffs((int)c) - 1u;
        fs_position<kFirst>(s, (const uint8_t *)(p + b), end, qmask, [&](uint32_t id) { emit(b, id); });
    }
}

__device__ __forceinline__ uint32_t fs_qmask(uint32_t q) { return q >= 4u ? 0xFFFFFFFFu : (1u << (8u * q)) - 1u; }

// the matcher (gzpx_find.h) of "some pattern of the set starts here"
struct FsAny {
    using Src = FsSet;
    using Lds = FsSet;
    const FsSet &set;
    uintptr_t end;  // of the region
    uint32_t q, qmask;
    __device__ __forceinline__ FsAny(const FdArgs &a, const Src *__restrict__ d_set, Lds &lds) : set(lds), end((uintptr_t)a.stage + a.r1) {
        fs_load_set(d_set, lds);
        q = set.hdr[kFsHdrQ], qmask = fs_qmask(q);
    }
    __device__ __forceinline__ uint32_t hits(const uint4 &v, uint32_t next, uintptr_t p, uintptr_t a0, uintptr_t ah) const {
        uint32_t h = 0;
        fs_word<true>(set, v, next, p, a0, ah, end, q, qmask, [&](uint32_t b, uint32_t) { h |= 1u << b; });
        return h;
    }
};

// Workgroup i counts piece x0 + i: cnt[2 i] hits, cnt[2 i + 1] delimiters; counts[k] += the hits of pattern k.
__global__ __launch_bounds__(kFdThreads) void k_fs_count(FdArgs a, uint32_t x0, const FsSet *__restrict__ d_set,
                                                         uint32_t *__restrict__ cnt, unsigned long long *counts) {
    __shared__ FsSet set;
    __shared__ uint32_t per[kFsMaxPatterns];
    __shared__ uint32_t wsum[2u * (kFdThreads / 64u)];
    const uint32_t tid = threadIdx.x;
    per[tid] = 0;
    fs_load_set(d_set, set);
    const uint32_t q = set.hdr[kFsHdrQ], qmask = fs_qmask(q);
    uintptr_t a0, a1, ah;
    fd_piece(a, x0 + blockIdx.x, a0, a1, ah);
    const uintptr_t end = (uintptr_t)a.stage + a.r1;
    const uintptr_t w0 = a0 & ~(uintptr_t)15;
    const uint32_t n_words = (uint32_t)((a1 - w0 + 15u) / 16u);  // (at most kFdItems * kFdThreads: a piece starts on a word)
    const uint32_t sd = a.delim * 0x01010101u;
    uint4 v[kFdItems];
#pragma unroll
    for (uint32_t u = 0; u < kFdItems; u++) {  // aligned words of staging, several loads in flight per lane
        const uint32_t k = u * kFdThreads + tid;
        v[u] = make_uint4(0, 0, 0, 0);
        if (k < n_words) v[u] = *(const uint4 *)(w0 + 16u * (uintptr_t)k);
    }
    uint32_t ch = 0, cd = 0;
#pragma unroll
    for (uint32_t u = 0; u < kFdItems; u++) {
        const uint32_t k = u * kFdThreads + tid;
        const uintptr_t p = w0 + 16u * (uintptr_t)k;
        const uint32_t next = fd_next(v[u], p, a1);
        if (k >= n_words) continue;
        fs_word<false>(set, v[u], next, p, a0, ah, end, q, qmask, [&](uint32_t, uint32_t id) {
            ch++;
            atomicAdd(&per[id], 1u);
        });
        if (a.lines) {
            uint32_t d[4];
            ln_word(v[u], sd, p, a0, a1, d);
            cd += (uint32_t)(__popc(d[0]) + __popc(d[1]) + __popc(d[2]) + __popc(d[3]));
        }
    }
    ch = wave_reduce_add(ch);
    cd = wave_reduce_add(cd);
    if ((tid & 63u) == 0) {
        wsum[2u * (tid >> 6)] = ch;
        wsum[2u * (tid >> 6) + 1u] = cd;
    }
    __syncthreads();  // (the counters of every lane are in, too)
    if (tid < 2u) {
        uint32_t s = 0;
        for (uint32_t w = 0; w < kFdThreads / 64u; w++) s += wsum[2u * w + tid];
        cnt[2u * (uint64_t)blockIdx.x + tid] = s;
    }
    if (tid < set.hdr[kFsHdrK] && per[tid]) atomicAdd(&counts[tid], (unsigned long long)per[tid]);
}

// Workgroup i writes the hits of piece x0 + i: positions[r], ids[r] and lines[r] for the ranks r < cap (each array may
// be absent).  A piece without a hit, or whose first rank is not below cap, is left at once.
__global__ __launch_bounds__(kFdThreads) void k_fs_write(FdArgs a, uint32_t x0, const FsSet *__restrict__ d_set,
                                                         const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ bases,
                                                         uint64_t *__restrict__ positions, uint32_t *__restrict__ ids,
                                                         uint64_t *__restrict__ lines, uint64_t cap) {
    __shared__ FsSet set;
    __shared__ uint64_t wsum[4];
    const uint32_t tid = threadIdx.x;
    uint64_t rank = bases[2u * (uint64_t)blockIdx.x], line = bases[2u * (uint64_t)blockIdx.x + 1u];
    if (cnt[2u * (uint64_t)blockIdx.x] == 0 || rank >= cap) return;  // (the whole workgroup)
    fs_load_set(d_set, set);
    const uint32_t q = set.hdr[kFsHdrQ], qmask = fs_qmask(q);
    uintptr_t a0, a1, ah;
    fd_piece(a, x0 + blockIdx.x, a0, a1, ah);
    const uintptr_t end = (uintptr_t)a.stage + a.r1;
    const uint32_t sd = a.delim * 0x01010101u;
    for (uintptr_t row = a0 & ~(uintptr_t)15; row < a1 && rank < cap; row += 16u * kFdThreads) {  // (the same in every lane)
        const uintptr_t p = row + 16u * tid;
        uint32_t nh = 0, dm = 0;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p < a1) v = *(const uint4 *)p;
        const uint32_t next = fd_next(v, p, a1);
        if (p < a1) {
            fs_word<false>(set, v, next, p, a0, ah, end, q, qmask, [&](uint32_t, uint32_t) { nh++; });
            if (lines) {
                uint32_t d[4];
                ln_word(v, sd, p, a0, a1, d);
                dm = fd_mask16(d);
            }
        }
        const uint64_t mine = ((uint64_t)nh << 32) | (uint32_t)__popc(dm);  // (2^20 hits and 4096 delimiters a step at most)
        uint64_t step;
        const uint64_t ex = block_exclusive_scan256(mine, wsum, &step);
        uint64_t r = rank + (ex >> 32);
        const uint64_t l = line + (uint32_t)ex;
        if (nh && r < cap)  // the word again, now that the rank of its first hit is known
            fs_word<false>(set, v, next, p, a0, ah, end, q, qmask, [&](uint32_t b, uint32_t id) {
                if (r < cap) {
                    // (a start in the carry lies in front of staging[kFdPad]: the sum stays >= 0, carry <= base)
                    if (positions) positions[r] = a.base + (uint64_t)(p + b - (uintptr_t)a.stage) - kFdPad;
                    if (ids) ids[r] = id;
                    if (lines) lines[r] = l + (uint32_t)__popc(dm & ((1u << b) - 1u));
                }
                r++;
            });
        rank += step >> 32;
        line += (uint32_t)step;
    }
}

// Workgroup i marks the records of the hits of piece x0 + i.
__global__ __launch_bounds__(kFdThreads) void k_fs_mark(FdArgs a, uint32_t x0, const FsSet *__restrict__ d_set,
                                                        const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ bases,
                                                        uint32_t *bitmap, uint64_t g, uint64_t n_records) {
    __shared__ FsSet set;
    __shared__ uint64_t wsum[4];
    sl_mark<FsAny>(a, x0, d_set, set, wsum, cnt, bases, bitmap, g, n_records);
}
