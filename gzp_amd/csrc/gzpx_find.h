// gzpx_find.h -- WHERE a byte string occurs in a BGZF / Mgzip stream in device memory: every position of the inflated
// stream at which the pattern starts, ascending, and the line each of them lies in.  Included from gzpx_kernels.hip
// behind gzpx_lines.h, whose exact equal-byte test (ln_marks, ln_word) marks the candidates and the delimiters.
// (Definitions: include/gzpx.h.)
//
// Staging holds, behind every batch of the inflate, a front pad of kFdPad bytes and then the batch's `len` bytes; the
// last `carry` <= m - 1 bytes of what the earlier batches held stand at the end of the pad.  The REGION of a batch is
// [kFdPad - carry, kFdPad + len) of staging; a start is allowed where the pattern ends inside the region, so a batch
// finds the hits whose LAST byte lies in it.  The region is cut on the 16 KiB grid of staging into PIECES.
//
// The writing pass of one pattern and the marking passes of the selection (gzpx_select.h: one pattern, a set) walk a
// piece on one frame; their __global__ kernels declare the LDS and name the matcher.
//   fd_walk     the WALK FRAME: 256 lanes x one aligned 16-byte word a step, so that lane order is byte order; the dword
//               behind a word comes from the neighbour lane (fd_next); hits from the matcher, delimiters with ln_word; a
//               block prefix of (hits << 32 | delimiters) in one 64-bit value; act(rank, address, line) per hit.  Three
//               things are decided here, once, for every kernel on the walk:
//                 - a ranked walk (the writing) ends with the row that reaches `cap`: no later row holds a hit below it;
//                 - an unranked walk (the marking) carries no hits in the prefix: it reads only the lines;
//                 - "delimiters wanted" is one argument: the writing pass wants them iff it stores lines, the marking
//                   always.
// A MATCHER is what one pattern and a set differ in on the walk: Src (what lies in device memory), Lds (what the kernel
// declares __shared__; the constructor loads it and ends in a barrier), and
//   hits(v, next, p, a0, ah)  bit b: a hit starts at byte b of the aligned word v read at p, for the starts in [a0, ah).
// FdPattern is the matcher of one pattern (fd_hits): its first three bytes are tested on the marks, the rest is compared
// byte by byte with the pattern in LDS (up to m - 1 bytes behind the piece).  FsAny (gzpx_findset.h) is the set's.
//
//   k_fd_count  one workgroup per piece: its bytes once as aligned 16-byte words, kFdItems loads in flight per lane;
//               hits with fd_hits, delimiters with ln_word when lines are asked for; a wave reduction.  cnt[2 i] hits,
//               cnt[2 i + 1] delimiters of piece x0 + i.  (k_fs_count, gzpx_findset.h, has this geometry with the
//               set's test and counters per pattern; a frame shared by the two measured 0.5 % slower for the set.)
//   k_fd_scan   one workgroup: the counts -> where every piece's hits go and how many delimiters lie in front of it,
//               the totals of the earlier batches (the record) added; the record moves on.
//   k_fd_write  the writing pass on the walk with FdPattern: positions and lines of the ranks below hits_cap.
//   k_fd_carry  one workgroup: the region's last min(m - 1, bytes seen) bytes go to the end of the pad (a batch
//               shorter than m - 1 bytes thereby appends), and their delimiters are counted: the next batch's pieces
//               count them again, so its scan starts that many lower.
// No kernel's depth of dependent global loads grows with the stream.

constexpr uint32_t kFdThreads = 256;
constexpr uint32_t kFdItems = kFdPiece / (16u * kFdThreads);  // 16-byte words per lane of a piece
constexpr uint32_t kFdScanItems = 16;                          // pieces per thread and step of k_fd_scan
static_assert(kFdItems * kFdThreads * 16u == kFdPiece, "a piece is a whole number of steps");
static_assert(kFdPad % 16u == 0 && kFdPad >= kFdMaxPattern && kFdMaxPattern <= kFdThreads, "the carry fits the pad and one workgroup");

// bit i: byte i of the dword is marked
__device__ __forceinline__ uint32_t fd_nibble(uint32_t marks) {
    return ((marks >> 7) & 1u) | ((marks >> 14) & 2u) | ((marks >> 21) & 4u) | ((marks >> 28) & 8u);
}

__device__ __forceinline__ uint32_t fd_mask16(const uint32_t (&m)[4]) {
    return fd_nibble(m[0]) | (fd_nibble(m[1]) << 4) | (fd_nibble(m[2]) << 8) | (fd_nibble(m[3]) << 12);
}

// what the kernels share of a call
struct FdArgs {
    const uint8_t *stage;  // staging: pad, then the batch
    uint64_t r0, r1;       // the region, in bytes of staging
    uint64_t base;         // the stream position of staging[kFdPad]
    uint32_t m;            // bytes of pattern
    uint32_t lines;        // 1: delimiters are counted
    uint32_t delim;
};

// the pattern from device memory into LDS (kFdMaxPattern bytes, the tail zero)
__device__ __forceinline__ void fd_load_pattern(const uint32_t *__restrict__ d_pat, uint32_t *pat) {
    if (threadIdx.x < kFdMaxPattern / 4u) pat[threadIdx.x] = d_pat[threadIdx.x];
    __syncthreads();
}

// The first dword of the word behind the lane's word v (read at address p < a1, the piece's end): the neighbour lane's;
// a wave's last lane and the lane of the piece's last word, whose neighbour holds none, load it (20 readable bytes lie
// behind every word of a region).  Every lane of the wave calls it.
__device__ __forceinline__ uint32_t fd_next(const uint4 &v, uintptr_t p, uintptr_t a1) {
    uint32_t next = __shfl_down(v.x, 1);
    if (p < a1 && ((threadIdx.x & 63u) == 63u || p + 16u >= a1)) next = *(const uint32_t *)(p + 16u);
    return next;
}

// bit b: the pattern starts at byte b of the aligned word v read at address p, for the starts that lie in [a0, ah).
// s0 / s1 / s2: the splats of the pattern's first three bytes; `next`: the dword behind the word.  The first three bytes
// are tested on the marks; the rest of the pattern byte by byte.
__device__ __forceinline__ uint32_t fd_hits(const uint4 &v, uint32_t next, uintptr_t p, uintptr_t a0, uintptr_t ah, uint32_t s0,
                                            uint32_t s1, uint32_t s2, uint32_t m, const uint8_t *pat) {
    uint32_t f[4];
    ln_word(v, s0, p, a0, ah, f);
    if (m == 1u) return fd_mask16(f);
    const uint32_t g0 = ln_marks(v.x, s1), g1 = ln_marks(v.y, s1), g2 = ln_marks(v.z, s1), g3 = ln_marks(v.w, s1);
    f[0] &= (g0 >> 8) | (g1 << 24);
    f[1] &= (g1 >> 8) | (g2 << 24);
    f[2] &= (g2 >> 8) | (g3 << 24);
    f[3] &= (g3 >> 8) | (ln_marks(next, s1) << 24);
    if (m == 2u) return fd_mask16(f);
    const uint32_t h0 = ln_marks(v.x, s2), h1 = ln_marks(v.y, s2), h2 = ln_marks(v.z, s2), h3 = ln_marks(v.w, s2);
    f[0] &= (h0 >> 16) | (h1 << 16);
    f[1] &= (h1 >> 16) | (h2 << 16);
    f[2] &= (h2 >> 16) | (h3 << 16);
    f[3] &= (h3 >> 16) | (ln_marks(next, s2) << 16);
    uint32_t c = fd_mask16(f);
    if (m == 3u) return c;
    uint32_t hits = 0;
    for (; c; c &= c - 1u) {
        const uint32_t b = (uint32_t)__ffs((int)c) - 1u;
        const uint8_t *s = (const uint8_t *)(p + b);  // (s + m <= the region's end)
        uint32_t j = 3;
        while (j < m && s[j] == pat[j]) j++;
        if (j == m) hits |= 1u << b;
    }
    return hits;
}

// the bounds of piece x inside the region: bytes [a0, a1), allowed starts [a0, ah)
__device__ __forceinline__ void fd_piece(const FdArgs &a, uint32_t x, uintptr_t &a0, uintptr_t &a1, uintptr_t &ah) {
    uint64_t b = (uint64_t)x * kFdPiece, e = b + kFdPiece;
    if (b < a.r0) b = a.r0;
    if (e > a.r1) e = a.r1;  // (b < e: the grid covers the region and no more)
    const uint64_t h = a.r1 + 1u - a.m;  // the first start whose pattern would leave the region (r1 >= kFdPad >= m)
    a0 = (uintptr_t)a.stage + b;
    a1 = (uintptr_t)a.stage + e;
    ah = (uintptr_t)a.stage + (h < e ? h : e);
}

// f(b) for every set bit b of a 16-bit mask, ascending
template <class F>
__device__ __forceinline__ void fd_each_bit(uint32_t mask, F &&f) {
    for (uint32_t c = mask; c; c &= c - 1u) f((uint32_t)__ffs((int)c) - 1u);
}

// the matcher of one pattern
struct FdPattern {
    using Src = uint32_t;                      // the pattern in device memory, kFdMaxPattern bytes
    using Lds = uint32_t[kFdMaxPattern / 4u];
    const uint8_t *pat;
    uint32_t s0, s1, s2, m;  // the splats of the first three bytes
    __device__ __forceinline__ FdPattern(const FdArgs &a, const Src *__restrict__ d_pat, Lds &lds) : pat((const uint8_t *)lds), m(a.m) {
        fd_load_pattern(d_pat, lds);
        s0 = pat[0] * 0x01010101u, s1 = pat[1] * 0x01010101u, s2 = pat[2] * 0x01010101u;
    }
    __device__ __forceinline__ uint32_t hits(const uint4 &v, uint32_t next, uintptr_t p, uintptr_t a0, uintptr_t ah) const {
        return fd_hits(v, next, p, a0, ah, s0, s1, s2, m, pat);
    }
};

// THE WALK FRAME.  The workgroup walks piece x, which lies behind `line` delimiters of the stream (counted iff
// `delims`): act(rank, address in staging, line) for every hit, ascending inside the lane and in no order between
// lanes.  kRanked: the piece's first hit has rank `rank`, the prefix carries the hits, and the walk ends with the row
// that reaches `cap`; the ranks at and above cap in a word whose first hit lies below it are the action's to drop.
// Not kRanked: the prefix carries the delimiters alone, rank and cap are not read and act's rank means nothing.
template <bool kRanked, class M, class Act>
__device__ __forceinline__ void fd_walk(const FdArgs &a, uint32_t x, const M &mt, bool delims, uint64_t rank, uint64_t line,
                                        uint64_t cap, uint64_t (&wsum)[4], Act &&act) {
    uintptr_t a0, a1, ah;
    fd_piece(a, x, a0, a1, ah);
    const uint32_t sd = a.delim * 0x01010101u;
    for (uintptr_t row = a0 & ~(uintptr_t)15; row < a1 && (!kRanked || rank < cap); row += 16u * kFdThreads) {  // (the same in every lane)
        const uintptr_t p = row + 16u * threadIdx.x;
        uint32_t h = 0, dm = 0;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p < a1) v = *(const uint4 *)p;
        const uint32_t next = fd_next(v, p, a1);
        if (p < a1) {
            h = mt.hits(v, next, p, a0, ah);
            if (delims) {
                uint32_t d[4];
                ln_word(v, sd, p, a0, a1, d);
                dm = fd_mask16(d);
            }
        }
        // (2^20 hits and 4096 delimiters a step at most)
        const uint64_t mine = (kRanked ? (uint64_t)__popc(h) << 32 : 0u) | (uint32_t)__popc(dm);
        uint64_t step;
        const uint64_t ex = block_exclusive_scan256(mine, wsum, &step);
        uint64_t r = rank + (ex >> 32);
        const uint64_t l = line + (uint32_t)ex;
        if (h && (!kRanked || r < cap))
            fd_each_bit(h, [&](uint32_t b) { act(r++, p + b, l + (uint32_t)__popc(dm & ((1u << b) - 1u))); });
        if (kRanked) rank += step >> 32;
        line += (uint32_t)step;
    }
}

// Workgroup i counts piece x0 + i: cnt[2 i] hits, cnt[2 i + 1] delimiters.
__global__ __launch_bounds__(kFdThreads) void k_fd_count(FdArgs a, uint32_t x0, const uint32_t *__restrict__ d_pat,
                                                         uint32_t *__restrict__ cnt) {
    __shared__ uint32_t pat[kFdMaxPattern / 4u];
    __shared__ uint32_t wsum[2u * (kFdThreads / 64u)];
    const uint32_t tid = threadIdx.x;
    fd_load_pattern(d_pat, pat);
    const uint8_t *pb = (const uint8_t *)pat;
    uintptr_t a0, a1, ah;
    fd_piece(a, x0 + blockIdx.x, a0, a1, ah);
    const uintptr_t w0 = a0 & ~(uintptr_t)15;
    const uint32_t n_words = (uint32_t)((a1 - w0 + 15u) / 16u);  // (at most kFdItems * kFdThreads: a piece starts on a word)
    const uint32_t s0 = pb[0] * 0x01010101u, s1 = pb[1] * 0x01010101u, s2 = pb[2] * 0x01010101u, sd = a.delim * 0x01010101u;
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
        ch += (uint32_t)__popc(fd_hits(v[u], next, p, a0, ah, s0, s1, s2, a.m, pb));
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
    __syncthreads();
    if (tid < 2u) {
        uint32_t s = 0;
        for (uint32_t w = 0; w < kFdThreads / 64u; w++) s += wsum[2u * w + tid];
        cnt[2u * (uint64_t)blockIdx.x + tid] = s;
    }
}

// One workgroup.  bases[2 i] = the rank of piece i's first hit in the stream, bases[2 i + 1] = the delimiters of the
// stream in front of piece i.  The record: [kFdRecHits] hits so far, [kFdRecDelims] delimiters so far, [kFdRecCarry] those of
// them that lie in the carry and are counted again by this batch's pieces.
__global__ __launch_bounds__(kFdThreads) void k_fd_scan(const uint32_t *__restrict__ cnt, uint32_t n_pieces,
                                                        uint64_t *__restrict__ bases, uint64_t *rec) {
    __shared__ uint64_t wsum[4];
    const uint32_t tid = threadIdx.x;
    uint64_t run_h = rec[kFdRecHits], run_d = rec[kFdRecDelims] - rec[kFdRecCarry];  // every thread keeps its own copy
    for (uint64_t i_base = 0; i_base < n_pieces; i_base += kFdThreads * kFdScanItems) {
        const uint64_t i0 = i_base + (uint64_t)tid * kFdScanItems;
        uint32_t h[kFdScanItems], d[kFdScanItems];
        uint64_t sum_h = 0, sum_d = 0, step;
#pragma unroll
        for (uint32_t j = 0; j < kFdScanItems; j++) {
            h[j] = i0 + j < n_pieces ? cnt[2u * (i0 + j)] : 0u;
            d[j] = i0 + j < n_pieces ? cnt[2u * (i0 + j) + 1u] : 0u;
            sum_h += h[j];
            sum_d += d[j];
        }
        uint64_t ex_h = run_h + block_exclusive_scan256(sum_h, wsum, &step);
        run_h += step;
        uint64_t ex_d = run_d + block_exclusive_scan256(sum_d, wsum, &step);
        run_d += step;
#pragma unroll
        for (uint32_t j = 0; j < kFdScanItems; j++) {
            if (i0 + j < n_pieces) {
                bases[2u * (i0 + j)] = ex_h;
                bases[2u * (i0 + j) + 1u] = ex_d;
            }
            ex_h += h[j];
            ex_d += d[j];
        }
    }
    __syncthreads();  // (every thread has read the record)
    if (tid == 0) {
        rec[kFdRecHits] = run_h;
        rec[kFdRecDelims] = run_d;
        rec[kFdRecCarry] = 0;
    }
}

// Workgroup i writes the hits of piece x0 + i: positions[r] and lines[r] for the ranks r < cap (either array may be
// absent).  A piece without a hit, or whose first rank is not below cap, is left at once, the pattern unloaded.
__global__ __launch_bounds__(kFdThreads) void k_fd_write(FdArgs a, uint32_t x0, const uint32_t *__restrict__ d_pat,
                                                         const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ bases,
                                                         uint64_t *__restrict__ positions, uint64_t *__restrict__ lines,
                                                         uint64_t cap) {
    __shared__ FdPattern::Lds pat;
    __shared__ uint64_t wsum[4];
    const uint64_t rank = bases[2u * (uint64_t)blockIdx.x], line = bases[2u * (uint64_t)blockIdx.x + 1u];
    if (cnt[2u * (uint64_t)blockIdx.x] == 0 || rank >= cap) return;  // (the whole workgroup)
    const FdPattern mt(a, d_pat, pat);
    fd_walk<true>(a, x0 + blockIdx.x, mt, lines != nullptr, rank, line, cap, wsum, [&](uint64_t r, uintptr_t at, uint64_t l) {
        if (r >= cap) return;
        // (a start in the carry lies in front of staging[kFdPad]: the sum stays >= 0, carry <= base)
        if (positions) positions[r] = a.base + (uint64_t)(at - (uintptr_t)a.stage) - kFdPad;
        if (lines) lines[r] = l;
    });
}

// One workgroup, one byte a thread: staging[src + t] -> staging[kFdPad - n + t] for t < n (the two may overlap: every
// byte is read in front of the barrier), and the delimiters among them into the record.
__global__ __launch_bounds__(kFdThreads) void k_fd_carry(uint8_t *stage, uint64_t src, uint32_t n, uint32_t lines, uint32_t delim,
                                                         uint64_t *rec) {
    __shared__ uint32_t wsum[kFdThreads / 64u];
    const uint32_t tid = threadIdx.x;
    uint32_t byte = 0x100u;
    if (tid < n) byte = stage[src + tid];
    __syncthreads();
    if (tid < n) stage[kFdPad - n + tid] = (uint8_t)byte;
    if (!lines) return;  // (the whole workgroup)
    const uint32_t c = wave_reduce_add(byte == delim ? 1u : 0u);
    if ((tid & 63u) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0;
        for (uint32_t w = 0; w < kFdThreads / 64u; w++) s += wsum[w];
        rec[kFdRecCarry] = s;
    }
}
