// gzpx_mscan.h -- member discovery on the device: the table gzpx_scan_blocks (the reader thread's header walk,
// src/par/decompress.rs:132-160) would produce for a BGZF / Mgzip stream that lies in device memory.  Included from
// gzpx_kernels.hip behind gzpx_wave.h (block_exclusive_scan256, load_le32_global).
//
// The walk is a chain of dependent loads (a member's size says where the next header is), so nothing here follows it.
//   1. candidates   k_mscan_cand<false> / k_mscan_offsets / k_mscan_cand<true>: every position whose header passes the walk's
//                   checks (FEXTRA flag, SID bytes, size >= header + footer) is a candidate, real member or not.  A
//                   wave owns one segment of the stream, reads it in 16-byte words and looks for the two SID bytes; the
//                   rest of a header is only read where they match.  Count, exclusive scan, write: the candidate
//                   arrays come out sorted by position.  The write pass rereads only segments that hold candidates.
//   2. successor    k_mscan_succ: where the walk goes from candidate c, pos + size, resolved by binary search to a
//                   candidate index, or to a terminal: kMsStop (fewer than a header's bytes left there, or a member that
//                   is cut short) or kMsErr (a header the walk rejects).
//   3. chain from 0 k_mscan_jump, one launch per round r: jump[c] becomes the 2^(r+1)-th successor (pointer doubling),
//                   and every candidate already known to be member i < 2^r of the walk marks its 2^r-th successor as
//                   member i + 2^r.  After ceil(log2 n) rounds idx[c] is c's index in the walk, or kMsNone for the
//                   impostors: they were looked up, never trusted.
//   4. record       k_mscan_finish: the member whose successor is a terminal gives the count, the kind of end and
//                   `consumed`; k_mscan_emit writes offsets[idx[c]] / sizes[idx[c]] wherever the caller wants them.
// No kernel's depth of dependent global loads grows with the number of members: log2 n for the binary search, one
// round trip per launch otherwise.

constexpr uint32_t kMsStop = 0xFFFFFFFFu;  // terminals of the successor function (anything below kMsErr is a candidate)
constexpr uint32_t kMsErr = 0xFFFFFFFEu;
constexpr uint32_t kMsNone = 0xFFFFFFFFu;  // idx: not on the walk from offset 0
constexpr uint32_t kMsThreads = 256;
// the scan record (MemberScanScratch.rec, u32 words): [0] candidates found (above cap: nothing else is valid),
// [1] members of the walk, [2] how it ended (0 stop, 1 invalid header), [4..5] consumed
enum { kMsRecCand = 0, kMsRecMembers = 1, kMsRecKind = 2, kMsRecConsumed = 4 };

struct MsStream {
    const uint8_t *in;  // the stream
    uint64_t len;
    uint32_t lead;      // in & 15: word k holds stream bytes [16 k - lead, 16 k - lead + 16)
    uint32_t hdr;       // 18 BGZF, 20 Mgzip
    uint32_t sid;       // the SID bytes at 12..13 as a little-endian u16
    uint32_t seg_words; // 16-byte words per segment (a multiple of 256: four words per lane and step)
};

// stream byte at offset o, 0 outside the stream (zeros never look like SID bytes)
__device__ __forceinline__ uint32_t ms_byte(const MsStream &s, int64_t o) {
    return o >= 0 && (uint64_t)o < s.len ? s.in[o] : 0u;
}

__device__ __forceinline__ uint4 ms_load16(const MsStream &s, uint64_t k) {
    const int64_t o = (int64_t)(k * 16u) - (int64_t)s.lead;
    if (o >= 0 && (uint64_t)o + 16u <= s.len) return *(const uint4 *)(s.in + o);  // (16-byte aligned: in - lead is)
    uint32_t w[4];
    for (int j = 0; j < 4; j++)
        w[j] = ms_byte(s, o + 4 * j) | (ms_byte(s, o + 4 * j + 1) << 8) | (ms_byte(s, o + 4 * j + 2) << 16) |
               (ms_byte(s, o + 4 * j + 3) << 24);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the member size a header states (get_block_size, src/lib.rs:420-437), 0 where the header fails check_header or
// the size rule -- the checks of gzpx_scan_blocks, no more.  p + hdr <= len.
__device__ __forceinline__ uint32_t ms_header_size(const MsStream &s, uint64_t p) {
    const uint8_t *h = s.in + p;
    if ((h[3] & 4u) == 0 || ((uint32_t)h[12] | ((uint32_t)h[13] << 8)) != s.sid) return 0;
    const uint32_t size = s.hdr == 18 ? ((uint32_t)h[16] | ((uint32_t)h[17] << 8)) + 1u
                                      : (uint32_t)h[16] | ((uint32_t)h[17] << 8) | ((uint32_t)h[18] << 16) | ((uint32_t)h[19] << 24);
    return size >= s.hdr + 8u ? size : 0u;
}

// Word k of the stream: bit i of the result = a candidate's SID bytes start at byte i of the word.  `next` is the
// first byte behind the word.  Both passes call this, so they agree on every candidate.
__device__ __forceinline__ uint32_t ms_word_mask(const MsStream &s, uint64_t k, uint4 w, uint32_t next) {
    const uint32_t d[5] = {w.x, w.y, w.z, w.w, next};
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t v = (uint64_t)d[j] | ((uint64_t)(d[j + 1] & 0xFFu) << 32);
#pragma unroll
        for (int i = 0; i < 4; i++)
            if ((uint32_t)((v >> (8 * i)) & 0xFFFFu) == s.sid) m |= 1u << (4 * j + i);
    }
    if (m == 0) return 0;
    uint32_t keep = 0;  // (rare: about one word in 4,000 of compressed data gets here)
    for (uint32_t t = m; t; t &= t - 1) {
        const uint32_t i = (uint32_t)__ffs((int)t) - 1u;
        const int64_t p = (int64_t)(k * 16u) + i - (int64_t)s.lead - 12;
        if (p < 0 || (uint64_t)p + s.hdr > s.len) continue;
        if (ms_header_size(s, (uint64_t)p)) keep |= 1u << i;
    }
    return keep;
}

// One wave per segment.  WRITE = false: seg_count[segment] = its candidates.  WRITE = true: their positions and
// sizes at seg_off[segment].., in stream order.
template <bool WRITE>
__global__ __launch_bounds__(kMsThreads) void k_mscan_cand(MsStream s, uint32_t n_seg, uint32_t *__restrict__ seg_count,
                                                           const uint32_t *__restrict__ seg_off,
                                                           const uint32_t *__restrict__ rec, uint32_t cap,
                                                           uint64_t *__restrict__ pos, uint32_t *__restrict__ size) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t seg = blockIdx.x * (kMsThreads / 64u) + (threadIdx.x >> 6);
    if (seg >= n_seg) return;
    uint32_t base = 0;
    if (WRITE) {
        if (rec[kMsRecCand] > cap || seg_count[seg] == 0) return;  // (wave-uniform)
        base = seg_off[seg];
    }
    const uint64_t k0 = (uint64_t)seg * s.seg_words;
    const uint64_t k_end = (s.lead + s.len + 15u) >> 4;  // words that hold stream bytes
    uint32_t cnt = 0;
    for (uint32_t it = 0; it < s.seg_words; it += 256) {
        if (k0 + it >= k_end) break;
        uint4 w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) w[u] = ms_load16(s, k0 + it + 64u * u + lane);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint64_t k = k0 + it + 64u * u + lane;
            uint32_t next = __shfl_down(w[u].x, 1);
            if (lane == 63) next = ms_byte(s, (int64_t)((k + 1) * 16u) - (int64_t)s.lead);
            const uint32_t m = ms_word_mask(s, k, w[u], next & 0xFFu);
            if (!WRITE) {
                cnt += (uint32_t)__popc(m);
            } else if (__ballot(m != 0)) {  // (wave-uniform)
                const uint32_t mine = (uint32_t)__popc(m);
                uint32_t inc = mine;
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t t = __shfl_up(inc, d);
                    if (lane >= (uint32_t)d) inc += t;
                }
                uint32_t o = base + inc - mine;
                for (uint32_t t = m; t; t &= t - 1, o++) {
                    const uint64_t p = k * 16u + ((uint32_t)__ffs((int)t) - 1u) - s.lead - 12u;
                    if (o < cap) {
                        pos[o] = p;
                        size[o] = ms_header_size(s, p);
                    }
                }
                base += __shfl(inc, 63);
            }
        }
    }
    if (!WRITE) {
        for (int d = 32; d; d >>= 1) cnt += __shfl_xor(cnt, d);
        if (lane == 0) seg_count[seg] = cnt;
    }
}

// exclusive scan of the segments' counts; starts the scan record
__global__ __launch_bounds__(256) void k_mscan_offsets(uint32_t n_seg, const uint32_t *__restrict__ seg_count,
                                                       uint32_t *__restrict__ seg_off, uint32_t *__restrict__ rec) {
    __shared__ uint64_t wsum[4];
    __shared__ uint64_t carry_s;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t b = 0; b < n_seg; b += 256) {
        const uint32_t i = b + tid;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan256(i < n_seg ? seg_count[i] : 0u, wsum, &total);
        const uint64_t carry = carry_s;
        if (i < n_seg) seg_off[i] = (uint32_t)(carry + ex);  // (meaningless above 2^32: then n_cand > cap below)
        __syncthreads();
        if (tid == 0) carry_s = carry + total;
        __syncthreads();
    }
    if (tid == 0) {
        rec[kMsRecCand] = carry_s > 0xFFFFFFF0ull ? 0xFFFFFFFFu : (uint32_t)carry_s;
        rec[kMsRecMembers] = 0;
        rec[kMsRecKind] = 1;  // no candidate at offset 0: the walk's first header is invalid
        rec[3] = 0;
        rec[kMsRecConsumed] = rec[kMsRecConsumed + 1] = 0;
    }
}

// what the walk finds at offset q: a candidate index, kMsStop or kMsErr (rules 1-3 of gzpx_scan_blocks)
__device__ __forceinline__ uint32_t ms_resolve(uint64_t q, uint64_t len, uint32_t hdr, uint32_t n,
                                               const uint64_t *__restrict__ pos, const uint32_t *__restrict__ size) {
    if (len - q < hdr) return kMsStop;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (pos[mid] < q) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= n || pos[lo] != q) return kMsErr;
    return len - q < size[lo] ? kMsStop : lo;  // a member that is cut short is left to the caller
}

__global__ __launch_bounds__(256) void k_mscan_succ(uint64_t len, uint32_t hdr, uint32_t cap, uint32_t *__restrict__ rec,
                                                    const uint64_t *__restrict__ pos, const uint32_t *__restrict__ size,
                                                    uint32_t *__restrict__ succ, uint32_t *__restrict__ jump,
                                                    uint32_t *__restrict__ idx) {
    const uint32_t n = rec[kMsRecCand];
    if (n > cap) return;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
        const uint64_t p = pos[c], q = p + size[c];
        const bool whole = q <= len;  // (a cut member is nobody's successor: ms_resolve gives kMsStop instead)
        const uint32_t t = whole ? ms_resolve(q, len, hdr, n, pos, size) : kMsStop;
        succ[c] = t;
        jump[c] = t;
        uint32_t i = kMsNone;
        if (c == 0 && p == 0) {
            if (whole) i = 0;
            else rec[kMsRecKind] = 0;  // the first member is cut short: nothing recorded, nothing wrong
        }
        idx[c] = i;
    }
}

// round r: jin = the 2^r-th successor.  (idx is read for values < 2^r and written with values >= 2^r only.)
__global__ __launch_bounds__(256) void k_mscan_jump(uint32_t r, uint32_t cap, const uint32_t *__restrict__ rec,
                                                    const uint32_t *__restrict__ jin, uint32_t *__restrict__ jout,
                                                    uint32_t *idx) {
    const uint32_t n = rec[kMsRecCand];
    if (n > cap || (n >> r) == 0 || n == (1u << r)) return;  // 2^r >= n: every member's index is below 2^r already
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
        const uint32_t a = jin[c];
        const bool node = a < kMsErr && a < n;
        jout[c] = node ? jin[a] : a;
        const uint32_t i = idx[c];
        if (node && i < (1u << r)) idx[a] = i + (1u << r);
    }
}

__global__ __launch_bounds__(256) void k_mscan_finish(uint32_t cap, uint32_t *__restrict__ rec,
                                                      const uint64_t *__restrict__ pos, const uint32_t *__restrict__ size,
                                                      const uint32_t *__restrict__ succ, const uint32_t *__restrict__ idx) {
    const uint32_t n = rec[kMsRecCand];
    if (n > cap) return;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
        if (idx[c] == kMsNone || succ[c] < kMsErr) continue;
        const uint64_t end = pos[c] + size[c];  // the walk's last member: exactly one candidate gets here
        rec[kMsRecMembers] = idx[c] + 1u;
        rec[kMsRecKind] = succ[c] == kMsErr ? 1u : 0u;
        rec[kMsRecConsumed] = (uint32_t)end;
        rec[kMsRecConsumed + 1] = (uint32_t)(end >> 32);
    }
}

// members 0 .. n_emit - 1 of the walk into the caller's tables
__global__ __launch_bounds__(256) void k_mscan_emit(uint32_t cap, const uint32_t *__restrict__ rec, uint32_t n_emit,
                                                    const uint64_t *__restrict__ pos, const uint32_t *__restrict__ size,
                                                    const uint32_t *__restrict__ idx, uint64_t *__restrict__ offsets,
                                                    uint32_t *__restrict__ sizes) {
    const uint32_t n = rec[kMsRecCand];
    if (n > cap) return;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
        const uint32_t i = idx[c];
        if (i >= n_emit) continue;  // (kMsNone included)
        offsets[i] = pos[c];
        sizes[i] = size[c];
    }
}
