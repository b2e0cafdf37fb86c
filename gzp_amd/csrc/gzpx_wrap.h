// gzpx_wrap.h -- batches of independent DEFLATE members in a wrapper of the caller's choice (raw RFC 1951, zlib
// RFC 1950, gzip RFC 1952), for gzpx_inflate_batch_device and gzpx_inflate_batch_sizes_device.  Included from
// gzpx_kernels.hip, namespace gzpx, behind k_inflate / k_inflate_seg / k_lzcopy, which do the inflating: what is here puts their records (DBlock) in place
// from a caller's table, checks what a wrapper carries, and reports per member.
//
//   k_dinit_wrap   one lane per member: the table entry against in_len, the wrapper's header, the trailer -> DBlock
//                  (payload bounds per member) and the member's slot in the output.  A member that fails here keeps
//                  isize = 0, so that no later kernel touches it.
//   k_dscan_slots  exclusive scan of the slots -> output offsets (they never depend on a member's fate); a member
//                  whose slot ends behind out_cap is taken out the same way.
//   (k_inflate_seg + k_lzcopy + k_inflate, or k_inflate alone: launch_inflate_members)
//   k_dadler32     zlib: Adler-32 of the bytes every member produced, a workgroup per member.
//   (k_dcrc32      gzip: as for BGZF; k_lzcopy's in-tile CRC serves too.  Raw: neither.)
//   k_dresult      per-member status / produced / check values, the caller's offsets, and the record for the host
//                  (kWrRec*, gzpx_device.h): first failing member, its status and two values, how many failed, the total.
//
// and for gzpx_inflate_batch_sizes_device, which inflates nothing and answers what every member inflates to:
//   k_dinit_wrap_sizes   k_dinit_wrap's entry and header rules (one routine, dinit_wrap_member) for a member whose end is
//                        not known: the payload runs to the end of the entry, no trailer is read, isize is the cap.
//   (k_inflate_seg<.., COUNT> + k_inflate<.., COUNT> over its hand-backs, or the latter alone: launch_inflate_sizes)
//   k_dresult_sizes      the member's length from where its stream ended, the trailer against the entry, the caller's
//                        tables, and the same record with the 64-bit sum of the sizes.
#pragma once

// DBlock.status of a member that the wrapper kernels took out (never decoded; InflateStatus: gzpx_device.h, kInfRedo: gzpx_inflate_seg.h)
constexpr uint32_t kWrapArg = 0x10u;     // the table entry reaches outside the input, or is shorter than its wrapper
constexpr uint32_t kWrapHeader = 0x11u;  // the wrapper's header is invalid
constexpr uint32_t kWrapSpace = 0x12u;   // the slot ends behind out_cap
constexpr uint32_t kWrapSize = 0x13u;    // gzip: ISIZE (kept in DBlock.crc) differs from the caller's size

enum { kWrapRaw = 0, kWrapZlib = 1, kWrapGzip = 2 };

// ------------------------------------------------------------------------------------------
// Adler-32 of p[0, n) by a workgroup of kAdlerThreads, as the pair every piece of a buffer gives on its own:
// s1 = sum d_i, s2 = sum (n - i) d_i (i = 0 .. n - 1), both mod 65521; entered with (a0, b0) the buffer ends with
// a = a0 + s1, b = b0 + n a0 + s2.
//
// The 16-byte-aligned middle of the buffer goes through aligned 16-byte loads, a lane's chunks a tile (256 lanes x 16
// bytes) apart; the bytes in front of and behind it, fewer than 16 each, one to a lane.  A lane keeps (a, b) of its
// own bytes relative to the end E of its last chunk: a tile further, b grows by 4096 a, then the chunk adds its byte
// sum c1 <= 4080 and its position-weighted sum c2 = sum (16 - j) d_j <= 34680.  64-bit accumulators, folded mod 65521
// every kAdlerFold chunks: with 0xFF bytes throughout a stays below 65521 + 256 * 4080 < 2^21 and b below
// 65521 + 256 * (4096 * 2^21 + 34680) < 2^42 between folds.  What a lane holds at the end moves to the buffer's end with
// (n - E) a -- below 2^32 * 2^16.  Then a wave reduction by shuffles and the four waves through LDS.
//
// It lives here because the zlib wrapper needs the same sum over every inflated member as gzpx_adler32
// (Adler32::update, src/check.rs:85-164, pinned on Python's zlib module in tests/test_checks.py and
// tests/test_gpu_checks.py): adler_workgroup is the one device routine, and k_adler32_tiles (one (s1, s2, n) per
// 64 KiB tile, combined on the host; launch_adler32 is with the other launchers in gzpx_kernels.hip), k_dadler32 (a
// workgroup per member) and k_cksum_tiles (gzpx_cksum.h) are its callers.  Adler32::combine and Crc32::combine are
// plain arithmetic in gzpx_api.cpp.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kAdlerBase = 65521u;
constexpr uint32_t kAdlerThreads = 256u;
constexpr uint32_t kAdlerFold = 256u;
constexpr uint32_t kAdlerTile = 65536u;  // launch_adler32: one (s1, s2, n) per 64 KiB of a buffer

// byte sum and weighted sum (weights 16 .. 1) of 16 bytes in memory order
__device__ __forceinline__ void adler_chunk16(const uint4 q, uint32_t &c1, uint32_t &c2) {
#if defined(__HIP_DEVICE_COMPILE__)
    c1 = __builtin_amdgcn_udot4(q.x, 0x01010101u, 0u, false);
    c1 = __builtin_amdgcn_udot4(q.y, 0x01010101u, c1, false);
    c1 = __builtin_amdgcn_udot4(q.z, 0x01010101u, c1, false);
    c1 = __builtin_amdgcn_udot4(q.w, 0x01010101u, c1, false);
    c2 = __builtin_amdgcn_udot4(q.x, 0x0D0E0F10u, 0u, false);
    c2 = __builtin_amdgcn_udot4(q.y, 0x090A0B0Cu, c2, false);
    c2 = __builtin_amdgcn_udot4(q.z, 0x05060708u, c2, false);
    c2 = __builtin_amdgcn_udot4(q.w, 0x01020304u, c2, false);
#else
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    c1 = c2 = 0;
    for (uint32_t j = 0; j < 16; j++) {
        const uint32_t d = (w[j >> 2] >> (8u * (j & 3u))) & 0xFFu;
        c1 += d;
        c2 += (16u - j) * d;
    }
#endif
}

struct AdlerLds {
    uint32_t part[2][kAdlerThreads / 64];
};

// Every thread of the workgroup calls it; every thread gets (s1, s2).  (A barrier in front: the LDS may be in use.)
__device__ __forceinline__ void adler_workgroup(AdlerLds &l, const uint8_t *__restrict__ p, uint64_t n, uint32_t tid,
                                                uint32_t &s1, uint32_t &s2) {
    uint32_t head = (uint32_t)((16u - ((uintptr_t)p & 15u)) & 15u);
    if (head > n) head = (uint32_t)n;
    const uint64_t nv = (n - head) >> 4;           // aligned 16-byte chunks
    const uint64_t tail0 = head + 16u * nv;        // the first byte behind them
    const uint4 *v = (const uint4 *)(p + head);
    uint64_t a = 0, b = 0, end = 0;
    uint32_t fold = 0;
    for (uint64_t k = tid; k < nv; k += kAdlerThreads) {
        uint32_t c1, c2;
        adler_chunk16(v[k], c1, c2);
        b += a * (16u * kAdlerThreads) + c2;
        a += c1;
        end = head + 16u * (k + 1u);
        if (++fold == kAdlerFold) {
            fold = 0;
            a %= kAdlerBase;
            b %= kAdlerBase;
        }
    }
    a %= kAdlerBase;
    b = (b + ((n - end) % kAdlerBase) * a) % kAdlerBase;
    if (tid < head) {  // the bytes in front of the aligned middle, one to a lane
        const uint64_t d = p[tid];
        a += d;
        b += ((n - tid) % kAdlerBase) * d;
    }
    if (tid < n - tail0) {  // and the ones behind it
        const uint64_t i = tail0 + tid, d = p[i];
        a += d;
        b += (n - i) * d;  // (n - i <= 15)
    }
    uint32_t ra = (uint32_t)(a % kAdlerBase), rb = (uint32_t)(b % kAdlerBase);
    for (int m = 32; m >= 1; m >>= 1) {  // 64 values below 2^16: no overflow
        ra += __shfl_xor(ra, m);
        rb += __shfl_xor(rb, m);
    }
    __syncthreads();
    if ((tid & 63u) == 0) {
        l.part[0][tid >> 6] = ra;
        l.part[1][tid >> 6] = rb;
    }
    __syncthreads();
    uint32_t ta = 0, tb = 0;
    for (uint32_t w = 0; w < kAdlerThreads / 64; w++) {
        ta += l.part[0][w];
        tb += l.part[1][w];
    }
    s1 = ta % kAdlerBase;
    s2 = tb % kAdlerBase;
}

// gzpx_adler32: (s1, s2, n) of every 64 KiB tile of in[0, n) -> out3[3 * tile + ..]; the host combines the tiles
__global__ __launch_bounds__(kAdlerThreads) void k_adler32_tiles(const uint8_t *__restrict__ in, uint64_t n,
                                                                 uint32_t *__restrict__ out3) {
    __shared__ AdlerLds l;
    const uint64_t lo = (uint64_t)blockIdx.x * kAdlerTile;
    const uint32_t len = (uint32_t)(n - lo < kAdlerTile ? n - lo : kAdlerTile);
    uint32_t s1, s2;
    adler_workgroup(l, in + lo, len, threadIdx.x, s1, s2);
    if (threadIdx.x == 0) {
        out3[3 * blockIdx.x + 0] = s1;
        out3[3 * blockIdx.x + 1] = s2;
        out3[3 * blockIdx.x + 2] = len;
    }
}

// zlib members: Adler-32 of the bytes each produced.  Members that were taken out or failed to decode are left alone
// (nothing of their slots is read); fewer bytes than the slot (kInfShortOutput) are the caller's to accept or not.
__global__ __launch_bounds__(kAdlerThreads) void k_dadler32(const uint8_t *__restrict__ out_all,
                                                            const uint64_t *__restrict__ out_off,
                                                            const DBlock *__restrict__ blk_all,
                                                            uint32_t *__restrict__ found) {
    __shared__ AdlerLds l;
    const uint32_t b = blockIdx.x;
    const uint32_t st = blk_all[b].status;
    if (st != kInfOk && st != kInfShortOutput) {
        if (threadIdx.x == 0) found[b] = 0;
        return;
    }
    const uint32_t n = blk_all[b].produced;
    uint32_t s1, s2;
    adler_workgroup(l, out_all + out_off[b], n, threadIdx.x, s1, s2);
    // from (a0, b0) = (1, 0): a = 1 + s1, b = n + s2
    if (threadIdx.x == 0) found[b] = ((1u + s1) % kAdlerBase) | (((n % kAdlerBase + s2) % kAdlerBase) << 16);
}

// ------------------------------------------------------------------------------------------
// the table
// ------------------------------------------------------------------------------------------
struct WrapTable {
    const uint8_t *in;         // the input, in_len bytes: no byte outside it is read, whatever the table says
    uint64_t in_len;
    const uint64_t *off;       // [nb] where a member starts
    const uint32_t *size;      // [nb] its length, wrapper included
    const uint32_t *out_size;  // [nb] its slot in the output; null (gzip): the trailer's ISIZE
    uint32_t wrap;
};

// SIZES (gzpx_inflate_batch_sizes_device, k_dinit_wrap_sizes): the same entry and header rules for a member whose end
// is not known.  size[b] is an upper bound; the payload runs from behind the header to the end of the entry (the
// trailer's place is found behind the final block: k_dresult_sizes), no trailer is read, and isize is the cap on the
// member's output, `max_out` -- never 0 for a member that is to be sized.  An entry's payload is cut at kWrapMaxPay
// bytes: bit positions are 32-bit words in the kernels that follow.
constexpr uint32_t kWrapMaxPay = 0x1FFFFF00u;
template <bool SIZES>
__device__ __forceinline__ void dinit_wrap_member(uint32_t b, const WrapTable &t, uint32_t max_out, DBlock *__restrict__ blk,
                                                  uint32_t *__restrict__ slot) {
    const uint64_t off = t.off[b];
    const uint32_t sz = t.size[b];
    const uint32_t want = t.out_size ? t.out_size[b] : 0u;
    const uint32_t overhead = t.wrap == kWrapGzip ? 18u : t.wrap == kWrapZlib ? 6u : 0u;
    DBlock d;
    d.in_off = off;
    d.size = sz;
    d.isize = 0;
    d.crc = 0;
    d.status = kInfOk;
    d.produced = 0;
    d.nmatch = 0;
    d.pay_off = 0;
    d.pay_len = 0;
    for (uint32_t k = 0; k < 8; k++) d.cyc[k] = 0;
    uint32_t my_slot = SIZES ? max_out : want;
    if (off > t.in_len || sz > t.in_len - off || sz < overhead) {
        d.status = kWrapArg;
    } else {
        const uint8_t *p = t.in + off;  // p[0, sz) is inside the input
        if (t.wrap == kWrapRaw) {
            d.pay_len = sz;
            if (sz == 0 && (SIZES || want != 0)) d.status = kInfBadData;  // (no final block; and nothing of such a member may be read)
        } else if (t.wrap == kWrapZlib) {
            const uint32_t cmf = p[0], flg = p[1];
            if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) d.status = kWrapHeader;
            d.pay_off = 2;
            d.pay_len = sz - 6u;
            if constexpr (!SIZES) {
                const uint8_t *f = p + sz - 4;  // Adler-32, big endian
                d.crc = ((uint32_t)f[0] << 24) | ((uint32_t)f[1] << 16) | ((uint32_t)f[2] << 8) | (uint32_t)f[3];
            }
        } else {
            const uint32_t lim = sz - 8u;  // every header field ends in front of the trailer
            const uint32_t flg = p[3];
            bool ok = p[0] == 0x1Fu && p[1] == 0x8Bu && p[2] == 8u && !(flg & 0xE0u);
            uint32_t pos = 10;
            if (ok && (flg & 4u)) {  // FEXTRA
                if (pos + 2u > lim) {
                    ok = false;
                } else {
                    pos += 2u + ((uint32_t)p[pos] | ((uint32_t)p[pos + 1] << 8));
                    ok = pos <= lim;
                }
            }
            for (uint32_t fld = 8u; fld <= 16u; fld <<= 1)  // FNAME, FCOMMENT: zero-terminated
                if (ok && (flg & fld)) {
                    while (pos < lim && p[pos] != 0) pos++;
                    ok = pos < lim;
                    pos++;
                }
            if (ok && (flg & 2u)) {  // FHCRC: skipped, not verified (libdeflate does not either)
                pos += 2u;
                ok = pos <= lim;
            }
            if (!ok) {
                d.status = kWrapHeader;
                pos = 10;
            }
            d.pay_off = pos;
            d.pay_len = lim - pos;
            if constexpr (!SIZES) {
                const uint8_t *f = p + lim;
                d.crc = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24);
                const uint32_t isz = (uint32_t)f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) | ((uint32_t)f[7] << 24);
                if (!t.out_size) {
                    my_slot = isz;
                } else if (isz != want && d.status == kInfOk) {
                    d.status = kWrapSize;
                    d.crc = isz;
                }
            }
        }
        if constexpr (SIZES) {  // the payload: everything behind the header, as far as the entry goes
            const uint32_t rest = sz - d.pay_off;
            d.pay_len = rest < kWrapMaxPay ? rest : kWrapMaxPay;
            d.size = d.pay_off + d.pay_len;
        }
    }
    if (d.status == kInfOk) d.isize = my_slot;
    if constexpr (!SIZES) slot[b] = my_slot;
    blk[b] = d;
}

__global__ __launch_bounds__(256) void k_dinit_wrap(uint32_t nb, WrapTable t, DBlock *__restrict__ blk,
                                                    uint32_t *__restrict__ slot, uint32_t *__restrict__ redo) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0 && redo) {
        redo[0] = 0;       // members handed back to k_inflate
        redo[1 + nb] = 0;  // k_inflate_seg's ticket counter
    }
    if (b >= nb) return;
    dinit_wrap_member<false>(b, t, 0u, blk, slot);
}

__global__ __launch_bounds__(256) void k_dinit_wrap_sizes(uint32_t nb, WrapTable t, uint32_t max_out, DBlock *__restrict__ blk,
                                                          uint32_t *__restrict__ redo) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0 && redo) {
        redo[0] = 0;
        redo[1 + nb] = 0;
    }
    if (b >= nb) return;
    dinit_wrap_member<true>(b, t, max_out, blk, nullptr);
}

__global__ __launch_bounds__(256) void k_dscan_slots(uint32_t nb, const uint32_t *__restrict__ slot, DBlock *__restrict__ blk,
                                                     uint64_t out_cap, uint64_t *__restrict__ out_off) {
    __shared__ uint64_t wsum[4];
    __shared__ uint64_t carry_s;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += 256) {
        const uint32_t i = base + tid;
        const uint64_t v = i < nb ? slot[i] : 0;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan256(v, wsum, &total);
        const uint64_t carry = carry_s;
        if (i < nb) {
            out_off[i] = carry + ex;
            if (carry + ex + v > out_cap && blk[i].status != kWrapArg && blk[i].status != kWrapHeader) {  // (those two come first)
                blk[i].status = kWrapSpace;
                blk[i].isize = 0;
            }
        }
        __syncthreads();
        if (tid == 0) carry_s = carry + total;
        __syncthreads();
    }
    if (tid == 0) out_off[nb] = carry_s;
}

// ------------------------------------------------------------------------------------------
// the report.  gzpx_member_result's layout; the status values are include/gzpx.h's GZPX_ERR_*.
// ------------------------------------------------------------------------------------------
struct WrapResult {
    uint32_t status, produced, found, expected;
};
constexpr uint32_t kWrOk = 0, kWrInvalidArg = 1, kWrInsufficientSpace = 4, kWrInvalidHeader = 12, kWrInvalidCheck = 13,
                   kWrBadData = 14;
// (the record k_dresult leaves for the host: kWrRec*, gzpx_device.h)

__device__ __forceinline__ WrapResult wrap_verdict(const DBlock &d, uint32_t slot, uint32_t check, uint32_t wrap, bool short_ok) {
    WrapResult r;
    r.produced = d.produced;
    r.found = r.expected = 0;
    const uint32_t st = d.status;
    if (st == kWrapArg) r.status = kWrInvalidArg;
    else if (st == kWrapHeader) r.status = kWrInvalidHeader;
    else if (st == kWrapSpace || st == kInfInsufficientSpace) r.status = kWrInsufficientSpace;
    else if (st == kWrapSize) {
        r.status = kWrInvalidCheck;
        r.found = d.crc;
        r.expected = slot;
    } else if (st != kInfOk && !(st == kInfShortOutput && short_ok)) {
        r.status = kWrBadData;  // an invalid stream, or fewer bytes than the slot
    } else if (wrap != kWrapRaw && check != d.crc) {
        r.status = kWrInvalidCheck;
        r.found = check;
        r.expected = d.crc;
    } else {
        r.status = kWrOk;
    }
    return r;
}

__global__ __launch_bounds__(256) void k_dresult(uint32_t nb, uint32_t wrap, uint32_t short_ok, const DBlock *__restrict__ blk,
                                                 const uint32_t *__restrict__ slot, const uint32_t *__restrict__ check,
                                                 const uint64_t *__restrict__ out_off, WrapResult *__restrict__ results,
                                                 uint64_t *__restrict__ user_off, uint32_t *__restrict__ rec) {
    __shared__ uint32_t first, failed;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        first = 0xFFFFFFFFu;
        failed = 0;
    }
    __syncthreads();
    for (uint32_t b = tid; b < nb; b += 256) {
        const WrapResult r = wrap_verdict(blk[b], slot[b], check[b], wrap, short_ok != 0);
        if (results) results[b] = r;
        if (user_off) user_off[b] = out_off[b];
        if (r.status != kWrOk) {
            atomicMin(&first, b);
            atomicAdd(&failed, 1u);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const uint32_t b = first;
        WrapResult r{0, 0, 0, 0};
        if (b != 0xFFFFFFFFu) r = wrap_verdict(blk[b], slot[b], check[b], wrap, short_ok != 0);
        const uint64_t total = out_off[nb];
        rec[kWrRecFirst] = b;
        rec[kWrRecStatus] = r.status;
        rec[kWrRecFound] = r.found;
        rec[kWrRecExpected] = r.expected;
        rec[kWrRecFailed] = failed;
        rec[5] = 0;
        rec[kWrRecTotal] = (uint32_t)total;
        rec[kWrRecTotal + 1] = (uint32_t)(total >> 32);
        if (user_off) user_off[nb] = total;
    }
}

// ------------------------------------------------------------------------------------------
// gzpx_inflate_batch_sizes_device: what k_inflate_seg<.., COUNT> / k_inflate<.., COUNT> left in the records -> the
// caller's tables.  A member's length is its header, the payload bytes its stream took and the trailer (0 / 4 / 8
// bytes), and it has to end inside the entry: a stream whose trailer does not fit is as invalid as one that ends
// early.  No trailer byte is read.  produced = the size, found = the member's length, for a good member; both 0 for a
// failed one.  The total goes through the workgroup's 64-bit sum (k_dscan's loop), one pass over the members.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ WrapResult sizes_verdict(const DBlock &d, uint32_t wrap) {
    WrapResult r{kWrOk, 0, 0, 0};
    const uint32_t st = d.status;
    if (st == kWrapArg) r.status = kWrInvalidArg;
    else if (st == kWrapHeader) r.status = kWrInvalidHeader;
    else if (st == kInfInsufficientSpace) r.status = kWrInsufficientSpace;
    else if (st != kInfOk) r.status = kWrBadData;
    else {
        const uint64_t used = (uint64_t)d.pay_off + d.nmatch + (wrap == kWrapGzip ? 8u : wrap == kWrapZlib ? 4u : 0u);
        if (used > d.size) {
            r.status = kWrBadData;
        } else {
            r.produced = d.produced;
            r.found = (uint32_t)used;
        }
    }
    return r;
}

__global__ __launch_bounds__(256) void k_dresult_sizes(uint32_t nb, uint32_t wrap, const DBlock *__restrict__ blk,
                                                       uint32_t *__restrict__ out_sizes, uint32_t *__restrict__ in_used,
                                                       WrapResult *__restrict__ results, uint32_t *__restrict__ rec) {
    __shared__ uint64_t wsum[4];
    __shared__ uint64_t carry_s;
    __shared__ uint32_t first, failed;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        carry_s = 0;
        first = 0xFFFFFFFFu;
        failed = 0;
    }
    __syncthreads();
    uint32_t my_first = 0xFFFFFFFFu, my_failed = 0;
    for (uint32_t base = 0; base < nb; base += 256) {
        const uint32_t b = base + tid;
        uint64_t v = 0;
        if (b < nb) {
            const WrapResult r = sizes_verdict(blk[b], wrap);
            out_sizes[b] = r.produced;
            if (in_used) in_used[b] = r.found;
            if (results) results[b] = r;
            v = r.produced;
            if (r.status != kWrOk) {
                my_first = my_first < b ? my_first : b;
                my_failed++;
            }
        }
        uint64_t total;
        (void)block_exclusive_scan256(v, wsum, &total);
        if (tid == 0) carry_s += total;  // (thread 0 alone reads and writes it; the scan's barriers order the rest)
    }
    if (my_failed) {  // once per lane, not once per member
        atomicMin(&first, my_first);
        atomicAdd(&failed, my_failed);
    }
    __syncthreads();
    if (tid == 0) {
        const uint32_t b = first;
        WrapResult r{0, 0, 0, 0};
        if (b != 0xFFFFFFFFu) r = sizes_verdict(blk[b], wrap);
        const uint64_t total = carry_s;
        rec[kWrRecFirst] = b;
        rec[kWrRecStatus] = r.status;
        rec[kWrRecFound] = 0;
        rec[kWrRecExpected] = 0;
        rec[kWrRecFailed] = failed;
        rec[5] = 0;
        rec[kWrRecTotal] = (uint32_t)total;
        rec[kWrRecTotal + 1] = (uint32_t)(total >> 32);
    }
}
