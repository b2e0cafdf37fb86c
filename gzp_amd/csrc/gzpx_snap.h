// gzpx_snap.h -- gzp's Snap format (src/snap.rs:38-83: snap::read::FrameEncoder over every buffer_size piece of the
// stream).  Included by gzpx_kernels.hip inside namespace gzpx, behind
// gzpx_wave.h (wave_sync, the scans, gzpx_crc.h).
//
// A buffer is cut into chunks of 65,536 bytes; every chunk is framed as a 4-byte header (type, 24-bit length), the
// masked CRC-32C of the uncompressed chunk and a body: the raw Snappy encoding of the chunk (type 0x00), or the chunk
// itself (type 0x01) when that encoding is not shorter than n - n/8.  A non-empty buffer starts with the 10-byte
// stream identifier; an empty one encodes to nothing.  The raw encoding is snappy 1.1.8's compressor, step for step
// (DESIGN.md "Snap" states the loop and what it is pinned on).
//
//   k_snap_chunk  one wave per chunk: the hash table (16,384 x u16 at most) in LDS, the input through the vector
//                 caches.  The literal scan takes 64 probes per step: until a match is found the probe positions
//                 depend only on the skip counter, so lane i takes probe j0 + i.  Each lane reads the table as it
//                 stood before the step; a lane whose hash equals an earlier lane's takes that lane's position
//                 instead.  The first lane whose 4 bytes match wins; the table writes of the lanes up to it are
//                 committed (the last writer per slot), the rest are dropped.  Match extension compares 64 bytes
//                 per step.  The body goes to the chunk's staging area, with the CRC-32C of the chunk.
//   k_snap_frame  one lane per buffer: the framed size of every chunk and of the buffer (BlockMeta.framed_bytes,
//                 for k_scan), and where each chunk's frame starts inside its buffer's.
//   k_snap_emit   one workgroup per chunk: stream identifier, chunk header and body at their offsets.

constexpr uint32_t kSnapChunk = 65536;                                // snap's MAX_BLOCK_SIZE
constexpr uint32_t kSnapMaxTable = 16384;                             // snappy's kMaxHashTableSize
constexpr uint32_t kSnapStageStride = kSnapStageBytes;
static_assert(kSnapStageBytes >= 32u + kSnapChunk + kSnapChunk / 6u, "MaxCompressedLength");
constexpr uint32_t kSnapMargin = 15;                                  // kInputMarginBytes
constexpr uint32_t kSnapEmitThreads = 256;

// The literal scan's probe j lies kSnapProbe.off[j] bytes behind the scan's start: skip starts at 32 and grows by
// skip >> 5, which is the step.  Entry 268 is past 65,536, so a scan has ended by step j0 = 256, whose lanes read
// entries up to 320.
constexpr uint32_t kSnapProbes = 336;
struct SnapProbeTable {
    uint32_t off[kSnapProbes];
};
constexpr SnapProbeTable snap_probe_table() {
    SnapProbeTable t{};
    uint32_t o = 0, skip = 32;
    for (uint32_t j = 0; j < kSnapProbes; j++) {
        t.off[j] = o;
        o += skip >> 5;
        skip += skip >> 5;
    }
    return t;
}
__constant__ SnapProbeTable kSnapProbe = snap_probe_table();

__device__ __forceinline__ uint32_t snap_chunk_len(uint64_t slab_len, uint32_t bs, uint32_t cpb, uint32_t c) {
    const uint32_t b = c / cpb, k = c % cpb;
    const uint64_t begin = (uint64_t)b * bs, kb = (uint64_t)k * kSnapChunk;
    if (kb >= bs || begin + kb >= slab_len) return 0;
    uint64_t n = slab_len - begin - kb;
    if (n > bs - kb) n = bs - kb;
    return n > kSnapChunk ? kSnapChunk : (uint32_t)n;
}

__device__ __forceinline__ bool snap_stored(uint32_t n, uint32_t clen) { return clen >= n - n / 8u; }

// x^(8 m) mod P of CRC-32C, squared up on the fly (a wave has no table to keep)
__device__ __forceinline__ uint32_t crc32c_x8n(uint32_t m) {
    uint32_t r = 0x80000000u, sq = 0x00800000u;  // x^0, x^8
    while (m) {
        if (m & 1u) r = crc_mulmod<kCrcPoly32c>(r, sq);
        sq = crc_mulmod<kCrcPoly32c>(sq, sq);
        m >>= 1;
    }
    return r;
}

// masked CRC-32C of src[0..n) by one wave: every lane takes a run of ceil(n / 64) bytes from zero, and the runs
// are shifted into place and added (the CRC is linear); the initial all-ones register is one more such term
__device__ uint32_t snap_crc32c_wave(const uint8_t *__restrict__ src, uint32_t n, uint32_t lane) {
    const uint32_t per = (n + 63u) / 64u;
    const uint32_t lo = lane * per < n ? lane * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t r = 0;
    for (uint32_t i = lo; i < hi; i++) {
        r ^= src[i];
        for (int t = 0; t < 8; t++) r = (r >> 1) ^ (kCrcPoly32c & (0u - (r & 1u)));
    }
    uint32_t v = hi > lo ? crc_mulmod<kCrcPoly32c>(crc32c_x8n(n - hi), r) : 0u;
    if (lane == 0) v ^= crc_mulmod<kCrcPoly32c>(crc32c_x8n(n), 0xFFFFFFFFu);
    for (int m = 32; m >= 1; m >>= 1) v ^= __shfl_xor(v, m);
    const uint32_t c = ~v;
    return ((c >> 15) | (c << 17)) + 0xa282ead8u;
}

__device__ __forceinline__ uint32_t snap_hash(uint32_t v, uint32_t shift) { return (v * 0x1e35a7bdu) >> shift; }

// the tags are written by lane 0; every lane keeps the same output position
__device__ __forceinline__ uint32_t snap_emit_literal(uint8_t *__restrict__ out, uint32_t op,
                                                      const uint8_t *__restrict__ src, uint32_t len, uint32_t lane) {
    const uint32_t m = len - 1u;
    uint32_t hdr = 1;
    if (m < 60u) {
        if (lane == 0) out[op] = (uint8_t)(m << 2);
    } else {
        const uint32_t k = m < 0x100u ? 1u : m < 0x10000u ? 2u : m < 0x1000000u ? 3u : 4u;
        if (lane == 0) {
            out[op] = (uint8_t)((59u + k) << 2);
            for (uint32_t i = 0; i < k; i++) out[op + 1 + i] = (uint8_t)(m >> (8u * i));
        }
        hdr += k;
    }
    op += hdr;
    for (uint32_t i = lane; i < len; i += 64u) out[op + i] = src[i];
    return op + len;
}

__device__ __forceinline__ uint32_t snap_copy64(uint8_t *__restrict__ out, uint32_t op, uint32_t o, uint32_t l,
                                                uint32_t lane) {
    if (l < 12u && o < 2048u) {
        if (lane == 0) {
            out[op] = (uint8_t)(1u | ((l - 4u) << 2) | ((o >> 8) << 5));
            out[op + 1] = (uint8_t)o;
        }
        return op + 2;
    }
    if (lane == 0) {
        out[op] = (uint8_t)(2u | ((l - 1u) << 2));
        out[op + 1] = (uint8_t)o;
        out[op + 2] = (uint8_t)(o >> 8);
    }
    return op + 3;
}

__device__ __forceinline__ uint32_t snap_emit_copy(uint8_t *__restrict__ out, uint32_t op, uint32_t o, uint32_t l,
                                                   uint32_t lane) {
    while (l >= 68u) {
        op = snap_copy64(out, op, o, 64, lane);
        l -= 64u;
    }
    if (l > 64u) {
        op = snap_copy64(out, op, o, 60, lane);
        l -= 60u;
    }
    return snap_copy64(out, op, o, l, lane);
}

// DBG: clock64 spans of the phases, per chunk: [0] whole kernel, [1] CRC, [2] literal scans, [3] match extension,
// [4] literal and copy emission, [5] scan steps, [6] copies
template <bool DBG>
__global__ __launch_bounds__(64) void k_snap_chunk(const uint8_t *__restrict__ slab, uint64_t slab_len, uint32_t bs,
                                                   uint32_t cpb, uint8_t *__restrict__ stage,
                                                   uint32_t *__restrict__ clen_out, uint32_t *__restrict__ crc_out,
                                                   uint64_t *__restrict__ dbg) {
    __shared__ uint16_t table[kSnapMaxTable];
    __shared__ uint32_t sh_h[64];
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    const uint32_t n = snap_chunk_len(slab_len, bs, cpb, c);
    if (n == 0) {
        if (lane == 0) clen_out[c] = 0;
        return;
    }
    uint64_t t_begin = 0, t_mark = 0, cyc[7] = {0, 0, 0, 0, 0, 0, 0};
    if (DBG) t_begin = t_mark = clock64();
    auto lap = [&](int k) {
        if (DBG) {
            const uint64_t t = clock64();
            cyc[k] += t - t_mark;
            t_mark = t;
        }
    };
    const uint8_t *__restrict__ src = slab + (uint64_t)(c / cpb) * bs + (uint64_t)(c % cpb) * kSnapChunk;
    uint8_t *__restrict__ out = stage + (size_t)c * kSnapStageStride;
    const uint32_t crc = snap_crc32c_wave(src, n, lane);
    lap(1);
    // varint of the length
    uint32_t op = 0;
    for (uint32_t v = n;; v >>= 7) {
        if (lane == 0) out[op] = (uint8_t)((v & 0x7Fu) | (v >= 0x80u ? 0x80u : 0u));
        op++;
        if (v < 0x80u) break;
    }
    uint32_t emit = 0;
    if (n >= kSnapMargin) {
        uint32_t size = 256;
        while (size < kSnapMaxTable && size < n) size <<= 1;
        const uint32_t shift = 32u - (31u - (uint32_t)__clz((int)size));
        for (uint32_t i = lane; i < size; i += 64u) table[i] = 0;
        const uint32_t limit = n - kSnapMargin;
        uint32_t ip0 = 1;  // where the current literal scan starts
        for (;;) {
            // ---- literal scan, 64 probes per step
            uint32_t ip = 0, cand = 0;
            bool found = false;
            for (uint32_t j0 = 0;; j0 += 64u) {
                wave_sync();  // (the table writes of the step before are in)
                const uint32_t j = j0 + lane;
                const uint32_t p = ip0 + kSnapProbe.off[j];
                const bool valid = ip0 + kSnapProbe.off[j + 1] <= limit;  // (a lane past the limit does not probe)
                const uint32_t nvalid = (uint32_t)__popcll(__ballot(valid));  // (the valid lanes are a prefix)
                if (nvalid == 0) break;
                const uint32_t here = valid ? load_le32_global(src + p) : 0u;
                const uint32_t h = valid ? snap_hash(here, shift) : 0xFFFFFFFFu;
                sh_h[lane] = h;
                wave_sync();
                const uint32_t old = valid ? (uint32_t)table[h] : 0u;
                // Probe against the table first; only the lanes up to the first of those matches can change their
                // answer through an earlier lane's position, so the same-slot search runs over them alone (lanes
                // 0..bound), and on past them only if that first match goes (rare).
                bool match = valid && here == load_le32_global(src + old);
                uint64_t mm = __ballot(match);
                uint32_t bound = mm ? (uint32_t)__ffsll((long long)mm) - 1u : nvalid - 1u;
                int prev = -1, next = 64;  // the latest earlier / the first later lane with the same slot
                uint32_t k = 0, first = 64;
                for (;;) {
                    for (; k <= bound; k++) {
                        const uint32_t hk = sh_h[k];
                        if (hk == h) {
                            if (k < lane) prev = (int)k;
                            if (k > lane && next == 64) next = (int)k;
                        }
                    }
                    const bool fwd = prev >= 0 && lane <= bound;
                    if (__ballot(fwd)) {
                        if (fwd) match = here == load_le32_global(src + ip0 + kSnapProbe.off[j0 + (uint32_t)prev]);
                    }
                    mm = __ballot(match && lane <= bound);
                    if (mm) {
                        first = (uint32_t)__ffsll((long long)mm) - 1u;
                        break;
                    }
                    if (bound + 1u >= nvalid) break;
                    bound = nvalid - 1u;
                }
                const uint32_t cpos = prev >= 0 ? ip0 + kSnapProbe.off[j0 + (uint32_t)prev] : old;
                const uint32_t ncommit = first < nvalid ? first + 1u : nvalid;
                if (lane < ncommit && (uint32_t)next >= ncommit) table[h] = (uint16_t)p;
                if (DBG) {
                    if (lane == 0) cyc[5]++;
                }
                if (first < 64u) {
                    ip = __shfl(p, (int)first);
                    cand = __shfl(cpos, (int)first);
                    found = true;
                    break;
                }
                if (nvalid < 64u) break;
            }
            lap(2);
            if (!found) break;
            op = snap_emit_literal(out, op, src + emit, ip - emit, lane);
            lap(4);
            // ---- one or more copies
            bool tail = false;
            for (;;) {
                uint32_t len = 4;
                for (;;) {  // match extension, 64 bytes per step, up to the chunk's end
                    const uint32_t t = len + lane;
                    const bool ne = ip + t >= n || src[cand + t] != src[ip + t];
                    const uint64_t m = __ballot(ne);
                    if (m) {
                        len += (uint32_t)__ffsll((long long)m) - 1u;
                        break;
                    }
                    len += 64u;
                }
                lap(3);
                op = snap_emit_copy(out, op, ip - cand, len, lane);
                if (DBG) {
                    if (lane == 0) cyc[6]++;
                }
                lap(4);
                ip += len;
                emit = ip;
                if (ip >= limit) {
                    tail = true;
                    break;
                }
                const uint32_t ph = snap_hash(load_le32_global(src + ip - 1), shift);
                const uint32_t here = load_le32_global(src + ip);
                const uint32_t ch = snap_hash(here, shift);
                const uint32_t old = table[ch];
                wave_sync();  // (every lane has read before lane 0 writes)
                cand = ph == ch ? ip - 1u : old;
                if (lane == 0) {
                    table[ph] = (uint16_t)(ip - 1u);
                    table[ch] = (uint16_t)ip;
                }
                const bool again = here == load_le32_global(src + cand);
                lap(3);
                if (!again) break;
            }
            if (tail) break;
            ip0 = ip + 1u;
        }
    }
    if (emit < n) op = snap_emit_literal(out, op, src + emit, n - emit, lane);
    lap(4);
    if (lane == 0) {
        clen_out[c] = op;
        crc_out[c] = crc;
        if (DBG) {
            cyc[0] = clock64() - t_begin;
            for (int k = 0; k < 7; k++) dbg[(size_t)c * 8 + k] = cyc[k];
            dbg[(size_t)c * 8 + 7] = n;
        }
    }
}

// one lane per buffer: chunk frames inside the buffer's frame, the buffer's framed size for k_scan
__global__ __launch_bounds__(256) void k_snap_frame(uint64_t slab_len, uint32_t bs, uint32_t cpb, uint32_t nb,
                                                    const uint32_t *__restrict__ clen, uint32_t *__restrict__ coff,
                                                    BlockMeta *__restrict__ meta) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    uint32_t acc = 10;  // the stream identifier
    for (uint32_t k = 0; k < cpb; k++) {
        const uint32_t c = b * cpb + k;
        const uint32_t n = snap_chunk_len(slab_len, bs, cpb, c);
        if (n == 0) break;
        coff[c] = acc;
        acc += 8u + (snap_stored(n, clen[c]) ? n : clen[c]);
    }
    BlockMeta m;
    m.n = snap_chunk_len(slab_len, bs, cpb, b * cpb) ? 1u : 0u;
    m.is_last = 0;
    m.ntok = 0;
    m.nsub = 0;
    m.payload_bytes = 0;
    m.framed_bytes = m.n ? acc : 0u;
    m.crc = 0;
    m.status = kStatusOk;
    meta[b] = m;
}

// one workgroup per chunk: stream identifier (first chunk of a buffer), header, masked CRC, body
__global__ __launch_bounds__(kSnapEmitThreads) void k_snap_emit(const uint8_t *__restrict__ slab, uint64_t slab_len,
                                                                uint32_t bs, uint32_t cpb,
                                                                const uint8_t *__restrict__ stage,
                                                                const uint32_t *__restrict__ clen,
                                                                const uint32_t *__restrict__ crc,
                                                                const uint32_t *__restrict__ coff,
                                                                const uint64_t *__restrict__ out_off,
                                                                uint8_t *__restrict__ out, uint64_t out_cap) {
    const uint32_t c = blockIdx.x, tid = threadIdx.x, b = c / cpb, k = c % cpb;
    const uint32_t n = snap_chunk_len(slab_len, bs, cpb, c);
    if (n == 0) return;
    const uint32_t cl = clen[c];
    const bool stored = snap_stored(n, cl);
    const uint32_t body = stored ? n : cl;
    const uint64_t at = out_off[b] + coff[c];
    if (at + 8u + body > out_cap) return;  // (reported by the host: the total exceeds the capacity)
    uint8_t *__restrict__ dst = out + at;
    if (k == 0 && tid < 10) {
        const uint64_t lo = 0x50614e73000006ffull;  // ff 06 00 00 73 4e 61 50 70 59: ff 06 00 00 "sNaPpY"
        dst[(int)tid - 10] = (uint8_t)(tid < 8 ? lo >> (8u * tid) : 0x5970u >> (8u * (tid - 8u)));
    }
    if (tid < 8) {
        const uint32_t w0 = (stored ? 0x01u : 0x00u) | ((body + 4u) << 8), w1 = crc[c];
        dst[tid] = (uint8_t)((tid < 4 ? w0 : w1) >> (8u * (tid & 3u)));
    }
    const uint8_t *__restrict__ from = stored ? slab + (uint64_t)b * bs + (uint64_t)k * kSnapChunk
                                              : stage + (size_t)c * kSnapStageStride;
    for (uint32_t i = tid; i < body; i += kSnapEmitThreads) dst[8u + i] = from[i];
}

void launch_snap_chunk(const uint8_t *slab, uint64_t slab_len, uint32_t bs, uint32_t nb, const SnapScratch &ss,
                       hipStream_t stream) {
    const uint32_t cpb = snap_chunks_per_buffer(bs);
    if (ss.dbg)
        hipLaunchKernelGGL(k_snap_chunk<true>, dim3(nb * cpb), dim3(64), 0, stream, slab, slab_len, bs, cpb, ss.stage,
                           ss.clen, ss.crc, ss.dbg);
    else
        hipLaunchKernelGGL(k_snap_chunk<false>, dim3(nb * cpb), dim3(64), 0, stream, slab, slab_len, bs, cpb, ss.stage,
                           ss.clen, ss.crc, (uint64_t *)nullptr);
}

void launch_snap_frame(uint64_t slab_len, uint32_t bs, uint32_t nb, const Scratch &s, const SnapScratch &ss,
                       hipStream_t stream) {
    hipLaunchKernelGGL(k_snap_frame, dim3((nb + 255) / 256), dim3(256), 0, stream, slab_len, bs,
                       snap_chunks_per_buffer(bs), nb, (const uint32_t *)ss.clen, ss.coff, s.meta);
}

void launch_snap_emit(const uint8_t *slab, uint64_t slab_len, uint32_t bs, uint32_t nb, const Scratch &s,
                      const SnapScratch &ss, uint8_t *out, uint64_t out_cap, hipStream_t stream) {
    const uint32_t cpb = snap_chunks_per_buffer(bs);
    hipLaunchKernelGGL(k_snap_emit, dim3(nb * cpb), dim3(kSnapEmitThreads), 0, stream, slab, slab_len, bs, cpb,
                       (const uint8_t *)ss.stage, (const uint32_t *)ss.clen, (const uint32_t *)ss.crc,
                       (const uint32_t *)ss.coff, (const uint64_t *)s.out_off, out, out_cap);
}
