// gzpx_crc.h -- the CRC arithmetic of the library, once: CRC-32 (gzip) and CRC-32C (Snap, the batch checksums), both
// reflected, the polynomial a template argument.  Two includers.  gzpx_wave.h, inside namespace gzpx, behind dword4 and
// with GZPX_CRC_KERNELS defined: that puts it in front of every kernel of gzpx_kernels.hip and of every header included
// there.  gzpx_api.cpp, for the host half alone.
//
//   host and device   crc_mulmod<P> (the one GF(2) product), CrcPow / crc_pow_table<P> / crc_xpow8<P> (the one power table
//                     and x^(8 m) out of it)
//   device            crc_tables_fill<P> (slice-by-4 tables in LDS), crc_byte / crc_word (the two steps over them),
//                     crc_bytes (a run of bytes at any alignment), crc_seg256 (one whole 256-byte segment from global
//                     memory: the only place that decides what may be read around a segment)
//
// Who calls them: crc32_workgroup (k_dcrc32) and crc32_direct (k_crc32) in gzpx_kernels.hip, k_lzcopy's tile CRC
// (gzpx_inflate_seg.h), ck_crc_tile (gzpx_cksum.h), snap_crc32c_wave (gzpx_snap.h); crc32_combine and crc_consts on
// the host.  The tables are passed as a reference to the array inside the caller's __shared__ object, so that the
// loads stay LDS loads once the call is inlined.
#pragma once

constexpr uint32_t kCrcPoly32 = 0xEDB88320u, kCrcPoly32c = 0x82F63B78u;  // reflected

// a * b mod P, both in the reflected representation of the CRC register (bit 31 is x^0).  The bits of a are tested, b
// is shifted: of the forms the library had, this one compiles to the fewest instructions in every kernel that uses it.
template <uint32_t P>
__host__ __device__ __forceinline__ uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ (P & (0u - (b & 1u)));
    }
    return p;
}

// sq[k] = x^(8 * 2^k) mod P: what x^(8 m) is a product of, for any 64-bit m.  Made once per polynomial on the host; the
// kernels that need powers of any m get it by value and keep it in LDS, the others get the few entries they use
// (CrcConsts).
struct CrcPow {
    uint32_t sq[64];
};
template <uint32_t P>
inline CrcPow crc_pow_table() {
    CrcPow t;
    t.sq[0] = 0x00800000u;  // x^8
    for (int k = 1; k < 64; k++) t.sq[k] = crc_mulmod<P>(t.sq[k - 1], t.sq[k - 1]);
    return t;
}
// x^(8 m) mod P
template <uint32_t P>
__host__ __device__ __forceinline__ uint32_t crc_xpow8(const uint32_t (&sq)[64], uint64_t m) {
    uint32_t r = 0x80000000u;  // 1
    for (uint32_t k = 0; m; k++, m >>= 1)
        if (m & 1u) r = crc_mulmod<P>(r, sq[k]);
    return r;
}

#ifdef GZPX_CRC_KERNELS
// t[0] is the byte table, t[j][i] the register behind byte i and j zero bytes.  Every thread of the workgroup calls it;
// the tables are complete behind the caller's next barrier (the one inside is between t[0] and the other three).
template <uint32_t P>
__device__ __forceinline__ void crc_tables_fill(uint32_t (&t)[4][256], uint32_t tid, uint32_t nthreads) {
    for (uint32_t i = tid; i < 256; i += nthreads) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (P & (0u - (c & 1u)));
        t[0][i] = c;
    }
    __syncthreads();
    for (uint32_t i = tid; i < 256; i += nthreads) {
        const uint32_t t0 = t[0][i];
        const uint32_t t1 = (t0 >> 8) ^ t[0][t0 & 0xFFu];
        const uint32_t t2 = (t1 >> 8) ^ t[0][t1 & 0xFFu];
        const uint32_t t3 = (t2 >> 8) ^ t[0][t2 & 0xFFu];
        t[1][i] = t1;
        t[2][i] = t2;
        t[3][i] = t3;
    }
}

__device__ __forceinline__ uint32_t crc_byte(const uint32_t (&t)[4][256], uint32_t c, uint32_t byte) {
    return (c >> 8) ^ t[0][(c ^ byte) & 0xFFu];
}
__device__ __forceinline__ uint32_t crc_word(const uint32_t (&t)[4][256], uint32_t c, uint32_t w) {
    c ^= w;
    return t[3][c & 0xFFu] ^ t[2][(c >> 8) & 0xFFu] ^ t[1][(c >> 16) & 0xFFu] ^ t[0][c >> 24];
}

// The register behind s[0, n), from c: bytes up to a dword boundary, whole dwords, bytes.  Reads s[0, n) alone.
__device__ __forceinline__ uint32_t crc_bytes(const uint32_t (&t)[4][256], const uint8_t *__restrict__ s, uint32_t n,
                                              uint32_t c) {
    uint32_t i = 0;
    for (; i < n && ((uintptr_t)(s + i) & 3u); i++) c = crc_byte(t, c, s[i]);
    for (; i + 4 <= n; i += 4) c = crc_word(t, c, *(const uint32_t *)(s + i));
    for (; i < n; i++) c = crc_byte(t, c, s[i]);
    return c;
}

// The register behind the 256 bytes s[0, 256), from c: sixteen 16-byte loads of dword-aligned addresses, the byte
// alignment of s taken out with v_alignbyte.  128 bytes (eight loads in flight) per step: a lane uses every cache line
// it fetches while it is still on chip -- with one 16-byte load per step the lanes' 256-byte stride made k_crc32 fetch
// its input four times over (PMC: 2.26 GB for 0.58 GB; 64 bytes per step: 1.21 GB).
// Reads: the dwords that hold bytes of the segment, and the one in front of them that shares s's dword -- bytes of the
// same buffer, or of the dword the buffer's first byte lies in.  With s dword-aligned the last load would reach one
// dword past the segment, which nothing needs; `ends_buffer` (the segment's last byte is the buffer's last) says that
// this dword is not the caller's to read, and then it is not loaded.
__device__ __forceinline__ uint32_t crc_seg256(const uint32_t (&t)[4][256], const uint8_t *__restrict__ s,
                                               bool ends_buffer, uint32_t c) {
    const uint32_t mis = (uint32_t)((uintptr_t)s & 3u);
    const uint32_t *q = (const uint32_t *)(s - mis);
    const bool no_lookahead = ends_buffer && mis == 0;  // q[64] lies behind the buffer
    uint32_t carry = q[0];
    for (uint32_t g = 0; g < 2; g++) {
        dword4 v[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            if (g == 1 && k == 7 && no_lookahead) {
                v[k].x = q[61];
                v[k].y = q[62];
                v[k].z = q[63];
                v[k].w = 0;
            } else {
                v[k] = *(const dword4 *)(q + 1 + 32 * g + 4 * k);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            c = crc_word(t, c, __builtin_amdgcn_alignbyte(v[k].x, carry, mis));
            c = crc_word(t, c, __builtin_amdgcn_alignbyte(v[k].y, v[k].x, mis));
            c = crc_word(t, c, __builtin_amdgcn_alignbyte(v[k].z, v[k].y, mis));
            c = crc_word(t, c, __builtin_amdgcn_alignbyte(v[k].w, v[k].z, mis));
            carry = v[k].w;
        }
    }
    return c;
}
#endif  // GZPX_CRC_KERNELS
