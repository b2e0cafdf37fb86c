// gzpx_deflate.h -- RFC 1951's alphabets and code tables, once.  Included inside namespace gzpx by gzpx_wave.h
// (with GZPX_DEFLATE_WAVE defined, behind wave_sync) and by gzpx_nearopt.hip (the arithmetic alone);
// gzpx_kernels.hip and gzpx_inflate_seg.h see it through gzpx_wave.h.  What libdeflate's compressor decides beyond the
// RFC -- where a block ends, which matches count -- is in gzpx_policy.h, included the same way.
//
//   arithmetic (constexpr, host and device)
//     length_sym / offset_sym       a symbol's (base, extra bits): seg_entry (k_inflate_seg), k_huffman's bit costs,
//                                   k_near_optimal's costs
//     length_slot / offset_slot     a length's / a distance's (slot, extra bits, extra value): length_entry (the LDS tables
//                                   of k_hist and k_emit), the offset codes of k_hist and k_emit, k_near_optimal's costs
//                                   and tallies
//     precode_order                 k_huffman's header writer, seg_header's reader
//     fixed_code_len                seg_header, k_huffman's static cost
//     dyn_header, precode_run       seg_header: the 14 header bits, what a precode symbol means
//     code_shape                    libdeflate's verdict on a code's shape: seg_build
//   wave routines (GZPX_DEFLATE_WAVE; all 64 lanes call them)
//     code_lengths_split            the dynamic header's last step: seg_header
//     code_count_lengths, code_only_symbol   seg_build
//     code_rank_step, canon_codeword         seg_build, make_code (k_huffman)
//
// k_inflate (inflate_entry, inflate_build, its header reader in gzpx_kernels.hip) says all of this in its own text: its
// route lost half a percent with these routines in it, so it is the one place that has to be kept in step by hand.
//
// The decoders keep their own entry layouts and their own rule for the symbols no length and no distance stands
// behind, and the two rules differ on purpose: k_inflate holds libdeflate's verdicts, whose table decodes 286 and 287
// as length 258 like 285 and fails on the use of offset symbol 30 or 31; k_inflate_seg judges nothing, marks all four
// invalid and hands the member that uses one to k_inflate.  So length_sym and offset_sym are asked about 257..285
// and 0..29 alone.
#pragma once

struct DeflateSym {
    uint32_t base, xbits;
};
struct DeflateSlot {
    uint32_t slot, xbits, xval;
};

// Length symbol 257 + slot, slot 0..28: base length and number of extra bits (closed forms of the RFC 1951 table)
__host__ __device__ constexpr DeflateSym length_sym(uint32_t slot) {
    if (slot < 8) return {3 + slot, 0};
    if (slot == 28) return {258, 0};
    const uint32_t xb = (slot - 4) >> 2;
    return {3 + ((4 + (slot & 3)) << xb), xb};
}
// Offset symbol 0..29: base distance and number of extra bits
__host__ __device__ constexpr DeflateSym offset_sym(uint32_t sym) {
    if (sym < 4) return {1 + sym, 0};
    const uint32_t xb = (sym - 2) >> 1;
    return {1 + ((2 + (sym & 1)) << xb), xb};
}

// DEFLATE length slot of len = 3..258: closed form of the RFC 1951 table (258 has a slot of its own, 28)
__host__ __device__ constexpr DeflateSlot length_slot(uint32_t len) {
    const uint32_t x = len - 3;
    if (x < 8) return {x, 0, 0};
    if (x == 255) return {28, 0, 0};
    const uint32_t k = 31u - (uint32_t)__builtin_clz(x);  // 3..7
    const uint32_t xb = k - 2;
    return {4 * k - 4 + ((x >> xb) & 3u), xb, x & ((1u << xb) - 1u)};
}
// DEFLATE offset slot of d = distance - 1 = 0..32767, without a branch (k_hist and k_emit look slots up in waves that
// hold literals and matches, so every side of a branch would run for every token): with k = floor(log2(d | 1)) the
// extra-bit count is max(k - 1, 0) and the slot 2k + the bit below d's top bit, which for d < 4 is d itself
__host__ __device__ constexpr DeflateSlot offset_slot(uint32_t d) {
    const uint32_t k = 31u - (uint32_t)__builtin_clz(d | 1u);
    const int below = (int)k - 1;
    const uint32_t xb = (uint32_t)(below > 0 ? below : 0);
    return {2u * k + ((d >> xb) & 1u), xb, d & ((1u << xb) - 1u)};
}

constexpr bool deflate_lengths_round_trip() {
    for (uint32_t len = 3; len <= 258; len++) {
        const DeflateSlot s = length_slot(len);
        const DeflateSym y = length_sym(s.slot);
        if (s.slot > 28 || s.xbits != y.xbits || s.xval >> y.xbits || y.base + s.xval != len) return false;
    }
    return true;
}
constexpr bool deflate_offsets_round_trip() {
    for (uint32_t sym = 0; sym < 30; sym++) {
        const DeflateSym y = offset_sym(sym);
        const uint32_t lo = y.base, hi = y.base + (1u << y.xbits) - 1u;
        const DeflateSlot a = offset_slot(lo - 1), b = offset_slot(hi - 1);
        if (a.slot != sym || a.xbits != y.xbits || a.xval != 0) return false;
        if (b.slot != sym || b.xbits != y.xbits || y.base + b.xval != hi) return false;
        if (sym == 29 ? hi != 32768u : hi + 1 != offset_sym(sym + 1).base) return false;
    }
    return true;
}
static_assert(deflate_lengths_round_trip(), "every length 3..258: slot -> base + extra gives the length back");
static_assert(deflate_offsets_round_trip(), "the lowest and highest distance of each of the 30 offset slots round-trip");

// RFC 1951's order of the code length code lengths (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13,
// 2, 14, 1, 15), five bits each in two constants: a table indexed by a lane or a loop counter would be an
// array in scratch memory.  i < 19.
__host__ __device__ constexpr uint32_t precode_order(uint32_t i) {
    const uint64_t lo = 0x22caa324e804a30ull, hi = 0x3c2e1346cull;
    return i < 12u ? (uint32_t)(lo >> (5u * i)) & 31u : (uint32_t)(hi >> (5u * (i - 12u))) & 31u;
}

// The fixed code of RFC 1951 3.2.6 in the decoders' layout of lens[320]: literal/length symbol i at [0, 288), the
// offset symbols behind them
__host__ __device__ constexpr uint32_t fixed_code_len(uint32_t i) { return i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5; }

// The 14 bits behind BFINAL and BTYPE of a dynamic block: HLIT, HDIST, HCLEN.  ok: libdeflate's bound, which lets
// 287 and 288 literal/length lengths through (RFC 1951 stops at 286).
struct DynHeader {
    uint32_t nlit, ndist, nclen;
    bool ok;
};
__host__ __device__ constexpr DynHeader dyn_header(uint32_t b) {
    const uint32_t nlit = (b & 31u) + 257, ndist = ((b >> 5) & 31u) + 1, nclen = ((b >> 10) & 15u) + 4;
    return {nlit, ndist, nclen, !(nlit > 286 + 2 || ndist > 32)};
}

// What a precode symbol of `cl` bits means, given the bits from its first one on: how many lengths it stands for, how
// many bits it takes with its extra bits, and the length -- kPrecodePrev for symbol 16, "the length before", which
// the caller refuses in front of the first length.  (The last run of a header may overrun the total: libdeflate
// ignores the excess, and so does whoever writes the run.)
constexpr uint32_t kPrecodePrev = 16;
struct PrecodeRun {
    uint32_t rep, used, val;
};
__host__ __device__ constexpr PrecodeRun precode_run(uint32_t sym, uint32_t bits, uint32_t cl) {
    if (sym == 16) return {3 + ((bits >> cl) & 3u), cl + 2, kPrecodePrev};
    if (sym == 17) return {3 + ((bits >> cl) & 7u), cl + 3, 0};
    if (sym == 18) return {11 + ((bits >> cl) & 127u), cl + 7, 0};
    return {1, cl, sym};
}

// libdeflate's verdict on the shape of a code (build_decode_table), from its Kraft sum in units of 2^-15 and the
// number of codewords of length 1: an over-subscribed code is refused, and so is an incomplete one, with two
// exceptions -- the empty code, in which every bit decodes symbol 0, and a single codeword of length 1, which both bit
// values decode.  inflate_build (gzpx_kernels.hip) states the same rule in its own text.
enum CodeShape { kCodeRefused = 0, kCodeComplete = 1, kCodeDegenerate = 2 };
__host__ __device__ constexpr CodeShape code_shape(uint32_t kraft, uint32_t cnt1) {
    if (kraft == (1u << 15)) return kCodeComplete;
    if (kraft == 0 || (kraft == (1u << 14) && cnt1 == 1)) return kCodeDegenerate;
    return kCodeRefused;
}

#ifdef GZPX_DEFLATE_WAVE
// The dynamic header's last step: tmp[0 .. nlit + ndist) holds the lengths as they were sent, lens[] gets the
// literal/length code at [0, 288) and the offset code at [288, 320), zero where nothing was sent
__device__ __forceinline__ void code_lengths_split(const uint8_t *tmp, uint8_t *lens, uint32_t nlit, uint32_t ndist,
                                                   uint32_t lane) {
    wave_sync();
    uint8_t mine[5];
    for (uint32_t k = 0; k < 5; k++) {
        const uint32_t s = lane + 64 * k;
        uint32_t v = 0;
        if (s < 288) v = s < nlit ? tmp[s] : 0;
        else if (s < 320) v = (s - 288) < ndist ? tmp[nlit + (s - 288)] : 0;
        mine[k] = (uint8_t)v;
    }
    wave_sync();
    for (uint32_t k = 0; k < 5; k++) lens[lane + 64 * k] = mine[k];
    wave_sync();
}

// cnt[l] = how many of lens[0 .. nsyms) are l, l = 1..15, by ballot: the same in every lane
__device__ __forceinline__ void code_count_lengths(const uint8_t *lens, uint32_t nsyms, uint32_t lane, uint32_t (&cnt)[16]) {
#pragma unroll
    for (uint32_t l = 0; l < 16; l++) cnt[l] = 0;
    for (uint32_t base = 0; base < nsyms; base += 64) {
        const uint32_t s = base + lane;
        const uint32_t myl = s < nsyms ? lens[s] : 0;
#pragma unroll
        for (uint32_t l = 1; l <= 15; l++) cnt[l] += (uint32_t)__popcll(__ballot(myl == l));
    }
}

// The one symbol of a code that code_shape calls degenerate and that is not empty: the one whose length is 1
__device__ __forceinline__ uint32_t code_only_symbol(const uint8_t *lens, uint32_t nsyms, uint32_t lane) {
    uint32_t only = 0;
    for (uint32_t base = 0; base < nsyms; base += 64) {
        const uint64_t m = __ballot(base + lane < nsyms && lens[base + lane] == 1);
        if (m) only = base + (uint32_t)__ffsll((long long)m) - 1;
    }
    return only;
}

// Canonical codes, one round of 64 symbols in symbol order: the lane's symbol has length myl (0: none) and gets
// run[myl] + its rank among this round's symbols of that length; run[] moves on past the round.  With run[] started
// at zero that is the rank within the length, to be added to the length's first code; started at the first codes
// (make_code) it is the code itself.  Lengths 1..MAXL.
template <uint32_t MAXL>
__device__ __forceinline__ uint32_t code_rank_step(uint32_t myl, uint32_t (&run)[16], uint64_t lane_below) {
    uint32_t rank = 0;
#pragma unroll
    for (uint32_t l = 1; l <= MAXL; l++) {
        const uint64_t m = __ballot(myl == l);
        if (myl == l) rank = run[l] + (uint32_t)__popcll(m & lane_below);
        run[l] += (uint32_t)__popcll(m);
    }
    return rank;
}
// ... and the codeword as DEFLATE sends it, first bit lowest
__device__ __forceinline__ uint32_t canon_codeword(uint32_t code, uint32_t len) { return __brev(code) >> (32 - len); }
#endif
