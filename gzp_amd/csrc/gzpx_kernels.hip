// gzpx_kernels.hip -- hand-written HIP kernels (gfx950 / CDNA4) for gzp's per-block encode and
// decode: libdeflate DEFLATE (levels 0-9; 10-12: gzpx_nearopt.hip) + CRC-32 + BGZF/Mgzip framing, and inflate with the
// per-block CRC check; thousands of blocks per launch.
//
// What this replaces (reference file:line, relative to the gzp tree):
//   Bgzf::encode / Mgzip::encode                  src/deflate.rs:613-626, 463-472
//   bgzf::compress / mgzip::compress              src/bgzf.rs:204-237 ; src/mgzip.rs:187-218
//   libdeflater::Compressor::deflate_compress     call site src/bgzf.rs:214-216
//   libdeflater::Crc                              call site src/bgzf.rs:224-225
//   header_inner / footer / BGZF_EOF              src/bgzf.rs:274-303, :233-234, :24-38
//   bgzf::decompress + decode_block               src/bgzf.rs:103-121 ; src/par/decompress.rs:162-186
//
// MI355X design: libdeflate's level-1 matchfinder inserts EVERY position into a
// 2-way hash bucket in order, so the two match candidates of a position are a pure function of
// the input ("the two most recent earlier positions with the same 15-bit hash, within 32767
// bytes") and do not depend on the parse.  That turns the sequential compressor into a pipeline
// of data-parallel stages, each a kernel over all blocks of a slab:
//   k_candidates   16 waves / CU    : (persistent: a workgroup walks its share of the blocks) LDS-resident
//                                     128 KiB bucket table that is never cleared, ordered atomicMax chain,
//                                     1024 positions per ticket turn, no barrier between blocks
//   k_mparse       1024 thr / CU    : (blocks <= 64 KiB; persistent) match on demand: the block's bytes and
//                                     half its candidate distances in LDS, the next block's on their way in
//                                     registers; the greedy parse as a speculative walk over 32-position
//                                     segments that searches only where it lands; every lane writes its
//                                     own tokens
//   k_match        1024 thr / block : (larger blocks, and blocks k_mparse hands back) block input in LDS;
//                                     both candidates of EVERY position extended by one lockstep
//                                     loop; run groups for long runs
//   k_parse        1024 thr / block : (same blocks) per-position match lengths in LDS; the greedy parse
//                                     as a speculative walk over 64-position segments, then the
//                                     position-parallel token build
//   k_hist         256 thr  / block : symbol frequencies per DEFLATE sub-block
//   k_huffman      one wave / block : libdeflate's length-limited Huffman construction, header
//                                     RLE, exact cost comparison (dynamic / static / stored)
//   k_crc32        256 thr  / block : 256-byte segments straight from global memory, slice-by-4, one GF(2)
//                                     combine tree per 64 KiB (side stream, beside the match kernels)
//   k_scan         one workgroup    : exclusive scan of framed sizes -> output offsets
//   k_emit         1024 thr / block : bit-exact bitstream assembly in LDS, coalesced write-out
// Levels 2-4 swap k_match / k_parse for k_match_hc / k_parse_hc (hc_matchfinder chains, block
// splitting), levels 5-9 for k_match_hc / k_parse_lazy (the lazy and lazy2 parsers); ParDecompress
// is k_dinit / k_dscan / k_inflate / k_dcrc32.
// Integer/byte work only: no MFMA; the path is bound by instruction issue, then LDS.
//
// What more than one stage or more than one of the headers included below uses -- wave_sync, the scans, dword4, the
// experiment counters, and through it gzpx_policy.h (libdeflate's parsing rules: lz_hash, where a sub-block ends, the
// minimum match length), gzpx_deflate.h and gzpx_crc.h -- is in gzpx_wave.h, in front of them all.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <cstring>

#include "gzpx_device.h"

namespace gzpx {

#include "gzpx_wave.h"

// ------------------------------------------------------------------------------------------
// k_init_meta: cut the slab into blocks the way ParCompress::write / flush_last do
// (src/par/compress.rs:415-416, :333-341): full `block_size` cuts, the remainder (possibly a
// full block, possibly empty when the slab is empty) last.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ BlockMeta block_meta_of(const Config &cfg, uint64_t slab_len, uint32_t nb, uint32_t is_last,
                                                   uint32_t b) {
    const uint64_t begin = (uint64_t)b * cfg.block_size;
    uint64_t len = slab_len > begin ? slab_len - begin : 0;
    if (len > cfg.block_size) len = cfg.block_size;
    BlockMeta m;
    m.n = (uint32_t)len;
    m.is_last = (is_last && b == nb - 1) ? 1u : 0u;
    m.ntok = 0;
    m.nsub = 0;
    m.payload_bytes = 0;
    m.framed_bytes = 0;
    m.crc = 0;
    m.status = kStatusOk;
    return m;
}

// (Level 0 and the decompressor's CRC pass only: at levels >= 1 the first k_candidates launch of a batch
// does this for its own block -- one launch and one dependent load at the head of every workgroup less.)
__global__ void k_init_meta(Config cfg, uint64_t slab_len, uint32_t nb, uint32_t is_last,
                            BlockMeta *meta, uint32_t *redo) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    // Scratch.redo[0] counts the blocks on the encode side's hand-back list (level 1: from k_mparse to the dense pair;
    // levels 3-4: the stale ones, from k_parse_hc to k_match_hc_stale).  The levels that come here read no such list;
    // the list is left empty, as the first k_candidates launch leaves it at the others.
    if (b == 0 && redo) redo[0] = 0;
    if (b >= nb) return;
    meta[b] = block_meta_of(cfg, slab_len, nb, is_last, b);
}

// ------------------------------------------------------------------------------------------
// k_candidates: ht_matchfinder's bucket table (2^15 buckets x 2 entries), restated as a chain:
// the two entries of a bucket are always "the previous position with this hash" and "the one
// before that", so it is enough to produce, for every position p, the distance d0[p] to its
// predecessor in its bucket; the older candidate is the predecessor's predecessor
// (d1 = d0[p] + d0[p - d0[p]]), which k_match_parse reads from the same array.
// One workgroup per block, 128 KiB table in LDS, one word per bucket = (newest position + 1), 0 =
// empty.  Positions only grow, so "newest" is an unsigned maximum, and liveness (libdeflate:
// cur_node > cutoff) is the plain distance test p - c <= 32767 on 32-bit positions -- the window
// slide of the reference never changes the outcome of a lookup, so none is needed.
//
// Fast kernel (k_candidates): every lane does  old = atomicMax(&tab[h], p + 1).
// The LDS applies same-address atomics of one instruction in ascending lane order (measured:
// tools/probes/lds_atomic_order.hip, 2000/2000 patterns), so `old` already is the lane's
// predecessor in its bucket -- whether that predecessor sits in an earlier step or in a lower
// lane of the same instruction.  No cross-lane matching is needed, and kCandSteps steps
// (kCandSteps * 64 positions) of atomics are kept in flight per iteration; sixteen waves (four per
// SIMD) take turns at the table so that only the atomic phase is serial.  The ordering
// assumption is CHECKED, never trusted: a lane that is handed a predecessor >= its own position
// flags the block, and one wave of the workgroup then redoes it in the same table with
// cand_block_safe (ballot match-any, order-independent) before the kernel ends.
// Output: cand[p] = d0 (u16, 0 = no live predecessor).
// ------------------------------------------------------------------------------------------
constexpr uint32_t kBuckets = 1u << 15;
// (measurement builds set another pair: python tools/build_variant.py w16s8 -DGZPX_CAND_STEPS=8)
#ifndef GZPX_CAND_STEPS
#define GZPX_CAND_STEPS 16
#endif
#ifndef GZPX_CAND_WAVES
#define GZPX_CAND_WAVES 16
#endif
constexpr uint32_t kCandSteps = GZPX_CAND_STEPS;  // steps per iteration; also the depth of the input prefetch

// aligned dword pair covering in[p .. p+3] (in32 = the block's bytes rounded down to a dword
// boundary, mis = bytes skipped by that rounding).  Unconditional (index clamped to the block's
// last dword) so that the number of loads in flight is static and the compiler can wait with
// exact vmcnt values instead of vmcnt(0).  (Tried: ONE 8-byte load of the 4-byte-aligned pair -- a hashed
// position never starts in the block's last dword, so one clamp would do -- four VALU less per 64
// positions, and k_candidates 0.56 -> 0.68 ms: under-aligned dwordx2 loads are the slower way.)
__device__ __forceinline__ uint2 cand_fetch(const uint32_t *__restrict__ in32, uint32_t mis,
                                            uint32_t p, uint32_t wmax) {
    const uint32_t w = (p + mis) >> 2;  // bytes p..p+4 lie inside dwords w, w+1
    uint2 v;
    v.x = in32[w < wmax ? w : wmax];
    v.y = in32[w + 1 < wmax ? w + 1 : wmax];
    return v;
}

// Waves per workgroup x steps per turn, measured on the 550 MiB slab (ms per launch, level 1, average
// (min-max) of 12 launches under a kernel trace, with the scalar cursor and the interior body):
//   16 x 8: 0.562 (0.556-0.569),  8 x 32: 0.532 (0.524-0.543),  16 x 16: 0.495 (0.490-0.504)  <- kept.
// 16 x 20 needs 125 VGPRs in modes 0 and 1 and spills three dwords in modes 2 and 3; 16 x 24 spills in
// every mode: neither was run.  (Before the scalar cursor, when the work around the turn was three
// times as many VALU instructions: 4 x 32: 1.00, 8 x 32: 0.74, 12 x 32: 0.84, 16 x 8: 0.73, 16 x 16: 0.64,
// and with the persistent workgroups 16 x 16: 0.54.)  The work AROUND the turn (loads, hashing,
// distance, stores) spreads over the waves; the turn itself -- sixteen atomics and the hand-off of
// the ticket -- is what a block waits for now, so a shorter turn (16 x 8) pays the hand-off twice as
// often and fewer waves (8 x 32) leave the table idle while a wave hashes.  16 x 16 is what the 512
// VGPRs of a SIMD lane allow (ring + address / value / result of every step stay in registers: 95).
constexpr uint32_t kCandWaves = GZPX_CAND_WAVES;  // sixteen: four per SIMD; they take turns at the table

// Which chain a candidate pass builds (MODE):
//   0  level 1, ht_matchfinder: 15-bit hash of 4 bytes
//   1  levels 2-4, hc_matchfinder hash3_tab: 15-bit hash of 3 bytes (single previous position)
//   2  levels 2-4, hc_matchfinder hash4_tab / next_tab: 16-bit hash of 4 bytes, buckets 0..32767
//   3  same, buckets 32768..65535 (the 2^16-bucket table does not fit LDS, so it takes two passes;
//      every position belongs to exactly one of them)
// Position 0 is filed under bucket 0 in every table (libdeflate starts with next_hash(es) = 0).
template <int MODE>
__device__ __forceinline__ bool cand_bucket(uint32_t v, uint32_t p, uint32_t &h) {
    if (MODE == 0) {
        h = p != 0 ? lz_hash(v, 15) : 0;
        return true;
    } else if (MODE == 1) {
        h = p != 0 ? lz_hash(v & 0xFFFFFFu, 15) : 0;
        return true;
    } else {
        const uint32_t h16 = p != 0 ? lz_hash(v, 16) : 0;
        h = h16 & 32767u;
        return MODE == 2 ? h16 < 32768u : h16 >= 32768u;
    }
}

// Order-independent restatement for a block whose order check failed in k_candidates (expected: never):
// lanes of a step that share a bucket are linked in position order with a 15-round ballot
// match-any; the last lane of each group rewrites the bucket (position mod 65536, with a dead
// marker 0x8000 behind that is refreshed every 32768 positions).
template <int MODE>
__device__ __forceinline__ void cand_step_safe(uint32_t *tab, uint32_t mis, uint32_t base,
                                               uint32_t lane, uint32_t n, uint2 raw,
                                               uint16_t *__restrict__ cand) {
    const uint32_t p = base + lane;
    uint32_t h = 0;
    const bool owns = cand_bucket<MODE>(__builtin_amdgcn_alignbyte(raw.y, raw.x, (p + mis) & 3u), p, h);
    const bool valid = owns && p + 5 <= n;  // positions the matchfinder hashes (REQUIRED_NBYTES = 5)
    if (!valid) h = 0;
    uint32_t c0 = tab[h];
    uint64_t same = __ballot(valid);
    for (int bit = 0; bit < 15; bit++) {
        const bool one = (h >> bit) & 1u;
        const uint64_t m = __ballot(one);
        same &= one ? m : ~m;
    }
    const uint64_t below = same & ((1ull << lane) - 1ull);
    const bool is_last_of_group = ((same >> lane) >> 1) == 0;
    if (below) c0 = (base + 63u - (uint32_t)__clzll((long long)below)) & 0xFFFFu;
    wave_sync();  // every lane has read its bucket before any lane rewrites one
    if (valid && is_last_of_group) tab[h] = p & 0xFFFFu;
    wave_sync();
    uint32_t d0 = (p - c0) & 0xFFFFu;
    if (d0 > 32767u) d0 = 0;
    if (MODE < 2 || valid || (MODE == 2 && p + 5 > n)) cand[p] = (uint16_t)(valid ? d0 : 0u);
}

// One wave redoes the block in `tab` (the workgroup's table, free again): k_candidates' fallback.
template <int MODE>
__device__ void cand_block_safe(uint32_t *tab, const uint32_t *in32, uint32_t mis, uint32_t wmax, uint32_t n,
                                uint32_t lane, uint16_t *__restrict__ cand) {
    for (uint32_t i = lane; i < kBuckets; i += 64) tab[i] = 0x8000u;
    wave_sync();
    for (uint32_t base = 0; base < n; base += 64) {
        if (base != 0 && (base & 32767u) == 0) {
            // sweep: entries farther than 32767 behind `base` become "dead for the next
            // 32768 positions" (the analogue of libdeflate's window slide)
            const uint32_t dead = (base + 0x8000u) & 0xFFFFu;
            for (uint32_t i = lane; i < kBuckets; i += 64) {
                const uint32_t e = tab[i];
                const uint32_t a = (base - e) & 0xFFFFu;
                if (a == 0 || a > 32767u) tab[i] = dead;
            }
            wave_sync();
        }
        cand_step_safe<MODE>(tab, mis, base, lane, n, cand_fetch(in32, mis, base + lane, wmax), cand);
    }
}

// One workgroup per CU walks the blocks blockIdx.x, + gridDim.x, ... WITHOUT ever clearing the table or
// meeting at a barrier: a block's positions are filed as vbase + p + 1 with vbase growing by n + 32768 from
// block to block, so whatever an earlier block left in a bucket is farther than the window behind every
// position of this one and fails the liveness test like any other stale entry; and the turn counter runs on
// through the blocks, so a wave that has done its last turn of a block goes straight on to its first turn
// of the next (its input already prefetched) while slower waves still finish the old one.  (One workgroup
// per block: every block paid for 128 KiB of LDS zeroing, the first loads' round trip, the wait for its
// slowest wave and the dispatch of the next workgroup -- 0.64 -> 0.xx ms on the 550 MiB slab.)
template <int MODE>
__global__ __launch_bounds__(64 * kCandWaves) void k_candidates(Config cfg,
                                                                 const uint8_t *__restrict__ slab,
                                                                 BlockMeta *__restrict__ meta,
                                                                 uint16_t *__restrict__ cand_all,
                                                                 uint64_t slab_len, uint32_t nb, uint32_t is_last,
                                                                 uint32_t *__restrict__ redo, uint32_t *__restrict__ claim) {
    __shared__ uint32_t tab[kBuckets + 64];  // 128 KiB + one spare word per lane for lanes without a bucket
    __shared__ uint32_t turn;               // index of the iteration (counted through the blocks) whose atomics may go next
    __shared__ uint32_t bad_any;            // some wave saw the order check fail
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    // (read from lane 0, so that the compiler knows it as wave-uniform: the cursor below, settle, the block
    // geometry and the loop branches are then scalar registers, scalar arithmetic and scalar branches)
    const uint32_t wave = uniform(tid >> 6);
    constexpr uint32_t kIterPos = 64 * kCandSteps;
    auto block_len = [&](uint32_t blk) -> uint32_t {  // k_init_meta's cut
        const uint64_t begin = (uint64_t)blk * cfg.block_size;
        const uint64_t len = slab_len > begin ? slab_len - begin : 0;
        return (uint32_t)(len > cfg.block_size ? cfg.block_size : len);
    };
    if (MODE <= 1) {  // the first launch of a batch (hash4 / hash3 pass): cut the slab, k_init_meta's rules
        for (uint32_t blk = blockIdx.x + tid * gridDim.x; blk < nb; blk += 64 * kCandWaves * gridDim.x)
            meta[blk] = block_meta_of(cfg, slab_len, nb, is_last, blk);
        if (blockIdx.x == 0 && tid == 0) redo[0] = 0;  // level 1: nothing handed back to the dense kernels yet
        if (blockIdx.x == 0 && tid < 8) claim[tid] = 0;  // the ticket counters of the kernels behind this one (k_mparse)
    }
    for (uint32_t i = tid; i < kBuckets + 64; i += 64 * kCandWaves) tab[i] = 0;
    if (tid == 0) {
        turn = 0;
        bad_any = 0;
    }
    __syncthreads();

    // The table is one LDS array, so the atomics of iteration i+1 must reach it after those of
    // iteration i -- but hashing / input prefetch before and distance / store work after are
    // independent.  Wave w owns iterations w, w+16, ... of every block; a ticket in LDS (`turn`)
    // serialises only the atomic phase, so fifteen waves hash, prefetch and store while one is at the table.
    //
    // A wave's cursor: block b (its geometry), iteration `it` of that block, and the block's bases
    // (vbase for positions, ibase for turns -- the same in every wave: they depend on the block lengths only).
    struct Cursor {
        uint32_t b, it, n, n_iters, vbase, ibase;
    };
    // the first block at or behind `c.b` (in this workgroup's sequence) in which this wave owns an iteration;
    // false = none left.  Blocks of at most cfg.passthrough bytes have no matchfinding and take no turns.
    auto settle = [&](Cursor &c) -> bool {
        for (;;) {
            if (c.b >= nb) return false;
            c.n = block_len(c.b);
            c.n_iters = c.n > cfg.passthrough ? (c.n + kIterPos - 1) / kIterPos : 0u;
            if (c.it < c.n_iters) return true;
            if (c.n_iters) {
                c.vbase += c.n + 32768u;
                c.ibase += c.n_iters;
            }
            c.b += gridDim.x;
            c.it = wave;
        }
    };
    const bool force_safe = (cfg.debug & 1u) != 0;  // diagnostics: the fallback on every block, instead of the fast form
    const bool clamp_all = (cfg.debug & 128u) != 0;  // diagnostics: every iteration through the clamped body (A/B timing)
    // An iteration has two bodies.  The INTERIOR one has no clamps and no per-position tests; it is taken
    // (wave-uniformly) when
    //   * the iteration is not the block's first (position 0 is filed under bucket 0), and
    //   * base0 + kIterPos + 16 <= n  (base0 = it * kIterPos, the iteration's first position).
    // Then every position p <= base0 + kIterPos - 1 of the iteration is hashed (p + 5 <= n), and the reads stay
    // inside the block's own bytes: the last dword touched is w + 1 with w = (base0 + kIterPos - 1 + mis) >> 2,
    // counted from in - mis, so its last byte lies at 4 * (w + 1) + 3 - mis <= base0 + kIterPos + 6 from the
    // block's first byte (the worst case is mis = 1), which is below n.  The first dword read starts at
    // in - mis + base0 with base0 >= kIterPos: behind the block's first byte.  Every other iteration -- a block's
    // first, its last one or two, everything under debug bit 7 -- takes the clamped body.  Both take the same one turn.
    auto interior = [&](const Cursor &c) -> bool {
        return !clamp_all && c.it != 0 && c.it * kIterPos + kIterPos + 16u <= c.n;
    };
    uint2 ring[kCandSteps];
    // the input of iteration c, one step per ring slot
    auto prefetch = [&](const Cursor &c) {
        const uint8_t *in = slab + (uint64_t)c.b * cfg.block_size;
        const uint32_t mis = (uint32_t)((uintptr_t)in & 3u);
        const uint32_t *in32 = (const uint32_t *)(in - mis);
        if (interior(c)) {
            // p + mis = (base0 + 64 k) + (lane + mis) and base0 + 64 k is a multiple of four: the lane's dword of
            // step k is its dword of step 0 plus 16 k, so one address per lane and an immediate offset per load.
            // The upper dword goes through an offset of its own that the compiler cannot see through: left
            // alone it merges the pair into one 4-byte-aligned dwordx2 load, the slower way (see cand_fetch).
            const uint8_t *row = (const uint8_t *)(in32 + c.it * (kIterPos / 4));  // (uniform)
            const uint32_t lo = (lane + mis) & ~3u;
            uint32_t hi = lo + 4;
            GZPX_PIN_VGPR(hi);
#pragma unroll
            for (uint32_t k = 0; k < kCandSteps; k++) {
                ring[k].x = *(const uint32_t *)(row + lo + 64 * k);
                ring[k].y = *(const uint32_t *)(row + hi + 64 * k);
            }
            GZPX_KEEP_ARM_APART();
        } else {
#pragma unroll
            for (uint32_t k = 0; k < kCandSteps; k++)
                ring[k] = cand_fetch(in32, mis, c.it * kIterPos + k * 64 + lane, (mis + c.n - 1) >> 2);
        }
    };
    Cursor cur{blockIdx.x, wave, 0, 0, 32768u, 0};  // (vbase starts a window's length up: an empty bucket, 0, reads as dead too)
    bool live = !force_safe && settle(cur);
    bool bad = false;
    if (live) prefetch(cur);
    while (live) {  // (wave-uniform)
        const uint32_t n = cur.n, base0 = cur.it * kIterPos, vbase = cur.vbase, my_turn = cur.ibase + cur.it;
        const uint32_t mis = (uint32_t)((uintptr_t)(slab + (uint64_t)cur.b * cfg.block_size) & 3u);
        uint16_t *cand = cand_all + (uint64_t)cur.b * cfg.stride;
        const bool inner = interior(cur);
        // The serial phase must be nothing but the atomics: a lone wave issues about one dependent
        // instruction per ten cycles, so every instruction inside the turn costs every wave.
        // LDS byte address and value of every step are therefore finished (and pinned in registers)
        // before the wave asks for its turn; lanes without a bucket aim a zero at a spare word.
        uint32_t addr[kCandSteps], val[kCandSteps], old[kCandSteps];
        bool mine[kCandSteps];  // this pass owns the position's bucket
        if (inner) {
            const uint32_t sh = (lane + mis) & 3u;  // (p + mis) & 3 of every step: 64 k + base0 is a multiple of four
            const uint32_t v0 = vbase + base0 + lane + 1;
#pragma unroll
            for (uint32_t k = 0; k < kCandSteps; k++) {
                const uint32_t v = __builtin_amdgcn_alignbyte(ring[k].y, ring[k].x, sh);
                if (MODE <= 1) {  // p != 0, p + 5 <= n: every position has its bucket
                    mine[k] = true;
                    addr[k] = 4u * lz_hash(MODE == 0 ? v : v & 0xFFFFFFu, 15);
                    val[k] = v0 + 64 * k;
                } else {
                    const uint32_t h16 = lz_hash(v, 16);
                    mine[k] = MODE == 2 ? h16 < 32768u : h16 >= 32768u;
                    addr[k] = 4u * (mine[k] ? h16 & 32767u : kBuckets + lane);
                    val[k] = mine[k] ? v0 + 64 * k : 0u;
                }
                GZPX_PIN_VGPR(addr[k]);
                GZPX_PIN_VGPR(val[k]);
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < kCandSteps; k++) {
                const uint32_t p = base0 + k * 64 + lane;
                const uint32_t v = __builtin_amdgcn_alignbyte(ring[k].y, ring[k].x, (p + mis) & 3u);
                uint32_t hk;
                mine[k] = cand_bucket<MODE>(v, p, hk) && p + 5 <= n;
                // byte offset into the table; a lane without a bucket (the other hash4 pass owns it) aims its
                // zero at a spare word of its own -- one shared spare word made half the lanes of every
                // atomic hit the same address, which the LDS serialises (hash4 passes 1.43 / 1.25 ms against
                // 1.00 ms for the hash3 pass)
                addr[k] = 4u * (mine[k] ? hk : kBuckets + lane);
                val[k] = mine[k] ? vbase + p + 1 : 0u;
                GZPX_PIN_VGPR(addr[k]);
                GZPX_PIN_VGPR(val[k]);
            }
        }
        // this wave's next iteration: of this block, or the first it owns in a later one
        Cursor nxt = cur;
        nxt.it += kCandWaves;
        const bool more = settle(nxt);
        if (more) prefetch(nxt);
        // (the turn: one place for both bodies, so that every iteration takes exactly one, with the same number)
        wave_sync();
        while (__hip_atomic_load(&turn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != my_turn)
            __builtin_amdgcn_s_sleep(1);
        // newest position per bucket; the return value is the predecessor
#pragma unroll
        for (uint32_t k = 0; k < kCandSteps; k++)
            old[k] = atomicMax((uint32_t *)((uint8_t *)tab + addr[k]), val[k]);
        // the returned values are in registers => every atomic of this iteration has been applied
        uint32_t seen = 0;
#pragma unroll
        for (uint32_t k = 0; k < kCandSteps; k++) seen |= old[k];
        bad |= seen > 0x7FFFFFFFu;  // (never) -- orders the ticket store after the atomics' return
        wave_sync();
        if (lane == 0) __hip_atomic_store(&turn, my_turn + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (inner) {
            uint16_t *out = cand + base0 + lane;  // step k's slot: out[64 k], an immediate offset
#pragma unroll
            for (uint32_t k = 0; k < kCandSteps; k++) {
                // val[k] = vbase + p + 1 is still in its register: one subtraction gives the distance, and the
                // order check (old >= val <=> a difference that is not positive; values stay below 2^31, see
                // `seen`) and the window test read it.  A lane without a bucket has 0 - 0 here and is left out.
                const uint32_t d0 = val[k] - old[k];
                bad |= (MODE < 2 || mine[k]) && (int32_t)d0 <= 0;
                if (MODE < 2 || mine[k]) out[64 * k] = (uint16_t)(d0 > 32767u ? 0u : d0);  // (every position is hashed)
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < kCandSteps; k++) {
                const uint32_t p = base0 + k * 64 + lane;
                bad |= old[k] > vbase + p;  // handed a predecessor that is not earlier: LDS order assumption broken
                uint32_t d0 = vbase + p + 1 - old[k];  // (an empty bucket, or an earlier block's entry: > 32767)
                if (d0 > 32767u) d0 = 0;  // farther than the window: dead
                // p < cfg.stride (padded by >= one iteration).  The two hash4 passes own disjoint
                // positions; positions that are never hashed are zeroed by the first of them.
                if (MODE < 2 || mine[k] || (MODE == 2 && p + 5 > n)) cand[p] = (uint16_t)d0;
            }
        }
        cur = nxt;
        live = more;
    }
    // (expected: never) the order check failed somewhere: one wave redoes this workgroup's blocks,
    // order-independently, in the same table -- in this launch, so that no second kernel has to look for them
    if (__ballot(bad) && lane == 0) atomicOr(&bad_any, 1u);
    __syncthreads();
    if ((bad_any || force_safe) && wave == 0) {
        for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
            const uint32_t n = block_len(b);
            if (n <= cfg.passthrough) continue;
            const uint8_t *in = slab + (uint64_t)b * cfg.block_size;
            const uint32_t mis = (uint32_t)((uintptr_t)in & 3u);
            cand_block_safe<MODE>(tab, (const uint32_t *)(in - mis), mis, (mis + n - 1) >> 2, n, lane,
                                  cand_all + (uint64_t)b * cfg.stride);
            wave_sync();
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_match: ht_matchfinder_longest_match for EVERY position of a block in parallel.
//   1024 threads per block, ~74 KiB of LDS (a window of the block's bytes + one bit per
//   position), so two workgroups = 32 waves share a CU and hide each other's LDS / L2 latency.
//   Blocks up to 64 KiB are one tile; larger blocks are walked in 32 KiB tiles whose LDS window
//   also holds the 32 KiB of history a match may reach back into.
//   d0 = distance to the bucket predecessor (from k_candidates), d1 = d0 + the predecessor's own
//   d0; 4-byte check + lz_extend run out of LDS with aligned dword reads + v_alignbyte.
//   Output: len8[p] (0 = no match, else length - 3), val[p] (the winning distance, or the literal
//   byte where there is no match) and one bit per position "a match starts here" (wave ballots).
// ------------------------------------------------------------------------------------------
constexpr uint32_t kSeg = 272;
constexpr uint32_t kInWords = kTile / 4 + 132;  // 64 KiB window + max match + alignment slack
constexpr uint32_t kMpThreads = 1024;
constexpr uint32_t kMpWaves = kMpThreads / 64;

// (two aligned reads + v_alignbyte on purpose: gfx950 accepts an under-aligned ds_read_b32, and the
// compiler emits one for a packed load, but it is slow -- k_match took 5.85 ms instead of 2.03 with it)
__device__ __forceinline__ uint32_t lds_le32(const uint32_t *in_w, uint32_t byte_addr) {
    const uint32_t w = byte_addr >> 2;
    return __builtin_amdgcn_alignbyte(in_w[w + 1], in_w[w], byte_addr & 3u);
}

// lz_extend from 4 matched bytes, clamped to max_len
__device__ __forceinline__ uint32_t lds_extend(const uint32_t *in_w, uint32_t a, uint32_t c,
                                               uint32_t max_len) {
    uint32_t len = 4;
    while (len < max_len) {
        const uint32_t x = lds_le32(in_w, a + len) ^ lds_le32(in_w, c + len);
        if (x) {
            len += (uint32_t)(__ffs((int)x) - 1) >> 3;
            break;
        }
        len += 4;
    }
    return len < max_len ? len : max_len;
}

__device__ __forceinline__ void match_block(const Config &cfg, const uint8_t *__restrict__ slab,
                                            BlockMeta *__restrict__ meta_all,
                                            const uint16_t *__restrict__ cand_all,
                                            uint8_t *__restrict__ len8_all, uint32_t *__restrict__ nz_all,
                                            uint16_t *__restrict__ val_all, const uint32_t b) {
    __shared__ uint32_t in_w[kInWords];  // window bytes (+ lead misalignment, + pad)
    __shared__ uint32_t run_mode;        // sticky: some wave of this block has met a long run
    const uint32_t tid = threadIdx.x;
    BlockMeta *meta = meta_all + b;
    const uint32_t n = meta->n;
    if (n <= cfg.passthrough) return;  // uniform for the workgroup
    if (tid == 0) run_mode = 0;
    const uint8_t *in = slab + (uint64_t)b * cfg.block_size;
    const uint16_t *cand = cand_all + (uint64_t)b * cfg.stride;
    uint8_t *len8 = len8_all + (uint64_t)b * cfg.stride;
    unsigned long long *nz_out = (unsigned long long *)(nz_all + (uint64_t)b * (cfg.stride / 32));
    uint16_t *val = val_all + (uint64_t)b * cfg.stride;

    const uint32_t tile_step = n <= kTile ? kTile : kTile / 2;
    for (uint32_t tile_begin = 0; tile_begin < n; tile_begin += tile_step) {
        const uint32_t tile_end = tile_begin + tile_step < n ? tile_begin + tile_step : n;
        const uint32_t win_begin = tile_begin >= 32768u ? tile_begin - 32768u : 0;  // history
        const uint32_t win_end = tile_end + 264 < n ? tile_end + 264 : n;           // look-ahead
        // LDS byte address of block byte i is (i - win_begin) + mis
        const uint32_t mis = (uint32_t)((uintptr_t)(in + win_begin) & 3u);
        __syncthreads();  // the previous tile is done with in_w / which_bits
        {
            const uint32_t *src = (const uint32_t *)(in + win_begin - mis);
            const uint32_t ndw = (mis + (win_end - win_begin) + 3) >> 2;
            // 16 bytes per load, four loads per thread in flight before the LDS stores
            const dword4 *src4 = (const dword4 *)src;
            dword4 *dst4 = (dword4 *)in_w;
            const uint32_t nq = ndw >> 2;
            for (uint32_t q0 = 0; q0 < nq; q0 += 4 * kMpThreads) {
                dword4 v[4];
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t q = q0 + tid + k * kMpThreads;
                    v[k] = src4[q < nq ? q : nq - 1];
                }
                // (left alone, the compiler sinks each load into the guarded block of its store and
                // waits for it there: four memory round trips in a row instead of one)
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    GZPX_PIN_VGPR(v[k].x);
                    GZPX_PIN_VGPR(v[k].y);
                    GZPX_PIN_VGPR(v[k].z);
                    GZPX_PIN_VGPR(v[k].w);
                }
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t q = q0 + tid + k * kMpThreads;
                    if (q < nq) dst4[q] = v[k];
                }
            }
            for (uint32_t i = 4 * nq + tid; i < ndw; i += kMpThreads) in_w[i] = src[i];
            for (uint32_t i = ndw + tid; i < ndw + 3 && i < kInWords; i += kMpThreads) in_w[i] = 0;
        }
        __syncthreads();

        // candidate distances, 4 positions per thread and step: d0 of the NEXT step is requested
        // together with this step's dependent gather cand[p - d0], so a step waits for memory once
        auto load_d0 = [&](uint32_t p) -> uint32_t { return (p < tile_end && p + 5 <= n) ? cand[p] : 0u; };
        uint32_t d0n[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) d0n[k] = load_d0(tile_begin + tid + k * kMpThreads);
        // One step = 4 positions per thread.  The step exists twice: the plain one, and one with
        // the run-group logic compiled in, taken once the block has shown a long run (keeping the
        // rarely needed code out of the plain step's registers and schedule).
        auto step = [&](uint32_t p0, auto runs_tag) {
            constexpr bool runs_on = decltype(runs_tag)::value;
            uint32_t d0s[4], d1s[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) d0s[k] = d0n[k];
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t p = p0 + k * kMpThreads;
                d1s[k] = (d0s[k] && !GZPX_EXP(cfg, 4)) ? cand[p - d0s[k]] : 0u;
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) d0n[k] = load_d0(p0 + (4 + k) * kMpThreads);
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): nothing below waits behind a store
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t r = d1s[k];
                d1s[k] = (r && d0s[k] + r <= 32767u) ? d0s[k] + r : 0u;
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t p = p0 + k * kMpThreads;
                // (no early exit: every lane takes part in the ballot below)
                uint32_t best = 0, value = 0;
                const uint32_t d0 = d0s[k], d1 = d1s[k];
                if (p < tile_end) value = (lds_le32(in_w, p - win_begin + mis)) & 0xFFu;  // the literal
                const uint32_t rem = p < n ? n - p : 0u;
                const uint32_t max_len = rem < 258u ? rem : 258u;
                const uint32_t nice_len = max_len < 32u ? max_len : 32u;
                const uint32_t a = p - win_begin + mis;
                // Run groups (only once the block has shown a long run, see run_mode): consecutive
                // lanes (= consecutive positions) whose newer candidate has the same distance compare
                // the same two byte streams, shifted by one byte per lane.  For a group of > 32 lanes
                // the wave measures the leader's common length L once, 256 bytes per step (every lane
                // one dword), and lane j of the group takes L - j.  Long runs (zeros, periodic data)
                // otherwise cost 64 loop steps for every wave.
                uint32_t pre0 = 0xFFFFFFFFu;  // common length with the newer candidate, if derived
                if constexpr (runs_on) {
                    const uint32_t wl = tid & 63u;
                    // d0 of the lane below (wave_shr:1 on the DPP network; lane 0 gets 0)
                    const uint32_t dprev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)d0, 0x138, 0xf, 0xf, false);
                    const unsigned long long same_mask = __ballot(d0 != 0 && d0 == dprev);
                    // leaders followed by >= 32 lanes of their group: such a match reaches nice_len,
                    // so the older candidate of these lanes cannot count either
                    unsigned long long run32 = same_mask & (same_mask >> 1);
                    run32 &= run32 >> 2;
                    run32 &= run32 >> 4;
                    run32 &= run32 >> 8;
                    run32 &= run32 >> 16;
                    unsigned long long leaders = ~same_mask & (run32 >> 1);
                    const uint32_t lds_end = win_end - win_begin + mis;  // LDS byte address of the window's end
                    while (leaders) {
                        const uint32_t sl = (uint32_t)__ffsll((long long)leaders) - 1;
                        leaders &= leaders - 1;
                        const unsigned long long rest = ~(same_mask >> (sl + 1));
                        const uint32_t size = rest ? (uint32_t)__ffsll((long long)rest) - 1 : 63u - sl;  // followers
                        const uint32_t a_s = rdlane(a, sl), c_s = a_s - rdlane(d0, sl);
                        uint32_t cap = 258u + size;
                        if (cap > lds_end - a_s) cap = lds_end - a_s;
                        uint32_t L = cap;
                        for (uint32_t base = 0; base < cap; base += 256) {
                            const uint32_t o4 = base + 4 * wl;
                            const uint32_t x = o4 < cap ? (lds_le32(in_w, a_s + o4) ^ lds_le32(in_w, c_s + o4)) : 0u;
                            const unsigned long long mm = __ballot(x != 0);
                            if (mm) {
                                const uint32_t m = (uint32_t)__ffsll((long long)mm) - 1;
                                L = base + 4 * m + ((uint32_t)(__ffs((int)rdlane(x, m)) - 1) >> 3);
                                break;
                            }
                        }
                        const bool exact = L < cap;  // a mismatch inside the compared range
                        if (L > cap) L = cap;
                        if (wl >= sl && wl <= sl + size) {
                            const uint32_t lj = L > wl - sl ? L - (wl - sl) : 0u;
                            if (exact || lj >= max_len) pre0 = lj;
                        }
                    }
                }
                if (d0) {
                    const uint32_t c0 = a - d0, c1 = a - (d1 ? d1 : d0);
                    const uint32_t *pa = in_w + (a >> 2), *p0 = in_w + (c0 >> 2), *p1 = in_w + (c1 >> 2);
                    uint32_t lo_a = pa[0], hi_a = pa[1], lo_0 = p0[0], hi_0 = p0[1], lo_1 = p1[0], hi_1 = p1[1];
                    const uint32_t seq = __builtin_amdgcn_alignbyte(hi_a, lo_a, a & 3u);
                    bool act0 = __builtin_amdgcn_alignbyte(hi_0, lo_0, c0 & 3u) == seq;
                    bool act1 = d1 != 0 && __builtin_amdgcn_alignbyte(hi_1, lo_1, c1 & 3u) == seq;
                    uint32_t len0 = act0 ? max_len : 0u, len1 = act1 ? max_len : 0u;  // still matching => max_len
                    if (runs_on && pre0 != 0xFFFFFFFFu) {  // known from the run group (pre0 < 4 <=> the 4-byte check fails)
                        len0 = pre0 >= 4 ? pre0 : 0u;
                        act0 = false;
                        if ((len0 < max_len ? len0 : max_len) >= nice_len) act1 = false;  // the older one cannot count
                    }
                    for (uint32_t off = 4; (act0 || act1) && off < max_len && !GZPX_EXP(cfg, 6); off += 4) {
                        const uint32_t j = (off >> 2) + 1;
                        lo_a = hi_a;
                        hi_a = pa[j];
                        lo_0 = hi_0;
                        hi_0 = p0[j];
                        lo_1 = hi_1;
                        hi_1 = p1[j];
                        const uint32_t own = __builtin_amdgcn_alignbyte(hi_a, lo_a, a & 3u);
                        const uint32_t x0 = own ^ __builtin_amdgcn_alignbyte(hi_0, lo_0, c0 & 3u);
                        const uint32_t x1 = own ^ __builtin_amdgcn_alignbyte(hi_1, lo_1, c1 & 3u);
                        if (act0 && x0) {
                            len0 = off + ((uint32_t)(__ffs((int)x0) - 1) >> 3);
                            act0 = false;
                        }
                        if (act1 && x1) {
                            len1 = off + ((uint32_t)(__ffs((int)x1) - 1) >> 3);
                            act1 = false;
                        }
                    }
                    if (len0 > max_len) len0 = max_len;
                    if (len1 > max_len) len1 = max_len;
                    best = len0;
                    if (best) value = d0;
                    if (best < nice_len && len1 > best) {  // the older candidate won
                        best = len1;
                        value = d1;
                    }
                }
                // a match this long means the wave has met a long run: switch the block to run groups
                if (!runs_on && __ballot(best >= 160) && (tid & 63u) == 0) run_mode = 1;
                // one 64-bit word of the "a match starts here" bitmap per wave step (the wave's 64
                // positions are consecutive and 64-aligned)
                const unsigned long long nzm = __ballot(best != 0);
                if (p < tile_end && !GZPX_EXP(cfg, 5)) {
                    len8[p] = (uint8_t)(best ? best - 3 : 0);
                    val[p] = (uint16_t)value;  // match distance, or the literal byte
                    if ((tid & 63u) == 0) nz_out[p >> 6] = nzm;
                }
            }
        };
        // (whole waves: the step's ballots and the uniform read below want every lane of a wave
        // that has a position in range; positions past tile_end do nothing)
        for (uint32_t p0 = tile_begin + tid; p0 - (tid & 63u) < tile_end; p0 += 4 * kMpThreads) {
            if (uniform(__hip_atomic_load(&run_mode, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != 0)
                step(p0, std::true_type{});
            else
                step(p0, std::false_type{});
        }
    }
}

// Which blocks a dense level-1 kernel (k_match, k_parse) works on: every block of the batch (`redo`
// null, grid = nb: blocks larger than one tile take this path), or the blocks that k_mparse handed
// back (`redo[0]` = how many, `redo[1..]` = which; a small grid strides over the list).
__device__ __forceinline__ uint32_t dense_count(const uint32_t *__restrict__ redo, uint32_t nb) {
    return redo ? redo[0] : nb;
}
__device__ __forceinline__ uint32_t dense_block(const uint32_t *__restrict__ redo, uint32_t i) {
    return redo ? redo[1 + i] : i;
}

__global__ __launch_bounds__(kMpThreads, 8) void k_match(Config cfg, const uint8_t *__restrict__ slab,
                                                      BlockMeta *__restrict__ meta_all,
                                                      const uint16_t *__restrict__ cand_all,
                                                      uint8_t *__restrict__ len8_all,
                                                      uint32_t *__restrict__ nz_all,
                                                      uint16_t *__restrict__ val_all, uint32_t nb,
                                                      const uint32_t *__restrict__ redo) {
    const uint32_t cnt = dense_count(redo, nb);
    for (uint32_t i = blockIdx.x; i < cnt; i += gridDim.x) {
        match_block(cfg, slab, meta_all, cand_all, len8_all, nz_all, val_all, dense_block(redo, i));
        __syncthreads();  // the next block of this workgroup reuses the LDS window
    }
}

// ------------------------------------------------------------------------------------------
// k_parse: deflate_compress_fastest's greedy parse + token stream + sub-block boundaries, per
// block (1024 threads, < 80 KiB of LDS so two workgroups share a CU), in tiles of 64 KiB
// positions whose len8 bytes are staged in LDS:
//   phase 2  the parse as a segment-parallel pointer chase over 64-position segments (one per
//            thread, token marks = one 64-bit word per segment),
//   phase 3  token build: per-group token / match counts from the bitmaps (tokens from the walk,
//            "match here" from k_match) + one workgroup scan, then coalesced val reads and token
//            stores; the same pass finds where the current DEFLATE sub-block ends (8192 matches,
//            or the 65535-byte soft limit of choose_max_block_end).
// ------------------------------------------------------------------------------------------
// (k_parse_hc) Walk one segment (tile-relative positions) from `pos`, marking every token start in tok_bits;
// returns the exit position.  A latency chain (LDS read -> add -> LDS read ...); the mark is a
// fire-and-forget LDS atomic.
__device__ __forceinline__ uint32_t walk_segment(const uint8_t *len8, uint32_t pos, uint32_t seg_end,
                                                 uint32_t *tok_bits) {
    while (pos < seg_end) {
        const uint32_t l = len8[pos];
        atomicOr(&tok_bits[pos >> 5], 1u << (pos & 31u));
        pos += l ? l + 3 : 1;
    }
    return pos;
}

// forget the marks of a walk that started from a wrong entry (a thread only marks positions of
// its own segment, words at the segment edges are shared with the neighbours)
__device__ __forceinline__ void clear_marks(uint32_t seg_begin, uint32_t seg_end, uint32_t *tok_bits) {
    for (uint32_t wi = seg_begin >> 5; wi <= (seg_end - 1) >> 5; wi++) {
        const uint32_t lo = wi * 32 < seg_begin ? seg_begin - wi * 32 : 0;
        const uint32_t hi = (wi + 1) * 32 > seg_end ? seg_end - wi * 32 : 32;
        const uint32_t mask = (hi >= 32 ? 0xFFFFFFFFu : (1u << hi) - 1u) & ~((1u << lo) - 1u);
        atomicAnd(&tok_bits[wi], ~mask);
    }
}

constexpr uint32_t kPSeg = 64;  // positions per walk segment = one 64-bit word of the token bitmap
constexpr uint32_t kRescueTokens = 512;

__device__ __forceinline__ void parse_block(
    const Config &cfg, const uint8_t *__restrict__ slab, BlockMeta *__restrict__ meta_all,
    SubMeta *__restrict__ sub_all, const uint8_t *__restrict__ len8_all,
    const uint32_t *__restrict__ nz_all, const uint16_t *__restrict__ val_all,
    uint32_t *__restrict__ tok_all, const uint32_t b) {
    __shared__ uint32_t len8_w[kTile / 4];                 // 0 = literal, else match length - 3 (bytes)
    __shared__ unsigned long long tok_bits[kTile / 64];    // 1 = a token starts here (tile-relative)
    __shared__ uint32_t rank_pre[kTile / 64];  // phase 2: exit of segment s; phase 3: (tokens |
                                               // matches << 17) before 64-position group s
    __shared__ uint32_t wsum_t[kMpWaves], wsum_m[kMpWaves];
    __shared__ unsigned long long bnd;  // (position << 32 | token index) of the sub-block boundary
    __shared__ uint32_t bnd_mat;        // matches before that boundary
    __shared__ uint32_t rescue[2];      // first inconsistent segment / end of the rescued range
    const uint8_t *len8 = (const uint8_t *)len8_w;
    uint32_t *seg_exit = rank_pre;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    BlockMeta *meta = meta_all + b;
    SubMeta *sub = sub_all + (uint64_t)b * cfg.max_sub;
    const uint32_t n = meta->n;
    if (n <= cfg.passthrough) return;  // uniform for the workgroup
    const unsigned long long *nz = (const unsigned long long *)(nz_all + (uint64_t)b * (cfg.stride / 32));
    const uint16_t *val = val_all + (uint64_t)b * cfg.stride;
    uint32_t *tok = tok_all + (uint64_t)b * cfg.stride;
    (void)slab;

    // state carried from tile to tile (uniform across the workgroup)
    uint32_t entry_carry = 0;            // where the parse enters the next tile
    uint32_t tok_carry = 0, mat_carry = 0;
    uint32_t cur_sub = 0, sub_start = 0, sub_start_tok = 0, sub_start_mat = 0;
    uint32_t sub_limit = max_block_end(0, n, kFastSoftMaxBlockLen);

    for (uint32_t tile_begin = 0; tile_begin < n; tile_begin += kTile) {
        const uint32_t tile_len = n - tile_begin < kTile ? n - tile_begin : kTile;
        __syncthreads();  // previous tile fully consumed
        {
            // 64 bytes per thread as four 16-byte loads, all in flight before the LDS stores (the
            // per-block stride is a multiple of 1024 and padded, so whole uint4s are readable)
            const uint4 *src = (const uint4 *)(len8_all + (uint64_t)b * cfg.stride + tile_begin);
            uint4 *dst = (uint4 *)len8_w;
            const uint32_t nq = (tile_len + 15) / 16;  // never past the block's own (padded) array
            uint4 v[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t q = tid + k * kMpThreads;
                v[k] = src[q < nq ? q : nq - 1];
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) dst[tid + k * kMpThreads] = v[k];
            if (tid == 0) bnd = ~0ull;
        }
        __syncthreads();

        // ---- phase 2: the greedy parse as a speculative segment walk.  Thread s owns the 64
        // positions of segment s and walks them from an entry position: first guess "my segment
        // start" (thread 0 knows the tile's true entry), then the exit of segment s-1, until no
        // entry changes.  A segment whose entry lies beyond its end (a long match flew over it) has
        // no tokens and hands the entry through.  Greedy walks re-synchronise within a few tokens,
        // so a handful of rounds suffice; the token marks of a walk are one 64-bit word, rewritten
        // by every re-walk.
        const uint32_t seg_begin = tid * kPSeg;  // tile-relative; kTile / kPSeg == kMpThreads
        const bool active = seg_begin < tile_len;
        const uint32_t seg_end = active ? (seg_begin + kPSeg < tile_len ? seg_begin + kPSeg : tile_len) : 0;
        auto walk = [&](uint32_t pos) -> uint32_t {
            unsigned long long marks = 0;
            while (pos < seg_end) {
                const uint32_t l = len8[pos];
                marks |= 1ull << (pos - seg_begin);
                pos += l ? l + 3 : 1;
            }
            tok_bits[tid] = marks;
            return pos;
        };
        uint32_t entry = tid == 0 ? entry_carry - tile_begin : seg_begin;
        if (active) seg_exit[tid] = walk(entry);
        else tok_bits[tid] = 0;
        const uint32_t n_seg = (tile_len + kPSeg - 1) / kPSeg;
        for (uint32_t round = 0;; round++) {
            __syncthreads();
            bool changed = false;
            uint32_t new_entry = entry;
            if (active && tid > 0) {
                new_entry = seg_exit[tid - 1];
                changed = new_entry != entry;
            }
            if (round >= 24) {
                // Slow convergence (long runs: every 258-byte match shifts the phase of the
                // segments behind it, one segment per round).  One thread then parses on from the
                // first inconsistent segment for up to kRescueTokens tokens -- a chain of LDS
                // reads, but each token of such data covers hundreds of bytes.
                if (tid == 0) rescue[0] = 0xFFFFFFFFu;
                __syncthreads();
                if (changed) atomicMin(&rescue[0], tid);
                __syncthreads();
                const uint32_t s_first = rescue[0];
                if (s_first == 0xFFFFFFFFu) break;  // nothing changed: converged
                if (tid == 0) {
                    uint32_t sg = s_first, pos = seg_exit[s_first - 1], budget = kRescueTokens;
                    while (sg < n_seg && budget) {
                        const uint32_t sb = sg * kPSeg, se = sb + kPSeg < tile_len ? sb + kPSeg : tile_len;
                        unsigned long long marks = 0;
                        while (pos < se) {
                            const uint32_t l = len8[pos];
                            marks |= 1ull << (pos - sb);
                            pos += l ? l + 3 : 1;
                            budget = budget ? budget - 1 : 0;
                        }
                        tok_bits[sg] = marks;
                        seg_exit[sg] = pos;
                        sg++;
                    }
                    rescue[1] = sg;  // segments [s_first, sg) are consistent with their entries now
                }
                __syncthreads();
                const uint32_t s_end = rescue[1];
                if (tid >= s_first && tid < s_end) {
                    entry = seg_exit[tid - 1];
                } else if (changed && tid > s_end) {  // the others keep correcting themselves in parallel
                    entry = new_entry;
                    seg_exit[tid] = walk(entry);
                }
                continue;
            }
            __syncthreads();
            if (changed) {
                entry = new_entry;
                seg_exit[tid] = walk(entry);
            }
            if (!__syncthreads_or(changed)) break;
        }
        // where the parse leaves this tile (a match may overhang the tile end)
        const uint32_t exit_rel = uniform(seg_exit[n_seg - 1]);
        __syncthreads();  // seg_exit is rank_pre from here on

        // ---- phase 3a: tokens / matches per 64-position group (one thread each, from the two
        // bitmaps), then one workgroup-wide scan
        const unsigned long long my_tok = tok_bits[tid];
        const unsigned long long my_mat = my_tok & (active ? nz[(tile_begin >> 6) + tid] : 0ull);
        uint32_t tile_tok, tile_mat;
        uint32_t my_pre;
        {
            const uint32_t vt = (uint32_t)__popcll(my_tok), vm = (uint32_t)__popcll(my_mat);
            const uint32_t it = wave_inclusive_scan(vt, lane), im = wave_inclusive_scan(vm, lane);
            if (lane == 63) {
                wsum_t[wave] = it;
                wsum_m[wave] = im;
            }
            __syncthreads();
            uint32_t bt = 0, bm = 0, tt = 0, tm = 0;
            for (uint32_t w = 0; w < kMpWaves; w++) {
                const uint32_t st = wsum_t[w], sm = wsum_m[w];
                if (w < wave) {
                    bt += st;
                    bm += sm;
                }
                tt += st;
                tm += sm;
            }
            tile_tok = uniform(tt);
            tile_mat = uniform(tm);
            // exclusive prefixes: tokens <= 65536 fit 17 bits, matches <= 16384 fit 15 bits
            my_pre = (bt + it - vt) | ((bm + im - vm) << 17);
            rank_pre[tid] = my_pre;
        }
        __syncthreads();

        // ---- phase 3b: build tokens in position order: lane l of a wave takes position l of a
        // 64-position group (coalesced val reads and token stores), ranks from the group's prefix +
        // popcounts below the lane.  The same pass looks for the end of the current sub-block.  A
        // second boundary inside one tile needs another 8192 matches after the first, so the
        // search is repeated only in that case.
        const uint32_t ngroups = (tile_len + 63) / 64;
        const unsigned long long lane_below = (1ull << lane) - 1ull;
        bool build = true;
        for (;;) {
            // 8 groups of a wave per step: all val loads first, then every token word is formed
            // (the last use of a loaded value), then the stores -- a loaded value consumed after a
            // store had been issued would make the compiler drain the stores first (loads and
            // stores share one counter on gfx9).  The match rank is only needed in the one group
            // where the 8192-match rule can fire, which the group prefixes tell.
            for (uint32_t g0 = wave; g0 < ngroups; g0 += 8 * kMpWaves) {
                uint32_t vals[8], tis[8];
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) {
                    const uint32_t g = g0 + k * kMpWaves;
                    const uint32_t r = g * 64 + lane;
                    vals[k] = (build && g < ngroups && r < tile_len && !GZPX_EXP(cfg, 9)) ? val[tile_begin + r] : 0u;
                }
                // every load has landed from here on, also on the paths that skip a group: without
                // this the compiler must assume a pending load behind each later store's data
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) {
                    const uint32_t g = g0 + k * kMpWaves;
                    tis[k] = 0xFFFFFFFFu;
                    if (g >= ngroups) continue;  // wave-uniform
                    const unsigned long long mt = tok_bits[g];
                    const uint32_t pre = rank_pre[g];
                    const uint32_t mat_after = mat_carry + (g + 1 < ngroups ? rank_pre[g + 1] >> 17 : tile_mat);
                    const bool count_rule = mat_after - sub_start_mat >= kFastSeqStoreLen;  // wave-uniform, rare
                    const uint32_t r = g * 64 + lane, p = tile_begin + r;
                    if (!((mt >> lane) & 1ull)) continue;
                    const uint32_t ti = tok_carry + (pre & 0x1FFFFu) + (uint32_t)__popcll(mt & lane_below);
                    // sub-block boundary: this token would start past the soft limit, or 8192
                    // matches precede it in the current sub-block (src: deflate_compress_fastest)
                    bool boundary = p >= sub_limit;
                    if (count_rule) {
                        const unsigned long long mm = mt & nz[(tile_begin >> 6) + g];
                        const uint32_t mi = mat_carry + (pre >> 17) + (uint32_t)__popcll(mm & lane_below);
                        boundary = boundary || mi - sub_start_mat >= kFastSeqStoreLen;
                    }
                    if (p > sub_start && boundary) atomicMin(&bnd, ((unsigned long long)p << 32) | ti);
                    const uint32_t l = len8[r];
                    vals[k] = l ? (kTokMatch | (vals[k] << 9) | (l + 3)) : vals[k];
                    tis[k] = ti;
                }
                if (build && !GZPX_EXP(cfg, 8)) {
#pragma unroll
                    for (uint32_t k = 0; k < 8; k++)
                        if (tis[k] != 0xFFFFFFFFu) tok[tis[k]] = vals[k];
                }
            }
            __syncthreads();
            const unsigned long long bv = bnd;
            if (bv == ~0ull) break;  // the current sub-block runs past this tile
            // the boundary token's match rank, from its group's prefix and the bitmaps
            const uint32_t bp = uniform((uint32_t)(bv >> 32)), bti = uniform((uint32_t)bv);
            if (tid == 0) {
                const uint32_t r = bp - tile_begin, g = r >> 6;
                const unsigned long long mm = tok_bits[g] & nz[(tile_begin >> 6) + g];
                bnd_mat = mat_carry + (rank_pre[g] >> 17) + (uint32_t)__popcll(mm & ((1ull << (r & 63u)) - 1ull));
            }
            __syncthreads();
            const uint32_t bm = uniform(bnd_mat);
            if (tid == 0) {
                sub[cur_sub].tok_begin = sub_start_tok;
                sub[cur_sub].tok_end = bti;
                sub[cur_sub].byte_begin = sub_start;
                sub[cur_sub].byte_len = bp - sub_start;
                sub[cur_sub].is_final = 0;
                bnd = ~0ull;
            }
            cur_sub++;
            sub_start = bp;
            sub_start_tok = bti;
            sub_start_mat = bm;
            sub_limit = max_block_end(bp, n, kFastSoftMaxBlockLen);
            __syncthreads();
            // another boundary in this tile needs 8192 more matches, or -- when this boundary sits
            // on the tile's first positions -- the 65535-byte soft limit falling on its last ones
            if (mat_carry + tile_mat - bm < kFastSeqStoreLen && sub_limit >= tile_begin + tile_len) break;
            build = false;
        }
        tok_carry += tile_tok;
        mat_carry += tile_mat;
        entry_carry = tile_begin + exit_rel;
    }
    if (tid == 0) {
        sub[cur_sub].tok_begin = sub_start_tok;
        sub[cur_sub].tok_end = tok_carry;
        sub[cur_sub].byte_begin = sub_start;
        sub[cur_sub].byte_len = n - sub_start;
        sub[cur_sub].is_final = 1;
        meta->ntok = tok_carry;
        meta->nsub = cur_sub + 1;
    }
}

__global__ __launch_bounds__(kMpThreads, 8) void k_parse(
    Config cfg, const uint8_t *__restrict__ slab, BlockMeta *__restrict__ meta_all,
    SubMeta *__restrict__ sub_all, const uint8_t *__restrict__ len8_all,
    const uint32_t *__restrict__ nz_all, const uint16_t *__restrict__ val_all,
    uint32_t *__restrict__ tok_all, uint32_t nb, const uint32_t *__restrict__ redo) {
    const uint32_t cnt = dense_count(redo, nb);
    for (uint32_t i = blockIdx.x; i < cnt; i += gridDim.x) {
        parse_block(cfg, slab, meta_all, sub_all, len8_all, nz_all, val_all, tok_all, dense_block(redo, i));
        __syncthreads();  // the next block of this workgroup reuses the LDS arrays
    }
}

// ------------------------------------------------------------------------------------------
// k_mparse: level 1, blocks of at most one tile -- k_match and k_parse fused into "match on demand".
// libdeflate's deflate_compress_fastest calls ht_matchfinder_longest_match only where a token
// starts (about a quarter of the positions of text); k_match searches EVERY position because the
// parse is not known yet, and hands len8 / val / the bitmap to k_parse through HBM.  Here the
// speculative segment walk of k_parse does the searching itself.  A walk lands on positions that
// nothing predicts, so everything a search touches must be randomly addressable at LDS cost (read
// from `cand` in global memory, 64 lanes = 64 cache lines per load, the walks were bound by the
// vector L1): the workgroup owns the CU's LDS -- the block's bytes (64 KiB) plus the candidate
// distances d0 of HALF the block (64 KiB) -- and takes the block in two passes of 32 Ki positions:
//   phase 1  thread s walks the 32 positions of segment s from an entry position and runs
//            longest_match (d0 and the older candidate's d0[p - d0] out of LDS; the few older
//            candidates of the second pass that lie in the first half come from global memory) at
//            every position it lands on; it keeps three 32-bit registers (token starts, "is a match",
//            "the older candidate won") and its exit.  Entries are corrected round by round as in
//            k_parse; a re-walk that lands on a token start of the previous walk has re-synchronised
//            and keeps the rest of that walk (no second search).  Positions without a candidate
//            (d0 == 0) are literals before anything is searched: one bit per position, built
//            where the pass's d0 goes into LDS, lets a walk step over a run of them at once.
//   phase 2  token / match counts per segment -> one workgroup scan.
//   phase 3  sub-block boundaries (the first token with 8192 matches of the current sub-block before
//            it: match ranks are known from the scan, every lane names its own candidate), then
//            every lane writes the tokens of its own segment: length = distance to the next token
//            start, distance = d0 or d0 + d0[p - d0] out of LDS again, literals from the LDS window.
// Nothing but tokens goes to HBM.  Long runs (every 258-byte match shifts the phase of the segments
// behind it, entries settle by one segment per round) are handed back to the dense kernels through the
// `redo` list -- the cooperative run logic lives there: at once when a pass's first walk shows them (one
// segment in eight left by a match that overshoots it by two segments or more), or when the entries have
// not settled after kMpMaxRounds rounds.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kMpMaxRounds = 24;
constexpr uint32_t kMhHalf = 32768;  // positions per pass (their d0: 64 KiB of LDS)
constexpr uint32_t kMhSeg = kMhHalf / kMpThreads;  // 32 positions per walk segment = one 32-bit mask

// ht_matchfinder_longest_match at block position p (block byte i sits at LDS byte i + mis; d0_h[i] =
// d0 of position hb + i).  Returns the match length (0 = none); `older` = the bucket's older entry won.
// TAIL = the segment lies within 266 bytes of the block's end (lengths clamp to what is left and the
// last four positions are not searched); everywhere else max_len = 258 and nice_len = 32.
// (Tried: both candidates compared 8 bytes per round -- three dwords per stream up front, two per
// later round.  Same VALU count, more LDS reads for the literal steps: k_mparse 2.20 -> 2.35 ms.)
template <bool TAIL>
__device__ __forceinline__ uint32_t l1_search(const uint32_t *in_w, const uint16_t *d0_h, uint32_t hb,
                                              const uint16_t *__restrict__ cand, uint32_t p, uint32_t n,
                                              uint32_t mis, bool &older, bool no_gather = false) {
    older = false;
    const uint32_t d0 = (!TAIL || p + 5 <= n) ? (uint32_t)d0_h[p - hb] : 0u;
    if (!d0) return 0;  // (the walks step over these positions; they ask under Config.debug bit 3 only)
    const uint32_t q = p - d0;  // the bucket's newer entry; the older one is ITS predecessor
    // (an LDS read for every lane and a masked global one for the few whose q lies before the pass.
    // Left alone, the compiler turns the two loads into ONE flat load of a selected pointer, which
    // goes down the vector-memory path for every lane and waits for both counters)
    uint32_t r = d0_h[q >= hb ? q - hb : 0u];
    if (q < hb) r = *(const volatile uint16_t *)(cand + q);  // (volatile: keeps the two loads apart)
    if (no_gather) r = 0;
    const uint32_t d1 = d0 + r;
    const bool two = r != 0 && d1 <= 32767u;  // the older entry is alive
    const uint32_t max_len = TAIL ? (n - p < 258u ? n - p : 258u) : 258u;
    const uint32_t nice_len = TAIL ? (max_len < 32u ? max_len : 32u) : 32u;
    const uint32_t a = p + mis;
    const uint32_t c0 = a - d0, c1 = two ? a - d1 : c0;
    const uint32_t *pa = in_w + (a >> 2), *p0 = in_w + (c0 >> 2), *p1 = in_w + (c1 >> 2);
    const uint32_t sa = a & 3u, s0 = c0 & 3u, s1 = c1 & 3u;
    uint32_t lo_a = pa[0], hi_a = pa[1], lo_0 = p0[0], hi_0 = p0[1], lo_1 = p1[0], hi_1 = p1[1];
    const uint32_t seq = __builtin_amdgcn_alignbyte(hi_a, lo_a, sa);
    bool act0 = __builtin_amdgcn_alignbyte(hi_0, lo_0, s0) == seq;
    bool act1 = two && __builtin_amdgcn_alignbyte(hi_1, lo_1, s1) == seq;
    uint32_t len0 = act0 ? max_len : 0u, len1 = act1 ? max_len : 0u;  // still matching => max_len
    for (uint32_t off = 4; (act0 || act1) && off < max_len; off += 4) {
        const uint32_t j = (off >> 2) + 1;
        lo_a = hi_a;
        hi_a = pa[j];
        lo_0 = hi_0;
        hi_0 = p0[j];
        lo_1 = hi_1;
        hi_1 = p1[j];
        const uint32_t own = __builtin_amdgcn_alignbyte(hi_a, lo_a, sa);
        const uint32_t x0 = own ^ __builtin_amdgcn_alignbyte(hi_0, lo_0, s0);
        const uint32_t x1 = own ^ __builtin_amdgcn_alignbyte(hi_1, lo_1, s1);
        if (act0 && x0) {
            len0 = off + ((uint32_t)(__ffs((int)x0) - 1) >> 3);
            act0 = false;
        }
        if (act1 && x1) {
            len1 = off + ((uint32_t)(__ffs((int)x1) - 1) >> 3);
            act1 = false;
        }
    }
    if (len0 > max_len) len0 = max_len;
    if (len1 > max_len) len1 = max_len;
    uint32_t best = len0;
    if (best < nice_len && len1 > best) {  // the older candidate won
        best = len1;
        older = true;
    }
    return best;
}

__global__ __launch_bounds__(kMpThreads, 4) void k_mparse(
    Config cfg, const uint8_t *__restrict__ slab, BlockMeta *__restrict__ meta_all,
    SubMeta *__restrict__ sub_all, const uint16_t *__restrict__ cand_all, uint32_t *__restrict__ tok_all,
    uint32_t *__restrict__ redo, uint64_t slab_len, uint32_t nb, uint32_t *__restrict__ claim) {
    __shared__ uint32_t in_w[kInWords];        // the block's bytes (+ lead misalignment, + pad)
    __shared__ uint32_t s_claimed;             // the block this workgroup takes after the next one
    __shared__ uint32_t d0_w[kMhHalf / 2];     // d0 (u16) of the positions of the current pass
    __shared__ uint32_t nz_w[kMpThreads];      // "has a candidate", one bit per position of the pass: a dword per segment
    __shared__ uint32_t seg_exit[2 * kMpThreads];  // where the walk of segment s leaves it (two copies, see the rounds)
    __shared__ uint32_t wsum_t[kMpWaves];
    __shared__ unsigned long long bnd;  // (position << 32 | token index) of the sub-block boundary
    __shared__ uint32_t bnd_mat;        // matches before that boundary
    const uint16_t *d0_h = (const uint16_t *)d0_w;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // One workgroup per CU (the LDS is its alone), walking the blocks blockIdx.x, + gridDim.x, ...: while it
    // parses a block, the NEXT block's bytes (requested at the top of the block) and first-pass d0 (requested behind
    // the last pass's walks) are on their way into registers, so the CU waits for HBM once per launch instead of
    // once per block (17 k of a block's 142 k cycles were that wait when every block was a workgroup of its own).
    // Where the kernel waits for them is written down, not left to the compiler: its own place for the wait is the
    // ds_write that stages the registers at the turn of a pass or a block, and there the wait also drains the token
    // stores issued since (loads and stores share one counter, and every wave stood still for their acknowledgement).
    auto block_len = [&](uint32_t blk) -> uint32_t {  // k_init_meta's cut
        const uint64_t begin = (uint64_t)blk * cfg.block_size;
        const uint64_t len = slab_len > begin ? slab_len - begin : 0;
        return (uint32_t)(len > cfg.block_size ? cfg.block_size : len);
    };
    // d0 of a pass: 64 bytes per thread (the per-block stride is padded: whole uint4s are readable)
    uint4 d0v0 = make_uint4(0u, 0u, 0u, 0u), d0v1 = d0v0, d0v2 = d0v0, d0v3 = d0v0;
#define GZPX_D0_REQUEST(cand_, hb_, n_)                                              \
    do {                                                                            \
        const uint32_t he_ = (hb_) + kMhHalf < (n_) ? (hb_) + kMhHalf : (n_);       \
        const uint4 *src_ = (const uint4 *)((cand_) + (hb_));                       \
        const uint32_t nq_ = (he_ - (hb_) + 7) / 8;                                 \
        d0v0 = src_[tid < nq_ ? tid : nq_ - 1];                                     \
        d0v1 = src_[tid + kMpThreads < nq_ ? tid + kMpThreads : nq_ - 1];           \
        d0v2 = src_[tid + 2 * kMpThreads < nq_ ? tid + 2 * kMpThreads : nq_ - 1];   \
        d0v3 = src_[tid + 3 * kMpThreads < nq_ ? tid + 3 * kMpThreads : nq_ - 1];   \
    } while (0)
    // The request only issues the loads; GZPX_D0_ARRIVED is where the kernel waits for them: an empty statement that
    // READS the registers (GZPX_HERE_VGPR), so the compiler puts its wait in front of it and knows them complete on
    // every way on from there.  (A read, not GZPX_PIN_VGPR's read-and-write: a written operand is a new value, the
    // register allocator then held the registers in a second set across the pass loop -- 113 to 127 VGPRs in the
    // forms tried -- and the copies between the sets brought waits of their own.  And all four dwords as ONE
    // 128-bit operand: the ds_write_b128 wants them as the tuple the load filled.)
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t here4 __attribute__((ext_vector_type(4)));
#define GZPX_HERE_UINT4(v_)                              \
    do {                                                 \
        const here4 t_ = {(v_).x, (v_).y, (v_).z, (v_).w}; \
        GZPX_HERE_VGPR(t_);                              \
    } while (0)
#else
#define GZPX_HERE_UINT4(v_) ((void)0)
#endif
    // (no next block: the registers still get a value, or the old one would stay alive, sixteen registers wide,
    // through the walks up to the place that reads them)
#define GZPX_D0_NONE() d0v0 = d0v1 = d0v2 = d0v3 = make_uint4(0u, 0u, 0u, 0u)
#define GZPX_D0_ARRIVED()     \
    do {                      \
        GZPX_HERE_UINT4(d0v0); \
        GZPX_HERE_UINT4(d0v1); \
        GZPX_HERE_UINT4(d0v2); \
        GZPX_HERE_UINT4(d0v3); \
    } while (0)
    // a block's bytes (n <= kTile): four 16-byte loads per thread + one dword of tail for three threads
    uint4 bv0 = make_uint4(0u, 0u, 0u, 0u), bv1 = bv0, bv2 = bv0, bv3 = bv0;
    uint32_t bvt = 0;
    auto load16 = [](const dword4 *p4) -> uint4 {  // (a 16-byte load of a 4-byte-aligned address)
        const dword4 t = *p4;
        return make_uint4(t.x, t.y, t.z, t.w);
    };
#define GZPX_BLOCK_REQUEST(blk_, n_)                                                 \
    do {                                                                            \
        const uint8_t *in_ = slab + (uint64_t)(blk_) * cfg.block_size;              \
        const uint32_t mis_ = (uint32_t)((uintptr_t)in_ & 3u);                      \
        const uint32_t *src_ = (const uint32_t *)(in_ - mis_);                      \
        const uint32_t ndw_ = (mis_ + (n_) + 3) >> 2, nq_ = ndw_ >> 2;              \
        const dword4 *src4_ = (const dword4 *)src_;                                 \
        const uint32_t last_ = nq_ - 1; /* (n > passthrough >= 15: nq_ >= 1) */      \
        bv0 = load16(src4_ + (tid < nq_ ? tid : last_));                            \
        bv1 = load16(src4_ + (tid + kMpThreads < nq_ ? tid + kMpThreads : last_));  \
        bv2 = load16(src4_ + (tid + 2 * kMpThreads < nq_ ? tid + 2 * kMpThreads : last_)); \
        bv3 = load16(src4_ + (tid + 3 * kMpThreads < nq_ ? tid + 3 * kMpThreads : last_)); \
        bvt = src_[4 * nq_ + tid < ndw_ ? 4 * nq_ + tid : ndw_ - 1];                \
    } while (0)
#define GZPX_BLOCK_ARRIVED()  \
    do {                     \
        GZPX_HERE_UINT4(bv0); \
        GZPX_HERE_UINT4(bv1); \
        GZPX_HERE_UINT4(bv2); \
        GZPX_HERE_UINT4(bv3); \
        GZPX_HERE_VGPR(bvt);  \
    } while (0)
    static_assert(((3 + kTile + 3) >> 4) <= 4 * kMpThreads, "a block is four uint4 per thread (+ tail dwords)");

    // Blocks are CLAIMED, not strided over (round 4): a workgroup's first two blocks are blockIdx.x and blockIdx.x +
    // gridDim.x, every later one comes from one global ticket counter -- the ticket for the block after the next is
    // drawn in the current block's last pass, beside the next block's d0 and in front of the same wait.  With the
    // static stride (b += gridDim.x) 8,835 blocks over 256 CUs left 121 CUs idle for the last 35th of the launch, and
    // a CU slowed by anything else on it (an RCCL channel, a heavier run of blocks) stretched the whole launch.
    // (The counter's index goes through a VGPR: an atomic on a uniform address is rewritten by the compiler into a
    // one-lane atomic whose result is broadcast at once, and the broadcast waits for the round trip where it stands.)
    uint32_t my_ticket = 0;
    auto draw_ticket = [&]() {
        uint32_t slot = 0;
        GZPX_PIN_VGPR(slot);
        if (tid == 0) my_ticket = atomicAdd(claim + slot, 1u);
    };
    uint32_t b = blockIdx.x;
    if (b >= nb) return;
    uint32_t next_b = b + gridDim.x;
    bool staged;  // (uniform) block b's bytes and first-pass d0 have been requested -- and have arrived
    {
        const uint32_t n0 = block_len(b);
        staged = n0 > cfg.passthrough;
        if (staged) {
            GZPX_D0_REQUEST(cand_all + (uint64_t)b * cfg.stride, 0u, n0);
            GZPX_BLOCK_REQUEST(b, n0);
            GZPX_D0_ARRIVED();  // (the one HBM round trip a launch waits for)
            GZPX_BLOCK_ARRIVED();
        }
    }
  for (;;) {
    const uint32_t next_n = next_b < nb ? block_len(next_b) : 0u;
    const bool next_staged = next_n > cfg.passthrough;  // (uniform; implies next_b < nb)
    my_ticket = 0;
    // A block that does not reach its last pass's token build (handed back, or stored-only) requests the next
    // block's d0 and draws the ticket late, and waits for both on the spot, with the next block's bytes: every way to
    // the top of a block leaves these registers finished, or the compiler would wait for them there, for all.
#define GZPX_TURN_LATE()                                                                         \
    do {                                                                                        \
        if (next_staged) GZPX_D0_REQUEST(cand_all + (uint64_t)next_b * cfg.stride, 0u, next_n); \
        else GZPX_D0_NONE();                                                                    \
        draw_ticket();                                                                          \
        GZPX_D0_ARRIVED();                                                                      \
        GZPX_BLOCK_ARRIVED();                                                                   \
        GZPX_HERE_VGPR(my_ticket);                                                               \
    } while (0)
    BlockMeta *meta = meta_all + b;
    SubMeta *sub = sub_all + (uint64_t)b * cfg.max_sub;
    const uint32_t n = block_len(b);
    const uint8_t *in = slab + (uint64_t)b * cfg.block_size;
    const uint16_t *cand = cand_all + (uint64_t)b * cfg.stride;
    uint32_t *tok = tok_all + (uint64_t)b * cfg.stride;
    const uint32_t mis = (uint32_t)((uintptr_t)in & 3u);
#ifdef GZPX_EXPERIMENT
    // measurement builds: cycles per phase, summed over the blocks of a launch (thread 0's clock)
    unsigned long long exp_t = __builtin_readcyclecounter();
    auto exp_lap = [&](uint32_t slot) {
        const unsigned long long t = __builtin_readcyclecounter();
        if (tid == 0) atomicAdd(&g_exp_cycles[(b & 1023u) * 8u + slot], t - exp_t);
        exp_t = t;
    };
#else
    auto exp_lap = [](uint32_t) {};
#endif
    // (A stored-only block -- !staged: n <= cfg.passthrough, nothing to parse -- takes the way of a block that is
    // handed back in its first pass, without being put on the list: it stages what the registers hold (a few dwords
    // nobody reads), walks nothing (no position has a candidate), meets the barriers -- without one, thread 0 could
    // overwrite s_claimed while a slower wave has not read the previous iteration's value yet, ADVICE round 4 --
    // requests its successor's bytes and leaves where the hand-back leaves.  Only a slab's last block can be that
    // short today, but the parse must not depend on how batches are cut; and a way of its own to the top of the next
    // block would be one more that has to leave the prefetch registers finished.)
    __syncthreads();  // the previous block is done with in_w
    {   // the block's bytes: registers -> LDS
        const uint32_t ndw = (mis + n + 3) >> 2;
        uint4 *dst4 = (uint4 *)in_w;
        const uint32_t nq = ndw >> 2;
        if (tid < nq) dst4[tid] = bv0;
        if (tid + kMpThreads < nq) dst4[tid + kMpThreads] = bv1;
        if (tid + 2 * kMpThreads < nq) dst4[tid + 2 * kMpThreads] = bv2;
        if (tid + 3 * kMpThreads < nq) dst4[tid + 3 * kMpThreads] = bv3;
        if (4 * nq + tid < ndw) in_w[4 * nq + tid] = bvt;
        for (uint32_t i = ndw + tid; i < ndw + 3 && i < kInWords; i += kMpThreads) in_w[i] = 0;
        if (tid == 0) bnd = ~0ull;
    }
    if (next_staged) GZPX_BLOCK_REQUEST(next_b, next_n);  // (uniform) travels while this block is parsed

    // state carried from pass to pass (uniform across the workgroup)
    uint32_t entry_carry = 0;  // where the parse enters the next pass
    uint32_t tok_carry = 0, mat_carry = 0;
    uint32_t cur_sub = 0, sub_start = 0, sub_start_tok = 0, sub_start_mat = 0;
    const uint8_t *in_b = (const uint8_t *)in_w + mis;

    bool handed_back = false;
    for (uint32_t hb = 0;; hb += kMhHalf) {  // (the last pass leaves below)
        const uint32_t he = hb + kMhHalf < n ? hb + kMhHalf : n;  // this pass: positions [hb, he)
        if (hb) __syncthreads();  // the previous pass is done with d0_w / seg_exit
        {
            uint4 *dst = (uint4 *)d0_w;
            dst[tid] = d0v0;
            dst[tid + kMpThreads] = d0v1;
            dst[tid + 2 * kMpThreads] = d0v2;
            dst[tid + 3 * kMpThreads] = d0v3;
            // which of them have a candidate: one bit per position, the eight of a uint4 are one byte and the 32
            // of a walk segment one aligned dword of nz_w (d0 <= 32767: adding 0x7fff carries into bit 15 of a
            // non-zero half and never out of it)
            auto nz8 = [](const uint4 &v) -> uint8_t {
                const uint32_t k = 0x7fff7fffu, h = 0x80008000u;
                const uint32_t a = (((v.x + k) & h) >> 15) | (((v.y + k) & h) >> 13) | (((v.z + k) & h) >> 11) |
                                   (((v.w + k) & h) >> 9);  // bits 0, 2, 4, 6: the low halves; 16, 18, 20, 22: the high ones
                return (uint8_t)(a | (a >> 15));
            };
            uint8_t *nz_b = (uint8_t *)nz_w;
            nz_b[tid] = nz8(d0v0);
            nz_b[tid + kMpThreads] = nz8(d0v1);
            nz_b[tid + 2 * kMpThreads] = nz8(d0v2);
            nz_b[tid + 3 * kMpThreads] = nz8(d0v3);
            // (these registers arrived in the pass before, in front of its token build: nothing is waited for here,
            // and that pass's token stores stay in flight across the turn)
        }
        __syncthreads();
        exp_lap(0);

        // ---- phase 1: the greedy parse as a speculative segment walk that searches where it lands
        const uint32_t seg_begin = hb + tid * kMhSeg;
        const bool active = seg_begin < he;
        const uint32_t seg_end = active ? (seg_begin + kMhSeg < he ? seg_begin + kMhSeg : he) : 0;
        uint32_t marks = 0, mbits = 0, wbits = 0;  // token starts / matches / older candidate won
        // (segments past the end exist only in the last pass, whose final token ends at n: that is
        // the "exit" the token build reads for them)
        uint32_t my_exit = active ? seg_begin : n;
        // Where the walk can stop: bit k = position seg_begin + k has a candidate (d0 != 0) and is searched at all
        // (p + 5 <= n, the TAIL rule of l1_search).  Every other position is a literal whatever lies around it, so a
        // walk steps over a run of them with one mask operation instead of one wave-step each (text: a fifth of
        // the positions, two fifths of the first walk's lane-steps).  The bits behind a short last segment are set:
        // a run that reaches them has left the segment.  Config.debug bit 3: all ones, a search at every position.
        uint32_t nz = nz_w[tid];
        {
            const uint32_t n_srch = n - 4u > seg_begin ? n - 4u - seg_begin : 0u;  // searched positions from seg_begin on
            if (n_srch < kMhSeg) nz &= (1u << n_srch) - 1u;
            if (seg_end - seg_begin < kMhSeg) nz |= ~0u << (seg_end - seg_begin);  // (inactive lanes never walk)
            if (cfg.debug & 8u) nz = ~0u;
            if (!staged) nz = 0u;
        }
        // (whole waves take the TAIL form of the search together: the last wave of the block)
        const bool tail_wave = __ballot(active && seg_end + 266u > n) != 0;
        auto walk_as = [&](uint32_t pos, auto tail_tag) {
            constexpr bool kTail = decltype(tail_tag)::value;
            const uint32_t o_marks = marks, o_mbits = mbits, o_wbits = wbits;  // (all zero before the first walk)
            marks = mbits = wbits = 0;
            while (pos < seg_end) {
                // the run of candidate-less positions from pos on: literals, up to the next candidate or -- the
                // sequential walk would have looked at each of them -- the next token start of the previous walk
                const uint32_t from = ~0u << (pos - seg_begin);
                const uint32_t stop = (nz | o_marks) & from;
                const uint32_t bit = stop & (0u - stop);  // (0: the run reaches the end of a whole segment)
                marks |= from & (bit - 1u);
                pos = stop ? seg_begin + (uint32_t)__ffs((int)stop) - 1u : seg_end;
                if (pos >= seg_end) break;
                if (o_marks & bit) {
                    // landed on a token start of the previous walk: from here on the two walks are one
                    const uint32_t keep = ~(bit - 1u);
                    marks |= o_marks & keep;
                    mbits |= o_mbits & keep;
                    wbits |= o_wbits & keep;
                    pos = my_exit;
                    break;
                }
                bool older;
                const uint32_t len = l1_search<kTail>(in_w, d0_h, hb, cand, pos, n, mis, older, GZPX_EXP(cfg, 13) != 0);
                marks |= bit;
                if (len) mbits |= bit;
                if (older) wbits |= bit;
                pos += len ? len : 1u;
            }
            my_exit = pos;
        };
        auto walk = [&](uint32_t pos) {
            if (tail_wave) walk_as(pos, std::true_type{});
            else walk_as(pos, std::false_type{});
        };
        uint32_t entry = tid == 0 ? entry_carry : seg_begin;  // thread 0 knows the true entry; the others guess
        if (active) walk(entry);
        // Rounds: every thread reads its left neighbour's exit from one copy of the exit array and
        // leaves its own (re-walked or not) in the other, so one barrier per round is enough -- the
        // one that also tells whether any entry moved.
        uint32_t cur = 0;
        seg_exit[tid] = my_exit;
        // Long runs show at once: their matches fly over whole segments, entries then settle by one
        // segment per round and the block would go to the dense kernels after kMpMaxRounds wasted
        // rounds.  One in eight segments left by a match that overshoots it by two segments or more:
        // hand the block over now (text: none; DNA / FASTQ / low-entropy binary: a few per block).
        const uint32_t n_over = (uint32_t)__syncthreads_count(active && my_exit >= seg_end + 2u * kMhSeg);
        exp_lap(1);
        bool settled = n_over * 8u <= (he - hb + kMhSeg - 1u) / kMhSeg;
        for (uint32_t round = 0; settled; round++) {
            uint32_t new_entry = entry;
            if (active && tid > 0) new_entry = seg_exit[cur * kMpThreads + tid - 1];
            const bool changed = new_entry != entry;
#ifdef GZPX_EXPERIMENT
            if (tid == 0) atomicAdd(&g_exp_cycles[(b & 1023u) * 8u + 5u], 1ull);  // barrier rounds
            {
                const unsigned long long cm = __ballot(changed);
                if (lane == 0 && cm) atomicAdd(&g_exp_cycles[(b & 1023u) * 8u + 6u], (unsigned long long)__popcll(cm));  // re-walks
            }
#endif
            if (changed && round < kMpMaxRounds) {
                entry = new_entry;
                walk(entry);
            }
            cur ^= 1u;
            seg_exit[cur * kMpThreads + tid] = my_exit;
            const bool any = __syncthreads_or(changed);
            exp_lap(2);
            if (!any) break;
            if (round >= kMpMaxRounds) {
                settled = false;
                break;
            }
        }
        // The next block's bytes were requested at the top of this block, a first walk and its rounds ago: they are
        // here.  Saying so in front of this branch covers every way the compiler sees from it to the top of the next
        // block (it keeps one that goes round the hand-back's own wait, for no lane).
        GZPX_BLOCK_ARRIVED();
        if (!settled || (cfg.debug & 4u) || !staged) {  // uniform: the dense kernels take this block (debug bit 2: every block)
            if (tid == 0 && staged) redo[1u + atomicAdd(&redo[0], 1u)] = b;
            handed_back = true;
            GZPX_TURN_LATE();
            break;
        }
        const uint32_t n_seg = (he - hb + kMhSeg - 1) / kMhSeg;
        const uint32_t exit_pos = uniform(seg_exit[cur * kMpThreads + n_seg - 1]);  // where the parse leaves this pass
        exp_lap(3);
        // (uniform) The next pass's d0 -- this block's, or the next block's first, and with that one the ticket -- is
        // requested here, behind the walks (whose rare gather of an older candidate out of global memory waits for
        // everything in flight) and waited for in front of the token build: the scan and the sub-block boundaries
        // cover the round trip, and the only stores still counted there are those of the pass before.
        const bool last_pass = he >= n;
        // (one request whose operands are chosen, not one of two: the compiler keeps a way from the first of two
        // into the second, and would have the second wait for the loads of the first)
        {
            const uint16_t *from = last_pass ? cand_all + (uint64_t)next_b * cfg.stride : cand;
            const uint32_t from_hb = last_pass ? 0u : he, from_n = last_pass ? next_n : n;
            if (!last_pass || next_staged) GZPX_D0_REQUEST(from, from_hb, from_n);
            else GZPX_D0_NONE();
            if (last_pass) draw_ticket();
        }
        if (GZPX_EXP(cfg, 14)) {  // measurement: without the token build
            GZPX_D0_ARRIVED();
            GZPX_HERE_VGPR(my_ticket);
            entry_carry = exit_pos;
            if (last_pass) break;
            continue;
        }

        // ---- phase 2: tokens / matches before every segment (one workgroup scan)
        uint32_t tile_tok, tile_mat, my_pre;
        {
            const uint32_t vt = (uint32_t)__popc(marks), vm = (uint32_t)__popc(mbits);
            // tokens <= 32768 fit 17 bits, matches <= 8192 fit 15 bits: one scan for both
            const uint32_t v = vt | (vm << 17);
            const uint32_t inc = wave_incl_add(v);
            if (lane == 63) wsum_t[wave] = inc;
            __syncthreads();
            // the wave totals: one LDS read per lane and a second DPP scan instead of 16 reads in every lane
            const uint32_t winc = wave_incl_add(lane < kMpWaves ? wsum_t[lane] : 0u);
            const uint32_t tot = rdlane(winc, kMpWaves - 1);
            const uint32_t base = wave ? rdlane(winc, wave - 1) : 0u;
            tile_tok = tot & 0x1FFFFu;
            tile_mat = tot >> 17;
            my_pre = base + inc - v;  // exclusive prefixes: tokens | matches << 17
        }

        // ---- phase 3a: sub-block boundaries.  A new DEFLATE sub-block starts at the first token that
        // has kFastSeqStoreLen matches of the current one before it (deflate_compress_fastest; the byte
        // limit of choose_max_block_end cannot fire in a block of at most one tile).  Match ranks are
        // known from the scan, so every lane names its own first such token and the smallest wins.
        const uint32_t my_mat0 = mat_carry + (my_pre >> 17);   // matches before my first token
        const uint32_t my_tok0 = tok_carry + (my_pre & 0x1FFFFu);  // tokens before it
        for (;;) {
            const uint32_t target = sub_start_mat + kFastSeqStoreLen;
            if (mat_carry + tile_mat < target) break;  // (uniform) the sub-block outlasts this pass
            if (marks) {
                uint32_t k = 32;  // bit of my first token with >= target matches before it
                if (my_mat0 >= target) {
                    k = (uint32_t)__ffs((int)marks) - 1u;
                } else if (my_mat0 + (uint32_t)__popc(mbits) >= target) {
                    uint32_t mb = mbits;  // drop my matches below the target-th one (at most 7 of them)
                    for (uint32_t i = target - my_mat0; i > 1; i--) mb &= mb - 1u;
                    const uint32_t kb = (uint32_t)__ffs((int)mb) - 1u;
                    const uint32_t above = kb < 31u ? marks & ~((2u << kb) - 1u) : 0u;
                    if (above) k = (uint32_t)__ffs((int)above) - 1u;  // (else: the first token of a later segment)
                }
                if (k < 32u)
                    atomicMin(&bnd, ((unsigned long long)(seg_begin + k) << 32) |
                                        (my_tok0 + (uint32_t)__popc(marks & ((1u << k) - 1u))));
            }
            __syncthreads();
            const unsigned long long bv = bnd;
            if (bv == ~0ull) break;  // the token behind the target-th match starts the next pass
            const uint32_t bp = uniform((uint32_t)(bv >> 32)), bti = uniform((uint32_t)bv);
            if (tid == (bp - hb) / kMhSeg)  // the boundary token's segment: matches before that token
                bnd_mat = my_mat0 + (uint32_t)__popc(mbits & ((1u << ((bp - hb) & (kMhSeg - 1u))) - 1u));
            __syncthreads();
            const uint32_t bm = uniform(bnd_mat);
            if (tid == 0) {
                sub[cur_sub].tok_begin = sub_start_tok;
                sub[cur_sub].tok_end = bti;
                sub[cur_sub].byte_begin = sub_start;
                sub[cur_sub].byte_len = bp - sub_start;
                sub[cur_sub].is_final = 0;
                bnd = ~0ull;
            }
            cur_sub++;
            sub_start = bp;
            sub_start_tok = bti;
            sub_start_mat = bm;
            __syncthreads();
        }

        // ---- phase 3b: every lane writes the tokens of its own segment: the length of a match is
        // the distance to the next token start (the next mark, or the segment's exit), its distance
        // d0 or d0 + d0[p - d0] out of LDS again, a literal is the byte itself
        // (in front of the first token store: everything requested for the next pass or the next block has arrived)
        // (the next block's bytes were requested before any of this, at the top of the block: they are complete
        // here without a word about them)
        GZPX_D0_ARRIVED();
        GZPX_HERE_VGPR(my_ticket);
        {
            uint32_t m = marks, ti = my_tok0;
            while (m) {
                const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
                m &= m - 1u;
                const uint32_t p = seg_begin + k;
                const uint32_t next = m ? seg_begin + (uint32_t)__ffs((int)m) - 1u : my_exit;
                uint32_t word = in_b[p];
                if ((mbits >> k) & 1u) {
                    const uint32_t d0 = d0_h[p - hb];
                    uint32_t dist = d0;
                    if ((wbits >> k) & 1u) {
                        const uint32_t q = p - d0;
                        uint32_t r = d0_h[q >= hb ? q - hb : 0u];
                        if (q < hb) r = *(const volatile uint16_t *)(cand + q);
                        dist += r;
                    }
                    word = kTokMatch | (dist << 9) | (next - p);
                }
                tok[ti++] = word;
            }
        }
        tok_carry += tile_tok;
        mat_carry += tile_mat;
        entry_carry = exit_pos;
        exp_lap(4);
        if (last_pass) break;
    }
    if (tid == 0 && !handed_back) {
        sub[cur_sub].tok_begin = sub_start_tok;
        sub[cur_sub].tok_end = tok_carry;
        sub[cur_sub].byte_begin = sub_start;
        sub[cur_sub].byte_len = n - sub_start;
        sub[cur_sub].is_final = 1;
        meta->ntok = tok_carry;
        meta->nsub = cur_sub + 1;
    }
    if (tid == 0) s_claimed = 2u * gridDim.x + my_ticket;
    if (next_b >= nb) break;  // (tickets only grow: nothing is left for this workgroup either)
    __syncthreads();  // s_claimed is written; everybody is done with this block's LDS
    b = next_b;
    staged = next_staged;
    next_b = s_claimed;
  }
#undef GZPX_D0_REQUEST
#undef GZPX_TURN_LATE
#undef GZPX_D0_NONE
#undef GZPX_D0_ARRIVED
#undef GZPX_BLOCK_REQUEST
#undef GZPX_BLOCK_ARRIVED
#undef GZPX_HERE_UINT4
}

// ------------------------------------------------------------------------------------------
// Levels 2-4: deflate_compress_greedy with hc_matchfinder (max_search_depth / nice_match_length:
// 6/10, 12/14, 16/30).  Like the level-1 table, hc_matchfinder inserts every position, so its
// state is parse independent: hash3_tab = "previous position with the same 3-byte hash" (d3) and
// hash4_tab + next_tab = a chain of previous positions with the same 4-byte hash (d4 links).
//
// k_match_hc: hc_matchfinder_longest_match + the greedy acceptance rule for every position of a
// block, in 16 KiB tiles whose LDS window also holds the 32 KiB of history: input bytes (48 KiB)
// and the d4 links of every position a chain can visit (96 KiB), so the whole chain walk (up to
// max_search_depth hops, each a 4-byte check and maybe an lz_extend) runs out of LDS.
//   best_len starts at min_len - 1, where min_len comes from calculate_min_match_len over the
//   first 4096 bytes of the DEFLATE sub-block -- so results depend on the sub-block a position
//   belongs to; HcState.resume_pos / min_len say from where and with which min_len to compute.
// Output: len8[p] = length - 3, which[p] (bit: a match was accepted at p), alt[p] = its distance.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kHcTile = 16384;
constexpr uint32_t kHcInWords = (32768 + kHcTile + 264) / 4 + 8;

// calculate_min_match_len for the sub-block that starts at `start`; all threads of the workgroup
// call it (two barriers), `used` is 8 words of LDS.
__device__ uint32_t hc_calc_min_len(const Config &cfg, const uint8_t *in, uint32_t start, uint32_t n,
                                    uint32_t *used, uint32_t tid, uint32_t nthreads) {
    // (min_len_scan_len and min_len_of_census in this kernel's own text -- a short block is scanned and its census dropped:
    // with the two calls k_parse_hc<true> spills 53 VGPRs, not 43, and levels 3 and 4 lose 0.3 to 0.8 %, gzpx_policy.h)
    uint32_t data_len = max_block_end(start, n, kSoftMaxBlockLen) - start;
    __syncthreads();
    if (tid < 8) used[tid] = 0;
    __syncthreads();
    const bool short_scan = cfg.compat == 0 && data_len < 512;  // libdeflate >= 1.1x
    if (data_len > 4096) data_len = 4096;
    // (Round 4, tried: whole dwords, four loads in flight per thread -- k_parse_lazy calls this with ONE wave, 64 round
    // trips in a row -- no change at levels 6 / 9, k_parse_hc + 0.1 ms: a sub-block starts too rarely to matter.)
    for (uint32_t i = tid; i < data_len; i += nthreads) {
        const uint32_t v = in[start + i];
        atomicOr(&used[v >> 5], 1u << (v & 31u));
    }
    __syncthreads();
    uint32_t num_used = 0;
    for (uint32_t k = 0; k < 8; k++) num_used += (uint32_t)__popc(used[k]);
    return short_scan ? kMinMatchLen : choose_min_match_len(num_used, cfg.hc_depth);
}

// lz_extend for the chain walk: bytes [0, start) of the two strings at LDS byte addresses a / c are known
// to be equal; returns the length of their common prefix, at most max_len (start <= max_len).  The first round
// compares four bytes -- most matches of the bench text end there -- and every later one sixteen (five
// dwords per side at once: a round waits for its LDS reads before it knows whether there is another, and
// the wave pays for its longest lane).  One exit per loop, no break: every extra way out of a divergent loop
// costs scalar mask bookkeeping per round.
#ifndef GZPX_EXT_FIRST
#define GZPX_EXT_FIRST 8
#endif
__device__ __forceinline__ uint32_t lds_extend_from(const uint32_t *in_w, uint32_t a, uint32_t c, uint32_t start,
                                                    uint32_t max_len) {
    uint32_t len = start;
#if GZPX_EXT_FIRST == 8
    {   // eight bytes: three dwords per side
        const uint32_t aa = a + len, cc = c + len;
        const uint32_t *pa = in_w + (aa >> 2), *pc = in_w + (cc >> 2);
        const uint32_t a0 = pa[0], a1 = pa[1], a2 = pa[2], c0 = pc[0], c1 = pc[1], c2 = pc[2];
        const uint32_t sa = aa & 3u, sc = cc & 3u;
        const uint32_t x0 = __builtin_amdgcn_alignbyte(a1, a0, sa) ^ __builtin_amdgcn_alignbyte(c1, c0, sc);
        const uint32_t x1 = __builtin_amdgcn_alignbyte(a2, a1, sa) ^ __builtin_amdgcn_alignbyte(c2, c1, sc);
        const uint32_t x = x0 ? x0 : x1;
        len += (x0 ? 0u : 4u) + (x ? ((uint32_t)(__ffs((int)x) - 1) >> 3) : 4u);
        if (x != 0 || len >= max_len) return len < max_len ? len : max_len;
    }
#else
    {
        const uint32_t x = lds_le32(in_w, a + len) ^ lds_le32(in_w, c + len);
        len += x ? ((uint32_t)(__ffs((int)x) - 1) >> 3) : 4u;
        if (x != 0 || len >= max_len) return len < max_len ? len : max_len;
    }
#endif
    bool more;
    do {
        const uint32_t aa = a + len, cc = c + len;
        const uint32_t *pa = in_w + (aa >> 2), *pc = in_w + (cc >> 2);
        const uint32_t a0 = pa[0], a1 = pa[1], a2 = pa[2], a3 = pa[3], a4 = pa[4];
        const uint32_t c0 = pc[0], c1 = pc[1], c2 = pc[2], c3 = pc[3], c4 = pc[4];
        const uint32_t sa = aa & 3u, sc = cc & 3u;
        const uint32_t x0 = __builtin_amdgcn_alignbyte(a1, a0, sa) ^ __builtin_amdgcn_alignbyte(c1, c0, sc);
        const uint32_t x1 = __builtin_amdgcn_alignbyte(a2, a1, sa) ^ __builtin_amdgcn_alignbyte(c2, c1, sc);
        const uint32_t x2 = __builtin_amdgcn_alignbyte(a3, a2, sa) ^ __builtin_amdgcn_alignbyte(c3, c2, sc);
        const uint32_t x3 = __builtin_amdgcn_alignbyte(a4, a3, sa) ^ __builtin_amdgcn_alignbyte(c4, c3, sc);
        const uint32_t x = x0 ? x0 : x1 ? x1 : x2 ? x2 : x3;
        const uint32_t same = (x0 ? 0u : x1 ? 4u : x2 ? 8u : x3 ? 12u : 16u) + (x ? ((uint32_t)(__ffs((int)x) - 1) >> 3) : 0u);
        len += same;
        more = x == 0 && len < max_len;
    } while (more);
    return len < max_len ? len : max_len;
}

// A staged d4 link that says "no live predecessor" (k_candidates writes 0): any distance above 32767 ends
// a walk, so the test for the end of the chain and the test for the window are one comparison.
constexpr uint32_t kHcNoLink = 0x8000u;
// bit 15 of a match distance in k_match_hc's arrays: the match is with position 0 and lies behind an empty hash3 bucket
// (k_hc_orphan writes it) -- libdeflate finds it only with a search that starts from best_len >= 4
constexpr uint32_t kHcOrphan = 0x8000u;

// hc_matchfinder_longest_match (started from best_len = 2) for the position at LDS byte address a /
// link index li: ONE loop with one chain node per iteration.  libdeflate's two loops ("first node whose
// 4 bytes match", then "a node longer than best_len") differ only in the byte offset of the pre-filter
// word -- 0 while best_len < 4, best_len - 3 after -- and every node costs one unit of depth in both, so
// the lanes of a wave, which sit in different phases, share the loop instead of waiting for each other's.
//   Round 4: the instructions of a node and of a hit are what bounds the kernel (VALU and SALU issue at four
//   waves per SIMD; tools/exp_hc_bounds.py on the round-3 form: 11 more nodes 2.4 ms, the hits without their
//   extension 4.7 ms, the extension 2.6 ms of 16.2), so both are cut to the bone:
//   * a node is its link read, its pre-filter word and three additions -- `tot`, the distance to the node,
//     is the only walk state, "chain over" / "window left" / "nice_len reached" are all `tot > 32767`;
//   * a hit behind the first one (the pre-filter word at best_len - 3 and the first four bytes equal) with
//     best_len <= 7 has bytes [0, best_len + 1) equal -- the two words overlap -- so it IS longer and its
//     extension starts at best_len + 1, usually one four-byte round; only longer best_len (a gap between
//     the two words) extends from 4 like lz_extend does.  Same result: a candidate only ever matters
//     through `len > best_len`;
//   * one position per lane (round 3 walked two together to have two LDS reads in flight: with a node down
//     to a dozen instructions four waves per SIMD cover the read, and the flags that let two chains share
//     a loop cost more than they hid).
//   NV > 1 (the lazy parsers): the searches with depth >> 1 (and >> 2) visit the same nodes in the
//   same order and just stop earlier, so their results are this search's best match at the moment
//   the smaller budget runs out: one stretch of the walk per variant, shortest budget first (if the
//   walk died before a budget ran out nothing changes any more, and that is the final match as well).
template <int NV>
__device__ __forceinline__ void hc_search(const uint32_t *in_w, const uint16_t *link, const uint32_t a,
                                          const uint32_t li, const uint32_t d3v, const uint32_t max_len,
                                          const uint32_t nice_len, const uint32_t depth0, uint32_t (&len_out)[NV],
                                          uint32_t (&dist_out)[NV], const uint32_t dbg = 0,
                                          uint32_t *tot_out = nullptr) {
    const uint32_t seq4 = lds_le32(in_w, a);
    uint32_t best_len = 2, best_dist = 0;
    uint32_t aoff = a;     // a + best_len - 3 once a node of the chain has matched (pre-filter address), a before
    uint32_t mine = seq4;  // the word at aoff
    uint32_t tot = kHcNoLink;  // distance to the node looked at next; > 32767: the walk is over
    if (d3v != 0) {  // (an empty hash3 bucket ends the search before the hash4 chain is looked at)
        if (((lds_le32(in_w, a - d3v) ^ seq4) & 0xFFFFFFu) == 0) {
            best_len = 3;
            best_dist = d3v;
        }
        tot = link[li];
    }
    uint32_t depth = depth0;  // (uniform: a round costs every lane that is still walking one unit)
#pragma unroll
    for (int v = NV - 1; v >= 0; v--) {
        const uint32_t stop = v ? depth0 - (depth0 >> v) : 0u;
        bool go = tot <= 32767u && depth != stop;
        while (go) {  // (one way out, a flag instead of breaks)
            const uint32_t nxt = link[li - tot];
            const uint32_t w = lds_le32(in_w, aoff - tot);
            bool hit = w == mine;
#ifdef GZPX_EXPERIMENT
            if ((dbg >> 11) & 1u) hit = false;
#endif
            uint32_t next_tot = tot + nxt;
            if (hit) {
                const uint32_t ca = a - tot;
                uint32_t start = 4;
                if (aoff != a) {  // behind the first hit: the first four bytes are a second test
                    hit = lds_le32(in_w, ca) == seq4;
                    start = best_len <= 7u ? best_len + 1u : 4u;
                }
                if (hit) {
#ifdef GZPX_EXPERIMENT
                    const uint32_t len = ((dbg >> 10) & 1u) ? (best_len + 1 < max_len ? best_len + 1 : max_len)
                                                            : lds_extend_from(in_w, a, ca, start, max_len);
#else
                    const uint32_t len = lds_extend_from(in_w, a, ca, start, max_len);
#endif
                    if (len > best_len) {
                        best_len = len;
                        best_dist = tot;
                        aoff = a + len - 3u;
                        mine = lds_le32(in_w, aoff);
                        if (len >= nice_len) next_tot = kHcNoLink;
                    }
                }
            }
            tot = next_tot;
            --depth;
            go = tot <= 32767u && depth != stop;
        }
        len_out[v] = best_len;
        dist_out[v] = best_dist;
    }
    // (k_match_hc_sparse) where the walk stands when its budget is used up: > 32767 = it is over -- the chain ended, left
    // the window or reached nice_len -- so a deeper search of this position would return the same match
    if (tot_out) *tot_out = tot;
}

// One workgroup's LDS as ONE array, the window of input bytes first: the byte reads of the walk then
// address LDS from 0 (an immediate offset, no addition per read) and the links sit within the 16-bit
// offset field of ds_read_u16.
constexpr uint32_t kHcLinkWords = (32768 + kHcTile) / 2;  // d4 of every position in the window (u16)
constexpr uint32_t kHcStaleChunk = 4096;  // k_match_hc_stale's unit of work: positions of one block, within one tile
static_assert(kHcTile % kHcStaleChunk == 0 && kHcStaleChunk % 1024 == 0, "a chunk lies in one tile and is whole strides of the workgroup");
constexpr uint32_t kHcLdsWords = kHcInWords + kHcLinkWords + kHcTile / 32;

// The dense search of one block by the calling workgroup (1024 threads), out of `hc_lds` (kHcLdsWords words at LDS address 0):
// k_match_hc's body, and what k_match_hc_sparse does itself with the blocks it does not compact (round 5).
__device__ __forceinline__ void hc_dense_block(uint32_t *hc_lds, const Config &cfg, const uint8_t *__restrict__ slab,
                                               const BlockMeta *__restrict__ meta_all, HcState *__restrict__ hc_all,
                                               const uint16_t *__restrict__ d3_all, const uint16_t *__restrict__ d4_all,
                                               uint8_t *__restrict__ len8_all, uint32_t *__restrict__ mbits_all,
                                               uint16_t *__restrict__ dist_all, uint8_t *__restrict__ lz_len_all,
                                               uint16_t *__restrict__ lz_dist_all, const uint32_t from_pos = 0xFFFFFFFFu,
                                               const bool mark_dense = true, const uint32_t block = 0xFFFFFFFFu,
                                               const uint32_t chunk_lo = 0xFFFFFFFFu) {
    // (from_pos / mark_dense: k_match_hc_sparse handing the REST of a block over -- from the tile that holds from_pos on,
    // the arrays in front of it keep what that kernel wrote, and the block's state stays that kernel's to set;
    // block / chunk_lo: k_match_hc_stale dealing the kHcStaleChunk-position pieces of a few blocks out to its workgroups --
    // only the positions [chunk_lo, chunk_lo + kHcStaleChunk) of the one tile that holds them, its window from memory)
    uint32_t *in_w = hc_lds;                     // 48 KiB window of the block's bytes
    uint32_t *link_w = hc_lds + kHcInWords;      // d4 of every position in the window
    uint32_t *mbits = link_w + kHcLinkWords;
    const uint16_t *link = (const uint16_t *)link_w;
    const uint32_t tid = threadIdx.x;
    const uint32_t b = block != 0xFFFFFFFFu ? block : blockIdx.x;
    const uint32_t n = meta_all[b].n;
    HcState *st = hc_all + b;
    if (n <= cfg.passthrough || st->done) return;  // uniform
    // (round 5) the arrays already hold what the parse needs: k_match_hc_sparse searched the block's token starts, or
    // this kernel has been over the block before
    const uint32_t have = st->sparse;
    if (have == kHcArraysPath || have == kHcArraysDense) return;  // uniform
    const uint8_t *in = slab + (uint64_t)b * cfg.block_size;
    const uint16_t *d3 = d3_all + (uint64_t)b * cfg.stride;
    const uint16_t *d4 = d4_all + (uint64_t)b * cfg.stride;
    uint8_t *len8 = len8_all + (uint64_t)b * cfg.stride;
    uint32_t *mbits_out = mbits_all + (uint64_t)b * (cfg.stride / 32);
    uint16_t *dist = dist_all + (uint64_t)b * cfg.stride;

    // The search starts from best_len = 2 (min_len 3) whatever the sub-block's min_len will be: the
    // chain nodes visited, their order and the depth they cost do not depend on the starting
    // best_len -- it only raises the bar a node must clear -- so the search that libdeflate starts at
    // min_len - 1 returns this very match whenever it is long enough and nothing otherwise.  k_parse_hc
    // applies `len >= min_len`; a sub-block with another min_len re-parses, it does not re-match.
    const uint32_t resume = from_pos != 0xFFFFFFFFu ? from_pos : st->resume_pos;
    const uint32_t min_len = 3;
    const uint32_t nice_level = cfg.hc_nice, depth = GZPX_EXP(cfg, 12) ? 1u : cfg.hc_depth;

    // The window slides: from its second tile on a block keeps what the previous tile's window shares with this one
    // -- up to 32 KiB of bytes and 64 KiB of links, moved down INSIDE the LDS -- and appends the 16 KiB of bytes and
    // 32 KiB of links that are new, which were loaded into registers (5 + 8 dwords a thread; the kernel has 128 VGPRs
    // to itself at one workgroup per CU) while the previous tile was searched.  (Round 4: every tile staged its whole
    // window from HBM, 144 KiB, with the CU's only workgroup waiting for it.)
    auto fix_links = [](uint32_t v) {  // two links; 0 = none
        if ((v & 0xFFFFu) == 0) v |= kHcNoLink;
        if ((v >> 16) == 0) v |= kHcNoLink << 16;
        return v;
    };
    constexpr uint32_t kPfIn = 5, kPfLk = kHcTile / 2 / 1024, kMvIn = (kHcInWords - kHcTile / 4 + 1023) / 1024, kMvLk = 32768 / 2 / 1024;
    uint32_t pf_in[kPfIn], pf_lk[kPfLk];
    uint32_t prev_win = 0, prev_ndw = 0, prev_nlw = 0;  // the window in LDS (prev_ndw = 0: none)
    const bool chunked = chunk_lo != 0xFFFFFFFFu;
    if (chunked && (chunk_lo >= n || chunk_lo + kHcStaleChunk <= resume)) return;  // uniform: nothing of it is parsed again
    const uint32_t tile_first = chunked ? chunk_lo / kHcTile * kHcTile : resume / kHcTile * kHcTile;
    const uint32_t tile_stop = chunked ? (tile_first + kHcTile < n ? tile_first + kHcTile : n) : n;  // (chunked: that one tile)
    for (uint32_t tile_begin = tile_first; tile_begin < tile_stop; tile_begin += kHcTile) {
        const uint32_t tile_end = tile_begin + kHcTile < n ? tile_begin + kHcTile : n;
        // the positions searched: the tile, or the chunk of it that was asked for
        const uint32_t lo = chunked ? chunk_lo : tile_begin;
        const uint32_t hi = chunked && chunk_lo + kHcStaleChunk < tile_end ? chunk_lo + kHcStaleChunk : tile_end;
        const uint32_t win_begin = tile_begin >= 32768u ? tile_begin - 32768u : 0;
        const uint32_t win_end = tile_end + 264 < n ? tile_end + 264 : n;
        const uint32_t mis = (uint32_t)((uintptr_t)(in + win_begin) & 3u);  // (the same for every tile: win_begin is a multiple of four)
        const uint32_t ndw = (mis + (win_end - win_begin) + 3) >> 2;  // dwords of bytes in the window
        const uint32_t nlw = (tile_end - win_begin + 1) / 2;           // dwords of links (win_begin is a multiple of 16384: aligned u16 pairs)
        __syncthreads();
        if (prev_ndw == 0) {  // a block's first tile: everything from memory
            const uint32_t *src = (const uint32_t *)(in + win_begin - mis);
            for (uint32_t i = tid; i < ndw; i += 1024) in_w[i] = src[i];
            const uint32_t *lsrc = (const uint32_t *)(d4 + win_begin);
            for (uint32_t i = tid; i < nlw; i += 1024) link_w[i] = fix_links(lsrc[i]);
        } else {
            const uint32_t sh = win_begin - prev_win;  // 0 while the window still grows, then kHcTile
            const uint32_t keep_in = prev_ndw - sh / 4, keep_lk = prev_nlw - sh / 2;
            if (sh) {
                uint32_t mv_in[kMvIn], mv_lk[kMvLk];
#pragma unroll
                for (uint32_t k = 0; k < kMvIn; k++) mv_in[k] = tid + 1024u * k < keep_in ? in_w[tid + 1024u * k + sh / 4] : 0u;
#pragma unroll
                for (uint32_t k = 0; k < kMvLk; k++) mv_lk[k] = tid + 1024u * k < keep_lk ? link_w[tid + 1024u * k + sh / 2] : 0u;
                __syncthreads();
#pragma unroll
                for (uint32_t k = 0; k < kMvIn; k++)
                    if (tid + 1024u * k < keep_in) in_w[tid + 1024u * k] = mv_in[k];
#pragma unroll
                for (uint32_t k = 0; k < kMvLk; k++)
                    if (tid + 1024u * k < keep_lk) link_w[tid + 1024u * k] = mv_lk[k];
            }
#pragma unroll
            for (uint32_t k = 0; k < kPfIn; k++)
                if (keep_in + tid + 1024u * k < ndw) in_w[keep_in + tid + 1024u * k] = pf_in[k];
#pragma unroll
            for (uint32_t k = 0; k < kPfLk; k++)
                if (keep_lk + tid + 1024u * k < nlw) link_w[keep_lk + tid + 1024u * k] = fix_links(pf_lk[k]);
        }
        for (uint32_t i = ndw + tid; i < ndw + 3 && i < kHcInWords; i += 1024) in_w[i] = 0;
        for (uint32_t i = tid; i < kHcTile / 32; i += 1024) mbits[i] = 0;
        prev_win = win_begin;
        prev_ndw = ndw;
        prev_nlw = nlw;
        if (tile_end < tile_stop) {  // what the next tile's window adds to this one
            const uint32_t nt_end = tile_end + kHcTile < n ? tile_end + kHcTile : n;
            const uint32_t nw_begin = tile_end >= 32768u ? tile_end - 32768u : 0;
            const uint32_t nw_end = nt_end + 264 < n ? nt_end + 264 : n;
            const uint32_t nsh = nw_begin - win_begin;
            const uint32_t n_ndw = (mis + (nw_end - nw_begin) + 3) >> 2, n_nlw = (nt_end - nw_begin + 1) / 2;
            const uint32_t *src = (const uint32_t *)(in + nw_begin - mis) + (ndw - nsh / 4);
            const uint32_t *lsrc = (const uint32_t *)(d4 + nw_begin) + (nlw - nsh / 2);
            const uint32_t more_in = n_ndw - (ndw - nsh / 4), more_lk = n_nlw - (nlw - nsh / 2);
#pragma unroll
            for (uint32_t k = 0; k < kPfIn; k++) pf_in[k] = tid + 1024u * k < more_in ? src[tid + 1024u * k] : 0u;
#pragma unroll
            for (uint32_t k = 0; k < kPfLk; k++) pf_lk[k] = tid + 1024u * k < more_lk ? lsrc[tid + 1024u * k] : 0u;
        }
        // the hash3 distance of a lane's next position travels while it searches the current one.  (Tried: the
        // sixteen of a tile prefetched with the window, packed in eight registers that the loop shifts through, so
        // that no load is waited for inside the loop: level 9 110.5 -> 113.5 ms, the others +0.1 ... 0.4.)
        uint32_t d3_next = lo + tid + 5 <= n && lo + tid < hi ? d3[lo + tid] : 0u;
        __syncthreads();
        uint8_t *lzl = lz_len_all + (uint64_t)b * 2u * cfg.stride;
        uint16_t *lzd = lz_dist_all + (uint64_t)b * 2u * cfg.stride;
        for (uint32_t p = lo + tid; p < hi; p += 1024) {
            // with fewer than 5 bytes left hc_matchfinder_longest_match bails out: d3v = 0 idles the search
            const uint32_t d3v = d3_next;
            const uint32_t pn = p + 1024u;
            d3_next = pn + 5 <= n && pn < hi ? d3[pn] : 0u;
            const uint32_t rem = n - p;
            const uint32_t max_len = rem < 258u ? rem : 258u;
            const uint32_t nice_len = max_len < nice_level ? max_len : nice_level;
            const uint32_t a = p - win_begin + mis, li = p - win_begin;
#ifdef GZPX_EXPERIMENT
            // measurement only (tools/exp_hc_sparse.py): search a pseudo-random share of the positions -- bits 16-22 of the
            // debug word, in 128ths -- and report "no match" for the rest: what would a wave cost whose lanes search only
            // where a token starts?  (the stream stays valid, it just is not libdeflate's)
            if (((cfg.debug >> 16) & 127u) && !cfg.lazy) {
                const uint32_t hsh = (p * 2654435761u + b * 40503u) >> 25;  // 0..127
                if (hsh >= ((cfg.debug >> 16) & 127u)) {
                    len8[p] = 0;
                    dist[p] = (uint16_t)(lds_le32(in_w, a) & 0xFFu);
                    continue;
                }
            }
#endif
            if (cfg.lazy) {  // (uniform)
                // Levels 5-9: the lazy parsers search a position up to three times -- where a decision
                // starts (full depth), as the position after a match (half), as the one after that
                // (lazy2: a quarter) -- from best_len = min_len - 1 or the current match's length - 1.
                // By the argument above each is the min_len-3 search of that depth plus a filter, so all
                // two / three are computed here for every position and k_parse_lazy picks.  No length-3
                // distance rule: the parser applies its own (8192, first search only).
                uint32_t len[3], dst[3];
                hc_search<3>(in_w, link, a, li, d3v, max_len, nice_len, depth, len, dst, cfg.debug);
                for (uint32_t v = 0; v <= cfg.lazy; v++) {
                    const bool have = len[v] >= 3u;
                    uint8_t *lo = v == 0 ? len8 : lzl + (uint64_t)(v - 1) * cfg.stride;
                    uint16_t *dd = v == 0 ? dist : lzd + (uint64_t)(v - 1) * cfg.stride;
                    lo[p] = (uint8_t)(have ? len[v] - 3u : 0u);
                    dd[p] = (uint16_t)(have ? dst[v] : 0u);
                }
                continue;
            }
            uint32_t ln[1], ds[1];
            hc_search<1>(in_w, link, a, li, d3v, max_len, nice_len, depth, ln, ds, cfg.debug);
            const uint32_t len = ln[0], dst = ds[0];
            const bool take = greedy_takes(len, dst, min_len);
            len8[p] = (uint8_t)(take ? len - 3 : 0);
            // val: the match distance, or the literal byte (what k_parse_hc's token needs either way)
            dist[p] = (uint16_t)(take ? dst : lds_le32(in_w, a) & 0xFFu);
            if (take) {
                const uint32_t r = p - tile_begin;
                atomicOr(&mbits[r >> 5], 1u << (r & 31u));
            }
        }
        if (cfg.lazy) continue;  // (uniform; the next tile's loads start behind a barrier)
        __syncthreads();
        for (uint32_t i = (lo - tile_begin) / 32 + tid; i < (hi - tile_begin + 31) / 32; i += 1024)  // (lo: a multiple of 32)
            mbits_out[tile_begin / 32 + i] = mbits[i];
    }
    if (tid == 0 && mark_dense) st->sparse = kHcArraysDense;  // (read at the top by every thread: behind the loop's barriers)
}

__global__ __launch_bounds__(1024) void k_match_hc(Config cfg, const uint8_t *__restrict__ slab,
                                                   const BlockMeta *__restrict__ meta_all,
                                                   HcState *__restrict__ hc_all,
                                                   const uint16_t *__restrict__ d3_all,
                                                   const uint16_t *__restrict__ d4_all,
                                                   uint8_t *__restrict__ len8_all,
                                                   uint32_t *__restrict__ mbits_all,
                                                   uint16_t *__restrict__ dist_all,
                                                   uint8_t *__restrict__ lz_len_all,
                                                   uint16_t *__restrict__ lz_dist_all) {
    __shared__ uint32_t hc_lds[kHcLdsWords];
    hc_dense_block(hc_lds, cfg, slab, meta_all, hc_all, d3_all, d4_all, len8_all, mbits_all, dist_all, lz_len_all, lz_dist_all);
}

// The dense search for the blocks k_parse_hc marked kHcArraysStale (round 5: behind k_match_hc_sparse, between the first
// and the second parse round) -- one in thousands, if any.  k_parse_hc lists them (`stale`: count, then block indices);
// a workgroup per CU deals the list out in pieces of kHcStaleChunk positions, so that ONE stale block is sixteen
// workgroups' work of a few searches per thread and not one workgroup's whole block with 255 CUs idle behind it (a
// slab of text with two stale blocks paid 0.22 ms of its 3.7 for that).  The blocks stay kHcArraysStale: a workgroup
// that set another state here would race the ones still reading it, and no kernel behind this one asks again.
__global__ __launch_bounds__(1024) void k_match_hc_stale(Config cfg, const uint8_t *__restrict__ slab,
                                                         const BlockMeta *__restrict__ meta_all, HcState *__restrict__ hc_all,
                                                         const uint16_t *__restrict__ d3_all, const uint16_t *__restrict__ d4_all,
                                                         uint8_t *__restrict__ len8_all, uint32_t *__restrict__ mbits_all,
                                                         uint16_t *__restrict__ dist_all, const uint32_t *__restrict__ stale) {
    __shared__ uint32_t hc_lds[kHcLdsWords];
    const uint32_t per_block = (cfg.block_size + kHcStaleChunk - 1) / kHcStaleChunk;
    const uint32_t items = stale[0] * per_block;
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t b = stale[1 + item / per_block];
        __syncthreads();  // (the piece before is done with the LDS)
        hc_dense_block(hc_lds, cfg, slab, meta_all, hc_all, d3_all, d4_all, len8_all, mbits_all, dist_all, (uint8_t *)nullptr,
                       (uint16_t *)nullptr, 0xFFFFFFFFu, false, b, (item % per_block) * kHcStaleChunk);
    }
}

// ------------------------------------------------------------------------------------------
// k_match_hc_sparse (round 5; levels 3-4): the COMPACTION form of k_match_hc.
//   libdeflate searches only where a token of the greedy parse starts -- a quarter of the positions of text -- and the
//   lockstep wave of the dense kernel pays for the longest chain walk of its 64 lanes at every position (DESIGN 7:
//   11.9 rounds per wave at level 3, the lanes using 48 % of them).  Here, per tile of a block:
//     A  every position gets the search's FIRST chain node only (hash3 check, one node, its extension): lockstep work, all
//        lanes busy, no divergent loop around it.  For a third of the positions of text that IS the whole search (`fin`).
//     B  the greedy parse over those lengths, as a speculative segment walk (32 positions per thread, one LDS byte per hop),
//        says where tokens start;
//     C  the token starts whose search is not over are listed and dealt out ONE PER LANE for the full search -- full waves
//        of long walks instead of a long walk holding 63 short ones.  A lane whose search changed a length follows the
//        corrected path over the lengths in LDS until it meets the old path, marks what it passes as token starts and
//        appends the open searches among them to the ring: the next round's list, without a walk of the tile (most
//        corrections move the next token start by a byte or two).  Short lists are searched serially by their own lanes.
//     D  when the ring runs dry the segments with a new length walk again and the list is built from the true marks: a
//        pass that finds nothing open on the path ends the tile.  By induction from the tile's entry the path is then
//        libdeflate's: every token start on it has the full search's match, so the next token start is right as well.
//   Positions OFF the path keep their first-node match in len8 / which / alt; k_parse_hc never uses them unless a later
//   sub-block of the block needs another min_len (the path was walked with the first sub-block's) -- it then marks the
//   block kHcArraysStale and the dense kernel goes over it before the next parse round.
//   What does not compact is searched the dense way by this kernel's own workgroup (hc_dense_block, one call site at the
//   end): blocks that can hold an orphan match (k_hc_orphan: one in 65 thousand); blocks whose sample says "noise" (no
//   real hash3 matches) or "open chains everywhere" (small alphabets: DNA, FASTQ, low-entropy binary -- nearly every
//   token start would need the deep search and the corrections cascade); and, from the tile that shows it on, blocks
//   with long matches (entries settle a segment per round) or with most token starts open after the first node.
//   Measured (match + parse, 550 MiB text): level 3 13.97 -> 12.9-13.3 ms, level 4 15.84 -> 14.0-14.3; 256 MiB per
//   class, whole step, against the dense kernel for every block: text - 3 ... - 9 %, repeated phrases - 10 ... - 20 %,
//   DNA / FASTQ / low-entropy / runs / noise + 1 ... + 3 % (the sample and the way round), mixed + 5 %; before the
//   sample and the per-tile tests existed DNA was + 103 %, FASTQ + 94 %, period-2 + 158 %.  Level 2 (six nodes at most:
//   too little behind the first one) stays with the dense kernel.
//   What it is bound by: a correction round is a search's latency (a dependent chain of LDS reads, a hit path in nearly
//   every round of a full wave) with the rest of the CU idle -- half of the kernel's time for a fifth of its instructions.
//   LDS: the window (bytes + links) of a 13,056-position tile (five per BGZF block), the tile's lengths, four bitmaps, ring.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kHsTile = 13056;  // 65280 / 5; a multiple of 256
constexpr uint32_t kHsInWords = (32768 + kHsTile + 264) / 4 + 8;
constexpr uint32_t kHsLinkWords = (32768 + kHsTile) / 2;
constexpr uint32_t kHsSeg = 32;                      // positions per walk segment = one 32-bit mask
constexpr uint32_t kHsSegs = kHsTile / kHsSeg;       // 408
// Ring entries (u16).  A tile's first list is 1,400-1,750 entries on text (tools/sim_hc_compact.py); what does not fit waits
// for the next pass -- and that is not only a loss: the searches of a round are SPECULATION on the path behind the ones
// before them, and an entry listed late is often off the path by the time its turn comes.  Measured (match + parse, ms;
// tools/gpu_r5_ring.sh, level 3 / level 4; english_like seeds 5-9 against the dense kernel, then the bench slab):
//   1,280:  -4.2 +6.9 -1.2 -2.7 +5.7 %   13.27 / 14.18      (the kernel's first size: two texts in five LOSE)
//   1,536:  -4.4 -1.1 -3.8 -4.2 -0.6 %   13.19 / 14.08      <- every text gains, at level 4 by 8-12 %
//   1,792:  -3.6 -1.6 -2.7 -2.8 -0.5 %   13.37 / 14.36
//   2,096:  -0.6 +3.3 -0.3 +0.4 +3.0 %   13.83 / 14.88      (the whole first list in one round: a third of it wasted)
// (Before the exits were u16, at 1,280: 2,048 entries with the accepted-match bits straight to memory and their LDS given
// to the ring -- 13.20 -> 14.19 ms, put down to pass A's global stores then; the table says the ring's size did its share.)
#ifndef GZPX_HS_LIST
#define GZPX_HS_LIST 1536  // (A/B builds: tools/gpu_r5_ring.sh)
#endif
constexpr uint32_t kHsList = GZPX_HS_LIST;
constexpr uint32_t kHsSerial = 128;                  // a list this short: its lanes search what they run into themselves
constexpr uint32_t kHsLdsWords = kHsInWords + kHsLinkWords + kHsTile / 4 + 4 * kHsSegs + kHsSegs + kHsList / 2 + 16;
static_assert(kHsLdsWords * 4 <= 160 * 1024, "k_match_hc_sparse: one workgroup's LDS");
static_assert(kHsTile % 256 == 0 && kHsSegs <= 1024 && kHsTile + 600 < 0xFFFF, "tile geometry (exits are u16; 0xFFFF is the poison)");

__global__ __launch_bounds__(1024) void k_match_hc_sparse(Config cfg, const uint8_t *__restrict__ slab,
                                                          const BlockMeta *__restrict__ meta_all,
                                                          HcState *__restrict__ hc_all,
                                                          const uint16_t *__restrict__ d3_all,
                                                          const uint16_t *__restrict__ d4_all,
                                                          uint8_t *__restrict__ len8_all,
                                                          uint32_t *__restrict__ mbits_all,
                                                          uint16_t *__restrict__ dist_all) {
    __shared__ uint32_t hs_lds[kHsLdsWords];
    uint32_t *in_w = hs_lds;                         // window of the block's bytes (LDS address 0: immediate offsets)
    uint32_t *link_w = in_w + kHsInWords;            // d4 of every position in the window
    uint32_t *len_w = link_w + kHsLinkWords;         // len - 3 of the tile's positions (u8)
    uint32_t *mbits = len_w + kHsTile / 4;           // a match was accepted here (min_len 3: what k_parse_hc reads)
    uint32_t *mbf = mbits + kHsSegs;                 // ... and is long enough for the sub-block's min_len: the walk's mask
    uint32_t *fin = mbf + kHsSegs;                   // the position's search is over: its match is the full search's
    uint32_t *marks = fin + kHsSegs;                 // a token starts here (the current walk)
    uint16_t *seg_exit = (uint16_t *)(marks + kHsSegs);  // [2][kHsSegs] where the walk leaves segment s (tile-relative, u16; 0xFFFF: walk again)
    uint32_t *list_w = marks + 2 * kHsSegs;          // u16 tile-relative positions to search
    uint32_t *misc = list_w + kHsList / 2;           // [0..7] hc_calc_min_len's census, [8] the ring's tail
    const uint16_t *link = (const uint16_t *)link_w;
    uint8_t *len_l = (uint8_t *)len_w;
    uint16_t *list = (uint16_t *)list_w;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t b = blockIdx.x;
    const uint32_t n = meta_all[b].n;
    HcState *st = hc_all + b;
    if (n <= cfg.passthrough || st->done || cfg.lazy) return;  // uniform
    const uint8_t *in = slab + (uint64_t)b * cfg.block_size;
    static_assert(kHcLdsWords <= kHsLdsWords, "the dense search fits this kernel's LDS");
    // (uniform) the block, or what is left of it, is searched the dense way by this very workgroup -- ONE call site at the
    // end of the kernel: four inlined copies of hc_dense_block cost this kernel 52 spilled VGPRs and level 3 on text 10 %
    bool go_dense = false, dense_whole = false;
    uint32_t dense_from = 0;
    const bool depth_is_deep = cfg.hc_depth > 1u;
    {   // a block that may hold an orphan match (k_hc_orphan) is not compacted
        const uint32_t first4 = n >= 9u ? (uint32_t)in[0] | (uint32_t)in[1] << 8 | (uint32_t)in[2] << 16 | (uint32_t)in[3] << 24 : 1u;
        if (n >= 9u && lz_hash(first4, 16) == 0) go_dense = dense_whole = true;  // uniform
    }
    const uint16_t *d3 = d3_all + (uint64_t)b * cfg.stride;
    const uint16_t *d4 = d4_all + (uint64_t)b * cfg.stride;
    uint8_t *len8 = len8_all + (uint64_t)b * cfg.stride;
    uint32_t *mbits_out = mbits_all + (uint64_t)b * (cfg.stride / 32);
    uint16_t *dist = dist_all + (uint64_t)b * cfg.stride;
#ifdef GZPX_EXPERIMENT
    // measurement builds (tools/exp_hc_sparse2.py): thread 0's clock per phase, summed over the blocks of a launch:
    // 0 window, 1 first nodes (A), 2 walks (B, D), 3 lists, 4 searches (C), 5 rounds, 6 listed searches, 7 tiles
    unsigned long long exp_t = __builtin_readcyclecounter();
    auto exp_lap = [&](uint32_t slot) {
        const unsigned long long t = __builtin_readcyclecounter();
        if (tid == 0) atomicAdd(&g_exp_sparse[(b & 1023u) * 8u + slot], t - exp_t);
        exp_t = t;
    };
    auto exp_count = [&](uint32_t slot, uint32_t v) {
        if (tid == 0) atomicAdd(&g_exp_sparse[(b & 1023u) * 8u + slot], (unsigned long long)v);
    };
#else
    auto exp_lap = [](uint32_t) {};
    auto exp_count = [](uint32_t, uint32_t) {};
#endif

    {   // Does this block compact at all?  Asked of 1,024 positions of the first tile's upper half (their chains have some
        // history), straight from memory, before anything is staged:
        //  * noise has no chains to walk: how many samples have a predecessor with the same three bytes (an occupied hash3
        //    bucket alone says little: random data fills the table by collisions) -- under one in eight: dense;
        //  * small alphabets have long chains everywhere: how many samples' searches are still OPEN behind their first chain
        //    node (a second live node follows it) -- DNA 99 %, FASTQ and low-entropy binary 92 %, text 62 %: over four in
        //    five, nearly every token start would need the deep search and the corrections would cascade (measured before
        //    this test: DNA + 103 %, FASTQ + 94 % against the dense kernel): dense.
        // The dense search is then done by this very workgroup (hc_dense_block at the end of the kernel).
        const uint32_t t0 = n < kHsTile ? n : kHsTile;
        const uint32_t p = t0 / 2u + t0 / 2048u * tid;  // (t0 >= 4096 or nothing is sampled: small blocks go the sparse way)
        bool real = false, open = false;
        if (t0 >= 4096u && p + 5u <= t0) {
            const uint32_t d = d3[p], l1 = d4[p];
            real = d != 0 && in[p] == in[p - d] && in[p + 1] == in[p - d + 1] && in[p + 2] == in[p - d + 2];
            if (d != 0 && l1 != 0) {
                const uint32_t l2 = d4[p - l1];
                open = l2 != 0 && l1 + l2 <= 32767u;
            }
        }
        const uint32_t n_real = (uint32_t)__syncthreads_count(real), n_open = (uint32_t)__syncthreads_count(open);
        if (t0 >= 4096u && (n_real * 8u < 1024u || (n_open * 5u > 1024u * 4u && depth_is_deep)) && !(cfg.debug & 32u))
            go_dense = dense_whole = true;  // uniform
    }
    // the first sub-block's min_len (calculate_min_match_len): the path is walked with it, k_parse_hc parses with it
    const uint32_t min_len = go_dense ? 0u : hc_calc_min_len(cfg, in, 0, n, misc, tid, 1024);  // (uniform)
    const uint32_t nice_level = cfg.hc_nice, depth = cfg.hc_depth;

    auto fix_links = [](uint32_t v) {  // two links; 0 = none
        if ((v & 0xFFFFu) == 0) v |= kHcNoLink;
        if ((v >> 16) == 0) v |= kHcNoLink << 16;
        return v;
    };
    // the window slides inside the LDS and what is new arrives in registers, as in k_match_hc
    constexpr uint32_t kPfIn = (kHsTile / 4 + 1023) / 1024, kPfLk = (kHsTile / 2 + 1023) / 1024;
    constexpr uint32_t kMvIn = (kHsInWords + 1023) / 1024, kMvLk = (32768 / 2 + 1023) / 1024;
    uint32_t pf_in[kPfIn], pf_lk[kPfLk];
    uint32_t prev_win = 0, prev_ndw = 0, prev_nlw = 0;
    uint32_t entry_carry = 0;  // where the parse enters the tile (block position; uniform)
    for (uint32_t tile_begin = 0; tile_begin < n && !go_dense; tile_begin += kHsTile) {
        const uint32_t tile_end = tile_begin + kHsTile < n ? tile_begin + kHsTile : n;
        const uint32_t tile_len = tile_end - tile_begin;
        const uint32_t n_seg = (tile_len + kHsSeg - 1) / kHsSeg;
        const uint32_t win_begin = tile_begin >= 32768u ? tile_begin - 32768u : 0;
        const uint32_t win_end = tile_end + 264 < n ? tile_end + 264 : n;
        const uint32_t mis = (uint32_t)((uintptr_t)(in + win_begin) & 3u);  // (the same for every tile: win_begin is a multiple of 256)
        const uint32_t ndw = (mis + (win_end - win_begin) + 3) >> 2;
        const uint32_t nlw = (tile_end - win_begin + 1) / 2;
        __syncthreads();
        if (prev_ndw == 0) {  // a block's first tile: everything from memory
            const uint32_t *src = (const uint32_t *)(in + win_begin - mis);
            for (uint32_t i = tid; i < ndw; i += 1024) in_w[i] = src[i];
            const uint32_t *lsrc = (const uint32_t *)(d4 + win_begin);
            for (uint32_t i = tid; i < nlw; i += 1024) link_w[i] = fix_links(lsrc[i]);
        } else {
            const uint32_t sh = win_begin - prev_win;  // 0 while the window still grows
            const uint32_t keep_in = prev_ndw - sh / 4, keep_lk = prev_nlw - sh / 2;
            if (sh) {
                uint32_t mv_in[kMvIn], mv_lk[kMvLk];
#pragma unroll
                for (uint32_t k = 0; k < kMvIn; k++) mv_in[k] = tid + 1024u * k < keep_in ? in_w[tid + 1024u * k + sh / 4] : 0u;
#pragma unroll
                for (uint32_t k = 0; k < kMvLk; k++) mv_lk[k] = tid + 1024u * k < keep_lk ? link_w[tid + 1024u * k + sh / 2] : 0u;
                __syncthreads();
#pragma unroll
                for (uint32_t k = 0; k < kMvIn; k++)
                    if (tid + 1024u * k < keep_in) in_w[tid + 1024u * k] = mv_in[k];
#pragma unroll
                for (uint32_t k = 0; k < kMvLk; k++)
                    if (tid + 1024u * k < keep_lk) link_w[tid + 1024u * k] = mv_lk[k];
            }
#pragma unroll
            for (uint32_t k = 0; k < kPfIn; k++)
                if (keep_in + tid + 1024u * k < ndw) in_w[keep_in + tid + 1024u * k] = pf_in[k];
#pragma unroll
            for (uint32_t k = 0; k < kPfLk; k++)
                if (keep_lk + tid + 1024u * k < nlw) link_w[keep_lk + tid + 1024u * k] = fix_links(pf_lk[k]);
        }
        for (uint32_t i = ndw + tid; i < ndw + 3 && i < kHsInWords; i += 1024) in_w[i] = 0;
        if (tid == 0) misc[8] = 0;
        prev_win = win_begin;
        prev_ndw = ndw;
        prev_nlw = nlw;
        if (tile_end < n) {  // what the next tile's window adds to this one
            const uint32_t nt_end = tile_end + kHsTile < n ? tile_end + kHsTile : n;
            const uint32_t nw_begin = tile_end >= 32768u ? tile_end - 32768u : 0;
            const uint32_t nw_end = nt_end + 264 < n ? nt_end + 264 : n;
            const uint32_t nsh = nw_begin - win_begin;
            const uint32_t n_ndw = (mis + (nw_end - nw_begin) + 3) >> 2, n_nlw = (nt_end - nw_begin + 1) / 2;
            const uint32_t *src = (const uint32_t *)(in + nw_begin - mis) + (ndw - nsh / 4);
            const uint32_t *lsrc = (const uint32_t *)(d4 + nw_begin) + (nlw - nsh / 2);
            const uint32_t more_in = n_ndw - (ndw - nsh / 4), more_lk = n_nlw - (nlw - nsh / 2);
#pragma unroll
            for (uint32_t k = 0; k < kPfIn; k++) pf_in[k] = tid + 1024u * k < more_in ? src[tid + 1024u * k] : 0u;
#pragma unroll
            for (uint32_t k = 0; k < kPfLk; k++) pf_lk[k] = tid + 1024u * k < more_lk ? lsrc[tid + 1024u * k] : 0u;
        }
        uint32_t d3_next = tile_begin + tid + 5 <= n && tile_begin + tid < tile_end ? d3[tile_begin + tid] : 0u;
        __syncthreads();
        exp_lap(0);

        // one position's search with `budget` nodes; the LDS lengths and bitmaps are the caller's to update
        auto search = [&](uint32_t p, uint32_t d3v, uint32_t budget, uint32_t &len, uint32_t &dst, bool &over) {
            const uint32_t rem = n - p;
            const uint32_t max_len = rem < 258u ? rem : 258u;
            const uint32_t nice_len = max_len < nice_level ? max_len : nice_level;
            const uint32_t a = p - win_begin + mis, li = p - win_begin;
            uint32_t ln[1], ds[1], tot;
            hc_search<1>(in_w, link, a, li, d3v, max_len, nice_len, budget, ln, ds, 0, &tot);
            len = ln[0];
            dst = ds[0];
            over = tot > 32767u;
        };

        // ---- A: the first chain node of every position
        for (uint32_t r0 = 0; r0 < tile_len; r0 += 1024) {  // (uniform trip count: the ballots below need whole waves)
            const uint32_t r = r0 + tid, p = tile_begin + r;
            const bool have = r < tile_len;
            const uint32_t d3v = d3_next;
            const uint32_t pn = p + 1024u;
            d3_next = pn + 5 <= n && pn < tile_end ? d3[pn] : 0u;
            uint32_t len = 0, dst = 0;
            bool over = true;
            if (have) search(p, d3v, 1u, len, dst, over);
            if (depth <= 1u) over = true;
            const bool take = have && greedy_takes(len, dst, kMinMatchLen);
            const unsigned long long bt = __ballot(take), bf = __ballot(take && len >= min_len), bo = __ballot(over || !have);
            if (have) {
                len_l[r] = (uint8_t)(take ? len - 3u : 0u);
                len8[p] = (uint8_t)(take ? len - 3u : 0u);
                dist[p] = (uint16_t)(take ? dst : lds_le32(in_w, p - win_begin + mis) & 0xFFu);
            }
            if (lane == 0 && r < tile_len + 64u) {  // (a wave covers two words of each bitmap)
                const uint32_t w = r >> 5;
                if (w < kHsSegs) {
                    mbits[w] = (uint32_t)bt;
                    mbf[w] = (uint32_t)bf;
                    fin[w] = (uint32_t)bo;
                }
                if (w + 1 < kHsSegs) {
                    mbits[w + 1] = (uint32_t)(bt >> 32);
                    mbf[w + 1] = (uint32_t)(bf >> 32);
                    fin[w + 1] = (uint32_t)(bo >> 32);
                }
            }
        }
        __syncthreads();
        exp_lap(1);

        // ---- B: the greedy parse over the lengths in LDS; thread s walks segment s from `pos` (tile-relative)
        auto walk_seg = [&](uint32_t sg, uint32_t pos) -> uint32_t {
            const uint32_t sb = sg * kHsSeg, se = sb + kHsSeg < tile_len ? sb + kHsSeg : tile_len;
            const uint32_t mbm = mbf[sg];
            uint32_t mk = 0;
            while (pos < se) {
                const uint32_t rel = pos - sb;
                const uint32_t rest = mbm >> rel;
                if (rest == 0) {  // literals to the end of the segment
                    mk |= ~0u << rel;
                    pos = se;
                    break;
                }
                const uint32_t k = (uint32_t)__ffs((int)rest) - 1u;  // literals rel .. rel+k-1, a match at rel+k
                mk |= ((2u << k) - 1u) << rel;
                pos = sb + rel + k + (uint32_t)len_l[sb + rel + k] + 3u;
            }
            if (se - sb < 32u) mk &= (1u << (se - sb)) - 1u;
            marks[sg] = mk;
            return pos;
        };
        const bool active = tid < n_seg;
        const uint32_t seg_begin = tid * kHsSeg;
        uint32_t entry = tid == 0 ? entry_carry - tile_begin : seg_begin;
        uint32_t my_exit = active ? walk_seg(tid, entry) : 0u;
        uint32_t cur = 0;
        if (active) seg_exit[tid] = (uint16_t)my_exit;
        // Two kinds of input do not compact, and the first walk of a tile tells (measured, 256 MiB per class, level 3 against
        // the dense kernel: DNA + 103 %, FASTQ + 94 %, low-entropy binary + 93 %, period-2 + 158 %, byte runs + 13 % before
        // this test; text - 4 %, repeated phrases - 11 %):
        //  * long matches -- segments left by a match that overshoots them by two segments or more: entries then settle one
        //    segment per round (what k_mparse hands its blocks back for);
        //  * small alphabets with long chains -- nearly every token start still has its search open after the first node
        //    (DNA: 96 % of them, FASTQ 74 %; text 18 %), so there is nothing to save and the corrections cascade.
        // The rest of the block then goes the dense way, by this workgroup, from this tile on.
        const uint32_t n_over = (uint32_t)__syncthreads_count(active && my_exit >= seg_begin + kHsSeg + 2u * kHsSeg);
        bool dense_rest = n_over * 8u > n_seg && !(cfg.debug & 32u);
        bool dirty = false;  // a search changed a length in my segment
        for (uint32_t pass = 0; !dense_rest; pass++) {
            // the entries settle: one barrier per round, two copies of the exits (as in k_mparse)
            for (;;) {
                __syncthreads();
                uint32_t new_entry = entry;
                if (active && tid > 0) new_entry = seg_exit[cur * kHsSegs + tid - 1];
                const bool changed = active && (new_entry != entry || dirty);
                dirty = false;
                if (changed) {
                    entry = new_entry;
                    my_exit = walk_seg(tid, entry);
                }
                cur ^= 1u;
                if (active) seg_exit[cur * kHsSegs + tid] = (uint16_t)my_exit;
                if (!__syncthreads_or(changed)) break;
            }
            exp_lap(2);
            // ---- C: the token starts whose search is not over go on the list (a ring of kHsList entries)
            if (tid < ((n_seg + 63u) & ~63u)) {  // (whole waves: one atomic per wave -- 400 lanes at one LDS word are 400 turns)
                uint32_t need = active ? marks[tid] & ~fin[tid] : 0u;
                if (pass >= 12u && active) need = ~fin[tid] & (seg_begin + 32u <= tile_len ? ~0u : (1u << (tile_len - seg_begin)) - 1u);  // give up predicting: every open search of the tile
                const uint32_t cnt = (uint32_t)__popc(need);
                const uint32_t inc = wave_incl_add(cnt);
                uint32_t base = 0;
                if (lane == 63) base = atomicAdd(&misc[8], inc);
                uint32_t at = rdlane(base, 63) + inc - cnt;
                while (need && at < kHsList) {  // (what does not fit is found again by the next pass.  Measured: lists of
                    // 1,024 -- one search per thread -- with the rest listed again without a walk: 27.7 rounds per block
                    // instead of 18.6, level 3 match + parse 13.33 -> 13.75 ms)
                    list[at++] = (uint16_t)(seg_begin + (uint32_t)__ffs((int)need) - 1u);
                    need &= need - 1u;
                }
            }
            __syncthreads();
            uint32_t head = 0, tail = misc[8] < kHsList ? misc[8] : kHsList;
            exp_lap(3);
            if (pass == 0 && misc[8] * 4u > tile_len && !(cfg.debug & 32u)) dense_rest = true;  // (uniform; misc[8] counts what did not fit too)
            if (dense_rest) break;
            if (tail == 0) break;  // uniform: the path holds only finished searches
            __syncthreads();       // (everybody has read the count)
            if (tid == 0) misc[8] = tail;
            __syncthreads();
            // Rounds without a walk of the whole tile: one listed search per lane; a lane whose search changed a length follows
            // the corrected path over the lengths in LDS until it meets the old one again, marks what it passes as token
            // starts and appends the open searches among them to the ring -- the next round's list.  Marks that fall off
            // the path stay behind and a walk may stop at one too early: the pass that follows (walks from the poisoned
            // segments on, list from the true marks) finds what that missed; it is empty nearly every time.
            while (head < tail) {  // (on entry: misc[8] == tail is visible, the ring's entries [head, tail) are complete)
                exp_count(5, 1);
                exp_count(6, tail - head);
                // A short list (the later rounds of a tile) leaves most lanes idle anyway: its lanes then search what their
                // walk runs into themselves, one position after the other, instead of handing it to another round (a
                // round is a search's latency plus two barriers for the whole CU, however few lanes work in it)
                const bool serial = tail - head <= kHsSerial;
                for (uint32_t i = head + tid; i < tail; i += 1024) {
                  uint32_t r = list[i % kHsList];
                  for (uint32_t chain = 0;; chain++) {
                    uint32_t follow = 0xFFFFFFFFu;
                    const uint32_t bit = 1u << (r & 31u);
                    if (chain == 0 && (fin[r >> 5] & bit)) break;  // (listed twice)
                    const uint32_t p = tile_begin + r;
                    uint32_t len, dst;
                    bool over;
                    search(p, p + 5 <= n ? (uint32_t)d3[p] : 0u, depth, len, dst, over);
                    const bool take = greedy_takes(len, dst, kMinMatchLen);
                    const bool had = (mbf[r >> 5] & bit) != 0;
                    const uint32_t old_step = had ? (uint32_t)len_l[r] + 3u : 1u;  // what the walk took here so far
                    uint32_t step = old_step;
                    atomicOr(&fin[r >> 5], bit);
                    if (take && (!had || len != old_step)) {  // (a deeper search only ever finds longer matches: bits are set, never cleared)
                        len_l[r] = (uint8_t)(len - 3u);
                        len8[p] = (uint8_t)(len - 3u);
                        dist[p] = (uint16_t)dst;
                        atomicOr(&mbits[r >> 5], bit);
                        if (len >= min_len) {
                            atomicOr(&mbf[r >> 5], bit);
                            step = len;
                        }
                    }
                    if (step == old_step) break;
                    seg_exit[(cur ^ 1u) * kHsSegs + (r >> 5)] = 0xFFFFu;  // the segment walks again in the next pass
                    uint32_t q = r + step;
                    for (uint32_t hop = 0; hop < 16u && q < tile_len; hop++) {
                        const uint32_t qb = 1u << (q & 31u);
                        if (atomicOr(&marks[q >> 5], qb) & qb) break;  // the old path (or somebody else's new one)
                        if (!(fin[q >> 5] & qb)) {
                            if (serial && chain < 8u) {
                                follow = q;  // (its own search says where the path goes on from there)
                                break;
                            }
                            const uint32_t at = atomicAdd(&misc[8], 1u);
                            if (at - head < kHsList) list[at % kHsList] = (uint16_t)q;  // (else: the next pass finds it)
                        }
                        q += (mbf[q >> 5] & qb) ? (uint32_t)len_l[q] + 3u : 1u;
                    }
                    if (follow == 0xFFFFFFFFu) break;
                    r = follow;
                  }
                }
                __syncthreads();
                const uint32_t ring_end = head + kHsList;  // entries from here on were dropped, not stored
                const uint32_t appended = misc[8];
                head = tail;
                tail = appended < ring_end ? appended : ring_end;
                __syncthreads();  // (everybody has read the ring's tail: the next round may append)
                if (appended > ring_end) {  // uniform, rare: the counter goes back to the last entry that was stored
                    if (tid == 0) misc[8] = tail;
                    __syncthreads();
                }
            }
            __syncthreads();
            if (tid == 0) misc[8] = 0;
            // ---- D: segments with a new length walk again (their exit in the copy nobody reads was poisoned)
            if (active) dirty = seg_exit[(cur ^ 1u) * kHsSegs + tid] == 0xFFFFu;
            exp_lap(4);
        }
        if (dense_rest) {  // uniform
            go_dense = true;
            dense_from = tile_begin;
            break;
        }
        entry_carry = tile_begin + uniform(seg_exit[cur * kHsSegs + n_seg - 1]);
        // the accepted-match bits of the tile (k_parse_hc reads them); tile_begin is a multiple of 32
        for (uint32_t i = tid; i < (tile_len + 31) / 32; i += 1024) mbits_out[tile_begin / 32 + i] = mbits[i];
        exp_count(7, 1);
    }
    if (go_dense) {  // uniform
        __syncthreads();
        hc_dense_block(hs_lds, cfg, slab, meta_all, hc_all, d3_all, d4_all, len8_all, mbits_all, dist_all, (uint8_t *)nullptr,
                       (uint16_t *)nullptr, dense_from, dense_whole);
        if (dense_whole) return;  // (the block's state is kHcArraysDense)
    }
    if (tid == 0) {
        st->min_len = min_len;
        st->sparse = kHcArraysPath;
    }
}

// ------------------------------------------------------------------------------------------
// k_hc_orphan: position 0 and the hash3 gate (levels 2-9; one wave per block, behind k_match_hc).
//   libdeflate files a buffer's first position under bucket 0 of BOTH hc_matchfinder tables (next_hashes starts as
//   {0, 0}), not under its own hashes.  A search that starts from best_len < 4 gives up at once when its hash3 bucket
//   is empty; one that starts from best_len >= 4 (min_len >= 5, or a lazy lookahead behind a match of >= 5) never looks
//   at hash3 and walks the hash4 chain.  k_match_hc searches every position once, from best_len 2, behind the gate --
//   and for every position but one the two kinds of search agree, because four equal bytes imply an occupied hash3
//   bucket.  The exception ("orphan") is the first later position with the buffer's first four bytes, when those hash
//   to hash4 bucket 0: position 0 is in its chain but not in its hash3 bucket.  One buffer in ~ 65 thousand starts that
//   way; the round-4 soak found one (seed 20260928, 'repeats', level 7: a stream one byte longer than libdeflate's).
//   Nothing else in that chain can have the position's four bytes, so its ungated search is: follow the chain to
//   position 0, within the depth budget, and extend.  This kernel does that for the one position per block that can
//   have it and writes the result over k_match_hc's "no match" with bit 15 of the distance set; the parsers use a
//   marked match only where libdeflate's search would have started at >= 4 (k_parse_hc: sub-blocks with min_len >= 5,
//   the position is in HcState.pad; k_parse_lazy: min_len >= 5 for a decision's first search, cur_len >= 5 for a
//   lookahead).  All but one block in 65 thousand leave after one load.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_hc_orphan(Config cfg, const uint8_t *__restrict__ slab,
                                                  const BlockMeta *__restrict__ meta_all, HcState *__restrict__ hc_all,
                                                  const uint16_t *__restrict__ d3_all, const uint16_t *__restrict__ d4_all,
                                                  uint8_t *__restrict__ len8_all, uint32_t *__restrict__ mbits_all,
                                                  uint16_t *__restrict__ dist_all, uint8_t *__restrict__ lz_len_all,
                                                  uint16_t *__restrict__ lz_dist_all) {
    const uint32_t lane = threadIdx.x, b = blockIdx.x;
    const uint32_t n = meta_all[b].n;
    if (n <= cfg.passthrough || n < 9u) return;  // (uniform)
    const uint8_t *in = slab + (uint64_t)b * cfg.block_size;
    auto le32 = [&](uint32_t p) {
        return (uint32_t)in[p] | (uint32_t)in[p + 1] << 8 | (uint32_t)in[p + 2] << 16 | (uint32_t)in[p + 3] << 24;
    };
    const uint32_t first4 = le32(0);
    if (lz_hash(first4, 16) != 0) return;  // position 0 sits in hash4 bucket 0 and in no other chain
    const uint16_t *d3 = d3_all + (uint64_t)b * cfg.stride;
    const uint16_t *d4 = d4_all + (uint64_t)b * cfg.stride;
    // the orphan: four bytes like the buffer's first, an empty hash3 bucket (at most one position: the next one with
    // those bytes finds this one in the bucket), position 0 still inside the window, five bytes left to hash
    const uint32_t last = (n - 5u < 32767u ? n - 5u : 32767u);
    uint32_t at = 0;
    for (uint32_t base = 1; base <= last && at == 0; base += 64) {
        const uint32_t p = base + lane;
        const bool hit = p <= last && d3[p] == 0 && le32(p) == first4;
        const unsigned long long m = __ballot(hit);
        if (m) at = base + (uint32_t)__ffsll((long long)m) - 1u;
    }
    if (at == 0) return;
    // position 0's place in the chain, and the match
    uint32_t pos = at, nodes = 0;
    bool found = false;
    const uint32_t depth = cfg.hc_depth;
    while (nodes < depth) {
        const uint32_t d = d4[pos];
        if (d == 0 || d > pos) break;
        pos -= d;
        nodes++;
        if (pos == 0) {
            found = true;
            break;
        }
    }
    if (!found) return;
    const uint32_t max_len = n - at < 258u ? n - at : 258u;
    uint32_t len = 4;
    for (;;) {  // 64 bytes a step
        const uint32_t i = len + lane;
        const unsigned long long ne = __ballot(i >= max_len || in[i] != in[at + i]);
        if (ne) {
            len += (uint32_t)__ffsll((long long)ne) - 1u;
            break;
        }
        len += 64;
    }
    if (lane != 0) return;
    uint8_t *len8 = len8_all + (uint64_t)b * cfg.stride;
    uint16_t *dist = dist_all + (uint64_t)b * cfg.stride;
    if (cfg.lazy) {  // the half / quarter depth searches reach position 0 if it is that near in the chain
        for (uint32_t v = 0; v <= cfg.lazy; v++) {
            if (nodes > (depth >> v)) continue;
            uint8_t *lo = v == 0 ? len8 : lz_len_all + ((uint64_t)b * 2u + (v - 1)) * cfg.stride;
            uint16_t *dd = v == 0 ? dist : lz_dist_all + ((uint64_t)b * 2u + (v - 1)) * cfg.stride;
            lo[at] = (uint8_t)(len - 3u);
            dd[at] = (uint16_t)(at | kHcOrphan);
        }
        return;
    }
    len8[at] = (uint8_t)(len - 3u);
    dist[at] = (uint16_t)(at | kHcOrphan);
    atomicOr(mbits_all + (uint64_t)b * (cfg.stride / 32) + at / 32u, 1u << (at & 31u));
    hc_all[b].pad = at + 1u;
}

// ------------------------------------------------------------------------------------------
// k_parse_hc: the greedy parse, token stream and sub-block boundaries of deflate_compress_greedy,
// per block in tiles of 32 KiB positions.  Walkers / ranks / token build as in k_parse (a match
// is flagged by a bit, because length 3 shares len8 == 0 with "literal").  A sub-block ends at
//   - the 300000-byte soft limit (choose_max_block_end) or after 50000 matches, or
//   - where should_end_block says so: every 512 tokens (once 5000 bytes are in and 5000 remain)
//     the histogram of 10 observation classes since the last check is compared with the
//     block's so far (do_end_block_check).
// The class counts per 512-token bin are gathered in parallel and all checks of a tile evaluated side
// by side from their prefix sums.  When the sub-block that follows a boundary needs a different
// min_len, the "long enough" filter of the matches from there on was the wrong one: the workgroup
// parses the block again from there (another "round" of its own loop; k_match_hc's results stand:
// they do not depend on min_len).
// ------------------------------------------------------------------------------------------
constexpr uint32_t kHpTile = 32768;  // (a BGZF block is two full tiles; ~50 KiB of LDS: three workgroups per CU.  48 KiB tiles: +0.3 ms per 550 MiB)
constexpr uint32_t kHpGroups = kHpTile / 64;  // 512 groups / walk segments of 64 positions
constexpr uint32_t kHpMaxBins = kHpTile / 512 + 3;
constexpr uint32_t kNoCheckYet = 0xFFFFFFFFu, kNoMoreChecks = 0xFFFFFFFEu;

// mask of the bit positions above the k-th set bit of m (k >= 1; 0 if m has fewer)
__device__ __forceinline__ unsigned long long mask_after_kth(unsigned long long m, uint32_t k) {
    unsigned long long t = m;
    for (uint32_t i = 1; i < k && t; i++) t &= t - 1;  // drop the k - 1 lowest
    if (!t) return 0;
    const unsigned long long kth = t & (~t + 1);
    return ~((kth << 1) - 1);
}

#ifndef GZPX_PHC_WAVES
#define GZPX_PHC_WAVES 8
#endif
template <bool LOOP>
__global__ __launch_bounds__(kMpThreads, GZPX_PHC_WAVES) void k_parse_hc(
    Config cfg, const uint8_t *__restrict__ slab, BlockMeta *__restrict__ meta_all,
    SubMeta *__restrict__ sub_all, HcState *__restrict__ hc_all, const uint8_t *__restrict__ len8_all,
    const uint32_t *__restrict__ mbits_all, const uint16_t *__restrict__ val_all,
    uint32_t *__restrict__ tok_all, uint32_t *__restrict__ pending, uint32_t *__restrict__ stale, uint32_t may_list_stale) {
    __shared__ uint32_t len8_w[kHpTile / 4];
    __shared__ unsigned long long tok_bits[kHpGroups];  // 1 = a token starts here (tile-relative)
    __shared__ unsigned long long mb[kHpGroups];        // 1 = k_match_hc's match here is long enough for min_len
    __shared__ unsigned long long mraw[kHpGroups];      // k_match_hc's own bits (min_len 3): the too-short matches are mraw & ~mb
    __shared__ uint32_t rank_pre[kHpGroups];            // walk: exit of segment s; then (tokens | matches << 17) before group s
    __shared__ uint32_t rescue[2];
    __shared__ uint32_t wsum_t[kMpWaves], wsum_m[kMpWaves];
    __shared__ unsigned long long bnd;  // limit / sequence-count boundary: (position << 32 | token)
    __shared__ uint32_t bnd_tok, bnd_mat;
    __shared__ uint32_t first_check;                // candidate for the first split check (token index)
    __shared__ uint32_t bins[kHpMaxBins][10];       // observation classes per 512-token bin
    __shared__ uint32_t cum[kHpMaxBins + 1][10];    // their exclusive prefix over the bins
    __shared__ uint32_t first_evt;                  // first check that ends the sub-block or the checking
    __shared__ uint32_t chk_end[kHpMaxBins];        // end position of every check token
    __shared__ uint32_t split_pos;                  // where should_end_block ended the sub-block
    __shared__ uint32_t s_next_check, s_obs[10], s_new[10];
    __shared__ uint32_t used[8];
    const uint8_t *len8 = (const uint8_t *)len8_w;
    uint32_t *seg_exit = rank_pre;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t b = blockIdx.x;
    BlockMeta *meta = meta_all + b;
    SubMeta *sub = sub_all + (uint64_t)b * cfg.max_sub;
    HcState *st = hc_all + b;
    const uint32_t n = meta->n;
    if (n <= cfg.passthrough || st->done) return;  // uniform
    const uint8_t *in = slab + (uint64_t)b * cfg.block_size;
    const uint16_t *val = val_all + (uint64_t)b * cfg.stride;
    const unsigned long long *mbits_g = (const unsigned long long *)(mbits_all + (uint64_t)b * (cfg.stride / 32));
    uint32_t *tok = tok_all + (uint64_t)b * cfg.stride;

    // A "round" parses from HcState.resume_pos with HcState.min_len until the block ends or a new
    // sub-block needs another minimum match length; the block then parses on from there in its next
    // round.  LOOP = false: one round per launch (the state is saved, the kernel returns).  LOOP = true:
    // the rounds are a loop of THIS workgroup (blocks owe each other nothing) until the block is done.
    // The host enqueues two single rounds and one looping launch and reads nothing back: nearly every
    // block is done after one round, the looping form -- which costs this kernel 20 more spilled VGPRs --
    // only ever sees the few that need a third.
    const unsigned long long lane_below = (1ull << lane) - 1ull;
#ifdef GZPX_EXPERIMENT
    // measurement builds (tools/exp_parse_hc.py): cycles per phase, summed over the blocks of a launch (thread 0's
    // clock): 0 stage, 1 min_len filter, 2 first walk, 3 walk rounds, 4 scan, 5 boundaries + checks, 6 token pass, 7 rounds
    unsigned long long exp_t = __builtin_readcyclecounter();
    auto exp_lap = [&](uint32_t slot) {
        const unsigned long long t = __builtin_readcyclecounter();
        if (tid == 0) atomicAdd(&g_exp_cycles[(b & 1023u) * 8u + slot], t - exp_t);
        exp_t = t;
    };
#else
    auto exp_lap = [](uint32_t) {};
#endif
    for (;;) {
    // state (uniform across the workgroup; in the looping form written by thread 0 a round ago)
    auto ld = [](const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    uint32_t entry_carry = ld(&st->resume_pos);
    uint32_t tok_carry = ld(&st->tok_carry), mat_carry = ld(&st->mat_carry);
    uint32_t cur_sub = ld(&st->cur_sub);
    const uint32_t orphan_at = ld(&st->pad);  // position + 1 of the block's orphan match (k_match_hc), 0 = none
    uint32_t sub_start = entry_carry, sub_start_tok = tok_carry, sub_start_mat = mat_carry;
    uint32_t sub_limit = max_block_end(sub_start, n, kSoftMaxBlockLen);
    uint32_t min_len = ld(&st->min_len);
    if (LOOP) __syncthreads();  // the previous round is done with the LDS state
    if (min_len == 0) {  // first round: the sub-block that starts the block (calculate_min_match_len)
        min_len = hc_calc_min_len(cfg, in, 0, n, used, tid, kMpThreads);
        __syncthreads();
        if (tid == 0) st->min_len = min_len;
    }
    if (tid == 0) {
        s_next_check = kNoCheckYet;
        for (int k = 0; k < 10; k++) {
            s_obs[k] = 0;
            s_new[k] = 0;
        }
    }

    for (uint32_t tile_begin = entry_carry / kHpTile * kHpTile; tile_begin < n; tile_begin += kHpTile) {
        const uint32_t tile_len = n - tile_begin < kHpTile ? n - tile_begin : kHpTile;
        const uint32_t ngroups = (tile_len + 63) / 64;
        __syncthreads();
        {
            const uint32_t *src = (const uint32_t *)(len8_all + (uint64_t)b * cfg.stride + tile_begin);
            for (uint32_t i = tid; i < (tile_len + 3) / 4; i += kMpThreads) len8_w[i] = src[i];
        }
        __syncthreads();
        exp_lap(0);
        if (tid < kHpGroups) {
            // k_match_hc's matches are those of min_len 3: keep the long enough ones.  (The bitmap
            // word of the tile's last group may carry bits of positions >= n: dropped.)
            unsigned long long w = tid < ngroups ? mbits_g[tile_begin / 64 + tid] : 0ull;
            const uint32_t left = tile_len - (tid < ngroups ? tid * 64 : tile_len);
            if (left < 64) w &= (1ull << left) - 1ull;
            mraw[tid] = w;
            if (min_len > 3 && !GZPX_EXP(cfg, 13)) {
                unsigned long long t = w, keep = 0;
                while (t) {
                    const uint32_t bit = (uint32_t)__ffsll((long long)t) - 1;
                    t &= t - 1;
                    if ((uint32_t)len8[tid * 64 + bit] + 3u >= min_len) keep |= 1ull << bit;
                }
                w = keep;
            }
            // the orphan match exists only for a search that starts at best_len >= 4 (min_len >= 5): below that
            // its position is a literal, like a match that is too short (the byte comes from the input, see the token pass)
            if (min_len <= 4 && orphan_at - 1u - tile_begin - tid * 64u < 64u)
                w &= ~(1ull << ((orphan_at - 1u - tile_begin) & 63u));
            mb[tid] = w;
            tok_bits[tid] = 0;
        }
        __syncthreads();
        exp_lap(1);

        // ---- greedy parse: speculative segment walk, as in k_parse: thread s owns the 64 positions of
        // segment s and walks them from an entry (first guess: its own start; thread 0 knows the
        // tile's true entry), then from the exit of segment s-1, until no entry changes.  The marks of
        // a walk are one 64-bit word; a segment's "match here" bits sit in a register, so a run of
        // literals is one mask operation and a hop costs one LDS byte read (the match length).
        const uint32_t n_seg = ngroups;
        auto walk_seg = [&](uint32_t sg, uint32_t pos) -> uint32_t {
            const uint32_t sb = sg * kPSeg, se = sb + kPSeg < tile_len ? sb + kPSeg : tile_len;
            const unsigned long long mbm = mb[sg];
            const unsigned long long in_seg = se - sb >= 64u ? ~0ull : (1ull << (se - sb)) - 1ull;
            unsigned long long marks = 0;
            while (pos < se) {
                const uint32_t rel = pos - sb;
                const unsigned long long rest = mbm >> rel;
                if (rest == 0) {  // literals to the end of the segment
                    marks |= ~0ull << rel;
                    pos = se;
                    break;
                }
                const uint32_t k = (uint32_t)__ffsll((long long)rest) - 1;  // literals rel .. rel+k-1, a match at rel+k
                marks |= (((1ull << k) - 1ull) | (1ull << k)) << rel;
                pos = sb + rel + k + (uint32_t)len8[sb + rel + k] + 3u;
            }
            marks &= in_seg;
            tok_bits[sg] = marks;
            return pos;
        };
        const bool active = tid < n_seg;
        const uint32_t seg_begin = tid * kPSeg;
        uint32_t entry = tid == 0 ? entry_carry - tile_begin : seg_begin;
        if (active) seg_exit[tid] = walk_seg(tid, entry);
        exp_lap(2);
        for (uint32_t round = 0;; round++) {
#ifdef GZPX_EXPERIMENT
            if (tid == 0) atomicAdd(&g_exp_cycles[(b & 1023u) * 8u + 7u], 1ull);
#endif
            __syncthreads();
            bool changed = false;
            uint32_t new_entry = entry;
            if (active && tid > 0) {
                new_entry = seg_exit[tid - 1];
                changed = new_entry != entry;
            }
            if (round >= 24) {
                // slow convergence (long runs shift the phase of the segments behind them one segment
                // per round): one thread parses on from the first inconsistent segment for a while
                if (tid == 0) rescue[0] = 0xFFFFFFFFu;
                __syncthreads();
                if (changed) atomicMin(&rescue[0], tid);
                __syncthreads();
                const uint32_t s_first = rescue[0];
                if (s_first == 0xFFFFFFFFu) break;  // nothing changed: converged
                if (tid == 0) {
                    uint32_t sg = s_first, pos = seg_exit[s_first - 1];
                    for (uint32_t budget = 0; sg < n_seg && budget < 64; sg++, budget++) {
                        pos = walk_seg(sg, pos);
                        seg_exit[sg] = pos;
                    }
                    rescue[1] = sg;  // segments [s_first, sg) are consistent with their entries now
                }
                __syncthreads();
                const uint32_t s_end = rescue[1];
                if (tid >= s_first && tid < s_end) {
                    entry = seg_exit[tid - 1];
                } else if (changed && tid > s_end) {  // the others keep correcting themselves in parallel
                    entry = new_entry;
                    seg_exit[tid] = walk_seg(tid, entry);
                }
                continue;
            }
            __syncthreads();
            if (changed) {
                entry = new_entry;
                seg_exit[tid] = walk_seg(tid, entry);
            }
            if (!__syncthreads_or(changed)) break;
        }
        const uint32_t exit_rel = uniform(seg_exit[n_seg - 1]);
        __syncthreads();  // seg_exit is rank_pre from here on
        exp_lap(3);

        // ---- tokens / matches per 64-position group (one thread each, from the two bitmaps), then
        // one workgroup-wide scan
        const unsigned long long my_tok = tid < kHpGroups ? tok_bits[tid] : 0ull;
        const unsigned long long my_mat = tid < kHpGroups ? my_tok & mb[tid] : 0ull;
        uint32_t tile_tok, tile_mat, my_pre;
        {
            const uint32_t vt = (uint32_t)__popcll(my_tok), vm = (uint32_t)__popcll(my_mat);
            const uint32_t it = wave_inclusive_scan(vt, lane), im = wave_inclusive_scan(vm, lane);
            if (lane == 63) {
                wsum_t[wave] = it;
                wsum_m[wave] = im;
            }
            __syncthreads();
            uint32_t bt = 0, bm = 0, tt = 0, tm = 0;
            for (uint32_t w = 0; w < kMpWaves; w++) {
                const uint32_t st_ = wsum_t[w], sm_ = wsum_m[w];
                if (w < wave) {
                    bt += st_;
                    bm += sm_;
                }
                tt += st_;
                tm += sm_;
            }
            tile_tok = uniform(tt);
            tile_mat = uniform(tm);
            my_pre = (bt + it - vt) | ((bm + im - vm) << 17);  // tokens <= 49152 < 2^17, matches <= 16384 < 2^15
            if (tid < kHpGroups) rank_pre[tid] = my_pre;
        }
        __syncthreads();
        exp_lap(4);

        // ---- per sub-block that starts or continues in this tile: where it ends, its tokens
        bool build = true;
        uint32_t stat_from = sub_start_tok > tok_carry ? sub_start_tok : tok_carry;  // first token not yet tallied
        for (;;) {
            if (tid == 0) {
                bnd = ~0ull;
                first_check = 0xFFFFFFFFu;
                split_pos = 0xFFFFFFFFu;
            }
            for (uint32_t i = tid; i < kHpMaxBins * 10; i += kMpThreads) (&bins[0][0])[i] = 0;
            __syncthreads();
            // (1) one thread per group, from the bitmaps and prefixes: the first token behind the soft
            // limit or the 50000th match (both monotone along the token stream), and -- until the
            // sub-block has had its first should_end_block check -- the first token with 511 tokens
            // before it whose end lies 5000 bytes into the sub-block
            if (tid < ngroups && my_tok) {
                const uint32_t gb = tile_begin + tid * 64;
                const uint32_t pt = tok_carry + (my_pre & 0x1FFFFu), pm = mat_carry + (my_pre >> 17);
                unsigned long long cand = 0;
                const uint32_t lo = sub_limit > sub_start + 1 ? sub_limit : sub_start + 1;
                if (gb + 64 > lo) cand = lo > gb ? my_tok & (~0ull << (lo - gb)) : my_tok;
                const uint32_t T = sub_start_mat + kSeqStoreLen;
                if (pm >= T) {
                    if (gb > sub_start) cand |= my_tok;
                    else if (gb + 63 > sub_start) cand |= my_tok & (~0ull << (sub_start + 1 - gb));
                } else if (pm + (uint32_t)__popcll(my_mat) >= T) {
                    cand |= my_tok & mask_after_kth(my_mat, T - pm);
                }
                if (cand) {
                    const uint32_t bit = (uint32_t)__ffsll((long long)cand) - 1;
                    const uint32_t ti = pt + (uint32_t)__popcll(my_tok & ((1ull << bit) - 1ull));
                    atomicMin(&bnd, ((unsigned long long)(gb + bit) << 32) | ti);
                }
                if (s_next_check == kNoCheckYet) {
                    const uint32_t A0 = sub_start_tok + kObsPerCheck - 1u, B0 = sub_start + kMinBlockLen;  // (split_due, taken apart)
                    const uint32_t cnt = (uint32_t)__popcll(my_tok);
                    if (pt + cnt > A0 && gb + 64 + 258 > B0) {
                        unsigned long long ca = my_tok;
                        if (A0 > pt) {
                            for (uint32_t i = 0; i < A0 - pt; i++) ca &= ca - 1;  // tokens with fewer than 511 before them
                        }
                        uint32_t found = 0xFFFFFFFFu;
                        while (ca) {
                            const uint32_t bit = (uint32_t)__ffsll((long long)ca) - 1;
                            ca &= ca - 1;
                            const uint32_t len = ((my_mat >> bit) & 1ull) ? (uint32_t)len8[tid * 64 + bit] + 3u : 1u;
                            if (gb + bit + len >= B0) {
                                found = bit;
                                break;
                            }
                        }
                        if (found != 0xFFFFFFFFu)
                            atomicMin(&first_check, pt + (uint32_t)__popcll(my_tok & ((1ull << found) - 1ull)));
                    }
                }
            }
            __syncthreads();
            const unsigned long long bv = bnd;
            const uint32_t lim_tok = bv == ~0ull ? 0xFFFFFFFFu : (uint32_t)bv;  // tokens from here are in the next sub-block
            if (tid == 0 && s_next_check == kNoCheckYet && first_check != 0xFFFFFFFFu) s_next_check = first_check;
            __syncthreads();
            const uint32_t nc = s_next_check;  // token index of the first check from here, or a sentinel
            exp_lap(5);
            // (2) one pass in position order, a wave per group: lane l takes position l (coalesced val
            // reads and token stores), ranks from the group's prefix + popcounts below the lane.  Builds
            // the tokens (first time through) and tallies the observation classes per 512-token bin
            // (bin 0 = up to and including the first check token).
            for (uint32_t g0 = wave; g0 < ngroups; g0 += 8 * kMpWaves) {
                uint32_t vals[8], tis[8];
                // (min_len > 3: a match k_match_hc found that is too short for this sub-block is a literal, and `val` holds
                // its distance, not its byte.  Which positions those are is in LDS (mraw), and the bytes are requested HERE,
                // beside the val loads: asked for where they are needed -- the bitmap word, then the byte -- they were two
                // dependent trips to memory per group, sixteen per turn of this loop, and half of the kernel's time on text)
                uint32_t inb[8];
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) {
                    const uint32_t g = g0 + k * kMpWaves;
                    const uint32_t r = g * 64 + lane;
                    const bool in_tile = g < ngroups && r < tile_len;
                    vals[k] = in_tile ? val[tile_begin + r] : 0u;
                    inb[k] = ((min_len > 3 || orphan_at != 0) && in_tile) ? (uint32_t)in[tile_begin + r] : 0u;
                }
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): no load is pending behind a later store's data
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) {
                    const uint32_t g = g0 + k * kMpWaves;
                    tis[k] = 0xFFFFFFFFu;
                    if (g >= ngroups) continue;  // wave-uniform
                    const unsigned long long mt = tok_bits[g], mm = mt & mb[g];
                    const uint32_t r = g * 64 + lane, p = tile_begin + r;
                    if (!((mt >> lane) & 1ull)) continue;
                    const bool is_match = (mm >> lane) & 1ull;
                    const uint32_t ti = tok_carry + (rank_pre[g] & 0x1FFFFu) + (uint32_t)__popcll(mt & lane_below);
                    const uint32_t len = is_match ? (uint32_t)len8[r] + 3u : 1u;
                    uint32_t v = vals[k];
                    // a match too short for this sub-block's min_len is a literal: val holds its distance
                    if (!is_match && ((mraw[g] >> lane) & 1ull)) v = inb[k];
                    vals[k] = is_match ? (kTokMatch | ((v & 0x7FFFu) << 9) | len) : v;  // (without k_match_hc's orphan mark)
                    tis[k] = ti;
                    if (ti < stat_from || ti >= lim_tok || GZPX_EXP(cfg, 14)) continue;
                    const uint32_t cls = is_match ? obs_match(len) : obs_literal(v);
                    uint32_t bin = 0;
                    if (nc < kNoMoreChecks && ti > nc) bin = 1u + (ti - nc - 1u) / 512u;
                    // (one count per class, bin and wave from ten ballots instead of an LDS atomic per token
                    // was measured: slower, 101 -> 120 ms on configs[2])
                    if (bin < kHpMaxBins) atomicAdd(&bins[bin][cls], 1u);
                    if (nc < kNoMoreChecks && ti >= nc && (ti - nc) % 512u == 0 && (ti - nc) / 512u < kHpMaxBins)
                        chk_end[(ti - nc) / 512u] = p + len;
                }
                if (build && !GZPX_EXP(cfg, 15)) {
#pragma unroll
                    for (uint32_t k = 0; k < 8; k++)
                        if (tis[k] != 0xFFFFFFFFu) tok[tis[k]] = vals[k];
                }
            }
            __syncthreads();
            exp_lap(6);
            // The checks themselves.  do_end_block_check for check k needs the observations merged so
            // far (everything before bin k) and the new ones (bin k): both follow from prefix sums over
            // the bins as long as no earlier check ended the block -- and the first one that does ends
            // the evaluation anyway -- so all checks of the tile are evaluated side by side (one thread
            // each) instead of as a 100-step recurrence on one thread.
            const uint32_t last_tok = (lim_tok < tok_carry + tile_tok ? lim_tok : tok_carry + tile_tok);  // exclusive
            const uint32_t nck0 = s_next_check;
            uint32_t n_checks = 0;
            if (nck0 < kNoMoreChecks && nck0 < last_tok) {
                n_checks = (last_tok - 1 - nck0) / 512u + 1u;
                if (n_checks > kHpMaxBins) n_checks = kHpMaxBins;
            }
            if (tid < 10) {  // exclusive prefix of every class over the bins
                uint32_t acc = 0;
                for (uint32_t k = 0; k <= n_checks; k++) {  // (n_checks <= kHpMaxBins)
                    cum[k][tid] = acc;
                    if (k < kHpMaxBins) acc += bins[k][tid];
                }
            }
            if (tid == 0) first_evt = 0xFFFFFFFFu;
            __syncthreads();
            if (tid < n_checks) {
                const uint32_t k = tid;
                uint32_t num_obs = 0, num_new = 0, total_delta = 0;
                uint32_t obs[10], nw[10];
                for (int c = 0; c < 10; c++) {
                    obs[c] = s_obs[c] + (k > 0 ? s_new[c] : 0u) + cum[k][c];
                    nw[c] = bins[k][c] + (k == 0 ? s_new[c] : 0u);
                    num_obs += obs[c];
                    num_new += nw[c];
                }
                const uint32_t e = chk_end[k];
                const uint32_t blen = e - sub_start;
                bool evt = n - e < kMinBlockLen;  // in_end - in_next < MIN_BLOCK_LENGTH: never again
                if (!evt && num_obs > 0) {
                    for (int c = 0; c < 10; c++) total_delta += split_delta(obs[c], nw[c], num_obs, num_new);
                    evt = split_verdict(total_delta, num_obs, num_new, blen);
                }
                if (evt) atomicMin(&first_evt, k);
            }
            __syncthreads();
            if (tid == 0) {
                const uint32_t fe = first_evt;
                if (fe != 0xFFFFFFFFu && n - chk_end[fe] >= kMinBlockLen) {  // check fe ends the sub-block
                    split_pos = chk_end[fe];
                    bnd_tok = nck0 + 512u * fe + 1;
                    s_next_check = nck0 + 512u * fe;
                } else {
                    // no split in this tile: the state after the last check (or at the point where
                    // checks stop for good -- what is carried then is never looked at again)
                    const uint32_t kk = fe != 0xFFFFFFFFu ? fe : n_checks;  // bins [0, kk) are merged
                    for (int c = 0; c < 10; c++) {
                        const uint32_t o = s_obs[c] + (kk > 0 ? s_new[c] : 0u) + cum[kk][c];
                        const uint32_t w = (kk < kHpMaxBins ? bins[kk][c] : 0u) + (kk == 0 ? s_new[c] : 0u);
                        s_obs[c] = o;
                        s_new[c] = w;
                    }
                    s_next_check = fe != 0xFFFFFFFFu ? kNoMoreChecks : (nck0 < kNoMoreChecks ? nck0 + 512u * n_checks : nck0);
                }
            }
            __syncthreads();
            // which boundary, if any, ends the sub-block inside this tile
            uint32_t bp = 0xFFFFFFFFu, bti = 0;
            if (split_pos != 0xFFFFFFFFu) {
                bp = split_pos;
                bti = bnd_tok;
            } else if (bv != ~0ull) {
                bp = (uint32_t)(bv >> 32);
                bti = (uint32_t)bv;
            }
            if (bp == 0xFFFFFFFFu) break;  // the sub-block continues in the next tile
            if (tid == 0) {  // matches before the boundary token
                if (bp >= tile_begin + tile_len) {
                    bnd_mat = mat_carry + tile_mat;  // it starts in the next tile
                } else {
                    const uint32_t r = bp - tile_begin, g = r >> 6;
                    const unsigned long long mm = tok_bits[g] & mb[g];
                    bnd_mat = mat_carry + (rank_pre[g] >> 17) + (uint32_t)__popcll(mm & ((1ull << (r & 63u)) - 1ull));
                }
                sub[cur_sub].tok_begin = sub_start_tok;
                sub[cur_sub].tok_end = bti;
                sub[cur_sub].byte_begin = sub_start;
                sub[cur_sub].byte_len = bp - sub_start;
                sub[cur_sub].is_final = 0;
                s_next_check = kNoCheckYet;
                for (int k = 0; k < 10; k++) {
                    s_obs[k] = 0;
                    s_new[k] = 0;
                }
            }
            __syncthreads();
            const uint32_t bm = bnd_mat;
            cur_sub++;
            sub_start = bp;
            sub_start_tok = bti;
            sub_start_mat = bm;
            sub_limit = max_block_end(bp, n, kSoftMaxBlockLen);
            stat_from = bti;
            const uint32_t new_min_len = hc_calc_min_len(cfg, in, bp, n, used, tid, kMpThreads);
            __syncthreads();
            if (new_min_len != min_len) {
                // the "long enough" filter of the matches from bp on was another sub-block's: parse
                // again from there (k_match_hc's results stand, they do not depend on min_len)
                if (tid == 0) {
                    // (round 5) arrays that hold the full search for ONE min_len's token starts only are no use from
                    // here on: the dense k_match_hc goes over the block from bp before the next round parses it
                    // (`stale`: their list for k_match_hc_stale -- count, then block indices; Scratch.redo, idle at these levels)
                    if (st->sparse == kHcArraysPath) {
                        // (k_match_hc_stale runs once, behind the FIRST round: a round can only end at `done` or here, so no
                        // block is still kHcArraysPath after it.  Should that ever stop being true, a block listed later would
                        // be parsed over first-node matches -- a valid stream that is not libdeflate's: stop loudly instead.)
                        if (!may_list_stale) __builtin_trap();
                        st->sparse = kHcArraysStale;
                        stale[1u + atomicAdd(&stale[0], 1u)] = b;
                    }
                    st->min_len = new_min_len;
                    st->resume_pos = bp;
                    st->tok_carry = bti;
                    st->mat_carry = bm;
                    st->cur_sub = cur_sub;
                    st->rounds++;
                    if (LOOP) __threadfence();
                }
                if (!LOOP) return;
                __syncthreads();
                goto next_round;
            }
            build = false;
        }
        tok_carry += tile_tok;
        mat_carry += tile_mat;
        entry_carry = tile_begin + exit_rel;
        exp_lap(5);
    }
    if (tid == 0) {
        sub[cur_sub].tok_begin = sub_start_tok;
        sub[cur_sub].tok_end = tok_carry;
        sub[cur_sub].byte_begin = sub_start;
        sub[cur_sub].byte_len = n - sub_start;
        sub[cur_sub].is_final = 1;
        meta->ntok = tok_carry;
        meta->nsub = cur_sub + 1;
        st->done = 1;
    }
    return;
next_round:;
    }
}

// ------------------------------------------------------------------------------------------
// k_parse_lazy: deflate_compress_lazy_generic (levels 5-7 lazy, 8-9 lazy2) over the matches
// k_match_hc found; one wave per block.
//   A decision that starts at p:  cur = M0[p]; literal unless len >= min_len and not (len 3,
//   offset > 8192); then, while cur is shorter than nice_len: next = M1[cur_pos+1] if at least as long
//   as cur, taken (cur_pos becomes a literal) when 4*(next_len-cur_len) + bsr(cur_off) -
//   bsr(next_off) > 2; lazy2 also tries M2[cur_pos+2] against > 6 (two literals).
// Whether p starts a decision depends on every choice before it, but WHAT a decision started at
// p does depends only on p and min_len.  So for a window of 64 positions every lane works out
// "the decision if one starts here" (literal count, match, where the next one starts); the
// positions where decisions really start are then a pointer chase through 64 registers
// (v_readlane), and their lanes write tokens at wave-prefix offsets and tally observations with
// LDS atomics.  What cuts a window short is checked per reached decision from the same prefixes:
// the sub-block ends (soft limit, 50000 sequences), should_end_block is due (512 new
// observations, 5000 bytes either side) or min_len is due for recalculate_min_match_len.
//   A decision's chain looks at most kLzReach positions ahead: each step raises 4*len - bsr(off),
//   which lives in [-2, 1032], by >= 3 per position it advances, so <= 345 positions and 2 of
//   lookahead.  Nearly every chain is a step or two, so a window starts wherever kLzNear positions of the
//   LDS tile are left behind it; a lane whose chain runs off the tile says so, and if the walk reaches
//   that lane the window is cut in front of it and the tile reloaded there (a tile that starts at a window
//   holds the longest chain of every lane: kLzSpan >= 64 + kLzReach + 3).
// ------------------------------------------------------------------------------------------
#ifndef GZPX_LZ_SPAN
#define GZPX_LZ_SPAN 512
#endif
constexpr uint32_t kLzSpan = GZPX_LZ_SPAN;  // positions per LDS tile
constexpr uint32_t kLzReach = 352;
constexpr uint32_t kLzNear = 16;
constexpr uint32_t kLzStep = kLzSpan - 64 - kLzNear;           // the grid of tile starts
constexpr uint32_t kLzInRegs = (kLzSpan / 4 + 2 + 63) / 64;  // dwords of input bytes per lane and tile
static_assert(kLzSpan >= 64 + kLzReach + 4 && kLzSpan % 256 == 0, "a tile holds a window and its longest chain");

template <int NV>  // match variants staged: 2 (lazy) or 3 (lazy2)
struct LzLds {
    uint32_t in8[kLzSpan / 4 + 2];
    uint32_t len[NV][kLzSpan / 4];
    uint32_t dist[NV][kLzSpan / 2];
    uint32_t freq[256];  // literal frequencies of the current sub-block
    uint32_t used[8];
    uint32_t obs[10], nw[10];
};

template <int NV>
__global__ __launch_bounds__(64) void k_parse_lazy(Config cfg, const uint8_t *__restrict__ slab,
                                                   BlockMeta *__restrict__ meta_all,
                                                   SubMeta *__restrict__ sub_all,
                                                   const uint8_t *__restrict__ len0_all,
                                                   const uint16_t *__restrict__ dist0_all,
                                                   const uint8_t *__restrict__ lz_len_all,
                                                   const uint16_t *__restrict__ lz_dist_all,
                                                   uint32_t *__restrict__ tok_all) {
    __shared__ LzLds<NV> L;
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    BlockMeta *meta = meta_all + b;
    const uint32_t n = meta->n;
    if (n <= cfg.passthrough) return;  // uniform
    SubMeta *sub = sub_all + (uint64_t)b * cfg.max_sub;
    const uint8_t *in = slab + (uint64_t)b * cfg.block_size;
    uint32_t *tok = tok_all + (uint64_t)b * cfg.stride;
    const uint8_t *gl[3] = {len0_all + (uint64_t)b * cfg.stride, lz_len_all + (uint64_t)b * 2u * cfg.stride,
                            lz_len_all + ((uint64_t)b * 2u + 1u) * cfg.stride};
    const uint16_t *gd[3] = {dist0_all + (uint64_t)b * cfg.stride, lz_dist_all + (uint64_t)b * 2u * cfg.stride,
                             lz_dist_all + ((uint64_t)b * 2u + 1u) * cfg.stride};
    constexpr bool lazy2 = NV == 3;
    const uint32_t nice_level = cfg.hc_nice;
    const uint8_t *t_l0 = (const uint8_t *)L.len[0], *t_l1 = (const uint8_t *)L.len[1], *t_l2 = (const uint8_t *)L.len[NV - 1];
    const uint16_t *t_d0 = (const uint16_t *)L.dist[0], *t_d1 = (const uint16_t *)L.dist[1],
                   *t_d2 = (const uint16_t *)L.dist[NV - 1];
    const uint64_t lane_below = (1ull << lane) - 1ull;

    uint32_t pos = 0, ti = 0, cur_sub = 0;
    uint32_t t0 = 0xFFFFFFFFu;  // the tile holds positions [t0, t0 + kLzSpan)
    const uint32_t mis = (uint32_t)((uintptr_t)in & 3u);  // (tiles start at multiples of four)
    // Tiles lie on a grid of kLzStep positions (a tile serves the windows that start in its first kLzStep), so the one
    // behind the current tile is known when the current one is stored to LDS: its loads are issued then, into
    // registers, and waited for a tile later.  (Round 4: loaded on demand, a tile cost the wave 16 thousand clocks
    // -- 139 times per BGZF block, a third of the kernel.)
    uint32_t pf0 = 0xFFFFFFFFu;  // start of the tile in the registers
    bool here = false;           // the next tile starts at pos, off the grid
    uint32_t pf_in[kLzInRegs], pf_len[NV][kLzSpan / 256], pf_dist[NV][kLzSpan / 128];
    auto tile_fetch = [&](uint32_t start) {
        const uint32_t t_end = start + kLzSpan < n ? start + kLzSpan : n;  // (exclusive)
        const uint32_t *src = (const uint32_t *)(in + start - mis);
        const uint32_t ndw = (mis + (t_end - start) + 3u) >> 2;
        const uint32_t nd4 = (t_end - start + 3u) / 4u, nd2 = (t_end - start + 1u) / 2u;
#pragma unroll
        for (uint32_t k = 0; k < kLzInRegs; k++) pf_in[k] = lane + 64u * k < ndw ? src[lane + 64u * k] : 0u;
#pragma unroll
        for (int v = 0; v < NV; v++) {
            const uint32_t *sl = (const uint32_t *)gl[v] + start / 4u;
            const uint32_t *sd = (const uint32_t *)gd[v] + start / 2u;
#pragma unroll
            for (uint32_t k = 0; k < kLzSpan / 256; k++) pf_len[v][k] = lane + 64u * k < nd4 ? sl[lane + 64u * k] : 0u;
#pragma unroll
            for (uint32_t k = 0; k < kLzSpan / 128; k++) pf_dist[v][k] = lane + 64u * k < nd2 ? sd[lane + 64u * k] : 0u;
        }
        pf0 = start;
    };
#ifdef GZPX_EXPERIMENT
    // measurement builds (tools/exp_parse_lazy.py): the wave's clock per phase, summed over a block's windows: 0 tile
    // loads, 1 decisions, 2 chase, 3 prefixes + what is due, 4 commit, 5 what was due; 6 windows, 7 tile loads
    unsigned long long exp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long exp_t = __builtin_readcyclecounter();
    auto exp_lap = [&](uint32_t slot) {
        const unsigned long long t = __builtin_readcyclecounter();
        exp_acc[slot] += t - exp_t;
        exp_t = t;
    };
    auto exp_count = [&](uint32_t slot) { exp_acc[slot] += 1; };
#else
    auto exp_lap = [](uint32_t) {};
    auto exp_count = [](uint32_t) {};
#endif
    for (;;) {                            // DEFLATE sub-blocks
        const uint32_t sub_start = pos, sub_start_tok = ti;
        const uint32_t block_end = max_block_end(sub_start, n, kSoftMaxBlockLen);
        uint32_t min_len = hc_calc_min_len(cfg, in, sub_start, n, L.used, lane, 64);
        // (split_due and the two recalculation points below in this kernel's own text: gzpx_policy.h says why)
        uint32_t next_recalc = sub_start + (n - sub_start < kFirstRecalc ? n - sub_start : kFirstRecalc);
        uint32_t nseq = 0, num_new = 0, num_obs = 0;
        __syncthreads();
        for (uint32_t i = lane; i < 256; i += 64) L.freq[i] = 0;
        if (lane < 10) {
            L.obs[lane] = 0;
            L.nw[lane] = 0;
        }
        for (;;) {  // windows of 64 positions from pos
            exp_lap(5);
            if (t0 == 0xFFFFFFFFu || pos - t0 + 64u + kLzNear > kLzSpan) {
                // the tile of the grid that serves a window at pos -- or, when a chain ran off its tile, the one that starts here
                const uint32_t start = here ? (pos & ~3u) : pos / kLzStep * kLzStep;
                here = false;
                if (pf0 != start) tile_fetch(start);  // (a block's first tile, or one out of turn)
                __syncthreads();
#pragma unroll
                for (uint32_t k = 0; k < kLzInRegs; k++)
                    if (lane + 64u * k < kLzSpan / 4 + 2) L.in8[lane + 64u * k] = pf_in[k];
#pragma unroll
                for (int v = 0; v < NV; v++) {
#pragma unroll
                    for (uint32_t k = 0; k < kLzSpan / 256; k++) L.len[v][lane + 64u * k] = pf_len[v][k];
#pragma unroll
                    for (uint32_t k = 0; k < kLzSpan / 128; k++) L.dist[v][lane + 64u * k] = pf_dist[v][k];
                }
                __syncthreads();
                t0 = start;
                // the next tile of the grid travels in registers while this one is parsed
                pf0 = (start / kLzStep + 1u) * kLzStep;
                if (pf0 < n) tile_fetch(pf0);
                else pf0 = 0xFFFFFFFFu;
                exp_count(7);
            }
            exp_lap(0);
            exp_count(6);
            const uint8_t *t_in = (const uint8_t *)L.in8 + mis;
            // ---- the decision a lane's position would start
            const uint32_t p = pos + lane, r = p - t0;
            uint32_t nlit = 0, mlen = 0, moff = 0, nrel = lane + 1u;
            bool off_tile = false;  // the chain needs positions behind the tile
            if (p < n) {
                uint32_t d = t_d0[r];
                const uint32_t l = (uint32_t)t_l0[r] + 3u;
                // (k_match_hc's orphan mark: a match that only a search started at best_len >= 4 finds)
                if (d & kHcOrphan) d = min_len >= 5u ? d & 0x7FFFu : 0u;
                if (d == 0 || l < min_len || (l == 3u && d > 8192u)) {
                    nlit = 1;
                } else {
                    uint32_t cp = p, cl = l, co = d;
                    for (;;) {  // have_cur_match
                        const uint32_t rem = n - cp;
                        const uint32_t max_len = rem < 258u ? rem : 258u;
                        const uint32_t nice_len = max_len < nice_level ? max_len : nice_level;
                        if (cl >= nice_len) break;  // take it as it is
                        const uint32_t rr = cp + 1u - t0;
                        if (rr + 1u >= kLzSpan) {
                            off_tile = true;
                            break;
                        }
                        const int bsr_cur = 31 - __clz((int)co);
                        {
                            uint32_t d1 = t_d1[rr];
                            const uint32_t l1 = (uint32_t)t_l1[rr] + 3u;
                            if (d1 & kHcOrphan) d1 = cl >= 5u ? d1 & 0x7FFFu : 0u;  // (the lookahead starts at cur_len - 1)
                            if (d1 != 0 && l1 >= cl && 4 * (int)(l1 - cl) + (bsr_cur - (31 - __clz((int)d1))) > 2) {
                                nlit += 1u;
                                cp += 1u;
                                cl = l1;
                                co = d1;
                                continue;
                            }
                        }
                        if (lazy2) {
                            uint32_t d2 = t_d2[rr + 1u];
                            const uint32_t l2 = (uint32_t)t_l2[rr + 1u] + 3u;
                            if (d2 & kHcOrphan) d2 = cl >= 5u ? d2 & 0x7FFFu : 0u;
                            if (d2 != 0 && l2 >= cl && 4 * (int)(l2 - cl) + (bsr_cur - (31 - __clz((int)d2))) > 6) {
                                nlit += 2u;
                                cp += 2u;
                                cl = l2;
                                co = d2;
                                continue;
                            }
                        }
                        break;
                    }
                    mlen = cl;
                    moff = co;
                    nrel = cp + cl - pos;
                }
                if (mlen == 0) nrel = lane + 1u;
            }
            exp_lap(1);
            // ---- where decisions really start: chase from the window's first position
            // (Round 4, tried: every lane learns its second, third and fourth successor with two rounds of ds_bpermute
            // and the chase takes four decisions a step -- the dependent v_readlane chain shrinks from 17 hops to 5, the
            // kernel grows from 4.33 to 4.8 ms: what it is short of while all its waves are resident is VALU issue.)
            uint64_t reach = 0;
            uint32_t q = 0;
            while (q < 64u) {
                reach |= 1ull << q;
                q = (uint32_t)__builtin_amdgcn_readlane((int)nrel, (int)q);
            }
            const uint32_t exit_rel = q;
            exp_lap(2);
            const bool in_r = (reach >> lane) & 1ull;
            const uint32_t cnt = in_r ? nlit + (mlen ? 1u : 0u) : 0u;
            const uint32_t inc = wave_incl_add(cnt);
            const uint32_t tb = inc - cnt;  // tokens of this window before the lane's decision
            const uint64_t mm = __ballot(in_r && mlen != 0);
            const uint32_t mb = (uint32_t)__popcll(mm & lane_below);
            // ---- the first reached decision in front of which something is due
            const bool due = in_r && (p >= block_end || nseq + mb >= kSeqStoreLen ||
                                      (num_new + tb >= kObsPerCheck && p - sub_start >= kMinBlockLen && n - p >= kMinBlockLen) ||
                                      p >= next_recalc);
            const uint64_t dm_real = __ballot(due);
            const uint64_t dm = dm_real | (__ballot(off_tile) & reach);
            const uint32_t e = dm ? (uint32_t)__ffsll((long long)dm) - 1u : 64u;
            const uint64_t commit = e < 64u ? reach & ((1ull << e) - 1ull) : reach;
            exp_lap(3);
            if ((commit >> lane) & 1ull) {
                const uint32_t o = ti + tb;
                for (uint32_t j = 0; j < nlit; j++) {
                    const uint32_t c = t_in[r + j];
                    tok[o + j] = c;
                    atomicAdd(&L.freq[c], 1u);
                    atomicAdd(&L.nw[obs_literal(c)], 1u);
                }
                if (mlen) {
                    tok[o + nlit] = kTokMatch | (moff << 9) | mlen;
                    atomicAdd(&L.nw[obs_match(mlen)], 1u);
                }
            }
            const uint32_t done_tok = e < 64u ? (uint32_t)__builtin_amdgcn_readlane((int)tb, (int)e)
                                              : (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            ti += done_tok;
            num_new += done_tok;
            nseq += (uint32_t)__popcll(mm & commit);
            pos += e < 64u ? e : exit_rel;
            exp_lap(4);
            if (e == 64u) continue;
            if (!((dm_real >> e) & 1ull)) {  // nothing is due: the decision at pos needs a tile that starts here
                t0 = 0xFFFFFFFFu;
                here = true;
                continue;
            }
            // ---- what is due at pos, in deflate_compress_lazy_generic's order
            if (pos >= block_end || nseq >= kSeqStoreLen) break;
            if (num_new >= kObsPerCheck && pos - sub_start >= kMinBlockLen && n - pos >= kMinBlockLen) {  // do_end_block_check
                __syncthreads();
                const uint32_t o = lane < 10 ? L.obs[lane] : 0u, w = lane < 10 ? L.nw[lane] : 0u;
                const uint32_t total_delta = wave_reduce_add(split_delta(o, w, num_obs, num_new));
                if (split_verdict(total_delta, num_obs, num_new, pos - sub_start)) break;
                if (lane < 10) {
                    L.obs[lane] = o + w;
                    L.nw[lane] = 0;
                }
                num_obs += num_new;
                num_new = 0;
                continue;
            }
            {  // recalculate_min_match_len: literals more frequent than 1/1024 of all of them count as used
                __syncthreads();
                uint32_t f[4], total = 0;
                for (uint32_t k = 0; k < 4; k++) {
                    f[k] = L.freq[lane + 64u * k];
                    total += f[k];
                }
                total = wave_reduce_add(total);
                const uint32_t cutoff = recalc_cutoff(total);
                uint32_t num_used = 0;
                for (uint32_t k = 0; k < 4; k++) num_used += (uint32_t)__popcll(__ballot(f[k] > cutoff));
                min_len = choose_min_match_len(num_used, cfg.hc_depth);
                const uint32_t a = n - next_recalc, bb = pos - sub_start;
                next_recalc += a < bb ? a : bb;
            }
        }
        if (lane == 0) {
            sub[cur_sub].tok_begin = sub_start_tok;
            sub[cur_sub].tok_end = ti;
            sub[cur_sub].byte_begin = sub_start;
            sub[cur_sub].byte_len = pos - sub_start;
            sub[cur_sub].is_final = pos == n ? 1u : 0u;
        }
        cur_sub++;
        if (pos == n) break;
    }
    if (lane == 0) {
        meta->ntok = ti;
        meta->nsub = cur_sub;
    }
#ifdef GZPX_EXPERIMENT
    exp_lap(5);
    if (lane == 0)
        for (uint32_t k = 0; k < 8; k++) atomicAdd(&g_exp_cycles[(b & 1023u) * 8u + k], exp_acc[k]);
#endif
}

__global__ void k_hc_init(uint32_t nb, HcState *hc, uint32_t *pending) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) *pending = 0;
    if (b >= nb) return;
    HcState s;
    s.done = 0;
    s.min_len = 0;
    s.resume_pos = 0;
    s.tok_carry = 0;
    s.mat_carry = 0;
    s.cur_sub = 0;
    s.rounds = 0;
    s.pad = 0;
    s.sparse = kHcArraysNone;
    hc[b] = s;
}

// ------------------------------------------------------------------------------------------
// k_hist: litlen / offset symbol frequencies of every DEFLATE sub-block (deflate_choose_literal /
// deflate_choose_match tallies), from the token stream.  256 threads per block, LDS atomics.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kHistCopies = 8;                 // (a power of two)
constexpr uint32_t kHistPad = kHistStride + 1;      // copies a word apart in the banks
constexpr uint32_t kHistStep = 2048;                // tokens per workgroup step: two 16-byte loads per lane
constexpr uint32_t kHistNoToken = 0x7FFFFFFFu;      // (never a real token: a literal is < 256)
static_assert(kHistStep % 1024 == 0, "whole 16-byte loads per lane");

__global__ __launch_bounds__(256) void k_hist(Config cfg, const BlockMeta *__restrict__ meta_all,
                                              const SubMeta *__restrict__ sub_all,
                                              const uint32_t *__restrict__ tok_all,
                                              uint32_t *__restrict__ hist_all) {
    // Text has a few very hot symbols (the space, 'e', the first offset slots): with one histogram the
    // lanes of an atomic instruction pile up on their words and the LDS applies them one by one (PMC:
    // three quarters of this kernel's LDS cycles were bank conflicts).  Eight copies, picked by the
    // lane, staggered by one bank; summed when the sub-block is written out.
    __shared__ uint32_t hist[kHistCopies * kHistPad];
    __shared__ uint8_t lslot[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const BlockMeta *meta = meta_all + b;
    if (meta->n <= cfg.passthrough) return;
    build_length_table(lslot, tid);
    const SubMeta *sub = sub_all + (uint64_t)b * cfg.max_sub;
    const uint32_t *tok = tok_all + (uint64_t)b * cfg.stride;
    const uint32_t nsub = meta->nsub;
    uint32_t *mine = hist + (tid & (kHistCopies - 1u)) * kHistPad;
    for (uint32_t s = 0; s < nsub; s++) {
        for (uint32_t i = tid; i < kHistCopies * kHistPad; i += 256) hist[i] = 0;
        __syncthreads();
        // A step is kHistStep tokens from an index that is a multiple of 4: two 16-byte loads per lane, issued
        // together.  (Token rows are 16-byte aligned and padded by 2048 entries, so a step that begins inside
        // the sub-block may be loaded whole.)  Whether a step lies inside [t_begin, t_end) is decided once, for
        // the workgroup; only the first and the last step look at each token's index.
        const uint32_t t_begin = sub[s].tok_begin, t_end = sub[s].tok_end;
        for (uint32_t t0 = t_begin & ~3u; t0 < t_end; t0 += kHistStep) {
            uint32_t tk[kHistStep / 256];
#pragma unroll
            for (uint32_t k = 0; k < kHistStep / 1024; k++) {
                const uint4 v = *(const uint4 *)(tok + t0 + 1024u * k + 4u * tid);
                tk[4 * k + 0] = v.x;
                tk[4 * k + 1] = v.y;
                tk[4 * k + 2] = v.z;
                tk[4 * k + 3] = v.w;
            }
            const bool edge = t0 < t_begin || t0 + kHistStep > t_end;
            if (edge) {
#pragma unroll
                for (uint32_t k = 0; k < kHistStep / 256; k++) {
                    const uint32_t i = t0 + 1024u * (k / 4) + 4u * tid + (k & 3u);
                    if (i < t_begin || i >= t_end) tk[k] = kHistNoToken;
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < kHistStep / 256; k++) {
                const uint32_t t = tk[k];
                if (edge && t == kHistNoToken) continue;
                const bool m = (int32_t)t < 0;
                const uint32_t lt = lslot[(t - 3u) & 0xFFu];
                atomicAdd(&mine[m ? 257u + (lt & 31u) : t], 1u);
                if (m) atomicAdd(&mine[kNumLitlen + offset_slot(((t >> 9) & 0xFFFFu) - 1u).slot], 1u);
            }
        }
        __syncthreads();
        uint32_t *out = hist_all + ((uint64_t)b * cfg.max_sub + s) * kHistStride;
        for (uint32_t i = tid; i < kHistStride; i += 256) {
            uint32_t sum = 0;
#pragma unroll
            for (uint32_t c = 0; c < kHistCopies; c++) sum += hist[c * kHistPad + i];
            out[i] = sum;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// k_huffman: deflate_flush_block's decisions for every sub-block of a block, one wave per
// block (sub-blocks in order: the stored-block cost depends on the running bit count).
//   make_code = libdeflate's deflate_make_huffman_code: sort by (freq, symbol), two-queue
//   tree build with leaf preference on ties, depth clamp to max_len, lengths handed out to the
//   sorted symbols, canonical codewords bit-reversed.  Rank sort and codeword assignment are
//   wave-parallel; the two inherently sequential scans (tree build, depth propagation) run on
//   lane 0 out of LDS -- thousands of blocks are in flight, so the chip hides that latency
//   across waves.
// ------------------------------------------------------------------------------------------
struct HuffLds {
    // Arrays whose lifetimes do not overlap share storage, which brings the structure under
    // 6.4 KiB: 25 blocks per CU instead of 16, so a slab's blocks take one round less.
    //   region A: sort keys -> internal node frequencies (tree build) -> header bit string
    //   region B: sorted leaf frequencies; from entry 32 on, the precode items (written when only
    //             the 19-symbol precode is still to be built)
    //   region C: input frequencies (read at the start of make_code); its upper half holds the
    //             internal node parents, which are written later in the same call
    union {
        uint32_t key[kNumLitlen];    // (freq << 10) | sym, or ~0 for unused
        uint32_t nfreq[kNumLitlen];  // internal node frequencies
        uint32_t hdr[kHdrWords];     // dynamic block header bits
    };
    union {
        uint32_t sfreq[kNumLitlen];  // sorted leaf frequencies
        struct {
            uint32_t sfreq_low[32];
            uint16_t items[kNumLitlen + kNumOffset];  // precode items
        };
    };
    union {
        uint32_t freq[kNumLitlen];  // input frequencies of the code being built
        struct {
            uint32_t freq_low[kNumLitlen / 2];
            uint16_t parent[kNumLitlen];  // internal node parents
        };
    };
    uint32_t lcw[kNumLitlen];
    uint16_t ssym[kNumLitlen];  // sorted leaf symbols
    uint8_t depth[kNumLitlen];
    uint8_t lens[kNumLitlen + kNumOffset];  // litlen lens, then (moved adjacent) offset lens
    uint8_t olens[kNumOffset + 2];
    uint8_t plens[32];
    uint32_t ocw[kNumOffset];
    uint32_t pcw[32];
    uint32_t pfreq[32];
    uint32_t len_counts[16];
    uint32_t misc[8];
};
static_assert(sizeof(HuffLds) <= 6400, "HuffLds: 25 workgroups per CU");
static_assert(kHdrWords <= kNumLitlen, "header bits fit region A");


// A lane-distributed array of up to 320 words in five registers: element k (wave-uniform) lives in
// lane k & 63 of r[k >> 6]; reading it is four selects and one v_readlane, no LDS round trip.
// Used by the run-length scan of the code lengths, which runs WAVE-UNIFORM (every lane computes the
// same thing: scalar branches, no exec-mask bookkeeping) with a run's end found by a ballot.
// (The tree build written the same way -- both queues in registers -- was slower, k_huffman 0.55 ->
// 0.66 ms: with six waves per SIMD the kernel is bound by instructions issued, not by the latency of
// lane 0's LDS reads, and the register queues cost more instructions per node.)
__device__ __forceinline__ uint32_t reg5_get(const uint32_t (&r)[5], uint32_t k) {
    // (k is wave-uniform.  Selecting the REGISTER first and reading the lane after it invites the
    // compiler to turn the selects into an indexed load of an array in scratch memory; five lane
    // reads and scalar selects stay in registers.)
    const uint32_t j = k >> 6, l = k & 63u;
    uint32_t v = rdlane(r[0], l);
    const uint32_t v1 = rdlane(r[1], l), v2 = rdlane(r[2], l), v3 = rdlane(r[3], l), v4 = rdlane(r[4], l);
    v = j == 1 ? v1 : v;
    v = j == 2 ? v2 : v;
    v = j == 3 ? v3 : v;
    v = j == 4 ? v4 : v;
    return v;
}

// Builds lens[] / cw[] for `num_syms` symbols from h.freq[].  All 64 lanes must call.
// NCH = 64-symbol chunks of the alphabet (5 for litlen, 1 for the offset code and the precode), MAXL = the
// code's length limit: the per-chunk and per-length loops below are unrolled to exactly what the alphabet
// needs -- written for the litlen code alone they made the 30-symbol offset code cost 62 % of the
// 286-symbol one (k_huffman's phases, tools/exp_huffman.py).
template <uint32_t NCH, uint32_t MAXL>
__device__ void make_code(HuffLds &h, uint32_t num_syms, uint32_t compat, uint8_t *lens, uint32_t *cw, uint32_t lane) {
    constexpr uint32_t max_len = MAXL;
    // keys + used count
    uint32_t used = 0;
    for (uint32_t base = 0; base < num_syms; base += 64) {
        const uint32_t s = base + lane;
        uint32_t f = 0;
        if (s < num_syms) {
            f = h.freq[s];
            h.key[s] = f ? ((f << 10) | s) : 0xFFFFFFFFu;
            lens[s] = 0;
            cw[s] = 0;
        }
        used += (uint32_t)__popcll(__ballot(f != 0));
    }
    wave_sync();
    if (used < 2) {
        if (used == 0 && compat == 1) return;  // libdeflate 1.10: empty code stays empty
        if (lane == 0) {
            uint32_t sym = 0;
            if (used)
                for (uint32_t s = 0; s < num_syms; s++)
                    if (h.freq[s]) sym = s;
            const uint32_t other = sym ? sym : 1;
            lens[0] = 1;
            cw[0] = 0;
            lens[other] = 1;
            cw[other] = 1;
        }
        wave_sync();
        return;
    }
    // Rank sort of the USED keys (distinct: the symbol is part of the key).  They are first packed to
    // the front of key[] (ballot ranks; every chunk is read before anything is written), so the
    // comparison loop runs over `used` keys and ceil(used / 64) chunks instead of num_syms and 5 --
    // about a quarter of the comparisons for a typical literal/length alphabet (~130 of 286 used).
    {
        uint32_t at = 0;  // wave-uniform
        uint32_t k0 = lane < num_syms ? h.key[lane] : 0xFFFFFFFFu;
        for (uint32_t base = 0; base < num_syms; base += 64) {
            // (the next chunk is read before this one is written: packed slots never run ahead of it)
            const uint32_t s1 = base + 64 + lane;
            const uint32_t k1 = s1 < num_syms ? h.key[s1] : 0xFFFFFFFFu;
            wave_sync();
            const bool u = k0 != 0xFFFFFFFFu;
            const unsigned long long m = __ballot(u);
            if (u) h.key[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = k0;
            at += (uint32_t)__popcll(m);
            k0 = k1;
        }
    }
    wave_sync();
    for (uint32_t base = 0; base < used; base += 64) {
        const uint32_t s = base + lane;
        const uint32_t k = s < used ? h.key[s] : 0u;  // (0: nothing counts as smaller)
        uint32_t rank = 0;
        for (uint32_t j = 0; j < used; j++) rank += h.key[j] < k ? 1u : 0u;
        if (s < used) {
            h.sfreq[rank] = k >> 10;
            h.ssym[rank] = (uint16_t)(k & 1023u);
        }
    }
    wave_sync();
    if (lane == 0) {
        // build_tree (two queues: sorted leaves sfreq[i], internal nodes nfreq[b..e))
        const uint32_t last = used - 1;
        uint32_t i = 0, bq = 0, e = 0;
        do {
            uint32_t nf;
            if (i + 1 <= last && (bq == e || h.sfreq[i + 1] <= h.nfreq[bq])) {
                nf = h.sfreq[i] + h.sfreq[i + 1];
                i += 2;
            } else if (bq + 2 <= e && (i > last || h.nfreq[bq + 1] < h.sfreq[i])) {
                nf = h.nfreq[bq] + h.nfreq[bq + 1];
                h.parent[bq] = (uint16_t)e;
                h.parent[bq + 1] = (uint16_t)e;
                bq += 2;
            } else {
                nf = h.sfreq[i] + h.nfreq[bq];
                h.parent[bq] = (uint16_t)e;
                i++;
                bq++;
            }
            h.nfreq[e] = nf;
        } while (++e < last);
    }
    wave_sync();
    // compute_length_counts.  Depths of the internal nodes by fixed-point iteration over
    // depth[node] = depth[parent[node]] + 1 (parents have higher indices; as many rounds as the
    // tree is high); when no leaf would get deeper than max_len -- the normal case -- the counts
    // follow from how many internal nodes sit at each depth, otherwise the sequential clamp runs.
    {
        const uint32_t last = used - 1, root = last - 1;
        uint32_t par[NCH], dep[NCH];
#pragma unroll
        for (uint32_t k = 0; k < NCH; k++) {
            const uint32_t node = lane + 64 * k;
            par[k] = node < root ? h.parent[node] : 0xFFFFu;
            dep[k] = node == root ? 0u : 0xFFu;
            if (node <= root) h.depth[node] = (uint8_t)dep[k];
        }
        wave_sync();
        for (;;) {
            bool changed = false;
#pragma unroll
            for (uint32_t k = 0; k < NCH; k++) {
                if (par[k] != 0xFFFFu && dep[k] == 0xFFu) {
                    const uint32_t pd = h.depth[par[k]];
                    if (pd != 0xFFu) {
                        dep[k] = pd + 1 > 0xFEu ? 0xFEu : pd + 1;
                        changed = true;
                    }
                }
            }
            wave_sync();
#pragma unroll
            for (uint32_t k = 0; k < NCH; k++)
                if (par[k] != 0xFFFFu && dep[k] != 0xFFu) h.depth[lane + 64 * k] = (uint8_t)dep[k];
            wave_sync();
            if (!__ballot(changed)) break;
        }
        uint32_t deepest = 0;
#pragma unroll
        for (uint32_t k = 0; k < NCH; k++)
            if (par[k] != 0xFFFFu && dep[k] > deepest) deepest = dep[k];
        const bool clamp = __ballot(deepest >= max_len) != 0;  // an internal node at depth >= max_len
        if (!clamp) {
            // len_counts[l] = [l == 1] * 2 - (#nodes at depth l) + 2 * (#nodes at depth l - 1)
            uint32_t prev = 0;
            for (uint32_t l = 1; l <= max_len; l++) {
                uint32_t c = 0;
#pragma unroll
                for (uint32_t k = 0; k < NCH; k++) c += (uint32_t)__popcll(__ballot(par[k] != 0xFFFFu && dep[k] == l));
                if (lane == 0) h.len_counts[l] = (l == 1 ? 2u : 0u) + 2u * prev - c;
                prev = c;
            }
            if (lane == 0) h.len_counts[0] = 0;
        } else if (lane == 0) {
            for (uint32_t l = 0; l <= max_len; l++) h.len_counts[l] = 0;
            h.len_counts[1] = 2;
            for (int node = (int)root - 1; node >= 0; node--) {
                uint32_t l = h.depth[node];
                if (l >= max_len) {
                    l = max_len;
                    do {
                        l--;
                    } while (h.len_counts[l] == 0);
                }
                h.len_counts[l]--;
                h.len_counts[l + 1] += 2;
            }
        }
    }
    wave_sync();
    // lengths: the k-th sorted symbol gets the length whose cumulative count (from max_len
    // downwards) covers k
    for (uint32_t base = 0; base < used; base += 64) {
        const uint32_t k = base + lane;
        if (k < used) {
            uint32_t acc = 0, l = max_len;
            for (; l >= 1; l--) {
                acc += h.len_counts[l];
                if (k < acc) break;
            }
            lens[h.ssym[k]] = (uint8_t)l;
        }
    }
    wave_sync();
    // canonical codewords: next_code[len] + (# lower symbols of the same length), bit-reversed
    uint32_t next_code[16];  // (wave-uniform; every loop over it unrolled, so it stays in registers)
    next_code[0] = 0;
    next_code[1] = 0;
#pragma unroll
    for (uint32_t l = 2; l <= MAXL; l++) next_code[l] = (next_code[l - 1] + h.len_counts[l - 1]) << 1;
    const uint64_t lane_below = (1ull << lane) - 1ull;
    for (uint32_t base = 0; base < num_syms; base += 64) {
        const uint32_t s = base + lane;
        const uint32_t myl = s < num_syms ? lens[s] : 0;
        const uint32_t code = code_rank_step<MAXL>(myl, next_code, lane_below);
        if (myl) cw[s] = canon_codeword(code, myl);
    }
    wave_sync();
}

// OR nbits (<= 25) bits of v into a zeroed bit string in LDS at bit position bitpos (any lane)
__device__ __forceinline__ void hdr_or_bits(uint32_t *hdr, uint32_t bitpos, uint32_t v, uint32_t nbits) {
    const uint32_t w = bitpos >> 5, sh = bitpos & 31u;
    atomicOr(&hdr[w], v << sh);
    if (sh + nbits > 32) atomicOr(&hdr[w + 1], v >> (32 - sh));
}

__device__ __forceinline__ void hdr_put(uint32_t *hdr, uint32_t &bitpos, uint32_t v, uint32_t nbits) {
    if (!nbits) return;
    const uint32_t w = bitpos >> 5, sh = bitpos & 31u;
    hdr[w] |= v << sh;
    if (sh + nbits > 32) hdr[w + 1] |= v >> (32 - sh);
    bitpos += nbits;
}

#ifndef GZPX_HUFF_WAVES
#define GZPX_HUFF_WAVES 6
#endif
__global__ __launch_bounds__(64, GZPX_HUFF_WAVES) void k_huffman(Config cfg, BlockMeta *__restrict__ meta_all,
                                                SubMeta *__restrict__ sub_all,
                                                const uint32_t *__restrict__ hist_all,
                                                uint32_t *__restrict__ codes_all,
                                                uint32_t *__restrict__ hdr_all) {
    __shared__ HuffLds h;
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    BlockMeta *meta = meta_all + b;
    SubMeta *sub = sub_all + (uint64_t)b * cfg.max_sub;
    const uint32_t n = meta->n;
    const uint32_t hdr_len = header_bytes(cfg.format);
    const uint32_t eof_len = (meta->is_last && cfg.format == 0) ? 28u : 0u;

    if (n <= cfg.passthrough) {
        // deflate_compress_none (short inputs, and every input at level 0): stored blocks only, one
        // per 65535 bytes (k_emit cuts them), the last one final
        if (lane == 0) {
            const uint32_t chunks = n ? (n + 65534u) / 65535u : 1u;
            const uint32_t c = 5u * chunks + n;
            meta->nsub = 1;
            meta->ntok = 0;
            sub[0].type = kStored;
            sub[0].tok_begin = 0;
            sub[0].tok_end = 0;
            sub[0].byte_begin = 0;
            sub[0].byte_len = n;
            sub[0].bit_begin = 0;
            sub[0].hdr_bits = 0;
            sub[0].is_final = 1;
            meta->payload_bytes = c;
            meta->framed_bytes = hdr_len + c + 8 + eof_len;
            if (cfg.format == 0 && c >= 65536u) meta->status = kStatusBlockSizeExceeded;
        }
        return;
    }

    const uint32_t nsub = meta->nsub;
    uint32_t bitpos = 0;  // bits of payload emitted so far (wave-uniform)
    for (uint32_t s = 0; s < nsub; s++) {
        const uint32_t *hist = hist_all + ((uint64_t)b * cfg.max_sub + s) * kHistStride;
        uint32_t *codes = codes_all + ((uint64_t)b * cfg.max_sub + s) * kCodeWords;
        uint32_t *hdr_out = hdr_all + ((uint64_t)b * cfg.max_sub + s) * kHdrWords;
        const uint32_t block_length = sub[s].byte_len;
        const uint32_t is_final = sub[s].is_final;

#ifdef GZPX_EXPERIMENT
        unsigned long long hx_t = __builtin_readcyclecounter();
#define GZPX_HLAP(slot)                                                                               \
    do {                                                                                              \
        const unsigned long long t_ = __builtin_readcyclecounter();                                   \
        if (lane == 0) atomicAdd(&g_exp_huff[(b & 1023u) * 8u + (slot)], t_ - hx_t);                  \
        hx_t = t_;                                                                                    \
    } while (0)
#else
#define GZPX_HLAP(slot) ((void)0)
#endif
        // ---- litlen code (EOB tallied once), offset code
        // per-lane copies of the frequencies for the cost sums (make_code reuses freq[]'s storage)
        uint32_t lfreq[5];
        for (uint32_t k = 0; k < 5; k++) {
            const uint32_t i = lane + 64 * k;
            lfreq[k] = i < kNumLitlen ? hist[i] + (i == 256 ? 1u : 0u) : 0;
            if (i < kNumLitlen) h.freq[i] = lfreq[k];
        }
        wave_sync();
        GZPX_HLAP(0);
        make_code<5, 14>(h, kNumLitlen, cfg.compat, h.lens, h.lcw, lane);
        GZPX_HLAP(1);
        const uint32_t ofreq = lane < kNumOffset ? hist[kNumLitlen + lane] : 0;
        if (lane < kNumOffset) h.freq[lane] = ofreq;
        wave_sync();
        make_code<1, 15>(h, kNumOffset, cfg.compat, h.olens, h.ocw, lane);
        GZPX_HLAP(2);
        wave_sync();

        // ---- deflate_precompute_huffman_header
        uint32_t num_litlen, num_offset;
        {
            uint32_t hi_l = 0;  // highest used litlen symbol + 1, at least 257
            for (uint32_t k = 0; k < 5; k++) {
                const uint32_t i = lane + 64 * k;
                if (i < kNumLitlen && h.lens[i]) hi_l = i + 1;
            }
            for (int m = 32; m >= 1; m >>= 1) {
                const uint32_t o = __shfl_xor(hi_l, m);
                hi_l = o > hi_l ? o : hi_l;
            }
            num_litlen = hi_l < 257 ? 257 : hi_l;
            uint32_t hi_o = (lane < kNumOffset && h.olens[lane]) ? lane + 1 : 0;
            for (int m = 32; m >= 1; m >>= 1) {
                const uint32_t o = __shfl_xor(hi_o, m);
                hi_o = o > hi_o ? o : hi_o;
            }
            num_offset = hi_o < 1 ? 1 : hi_o;
        }
        if (lane < num_offset) h.lens[num_litlen + lane] = h.olens[lane];
        if (lane < 32) h.pfreq[lane] = 0;
        wave_sync();
        uint32_t num_items;
        {
            // deflate_compute_precode_items: run-length coding of the concatenated code lengths, one
            // POSITION per lane (five per lane: <= 316 lengths) instead of a walk over the ~150 runs.
            // libdeflate's loops cut a run of zeros into pieces of 138 from its start (symbol 18 while
            // >= 11 are left, symbol 17 for 3..10, literal zeros for 1..2) and a run of >= 4 equal
            // non-zero lengths into one literal plus pieces of 6 (symbol 16 while >= 3 are left,
            // literals for the rest) -- so whether an item starts at a position, and which, follows
            // from the position's offset in its run and the run's length.  Run starts come from
            // ballots; items land in position order by their rank among the item starts.
            const uint32_t num_lens = num_litlen + num_offset;
            uint32_t lr[5];
            unsigned long long sm[5];  // run starts per chunk of 64 positions (uniform)
#pragma unroll
            for (uint32_t k = 0; k < 5; k++) {
                const uint32_t idx = lane + 64 * k;
                // (no length behind the last one: position num_lens "starts a run", which ends the last real one)
                lr[k] = idx < num_lens ? (uint32_t)h.lens[idx] : 0xFFu;
            }
#pragma unroll
            for (uint32_t k = 0; k < 5; k++) {
                uint32_t prev = (uint32_t)__shfl_up((int)lr[k], 1);
                const uint32_t carry = k ? rdlane(lr[k ? k - 1 : 0], 63) : 0x100u;  // (position 0 starts a run)
                if (lane == 0) prev = carry;
                sm[k] = __ballot(lr[k] != prev);
            }
            uint32_t ni = 0;
#pragma unroll
            for (uint32_t k = 0; k < 5; k++) {
                if (64 * k >= num_lens) break;  // (uniform)
                uint32_t before = 0, after = num_lens;  // the nearest run start in the chunks before / behind this one
#pragma unroll
                for (uint32_t j = 0; j < 5; j++)
                    if (j < k && sm[j]) before = 64 * j + 63u - (uint32_t)__clzll((long long)sm[j]);
#pragma unroll
                for (uint32_t j = 4; j >= 1; j--)
                    if (j > k && sm[j]) after = 64 * j + (uint32_t)__ffsll((long long)sm[j]) - 1u;
                const uint32_t idx = lane + 64 * k;
                const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;  // bits <= lane
                const unsigned long long lo = sm[k] & upto, hi = sm[k] & ~upto;
                const uint32_t rs = lo ? 64 * k + 63u - (uint32_t)__clzll((long long)lo) : before;
                const uint32_t re = hi ? 64 * k + (uint32_t)__ffsll((long long)hi) - 1u : after;
                const uint32_t L = re - rs, t = idx - rs, v = lr[k];
                bool is = idx < num_lens;
                uint32_t item = v;
                if (v == 0) {
                    const uint32_t tb = t >= 276u ? 276u : t >= 138u ? 138u : 0u;
                    const uint32_t rb = L - tb;
                    if (rb >= 11u) {
                        is = is && t == tb;
                        item = 18u | ((rb - 11u > 0x7Fu ? 0x7Fu : rb - 11u) << 5);
                    } else if (rb >= 3u) {
                        is = is && t == tb;
                        item = 17u | ((rb - 3u) << 5);
                    }
                } else if (L >= 4u && t != 0u) {
                    const uint32_t u = t - 1u;
                    const uint32_t ub = 6u * ((u * 10923u) >> 16);  // (u / 6, u < 316)
                    const uint32_t rb = L - 1u - ub;
                    if (rb >= 3u) {
                        is = is && u == ub;
                        item = 16u | ((rb - 3u > 3u ? 3u : rb - 3u) << 5);
                    }
                }
                const unsigned long long im = __ballot(is);
                if (is) {
                    h.items[ni + (uint32_t)__popcll(im & (upto >> 1))] = (uint16_t)item;
                    atomicAdd(&h.pfreq[item & 31u], 1u);
                }
                ni += (uint32_t)__popcll(im);
            }
            num_items = ni;
        }
        wave_sync();
        const uint32_t pf = lane < 19 ? h.pfreq[lane] : 0;
        wave_sync();
        if (lane < 32) h.freq[lane] = lane < 19 ? pf : 0;
        wave_sync();
        GZPX_HLAP(3);
        make_code<1, 7>(h, 19, cfg.compat, h.plens, h.pcw, lane);
        GZPX_HLAP(4);
        uint32_t num_explicit;
        {
            uint32_t ne = 4;
            for (uint32_t i = 0; i < 19; i++)
                if (h.plens[precode_order(i)]) ne = i + 1 > ne ? i + 1 : ne;
            num_explicit = ne;
        }

        // ---- exact bit costs (deflate_flush_block)
        uint32_t dyn = 0, sta = 0;
        if (lane < 19) {
            const uint32_t xb = lane == 16 ? 2u : lane == 17 ? 3u : lane == 18 ? 7u : 0u;
            dyn += pf * (xb + h.plens[lane]);
        }
        for (uint32_t k = 0; k < 5; k++) {
            const uint32_t i = lane + 64 * k;
            if (i >= kNumLitlen) break;
            const uint32_t f = lfreq[k];
            const uint32_t dl = h.lens[i];
            if (i < 256) {
                dyn += f * dl;
                sta += f * fixed_code_len(i);
            } else if (i == 256) {
                dyn += dl;  // one EOB
                sta += fixed_code_len(256);
            } else if (i < 257 + 29) {
                const uint32_t xb = length_sym(i - 257).xbits;
                dyn += f * (xb + dl);
                sta += f * (xb + fixed_code_len(i));
            }
        }
        if (lane < 30) {
            const uint32_t xb = offset_sym(lane).xbits;
            dyn += ofreq * (xb + h.olens[lane]);
            sta += ofreq * (xb + fixed_code_len(288 + lane));
        }
        dyn = wave_reduce_add(dyn) + 5 + 5 + 4 + 3 * num_explicit;
        sta = wave_reduce_add(sta);
        const uint32_t unc = ((0u - ((bitpos & 7u) + 3u)) & 7u) + 32u +
                             40u * ((block_length + 65534u) / 65535u - 1u) + 8u * block_length;

        uint32_t type, hdr_bits = 0, sub_bits;
        if (dyn < (sta < unc ? sta : unc)) {
            type = kDynamic;
        } else if (sta < unc) {
            type = kStatic;
        } else {
            type = kStored;
        }

        GZPX_HLAP(5);
        // ---- header bit string + code tables for k_emit
        for (uint32_t i = lane; i < kHdrWords; i += 64) h.hdr[i] = 0;
        wave_sync();
        if (type == kDynamic) {
            {
                // BFINAL, BTYPE, HLIT, HDIST, HCLEN (17 bits), the explicit precode lengths (3 bits
                // each, one per lane), then the items: codeword + extra bits, placed by a running
                // prefix sum of their bit counts and OR-ed into the header words
                if (lane == 0)
                    atomicOr(&h.hdr[0], is_final | (2u << 1) | ((num_litlen - 257) << 3) | ((num_offset - 1) << 8) |
                                            ((num_explicit - 4) << 13));
                if (lane < num_explicit) hdr_or_bits(h.hdr, 17 + 3 * lane, h.plens[precode_order(lane < 19 ? lane : 0)], 3);
                uint32_t bp = 17 + 3 * num_explicit;
                for (uint32_t base = 0; base < num_items; base += 64) {
                    const uint32_t i = base + lane;
                    uint32_t v = 0, nb = 0;
                    if (i < num_items) {
                        const uint32_t it = h.items[i];
                        const uint32_t psym = it & 31u, extra = it >> 5;
                        nb = h.plens[psym];
                        v = h.pcw[psym];
                        if (psym >= 16) {
                            v |= extra << nb;
                            nb += psym == 16 ? 2u : psym == 17 ? 3u : 7u;
                        }
                    }
                    const uint32_t incl = wave_incl_add(nb);
                    if (nb) hdr_or_bits(h.hdr, bp + incl - nb, v, nb);
                    bp += rdlane(incl, 63);
                }
                if (lane == 0) h.misc[1] = bp;
            }
            wave_sync();
            hdr_bits = h.misc[1];
            sub_bits = 3 + dyn;
            for (uint32_t i = lane; i < kNumLitlen; i += 64)
                codes[i] = h.lcw[i] | ((uint32_t)h.lens[i] << 16);
            if (lane < kNumOffset) codes[kNumLitlen + lane] = h.ocw[lane] | ((uint32_t)h.olens[lane] << 16);
        } else if (type == kStatic) {
            if (lane == 0) {
                uint32_t bp = 0;
                hdr_put(h.hdr, bp, is_final, 1);
                hdr_put(h.hdr, bp, 1, 2);
            }
            wave_sync();
            hdr_bits = 3;
            sub_bits = 3 + sta;
            // fixed codes of RFC 1951 3.2.6 (canonical, bit-reversed; the lengths are fixed_code_len's)
            for (uint32_t i = lane; i < kNumLitlen; i += 64) {
                uint32_t len, code;
                if (i < 144) {
                    len = 8;
                    code = 0x30 + i;
                } else if (i < 256) {
                    len = 9;
                    code = 0x190 + (i - 144);
                } else if (i < 280) {
                    len = 7;
                    code = i - 256;
                } else {
                    len = 8;
                    code = 0xC0 + (i - 280);
                }
                codes[i] = (__brev(code) >> (32 - len)) | (len << 16);
            }
            if (lane < kNumOffset) codes[kNumLitlen + lane] = (__brev(lane) >> 27) | (5u << 16);
        } else {
            hdr_bits = 0;
            // per <=65535-byte chunk: 3 header bits, pad to a byte, LEN, NLEN, data
            uint32_t bp = bitpos, left = block_length;
            do {
                const uint32_t chunk = left > 65535u ? 65535u : left;
                bp += 3;
                bp = (bp + 7u) & ~7u;
                bp += 32 + 8 * chunk;
                left -= chunk;
            } while (left);
            sub_bits = bp - bitpos;
        }
        for (uint32_t i = lane; i < kHdrWords; i += 64) hdr_out[i] = h.hdr[i];
        if (lane == 0) {
            sub[s].type = type;
            sub[s].bit_begin = bitpos;
            sub[s].hdr_bits = hdr_bits;
        }
        bitpos += sub_bits;
        wave_sync();
        GZPX_HLAP(6);
    }
#undef GZPX_HLAP
    if (lane == 0) {
        const uint32_t c = (bitpos + 7u) >> 3;
        meta->payload_bytes = c;
        meta->framed_bytes = hdr_len + c + 8 + eof_len;
        if (cfg.format == 0 && c >= 65536u) meta->status = kStatusBlockSizeExceeded;
    }
}

// ------------------------------------------------------------------------------------------
// CRC-32 of a buffer by one workgroup, two ways (the arithmetic both are made of: gzpx_crc.h).
// crc32_workgroup (k_dcrc32): the buffer is staged in LDS with coalesced dword loads (one HBM read of
// the input, no strided re-fetching).  1024 threads: thread t owns the 64-byte segment that ENDS at
// n - 64*(1023 - t) (so only the first used segment is short), runs slice-by-4 over it out of LDS
// (16 dependent steps; segments are laid out 17 dwords apart), and the 1024 CRCs are merged by a
// log-tree of zlib-style crc32_combine steps:
// crc(A||B) = crc(A) * x^(8|B|) mod P  xor  crc(B), with |B| = 64 * 2^level at every level.
// crc32_direct (k_crc32): 256 threads, 256-byte segments read straight from global memory, the same tree.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kCrcThreads = 1024;  // one 64-byte segment per thread and chunk (k_dcrc32)
constexpr uint32_t kCrcSmall = 256;     // the compressor's k_crc32: one 256-byte segment per thread and chunk
constexpr uint32_t kCrcSeg = 64;        // bytes per thread and chunk of crc32_workgroup
constexpr uint32_t kCrcSegWords = kCrcSeg / 4;  // 16
constexpr uint32_t kCrcChunk = kCrcThreads * kCrcSeg;  // 64 KiB; crc32_direct's 256 * 256 is the same

// dword index -> padded LDS index (one pad word after every 16: segments lie 17 dwords apart, so
// the 64 lanes of a wave, each in its own segment, spread evenly over the banks)
__device__ __forceinline__ uint32_t crc_pad(uint32_t w) { return w + (w / kCrcSegWords); }

struct CrcWgLds {
    uint32_t table[4][256];
    uint32_t data[(kCrcChunk / 4 + 2) + (kCrcChunk / 4 + 2) / kCrcSegWords + 2];
    uint32_t part[kCrcThreads];
};

// CRC-32 of in[0..n) by a workgroup of kCrcThreads (ten combine levels, chunk constant cc.pow_tile); the
// result is valid in every thread.
__device__ uint32_t crc32_workgroup(CrcWgLds &l, const uint8_t *__restrict__ in, uint32_t n, const CrcConsts &cc,
                                    uint32_t tid) {
    constexpr uint32_t T = kCrcThreads, kChunk = kCrcChunk;
    crc_tables_fill<kCrcPoly32>(l.table, tid, T);
    // Inputs above one chunk are cut into chunks aligned to the END of the input (only the first
    // chunk is short), so every chunk-to-chunk combine uses the same x^(8 * chunk) constant.
    uint32_t total = 0;
    const uint32_t first_len = n ? ((n - 1) % kChunk) + 1 : 0;
    for (uint32_t cb = 0; cb < n || cb == 0; cb += (cb == 0 ? first_len : kChunk)) {
        const uint32_t clen = n == 0 ? 0 : (cb == 0 ? first_len : kChunk);
        const uint8_t *cin = in + cb;
        const uint32_t mis = (uint32_t)((uintptr_t)cin & 3u);
        __syncthreads();  // tables ready / previous chunk consumed
        if (clen) {
            const uint32_t *src = (const uint32_t *)(cin - mis);
            const uint32_t ndw = (mis + clen + 3) >> 2;
            for (uint32_t i = tid; i < ndw; i += T) l.data[crc_pad(i)] = src[i];
        }
        __syncthreads();
        // segment of thread t in chunk bytes: [clen - 64*(T - t), clen - 64*(T - 1 - t)) clipped
        // at 0; LDS byte address of chunk byte i is i + mis (before padding)
        const int32_t seg_end_i = (int32_t)clen - (int32_t)kCrcSeg * (int32_t)(T - 1 - tid);
        uint32_t crc = 0;
        if (seg_end_i > 0) {
            const uint32_t seg_end = (uint32_t)seg_end_i + mis;
            uint32_t pos = (seg_end_i > (int32_t)kCrcSeg ? (uint32_t)(seg_end_i - (int32_t)kCrcSeg) : 0u) + mis;
            uint32_t c = 0xFFFFFFFFu;
            auto byte_at = [&](uint32_t at) { return (l.data[crc_pad(at >> 2)] >> (8u * (at & 3u))) & 0xFFu; };
            for (; pos < seg_end && (pos & 3u); pos++) c = crc_byte(l.table, c, byte_at(pos));  // up to a dword boundary
            for (; pos + 4 <= seg_end; pos += 4) c = crc_word(l.table, c, l.data[crc_pad(pos >> 2)]);
            for (; pos < seg_end; pos++) c = crc_byte(l.table, c, byte_at(pos));
            crc = ~c;
        }
        l.part[tid] = crc;
        __syncthreads();
        // the pairs of a level are handled by the LOWEST threads, so that a level keeps only as many
        // waves busy as it has work for
        for (uint32_t level = 0; level < 10; level++) {
            const uint32_t stride = 1u << level;
            const uint32_t left = 2 * stride * tid;  // index of the pair's left part
            uint32_t merged = 0;
            const bool act = left < T;
            if (act) merged = crc_mulmod<kCrcPoly32>(cc.pow64[level], l.part[left]) ^ l.part[left + stride];
            __syncthreads();
            if (act) l.part[left] = merged;
            __syncthreads();
        }
        // crc(A || chunk) = crc(A) * x^(8 * chunk) + crc(chunk); the first chunk has no A.  (The constant is the
        // second factor: as the first, its 32 bit tests are hoisted out of the loop as 64-bit masks, which spill.)
        total = cb == 0 ? l.part[0] : (crc_mulmod<kCrcPoly32>(total, cc.pow_tile) ^ l.part[0]);
        if (n == 0) break;
    }
    return total;
}

// CRC-32 of in[0..n) by a 256-thread workgroup whose threads read their bytes straight from global
// memory: thread t owns ONE contiguous 256-byte segment per 64 KiB chunk (segments aligned to the end of
// the input, so only the first is short), runs slice-by-4 over it out of registers (crc_seg256), and the
// 256 partial CRCs are combined by the GF(2) log-tree once per chunk.  Against 64-byte segments staged in
// LDS with a tree per 16 KiB, which this replaced: a BGZF block needs one tree instead of four to five (the
// tree was more than half of that routine's instructions), no staging traffic through LDS, and 5 KiB of
// LDS instead of 21.
struct CrcDirectLds {
    uint32_t table[4][256];
    uint32_t part[kCrcSmall];
};

__device__ uint32_t crc32_direct(CrcDirectLds &l, const uint8_t *__restrict__ in, uint32_t n, const CrcConsts &cc,
                                 uint32_t tid) {
    constexpr uint32_t T = kCrcSmall, kSegB = 256, kChunk = T * kSegB;  // 64 KiB per chunk
    crc_tables_fill<kCrcPoly32>(l.table, tid, T);
    uint32_t total = 0;
    const uint32_t first_len = n ? ((n - 1) % kChunk) + 1 : 0;
    for (uint32_t cb = 0; cb < n || cb == 0; cb += (cb == 0 ? first_len : kChunk)) {
        const uint32_t clen = n == 0 ? 0 : (cb == 0 ? first_len : kChunk);
        __syncthreads();  // tables ready / part[] of the previous chunk consumed
        const int32_t seg_end_i = (int32_t)clen - (int32_t)kSegB * (int32_t)(T - 1 - tid);
        uint32_t crc = 0;
        if (seg_end_i > 0) {
            const uint32_t sb = seg_end_i > (int32_t)kSegB ? (uint32_t)seg_end_i - kSegB : 0u;
            const uint32_t len = (uint32_t)seg_end_i - sb;
            const uint8_t *p = in + cb + sb;
            if (len == kSegB) crc = ~crc_seg256(l.table, p, cb + (uint32_t)seg_end_i == n, 0xFFFFFFFFu);
            else crc = ~crc_bytes(l.table, p, len, 0xFFFFFFFFu);  // the short first segment of the input (one thread per input)
        }
        l.part[tid] = crc;
        __syncthreads();
        // log-tree over the 256 parts: x^(8 * 256 * 2^level) = pow64[level + 2]; a level's pairs are
        // handled by the LOWEST threads, so that it keeps only as many waves busy as it has work for
        for (uint32_t level = 0; level < 8; level++) {
            const uint32_t stride = 1u << level;
            const uint32_t left = 2 * stride * tid;
            uint32_t merged = 0;
            const bool act = left < T;
            if (act) merged = crc_mulmod<kCrcPoly32>(cc.pow64[level + 2], l.part[left]) ^ l.part[left + stride];
            __syncthreads();
            if (act) l.part[left] = merged;
            __syncthreads();
        }
        // crc(A || chunk) = crc(A) * x^(8 * chunk) + crc(chunk); the first chunk has no A.  (The constant is the
        // second factor: as the first, its 32 bit tests are hoisted out of the loop as 64-bit masks, which spill.)
        total = cb == 0 ? l.part[0] : (crc_mulmod<kCrcPoly32>(total, cc.pow_tile) ^ l.part[0]);
        if (n == 0) break;
    }
    return total;
}

// The compressor's CRC kernel needs nothing but the input, so it runs on a low-priority SIDE STREAM
// beside k_hist / k_huffman (gzpx_api.cpp, enqueue_batch): small workgroups (256 threads, 5 KiB of
// LDS) that slip in between k_huffman's one-wave workgroups.  (The 1024-thread routine of k_dcrc32
// in the same place: the join waits 0.24 ms for it, step 4.86 -> 5.00 ms.)
__global__ __launch_bounds__(kCrcSmall) void k_crc32(Config cfg, const uint8_t *__restrict__ slab,
                                                     BlockMeta *__restrict__ meta_all, CrcConsts cc) {
    __shared__ CrcDirectLds l;
    const uint32_t b = blockIdx.x;
    const uint32_t total = crc32_direct(l, slab + (uint64_t)b * cfg.block_size, meta_all[b].n, cc, threadIdx.x);
    if (threadIdx.x == 0) meta_all[b].crc = total;
}

// ------------------------------------------------------------------------------------------
// k_scan: exclusive scan of the framed block sizes -> byte offset of every block in the output
// stream (the in-order property of the reference's writer loop, src/par/compress.rs:305-310).
// ------------------------------------------------------------------------------------------
// (One workgroup: the kernel is a chain of memory round trips, not work.  Every thread owns a run of
// consecutive blocks, so the loads of a pass are independent and in flight together: two passes of
// ceil(nb / 1024) loads per thread around ONE workgroup scan -- the 550 MiB slab's 8,815 blocks in
// 0.034 -> 0.0xx ms; it was 35 scans of 256 blocks, each waiting for its own loads.)
constexpr uint32_t kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_scan(uint32_t nb, const BlockMeta *__restrict__ meta,
                                                       uint64_t *__restrict__ out_off, uint32_t *__restrict__ sizes,
                                                       const SlabResult *__restrict__ prev,
                                                       SlabResult *__restrict__ result) {
    __shared__ uint64_t wsum[kScanThreads / 64];
    __shared__ uint32_t fail_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) fail_s = 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t per = (nb + kScanThreads - 1) / kScanThreads;
    const uint32_t i0 = tid * per < nb ? tid * per : nb, i1 = i0 + per < nb ? i0 + per : nb;
    uint64_t mine = 0;
    uint32_t bad = 0xFFFFFFFFu;
#pragma unroll 8
    for (uint32_t i = i0; i < i1; i++) {
        mine += meta[i].framed_bytes;
        if (meta[i].status != kStatusOk && bad == 0xFFFFFFFFu) bad = i;
    }
    if (bad != 0xFFFFFFFFu) atomicMin(&fail_s, bad);
    uint64_t inc = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(inc, d);
        if (lane >= (unsigned)d) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint64_t run = prev ? prev->total : 0;  // a slab of several batches: offsets run on
    uint64_t total = run;
    for (uint32_t w = 0; w < kScanThreads / 64; w++) {
        const uint64_t v = wsum[w];
        if (w < wave) run += v;
        total += v;
    }
    run += inc - mine;
#pragma unroll 8
    for (uint32_t i = i0; i < i1; i++) {
        const uint32_t v = meta[i].framed_bytes;
        sizes[i] = v;
        out_off[i] = run;
        run += v;
    }
    if (tid == 0) {
        const uint32_t f = fail_s;
        out_off[nb] = total;
        result->total = total;
        result->fail_block = f;
        result->fail_status = f != 0xFFFFFFFFu ? meta[f].status : kStatusOk;
    }
}

// ------------------------------------------------------------------------------------------
// k_emit: assemble each framed block (gzip header with the BC/IG extra field, DEFLATE payload,
// CRC32 + ISIZE footer, BGZF_EOF after the last block) in LDS at the byte alignment it will
// have in the output stream, then write it out with aligned dword stores.
// ------------------------------------------------------------------------------------------
// The stage is a sliding window over the block's output: when the next piece (a header, 1024
// tokens, 16 KiB of stored bytes, the footer) might not fit, everything complete is written out
// and the window moves on.  A 64 KiB BGZF block never needs to slide.
constexpr uint32_t kStageWords = 18224;  // 71.2 KiB (a BGZF block is at most 65,6xx bytes; the rest of 72 KiB: the length table, the second set of wave sums)

__device__ __forceinline__ void stage_or_bits(uint32_t *stage, uint32_t bitpos, uint64_t v) {
    const uint32_t w = bitpos >> 5, sh = bitpos & 31u;
    const uint64_t t = v << sh;
    const uint32_t x0 = (uint32_t)t, x1 = (uint32_t)(t >> 32);
    const uint32_t x2 = sh ? (uint32_t)(v >> (64 - sh)) : 0u;
    if (x0) atomicOr(&stage[w], x0);
    if (x1) atomicOr(&stage[w + 1], x1);
    if (x2) atomicOr(&stage[w + 2], x2);
}

__device__ __forceinline__ void stage_put_byte(uint32_t *stage, uint32_t byte_idx, uint32_t v) {
    atomicOr(&stage[byte_idx >> 2], (v & 0xFFu) << (8u * (byte_idx & 3u)));
}

// Write the window's bytes [win_base, upto) (coordinates: bytes from the 4-byte-aligned address
// just below the block's first output byte) to global memory: whole dwords where every byte
// belongs to this block, single bytes at the block's two edges.
constexpr uint32_t kEmitThreads = 1024;
constexpr uint32_t kEmitTpl = 4;                         // tokens per thread and step of the token loop (8: the compiler spills)
constexpr uint32_t kEmitStep = kEmitTpl * kEmitThreads;  // tokens per workgroup scan
// The sub-block's codes in LDS, as the token loop wants them:
//   [0, 288)    litlen symbols: codeword | length << 24 (so a literal and a match length are read alike)
//   [288, 320)  offset symbols: codeword | length << 16, as in global memory
//   [320, 576)  match length - 3 -> length codeword with its extra bits above | the bit count of both << 24
constexpr uint32_t kEmitLenTab = kCodeWords;
constexpr uint32_t kEmitCodeWords = kCodeWords + 256;
constexpr uint32_t kNullSym = 287;  // a litlen symbol no stream holds: its entry is kept 0, the token without bits
static_assert(kEmitTpl % 4 == 0 && kEmitTpl <= 8, "16-byte token loads; two byte-wide bit counts summed in one word");

__device__ __forceinline__ void stage_flush(const uint32_t *stage, uint8_t *dst_aligned,
                                            uint32_t win_base, uint32_t upto, uint32_t lead,
                                            uint32_t end_byte, uint32_t tid) {
    const uint32_t words = (upto - win_base + 3) >> 2;
    for (uint32_t w = tid; w < words; w += kEmitThreads) {
        const uint32_t v = stage[w];
        const uint32_t b0 = win_base + 4 * w;
        if (b0 >= lead && b0 + 4 <= end_byte && b0 + 4 <= upto) {
            *(uint32_t *)(dst_aligned + b0) = v;
        } else {
            for (uint32_t k = 0; k < 4; k++)
                if (b0 + k >= lead && b0 + k < end_byte && b0 + k < upto)
                    dst_aligned[b0 + k] = (uint8_t)(v >> (8 * k));
        }
    }
}

// block_exclusive_scan with ONE barrier: consecutive steps of a sub-block's token loop alternate between two sets of
// wave sums, and a wave that writes a set again has passed the barrier of the step between (or the barriers between
// two sub-blocks), behind every reader of that set.
__device__ __forceinline__ uint32_t emit_scan(uint32_t v, uint32_t *wsum, uint32_t *total) {
    constexpr unsigned NW = kEmitThreads / 64;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t inc = wave_incl_add(v);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    const uint32_t mine = lane < NW ? wsum[lane] : 0u;
    const uint32_t winc = wave_incl_add(mine);
    *total = rdlane(winc, NW - 1);
    const uint32_t base = wave ? rdlane(winc, wave - 1) : 0u;
    return base + inc - v;
}

__device__ __forceinline__ void emit_block(const Config &cfg, const uint8_t *__restrict__ slab,
                                           const BlockMeta *__restrict__ meta_all,
                                           const SubMeta *__restrict__ sub_all,
                                           const uint32_t *__restrict__ tok_all,
                                           const uint32_t *__restrict__ codes_all,
                                           const uint32_t *__restrict__ hdr_all,
                                           const uint64_t *__restrict__ out_off,
                                           uint8_t *__restrict__ out, uint64_t out_cap, const uint32_t b,
                                           uint32_t *stage, uint32_t *codes, uint32_t *wsum) {
    const uint32_t tid = threadIdx.x;
    const BlockMeta *meta = meta_all + b;
    const SubMeta *sub = sub_all + (uint64_t)b * cfg.max_sub;
    const uint32_t n = meta->n;
    const uint32_t framed = meta->framed_bytes;
    const uint32_t c = meta->payload_bytes;
    const uint64_t dst_off = out_off[b];
    if (meta->status != kStatusOk || dst_off + framed > out_cap) return;  // host reports the error
    const uint8_t *in = slab + (uint64_t)b * cfg.block_size;
    const uint32_t hdr_len = header_bytes(cfg.format);
    // "aligned coordinates": byte i of the framed block lives at lead + i, so that dword
    // boundaries of the stage are dword boundaries of the output address
    const uint32_t lead = (uint32_t)(((uintptr_t)out + dst_off) & 3u);
    uint8_t *dst_aligned = out + dst_off - lead;
    const uint32_t end_byte = lead + framed;
    uint32_t win_base = 0;  // aligned coordinate of stage[0] (multiple of 4)

    // (only what the block will use; a block that slides zeroes the whole window from then on)
    const uint32_t used_words = (end_byte + 3) >> 2 < kStageWords ? (end_byte + 3) >> 2 : kStageWords;
    for (uint32_t i = tid; i < used_words; i += kEmitThreads) stage[i] = 0;
    __syncthreads();

    // ---- gzip member header (src/bgzf.rs:274-303 / src/mgzip.rs:246-275)
    if (tid == 0) {
        const uint32_t hb = lead;
        stage_put_byte(stage, hb + 0, 0x1f);
        stage_put_byte(stage, hb + 1, 0x8b);
        stage_put_byte(stage, hb + 2, 8);
        stage_put_byte(stage, hb + 3, 4);
        stage_put_byte(stage, hb + 8, cfg.xfl);
        stage_put_byte(stage, hb + 9, 255);
        if (cfg.format == 0) {
            const uint32_t bsize = c + 25;  // total block size - 1
            stage_put_byte(stage, hb + 10, 6);
            stage_put_byte(stage, hb + 12, 'B');
            stage_put_byte(stage, hb + 13, 'C');
            stage_put_byte(stage, hb + 14, 2);
            stage_put_byte(stage, hb + 16, bsize);
            stage_put_byte(stage, hb + 17, bsize >> 8);
        } else {
            const uint32_t tot = c + 28;
            stage_put_byte(stage, hb + 10, 8);
            stage_put_byte(stage, hb + 12, 'I');
            stage_put_byte(stage, hb + 13, 'G');
            stage_put_byte(stage, hb + 14, 4);
            stage_put_byte(stage, hb + 16, tot);
            stage_put_byte(stage, hb + 17, tot >> 8);
            stage_put_byte(stage, hb + 18, tot >> 16);
            stage_put_byte(stage, hb + 19, tot >> 24);
        }
    }

    const uint32_t *tok = tok_all + (uint64_t)b * cfg.stride;
    const uint32_t nsub = meta->nsub;
    // bit cursor, relative to the window (stage[0] = aligned coordinate win_base)
    uint32_t bitpos = 8u * (lead + hdr_len);
    // Make room for `need_bits` more bits (+ slack for the 3-word OR) by writing out every
    // complete dword and sliding the window so that the dword being filled becomes stage[0].
    // Uniform: all threads call it at the same points.
    auto ensure = [&](uint32_t need_bits) {
        if (((bitpos + need_bits + 7) >> 3) + 16u <= 4u * kStageWords) return;
        __syncthreads();
        const uint32_t upto_rel = (bitpos >> 3) & ~3u;
        stage_flush(stage, dst_aligned, win_base, win_base + upto_rel, lead, end_byte, tid);
        const uint32_t keep = stage[upto_rel >> 2];
        __syncthreads();
        for (uint32_t i = tid; i < kStageWords; i += kEmitThreads) stage[i] = 0;
        __syncthreads();
        if (tid == 0) stage[0] = keep;
        win_base += upto_rel;
        bitpos -= 8u * upto_rel;
        __syncthreads();
    };
    for (uint32_t s = 0; s < nsub; s++) {
        const SubMeta sm = sub[s];
        // (sm.bit_begin is where this sub-block starts inside the payload; the cursor is there)
        if (sm.type == kStored) {
            uint32_t left = sm.byte_len, src = sm.byte_begin;
            do {
                const uint32_t chunk = left > 65535u ? 65535u : left;
                const bool last_chunk = chunk == left;
                ensure(64);
                if (tid == 0) stage_or_bits(stage, bitpos, (sm.is_final && last_chunk) ? 1u : 0u);
                bitpos = (bitpos + 3 + 7u) & ~7u;
                if (tid == 0) {
                    const uint32_t bytepos = bitpos >> 3;
                    stage_put_byte(stage, bytepos + 0, chunk);
                    stage_put_byte(stage, bytepos + 1, chunk >> 8);
                    stage_put_byte(stage, bytepos + 2, ~chunk);
                    stage_put_byte(stage, bytepos + 3, (~chunk) >> 8);
                }
                bitpos += 32;
                for (uint32_t done = 0; done < chunk; done += 16384u) {  // raw bytes, 16 KiB at a time
                    const uint32_t piece = chunk - done < 16384u ? chunk - done : 16384u;
                    ensure(8u * piece);
                    const uint32_t bytepos = bitpos >> 3;
                    for (uint32_t i = tid; i < piece; i += kEmitThreads)
                        stage_put_byte(stage, bytepos + i, in[src + done + i]);
                    bitpos += 8u * piece;
                }
                src += chunk;
                left -= chunk;
            } while (left);
            __syncthreads();
            continue;
        }
        // ---- Huffman-coded sub-block: header bits, tokens, end-of-block
        __syncthreads();  // the previous sub-block is done with `codes`
        const uint32_t *cd = codes_all + ((uint64_t)b * cfg.max_sub + s) * kCodeWords;
        if (tid < kEmitCodeWords) {
            uint32_t e;
            if (tid < kNumLitlen) {
                const uint32_t lc = cd[tid];
                e = tid == kNullSym ? 0u : (lc & 0xFFFFu) | (lc >> 16 << 24);
            } else if (tid < kEmitLenTab) {
                e = cd[tid];
            } else {
                const uint32_t x = tid - kEmitLenTab, lt = length_entry(x);
                const uint32_t lc = cd[257u + (lt & 31u)], le = lt >> 5;
                e = (lc & 0xFFFFu) | ((x & ((1u << le) - 1u)) << (lc >> 16)) | (((lc >> 16) + le) << 24);
            }
            codes[tid] = e;
        }
        const uint32_t *hw = hdr_all + ((uint64_t)b * cfg.max_sub + s) * kHdrWords;
        const uint32_t nhw = (sm.hdr_bits + 31) >> 5;
        ensure(32u * kHdrWords);
        for (uint32_t i = tid; i < nhw; i += kEmitThreads) stage_or_bits(stage, bitpos + 32 * i, hw[i]);
        bitpos += sm.hdr_bits;
        __syncthreads();
        // kEmitTpl consecutive tokens per thread and step, from an index that is a multiple of 4: 16-byte
        // token loads, one workgroup scan per kEmitStep tokens.  A wave whose tokens all lie behind tok_end
        // takes part in the scan only; a wave that straddles an end of [tok_begin, tok_end) swaps the
        // tokens outside for kNullSym, which has no bits.  (Token rows are 16-byte aligned and padded by
        // 2048 entries: a wave that begins inside the sub-block may load all its tokens.)  The next step's
        // tokens are fetched a step ahead.
        const uint32_t wtok = uniform((tid >> 6) * (64u * kEmitTpl));  // this wave's first token within a step
        const uint32_t *ltok = tok + kEmitTpl * tid;
        uint4 tnext[kEmitTpl / 4];
        if ((sm.tok_begin & ~3u) + wtok < sm.tok_end) {
#pragma unroll
            for (uint32_t q = 0; q < kEmitTpl / 4; q++) tnext[q] = *(const uint4 *)(ltok + (sm.tok_begin & ~3u) + 4 * q);
        }
        uint32_t step = 0;
        for (uint32_t tb = sm.tok_begin & ~3u; tb < sm.tok_end; tb += kEmitStep) {
            // per token: first symbol's codeword + extra bits (<= 20 bits), offset codeword + extra bits
            // (<= 28, none for a literal), and the two bit counts in one word (low byte | next byte)
            uint32_t pa[kEmitTpl], pb[kEmitTpl], nn[kEmitTpl], sumnn = 0;
#pragma unroll
            for (uint32_t j = 0; j < kEmitTpl; j++) pa[j] = pb[j] = nn[j] = 0;
            const bool live = tb + wtok < sm.tok_end;
            if (live) {
                uint32_t t[kEmitTpl];
#pragma unroll
                for (uint32_t q = 0; q < kEmitTpl / 4; q++) {
                    t[4 * q + 0] = tnext[q].x;
                    t[4 * q + 1] = tnext[q].y;
                    t[4 * q + 2] = tnext[q].z;
                    t[4 * q + 3] = tnext[q].w;
                }
                if (tb + wtok < sm.tok_begin || tb + wtok + 64u * kEmitTpl > sm.tok_end) {
#pragma unroll
                    for (uint32_t j = 0; j < kEmitTpl; j++) {
                        const uint32_t i = tb + kEmitTpl * tid + j;
                        if (i < sm.tok_begin || i >= sm.tok_end) t[j] = kNullSym;
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < kEmitTpl; j++) {
                    const uint32_t tk = t[j];
                    const bool m = (int32_t)tk < 0;
                    const uint32_t lc = codes[m ? kEmitLenTab + ((tk - 3u) & 0xFFu) : tk];
                    const uint32_t d = m ? ((tk >> 9) & 0xFFFFu) - 1u : 0u;
                    const DeflateSlot os = offset_slot(d);  // (a literal: slot 0, no extra bits)
                    // (read by every lane and masked: a branch here would keep the tokens' LDS reads apart)
                    const uint32_t oc = codes[kNumLitlen + os.slot] & (uint32_t)((int32_t)tk >> 31);
                    pa[j] = lc & 0xFFFFFFu;
                    pb[j] = (oc & 0xFFFFu) | (os.xval << (oc >> 16));
                    nn[j] = (lc >> 24) | (((oc >> 16) + os.xbits) << 8);
                    sumnn += nn[j];  // (8 tokens: <= 160 and <= 224, the bytes do not carry)
                }
                // (fetched here, not before the lookups: the scan and the bit writer cover the latency, and this step's
                // token registers are free again)
                if (tb + kEmitStep + wtok < sm.tok_end) {
#pragma unroll
                    for (uint32_t q = 0; q < kEmitTpl / 4; q++) tnext[q] = *(const uint4 *)(ltok + tb + kEmitStep + 4 * q);
                }
            }
            uint32_t total;
            const uint32_t ex = emit_scan((sumnn & 0xFFu) + (sumnn >> 8), wsum + (kEmitThreads / 64) * (step & 1u), &total);
            step++;
            ensure(total);
            if (live) {
                // The lane's bits go through a 32-bit accumulator that starts at the lane's bit offset within its
                // first dword and hands over every dword it completes.  Only the first and the last dword are
                // shared with a neighbour; the OR into the zeroed stage serves both kinds.
                uint32_t *w = stage + ((bitpos + ex) >> 5);
                uint32_t accn = (bitpos + ex) & 31u, lo = 0;
                auto append = [&](uint32_t v, uint32_t nbits) {
                    lo |= v << accn;
                    accn += nbits;
                    if (accn >= 32u) {  // (nbits <= 28: there were bits before, and 1..31 of v's are left over or none)
                        atomicOr(w, lo);
                        w++;
                        accn -= 32u;
                        lo = v >> (nbits - accn);
                    }
                };
#pragma unroll
                for (uint32_t j = 0; j < kEmitTpl; j++) {
                    append(pa[j], nn[j] & 0xFFu);
                    append(pb[j], nn[j] >> 8);
                }
                if (lo) atomicOr(w, lo);
            }
            bitpos += total;
        }
        ensure(64);
        if (tid == 0) {
            const uint32_t ec = codes[256];
            stage_or_bits(stage, bitpos, ec & 0xFFFFFFu);
        }
        bitpos += codes[256] >> 24;
        __syncthreads();
    }

    // ---- footer (src/bgzf.rs:233-234) and, after the stream's last block, BGZF_EOF
    ensure(8u * (8u + 28u + 8u));
    if (tid == 0) {
        const uint32_t fb = lead + hdr_len + c - win_base;
        const uint32_t crc = meta->crc;
        for (uint32_t k = 0; k < 4; k++) {
            stage_put_byte(stage, fb + k, crc >> (8 * k));
            stage_put_byte(stage, fb + 4 + k, n >> (8 * k));
        }
        if (meta->is_last && cfg.format == 0) {
            // BGZF_EOF (src/bgzf.rs:24-38), appended inside the last block by Bgzf::encode
            const uint8_t eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
                                     0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0, 0, 0, 0, 0, 0, 0, 0};
            for (uint32_t k = 0; k < 28; k++) stage_put_byte(stage, fb + 8 + k, eof[k]);
        }
    }
    __syncthreads();
    stage_flush(stage, dst_aligned, win_base, end_byte, lead, end_byte, tid);
}

// (One workgroup per block.  Measured in round 3: two or four persistent workgroups per CU walking the blocks
// blockIdx.x, + gridDim.x, ... 0.383 -> 0.423 / 0.411 ms -- blocks differ in cost and the dispatcher balances
// them better than a fixed stride; the loop below is what is left of that and runs once.)
__global__ __launch_bounds__(kEmitThreads, 8) void k_emit(Config cfg, const uint8_t *__restrict__ slab,
                                              const BlockMeta *__restrict__ meta_all,
                                              const SubMeta *__restrict__ sub_all,
                                              const uint32_t *__restrict__ tok_all,
                                              const uint32_t *__restrict__ codes_all,
                                              const uint32_t *__restrict__ hdr_all,
                                              const uint64_t *__restrict__ out_off,
                                              uint8_t *__restrict__ out, uint64_t out_cap, uint32_t nb) {
    __shared__ uint32_t stage[kStageWords];
    __shared__ uint32_t codes[kEmitCodeWords];
    __shared__ uint32_t wsum[2 * (kEmitThreads / 64)];
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        __syncthreads();  // the previous block is done with the stage
        emit_block(cfg, slab, meta_all, sub_all, tok_all, codes_all, hdr_all, out_off, out, out_cap, b, stage, codes, wsum);
    }
}

// ------------------------------------------------------------------------------------------
// ParDecompress<Bgzf/Mgzip> (src/par/decompress.rs:132-220): every block is an independent gzip
// member, so a slab of blocks is inflated by one launch.
//   k_dinit    footer (CRC32, ISIZE) of every block -> DBlock
//   k_dscan    exclusive scan of ISIZE -> output offsets
//   k_inflate  libdeflate_deflate_decompress for every block: one wave per block.  The wave writes
//              its output straight to HBM and reads match sources back from there (the DEFLATE
//              window is the block's own output); compressed dwords come through a 1 KiB LDS ring
//              with one 256-byte piece prefetched in registers; Huffman decode tables (10-bit /
//              8-bit direct lookup + canonical fallback) are rebuilt in LDS for every dynamic
//              sub-block by all 64 lanes.  Symbols are decoded 128 bit positions per round: every
//              lane decodes the symbol that would start at its two positions, a scalar walk picks
//              the real ones, a prefix sum places them, and each output pass writes 64 bytes.
//   k_crc32    (shared with the compressor) CRC-32 of the inflated bytes, checked against the footer
// ------------------------------------------------------------------------------------------
struct InfLds {
    // No window here: output bytes go straight to the block's place in HBM and matches read them back from
    // there (L2-hot).  An earlier version kept a 32 KiB ring of the most recent output bytes (the DEFLATE window)
    // in LDS and flushed it to HBM in dwords; without it ~7.7 KiB are left, so 20 waves share a CU instead of 4
    // and hide each other's latencies (measured: 2 / 3 / 4 / 5 / 6 waves per SIMD = 52 / 58 / 58 / 65 / 62 GiB/s
    // on the bench stream; the LDS-ring version with 1: 23).
    uint32_t ring_was_here;  // (one word where the ring began: every offset below, and with them k_inflate's instructions, stay as measured)
    uint32_t lfast[1024];   // litlen entries for codes of <= 10 bits, 0 = longer code
    uint32_t ofast[256];    // offset entries for codes of <= 8 bits (and the 7-bit precode table)
    uint32_t inr[256];      // ring of compressed dwords (absolute dword index & 255)
    uint32_t own[64];       // output pass: which symbol starts at each output byte
    uint16_t lsorted[288];  // symbols in canonical order
    uint16_t osorted[32];
    uint8_t lens[320];      // code lengths: litlen then offset
    uint32_t lcount[16], lfirst[16], loffs[16];
    uint32_t ocount[16], ofirst[16], ooffs[16];
};

#ifndef GZPX_INF_R
#define GZPX_INF_R 2
#endif
constexpr uint32_t kInfR = GZPX_INF_R;  // groups of 64 bit positions decoded per round

// Decode-table entries (32 bit).  bits 0-3: codeword length (0 = not in the fast table);
//   litlen: bits 4-5 type (0 literal, 1 length, 2 end of block), bits 8-15 the
//           literal byte or the number of extra bits, bits 16-24 the base match length;
//   offset: bit 4 invalid symbol, bits 8-11 number of extra bits, bits 16-31 base distance;
//   precode: bits 8-12 the symbol.
enum InfKind { kInfLitlen = 0, kInfOffset = 1, kInfPrecode = 2 };

// k_inflate states RFC 1951 in its own text -- the alphabets here, code counts, verdict and ranks in inflate_build,
// the dynamic header in the kernel -- and every statement has to agree with gzpx_deflate.h (length_sym, offset_sym,
// code_shape, code_rank_step, precode_order, fixed_code_len, dyn_header, precode_run, code_lengths_split), which
// k_inflate_seg and the encoders call.  Measured, not preferred: with the shared routines in any of three mixes the
// k_inflate route of the bench stream was 0.4 to 0.9 % slower than with this text, over eight alternations each
// (docs/LAB_NOTES.md, "gzpx_deflate.h"); tests/inflate_cases.py and tests/alphabet_cases.py hold both routes to the same answers.
template <int KIND>
__device__ __forceinline__ uint32_t inflate_entry(uint32_t sym, uint32_t cl) {
    if (KIND == kInfPrecode) return cl | (sym << 8);
    if (KIND == kInfLitlen) {
        if (sym < 256) return cl | (sym << 8);
        if (sym == 256) return cl | (2u << 4);
        const uint32_t slot = sym - 257;
        uint32_t base, xb = 0;
        if (slot < 8) {
            base = 3 + slot;
        } else if (slot >= 28) {  // (286 and 287 too: libdeflate's table decodes them as length 258, like 285)
            base = 258;
        } else {
            xb = (slot - 4) >> 2;
            base = 3 + ((4 + (slot & 3)) << xb);
        }
        return cl | (1u << 4) | (xb << 8) | (base << 16);
    }
    if (sym > 29) return cl | (1u << 4);
    uint32_t base, xb = 0;
    if (sym < 4) {
        base = 1 + sym;
    } else {
        xb = (sym - 2) >> 1;
        base = 1 + ((2 + (sym & 1)) << xb);
    }
    return cl | (xb << 8) | (base << 16);
}

// Build the decode tables of one code from lens[0 .. nsyms): counts, canonical first codes, symbols
// in canonical order, and the direct-lookup table for codes of <= fast_bits bits.  All 64 lanes
// call it.  Returns false for an over-subscribed code and for an incomplete one, with libdeflate's two
// exceptions (build_decode_table): the empty code, in which every bit decodes symbol 0, and a single
// codeword of length 1, which both bit values decode.
// (Not inlined on purpose, and cnt / fst / off indexed by a lane's own code length -- 544 bytes of
// scratch per lane in a part of the kernel that runs once per DEFLATE sub-block.  Measured in round 3:
// with the tables in registers / LDS and the function inlined the kernel has no scratch and 64 VGPRs,
// but the register allocator then spills 130 SGPRs inside the decode loop: 8.35 -> 9.08 ms on the
// bench stream; padded back to five waves per SIMD 9.08; not inlined but without the arrays 10.6.)
template <int KIND>
__device__ bool inflate_build(const uint8_t *lens, uint32_t nsyms, uint32_t fast_bits, uint32_t *fast,
                              uint16_t *sorted, uint32_t *count, uint32_t *first, uint32_t *offs,
                              uint32_t lane) {
    const uint64_t lane_below = (1ull << lane) - 1ull;
    uint32_t cnt[16];
    for (uint32_t l = 0; l < 16; l++) cnt[l] = 0;
    for (uint32_t base = 0; base < nsyms; base += 64) {
        const uint32_t s = base + lane;
        const uint32_t myl = s < nsyms ? lens[s] : 0;
        for (uint32_t l = 1; l <= 15; l++) cnt[l] += (uint32_t)__popcll(__ballot(myl == l));
    }
    uint32_t code = 0, idx = 0, kraft = 0;
    uint32_t fst[16], off[16];
    for (uint32_t l = 1; l <= 15; l++) {
        code <<= 1;
        fst[l] = code;
        off[l] = idx;
        code += cnt[l];
        idx += cnt[l];
        kraft += cnt[l] << (15 - l);
    }
    if (kraft > (1u << 15)) return false;
    if (kraft < (1u << 15)) {
        if (kraft != 0 && (kraft != (1u << 14) || cnt[1] != 1)) return false;
        uint32_t only = 0;  // the one symbol of the code (symbol 0 for the empty code)
        for (uint32_t base = 0; base < nsyms && kraft; base += 64) {
            const uint64_t m = __ballot(base + lane < nsyms && lens[base + lane] == 1);
            if (m) only = base + (uint32_t)__ffsll((long long)m) - 1;
        }
        wave_sync();
        if (lane < 16) count[lane] = 0;  // (every index of the fast table holds the entry: the slow path is never asked)
        const uint32_t e = inflate_entry<KIND>(only, 1);
        for (uint32_t i = lane; i < (1u << fast_bits); i += 64) fast[i] = e;
        wave_sync();
        return true;
    }
    wave_sync();
    if (lane < 16) {
        count[lane] = lane ? cnt[lane] : 0;
        first[lane] = lane ? fst[lane] : 0;
        offs[lane] = lane ? off[lane] : 0;
    }
    for (uint32_t i = lane; i < (1u << fast_bits); i += 64) fast[i] = 0;
    wave_sync();
    uint32_t run[16];
    for (uint32_t l = 0; l < 16; l++) run[l] = 0;
    for (uint32_t base = 0; base < nsyms; base += 64) {
        const uint32_t s = base + lane;
        const uint32_t myl = s < nsyms ? lens[s] : 0;
        uint32_t rank = 0;
        for (uint32_t l = 1; l <= 15; l++) {
            const uint64_t m = __ballot(myl == l);
            if (myl == l) rank = run[l] + (uint32_t)__popcll(m & lane_below);
            run[l] += (uint32_t)__popcll(m);
        }
        if (myl) {
            sorted[off[myl] + rank] = (uint16_t)s;
            if (myl <= fast_bits) {
                const uint32_t cw = __brev(fst[myl] + rank) >> (32 - myl);  // LSB-first codeword
                const uint32_t e = inflate_entry<KIND>(s, myl);
                for (uint32_t k = cw; k < (1u << fast_bits); k += 1u << myl) fast[k] = e;
            }
        }
    }
    wave_sync();
    return true;
}

// A codeword that is not in the fast table: canonical decode from the low bits of `bits` (LSB
// first).  Wave-uniform.  Returns the entry, or 0 when no codeword matches (bad data).
template <int KIND>
__device__ uint32_t inflate_slow(uint32_t bits, const uint16_t *sorted, const uint32_t *count,
                                 const uint32_t *first, const uint32_t *offs) {
    uint32_t code = 0;
    for (uint32_t l = 1; l <= 15; l++) {
        code = (code << 1) | ((bits >> (l - 1)) & 1u);
        const uint32_t c = count[l];
        if (code - first[l] < c) return inflate_entry<KIND>(sorted[offs[l] + code - first[l]], l);
    }
    return 0;
}

struct DBlock {
    uint64_t in_off;    // offset of the block (its gzip header) in the compressed slab
    uint32_t size;      // total block size (header + payload + footer)
    uint32_t isize;     // ISIZE from the footer
    uint32_t crc;       // CRC32 from the footer
    uint32_t status;    // InflateStatus
    uint32_t produced;  // bytes actually inflated
    uint32_t nmatch;    // k_inflate_seg: records in the member's match list (0 after k_inflate)
    uint32_t pay_off;   // where the DEFLATE payload starts inside the member (BGZF 18, Mgzip 20; gzpx_wrap.h: per member)
    uint32_t pay_len;   // its length; the member's bytes behind it (the trailer) are readable, nothing behind the member is
    uint32_t cyc[8];    // debug launches only: shader-clock cycles [0] whole block, [1] headers + table
                        // builds, [2] round set-up (input bits + table gathers), [3] literal stores +
                        // match copies; counts [4] rounds, [5] literals, [6] matches, [7] unused (the LDS ring's flushes)
};

__global__ void k_dinit(uint32_t hdr_len, uint32_t nb, const uint8_t *__restrict__ in, const uint64_t *__restrict__ offsets,
                        const uint32_t *__restrict__ sizes, DBlock *__restrict__ blk, uint32_t *__restrict__ redo) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0 && redo) {
        redo[0] = 0;       // members handed back to k_inflate
        redo[1 + nb] = 0;  // k_inflate_seg's ticket counter
    }
    if (b >= nb) return;
    const uint8_t *f = in + offsets[b] + sizes[b] - 8;  // get_footer_values, src/lib.rs:440-447
    DBlock d;
    d.in_off = offsets[b];
    d.size = sizes[b];
    d.crc = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24);
    d.isize = (uint32_t)f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) | ((uint32_t)f[7] << 24);
    d.status = kInfOk;
    d.produced = 0;
    d.nmatch = 0;
    d.pay_off = hdr_len;
    d.pay_len = sizes[b] - hdr_len - 8;
    for (uint32_t k = 0; k < 8; k++) d.cyc[k] = 0;
    blk[b] = d;
}

__global__ __launch_bounds__(256) void k_dscan(uint32_t nb, const DBlock *__restrict__ blk,
                                               uint64_t *__restrict__ out_off) {
    __shared__ uint64_t wsum[4];
    __shared__ uint64_t carry_s;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += 256) {
        const uint32_t i = base + tid;
        const uint64_t v = i < nb ? blk[i].isize : 0;  // untrusted footers: sums need 64 bits
        uint64_t total;
        const uint64_t ex = block_exclusive_scan256(v, wsum, &total);
        const uint64_t carry = carry_s;
        if (i < nb) out_off[i] = carry + ex;
        __syncthreads();
        if (tid == 0) carry_s = carry + total;
        __syncthreads();
    }
    if (tid == 0) out_off[nb] = carry_s;
}



// The symbol loop works in rounds of 64 bit positions.  Lane i takes the 32 bits that start at bit
// bp + i of the payload and looks them up in BOTH fast tables (two LDS gathers for the whole wave:
// every lane decodes "as if a codeword started here").  The wave-uniform walk then hops from real
// codeword to real codeword reading those per-lane results with v_readlane -- scalar ALU only, no
// memory latency per symbol.  Literals of a round are stored together (one ds_write_b8, each marked
// lane at o + its rank); a match first commits the literals before it, then copies with the wave.
#ifndef GZPX_INF_WAVES
#define GZPX_INF_WAVES 5  // waves per SIMD k_inflate is compiled for (VGPR budget 512 / n)
#endif
// COUNT (gzpx_inflate_batch_sizes_device): the same walk with nothing stored and no match source read -- a DEFLATE
// stream's length does not depend on its window.  isize is the cap on the member's output (kInfInsufficientSpace behind
// it); what the wave leaves is the byte count in DBlock.produced and the payload bytes the stream took, through the byte
// that holds the last bit of the final block, in DBlock.nmatch.  out_off / out_all / out_cap are not read.
template <bool DBG, bool COUNT = false>
__global__ __launch_bounds__(64, GZPX_INF_WAVES) void k_inflate(const uint8_t *__restrict__ in_all, DBlock *__restrict__ blk_all,
                                                                const uint64_t *__restrict__ out_off, uint8_t *out_all,
                                                                uint64_t out_cap, const uint32_t *__restrict__ redo) {
    __shared__ InfLds h;
    const uint32_t lane = threadIdx.x;
    // with a redo list (k_inflate_seg / k_lzcopy): the members on it, which those kernels left for this one
    uint32_t bidx = blockIdx.x;
    if (redo) {
        if (bidx >= redo[0]) return;
        bidx = redo[1 + bidx];
    }
    DBlock *blk = blk_all + bidx;
    const uint32_t isize = blk->isize;
    if (isize == 0) return;  // src/par/decompress.rs:163-171: nothing to decode
    const uint64_t ooff = COUNT ? 0ull : out_off[bidx];
    if (!COUNT && ooff + isize > out_cap) {
        if (lane == 0) blk->status = kInfInsufficientSpace;
        return;
    }
    uint8_t *out = out_all + ooff;  // (COUNT: null, and never used)
    // does output [at, at + add) end behind isize?  (COUNT: the cap may be 0xFFFFFFFF, the sum needs 33 bits)
    auto over = [&](uint32_t at, uint32_t add) -> bool {
        if constexpr (COUNT) return (uint64_t)at + add > isize;
        else return at + add > isize;
    };
    const uint8_t *pay = in_all + blk->in_off + blk->pay_off;
    const uint32_t pay_len = blk->pay_len;
    const long long t_begin = DBG ? clock64() : 0;
    uint32_t dbg[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    // ---- compressed bytes: aligned dwords through an LDS ring, one 256-byte piece prefetched in
    // registers; bit positions count from the aligned dword that holds the first payload byte
    const uint32_t pmis = (uint32_t)((uintptr_t)pay & 3u);
    const uint32_t *pay32 = (const uint32_t *)(pay - pmis);
    // (the member's bytes behind the payload -- a BGZF footer's 8 -- are readable too; nothing behind the member is.
    // A member of no bytes at all never gets here: k_dinit_wrap.)
    const uint32_t pay_words = (pmis + (blk->size - blk->pay_off) + 3) >> 2;
    const uint32_t bit0 = 8u * pmis, bit_end = bit0 + 8u * pay_len;
    uint32_t hi_w = 0;  // dwords [.., hi_w) are in the ring; `pre` holds [hi_w, hi_w + 64)
    // (index clamped to readable memory.)  Bits past the end of the payload read as zeros, the way
    // libdeflate's bit reader pads an exhausted input: a truncated member then fails with the same
    // error class as in the reference (the output overflows, a header turns invalid, or the final
    // end-of-block is "found" inside the padding -- checked after the last block).
    auto fetch = [&](uint32_t w) -> uint32_t {
        uint32_t v = pay32[w < pay_words ? w : pay_words - 1];
        const uint32_t wb = 32u * w;
        if (wb >= bit_end) v = 0;
        else if (bit_end - wb < 32u) v &= (1u << (bit_end - wb)) - 1u;
        return v;
    };
    uint32_t pre = fetch(lane);
    auto ensure = [&](uint32_t bpos) {  // the ring covers dwords (bpos >> 5) .. (bpos >> 5) + 5
        const uint32_t w = bpos >> 5;
        if (w >= hi_w + 64) {  // a jump (after a stored block)
            hi_w = w;
            pre = fetch(hi_w + lane);
        }
        if (w + 6 > hi_w) {
            wave_sync();
            do {
                h.inr[(hi_w + lane) & 255u] = pre;
                hi_w += 64;
                pre = fetch(hi_w + lane);
            } while (w + 6 > hi_w);
            wave_sync();
        }
    };
    auto bits_at = [&](uint32_t bpos) -> uint32_t {  // 32 payload bits from bit position bpos
        const uint32_t w = bpos >> 5;
        const uint32_t lo = h.inr[w & 255u], hi = h.inr[(w + 1) & 255u];
        return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (bpos & 31u));
    };

    uint32_t bp = bit0;
    uint32_t o = 0;        // bytes produced
    uint32_t status = kInfOk;
    // the window: byte `pos` of the block's output, in HBM, where a wave reads its own earlier stores back in
    // program order
    auto win_load = [&](uint32_t pos) -> uint32_t { return (uint32_t)out[pos]; };
    auto win_store = [&](uint32_t pos, uint32_t v) { out[pos] = (uint8_t)v; };
    // one more of the events dbg[k] counts.  (A lambda that holds dbg by reference, as the ring's flush did: with it the
    // instrumented kernel compiles to the instructions its clocks have been read with; the plain one has no dbg.)
    auto tick = [&](uint32_t k) {
        if (DBG) dbg[k]++;
    };

    bool final_block = false;
    while (!final_block && status == kInfOk) {
        bp = uniform(bp);
        o = uniform(o);
        hi_w = uniform(hi_w);
        status = uniform(status);
        if (bp > bit_end) {
            status = kInfBadData;
            break;
        }
        ensure(bp);
        const long long t_hdr = DBG ? clock64() : 0;
        const uint32_t hb = uniform(bits_at(bp));
        final_block = (hb & 1u) != 0;
        const uint32_t btype = (hb >> 1) & 3u;
        bp += 3;
        if (btype == 0) {
            // stored: skip to a byte boundary, LEN, NLEN, raw bytes
            bp = (bp + 7u) & ~7u;
            ensure(bp);
            const uint32_t x = uniform(bits_at(bp));
            const uint32_t len = x & 0xFFFFu, nlen = x >> 16;
            bp += 32;
            if ((len ^ 0xFFFFu) != nlen) {
                status = kInfBadData;
                break;
            }
            const uint32_t src = (bp - bit0) >> 3;  // next unread payload byte
            if (src + len > pay_len) {
                status = kInfBadData;
                break;
            }
            if (over(o, len)) {
                status = kInfInsufficientSpace;
                break;
            }
            if constexpr (COUNT) {
                o += len;
                bp += 8u * len;
                continue;
            }
            // straight from the payload to the output: head bytes up to a dword boundary of the
            // destination, then dwords (the source is read as aligned dword pairs), then the tail
            const uint8_t *sp = pay + src;
            uint8_t *dp = out + o;
            uint32_t head = (uint32_t)((4u - ((uintptr_t)dp & 3u)) & 3u);
            if (head > len) head = len;
            if (lane < head) dp[lane] = sp[lane];
            const uint32_t nw = (len - head) >> 2;
            const uint32_t smis = (uint32_t)((uintptr_t)(sp + head) & 3u);
            const uint32_t *s32 = (const uint32_t *)(sp + head - smis);
            for (uint32_t k = lane; k < nw; k += 64) {
                const uint32_t lo = s32[k], hi = smis ? s32[k + 1] : 0u;  // (hi: inside the member, the footer follows)
                *(uint32_t *)(dp + head + 4 * k) = __builtin_amdgcn_alignbyte(hi, lo, smis);
            }
            const uint32_t donew = head + 4 * nw;
            if (donew + lane < len) dp[donew + lane] = sp[donew + lane];
            o += len;
            bp += 8u * len;
            continue;
        }
        if (btype == 3) {
            status = kInfBadData;
            break;
        }
        // ---- code lengths
        if (btype == 1) {
            for (uint32_t i = lane; i < 320; i += 64)
                h.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
            wave_sync();
        } else {
            const uint32_t nlit = ((hb >> 3) & 31u) + 257, ndist = ((hb >> 8) & 31u) + 1;
            const uint32_t nclen = ((hb >> 13) & 15u) + 4;
            bp += 14;
            if (nlit > 286 + 2 || ndist > 32) {
                status = kInfBadData;
                break;
            }
            // the precode: nclen lengths of 3 bits in a fixed order (one per lane), decoded with a
            // 7-bit table that lives in ofast[0..127] until the real offset table is built
            ensure(bp + 64);
            wave_sync();
            {
                const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                const uint32_t v = bits_at(bp + 3u * (lane < 19 ? lane : 0)) & 7u;
                if (lane < 19) h.lens[order[lane]] = (uint8_t)(lane < nclen ? v : 0u);
            }
            bp += 3u * nclen;
            wave_sync();
            if (!inflate_build<kInfPrecode>(h.lens, 19, 7, h.ofast, h.osorted, h.ocount, h.ofirst, h.ooffs,
                                            lane)) {
                status = kInfBadData;
                break;
            }
            // litlen + offset lengths, run-length coded with the precode (sequential, uniform)
            uint32_t i = 0;
            const uint32_t total = nlit + ndist;
            uint32_t prev = 0;
            uint8_t *tmp = (uint8_t *)h.lfast;  // scratch, free until the litlen table is built
            while (i < total) {
                ensure(bp);
                const uint32_t b = uniform(bits_at(bp));
                const uint32_t e = uniform(h.ofast[b & 127u]);
                const uint32_t cl = e & 15u, sym = e >> 8;
                if (cl == 0) {  // precode words are <= 7 bits: a miss is an unused codeword
                    status = kInfBadData;
                    break;
                }
                uint32_t rep = 1, val = sym, used = cl;
                if (sym == 16) {
                    if (i == 0) {
                        status = kInfBadData;
                        break;
                    }
                    rep = 3 + ((b >> cl) & 3u);
                    used += 2;
                    val = prev;
                } else if (sym == 17) {
                    rep = 3 + ((b >> cl) & 7u);
                    used += 3;
                    val = 0;
                } else if (sym == 18) {
                    rep = 11 + ((b >> cl) & 127u);
                    used += 7;
                    val = 0;
                }
                bp += used;
                // (the last run may overrun the total: libdeflate ignores the excess, and so do the writes here)
                const uint32_t nw = rep < total - i ? rep : total - i;
                if (lane < nw) tmp[i + lane] = (uint8_t)val;  // rep <= 138: up to 3 rounds
                if (lane + 64 < nw) tmp[i + lane + 64] = (uint8_t)val;
                if (lane + 128 < nw) tmp[i + lane + 128] = (uint8_t)val;
                prev = val;
                i += rep;
            }
            if (status != kInfOk) break;
            wave_sync();
            // split into litlen [0,288) and offset [288,320)
            uint8_t mine[5];
            for (uint32_t k = 0; k < 5; k++) {
                const uint32_t s = lane + 64 * k;
                uint32_t v = 0;
                if (s < 288) v = s < nlit ? tmp[s] : 0;
                else if (s < 320) v = (s - 288) < ndist ? tmp[nlit + (s - 288)] : 0;
                mine[k] = (uint8_t)v;
            }
            wave_sync();
            for (uint32_t k = 0; k < 5; k++) h.lens[lane + 64 * k] = mine[k];
            wave_sync();
            // (a code without an end-of-block codeword is not judged: like libdeflate's, the symbol loop below runs
            // until the output is full -- InsufficientSpace -- or the input is spent -- BadData; every symbol takes a bit)
        }
        if (!inflate_build<kInfLitlen>(h.lens, 288, 10, h.lfast, h.lsorted, h.lcount, h.lfirst, h.loffs, lane) ||
            !inflate_build<kInfOffset>(h.lens + 288, 32, 8, h.ofast, h.osorted, h.ocount, h.ofirst, h.ooffs,
                                       lane)) {
            status = kInfBadData;
            break;
        }
        if (DBG) dbg[1] += (uint32_t)(clock64() - t_hdr);
        // ---- symbols, 64 * kInfR bit positions per round
        bool eob = false;
        // A symbol that starts a byte or more past the payload's end is where libdeflate's bit reader
        // gives up (more than sizeof(bitbuf) bytes of padding buffered): BadData.  (libdeflate's own
        // limit depends on when it last refilled; against the v1.10 binary this rule gives the same
        // error class for 99 % of members cut within 80 bytes of their end -- 594 of 600 -- and
        // BadData instead of InsufficientSpace for the rest.)
        const uint32_t bit_lim = bit_end + 8u;
        while (!eob && status == kInfOk) {
            if (bp >= bit_lim) {
                status = kInfBadData;
                break;
            }
            const long long t_round = DBG ? clock64() : 0;
            // (these are wave-uniform by construction; saying so keeps the loop on the scalar unit)
            bp = uniform(bp);
            o = uniform(o);
            hi_w = uniform(hi_w);
            status = uniform(status);
            ensure(bp + 64 * kInfR - 64);
            // (1) every lane decodes the symbols that would start at bits bp + 64 * g + lane
            // (g < kInfR), completely: litlen codeword, extra bits, offset codeword, extra bits
            // (<= 48 of the 64 bits it reads from each position)
            uint32_t le[kInfR], pack2[kInfR], adv[kInfR], outlen[kInfR];
            bool is_match[kInfR];
            uint64_t stop_mask[kInfR];
#pragma unroll
            for (uint32_t hf = 0; hf < kInfR; hf++) {
                const uint32_t q = bp + 64 * hf + lane, qw = q >> 5;
                const uint32_t d0 = h.inr[qw & 255u], d1 = h.inr[(qw + 1) & 255u], d2 = h.inr[(qw + 2) & 255u];
                const uint32_t b_lo = __builtin_amdgcn_alignbit(d1, d0, q & 31u);
                const uint32_t b_hi = __builtin_amdgcn_alignbit(d2, d1, q & 31u);
                le[hf] = h.lfast[b_lo & 1023u];
                const uint32_t cl = le[hf] & 15u, type = (le[hf] >> 4) & 3u, xb = (le[hf] >> 8) & 7u;  // (a literal entry keeps its byte here: masked, unused)
                const bool is_lit = cl != 0 && type == 0;
                const bool is_len = cl != 0 && type == 1;
                const uint32_t used1 = is_len ? cl + xb : 0u;  // <= 20
                const uint32_t b2 = (uint32_t)(((((uint64_t)b_hi) << 32) | b_lo) >> used1);
                uint32_t oe = 0;
                if (is_len) oe = h.ofast[b2 & 255u];
                const uint32_t dcl = oe & 15u, dxb = (oe >> 8) & 15u;
                is_match[hf] = is_len && dcl != 0 && (oe & 16u) == 0;
                const uint32_t mlen = (le[hf] >> 16) + ((b_lo >> cl) & ((1u << xb) - 1u));
                const uint32_t mdist = (oe >> 16) + ((b2 >> dcl) & ((1u << dxb) - 1u));
                pack2[hf] = mdist | (mlen << 16);
                // anything else (end of block, codeword outside the fast tables, invalid symbol)
                // stops the walk: that symbol goes through the one-symbol path below
                adv[hf] = is_lit ? cl : is_match[hf] ? used1 + dcl + dxb : 64u * kInfR;
                outlen[hf] = is_lit ? 1u : is_match[hf] ? mlen : 0u;
                stop_mask[hf] = __ballot(!is_lit && !is_match[hf]);
            }
            // (2) the walk: which positions hold real symbols (wave-uniform, scalar)
            // (a lone wave gets roughly one dependent scalar instruction per ten cycles, so the hop
            // is kept to the bare chain: mark, read the lane, add; the last hop is recovered from
            // the marks afterwards)
            uint64_t started[kInfR];
            uint32_t pos = 0;
#pragma unroll
            for (uint32_t g = 0; g < kInfR; g++) {
                uint64_t marks = 0;
                while (pos < 64 * (g + 1)) {
                    marks |= 1ull << (pos - 64 * g);
                    pos += rdlane(adv[g], pos - 64 * g);
                }
                started[g] = marks;
            }
            uint32_t last = 0;
#pragma unroll
            for (uint32_t g = 0; g < kInfR; g++)
                if (started[g]) last = 64 * g + 63u - (uint32_t)__clzll((long long)started[g]);
            bool hit_stop = false;
#pragma unroll
            for (uint32_t g = 0; g < kInfR; g++) {
                if ((last >> 6) == g && ((stop_mask[g] >> (last & 63u)) & 1ull)) {
                    hit_stop = true;
                    started[g] &= ~(1ull << (last & 63u));
                }
            }
            uint32_t nstarted = 0;
            bool any_started = false;
#pragma unroll
            for (uint32_t g = 0; g < kInfR; g++) {
                any_started = any_started || started[g] != 0;
                if (DBG) nstarted += (uint32_t)__popcll(started[g]);
            }
            if (DBG) {
                dbg[2] += (uint32_t)(clock64() - t_round);
                dbg[4]++;
                dbg[5] += nstarted;
            }
            // (3) output of the started symbols: positions by a prefix sum of their lengths, then
            // 64 output bytes per pass, every lane producing one byte
            if (any_started) {
                const long long t_out = DBG ? clock64() : 0;
                bool mine[kInfR];
                uint32_t opos[kInfR], pack1[kInfR];
                uint32_t tout = 0;
                bool bad_dist = false;
#pragma unroll
                for (uint32_t hf = 0; hf < kInfR; hf++) {
                    mine[hf] = ((started[hf] >> lane) & 1ull) != 0;
                    const uint32_t mylen = mine[hf] ? outlen[hf] : 0u;
                    const uint32_t incl = wave_incl_add(mylen) + tout;
                    opos[hf] = incl - mylen;  // relative to o
                    tout = rdlane(incl, 63);
                    if constexpr (COUNT) bad_dist = bad_dist || (mine[hf] && is_match[hf] && (uint64_t)(pack2[hf] & 0xFFFFu) > (uint64_t)o + opos[hf]);
                    else bad_dist = bad_dist || (mine[hf] && is_match[hf] && (pack2[hf] & 0xFFFFu) > o + opos[hf]);
                    pack1[hf] = opos[hf] | ((le[hf] >> 8 & 0xFFu) << 16) | (is_match[hf] ? 1u << 24 : 0u);
                }
                if (__ballot(bad_dist)) {
                    status = kInfBadData;
                    break;
                }
                if (bp + 64 * kInfR > bit_end || over(o, tout)) {
                    // The last round(s) of a member, or an overflow.  libdeflate's order of events: a
                    // symbol that starts past the limit above is BadData, one that does not fit the
                    // output is InsufficientSpace, and the earlier symbol decides (the bit reader's
                    // check comes first within a symbol).
                    uint32_t first_bad = 0xFFFFFFFFu, first_ovf = 0xFFFFFFFFu;
#pragma unroll
                    for (uint32_t hf = 0; hf < kInfR; hf++) {
                        const uint32_t q = bp + 64 * hf + lane;
                        const uint64_t mb = __ballot(mine[hf] && q >= bit_lim);
                        const uint64_t mo = __ballot(mine[hf] && over(o, opos[hf] + outlen[hf]));
                        if (mb && first_bad == 0xFFFFFFFFu) first_bad = 64 * hf + (uint32_t)__ffsll((long long)mb) - 1;
                        if (mo && first_ovf == 0xFFFFFFFFu) first_ovf = 64 * hf + (uint32_t)__ffsll((long long)mo) - 1;
                    }
                    if (first_bad != 0xFFFFFFFFu || first_ovf != 0xFFFFFFFFu) {
                        status = first_bad <= first_ovf ? kInfBadData : kInfInsufficientSpace;
                        break;
                    }
                }
                if (over(o, tout)) {
                    status = kInfInsufficientSpace;
                    break;
                }
                if constexpr (COUNT) {  // the round's bytes are counted, and that is all there is to them
                    o += tout;
                    tout = 0;
                }
                // A round whose symbols are all literals (nearly every round of an incompressible member: configs[2]'s
                // printable noise is literals of 7-8 bits, ~15 per round) needs no owners, no window and no order:
                // every marked lane stores its byte where the prefix sum put it.
                bool any_match = false;
#pragma unroll
                for (uint32_t g = 0; g < kInfR; g++) any_match = any_match || (mine[g] && is_match[g]);
                if (!COUNT && __ballot(any_match) == 0) {
#pragma unroll
                    for (uint32_t g = 0; g < kInfR; g++)
                        if (mine[g]) out[o + opos[g]] = (uint8_t)(le[g] >> 8);
                    o += tout;
                    if (DBG) dbg[3] += (uint32_t)(clock64() - t_out);
                    if (!hit_stop) {
                        bp += pos;
                        continue;
                    }
                    tout = 0;  // (falls through to the one-symbol path below)
                }
                uint32_t carry = 0;
                for (uint32_t pass = 0; pass < tout; pass += 64) {
                    // owner (position + 1) of every output byte of this pass: scatter the symbol
                    // starts, then a running maximum
                    wave_sync();
                    h.own[lane] = 0;
                    wave_sync();
#pragma unroll
                    for (uint32_t g = 0; g < kInfR; g++)
                        if (mine[g] && opos[g] - pass < 64u) h.own[opos[g] - pass] = 64 * g + lane + 1;
                    wave_sync();
                    uint32_t own = h.own[lane];
                    if (lane == 0 && own < carry) own = carry;
                    own = wave_incl_max(own);
                    carry = rdlane(own, 63);
                    const int from = (int)(((own - 1) & 63u) << 2);
                    uint32_t p1 = 0, p2 = 0;
#pragma unroll
                    for (uint32_t g = 0; g < kInfR; g++) {
                        const uint32_t a1 = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)pack1[g]);
                        const uint32_t a2 = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)pack2[g]);
                        if (((own - 1) >> 6) == g) {
                            p1 = a1;
                            p2 = a2;
                        }
                    }
                    const uint32_t prel = pass + lane;
                    const bool active = prel < tout;
                    const bool m = ((p1 >> 24) & 1u) != 0;
                    const uint32_t sdist = p2 & 0xFFFFu, slen = p2 >> 16;
                    uint32_t r = prel - (p1 & 0xFFFFu);
                    if (m && sdist < slen) {  // overlapping copy: the source repeats with period dist
                        uint32_t rr = r - (uint32_t)((float)r * (1.0f / (float)sdist)) * sdist;
                        if ((int32_t)rr < 0) rr += sdist;
                        if (rr >= sdist) rr -= sdist;
                        r = rr;
                    }
                    const uint32_t srcrel = (p1 & 0xFFFFu) - sdist + r;  // relative to o; "negative" = older
                    uint64_t done = __ballot(!active);
                    bool pending = active;
                    // sources older than this pass come from HBM (one gather for all of them, issued
                    // before the loop); sources inside the pass are handed over between lanes
                    const bool in_pass = m && (int32_t)(srcrel - pass) >= 0;
                    uint32_t myv = (p1 >> 16) & 0xFFu;  // the literal
                    if (active && m && !in_pass) myv = out[o + srcrel];
                    bool have = active && (!m || !in_pass);
                    if (have) out[o + prel] = (uint8_t)myv;
                    done |= __ballot(have);
                    pending = pending && !have;
                    while (__ballot(pending) != 0) {
                        const uint32_t sl = (srcrel - pass) & 63u;
                        const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(sl << 2), (int)myv);
                        const bool ready = pending && ((done >> sl) & 1ull) != 0;
                        if (ready) {
                            myv = got;
                            out[o + prel] = (uint8_t)myv;
                        }
                        done |= __ballot(ready);
                        pending = pending && !ready;
                        tick(6);
                    }
                }
                o += tout;
                if (DBG) dbg[3] += (uint32_t)(clock64() - t_out);
            }
            if (!hit_stop) {
                bp += pos;
                continue;
            }
            // (4) one symbol the slow way: end of block, long codewords, errors
            bp += last;
            if (bp >= bit_lim) {
                status = kInfBadData;
                break;
            }
            ensure(bp);
            const uint32_t sw = bp >> 5;
            const uint32_t s0 = h.inr[sw & 255u], s1 = h.inr[(sw + 1) & 255u], s2 = h.inr[(sw + 2) & 255u];
            const uint32_t sb_lo = uniform(__builtin_amdgcn_alignbit(s1, s0, bp & 31u));
            const uint32_t sb_hi = uniform(__builtin_amdgcn_alignbit(s2, s1, bp & 31u));
            uint32_t e = uniform(h.lfast[sb_lo & 1023u]);
            if ((e & 15u) == 0) {
                e = uniform(inflate_slow<kInfLitlen>(sb_lo, h.lsorted, h.lcount, h.lfirst, h.loffs));
                if (e == 0) {
                    status = kInfBadData;
                    break;
                }
            }
            const uint32_t stype = (e >> 4) & 3u, scl = e & 15u;
            if (stype == 2) {
                bp += scl;
                eob = true;
                break;
            }
            if (stype == 0) {
                if (o >= isize) {
                    status = kInfInsufficientSpace;
                    break;
                }
                if constexpr (!COUNT) {
                    wave_sync();
                    if (lane == 0) win_store(o, e >> 8);
                    wave_sync();
                }
                o++;
                bp += scl;
                continue;
            }
            const uint32_t sxb = (e >> 8) & 7u;
            const uint32_t len = (e >> 16) + ((sb_lo >> scl) & ((1u << sxb) - 1u));
            const uint32_t sb2 = (uint32_t)(((((uint64_t)sb_hi) << 32) | sb_lo) >> (scl + sxb));
            uint32_t d = uniform(h.ofast[sb2 & 255u]);
            if ((d & 15u) == 0) {
                d = uniform(inflate_slow<kInfOffset>(sb2, h.osorted, h.ocount, h.ofirst, h.ooffs));
                if (d == 0) {
                    status = kInfBadData;
                    break;
                }
            }
            if (d & 16u) {
                status = kInfBadData;
                break;
            }
            const uint32_t sdcl = d & 15u, sdxb = (d >> 8) & 15u;
            const uint32_t dist = (d >> 16) + ((sb2 >> sdcl) & ((1u << sdxb) - 1u));
            bp += scl + sxb + sdcl + sdxb;
            if (dist > o) {
                status = kInfBadData;
                break;
            }
            if (over(o, len)) {
                status = kInfInsufficientSpace;
                break;
            }
            if constexpr (COUNT) {
                o += len;
                continue;
            }
            // out[o + i] = out[o - dist + (i mod dist)]: every source byte is older than o
            wave_sync();
            const uint32_t src0 = o - dist;
            const float rcp = 1.0f / (float)dist;
            for (uint32_t base = 0; base < len; base += 64) {
                const uint32_t i = base + lane;
                uint32_t r = i;
                if (dist < len) {
                    r = i - (uint32_t)((float)i * rcp) * dist;  // i mod dist (i < 320)
                    if ((int32_t)r < 0) r += dist;
                    if (r >= dist) r -= dist;
                }
                const uint32_t v = win_load(src0 + (i < len ? r : 0u));
                wave_sync();
                if (i < len) win_store(o + i, v);
            }
            o += len;
            wave_sync();
        }
    }
    // libdeflate's final check (overread_count > bitsleft / 8): the stream "ended" inside the zero
    // padding behind a truncated payload -> BadData
    if (status == kInfOk && bp > bit_end) status = kInfBadData;
    if constexpr (!COUNT) {
        if (status == kInfOk && o != isize) status = kInfShortOutput;
        // libdeflater hands back a zero-initialised Vec of orig_size bytes: a short block stays zero
        for (uint32_t i = o + lane; i < isize; i += 64) out[i] = 0;
    }
    if (lane == 0) {
        blk->status = status;
        blk->produced = o;
        blk->nmatch = COUNT ? (bp - bit0 + 7u) >> 3 : 0u;
        if (DBG) {
            dbg[0] = (uint32_t)(clock64() - t_begin);
            for (uint32_t k = 0; k < 8; k++) blk->cyc[k] = dbg[k];
        }
    }
}

#include "gzpx_inflate_seg.h"
#include "gzpx_snap.h"
#include "gzpx_mscan.h"
#include "gzpx_ranges.h"
#include "gzpx_lines.h"
#include "gzpx_find.h"
#include "gzpx_select.h"
#include "gzpx_fields.h"
#include "gzpx_columns.h"
#include "gzpx_where.h"
#include "gzpx_findset.h"
#include "gzpx_wrap.h"
#include "gzpx_cksum.h"

// CRC-32 of the inflated blocks (LibDeflateCrc over the whole orig_size buffer, src/check.rs:45-71):
// crc32_workgroup, blocks addressed through their output offsets.
__global__ __launch_bounds__(kCrcThreads, 8) void k_dcrc32(const uint8_t *__restrict__ out_all,
                                                const uint64_t *__restrict__ out_off,
                                                const DBlock *__restrict__ blk_all,
                                                uint32_t *__restrict__ crc_found, CrcConsts cc) {
    __shared__ CrcWgLds l;
    const uint32_t b = blockIdx.x;
    if (blk_all[b].nmatch & 0x80000000u) return;  // (kLcCrcDone: k_lzcopy took the member's CRC from its tiles in LDS)
    const uint32_t total = crc32_workgroup(l, out_all + out_off[b], blk_all[b].isize, cc, threadIdx.x);
    if (threadIdx.x == 0) crc_found[b] = total;
}

// What the host wants to know of a launch: the first failing member in stream order (src/par/decompress.rs:162-186),
// once under the framed rule (a member that inflates to fewer bytes than its footer says is BadData) and once under
// the libdeflate-shaped call's (fewer bytes are accepted), with its status and the two checksums -- 48 bytes instead
// of a record per member (kDs*, gzpx_device.h).
__global__ __launch_bounds__(256) void k_dsummary(uint32_t nb, const DBlock *__restrict__ blk, const uint32_t *__restrict__ crc_found,
                                                  uint32_t *__restrict__ sum) {
    static_assert(kDsStrict == 0 && kDsLenient == 4, "thread 0 writes the strict quadruple, thread 1 the lenient one");
    __shared__ uint32_t first[2];
    const uint32_t tid = threadIdx.x;
    if (tid < 2) first[tid] = 0xFFFFFFFFu;
    __syncthreads();
    for (uint32_t b = tid; b < nb; b += 256) {
        const uint32_t st = blk[b].status;
        const bool crc_bad = crc_found[b] != blk[b].crc;
        if (st != kInfOk || crc_bad) atomicMin(&first[0], b);
        if (st == kInfBadData || st == kInfInsufficientSpace || crc_bad) atomicMin(&first[1], b);
    }
    __syncthreads();
    if (tid < 2) {
        const uint32_t b = first[tid];
        uint32_t *q = sum + kDsLenient * tid;
        q[kDsFirst] = b;
        q[kDsStatus] = b != 0xFFFFFFFFu ? blk[b].status : 0u;
        q[kDsFound] = b != 0xFFFFFFFFu ? crc_found[b] : 0u;
        q[kDsExpected] = b != 0xFFFFFFFFu ? blk[b].crc : 0u;
    }
    if (tid == 0) sum[kDsProduced0] = nb ? blk[0].produced : 0u;
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
void launch_init_meta(const Config &cfg, uint64_t slab_len, uint32_t nb, int is_last,
                      const Scratch &s, hipStream_t stream) {
    hipLaunchKernelGGL(k_init_meta, dim3((nb + 255) / 256), dim3(256), 0, stream, cfg, slab_len, nb,
                       (uint32_t)(is_last ? 1 : 0), s.meta, s.redo);
}

template <int MODE>
static void launch_candidates_mode(const Config &cfg, const uint8_t *slab, uint64_t slab_len, uint32_t nb,
                                   int is_last, const Scratch &s, uint16_t *out, hipStream_t stream) {
    // one workgroup per CU (more only if a workgroup's positions, counted on through its blocks, could pass 2^30)
    uint64_t wgs = cfg.n_cu ? cfg.n_cu : 256u;
    const uint64_t span = slab_len + (uint64_t)nb * 32768u;
    if (span / wgs >= (1ull << 30)) wgs = span / (1ull << 30) + 1;
    hipLaunchKernelGGL(k_candidates<MODE>, dim3((uint32_t)(nb < wgs ? nb : wgs)), dim3(64 * kCandWaves), 0, stream, cfg,
                       slab, s.meta, out, slab_len, nb, (uint32_t)(is_last ? 1 : 0), s.redo, s.claim);
}

// Levels >= 1: the first launch also fills BlockMeta (k_init_meta's work); level 0 has no matchfinding and
// goes through launch_init_meta alone.
void launch_candidates(const Config &cfg, const uint8_t *slab, uint64_t slab_len, uint32_t nb, int is_last,
                       const Scratch &s, hipStream_t stream) {
    if (cfg.level == 0 || cfg.level >= 10) {  // stored blocks only / bt_matchfinder (gzpx_nearopt.hip) keeps its own tables
        launch_init_meta(cfg, slab_len, nb, is_last, s, stream);
        return;
    }
    if (cfg.level == 1) {
        launch_candidates_mode<0>(cfg, slab, slab_len, nb, is_last, s, s.cand, stream);
    } else {  // hc_matchfinder: hash3 predecessor in cand, hash4 chain links in d4
        launch_candidates_mode<1>(cfg, slab, slab_len, nb, is_last, s, s.cand, stream);
        launch_candidates_mode<2>(cfg, slab, slab_len, nb, is_last, s, s.d4, stream);
        launch_candidates_mode<3>(cfg, slab, slab_len, nb, is_last, s, s.d4, stream);
    }
}

// Level 1.  Blocks of at most one tile (every BGZF block): k_mparse, match on demand, and the dense
// pair k_match / k_parse over the blocks it handed back (normally none: two small launches that
// find an empty list).  Larger blocks, or Config.debug bit 1: the dense pair over every block.
bool level1_fused(const Config &cfg) { return cfg.block_size <= kTile && !(cfg.debug & 2u); }

#ifdef GZPX_EXPERIMENT
// the column sums of one of the 1024 x 8 counter tables, which is cleared afterwards if `reset`
static int exp_read(const void *symbol, unsigned long long out[8], int reset) {
    static unsigned long long rows[1024 * 8];
    if (hipMemcpyFromSymbol(rows, symbol, sizeof(rows)) != hipSuccess) return -1;
    for (int k = 0; k < 8; k++) out[k] = 0;
    for (int r = 0; r < 1024; r++)
        for (int k = 0; k < 8; k++) out[k] += rows[r * 8 + k];
    if (reset) {
        memset(rows, 0, sizeof(rows));
        if (hipMemcpyToSymbol(symbol, rows, sizeof(rows)) != hipSuccess) return -1;
    }
    return 0;
}
extern "C" int gzpx_exp_huff(unsigned long long out[8], int reset) { return exp_read(HIP_SYMBOL(g_exp_huff), out, reset); }
extern "C" int gzpx_exp_cycles(unsigned long long out[8], int reset) { return exp_read(HIP_SYMBOL(g_exp_cycles), out, reset); }
extern "C" int gzpx_exp_sparse(unsigned long long out[8], int reset) { return exp_read(HIP_SYMBOL(g_exp_sparse), out, reset); }
#endif

void launch_match(const Config &cfg, const uint8_t *slab, uint64_t slab_len, uint32_t nb, const Scratch &s,
                  hipStream_t stream) {
    const bool fused = level1_fused(cfg);
    if (fused) {  // (the batch's first k_candidates launch has emptied the redo list)
        const uint32_t wgs = cfg.n_cu ? cfg.n_cu : 256u;  // one per CU, each walking its share of the blocks
        hipLaunchKernelGGL(k_mparse, dim3(nb < wgs ? nb : wgs), dim3(kMpThreads), 0, stream, cfg, slab, s.meta, s.sub,
                           (const uint16_t *)s.cand, s.tok, s.redo, slab_len, nb, s.claim + 0);
    }
    const uint32_t grid = fused ? (nb < 512u ? nb : 512u) : nb;
    hipLaunchKernelGGL(k_match, dim3(grid), dim3(kMpThreads), 0, stream, cfg, slab, s.meta,
                       (const uint16_t *)s.cand, s.len8, s.which, s.alt, nb,
                       fused ? (const uint32_t *)s.redo : (const uint32_t *)nullptr);
}

void launch_parse(const Config &cfg, const uint8_t *slab, uint64_t, uint32_t nb, const Scratch &s,
                  hipStream_t stream) {
    const bool fused = level1_fused(cfg);
    const uint32_t grid = fused ? (nb < 512u ? nb : 512u) : nb;
    hipLaunchKernelGGL(k_parse, dim3(grid), dim3(kMpThreads), 0, stream, cfg, slab, s.meta, s.sub,
                       (const uint8_t *)s.len8, (const uint32_t *)s.which, (const uint16_t *)s.alt, s.tok, nb,
                       fused ? (const uint32_t *)s.redo : (const uint32_t *)nullptr);
}

// levels 2-4: every match once (it does not depend on a sub-block's min_len, see k_match_hc), then the
// greedy parse with its re-parse rounds: nothing comes back to the host
void launch_hc(const Config &cfg, const uint8_t *slab, uint32_t nb, const Scratch &s, hipStream_t stream) {
    hipLaunchKernelGGL(k_hc_init, dim3((nb + 255) / 256), dim3(256), 0, stream, nb, s.hc, s.pending);
    auto dense = [&]() {  // (returns at once for the blocks whose arrays already hold what the parse needs)
        hipLaunchKernelGGL(k_match_hc, dim3(nb), dim3(1024), 0, stream, cfg, slab, (const BlockMeta *)s.meta, s.hc,
                           (const uint16_t *)s.cand, (const uint16_t *)s.d4, s.len8, s.which, s.alt,
                           (uint8_t *)nullptr, (uint16_t *)nullptr);
    };
    auto parse_round = [&](uint32_t may_list_stale) {
        hipLaunchKernelGGL(k_parse_hc<false>, dim3(nb), dim3(kMpThreads), 0, stream, cfg, slab, s.meta, s.sub, s.hc,
                           (const uint8_t *)s.len8, (const uint32_t *)s.which, (const uint16_t *)s.alt, s.tok,
                           s.pending, s.redo, may_list_stale);
    };
    // Round 5: the full search only where the greedy parse starts a token (k_match_hc_sparse).  Config.debug bit 4: the
    // dense kernel for every block, as in rounds 2-4 (A/B runs and the tests that compare the two routes).
    // Level 2 (six chain nodes at most) is the dense kernel's: there is too little behind the first node to compact.
    // (Config.debug bit 5: the sparse kernel at every greedy level and for every block, noise included -- tests.)
    const bool sparse = !(cfg.debug & 16u) && (cfg.level >= 3 || (cfg.debug & 32u));
    if (sparse)  // (searches the blocks it does not compact -- noise, orphan candidates -- the dense way itself)
        hipLaunchKernelGGL(k_match_hc_sparse, dim3(nb), dim3(1024), 0, stream, cfg, slab, (const BlockMeta *)s.meta, s.hc,
                           (const uint16_t *)s.cand, (const uint16_t *)s.d4, s.len8, s.which, s.alt);
    else
        dense();
    hipLaunchKernelGGL(k_hc_orphan, dim3(nb), dim3(64), 0, stream, cfg, slab, (const BlockMeta *)s.meta, s.hc,
                       (const uint16_t *)s.cand, (const uint16_t *)s.d4, s.len8, s.which, s.alt, (uint8_t *)nullptr,
                       (uint16_t *)nullptr);
    // two single rounds (the second finds nearly every block done), then the looping form for the rest.  A block whose
    // first round ended at a sub-block with another min_len has arrays that are no use from there on if they came from
    // the sparse kernel (kHcArraysStale): the dense kernel goes over it before its second round.
    parse_round(1u);
    if (sparse) {  // (the list of stale blocks is Scratch.redo: zeroed by the batch's first k_candidates launch, filled by the round above)
        const uint32_t wgs = cfg.n_cu ? cfg.n_cu : 256u;
        hipLaunchKernelGGL(k_match_hc_stale, dim3(wgs), dim3(1024), 0, stream, cfg, slab, (const BlockMeta *)s.meta,
                           s.hc, (const uint16_t *)s.cand, (const uint16_t *)s.d4, s.len8, s.which, s.alt,
                           (const uint32_t *)s.redo);
    }
    parse_round(0u);
    hipLaunchKernelGGL(k_parse_hc<true>, dim3(nb), dim3(kMpThreads), 0, stream, cfg, slab, s.meta, s.sub, s.hc,
                       (const uint8_t *)s.len8, (const uint32_t *)s.which, (const uint16_t *)s.alt, s.tok,
                       s.pending, s.redo, 0u);
}

void launch_lazy(const Config &cfg, const uint8_t *slab, uint32_t nb, const Scratch &s, hipStream_t stream) {
    hipLaunchKernelGGL(k_hc_init, dim3((nb + 255) / 256), dim3(256), 0, stream, nb, s.hc, s.pending);
    hipLaunchKernelGGL(k_match_hc, dim3(nb), dim3(1024), 0, stream, cfg, slab, (const BlockMeta *)s.meta, s.hc,
                       (const uint16_t *)s.cand, (const uint16_t *)s.d4, s.len8, s.which, s.alt, s.lz_len,
                       s.lz_dist);
    hipLaunchKernelGGL(k_hc_orphan, dim3(nb), dim3(64), 0, stream, cfg, slab, (const BlockMeta *)s.meta, s.hc,
                       (const uint16_t *)s.cand, (const uint16_t *)s.d4, s.len8, s.which, s.alt, s.lz_len, s.lz_dist);
    if (cfg.lazy >= 2)
        hipLaunchKernelGGL(k_parse_lazy<3>, dim3(nb), dim3(64), 0, stream, cfg, slab, s.meta, s.sub,
                           (const uint8_t *)s.len8, (const uint16_t *)s.alt, (const uint8_t *)s.lz_len,
                           (const uint16_t *)s.lz_dist, s.tok);
    else
        hipLaunchKernelGGL(k_parse_lazy<2>, dim3(nb), dim3(64), 0, stream, cfg, slab, s.meta, s.sub,
                           (const uint8_t *)s.len8, (const uint16_t *)s.alt, (const uint8_t *)s.lz_len,
                           (const uint16_t *)s.lz_dist, s.tok);
}

void launch_hist(const Config &cfg, uint32_t nb, const Scratch &s, hipStream_t stream) {
    hipLaunchKernelGGL(k_hist, dim3(nb), dim3(256), 0, stream, cfg, (const BlockMeta *)s.meta,
                       (const SubMeta *)s.sub, (const uint32_t *)s.tok, s.hist);
}

void launch_huffman(const Config &cfg, uint32_t nb, const Scratch &s, hipStream_t stream) {
    hipLaunchKernelGGL(k_huffman, dim3(nb), dim3(64), 0, stream, cfg, s.meta, s.sub,
                       (const uint32_t *)s.hist, s.codes, s.hdr);
}

void launch_crc32(const Config &cfg, const uint8_t *slab, uint64_t, uint32_t nb, const Scratch &s,
                  const CrcConsts &cc, hipStream_t stream) {
    hipLaunchKernelGGL(k_crc32, dim3(nb), dim3(kCrcSmall), 0, stream, cfg, slab, s.meta, cc);
}

void launch_scan(uint32_t nb, const Scratch &s, const SlabResult *prev, SlabResult *result, hipStream_t stream) {
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanThreads), 0, stream, nb, (const BlockMeta *)s.meta,
                       s.out_off, s.sizes, prev, result);
}

void launch_emit(const Config &cfg, const uint8_t *slab, uint64_t, uint32_t nb, const Scratch &s,
                 uint8_t *out, uint64_t out_cap, hipStream_t stream) {
    hipLaunchKernelGGL(k_emit, dim3(nb), dim3(kEmitThreads), 0, stream, cfg, slab, (const BlockMeta *)s.meta,
                       (const SubMeta *)s.sub, (const uint32_t *)s.tok, (const uint32_t *)s.codes,
                       (const uint32_t *)s.hdr, (const uint64_t *)s.out_off, out, out_cap, nb);
}

// How k_inflate_seg goes over nb members, in both of its forms: the waves per member, the grid, the hint word
struct SegLaunch {
    bool big;        // Mgzip-sized members: kSegBigW waves each
    uint32_t grid;   // nb, or the resident workgroups if that is fewer
    uint32_t *hint;
};
static SegLaunch seg_launch_of(const InflateScratch &sc, uint32_t nb) {
    const bool big = nb && sc.in_bytes / nb >= kSegBigBytes;
    const uint32_t wgs = (uint32_t)(sc.n_cu > 0 ? sc.n_cu : 256) * 4u * GZPX_SEG_WAVES / (big ? (uint32_t)kSegBigW : (uint32_t)kSegSmallW);
    return {big, nb < wgs ? nb : wgs, sc.summary ? sc.summary + kDsSegHint : nullptr};
}

// The decode of l.nb members whose records are in place (k_dinit + k_dscan, k_dinit_wrap + k_dscan_slots, or
// k_dinit_wrap_sizes): k_inflate_seg + k_lzcopy + k_inflate over the redo list, or k_inflate for every member.  The
// first three template arguments say which of the three kernels carries its clocks.  COUNT: the count-only forms of
// the inflate kernels (gzpx_inflate_batch_sizes_device) -- nothing but the compressed bytes is read, and nothing written
// but the records: the launch has no output, and the match list, the tile table and k_lzcopy have no part in it
// (sc.mlist / sc.tfirst are not looked at).
template <bool SEG_DBG, bool LC_DBG, bool INF_DBG, bool COUNT>
static void launch_inflate_members_as(const InflateLaunch &l, DBlock *blk, bool seg) {
    const InflateScratch &sc = *l.sc;
    const uint64_t *out_off = l.d_out_off;
    hipStream_t stream = l.stream;
    if (!seg) {
        hipLaunchKernelGGL((k_inflate<INF_DBG, COUNT>), dim3(l.nb), dim3(64), 0, stream, l.d_in, blk, out_off, l.d_out, l.out_cap,
                           (const uint32_t *)nullptr);
        return;
    }
    // decode (literals + match records), LZ copy, then k_inflate over whatever the two left on the redo list
    LzMatch *ml = COUNT ? nullptr : (LzMatch *)sc.mlist;
    uint32_t *tfirst = COUNT ? nullptr : sc.tfirst;
    const SegLaunch sl = seg_launch_of(sc, l.nb);
    if (sl.big)
        hipLaunchKernelGGL((k_inflate_seg<SEG_DBG, kSegBigW, COUNT>), dim3(sl.grid), dim3(64 * kSegBigW), 0, stream, l.d_in, blk,
                           out_off, l.d_out, l.out_cap, ml, tfirst, sc.redo, l.nb, sl.hint);
    else
        hipLaunchKernelGGL((k_inflate_seg<SEG_DBG, kSegSmallW, COUNT>), dim3(sl.grid), dim3(64 * kSegSmallW), 0, stream, l.d_in, blk,
                           out_off, l.d_out, l.out_cap, ml, tfirst, sc.redo, l.nb, sl.hint);
    if (l.ev_mid) (void)hipEventRecord(l.ev_mid, stream);
    if (SEG_DBG || LC_DBG)  // (a debug launch: why each member was handed back, InflateHandback)
        hipLaunchKernelGGL(k_seg_reasons, dim3((l.nb + 255) / 256), dim3(256), 0, stream, (const DBlock *)blk, sc.redo, l.nb,
                           SEG_DBG ? 1u : 0u);
    if (!COUNT)
        hipLaunchKernelGGL((k_lzcopy<LC_DBG>), dim3(l.nb), dim3(kLcThreads), 0, stream, blk, out_off, l.d_out,
                           (const LzMatch *)ml, (const uint32_t *)tfirst, sc.redo, l.d_check, *l.cc);
    hipLaunchKernelGGL((k_inflate<INF_DBG, COUNT>), dim3(l.nb), dim3(64), 0, stream, l.d_in, blk, out_off, l.d_out, l.out_cap,
                       (const uint32_t *)sc.redo);
}

// debug 1: k_inflate_seg's and k_inflate's clocks; 2: k_lzcopy's instead.  The k_inflate route has one kernel to
// instrument and does so for any non-zero value, and so does the count form, which has no k_lzcopy.
static void launch_inflate_members(const InflateLaunch &l, DBlock *blk, bool seg, bool count) {
    if (count && l.debug)
        launch_inflate_members_as<true, false, true, true>(l, blk, seg);
    else if (count)
        launch_inflate_members_as<false, false, false, true>(l, blk, seg);
    else if (l.debug == 1 || (l.debug && !seg))
        launch_inflate_members_as<true, false, true, false>(l, blk, seg);
    else if (l.debug == 2)
        launch_inflate_members_as<false, true, false, false>(l, blk, seg);
    else
        launch_inflate_members_as<false, false, false, false>(l, blk, seg);
}

void launch_inflate(const InflateLaunch &l, uint32_t hdr_len, const uint64_t *d_offsets, const uint32_t *d_sizes) {
    static_assert(sizeof(DBlock) == sizeof(DBlockHost), "the host allocates and reads the records as DBlockHost");
    const InflateScratch &sc = *l.sc;
    DBlock *blk = (DBlock *)l.d_blk;
    const bool seg = l.route != kInflateRouteWave && sc.mlist && sc.tfirst && sc.redo;
    hipLaunchKernelGGL(k_dinit, dim3((l.nb + 255) / 256), dim3(256), 0, l.stream, hdr_len, l.nb, l.d_in, d_offsets, d_sizes, blk,
                       seg ? sc.redo : (uint32_t *)nullptr);
    hipLaunchKernelGGL(k_dscan, dim3(1), dim3(256), 0, l.stream, l.nb, (const DBlock *)blk, l.d_out_off);
    if (l.ev_begin) (void)hipEventRecord(l.ev_begin, l.stream);
    launch_inflate_members(l, blk, seg, false);
    if (l.ev_end) (void)hipEventRecord(l.ev_end, l.stream);
    hipLaunchKernelGGL(k_dcrc32, dim3(l.nb), dim3(kCrcThreads), 0, l.stream, (const uint8_t *)l.d_out,
                       (const uint64_t *)l.d_out_off, (const DBlock *)blk, l.d_check, *l.cc);
    if (sc.summary)
        hipLaunchKernelGGL(k_dsummary, dim3(1), dim3(256), 0, l.stream, l.nb, (const DBlock *)blk, (const uint32_t *)l.d_check,
                           sc.summary);
}

// A batch of members in a wrapper (gzpx_wrap.h).  Everything is read from and written to device memory; what the host
// reads afterwards is k_dresult's record in sc.summary.  `d_slot` is scratch of nb words.
void launch_inflate_batch(const InflateLaunch &l, int wrap, int short_ok, uint64_t in_len, const uint64_t *d_offsets,
                          const uint32_t *d_sizes, const uint32_t *d_out_sizes, uint32_t *d_slot, uint64_t *d_user_off,
                          void *d_results) {
    const InflateScratch &sc = *l.sc;
    DBlock *blk = (DBlock *)l.d_blk;
    // (fewer bytes than the slot are k_inflate's to see: k_inflate_seg hands such a member over anyway)
    const bool seg = l.route != kInflateRouteWave && !short_ok && sc.mlist && sc.tfirst && sc.redo;
    WrapTable t{l.d_in, in_len, d_offsets, d_sizes, d_out_sizes, (uint32_t)wrap};
    hipLaunchKernelGGL(k_dinit_wrap, dim3((l.nb + 255) / 256), dim3(256), 0, l.stream, l.nb, t, blk, d_slot,
                       seg ? sc.redo : (uint32_t *)nullptr);
    hipLaunchKernelGGL(k_dscan_slots, dim3(1), dim3(256), 0, l.stream, l.nb, (const uint32_t *)d_slot, blk, l.out_cap,
                       l.d_out_off);
    if (l.ev_begin) (void)hipEventRecord(l.ev_begin, l.stream);
    launch_inflate_members(l, blk, seg, false);
    if (l.ev_end) (void)hipEventRecord(l.ev_end, l.stream);
    if (wrap == kWrapGzip)
        hipLaunchKernelGGL(k_dcrc32, dim3(l.nb), dim3(kCrcThreads), 0, l.stream, (const uint8_t *)l.d_out,
                           (const uint64_t *)l.d_out_off, (const DBlock *)blk, l.d_check, *l.cc);
    else if (wrap == kWrapZlib)
        hipLaunchKernelGGL(k_dadler32, dim3(l.nb), dim3(kAdlerThreads), 0, l.stream, (const uint8_t *)l.d_out,
                           (const uint64_t *)l.d_out_off, (const DBlock *)blk, l.d_check);
    if (l.ev_check) (void)hipEventRecord(l.ev_check, l.stream);
    hipLaunchKernelGGL(k_dresult, dim3(1), dim3(256), 0, l.stream, l.nb, (uint32_t)wrap, (uint32_t)(short_ok ? 1 : 0),
                       (const DBlock *)blk, (const uint32_t *)d_slot, (const uint32_t *)l.d_check, (const uint64_t *)l.d_out_off,
                       (WrapResult *)d_results, d_user_off, sc.summary);
}

// The sizes of a batch of members (gzpx_inflate_batch_sizes_device): the count form of launch_inflate_members between
// k_dinit_wrap_sizes and k_dresult_sizes; the caller's tables are all that is written.
void launch_inflate_sizes(const InflateLaunch &l, int wrap, uint64_t in_len, const uint64_t *d_offsets, const uint32_t *d_sizes,
                          uint32_t max_out, uint32_t *d_out_sizes, uint32_t *d_in_used, void *d_results) {
    const InflateScratch &sc = *l.sc;
    DBlock *blk = (DBlock *)l.d_blk;
    const bool seg = l.route != kInflateRouteWave && sc.redo;
    WrapTable t{l.d_in, in_len, d_offsets, d_sizes, nullptr, (uint32_t)wrap};
    hipLaunchKernelGGL(k_dinit_wrap_sizes, dim3((l.nb + 255) / 256), dim3(256), 0, l.stream, l.nb, t,
                       max_out ? max_out : 0xFFFFFFFFu, blk, seg ? sc.redo : (uint32_t *)nullptr);
    if (l.ev_begin) (void)hipEventRecord(l.ev_begin, l.stream);
    launch_inflate_members(l, blk, seg, true);
    if (l.ev_end) (void)hipEventRecord(l.ev_end, l.stream);
    hipLaunchKernelGGL(k_dresult_sizes, dim3(1), dim3(256), 0, l.stream, l.nb, (uint32_t)wrap, (const DBlock *)blk, d_out_sizes,
                       d_in_used, (WrapResult *)d_results, sc.summary);
}

// gzpx_adler32: (s1, s2, n) of every 64 KiB tile of d_in[0..n) -> d_out3[3 * tile + ..]
void launch_adler32(const uint8_t *d_in, uint64_t n, uint32_t *d_out3, hipStream_t stream) {
    const uint32_t tiles = (uint32_t)((n + kAdlerTile - 1) / kAdlerTile);
    if (tiles) hipLaunchKernelGGL(k_adler32_tiles, dim3(tiles), dim3(kAdlerThreads), 0, stream, d_in, n, d_out3);
}

// Checksums of a table of buffers (gzpx_cksum.h): plan, tiles, finish, record, with no host round trip between them --
// the persistent launch is sized by the device (or by `width`, for tests), the number of tiles is read on the device.
uint32_t cksum_workgroups(int n_cu, uint32_t width) { return width ? width : (uint32_t)(n_cu > 0 ? n_cu : 256) * kCkWgPerCu; }

void launch_cksum_batch(int kind, const uint8_t *d_in, uint64_t in_len, const uint64_t *d_offsets, const uint32_t *d_sizes,
                        uint32_t n, const uint32_t *d_seeds, const uint32_t *d_expected, uint32_t *d_sums, void *d_results,
                        const CksumScratch &s, uint32_t workgroups, hipStream_t stream) {
    static const CrcPow pw_crc32 = crc_pow_table<kCrcPoly32>(), pw_crc32c = crc_pow_table<kCrcPoly32c>();
    const CkTable t{d_in, in_len, d_offsets, d_sizes, n};
    const CkOut o{d_seeds, d_expected, d_sums, (WrapResult *)d_results};
    hipLaunchKernelGGL(k_cksum_plan, dim3(1), dim3(kCkPlanThreads), 0, stream, t, s.prefix, s.rec);
    if (kind == (int)kCkAdler32)
        hipLaunchKernelGGL((k_cksum_tiles<kCkAdler32>), dim3(workgroups), dim3(kCkThreads), 0, stream, t, d_seeds,
                           (const uint64_t *)s.prefix, s.part, s.carry, pw_crc32);
    else if (kind == (int)kCkCrc32c)
        hipLaunchKernelGGL((k_cksum_tiles<kCkCrc32c>), dim3(workgroups), dim3(kCkThreads), 0, stream, t, d_seeds,
                           (const uint64_t *)s.prefix, s.part, s.carry, pw_crc32c);
    else
        hipLaunchKernelGGL((k_cksum_tiles<kCkCrc32>), dim3(workgroups), dim3(kCkThreads), 0, stream, t, d_seeds,
                           (const uint64_t *)s.prefix, s.part, s.carry, pw_crc32);
    hipLaunchKernelGGL(k_cksum_finish, dim3((n + 255) / 256), dim3(256), 0, stream, (uint32_t)kind, t, o,
                       (const uint64_t *)s.prefix, s.part, (const uint32_t *)s.carry, workgroups, s.rec);
    hipLaunchKernelGGL(k_cksum_record, dim3(1), dim3(64), 0, stream, t, d_expected, (const uint32_t *)s.part, s.rec);
}

// Member discovery (gzpx_mscan.h).  Everything the later kernels need to know about the candidates they work on is
// read from the scan record on the device, so the whole sequence is enqueued without a host round trip; grids are
// sized by the capacity of the candidate arrays.
void launch_member_scan(int format, const uint8_t *d_in, uint64_t in_len, uint32_t seg_bytes, uint32_t n_seg,
                        uint32_t rounds, const MemberScanScratch &m, hipStream_t stream) {
    MsStream s;
    s.in = d_in;
    s.len = in_len;
    s.lead = (uint32_t)((uintptr_t)d_in & 15u);
    s.hdr = header_bytes((uint32_t)format);
    s.sid = format == 0 ? ('B' | ('C' << 8)) : ('I' | ('G' << 8));
    s.seg_words = seg_bytes / 16u;
    const uint32_t cand_grid = (n_seg + kMsThreads / 64u - 1u) / (kMsThreads / 64u);
    const uint32_t g = m.cap / 256u + 1u < 2048u ? m.cap / 256u + 1u : 2048u;
    hipLaunchKernelGGL((k_mscan_cand<false>), dim3(cand_grid), dim3(kMsThreads), 0, stream, s, n_seg, m.seg_count,
                       (const uint32_t *)nullptr, (const uint32_t *)nullptr, m.cap, (uint64_t *)nullptr, (uint32_t *)nullptr);
    hipLaunchKernelGGL(k_mscan_offsets, dim3(1), dim3(256), 0, stream, n_seg, (const uint32_t *)m.seg_count, m.seg_off, m.rec);
    hipLaunchKernelGGL((k_mscan_cand<true>), dim3(cand_grid), dim3(kMsThreads), 0, stream, s, n_seg, m.seg_count,
                       (const uint32_t *)m.seg_off, (const uint32_t *)m.rec, m.cap, m.pos, m.size);
    hipLaunchKernelGGL(k_mscan_succ, dim3(g), dim3(256), 0, stream, in_len, s.hdr, m.cap, m.rec, (const uint64_t *)m.pos,
                       (const uint32_t *)m.size, m.succ, m.jump[0], m.idx);
    for (uint32_t r = 0; r < rounds; r++)
        hipLaunchKernelGGL(k_mscan_jump, dim3(g), dim3(256), 0, stream, r, m.cap, (const uint32_t *)m.rec,
                           (const uint32_t *)m.jump[r & 1u], m.jump[(r & 1u) ^ 1u], m.idx);
    hipLaunchKernelGGL(k_mscan_finish, dim3(g), dim3(256), 0, stream, m.cap, m.rec, (const uint64_t *)m.pos,
                       (const uint32_t *)m.size, (const uint32_t *)m.succ, (const uint32_t *)m.idx);
}

void launch_member_emit(const MemberScanScratch &m, uint32_t n_emit, uint64_t *d_offsets, uint32_t *d_sizes,
                        hipStream_t stream) {
    const uint32_t g = m.cap / 256u + 1u < 2048u ? m.cap / 256u + 1u : 2048u;
    hipLaunchKernelGGL(k_mscan_emit, dim3(g), dim3(256), 0, stream, m.cap, (const uint32_t *)m.rec, n_emit,
                       (const uint64_t *)m.pos, (const uint32_t *)m.size, (const uint32_t *)m.idx, d_offsets, d_sizes);
}

// the footers of nb members and the exclusive prefix sum of their ISIZE fields (d_out_off[nb] = the total)
void launch_member_index(const uint8_t *d_in, const uint64_t *d_offsets, const uint32_t *d_sizes, uint32_t nb, void *d_blk,
                         uint64_t *d_out_off, hipStream_t stream) {
    DBlock *blk = (DBlock *)d_blk;
    hipLaunchKernelGGL(k_dinit, dim3((nb + 255) / 256), dim3(256), 0, stream, 18u, nb, d_in, d_offsets, d_sizes, blk,
                       (uint32_t *)nullptr);  // (the footers only: nothing reads the payload bounds)
    hipLaunchKernelGGL(k_dscan, dim3(1), dim3(256), 0, stream, nb, (const DBlock *)blk, d_out_off);
}

// Random access by range (gzpx_ranges.h): the marks and the record are cleared, every range located, the selection
// compacted; the caller reads r.rec before it sizes the inflate.
void launch_ranges_select(const RrIndex &ix, uint32_t n_ranges, int virt, const RangeScratch &r, uint64_t *d_sel_off,
                          uint32_t *d_sel_size, hipStream_t stream) {
    (void)hipMemsetAsync(r.diff, 0, ((size_t)ix.n + 1u) * 4u, stream);
    (void)hipMemsetAsync(r.rec, 0xFF, 32, stream);
    if (n_ranges)
        hipLaunchKernelGGL(k_rr_locate, dim3((n_ranges + kRrThreads - 1u) / kRrThreads), dim3(kRrThreads), 0, stream, ix,
                           n_ranges, (const uint64_t *)r.ranges, (uint32_t)(virt ? 1 : 0), r.first, r.len, r.src, r.diff, r.rec);
    hipLaunchKernelGGL(k_rr_select, dim3(1), dim3(kRrThreads), 0, stream, ix, n_ranges, (const uint32_t *)r.diff, d_sel_off,
                       d_sel_size, r.map, r.soff, (const uint32_t *)r.first, (const uint64_t *)r.len, r.src, r.out_off, r.rec);
}

void launch_ranges_gather(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, uint8_t *d_out, uint64_t total,
                          hipStream_t stream) {
    if (!total) return;
    const uint32_t lead = (uint32_t)((uintptr_t)d_out & 15u);
    const uint64_t tiles = (lead + total + kRrTile - 1u) / kRrTile;
    hipLaunchKernelGGL(k_rr_gather, dim3((uint32_t)tiles), dim3(kRrThreads), 0, stream, d_stage, (const uint64_t *)r.src,
                       (const uint64_t *)r.out_off, n_ranges, d_out, lead, total);
}

// Reads by line (gzpx_lines.h).  The build: a count behind every batch of the inflate, then the prefix sums.
void launch_lines_count(const uint8_t *d_stage, uint64_t base, uint64_t len, uint64_t total, uint32_t delim, uint32_t *d_cnt,
                        uint32_t *d_rec, hipStream_t stream) {
    if (!len) return;
    const uint64_t grid = (base + len + kLnTile - 1u) / kLnTile - base / kLnTile;  // the tiles the batch has bytes of
    hipLaunchKernelGGL(k_ln_count, dim3((uint32_t)grid), dim3(kLnThreads), 0, stream, d_stage, base, len, total, delim, d_cnt,
                       d_rec);
}

void launch_lines_prefix(const uint32_t *d_cnt, uint32_t tiles, uint64_t total, uint64_t *d_prefix, uint32_t *d_rec,
                         hipStream_t stream) {
    hipLaunchKernelGGL(k_ln_prefix, dim3(1), dim3(kLnThreads), 0, stream, d_cnt, tiles, total, d_prefix, d_rec);
}

// The search: the covers go where k_rr_locate reads its ranges; the walk of the boundary tiles runs behind the inflate.
void launch_lines_tiles(const LnTable &tb, uint32_t n, uint32_t per, const LinesScratch &l, const RangeScratch &r,
                        hipStream_t stream) {
    (void)hipMemsetAsync(l.rec, 0xFF, 32, stream);
    hipLaunchKernelGGL(k_ln_tiles, dim3((n + kLnThreads - 1u) / kLnThreads), dim3(kLnThreads), 0, stream, tb, n, per,
                       (const uint64_t *)l.bounds, r.ranges, l.btile, l.bpos, l.rec);
}

void launch_lines_find(const LnTable &tb, uint32_t n, uint32_t per, uint32_t delim, const LinesScratch &l, const RangeScratch &r,
                       const uint8_t *d_stage, hipStream_t stream) {
    const uint32_t n_bounds = n * per, waves = kLnThreads / 64u;
    hipLaunchKernelGGL(k_ln_find, dim3((n_bounds + waves - 1u) / waves), dim3(kLnThreads), 0, stream, tb, n_bounds, per, delim,
                       (const uint64_t *)l.bounds, (const uint64_t *)r.ranges, (const uint64_t *)r.src, d_stage,
                       (const uint32_t *)l.btile, l.bpos);
    if (per == 2u)
        hipLaunchKernelGGL(k_ln_offsets, dim3(1), dim3(kLnThreads), 0, stream, n, (const uint64_t *)r.ranges,
                           (const uint64_t *)l.bpos, r.src, r.out_off, l.rec);
}

// The search (gzpx_find.h, for a set gzpx_findset.h), behind the inflate of a batch into staging.
static FdArgs find_args(const FindBatch &b, uint32_t &x0, uint32_t &grid) {
    const uint64_t r0 = kFdPad - b.carry, r1 = kFdPad + b.len;
    x0 = (uint32_t)(r0 / kFdPiece);
    grid = (uint32_t)((r1 + kFdPiece - 1u) / kFdPiece) - x0;
    return FdArgs{b.stage, r0, r1, b.base, b.m, b.delim >= 0 ? 1u : 0u, b.delim >= 0 ? (uint32_t)b.delim : 0u};
}

// (mt says which matcher runs: the pattern in f.pat, or the set of gzpx_findset.h)
void launch_find_count(const FindBatch &b, const FindScratch &f, const FindMatcher &mt, hipStream_t stream) {
    uint32_t x0, grid;
    const FdArgs a = find_args(b, x0, grid);
    if (mt.d_set)
        hipLaunchKernelGGL(k_fs_count, dim3(grid), dim3(kFdThreads), 0, stream, a, x0, mt.d_set, f.cnt, (unsigned long long *)mt.d_counts);
    else
        hipLaunchKernelGGL(k_fd_count, dim3(grid), dim3(kFdThreads), 0, stream, a, x0, (const uint32_t *)f.pat, f.cnt);
    hipLaunchKernelGGL(k_fd_scan, dim3(1), dim3(kFdThreads), 0, stream, (const uint32_t *)f.cnt, grid, f.bases, f.rec);
}

void launch_find_write(const FindBatch &b, const FindScratch &f, const FindMatcher &mt, uint64_t *d_positions, uint32_t *d_ids,
                       uint64_t *d_lines, uint64_t cap, hipStream_t stream) {
    uint32_t x0, grid;
    const FdArgs a = find_args(b, x0, grid);
    if (mt.d_set)
        hipLaunchKernelGGL(k_fs_write, dim3(grid), dim3(kFdThreads), 0, stream, a, x0, mt.d_set, (const uint32_t *)f.cnt,
                           (const uint64_t *)f.bases, d_positions, d_ids, d_lines, cap);
    else
        hipLaunchKernelGGL(k_fd_write, dim3(grid), dim3(kFdThreads), 0, stream, a, x0, (const uint32_t *)f.pat,
                           (const uint32_t *)f.cnt, (const uint64_t *)f.bases, d_positions, d_lines, cap);
}

void launch_find_carry(const FindBatch &b, const FindScratch &f, uint32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(k_fd_carry, dim3(1), dim3(kFdThreads), 0, stream, b.stage, kFdPad + b.len - n, n,
                       b.delim >= 0 ? 1u : 0u, b.delim >= 0 ? (uint32_t)b.delim : 0u, f.rec);
}

// The selection (gzpx_select.h): the marking pass behind the count and the scan of a batch, the runs behind the last.
void launch_select_mark(const FindBatch &b, const FindScratch &f, const FindMatcher &mt, const SelectScratch &s, uint64_t group,
                        uint64_t n_records, hipStream_t stream) {
    uint32_t x0, grid;
    const FdArgs a = find_args(b, x0, grid);
    if (mt.d_set)
        hipLaunchKernelGGL(k_fs_mark, dim3(grid), dim3(kFdThreads), 0, stream, a, x0, mt.d_set, (const uint32_t *)f.cnt,
                           (const uint64_t *)f.bases, s.bitmap, group, n_records);
    else
        hipLaunchKernelGGL(k_sl_mark, dim3(grid), dim3(kFdThreads), 0, stream, a, x0, (const uint32_t *)f.pat,
                           (const uint32_t *)f.cnt, (const uint64_t *)f.bases, s.bitmap, group, n_records);
}

void launch_select_runs(const SelectScratch &s, const FindScratch &f, uint64_t n_records, uint64_t group, uint64_t n_lines,
                        int invert, uint64_t *d_runs, uint64_t cap, hipStream_t stream) {
    const uint32_t groups = (uint32_t)select_groups(n_records), inv = invert ? 1u : 0u;
    const uint8_t *bits = (const uint8_t *)s.bitmap;
    hipLaunchKernelGGL(k_sl_runs_count, dim3(groups), dim3(kSlRunThreads), 0, stream, bits, n_records, inv, s.cnt);
    hipLaunchKernelGGL(k_sl_runs_scan, dim3(1), dim3(kFdThreads), 0, stream, (const uint32_t *)s.cnt, groups, s.bases,
                       (const uint64_t *)f.rec, s.rec);
    if (d_runs && cap)
        hipLaunchKernelGGL(k_sl_runs_write, dim3(groups), dim3(kSlRunThreads), 0, stream, bits, n_records, inv,
                           (const uint32_t *)s.cnt, (const uint32_t *)s.bases, group, n_lines, d_runs, cap);
}

// Fields of lines (gzpx_fields.h), behind launch_lines_find of line ranges: three passes over the ranges' bytes in
// staging with no host round trip between them.  `grid` = fields_pieces(): the pieces are counted on the device.
static FlArgs fields_args(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const FieldsScratch &f, uint32_t delim,
                          uint32_t field_delim) {
    return FlArgs{d_stage, r.src, r.out_off, f.pfirst, n_ranges, delim, field_delim};
}

void launch_fields_carry(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const FieldsScratch &f, uint32_t delim,
                         uint32_t field_delim, uint32_t grid, hipStream_t stream) {
    hipLaunchKernelGGL(k_fl_plan, dim3(1), dim3(kFlThreads), 0, stream, n_ranges, (const uint64_t *)r.src,
                       (const uint64_t *)r.out_off, f.pfirst, f.rec);
    if (grid)
        hipLaunchKernelGGL(k_fl_carry, dim3(grid), dim3(kFlThreads), 0, stream, fields_args(d_stage, n_ranges, r, f, delim, field_delim),
                           f.carry);
    hipLaunchKernelGGL(k_fl_carry_scan, dim3(1), dim3(kFlThreads), 0, stream, (const uint32_t *)f.carry, (const uint64_t *)f.pfirst,
                       n_ranges, f.cin);
}

void launch_fields_count(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const FieldsScratch &f, uint32_t delim,
                         uint32_t field_delim, uint32_t grid, uint64_t *d_out_off, hipStream_t stream) {
    if (grid)
        hipLaunchKernelGGL(k_fl_count, dim3(grid), dim3(kFlThreads), 0, stream, fields_args(d_stage, n_ranges, r, f, delim, field_delim),
                           (const FlSet *)f.set, (const uint64_t *)f.cin, f.cnt);
    hipLaunchKernelGGL(k_fl_scan, dim3(1), dim3(kFlThreads), 0, stream, (const uint32_t *)f.cnt, (const uint64_t *)f.pfirst, n_ranges,
                       f.obase, d_out_off, f.rec);
}

void launch_fields_write(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const FieldsScratch &f, uint32_t delim,
                         uint32_t field_delim, uint32_t grid, uint8_t *d_out, uint64_t out_cap, hipStream_t stream) {
    if (grid)
        hipLaunchKernelGGL(k_fl_write, dim3(grid), dim3(kFlThreads), 0, stream, fields_args(d_stage, n_ranges, r, f, delim, field_delim),
                           (const FlSet *)f.set, (const uint64_t *)f.cin, (const uint32_t *)f.cnt, (const uint64_t *)f.obase,
                           (const uint64_t *)f.rec, d_out, out_cap);
}

// Numeric columns of lines (gzpx_columns.h), behind launch_fields_carry on c.fl: the rows, then the one parsing pass.
void launch_columns_rows(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const LinesScratch &l,
                         const ColumnsScratch &c, uint32_t delim, uint32_t field_delim, uint32_t grid, uint64_t *d_row_off,
                         hipStream_t stream) {
    (void)hipMemsetAsync(c.rec, 0, kClRecWords * 8, stream);
    if (grid)
        hipLaunchKernelGGL(k_cl_rows, dim3(grid), dim3(kFlThreads), 0, stream, fields_args(d_stage, n_ranges, r, c.fl, delim, field_delim),
                           c.rcnt);
    hipLaunchKernelGGL(k_cl_rows_scan, dim3(1), dim3(kFlThreads), 0, stream, (const uint64_t *)l.bounds, (const uint32_t *)c.fl.carry,
                       (const uint32_t *)c.rcnt, (const uint64_t *)c.fl.pfirst, n_ranges, c.rin, d_row_off, c.rec);
}

void launch_columns_parse(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const ColumnsScratch &c, uint32_t delim,
                          uint32_t field_delim, uint32_t grid, const uint64_t *d_row_off, uint64_t *d_values, uint8_t *d_status,
                          uint64_t rows_cap, hipStream_t stream) {
    if (grid)
        hipLaunchKernelGGL(k_cl_parse, dim3(grid), dim3(kFlThreads), 0, stream, fields_args(d_stage, n_ranges, r, c.fl, delim, field_delim),
                           (const ClCols *)c.cols, (const uint64_t *)c.fl.cin, (const uint64_t *)c.rin, d_row_off, c.rec, d_values,
                           d_status, rows_cap);
}

// Selection of lines by their numbers (gzpx_where.h), behind launch_columns_rows on w.cl: the parse with the predicate,
// then the runs.  The rows are known on the device only: `bits` sizes the bitmaps and bounds the grids.
void launch_where_parse(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const WhereScratch &w, uint32_t delim,
                        uint32_t field_delim, uint32_t grid, const uint64_t *d_row_off, uint64_t bits, bool text, hipStream_t stream) {
    (void)hipMemsetAsync(w.bitmap, 0, (size_t)(bits / 8u) * 2u, stream);  // (w.starts lies behind w.bitmap)
    if (!grid) return;
    const FlArgs a = fields_args(d_stage, n_ranges, r, w.cl.fl, delim, field_delim);
    if (text)
        hipLaunchKernelGGL(k_wh_parse<true>, dim3(grid), dim3(kFlThreads), 0, stream, a, (const ClCols *)w.cl.cols,
                           (const WhTextTerms *)w.terms, (const uint64_t *)w.cl.fl.cin, (const uint64_t *)w.cl.rin, d_row_off, w.cl.rec,
                           w.bitmap, bits);
    else
        hipLaunchKernelGGL(k_wh_parse<false>, dim3(grid), dim3(kFlThreads), 0, stream, a, (const ClCols *)w.cl.cols,
                           (const WhTextTerms *)w.terms, (const uint64_t *)w.cl.fl.cin, (const uint64_t *)w.cl.rin, d_row_off, w.cl.rec,
                           w.bitmap, bits);
}

void launch_where_runs(uint32_t n_ranges, const LinesScratch &l, const WhereScratch &w, const uint64_t *d_row_off, uint64_t bits,
                       int invert, uint64_t *d_runs, uint64_t cap, hipStream_t stream) {
    const uint64_t groups = bits / kSlRunRecords;
    const uint32_t grid = (uint32_t)(groups < kWhRunGrid ? groups : kWhRunGrid), inv = invert ? 1u : 0u;
    const uint8_t *rows = (const uint8_t *)w.bitmap, *starts = (const uint8_t *)w.starts;
    hipLaunchKernelGGL(k_wh_starts, dim3((n_ranges + kFlThreads - 1u) / kFlThreads), dim3(kFlThreads), 0, stream, d_row_off, n_ranges, bits,
                       w.starts);
    if (grid) hipLaunchKernelGGL(k_wh_runs_count, dim3(grid), dim3(kSlRunThreads), 0, stream, rows, starts, (const uint64_t *)w.cl.rec, bits, inv, w.cnt);
    hipLaunchKernelGGL(k_wh_runs_scan, dim3(1), dim3(kFdThreads), 0, stream, (const uint32_t *)w.cnt, (const uint64_t *)w.cl.rec, bits,
                       w.bases, w.rec);
    if (grid && d_runs && cap)
        hipLaunchKernelGGL(k_wh_runs_write, dim3(grid), dim3(kSlRunThreads), 0, stream, rows, starts, (const uint64_t *)w.cl.rec, bits, inv,
                           (const uint32_t *)w.cnt, (const uint32_t *)w.bases, d_row_off, (const uint64_t *)l.bounds, n_ranges, d_runs, cap);
}

size_t inflate_mlist_bytes(uint64_t out_cap, uint64_t nb) { return (size_t)((out_cap / 3u + nb + 2u) * sizeof(LzMatch)); }
size_t inflate_tfirst_bytes(uint64_t out_cap, uint64_t nb) { return (size_t)(((out_cap >> kLzTileShift) + 2u * nb + 4u) * 4u); }

}  // namespace gzpx
