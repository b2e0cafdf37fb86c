// gzpx_policy.h -- the decisions of libdeflate's compressor that are not in RFC 1951, once: where a DEFLATE block ends
// and which matches count.  Arithmetic without state (constexpr, host and device), included inside namespace gzpx by
// gzpx_wave.h (for gzpx_kernels.hip), by gzpx_nearopt.hip and by gzpx_api.cpp.  One wrong constant here breaks
// bit-exactness for some level on some input: tests/policy_cases.py sits on both sides of every threshold.  Each comment
// names the libdeflate routine restated and the callers.  Only the scalar rule is shared; each parser keeps its lane
// shape: one thread per check in k_parse_hc, one lane per class and a wave reduction in k_parse_lazy, a serial loop in
// k_near_optimal.  The lazy and lazy2 preference formulas have one site each (k_parse_lazy) and stay there; the `>> 11`
// of deflate_choose_default_litlen_costs (no_optimize_block) is another routine's cutoff, not recalc_cutoff.
//
// Two sites keep their own text for measured speed, MiB/s on the 550 MiB text slab, parent | branch alternating, the
// branch below the parent in every pair; both have to be kept in step by hand.
//   hc_calc_min_len (gzpx_kernels.hip) says the 512 and the 4096 of min_len_scan_len itself and scans a short block
//     whose census it then drops; no_calc_min_len calls min_len_scan_len and min_len_of_census.  With the two calls
//     k_parse_hc<true> spilled 53 VGPRs, not 43, and k_match_hc_sparse grew by 112 instructions: level 3 35647 35404
//     35369 | 35417 35212 35322, level 4 33426 33605 33620 | 32826 33341 33348.
//   k_parse_lazy says should_end_block's gate (twice) and the two recalculation points in its own words, over
//     kObsPerCheck, kMinBlockLen and kFirstRecalc; k_near_optimal calls split_due.  With split_due and two routines
//     for the points in it: level 6 20463 20494 20482 20427 20425 | 20422 20431 20356 20404 20294.  With its own text
//     the kernel is the parent's instruction for instruction.
// (All measurements: docs/LAB_NOTES.md, "gzpx_policy.h".)
#pragma once

// lz_hash (ht_, hc_, bt_matchfinder): cand_bucket, k_candidates' interior body, the bucket-0 tests of k_match_hc_sparse
// and k_hc_orphan, no_bt_advance
__host__ __device__ constexpr uint32_t lz_hash(uint32_t v, uint32_t bits) { return (v * 0x1E35A7BDu) >> (32u - bits); }

constexpr uint32_t kFastSeqStoreLen = 8192, kFastSoftMaxBlockLen = 65535;  // FAST_SEQ_STORE_LENGTH, FAST_SOFT_MAX_BLOCK_LENGTH: level 1
constexpr uint32_t kSeqStoreLen = 50000, kSoftMaxBlockLen = 300000;        // SEQ_STORE_LENGTH, SOFT_MAX_BLOCK_LENGTH: levels 2-12
constexpr uint32_t kMinBlockLen = 5000;                                    // MIN_BLOCK_LENGTH (the host's capacities as well)
constexpr uint32_t kMinMatchLen = 3;                                       // DEFLATE_MIN_MATCH_LEN
constexpr uint32_t kNumObs = 10, kObsPerCheck = 512;  // NUM_OBSERVATION_TYPES, NUM_OBSERVATIONS_PER_BLOCK_CHECK

// choose_max_block_end, no tail shorter than kMinBlockLen: parse_block, hc_calc_min_len, the three splitting parsers
__host__ __device__ constexpr uint32_t max_block_end(uint32_t start, uint32_t n, uint32_t soft_max) {
    return n - start < soft_max + kMinBlockLen ? n : start + soft_max;
}

// observe_literal / observe_match, the block splitter's classes: the three splitting parsers
__host__ __device__ constexpr uint32_t obs_literal(uint32_t byte) { return ((byte >> 5) & 6u) | (byte & 1u); }
__host__ __device__ constexpr uint32_t obs_match(uint32_t len) { return 8u + (len >= 9u ? 1u : 0u); }

// should_end_block's gate: k_near_optimal (k_parse_lazy: see above).  k_parse_hc takes it apart over token indices --
// the token with kObsPerCheck - 1 before it, the first one that ends kMinBlockLen bytes in, the check that ends less
// than kMinBlockLen before the end -- and names the two constants where it does.
__host__ __device__ constexpr bool split_due(uint32_t num_new, uint32_t pos, uint32_t start, uint32_t n) {
    return num_new >= kObsPerCheck && pos - start >= kMinBlockLen && n - pos >= kMinBlockLen;
}
// do_end_block_check (k_parse_hc, k_parse_lazy, no_end_block_check): one class's share of total_delta, obs of num_obs
// merged observations against nw of num_new new ones, and the verdict on the ten shares' sum -- true ends the block
__host__ __device__ constexpr uint32_t split_delta(uint32_t obs, uint32_t nw, uint32_t num_obs, uint32_t num_new) {
    const uint32_t expected = obs * num_new, actual = nw * num_obs;
    return actual > expected ? actual - expected : expected - actual;
}
__host__ __device__ constexpr bool split_verdict(uint32_t total_delta, uint32_t num_obs, uint32_t num_new, uint32_t block_len) {
    if (num_obs == 0) return false;
    const uint32_t num_items = num_obs + num_new;
    uint32_t cutoff = num_new * 200u / 512u * num_obs;
    if (block_len < 10000u && num_items < 8192u) cutoff += (uint32_t)((unsigned long long)cutoff * (8192u - num_items) / 8192u);
    return total_delta + (block_len / 4096u) * num_obs >= cutoff;
}

// choose_min_match_len, by the number of distinct literals in use and capped where the search is shallow:
// min_len_of_census, k_parse_lazy's recalculation, no_optimize_block.  The cap 4 (depth < 5) is reached by no level: the
// static_assert below is its only check.
__host__ __device__ constexpr uint32_t choose_min_match_len(uint32_t num_used, uint32_t depth) {
    uint32_t m = num_used < 6 ? 9 : num_used < 8 ? 8 : num_used < 10 ? 7 : num_used < 16 ? 6 : num_used < 45 ? 5 : num_used < 80 ? 4 : 3;
    if (depth < 16) {
        const uint32_t cap = depth < 5 ? 4 : depth < 10 ? 5 : 7;
        if (m > cap) m = cap;
    }
    return m;
}

// calculate_min_match_len (no_calc_min_len; hc_calc_min_len says the same in its own text, see above): how many bytes
// from the block's start are counted -- 0: none, the answer is kMinMatchLen (libdeflate >= 1.1x, compat 0, does not scan
// a block shorter than 512 bytes) -- and the answer from the census, bit v of used[v >> 5] set for every byte value v seen
__host__ __device__ constexpr uint32_t min_len_scan_len(uint32_t data_len, uint32_t compat) {
    return compat == 0 && data_len < 512u ? 0u : data_len < 4096u ? data_len : 4096u;
}
__host__ __device__ constexpr uint32_t min_len_of_census(const uint32_t *used, uint32_t depth) {
    uint32_t num_used = 0;
    for (uint32_t k = 0; k < 8; k++) num_used += (uint32_t)__builtin_popcount(used[k]);
    return choose_min_match_len(num_used, depth);
}

// recalculate_min_match_len (k_parse_lazy): first due kFirstRecalc bytes into the block, and again once the block is as
// long again as it was (both in the kernel's text); literals more frequent than 1/1024 of all of them count as used
constexpr uint32_t kFirstRecalc = 10000;
__host__ __device__ constexpr uint32_t recalc_cutoff(uint32_t total) { return total >> 10; }

// deflate_compress_greedy, long enough and a length-3 match only at a short distance: hc_dense_block, k_match_hc_sparse
__host__ __device__ constexpr bool greedy_takes(uint32_t len, uint32_t dist, uint32_t min_len) {
    return len >= min_len && (len > 3u || dist <= 4096u);
}

// libdeflate_alloc_compressor, levels 2-12 (0 and 1 search no chains): max_search_depth, nice_match_length, the parser
// (0 greedy and near-optimal, 1 lazy, 2 lazy2), num_optim_passes.  gzpx_ctx_create fills Config from it.
struct LevelParams {
    uint32_t depth, nice, lazy, passes;
};
__host__ __device__ constexpr LevelParams level_params(uint32_t level) {
    const uint32_t depth[13] = {0, 0, 6, 12, 16, 16, 35, 100, 300, 600, 35, 70, 150};
    const uint32_t nice[13] = {0, 0, 10, 14, 30, 30, 65, 130, 258, 258, 75, 150, 258};
    return {depth[level], nice[level], level >= 10 ? 0u : level >= 8 ? 2u : level >= 5 ? 1u : 0u, level >= 10 ? level - 8u : 0u};
}

// libdeflate's own words, for the static_asserts: min_lens[] with the caps behind it, for every depth up to 16 and
// every level's; the level table row by row
constexpr bool policy_min_len_is_libdeflates() {
    const uint8_t min_lens[80] = {9, 9, 9, 9, 9, 9, 8, 8, 7, 7, 6, 6, 6, 6, 6, 6, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5,
                                  5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 4, 4, 4, 4, 4, 4, 4, 4, 4,
                                  4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4};
    for (uint32_t i = 0; i <= 16 + 12; i++) {
        const uint32_t depth = i <= 16 ? i : level_params(i - 16).depth;
        for (uint32_t num_used = 0; num_used < 256; num_used++) {
            uint32_t min_len = num_used >= 80 ? kMinMatchLen : min_lens[num_used];
            if (depth < 16) {
                if (depth < 5) min_len = min_len < 4 ? min_len : 4;
                else if (depth < 10) min_len = min_len < 5 ? min_len : 5;
                else min_len = min_len < 7 ? min_len : 7;
            }
            if (choose_min_match_len(num_used, depth) != min_len) return false;
        }
    }
    return true;
}
constexpr bool policy_level_is(uint32_t level, uint32_t depth, uint32_t nice, uint32_t lazy, uint32_t passes) {
    const LevelParams p = level_params(level);
    return p.depth == depth && p.nice == nice && p.lazy == lazy && p.passes == passes;
}
static_assert(policy_min_len_is_libdeflates(), "the comparison chain is libdeflate's min_lens[] table, caps included, for 0..255 literals in use");
static_assert(policy_level_is(2, 6, 10, 0, 0) && policy_level_is(3, 12, 14, 0, 0) && policy_level_is(4, 16, 30, 0, 0) &&
                  policy_level_is(5, 16, 30, 1, 0) && policy_level_is(6, 35, 65, 1, 0) && policy_level_is(7, 100, 130, 1, 0) &&
                  policy_level_is(8, 300, 258, 2, 0) && policy_level_is(9, 600, 258, 2, 0) && policy_level_is(10, 35, 75, 0, 2) &&
                  policy_level_is(11, 70, 150, 0, 3) && policy_level_is(12, 150, 258, 0, 4),
              "levels 2-12 as libdeflate_alloc_compressor's switch has them");
