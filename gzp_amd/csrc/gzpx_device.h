// gzpx_device.h -- data layout shared by the HIP kernels and the host pipeline.  Included by gzpx_kernels.hip and
// gzpx_nearopt.hip (the kernels and their launchers), gzpx_api.cpp (the C ABI over them) and gzpx_par.cpp (the
// members' header length), each behind hip/hip_runtime.h.
//
// Vocabulary (follows the reference): a *block* is one BGZF/Mgzip member = one `buffer_size`
// cut of the caller's stream (src/par/compress.rs:415-416); a *sub-block* is one DEFLATE block
// inside its payload (libdeflate starts a new one every 8192 matches); a *token* is one
// literal or one match of the level-1 greedy parse.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gzpx {

constexpr unsigned kTile = 65536;         // positions handled per LDS tile (k_parse) / stage window
constexpr unsigned kMaxBlockSize = 1u << 26;  // largest buffer_size the kernels accept (64 MiB; round 6: tested at 32 MiB)
constexpr unsigned kNumLitlen = 288;
constexpr unsigned kNumOffset = 32;
constexpr unsigned kHistStride = kNumLitlen + kNumOffset;  // 320 u32 per sub-block
constexpr unsigned kHdrWords = 160;                        // dynamic header bit string, <= 4554 bits
constexpr unsigned kCodeWords = kNumLitlen + kNumOffset;   // (codeword | len << 16) per symbol

// bytes in front of a member's DEFLATE payload (BlockFormatSpec::HEADER_SIZE); `format` as in Config: 0 BGZF, 1 Mgzip
constexpr uint32_t header_bytes(uint32_t format) { return format == 0 ? 18u : 20u; }

constexpr uint32_t kTokMatch = 0x80000000u;  // token = kTokMatch | offset << 9 | length

enum SubType : uint32_t { kStored = 0, kStatic = 1, kDynamic = 2 };

enum BlockStatus : uint32_t {
    kStatusOk = 0,
    kStatusBlockSizeExceeded = 2,  // BGZF payload >= 65536 (src/bgzf.rs:218-223)
    kStatusInternal = 3,           // a capacity this implementation sizes was exceeded (reported as a device error)
};

struct SubMeta {
    uint32_t type;       // SubType
    uint32_t tok_begin;  // token range in the block's token array
    uint32_t tok_end;
    uint32_t byte_begin;  // input range covered (for stored blocks and the uncompressed cost)
    uint32_t byte_len;
    uint32_t bit_begin;  // first bit of this sub-block inside the payload
    uint32_t hdr_bits;   // bits of BFINAL+BTYPE(+dynamic header) held in hdr[]
    uint32_t is_final;
};

struct BlockMeta {
    uint32_t n;              // input bytes
    uint32_t is_last;        // append BGZF_EOF
    uint32_t ntok;
    uint32_t nsub;
    uint32_t payload_bytes;  // raw DEFLATE size c
    uint32_t framed_bytes;   // header + c + footer (+ EOF)
    uint32_t crc;
    uint32_t status;
};

// What the host needs back from one batch (written by k_scan): 16 bytes instead of every BlockMeta.
struct SlabResult {
    uint64_t total;        // framed bytes of the slab up to and including this batch
    uint32_t fail_block;   // first block whose status is not kStatusOk, 0xFFFFFFFF = none
    uint32_t fail_status;  // that block's BlockStatus
};

// Levels 2-4: per-block parse state carried between tiles and between match/parse rounds (a
// round ends early when a new DEFLATE sub-block needs another minimum match length).
struct HcState {
    uint32_t done;        // the block's token stream is complete
    uint32_t min_len;     // min_len of the sub-block that starts at resume_pos (0 = not computed yet)
    uint32_t resume_pos;  // where match results must be (re)computed and the parse resumes
    uint32_t tok_carry;   // tokens emitted before resume_pos
    uint32_t mat_carry;   // matches emitted before resume_pos
    uint32_t cur_sub;     // index of the sub-block that starts at resume_pos
    uint32_t rounds;      // diagnostics
    uint32_t pad;
    // what k_match_hc's arrays (len8 / which / alt) hold for this block (round 5, k_match_hc_sparse):
    //   0 nothing yet, or not usable: the dense k_match_hc must run (from resume_pos)
    //   1 the full search ONLY for the token starts of the greedy parse from position 0 with HcState.min_len (every other
    //     position: the search's first chain node) -- all a parse needs as long as min_len does not change
    //   2 a later sub-block needs another min_len (k_parse_hc found out, and listed the block for k_match_hc_stale): as 0
    //     until that kernel has been over the block, as 3 from resume_pos on behind it (the value stays 2)
    //   3 the full search of every position (the dense kernel ran)
    uint32_t sparse;
};
constexpr uint32_t kHcArraysNone = 0, kHcArraysPath = 1, kHcArraysStale = 2, kHcArraysDense = 3;

struct CrcConsts {
    uint32_t pow64[10];  // x^(8*64*2^l) mod P (reflected), l = 0..9
    uint32_t pow_tile;   // x^(8*65536) mod P: appends one full 64 KiB chunk
};

struct Config {
    uint32_t format;      // 0 BGZF, 1 Mgzip
    uint32_t level;       // 1
    uint32_t compat;      // 0: libdeflate >= 1.1x Huffman rule, 1: libdeflate 1.10
    uint32_t block_size;  // buffer_size of the reference's builder
    uint32_t xfl;         // gzip XFL byte derived from level (src/bgzf.rs:278-284)
    uint32_t debug;       // diagnostics only: bit 0 = k_candidates' order-independent fallback on every block, bit 1 =
                          // level 1 through the dense k_match / k_parse pair instead of k_mparse, bit 2 =
                          // k_mparse hands every block back (exercises the redo list); bit 7 = k_candidates takes
                          // every iteration through its clamped body (same stream; A/B timing); bits 8-9 (host
                          // side, experiments): where the CRC kernel is forked onto the side stream
    uint32_t stride;      // per-block stride (positions) of cand / len8 / alt / tok: >= block_size + 1024
    uint32_t max_sub;     // per-block capacity of sub / hist / codes / hdr (sub-blocks >= 32768 bytes)
    uint32_t passthrough; // n <= 55 - 4*level is emitted as stored blocks only (deflate_compress_none)
    uint32_t hc_depth;    // levels 2-9: max_search_depth
    uint32_t hc_nice;     // levels 2-9: nice_match_length
    uint32_t lazy;        // 0: greedy parser (levels 2-4), 1: lazy (5-7), 2: lazy2 (8-9)
    uint32_t n_cu;        // compute units of the device (persistent kernels launch one workgroup per CU)
    uint32_t no_passes;   // levels 10-12: num_optim_passes (hc_depth / hc_nice hold max_search_depth / nice_match_length)
};

// Device scratch for one batch of blocks.
struct Scratch {
    BlockMeta *meta;      // [nb]
    SubMeta *sub;         // [nb][max_sub]
    uint16_t *cand;       // [nb][stride]        d0: distance to the bucket predecessor (0 = none)
    uint8_t *len8;        // [nb][stride]        0 = no match at p, else match length - 3
    uint32_t *which;      // [nb][stride/32]     bit p: the older candidate won at p
    uint16_t *alt;        // [nb][stride]        match distance at p where that bit is set
    uint16_t *d4;         // [nb][stride]        levels 2-9: distance to the hash4 chain predecessor
    uint8_t *lz_len;      // [nb][2][stride]     levels 5-9: length - 3 of the half / quarter depth searches
    uint16_t *lz_dist;    // [nb][2][stride]     levels 5-9: their distances (0 = no match)
    HcState *hc;          // [nb]                levels 2-4: parse state
    uint32_t *pending;    // [1]                 levels 2-4: blocks that need another round
    uint32_t *tok;        // [nb][stride]        worst case one token per byte
    uint32_t *redo;       // [1 + nb]            level 1: blocks k_mparse hands back to k_match / k_parse
    uint32_t *claim;      // [8]                 ticket counters of the persistent kernels that claim their blocks (behind redo's list)
    uint32_t *hist;       // [nb][max_sub][kHistStride]
    uint32_t *codes;      // [nb][max_sub][kCodeWords]
    uint32_t *hdr;        // [nb][max_sub][kHdrWords]
    uint64_t *out_off;    // [nb + 1] byte offset of each framed block in the output
    uint32_t *sizes;      // [nb]     framed size of each block (compact copy for the host / the index)
    // levels 10-12 (gzpx_nearopt.hip): the state of the blocks in flight, one lane each
    uint32_t no_lanes;    // how many
    void *no_state;       // [no_lanes] NoLane: trees, hash tables, costs, frequencies, Huffman scratch
    uint8_t *no_cache;    // [no_lanes] match cache (libdeflate's MATCH_CACHE_LENGTH entries + slack)
    uint8_t *no_nodes;    // [no_lanes] minimum-cost path nodes of a DEFLATE block
};

// Snap (gzpx_snap.h): per chunk of 64 KiB of a batch, chunk c = buffer * chunks_per_buffer + k
constexpr uint32_t kSnapStageBytes = 76544;  // >= MaxCompressedLength(65536) = 32 + 65536 + 65536 / 6
struct SnapScratch {
    uint8_t *stage;  // [chunks][kSnapStageBytes]  raw Snappy body of each chunk
    uint32_t *clen;  // [chunks]  its length (0: no such chunk)
    uint32_t *crc;   // [chunks]  masked CRC-32C of the uncompressed chunk
    uint32_t *coff;  // [chunks]  where the chunk's frame starts inside its buffer's
    uint64_t *dbg;   // [chunks][8] k_snap_chunk's phase clocks, when measuring (else null)
};
inline uint32_t snap_chunks_per_buffer(uint32_t bs) { return (bs + 65535u) / 65536u; }
void launch_snap_chunk(const uint8_t *slab, uint64_t slab_len, uint32_t bs, uint32_t nb, const SnapScratch &ss,
                       hipStream_t stream);
void launch_snap_frame(uint64_t slab_len, uint32_t bs, uint32_t nb, const Scratch &s, const SnapScratch &ss,
                       hipStream_t stream);
void launch_snap_emit(const uint8_t *slab, uint64_t slab_len, uint32_t bs, uint32_t nb, const Scratch &s,
                      const SnapScratch &ss, uint8_t *out, uint64_t out_cap, hipStream_t stream);

// Host-side launchers (gzpx_kernels.hip).  All asynchronous on `stream`.
void launch_init_meta(const Config &cfg, uint64_t slab_len, uint32_t nb, int is_last,
                      const Scratch &s, hipStream_t stream);
void launch_candidates(const Config &cfg, const uint8_t *slab, uint64_t slab_len, uint32_t nb, int is_last,
                       const Scratch &s, hipStream_t stream);  // (fills BlockMeta too: k_init_meta's work)
void launch_match(const Config &cfg, const uint8_t *slab, uint64_t slab_len, uint32_t nb,
                  const Scratch &s, hipStream_t stream);
void launch_parse(const Config &cfg, const uint8_t *slab, uint64_t slab_len, uint32_t nb,
                  const Scratch &s, hipStream_t stream);
void launch_hc(const Config &cfg, const uint8_t *slab, uint32_t nb, const Scratch &s, hipStream_t stream);
void launch_lazy(const Config &cfg, const uint8_t *slab, uint32_t nb, const Scratch &s, hipStream_t stream);
// levels 10-12 (gzpx_nearopt.hip)
size_t no_lane_bytes();
size_t no_cache_bytes();
size_t no_nodes_bytes(uint32_t block_size);
void launch_near_optimal_tables(void *lanes, uint32_t n_lanes, const uint8_t *d_tables, hipStream_t stream);
void launch_near_optimal(const Config &cfg, const uint8_t *slab, uint32_t nb, const Scratch &s, hipStream_t stream);
void launch_hist(const Config &cfg, uint32_t nb, const Scratch &s, hipStream_t stream);
void launch_huffman(const Config &cfg, uint32_t nb, const Scratch &s, hipStream_t stream);
void launch_crc32(const Config &cfg, const uint8_t *slab, uint64_t slab_len, uint32_t nb,
                  const Scratch &s, const CrcConsts &cc, hipStream_t stream);
void launch_scan(uint32_t nb, const Scratch &s, const SlabResult *prev, SlabResult *result, hipStream_t stream);
void launch_emit(const Config &cfg, const uint8_t *slab, uint64_t slab_len, uint32_t nb,
                 const Scratch &s, uint8_t *out, uint64_t out_cap, hipStream_t stream);

// ParDecompress side: one record per block (filled by k_dinit / k_inflate)
struct DBlockHost {
    uint64_t in_off;
    uint32_t size, isize, crc, status, produced, nmatch;
    uint32_t pay_off, pay_len;  // the DEFLATE payload inside the member
    uint32_t cyc[8];  // debug launches: see DBlock in gzpx_kernels.hip
};
// DBlockHost.status of a member that was inflated (kInfShortOutput: fewer bytes than its ISIZE)
enum InflateStatus : uint32_t { kInfOk = 0, kInfBadData = 1, kInfInsufficientSpace = 2, kInfShortOutput = 3 };
// Why the decode / copy pair handed a member to k_inflate (gzpx_inflate_seg.h): recorded per member by the debug
// instances of k_inflate_seg and k_lzcopy only, read back by gzpx_debug_inflate_handback (GZPX_HANDBACK_*).
enum InflateHandback : uint32_t {
    kHbNone = 0,           // the pair decoded the member (or never looked at it: ISIZE 0, no room in the output)
    kHbHeader = 1,         // seg_header refused the block header: block type 3, the shape of a code, the header's runs,
                           // no end-of-block code, stored LEN / NLEN, or the payload ends inside the header
    kHbStored = 2,         // a stored block reaches past the payload or past ISIZE
    kHbNoEob = 3,          // the payload ends and the block has not
    kHbResync = 4,         // pass 2 took more than kSegMaxFix iterations
    kHbSpanSymbol = 5,     // the span's true path stops at something that is no end-of-block code
    kHbSpanOverrun = 6,    // the span's output overruns ISIZE, or its exit lies behind the payload
    kHbDistance = 7,       // pass 3: a distance reaches in front of the output's start
    kHbOffsetSymbol = 8,   // pass 3: an invalid offset codeword behind a length
    kHbCodeword = 9,       // pass 3: an invalid litlen codeword (litlen 286 and 287 are among them)
    kHbCountMismatch = 10, // pass 3, count-only: the walk from the true entry disagrees with pass 2
    kHbFinal = 11,         // behind the final block: fewer bytes than ISIZE, or the stream ends behind the payload
    kHbLzcopy = 12,        // k_lzcopy gave up (its polling loop ran out of spins)
};
// Scratch of the two-kernel inflate (gzpx_inflate_seg.h): the members' match records, the first record of every
// 32 KiB output tile, and the list of members handed back to k_inflate ([0] = how many).
struct InflateScratch {
    void *mlist = nullptr;       // inflate_mlist_bytes(out_cap, nb)
    uint32_t *tfirst = nullptr;  // inflate_tfirst_bytes(out_cap, nb)
    uint32_t *redo = nullptr;    // [1 + nb] the list, [1 + nb] behind it k_inflate_seg's ticket counter, [2 + nb + b]
                                 // member b's InflateHandback (debug launches; room for 2 + 2 nb words)
    uint32_t *summary = nullptr; // [kDsWords] the launch record below
    int n_cu = 0;                // compute units of the device (the size of the persistent launch)
    uint64_t in_bytes = 0;       // compressed bytes that stand for the members' total: launch_inflate_members takes their
                                 // average per member to choose k_inflate_seg's launch form (kSegBigBytes)
};
// The record of a launch (InflateScratch.summary, u32 words), 64 bytes of which the host reads the first 48 or 32.
// k_dsummary (the framed paths): the first failing member in stream order as a quadruple -- its index (0xFFFFFFFF:
// none), its InflateStatus, the CRC found, the CRC expected -- once under the framed rule (strict: fewer bytes than
// ISIZE is a failure) and once under the libdeflate-shaped call's (lenient); then the bytes member 0 produced.
enum { kDsFirst = 0, kDsStatus = 1, kDsFound = 2, kDsExpected = 3 };  // the fields of a quadruple
enum { kDsStrict = 0, kDsLenient = 4, kDsProduced0 = 8, kDsHostWords = 12 };
// k_dresult (a batch, gzpx_wrap.h): the first failing member (0xFFFFFFFF: none), its GZPX_* status, found, expected,
// how many failed, [6..7] the sum of the slots
enum { kWrRecFirst = 0, kWrRecStatus = 1, kWrRecFound = 2, kWrRecExpected = 3, kWrRecFailed = 4, kWrRecTotal = 6, kWrRecHostWords = 8 };
// behind both, and nobody's to read on the host: where a member's first block ended, per mille -- k_inflate_seg's
// guess for the next members, kept from launch to launch
enum { kDsSegHint = 15, kDsWords = 16 };
enum { kInflateRouteSeg = 0, kInflateRouteWave = 1 };  // k_inflate_seg + k_lzcopy (default) | k_inflate for every member
size_t inflate_mlist_bytes(uint64_t out_cap, uint64_t nb);
size_t inflate_tfirst_bytes(uint64_t out_cap, uint64_t nb);
// What the three inflate launches below have in common: each adds the tables that are its own.
struct InflateLaunch {
    const uint8_t *d_in = nullptr;  // the compressed bytes the tables point into
    uint32_t nb = 0;                // members
    void *d_blk = nullptr;          // [nb] their records (DBlockHost)
    uint64_t *d_out_off = nullptr;  // [nb + 1] where each member's output starts in d_out, the total
    uint8_t *d_out = nullptr;       // [out_cap] (the sizes call: no offsets, no output, a capacity of 0)
    uint64_t out_cap = 0;
    uint32_t *d_check = nullptr;    // [nb] the checksum found for each member
    int debug = 0;                  // which kernels carry their clocks (launch_inflate_members, gzpx_kernels.hip)
    int route = kInflateRouteSeg;
    // optional; recorded in front of the members' kernels, behind k_inflate_seg (the decode / copy route alone), behind
    // the members' kernels, and behind the check kernel (launch_inflate_batch alone)
    hipEvent_t ev_begin = nullptr, ev_mid = nullptr, ev_end = nullptr, ev_check = nullptr;
    hipStream_t stream = nullptr;
    const InflateScratch *sc = nullptr;
    const CrcConsts *cc = nullptr;
};
// The framed members of a stream (the header is hdr_len bytes), listed by d_offsets / d_sizes; sc.summary gets
// k_dsummary's record (kDs*).
void launch_inflate(const InflateLaunch &l, uint32_t hdr_len, const uint64_t *d_offsets, const uint32_t *d_sizes);

// A batch of independent members in a raw / zlib / gzip wrapper (gzpx_wrap.h): the table and every result in device
// memory; sc.summary gets k_dresult's record (kWrRec*).
void launch_inflate_batch(const InflateLaunch &l, int wrap, int short_ok, uint64_t in_len, const uint64_t *d_offsets,
                          const uint32_t *d_sizes, const uint32_t *d_out_sizes, uint32_t *d_slot, uint64_t *d_user_off,
                          void *d_results);

// The sizes of such a batch (gzpx_inflate_batch_sizes_device): the count-only inflate kernels; d_out_sizes [nb] is
// written, d_in_used [nb] and d_results [nb] if given, sc.summary gets k_dresult_sizes' record (kWrRec*, [6..7] the sum
// of the good members' sizes).  Of `sc` only redo, summary, n_cu and in_bytes are used.  max_out 0: no cap below 2^32.
void launch_inflate_sizes(const InflateLaunch &l, int wrap, uint64_t in_len, const uint64_t *d_offsets, const uint32_t *d_sizes,
                          uint32_t max_out, uint32_t *d_out_sizes, uint32_t *d_in_used, void *d_results);

// Checksums of a table of buffers (gzpx_cksum.h, gzpx_checksum_batch_device): CRC-32 / Adler-32 / CRC-32C (`kind`:
// GZPX_CHECK_*) of n entries of d_in -- entry i is [off[i], off[i] + size[i]), or [off[i], off[i + 1]) with d_sizes null.
// Every table is device memory; s.rec gets the record (kWrRec*, [6..7] zero).  `workgroups`: the persistent launch,
// cksum_workgroups(n_cu, 0) unless a test asks for another width; s.carry holds two words for each of them.
struct CksumScratch {
    uint64_t *prefix = nullptr;  // [n + 1] exclusive scan of the entries' tiles
    uint32_t *part = nullptr;    // [n]     the term of an entry that one workgroup took whole; then its sum
    uint32_t *carry = nullptr;   // [2 * workgroups] the terms of entries that reach across workgroups
    uint32_t *rec = nullptr;     // the launch record (a slot's summary)
};
uint32_t cksum_workgroups(int n_cu, uint32_t width);
void launch_cksum_batch(int kind, const uint8_t *d_in, uint64_t in_len, const uint64_t *d_offsets, const uint32_t *d_sizes,
                        uint32_t n, const uint32_t *d_seeds, const uint32_t *d_expected, uint32_t *d_sums, void *d_results,
                        const CksumScratch &s, uint32_t workgroups, hipStream_t stream);

// Member discovery on the device (gzpx_mscan.h): the candidate headers of a stream, sorted by position, and what the
// chain from offset 0 makes of them.
struct MemberScanScratch {
    uint32_t *seg_count = nullptr;  // [segments] candidates in each segment of the stream
    uint32_t *seg_off = nullptr;    // [segments] their exclusive prefix sum
    uint64_t *pos = nullptr;        // [cap] candidate positions
    uint32_t *size = nullptr;       // [cap] the member sizes their headers state
    uint32_t *succ = nullptr;       // [cap] index of the candidate at pos + size, or a terminal
    uint32_t *jump[2] = {nullptr, nullptr};  // [cap] pointer doubling, ping-pong
    uint32_t *idx = nullptr;        // [cap] index in the walk from offset 0, 0xFFFFFFFF for impostors
    uint32_t *rec = nullptr;        // [8] the scan record: candidates, members, kind of end, consumed (u64 at [4])
    uint32_t cap = 0;
};
void launch_member_scan(int format, const uint8_t *d_in, uint64_t in_len, uint32_t seg_bytes, uint32_t n_seg,
                        uint32_t rounds, const MemberScanScratch &m, hipStream_t stream);
void launch_member_emit(const MemberScanScratch &m, uint32_t n_emit, uint64_t *d_offsets, uint32_t *d_sizes,
                        hipStream_t stream);
void launch_member_index(const uint8_t *d_in, const uint64_t *d_offsets, const uint32_t *d_sizes, uint32_t nb, void *d_blk,
                         uint64_t *d_out_off, hipStream_t stream);

// Random access by range (gzpx_ranges.h).  The index of a stream, in device memory:
struct RrIndex {
    const uint64_t *off;     // [n]     member starts in the compressed stream
    const uint32_t *size;    // [n]     member sizes
    const uint64_t *ustart;  // [n + 1] exclusive prefix sum of ISIZE: member starts in the inflated stream, the total
    uint32_t n;
};
// the record of locate + select (RangeScratch.rec, u32 words): [0] the first invalid range (0xFFFFFFFF: none),
// [1] members selected, [2..3] the sum of their ISIZE = bytes of staging, [4..5] bytes of output
enum { kRrRecBad = 0, kRrRecSelected = 1, kRrRecStage = 2, kRrRecTotal = 4 };
struct RangeScratch {
    uint64_t *ranges = nullptr;   // [2 * ranges] the caller's (begin, end) pairs
    uint32_t *first = nullptr;    // [ranges]     the first member a range reads
    uint64_t *len = nullptr;      // [ranges]     its length in bytes
    uint64_t *src = nullptr;      // [ranges]     where its bytes start in staging
    uint64_t *out_off = nullptr;  // [ranges + 1] where they go in the output
    uint32_t *diff = nullptr;     // [members + 1] +1 / -1 where the spans [first, last] begin / end
    uint32_t *map = nullptr;      // [members]    rank in the selection -> index in the stream
    uint64_t *soff = nullptr;     // [members]    where a selected member starts in staging
    uint32_t *rec = nullptr;      // [8]
};
// locate + select: fills the compacted member table (d_sel_off / d_sel_size, room for ix.n) and r.rec
void launch_ranges_select(const RrIndex &ix, uint32_t n_ranges, int virt, const RangeScratch &r, uint64_t *d_sel_off,
                          uint32_t *d_sel_size, hipStream_t stream);
// the ranges' bytes from staging (16 readable bytes behind its last) to d_out, back to back
void launch_ranges_gather(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, uint8_t *d_out, uint64_t total,
                          hipStream_t stream);

// Reads by line (gzpx_lines.h).  The table of a stream, in device memory: P[t] = delimiters in front of tile t of the
// inflated stream (tiles of kLnTile bytes); D delimiters, L lines, `total` inflated bytes.
constexpr uint32_t kLnTile = 16384;  // GZPX_LINES_TILE
struct LnTable {
    const uint64_t *P;  // [tiles + 1]
    uint32_t tiles;
    uint64_t D, L, total;
};
// the records (u32 words): a table's own holds [1] whether the stream's last byte is a delimiter, [2..3] D, [4..5] L;
// a search's holds [0] the first invalid boundary or range (0xFFFFFFFF: none) and [6..7] the bytes of output
enum { kLnRecBad = 0, kLnRecLast = 1, kLnRecD = 2, kLnRecL = 4, kLnRecTotal = 6 };
struct LinesScratch {
    uint64_t *bounds = nullptr;  // [boundaries] the caller's line numbers; of a read, (a, b) of every line range
    uint32_t *btile = nullptr;   // [boundaries] the tile a boundary lies in, 0xFFFFFFFF where none has to be walked
    uint64_t *bpos = nullptr;    // [boundaries] start(k); of a read, (begin, end) of every range in bytes
    uint32_t *rec = nullptr;     // [8]
};
// the delimiters of staging = inflated bytes [base, base + len) of a stream of `total`, added to the tiles' counters
void launch_lines_count(const uint8_t *d_stage, uint64_t base, uint64_t len, uint64_t total, uint32_t delim, uint32_t *d_cnt,
                        uint32_t *d_rec, hipStream_t stream);
void launch_lines_prefix(const uint32_t *d_cnt, uint32_t tiles, uint64_t total, uint64_t *d_prefix, uint32_t *d_rec,
                         hipStream_t stream);
// n items of `per` boundaries each (1: line numbers, 2: line ranges): l.rec is cleared, every item validated and its
// cover written to r.ranges, for launch_ranges_select (n ranges, uncompressed coordinates) and launch_inflate
void launch_lines_tiles(const LnTable &tb, uint32_t n, uint32_t per, const LinesScratch &l, const RangeScratch &r,
                        hipStream_t stream);
// behind the inflate of the selection into d_stage: l.bpos of every boundary; per == 2: then r.src / r.out_off in the
// form launch_ranges_gather takes, and the total in l.rec
void launch_lines_find(const LnTable &tb, uint32_t n, uint32_t per, uint32_t delim, const LinesScratch &l, const RangeScratch &r,
                       const uint8_t *d_stage, hipStream_t stream);

// Search (gzpx_find.h).  Staging of a batch: kFdPad bytes, of which the last `carry` are the end of the earlier
// batches, then the batch's `len` inflated bytes (16 readable bytes behind them); `base` is where the batch starts in
// the inflated stream.  The region [kFdPad - carry, kFdPad + len) is searched in pieces of kFdPiece bytes of staging.
constexpr uint32_t kFdMaxPattern = 256;  // GZPX_FIND_MAX_PATTERN
constexpr uint32_t kFdPad = 256;
constexpr uint32_t kFdPiece = 16384;
// the record (u64 words): hits and delimiters of the batches so far, and how many of those delimiters lie in the carry
enum { kFdRecHits = 0, kFdRecDelims = 1, kFdRecCarry = 2, kFdRecWords = 4 };
struct FindScratch {
    uint32_t *pat = nullptr;    // [kFdMaxPattern / 4] the pattern, the tail zero
    uint32_t *cnt = nullptr;    // [2 * pieces] (hits, delimiters) of every piece of a batch
    uint64_t *bases = nullptr;  // [2 * pieces] (rank of the first hit, delimiters in front) of every piece
    uint64_t *rec = nullptr;    // [kFdRecWords]
};
struct FindBatch {
    uint8_t *stage;
    uint64_t base, len;
    uint32_t carry, m;
    int delim;  // -1: no line numbers
};
inline uint64_t find_pieces(uint64_t len) { return (kFdPad + len + kFdPiece - 1u) / kFdPiece; }  // of a batch, at most
// which matcher a pass runs: the pattern in f.pat (d_set null), or a compiled set (gzpx_findset.h) and its counters
struct FsSet;
struct FindMatcher {
    const FsSet *d_set = nullptr;
    uint64_t *d_counts = nullptr;  // [kFsMaxPatterns] the counting pass adds the hits of pattern k to d_counts[k]
};
// count + scan of one batch (region not empty): f.cnt, f.bases and the record
void launch_find_count(const FindBatch &b, const FindScratch &f, const FindMatcher &mt, hipStream_t stream);
// behind launch_find_count: the batch's hits below rank `cap` into d_positions / d_ids / d_lines (each may be null; one
// pattern: no ids)
void launch_find_write(const FindBatch &b, const FindScratch &f, const FindMatcher &mt, uint64_t *d_positions, uint32_t *d_ids,
                       uint64_t *d_lines, uint64_t cap, hipStream_t stream);
// behind both: the last `n` <= m - 1 bytes of the region become the next batch's carry
void launch_find_carry(const FindBatch &b, const FindScratch &f, uint32_t n, hipStream_t stream);

// Selection of lines by content (gzpx_select.h).  The record bitmap holds one bit per record of `group` lines; behind
// the last batch its runs of set (INVERT: clear) bits are counted kSlRunRecords records a workgroup, the counts scanned
// kSlScanStep workgroups a step, and the runs written as line ranges.
constexpr uint32_t kSlRunRecords = 512;  // records per workgroup of k_sl_runs_count / k_sl_runs_write
constexpr uint32_t kSlScanStep = 256;    // workgroups of them per step of k_sl_runs_scan
// the record (u64 words): runs, selected records, hits
enum { kSlRecRuns = 0, kSlRecRecords = 1, kSlRecHits = 2, kSlRecWords = 4 };
struct SelectScratch {
    uint32_t *bitmap = nullptr;  // [(records + 31) / 32] bit r: a hit's line lies in record r
    uint32_t *cnt = nullptr;     // [2 * groups] (rising edges, set bits) of every kSlRunRecords records
    uint32_t *bases = nullptr;   // [groups] the rank of a group's first rising edge
    uint64_t *rec = nullptr;     // [kSlRecWords]
};
inline uint64_t select_groups(uint64_t n_records) { return (n_records + kSlRunRecords - 1u) / kSlRunRecords; }
// behind launch_find_count of a batch with a delimiter: the records of the batch's hits into s.bitmap
void launch_select_mark(const FindBatch &b, const FindScratch &f, const FindMatcher &mt, const SelectScratch &s, uint64_t group,
                        uint64_t n_records, hipStream_t stream);
// behind the last batch (n_records > 0): s.rec, and the runs below rank `cap` into d_runs (null: counts only) as
// (begin, end) pairs of line numbers
void launch_select_runs(const SelectScratch &s, const FindScratch &f, uint64_t n_records, uint64_t group, uint64_t n_lines,
                        int invert, uint64_t *d_runs, uint64_t cap, hipStream_t stream);

// Fields of lines (gzpx_fields.h): behind a line search of line ranges (launch_lines_find, per == 2) the ranges' bytes
// lie in staging, range r at r.src[r] with r.out_off[r + 1] - r.out_off[r] bytes.  They are cut on the 16 KiB grid of
// staging into PIECES, the pieces of all ranges numbered in one row; three passes over them (carry, count, write) keep
// the bytes of the selected fields.  The host compiles the field list into an FlSet: the field numbers at which
// membership in S changes, ascending, field 0 outside S; n of them, the rest of the array UINT64_MAX.
constexpr uint32_t kFlPiece = 16384;
constexpr uint32_t kFlMaxRanges = 64;                  // GZPX_FIELDS_MAX_RANGES
constexpr uint32_t kFlBounds = 2u * kFlMaxRanges + 8u;  // 129 changes at most (64 ranges, complemented), and sentinels
struct FlSet {
    uint64_t b[kFlBounds];
    uint64_t n;
};
// the record (u64 words): bytes of output, pieces
enum { kFlRecTotal = 0, kFlRecPieces = 1, kFlRecWords = 4 };
struct FieldsScratch {
    FlSet *set = nullptr;         // the compiled field list
    uint64_t *pfirst = nullptr;   // [ranges + 1] the first piece of every range; [ranges] = the pieces
    uint64_t *out_off = nullptr;  // [ranges + 1] where every range's output starts (a caller's device array takes its place)
    uint32_t *carry = nullptr;    // [pieces] of a piece: bit 31 it holds a line delimiter or is a range's first, bit 30 it is a
                                  //          range's first, below them the field delimiters behind its last line delimiter
    uint64_t *cin = nullptr;      // [pieces] the field number of a piece's first byte
    uint32_t *cnt = nullptr;      // [pieces] the bytes a piece keeps
    uint64_t *obase = nullptr;    // [pieces + 1] where they go in the output
    uint64_t *rec = nullptr;      // [kFlRecWords]
};
// the pieces of n_ranges ranges that hold `total` bytes, at most: a range of len > 0 bytes touches at most len / 16 KiB + 2
inline uint64_t fields_pieces(uint64_t total, uint64_t n_ranges) { return total / kFlPiece + 2u * n_ranges; }
// the pieces, the carries and their scan: f.pfirst, f.carry, f.cin
void launch_fields_carry(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const FieldsScratch &f, uint32_t delim,
                         uint32_t field_delim, uint32_t grid, hipStream_t stream);
// behind it: f.cnt, f.obase, d_out_off[n_ranges + 1] and the record
void launch_fields_count(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const FieldsScratch &f, uint32_t delim,
                         uint32_t field_delim, uint32_t grid, uint64_t *d_out_off, hipStream_t stream);
// behind both: the kept bytes to d_out, unless the record's total exceeds out_cap
void launch_fields_write(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const FieldsScratch &f, uint32_t delim,
                         uint32_t field_delim, uint32_t grid, uint8_t *d_out, uint64_t out_cap, hipStream_t stream);

// Numeric columns of lines (gzpx_columns.h): behind the same line search, the pieces and cin of launch_fields_carry,
// then a row number per piece and one parsing pass that stores a cell and a status byte per (column, row).
constexpr uint32_t kClMaxCols = 16;    // GZPX_COLUMNS_MAX
constexpr uint32_t kClMaxBytes = 64;   // GZPX_CELL_MAX_BYTES
constexpr uint32_t kClOverhang = 80;   // bytes behind a piece that k_cl_parse stages: a field opened by the piece's last byte
struct ClCols {
    uint64_t field[kClMaxCols];  // ascending; UINT64_MAX behind the n in use
    uint32_t type[kClMaxCols];   // GZPX_COL_*
    uint32_t n, pad;
};
// the record (u64 words): rows, cells that are not OK, then the same count per column
enum { kClRecRows = 0, kClRecNotOk = 1, kClRecCol = 2, kClRecWords = 2 + kClMaxCols };
struct ColumnsScratch {
    FieldsScratch fl;             // pfirst, carry, cin and k_fl_plan's record; the rest of it stays null
    ClCols *cols = nullptr;       // the column list
    uint32_t *rcnt = nullptr;     // [pieces] the line delimiters of a piece
    uint64_t *rin = nullptr;      // [pieces] the lines of its range in front of a piece's first byte
    uint64_t *row_off = nullptr;  // [ranges + 1] rbase (a caller's device array takes its place)
    uint64_t *rec = nullptr;      // [kClRecWords]
};
// behind launch_fields_carry on c.fl: c.rcnt, c.rin, d_row_off[n_ranges + 1] and the record's rows; the record is cleared
// first.  l.bounds holds the (begin, end) line numbers of the ranges.
void launch_columns_rows(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const LinesScratch &l,
                         const ColumnsScratch &c, uint32_t delim, uint32_t field_delim, uint32_t grid, uint64_t *d_row_off,
                         hipStream_t stream);
// behind it: the cells to d_values / d_status (either may be null), unless one is given and the rows exceed rows_cap; the
// counts of cells that are not OK into the record
void launch_columns_parse(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const ColumnsScratch &c, uint32_t delim,
                          uint32_t field_delim, uint32_t grid, const uint64_t *d_row_off, uint64_t *d_values, uint8_t *d_status,
                          uint64_t rows_cap, hipStream_t stream);

// Selection of lines by their numbers (gzpx_where.h): the columns' stages with the distinct fields of the terms as the
// column list, the parse testing every cell against the terms of its column instead of storing it, then the runs of the
// row bitmap, cut at every range's first row.  The host compiles the terms into a WhTerms; the terms of column c are
// [first[c], first[c + 1]), in the caller's order.
constexpr uint32_t kWhMaxTerms = 32;  // GZPX_WHERE_MAX_TERMS
enum { kWhLt = 0, kWhLe = 1, kWhEq = 2, kWhNe = 3, kWhGe = 4, kWhGt = 5, kWhIsOk = 6, kWhNotOk = 7 };  // GZPX_WHERE_*
struct WhTerms {
    uint64_t value[kWhMaxTerms];
    uint32_t op[kWhMaxTerms];
    uint32_t first[kClMaxCols + 1u];
    uint32_t any;  // 1: a cell that makes a term TRUE marks its row; 0: one that makes a term FALSE does
};
// Terms on the TEXT of a field (gzpx_where_text_device).  A TEXT column's cell is the field's bytes where the walk staged
// them; a TEXT term's value is offset | len << 32 into the pool of constants.  A constant of c <= kWhTextMax bytes is
// decided by the field's first c + 1 bytes, which kClOverhang keeps in LDS behind the piece whatever byte opens the field.
constexpr uint32_t kClText = 2;         // GZPX_COL_TEXT
constexpr uint32_t kWhTextMax = 64;     // GZPX_WHERE_TEXT_MAX
constexpr uint32_t kWhPoolMax = 2048;   // GZPX_WHERE_TEXT_POOL_MAX
enum { kWhPrefix = 8, kWhNotPrefix = 9 };  // GZPX_WHERE_PREFIX, GZPX_WHERE_NOT_PREFIX
static_assert(kWhTextMax == kClMaxBytes && kClOverhang >= kWhTextMax + 1u && kWhPoolMax == kWhMaxTerms * kWhTextMax,
              "a constant is decided inside the overhang; every term may bring a constant of its own");
struct WhTextTerms {
    WhTerms t;          // (first: the numeric-only parse reads this much and no more)
    uint32_t pool_len;  // the bytes of the pool in use
    uint32_t pad;
    uint8_t pool[kWhPoolMax];
};
// the record (u64 words): runs, selected rows, rows, cells that are not OK
enum { kWhRecRuns = 0, kWhRecSelected = 1, kWhRecRows = 2, kWhRecNotOk = 3, kWhRecWords = 4 };
struct WhereScratch {
    ColumnsScratch cl;           // the columns' stages: every member but the arrays of cells
    WhTextTerms *terms = nullptr;  // the compiled terms (its head is the WhTerms of a call without TEXT terms)
    uint32_t *bitmap = nullptr;  // [bits / 32] bit i: a cell of row i decided its row (rejected it, or under ANY accepted it)
    uint32_t *starts = nullptr;  // [bits / 32] bit i: row i is the first of its range; it lies behind bitmap, one memset clears both
    uint32_t *cnt = nullptr;     // [2 * groups] (rising edges, set bits) of every kSlRunRecords rows
    uint32_t *bases = nullptr;   // [groups] the rank of a group's first rising edge
    uint64_t *rec = nullptr;     // [kWhRecWords]
};
// the bits of a bitmap that serves `bound` rows: whole groups of the runs kernels
inline uint64_t where_bits(uint64_t bound) { return select_groups(bound) * kSlRunRecords; }
// behind launch_columns_rows on w.cl: both bitmaps cleared (`bits` = where_bits()), then the parse with the predicate;
// nothing is marked when the record's rows exceed `bits`.  `text`: a term is on a TEXT column, and w.terms holds the pool.
void launch_where_parse(const uint8_t *d_stage, uint32_t n_ranges, const RangeScratch &r, const WhereScratch &w, uint32_t delim,
                        uint32_t field_delim, uint32_t grid, const uint64_t *d_row_off, uint64_t bits, bool text, hipStream_t stream);
// behind it: w.rec, and the runs below rank `cap` into d_runs (null: counts only) as (begin, end) pairs of line numbers.
// `invert`: the selected rows are those whose bit is clear.  l.bounds holds the (begin, end) line numbers of the ranges.
void launch_where_runs(uint32_t n_ranges, const LinesScratch &l, const WhereScratch &w, const uint64_t *d_row_off, uint64_t bits,
                       int invert, uint64_t *d_runs, uint64_t cap, hipStream_t stream);

// Search for a set of patterns (gzpx_findset.h).  The host compiles the set into an FsSet, the form the kernels stage
// into LDS: q = min(shortest pattern, 4); the WINDOW of a pattern is its first q bytes as a little-endian number.
constexpr uint32_t kFsMaxPatterns = 256;  // GZPX_FINDSET_MAX_PATTERNS
constexpr uint32_t kFsMaxBytes = 16384;   // GZPX_FINDSET_MAX_BYTES
constexpr uint32_t kFsBitmapWords = 2048;  // 2^16 bits
constexpr uint32_t kFsByteWords = (kFsMaxBytes + 3u * kFsMaxPatterns) / 4u;  // every pattern starts on a dword
enum { kFsHdrK = 0, kFsHdrQ = 1, kFsHdrM = 2, kFsHdrGrams = 3, kFsHdrBitmapWords = 4, kFsHdrByteWords = 5, kFsHdrWords = 8 };
struct alignas(16) FsSet {
    uint32_t hdr[kFsHdrWords];        // patterns, q, the longest pattern, distinct windows, words in use of bitmap and bytes
    uint32_t bitmap[kFsBitmapWords];  // bit fs_gram_index(window): some pattern starts with it (q = 1: 8 words in use)
    uint32_t keys[kFsMaxPatterns];    // the distinct windows, ascending
    uint32_t bstart[kFsMaxPatterns + 4u];  // bucket g = ids[bstart[g] .. bstart[g + 1]): the patterns of window keys[g]
    uint32_t ids[kFsMaxPatterns];     // ... ids ascending inside a bucket
    uint32_t meta[kFsMaxPatterns];    // of pattern k: (its first word in bytes) << 16 | its length
    uint32_t bytes[kFsByteWords];     // the patterns, each padded with zeros to a whole dword
};
static_assert(sizeof(FsSet) % 16u == 0, "staged as 16-byte words");
// where the filter keeps the bit of a window of q bytes
constexpr uint32_t fs_gram_index(uint32_t window, uint32_t q) { return q <= 2u ? window : (window * 0x9E3779B1u) >> 16; }
// The set's passes over one batch are the search's (launch_find_count, launch_find_write, launch_select_mark) with
// FindMatcher::d_set given.  b.m says which starts the batch owns: the longest pattern for a batch that is not the last,
// 1 for the last (gzpx_findset.h).

// gzpx_wrap.h (k_adler32_tiles): (s1, s2, n) of every 64 KiB tile of d_in[0..n) -> d_out3[3 * tile + ..]
void launch_adler32(const uint8_t *d_in, uint64_t n, uint32_t *d_out3, hipStream_t stream);

}  // namespace gzpx
