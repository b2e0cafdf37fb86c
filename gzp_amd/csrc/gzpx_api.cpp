// gzpx_api.cpp -- the C ABI of include/gzpx.h over the HIP pipeline of gzpx_kernels.hip.
//
// Host-side mirror of what a gzp worker thread does per block (src/par/compress.rs:279-294:
// create_compressor once, encode per block) lifted to whole slabs: one call = every block of the
// slab through the kernel pipeline, blocks cut and ordered exactly like ParCompress::write /
// flush_last (src/par/compress.rs:413-463, 332-362).  No CPU fallback exists on purpose: without
// a HIP device every entry point fails with GZPX_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <new>
#include <string.h>
#include <vector>

#include "../../include/gzpx.h"
#include "gzpx_device.h"
#include "gzpx_own.h"

using namespace gzpx;

namespace {

constexpr size_t kDictSize = 32768;  // DICT_SIZE, src/lib.rs:108
constexpr uint32_t kMaxBatchBlocks = 16384;
constexpr size_t kMaxScratchBytes = (size_t)24 << 30;  // per-context cap of the per-block scratch

// ---- CRC-32 combination over the host half of gzpx_crc.h: sq[k] = x^(8 * 2^k) mod P
#include "gzpx_crc.h"
const CrcPow kCrc32Pow = crc_pow_table<kCrcPoly32>();

// crc(A || B) = crc(A) * x^(8 |B|) mod P  xor  crc(B)
uint32_t crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) {
    return crc_mulmod<kCrcPoly32>(crc_xpow8<kCrcPoly32>(kCrc32Pow.sq, len2), crc1) ^ crc2;
}

#include "gzpx_policy.h"  // kMinBlockLen, kFastSeqStoreLen, level_params

constexpr size_t kTrailerBytes = 8;  // CRC-32 + ISIZE behind a member's payload
// BGZF's end-of-file marker, an empty member: header + the two bytes of an empty static block + trailer
constexpr size_t kEofMarkerBytes = header_bytes(GZPX_FORMAT_BGZF) + 2 + kTrailerBytes;

CrcConsts crc_consts() {
    CrcConsts cc;
    for (unsigned l = 0; l < 10; l++) cc.pow64[l] = kCrc32Pow.sq[6 + l];  // x^(8 * 64 * 2^l)
    cc.pow_tile = kCrc32Pow.sq[16];                                       // x^(8 * 65536)
    return cc;
}

// The stages of gzpx_ctx_last_stage_ms, in pipeline order (include/gzpx.h).  A Snap context fills kStMatch
// (k_snap_chunk), kStScan (k_snap_frame + k_scan) and kStEmit (k_snap_emit).
enum Stage : int { kStInitMeta, kStCandidates, kStMatch, kStParse, kStHist, kStHuffman, kStCrc32, kStScan, kStEmit, kNStages };
static_assert(kNStages == GZPX_N_STAGES, "the stage enum and include/gzpx.h disagree");

constexpr int kProfPairs = 64;  // launch groups of one batch that measurement mode can bracket
// measurement mode: the timing events of a context and the groups of the batch enqueued last
struct ProfLog {
    Event ev[2 * kProfPairs];                // begin / end of launch groups
    Stage stage[kProfPairs] = {};
    int b[kProfPairs] = {0}, e[kProfPairs] = {0};  // a group's begin / end event (indices into ev)
    int n = 0;
};

constexpr int kSlots = 3;  // slabs of one context that may be in flight (copy in / kernels / copy out)

// ---- what gzpx_ctx and gzpx_dctx do alike.  Both keep `slots[kSlots]` (state: 0 free, 1 submitted, 2 a thread is
// inside wait(); gen: which job), `next_gen`, and `mu` + `cv_slot` for them.

// The first free slot, with the context's mutex held through `lk`.  None: waits for one (the wait lets go of the
// mutex), or returns -1 at once.
template <class Ctx>
int free_slot(Ctx *c, std::unique_lock<std::mutex> &lk, bool wait) {
    for (;;) {
        for (int i = 0; i < kSlots; i++)
            if (c->slots[i].state == 0) return i;
        if (!wait) return -1;
        c->cv_slot.wait(lk);
    }
}

// slot si holds a submitted job from here on: its ticket (mutex held)
template <class Ctx>
uint64_t issue_ticket(Ctx *c, int si) {
    c->slots[si].state = 1;
    c->slots[si].gen = c->next_gen++;
    return (c->slots[si].gen << 8) | (uint64_t)si;
}

// the slot of a ticket whose job is submitted and not being waited for, else -1 (mutex held)
template <class Ctx>
int ticket_slot(Ctx *c, uint64_t ticket) {
    const int si = (int)(ticket & 0xFF);
    return si < kSlots && c->slots[si].state == 1 && c->slots[si].gen == (ticket >> 8) ? si : -1;
}

// ... which the calling thread now waits for
template <class Ctx>
int claim_ticket(Ctx *c, uint64_t ticket) {
    std::lock_guard<std::mutex> lk(c->mu);
    const int si = ticket_slot(c, ticket);
    if (si >= 0) c->slots[si].state = 2;
    return si;
}

// A device job's buffers are ready once the caller's stream `after` has reached this point: `stream`, one of a
// context's own, waits for it.  NULL is the legacy default stream (PyTorch's current stream unless told otherwise) --
// the contexts' streams are non-blocking, so nothing orders them behind it implicitly.  Nothing to do for the stream
// itself and for GZPX_STREAM_NONE.
int order_behind(hipStream_t stream, hipStream_t after, hipEvent_t ev_dep) {
    if (after == stream || after == (hipStream_t)GZPX_STREAM_NONE) return GZPX_OK;
    HIP_TRY(hipEventRecord(ev_dep, after));
    HIP_TRY(hipStreamWaitEvent(stream, ev_dep, 0));
    return GZPX_OK;
}

// A call that fails may already have put copies and kernels on its streams: nothing of them may still be running
// when the caller gets its buffers back, the next call reuses a slot's staging, or an owner frees what they work on.
// Armed behind the points that return without having enqueued anything (BUSY, INVALID_ARG); disarmed on success.
struct Drain {
    hipStream_t s[4];
    int n;
    bool armed = true;
    ~Drain() {
        for (int i = 0; armed && i < n; i++) (void)hipStreamSynchronize(s[i]);
    }
};

// One slab in flight.  Host-buffer jobs own a pair of device staging buffers per slot, so the H2D
// copy of slab k+1 and the D2H copy of slab k-1 run (on their own streams) while the kernels of
// slab k occupy the compute stream.
struct Slot : NoCopy {
    int state = 0;  // 0 free, 1 submitted, 2 a thread is inside wait()
    uint64_t gen = 0;
    Event ev_h2d, ev_kernels, ev_d2h;  // (created with the slot's first job)
    Event ev_dom_b, ev_dom_e;          // profiling mode 2: around the dominant stage of this job (timing enabled)
    bool dom_timed = false;            // ... recorded for this job (read back in wait)
    uint8_t *d_in = nullptr, *d_out = nullptr;  // staging of host-buffer jobs (grown on demand)
    size_t d_in_cap = 0, d_out_cap = 0;
    Allocs in_mem, out_mem;
    SlabResult *d_results = nullptr, *h_results = nullptr;  // one per batch of the slab (h_: pinned)
    size_t results_cap = 0;
    Allocs results_mem;
    uint32_t *h_sizes = nullptr;  // pinned: framed size of every block of the slab
    size_t sizes_cap = 0;
    Allocs sizes_mem;
    // the job
    uint8_t *job_d_out = nullptr;  // where the kernels wrote
    size_t job_out_cap = 0;
    uint8_t *host_out = nullptr;  // null: nothing for wait to copy out (device job; a shard of the multi-device call)
    size_t host_out_cap = 0;
    uint64_t total_nb = 0;
    uint32_t n_batches = 0;
};

}  // namespace

// (members are destroyed last to first: memory, then events, then streams)
struct gzpx_ctx : NoCopy {
    gzpx_config cfg;
    Config dcfg;
    CrcConsts crc_consts;
    Stream stream;  // compute: every kernel of this context, in submission order
    Stream s_h2d, s_d2h;
    Stream s_side;  // k_crc32 next to k_candidates (needs only the input); lowest priority
    Event ev_meta, ev_crc;        // fork / join of the side stream
    Event ev_crc_t0, ev_crc_t1;   // timing of k_crc32 when profiling
    Event ev_dep;  // "the caller's stream got this far" (device jobs)
    ProfLog prof;
    uint32_t batch_blocks = 0;
    Scratch scratch = {};
    SnapScratch snap = {};  // GZPX_FORMAT_SNAP only
    BlockMeta *h_meta = nullptr;  // pinned, one entry (debug hooks)
    SubMeta *h_sub = nullptr;     // pinned, max_sub entries (debug hooks)
    Allocs fixed;     // everything alloc_scratch allocates, but for ...
    Allocs lanes;     // ... scratch.no_*: the near-optimal lanes (retried with fewer of them)
    Allocs snap_dbg;  // snap.dbg, while gzpx_debug_snap has it enabled
    Slot slots[kSlots];
    uint64_t next_gen = 1;
    int profiling = 0;  // 0 off, 1 every stage, 2 the dominant stage only (two markers per batch instead of thirteen)
    float stage_ms[GZPX_N_STAGES] = {0};
    uint32_t last_nb = 0;
    char devname[256] = {0};
    std::mutex mu;
    std::condition_variable cv_slot;
};

namespace {

thread_local int t_last_status = GZPX_OK;  // libdeflate-shaped calls have no status channel

size_t extra_amount(size_t n) {  // src/bgzf.rs:45,50-52
    size_t e = (size_t)((double)n * 0.1);
    return e < 128 ? 128 : e;
}

// Snap: stream identifier + one 8-byte chunk header per 64 KiB + the chunk stored (src/snap.rs:61-74)
size_t snap_bound_per_block(size_t bs) { return 10 + bs + 8 * (size_t)snap_chunks_per_buffer((uint32_t)bs); }

size_t framed_bound_per_block(const gzpx_ctx *ctx) {
    if (ctx->cfg.format == GZPX_FORMAT_SNAP) return snap_bound_per_block(ctx->cfg.buffer_size);
    return header_bytes(ctx->cfg.format) + ctx->cfg.buffer_size + extra_amount(ctx->cfg.buffer_size) + kTrailerBytes;
}

// blocks a slab of in_len bytes is cut into (an empty slab is one empty block)
uint64_t blocks_of(size_t bs, size_t in_len) { return in_len == 0 ? 1 : (in_len + bs - 1) / bs; }

// bytes of device scratch one block needs (see gzpx_device.h Scratch)
size_t scratch_bytes_per_block(const Config &c) {
    return (size_t)c.stride * (2 + 1 + 2 + 4 + (c.level >= 2 ? 2 : 0) + (c.lazy ? 6 : 0)) + c.stride / 8 +
           (size_t)c.max_sub * (sizeof(SubMeta) + (kHistStride + kCodeWords + kHdrWords) * 4) +
           sizeof(BlockMeta) + 8 + 4;
}

// Snap: staging per chunk, and the arrays k_scan works on
size_t snap_scratch_bytes_per_block(size_t bs) {
    return (size_t)snap_chunks_per_buffer((uint32_t)bs) * (kSnapStageBytes + 3 * 4) + sizeof(BlockMeta) + 8 + 4;
}

int alloc_scratch(gzpx_ctx *ctx) {
    const size_t nb = ctx->batch_blocks;
    const Config &c = ctx->dcfg;
    Scratch &s = ctx->scratch;
    Allocs &a = ctx->fixed;
    GZPX_TRY(a.dev(s.meta, nb * sizeof(BlockMeta)));
    if (ctx->cfg.format == GZPX_FORMAT_SNAP) {
        SnapScratch &ss = ctx->snap;
        const size_t chunks = nb * snap_chunks_per_buffer((uint32_t)ctx->cfg.buffer_size);
        GZPX_TRY(a.dev(ss.stage, chunks * kSnapStageBytes));
        GZPX_TRY(a.dev(ss.clen, chunks * 4));
        GZPX_TRY(a.dev(ss.crc, chunks * 4));
        GZPX_TRY(a.dev(ss.coff, chunks * 4));
        GZPX_TRY(a.dev(s.out_off, (nb + 1) * sizeof(uint64_t)));
        GZPX_TRY(a.dev(s.sizes, nb * sizeof(uint32_t)));
        return GZPX_OK;
    }
    GZPX_TRY(a.pinned(ctx->h_meta, sizeof(BlockMeta)));
    GZPX_TRY(a.dev(s.sub, nb * (size_t)c.max_sub * sizeof(SubMeta)));
    GZPX_TRY(a.dev(s.cand, nb * (size_t)c.stride * sizeof(uint16_t)));
    GZPX_TRY(a.dev(s.len8, nb * (size_t)c.stride));
    GZPX_TRY(a.dev(s.which, nb * (size_t)(c.stride / 32) * 4));
    GZPX_TRY(a.dev(s.alt, nb * (size_t)c.stride * sizeof(uint16_t)));
    GZPX_TRY(a.dev(s.tok, nb * (size_t)c.stride * 4));
    GZPX_TRY(a.dev(s.redo, (nb + 1 + 8) * sizeof(uint32_t)));
    HIP_TRY(hipMemset(s.redo, 0, (nb + 1 + 8) * sizeof(uint32_t)));
    s.claim = s.redo + nb + 1;
    if (c.level >= 2) {  // hc_matchfinder levels: hash4 chain links + per-block parse state
        GZPX_TRY(a.dev(s.d4, nb * (size_t)c.stride * sizeof(uint16_t)));
        GZPX_TRY(a.dev(s.hc, nb * sizeof(HcState)));
        GZPX_TRY(a.dev(s.pending, 64));
    }
    if (c.lazy) {  // levels 5-9: the matches of the half / quarter depth searches
        GZPX_TRY(a.dev(s.lz_len, nb * 2 * (size_t)c.stride));
        GZPX_TRY(a.dev(s.lz_dist, nb * 2 * (size_t)c.stride * sizeof(uint16_t)));
    }
    if (c.level >= 10) {
        // levels 10-12: one lane per block in flight, each with its trees / cache / path nodes (gzpx_nearopt.hip);
        // as many as half the free HBM holds, 96 GiB at most (a BGZF block: 7.5 MiB); the lanes walk the batch's blocks
        const size_t per_lane = no_lane_bytes() + no_cache_bytes() + no_nodes_bytes(c.block_size);
        // (never more than half of what is free right now; if an allocation still fails -- fragmentation, another
        // context growing meanwhile -- the lane count is halved and tried again: fewer lanes are slower, not wrong)
        size_t free_b = 0, total_b = 0, budget = (size_t)12 << 30;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            if (free_b / 2 > budget) budget = free_b / 2 < ((size_t)96 << 30) ? free_b / 2 : ((size_t)96 << 30);  // (288 GB of HBM: up to 96 GiB of it)
            if (free_b / 2 < budget) budget = free_b / 2;
        }
        size_t lanes = budget / per_lane;
        if (lanes > nb) lanes = nb;
        if (lanes < 1) lanes = 1;
        Allocs &l = ctx->lanes;
        while (l.dev(s.no_state, lanes * no_lane_bytes()) != GZPX_OK || l.dev(s.no_cache, lanes * no_cache_bytes()) != GZPX_OK ||
               l.dev(s.no_nodes, lanes * no_nodes_bytes(c.block_size)) != GZPX_OK) {
            (void)hipGetLastError();
            l.release();
            if (lanes == 1) return GZPX_ERR_DEVICE;
            lanes = (lanes + 1) / 2;
        }
        s.no_lanes = (uint32_t)lanes;
        // libdeflate's default_litlen_costs[]: int(-log2((1 - p) / max(j, 1)) * 16), int(-log2(p / 29) * 16)
        uint8_t tables[3 * 258];
        static const double probs[3] = {0.25, 0.5, 0.75};
        for (int k = 0; k < 3; k++) {
            for (int j = 0; j <= 256; j++) tables[258 * k + j] = (uint8_t)(int)(-std::log2((1.0 - probs[k]) / (double)(j ? j : 1)) * 16);
            tables[258 * k + 257] = (uint8_t)(int)(-std::log2(probs[k] / 29.0) * 16);
        }
        uint8_t *d_tables = nullptr;
        Allocs tmp;  // (gone at the end of this block, on every path)
        GZPX_TRY(tmp.dev(d_tables, sizeof(tables)));
        HIP_TRY(hipMemcpy(d_tables, tables, sizeof(tables), hipMemcpyHostToDevice));
        launch_near_optimal_tables(s.no_state, s.no_lanes, d_tables, nullptr);
        HIP_TRY(hipDeviceSynchronize());
    }
    GZPX_TRY(a.dev(s.hist, nb * (size_t)c.max_sub * kHistStride * 4));
    GZPX_TRY(a.dev(s.codes, nb * (size_t)c.max_sub * kCodeWords * 4));
    GZPX_TRY(a.dev(s.hdr, nb * (size_t)c.max_sub * kHdrWords * 4));
    GZPX_TRY(a.dev(s.out_off, (nb + 1) * sizeof(uint64_t)));
    GZPX_TRY(a.dev(s.sizes, nb * sizeof(uint32_t)));
    GZPX_TRY(a.pinned(ctx->h_sub, (size_t)c.max_sub * sizeof(SubMeta)));
    return GZPX_OK;
}

// Everything a context holds for its whole life: streams, events, the scratch of one batch.  A failure leaves what
// exists by then to gzpx_ctx_destroy.
int ctx_acquire(gzpx_ctx *ctx) {
    GZPX_TRY(ctx->stream.create());
    GZPX_TRY(ctx->s_h2d.create());
    GZPX_TRY(ctx->s_d2h.create());
    GZPX_TRY(ctx->s_side.create(true));
    GZPX_TRY(ctx->ev_meta.create());
    GZPX_TRY(ctx->ev_crc.create());
    GZPX_TRY(ctx->ev_crc_t0.create(true));
    GZPX_TRY(ctx->ev_crc_t1.create(true));
    GZPX_TRY(ctx->ev_dep.create());
    GZPX_TRY(alloc_scratch(ctx));
    for (Event &e : ctx->prof.ev) GZPX_TRY(e.create(true));
    return GZPX_OK;
}

// HIP-event pairs around groups of launches (measurement mode only): a stage may consist of several
// launches on several streams, its time is the sum of its pairs.
// (A group that begins where the previous group of the same stream ended shares that event: every
// event record is a marker the stream has to process, and twenty of them cost the 3.7 ms step of the
// bench slab 0.08 ms.)
struct ProfPairs {
    gzpx_ctx *ctx;
    ProfLog &log;
    bool on;
    hipEvent_t dom_b = nullptr, dom_e = nullptr;  // mode 2, asynchronous: the job's own pair, read when it is waited for
    int used = 0;              // events handed out
    int last_ev = -1;          // the event recorded last ...
    hipStream_t last_st = nullptr;  // ... on this stream, with nothing enqueued behind it yet
    // a batch of the job in slot `sl` (which says whether the job carries the pair around its dominant stage)
    ProfPairs(gzpx_ctx *c, const Slot &sl) : ctx(c), log(c->prof), on(c->profiling != 0) {
        if (sl.dom_timed) {
            dom_b = sl.ev_dom_b;
            dom_e = sl.ev_dom_e;
        }
        log.n = 0;
    }
    int begin(Stage stage, hipStream_t st) {
        if (!on || log.n >= kProfPairs || used + 2 > 2 * kProfPairs) return -1;
        if (ctx->profiling == 2 && stage != kStMatch) return -1;
        if (dom_b) {
            (void)hipEventRecord(dom_b, st);
            return -2;
        }
        const int i = log.n++;
        log.stage[i] = stage;
        if (last_ev >= 0 && last_st == st) {
            log.b[i] = last_ev;
        } else {
            log.b[i] = used++;
            (void)hipEventRecord(log.ev[log.b[i]], st);
        }
        last_ev = -1;
        return i;
    }
    void end(int i, hipStream_t st) {
        if (i == -2) (void)hipEventRecord(dom_e, st);
        if (i < 0) return;
        log.e[i] = used++;
        (void)hipEventRecord(log.ev[log.e[i]], st);
        last_ev = log.e[i];
        last_st = st;
    }
    // something that is not part of a measured group went onto `st`: the next group records its own begin
    void touch(hipStream_t st) {
        if (last_st == st) last_ev = -1;
    }
    // the batch is enqueued.  Measurement mode, unless the job carries its own pair: one host wait per batch
    int finish(hipStream_t stream) {
        if (!on || dom_b) return GZPX_OK;
        HIP_TRY(hipStreamSynchronize(stream));
        for (int i = 0; i < log.n; i++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, log.ev[log.b[i]], log.ev[log.e[i]]));
            ctx->stage_ms[log.stage[i]] += ms;
        }
        return GZPX_OK;
    }
};

// Where the CRC of every block forks onto the low-priority side stream (it needs only the input; k_emit joins it).
// It is a question of whom it takes issue slots from (per 550 MiB step, round 3): beside k_mparse that kernel goes
// from 2.01 to 2.07 ms and k_hist + k_huffman, alone now, from 0.41 to 0.33 -- 3.50 against 3.53 ms; forked behind
// k_mparse (in front of the dense pair) 3.56.  (Round 2, beside the one-workgroup-per-block k_candidates: that kernel
// slowed down by the CRC's time.)  Levels 2-12 fork BEHIND their match / parse kernels, beside k_hist / k_huffman
// (round 6, tools/gpu_r6_fork_ab.sh: the one-workgroup-per-CU matchers lose more to the CRC's waves than the small
// kernels do -- configs[2] 61.2-62.0 -> 60.7 ms, text at levels 2-9 0.04 ms each).
enum CrcFork {
    kForkBesideMatch,   // behind k_candidates
    kForkBehindMparse,  // level 1: behind k_mparse / k_match, in front of k_parse
    kForkBehindMatch,   // behind every match / parse kernel
};
// (Config.debug bits 8-9, experiments: 1 = behind all match / parse kernels, 2 = behind the first of them, which
// levels 2-12 have only one group of, 3 = beside them whatever the level)
CrcFork crc_fork_of(const Config &c) {
    switch ((c.debug >> 8) & 3u) {
    case 1: return kForkBehindMatch;
    case 2: return c.level <= 1 ? kForkBehindMparse : kForkBehindMatch;
    case 3: return kForkBesideMatch;
    default: return c.level <= 1 ? kForkBesideMatch : kForkBehindMatch;
    }
}

// One batch of blocks through the pipeline, enqueued on `stream`.  Nothing here waits for the device.
// `sl`: the slot of the batch's job.  `prev` / `result`: the batch before this one of the same slab (device, may
// be null) and this batch's own record; output offsets continue from prev->total.
int enqueue_batch(gzpx_ctx *ctx, const Slot &sl, const uint8_t *d_in, size_t in_len, uint32_t nb, int is_last,
                  uint8_t *d_out, size_t out_cap, hipStream_t stream, const SlabResult *prev, SlabResult *result) {
    const Config &c = ctx->dcfg;
    const Scratch &s = ctx->scratch;
    ProfPairs pp(ctx, sl);
    auto fork_crc = [&]() -> int {
        HIP_TRY(hipEventRecord(ctx->ev_meta, stream));
        HIP_TRY(hipStreamWaitEvent(ctx->s_side, ctx->ev_meta, 0));
        pp.touch(stream);
        const int tc = pp.begin(kStCrc32, ctx->s_side);
        launch_crc32(c, d_in, in_len, nb, s, ctx->crc_consts, ctx->s_side);
        pp.end(tc, ctx->s_side);
        HIP_TRY(hipEventRecord(ctx->ev_crc, ctx->s_side));
        return GZPX_OK;
    };
    const CrcFork fork = crc_fork_of(c);
    // (the slab is cut into blocks -- BlockMeta -- by the first k_candidates launch; level 0: k_init_meta)
    int t = pp.begin(c.level == 0 ? kStInitMeta : kStCandidates, stream);
    launch_candidates(c, d_in, in_len, nb, is_last, s, stream);
    pp.end(t, stream);
    if (fork == kForkBesideMatch) GZPX_TRY(fork_crc());
    if (c.level <= 1) {  // (at level 0 every block is a passthrough block: the kernels return at once)
        // (Tried in round 3: the batch cut into 2..8 block ranges, k_hist / k_huffman of range k on a
        // side stream beside the matching of range k + 1.  4.27 -> 4.83 / 5.90 / 7.44 ms per step: the
        // 24 six-KiB workgroups k_huffman puts on a CU take the LDS that k_candidates / k_mparse need
        // whole, so the big kernels lose CUs to the small one instead of sharing them.)
        t = pp.begin(kStMatch, stream);
        launch_match(c, d_in, in_len, nb, s, stream);  // k_mparse, and k_match over the blocks it handed back
        pp.end(t, stream);
        if (fork == kForkBehindMparse) GZPX_TRY(fork_crc());
        t = pp.begin(kStParse, stream);
        launch_parse(c, d_in, in_len, nb, s, stream);
        pp.end(t, stream);
    } else {
        t = pp.begin(kStMatch, stream);
        if (c.level >= 10) {  // levels 10-12: the near-optimal parser, one lane per block (gzpx_nearopt.hip)
            launch_near_optimal(c, d_in, nb, s, stream);
        } else if (c.lazy) {  // levels 5-9: every match variant once, then the serial-per-block lazy parse
            launch_lazy(c, d_in, nb, s, stream);
        } else {
            // levels 2-4: every match once, then the greedy parse; a block whose new sub-block needs
            // another min_len parses on inside k_parse_hc, so nothing is read back and submit returns
            // without waiting for the device (round 2 ran these rounds from the host, a word per round)
            launch_hc(c, d_in, nb, s, stream);
        }
        pp.end(t, stream);
    }
    if (fork == kForkBehindMatch) GZPX_TRY(fork_crc());
    t = pp.begin(kStHist, stream);
    launch_hist(c, nb, s, stream);
    pp.end(t, stream);
    t = pp.begin(kStHuffman, stream);
    launch_huffman(c, nb, s, stream);
    pp.end(t, stream);
    t = pp.begin(kStScan, stream);
    launch_scan(nb, s, prev, result, stream);
    pp.end(t, stream);
    // join behind k_scan (which does not read the CRCs): k_emit writes them into the footers
    HIP_TRY(hipStreamWaitEvent(stream, ctx->ev_crc, 0));
    pp.touch(stream);  // (the wait for the side stream is nobody's stage time)
    t = pp.begin(kStEmit, stream);
    launch_emit(c, d_in, in_len, nb, s, d_out, out_cap, stream);
    pp.end(t, stream);
    HIP_TRY(hipGetLastError());
    GZPX_TRY(pp.finish(stream));
    ctx->last_nb = nb;
    return GZPX_OK;
}

// Snap's batch (src/snap.rs:61-74, FrameEncoder over every buffer): k_snap_chunk (raw Snappy + CRC-32C of every
// 64 KiB chunk), k_snap_frame + k_scan (framed sizes, offsets), k_snap_emit; the other stages stay 0.  Snap has no
// end-of-stream marker: is_last has no effect.
int enqueue_snap_batch(gzpx_ctx *ctx, const Slot &sl, const uint8_t *d_in, size_t in_len, uint32_t nb, uint8_t *d_out,
                       size_t out_cap, hipStream_t stream, const SlabResult *prev, SlabResult *result) {
    const Scratch &s = ctx->scratch;
    const uint32_t bs = (uint32_t)ctx->cfg.buffer_size;
    ProfPairs pp(ctx, sl);
    if (ctx->snap.dbg)
        HIP_TRY(hipMemsetAsync(ctx->snap.dbg, 0,
                               (size_t)nb * snap_chunks_per_buffer(bs) * 8 * sizeof(uint64_t), stream));
    int t = pp.begin(kStMatch, stream);
    launch_snap_chunk(d_in, in_len, bs, nb, ctx->snap, stream);
    pp.end(t, stream);
    t = pp.begin(kStScan, stream);
    launch_snap_frame(in_len, bs, nb, s, ctx->snap, stream);
    launch_scan(nb, s, prev, result, stream);
    pp.end(t, stream);
    t = pp.begin(kStEmit, stream);
    launch_snap_emit(d_in, in_len, bs, nb, s, ctx->snap, d_out, out_cap, stream);
    pp.end(t, stream);
    HIP_TRY(hipGetLastError());
    GZPX_TRY(pp.finish(stream));
    ctx->last_nb = nb;
    return GZPX_OK;
}

int slot_reserve(Slot &sl, size_t n_batches, size_t n_blocks) {
    GZPX_TRY(grow(sl.results_mem, sl.results_cap, n_batches, n_batches + 8, [&](size_t cap) -> int {
        GZPX_TRY(sl.results_mem.dev(sl.d_results, cap * sizeof(SlabResult)));
        return sl.results_mem.pinned(sl.h_results, cap * sizeof(SlabResult));
    }));
    return grow(sl.sizes_mem, sl.sizes_cap, n_blocks, n_blocks + n_blocks / 4 + 64,
                [&](size_t cap) { return sl.sizes_mem.pinned(sl.h_sizes, cap * sizeof(uint32_t)); });
}

int slot_staging(Slot &sl, size_t in_len, size_t out_need) {
    GZPX_TRY(grow(sl.in_mem, sl.d_in_cap, in_len + 16, in_len + in_len / 8 + 4096,
                  [&](size_t cap) { return sl.in_mem.dev(sl.d_in, cap); }));
    return grow(sl.out_mem, sl.d_out_cap, out_need, out_need + out_need / 8 + 4096,
                [&](size_t cap) { return sl.out_mem.dev(sl.d_out, cap); });
}

// One slab to compress.  A host job goes through the slot's staging buffers and its stream is copied to `out` when
// the ticket is waited for (the multi-device call, which learns every shard's place only then, leaves `out` null
// and starts the copies itself); a device job works on the caller's buffers in HBM.
struct SlabJob {
    const uint8_t *in;
    size_t in_len;
    int mode;  // GZPX_SLAB_*
    uint8_t *out;
    size_t out_cap;
    bool device;                  // in / out are device memory
    hipStream_t after = nullptr;  // device jobs: the stream to order behind (order_behind)
    bool wait_for_slot = false;   // every slot in flight: wait for one, instead of GZPX_ERR_BUSY
};

int check_slab_args(const gzpx_ctx *ctx, const void *in, size_t in_len, int mode, const void *out) {
    const size_t bs = ctx->cfg.buffer_size;
    if (mode != GZPX_SLAB_FULL_BLOCKS && mode != GZPX_SLAB_LAST && mode != GZPX_SLAB_FLUSH)
        return GZPX_ERR_INVALID_ARG;
    if (mode == GZPX_SLAB_FULL_BLOCKS && (in_len == 0 || in_len % bs != 0)) return GZPX_ERR_INVALID_ARG;
    if ((in_len && !in) || !out) return GZPX_ERR_INVALID_ARG;
    return GZPX_OK;
}

// Enqueue one slab: lock, set device, take a slot, put the job's copies and kernels on the context's streams.
int submit_enqueue(gzpx_ctx *ctx, const SlabJob &job, uint64_t *ticket) {
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return GZPX_ERR_DEVICE;
    const int si = free_slot(ctx, lk, job.wait_for_slot);
    if (si < 0) return GZPX_ERR_BUSY;
    Drain drain{{ctx->s_h2d, ctx->stream, ctx->s_side}, 3};  // (a failure leaves the slot free)
    Slot &sl = ctx->slots[si];
    if (!sl.ev_kernels) {
        GZPX_TRY(sl.ev_h2d.create());
        GZPX_TRY(sl.ev_kernels.create());
        GZPX_TRY(sl.ev_d2h.create());
        GZPX_TRY(sl.ev_dom_b.create(true));
        GZPX_TRY(sl.ev_dom_e.create(true));
    }
    const size_t bs = ctx->cfg.buffer_size, in_len = job.in_len;
    const uint64_t total_nb = blocks_of(bs, in_len);
    const uint64_t n_batches = (total_nb + ctx->batch_blocks - 1) / ctx->batch_blocks;
    GZPX_TRY(slot_reserve(sl, (size_t)n_batches, (size_t)total_nb));
    hipStream_t stream = ctx->stream;
    const uint8_t *d_in = job.in;  // where the kernels read and write, and how much they may write
    uint8_t *d_out = job.out;
    size_t out_cap = job.out_cap;
    if (!job.device) {
        GZPX_TRY(slot_staging(sl, in_len, gzpx_slab_bound(ctx, in_len)));
        if (in_len) {
            HIP_TRY(hipMemcpyAsync(sl.d_in, job.in, in_len, hipMemcpyHostToDevice, ctx->s_h2d));
            HIP_TRY(hipEventRecord(sl.ev_h2d, ctx->s_h2d));
            HIP_TRY(hipStreamWaitEvent(stream, sl.ev_h2d, 0));
        }
        d_in = sl.d_in;
        d_out = sl.d_out;
        out_cap = sl.d_out_cap;
    } else {
        GZPX_TRY(order_behind(stream, job.after, ctx->ev_dep));
    }
    memset(ctx->stage_ms, 0, sizeof(ctx->stage_ms));
    // profiling mode 2 on a one-batch slab: the job carries its own pair of events around the dominant stage and
    // stays asynchronous (the pair is read when the ticket is waited for); every other measurement waits per batch
    sl.dom_timed = ctx->profiling == 2 && n_batches == 1;
    const int is_last = job.mode == GZPX_SLAB_LAST;
    for (uint64_t bi = 0; bi < n_batches; bi++) {
        const uint64_t b0 = bi * ctx->batch_blocks;
        const uint32_t nb = (uint32_t)((total_nb - b0 < ctx->batch_blocks) ? total_nb - b0 : ctx->batch_blocks);
        const size_t in_begin = (size_t)b0 * bs;
        size_t in_batch = in_len > in_begin ? in_len - in_begin : 0;
        if (in_batch > (size_t)nb * bs) in_batch = (size_t)nb * bs;
        const int last_batch = (b0 + nb == total_nb) ? is_last : 0;
        const SlabResult *prev = bi ? sl.d_results + (bi - 1) : nullptr;
        if (ctx->cfg.format == GZPX_FORMAT_SNAP)
            GZPX_TRY(enqueue_snap_batch(ctx, sl, d_in + in_begin, in_batch, nb, d_out, out_cap, stream, prev, sl.d_results + bi));
        else
            GZPX_TRY(enqueue_batch(ctx, sl, d_in + in_begin, in_batch, nb, last_batch, d_out, out_cap, stream, prev,
                                   sl.d_results + bi));
        // the per-block sizes of this batch, before the next batch reuses the scratch
        HIP_TRY(hipMemcpyAsync(sl.h_sizes + b0, ctx->scratch.sizes, nb * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               stream));
    }
    HIP_TRY(hipMemcpyAsync(sl.h_results, sl.d_results, (size_t)n_batches * sizeof(SlabResult),
                           hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(sl.ev_kernels, stream));
    sl.job_d_out = d_out;
    sl.job_out_cap = out_cap;
    sl.host_out = job.device ? nullptr : job.out;
    sl.host_out_cap = job.device ? 0 : job.out_cap;
    sl.total_nb = total_nb;
    sl.n_batches = (uint32_t)n_batches;
    *ticket = issue_ticket(ctx, si);
    drain.armed = false;
    return GZPX_OK;
}

// Completing a ticket, in three phases (the multi-device entry runs them device by device so that the
// shards' copies overlap): wait for the kernels and read the result record; start the copy-out of a
// host job; wait for it and free the slot.
struct Completion {
    int rc = GZPX_OK;
    size_t produced = 0, blocks_done = 0;
};

Completion kernels_done(gzpx_ctx *ctx, Slot &sl) {
    Completion c;
    c.blocks_done = (size_t)sl.total_nb;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess || hipEventSynchronize(sl.ev_kernels) != hipSuccess) {
        c.rc = GZPX_ERR_DEVICE;
        return c;
    }
    if (sl.dom_timed) {  // the stage times of the job that has just been waited for
        float ms = 0;
        std::lock_guard<std::mutex> lk(ctx->mu);  // (a submit on another thread clears stage_ms under this lock)
        memset(ctx->stage_ms, 0, sizeof(ctx->stage_ms));
        if (hipEventElapsedTime(&ms, sl.ev_dom_b, sl.ev_dom_e) == hipSuccess) ctx->stage_ms[kStMatch] = ms;
        sl.dom_timed = false;
    }
    for (uint32_t bi = 0; bi < sl.n_batches && c.rc == GZPX_OK; bi++) {
        const SlabResult &r = sl.h_results[bi];
        if (r.fail_block != 0xFFFFFFFFu) {
            c.blocks_done = (size_t)bi * ctx->batch_blocks + r.fail_block;
            c.rc = r.fail_status == kStatusBlockSizeExceeded ? GZPX_ERR_BLOCK_SIZE_EXCEEDED : GZPX_ERR_DEVICE;
        }
    }
    if (c.rc == GZPX_OK) {
        c.produced = (size_t)sl.h_results[sl.n_batches - 1].total;
        if (c.produced > sl.job_out_cap) c.rc = GZPX_ERR_INSUFFICIENT_SPACE;
    }
    return c;
}

// the kernels are done (the host has seen their event): the copy needs no stream dependency
int start_copy_out(gzpx_ctx *ctx, Slot &sl, uint8_t *host_out, size_t produced) {
    if (!produced) return GZPX_OK;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess ||
        hipMemcpyAsync(host_out, sl.job_d_out, produced, hipMemcpyDeviceToHost, ctx->s_d2h) != hipSuccess ||
        hipEventRecord(sl.ev_d2h, ctx->s_d2h) != hipSuccess)
        return GZPX_ERR_DEVICE;
    return GZPX_OK;
}

int finish_copy_out(gzpx_ctx *ctx, Slot &sl, size_t produced) {
    if (!produced) return GZPX_OK;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess || hipEventSynchronize(sl.ev_d2h) != hipSuccess) return GZPX_ERR_DEVICE;
    return GZPX_OK;
}

void release_slot(gzpx_ctx *ctx, Slot &sl) {
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        sl.state = 0;
    }
    ctx->cv_slot.notify_all();
}

// Complete a ticket: wait for its kernels, copy the stream out (host jobs), report.
int wait_ticket(gzpx_ctx *ctx, uint64_t ticket, size_t *out_len, uint32_t *block_sizes, size_t max_blocks,
                size_t *n_blocks) {
    const int si = claim_ticket(ctx, ticket);
    if (si < 0) return GZPX_ERR_INVALID_ARG;
    Slot &sl = ctx->slots[si];
    const size_t host_out_cap = sl.host_out_cap;  // (the slot is ours from the claim on: no other thread writes it)
    Completion c = kernels_done(ctx, sl);
    int rc = c.rc;
    if (rc == GZPX_OK && sl.host_out && c.produced > host_out_cap) rc = GZPX_ERR_INSUFFICIENT_SPACE;
    if (rc == GZPX_OK && block_sizes) {
        if (max_blocks < sl.total_nb) rc = GZPX_ERR_INVALID_ARG;
        else memcpy(block_sizes, sl.h_sizes, (size_t)sl.total_nb * sizeof(uint32_t));
    }
    if (rc == GZPX_OK && sl.host_out) {
        rc = start_copy_out(ctx, sl, sl.host_out, c.produced);
        if (rc == GZPX_OK) rc = finish_copy_out(ctx, sl, c.produced);
    }
    if (out_len) *out_len = rc == GZPX_OK ? c.produced : 0;
    if (n_blocks) *n_blocks = c.blocks_done;
    release_slot(ctx, sl);
    return rc;
}

// the four single-context entry points: check, submit
int submit_checked(gzpx_ctx *ctx, const SlabJob &job, uint64_t *ticket) {
    if (!ctx || !ticket) return GZPX_ERR_INVALID_ARG;
    GZPX_TRY(check_slab_args(ctx, job.in, job.in_len, job.mode, job.out));
    return submit_enqueue(ctx, job, ticket);
}

// ... of which the two run forms wait for a slot, and then for the job
int run_checked(gzpx_ctx *ctx, SlabJob job, size_t *out_len, uint32_t *block_sizes, size_t max_blocks, size_t *n_blocks) {
    if (!ctx || !out_len) return GZPX_ERR_INVALID_ARG;
    if (block_sizes && max_blocks < blocks_of(ctx->cfg.buffer_size, job.in_len)) return GZPX_ERR_INVALID_ARG;
    uint64_t ticket = 0;
    job.wait_for_slot = true;
    GZPX_TRY(submit_checked(ctx, job, &ticket));
    return wait_ticket(ctx, ticket, out_len, block_sizes, max_blocks, n_blocks);
}

}  // namespace

// ---------------------------------------------------------------- multi-device slab call
// SURVEY 8(b) "multi-device variant", 8(e): blocks share no state, so a slab shards into contiguous
// block ranges, one per device, balanced to one block; only the range that holds the slab's end is
// cut with the caller's mode (short final piece / EOF marker).  Every device runs the single-device
// pipeline on its range -- no data-path exchange between them -- and the in-order write-out is done
// on the host side of the boundary: once the shard sizes are known (16 bytes per device), every
// device copies its shard straight to its offset in `out`, all copies in flight together, each
// over its own PCIe link.  (The one-process-per-GPU form of the same split, with the shards
// gathered over RCCL, is gzp_amd/shard.py + bench.py --gpus N.)
struct gzpx_multi {
    std::vector<gzpx_ctx *> ctxs;
    size_t buffer_size = 0;
    std::mutex mu;
    // device-resident form: every device's own output staging (its shard before the gather)
    struct Stage {
        uint8_t *d = nullptr;
        size_t cap = 0;
        Allocs mem;
    };
    std::unique_ptr<Stage[]> stage;  // one per device
};

namespace {

// the block range of device g of G when a slab of in_len bytes is cut (contiguous, balanced to one block)
struct MultiPart {
    uint64_t first = 0, nb = 0;
    size_t lo = 0, n = 0;
};
void multi_part_of(size_t in_len, size_t bs, size_t G, size_t g, MultiPart &p) {
    const uint64_t total_nb = blocks_of(bs, in_len);
    p = MultiPart();
    for (size_t k = 0; k <= g; k++) {
        p.first += p.nb;
        p.nb = total_nb / G + (k < total_nb % G ? 1 : 0);
    }
    p.lo = (size_t)(p.first * bs < in_len ? p.first * bs : in_len);
    const size_t hi = (size_t)((p.first + p.nb) * bs < in_len ? (p.first + p.nb) * bs : in_len);
    p.n = hi - p.lo;
}

// One slab over the devices of `m`, the sequence both forms of the call share.  They differ in what a device submits
// -- `job_of(g, range, job)` fills in device g's job, with nothing of that device's enqueued yet -- and in how a
// shard travels to its place once the sizes are known: `start_copy(g, slot, offset, produced)`.
template <class JobOf, class StartCopy>
int multi_compress(gzpx_multi *m, size_t in_len, int mode, size_t out_cap, size_t *out_len, uint32_t *block_sizes,
                   size_t max_blocks, size_t *n_blocks, JobOf &&job_of, StartCopy &&start_copy) {
    std::lock_guard<std::mutex> guard(m->mu);
    const size_t bs = m->buffer_size, G = m->ctxs.size();
    const uint64_t total_nb = blocks_of(bs, in_len);
    if (block_sizes && max_blocks < total_nb) return GZPX_ERR_INVALID_ARG;
    struct Part {
        MultiPart r;
        uint64_t ticket = 0;
        Slot *slot = nullptr;
        Completion c;
        bool submitted = false;
    };
    std::vector<Part> parts(G);
    int rc = GZPX_OK;
    // 1. every device: copy-in (host form) + kernels of its range; the devices work concurrently.  Only the range
    // that holds the slab's end is cut with the caller's mode.
    for (size_t g = 0; g < G && rc == GZPX_OK; g++) {
        Part &p = parts[g];
        multi_part_of(in_len, bs, G, g, p.r);
        if (p.r.nb == 0) continue;
        SlabJob job{nullptr, p.r.n, p.r.first + p.r.nb == total_nb ? mode : GZPX_SLAB_FULL_BLOCKS, nullptr, 0, false};
        job.wait_for_slot = true;
        rc = job_of(g, p.r, job);
        if (rc == GZPX_OK) rc = submit_enqueue(m->ctxs[g], job, &p.ticket);
        p.submitted = rc == GZPX_OK;
    }
    // 2. shard sizes (a 16-byte record per device) -> stream offsets
    size_t fail_block = (size_t)total_nb;
    for (size_t g = 0; g < G; g++) {
        Part &p = parts[g];
        if (!p.submitted) continue;
        const int si = claim_ticket(m->ctxs[g], p.ticket);
        if (si < 0) {
            if (rc == GZPX_OK) rc = GZPX_ERR_DEVICE;
            p.submitted = false;
            continue;
        }
        p.slot = &m->ctxs[g]->slots[si];
        p.c = kernels_done(m->ctxs[g], *p.slot);
        if (p.c.rc != GZPX_OK && rc == GZPX_OK) {  // the first failing block in stream order
            rc = p.c.rc;
            fail_block = (size_t)p.r.first + p.c.blocks_done;
        }
    }
    size_t total = 0;
    std::vector<size_t> offs(G, 0);
    for (size_t g = 0; g < G; g++) {
        offs[g] = total;
        if (parts[g].submitted) total += parts[g].c.produced;
    }
    if (rc == GZPX_OK && total > out_cap) rc = GZPX_ERR_INSUFFICIENT_SPACE;
    // 3. the ordered gather: every shard straight into its place, all copies started; 4. all copies finished
    for (size_t g = 0; g < G && rc == GZPX_OK; g++)
        if (parts[g].submitted && parts[g].c.produced) rc = start_copy(g, *parts[g].slot, offs[g], parts[g].c.produced);
    for (size_t g = 0; g < G; g++) {
        Part &p = parts[g];
        if (!p.submitted) continue;
        const int r2 = finish_copy_out(m->ctxs[g], *p.slot, p.c.produced);
        if (rc == GZPX_OK) rc = r2;
        if (rc == GZPX_OK && block_sizes)
            memcpy(block_sizes + p.r.first, p.slot->h_sizes, (size_t)p.r.nb * sizeof(uint32_t));
        release_slot(m->ctxs[g], *p.slot);
    }
    *out_len = rc == GZPX_OK ? total : 0;
    if (n_blocks) *n_blocks = rc == GZPX_OK ? (size_t)total_nb : fail_block;
    return rc;
}

constexpr size_t kCheckChunk = (size_t)64 << 20, kCheckTiles = kCheckChunk / kTile;  // a checksum call's unit of work

// The process-lifetime state behind gzpx_crc32 / gzpx_adler32 (device 0; the caller holds the state's mutex): the
// stream and the buffers of every call, made by the first one, whole or not at all -- a call that fails to make them
// leaves nothing behind and the next one tries again -- and never deleted: no HIP call at process exit.
template <class State>
int checksum_state(State *&state) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GZPX_ERR_NO_DEVICE;
    if (hipSetDevice(0) != hipSuccess) return GZPX_ERR_DEVICE;
    if (state) return GZPX_OK;
    std::unique_ptr<State> fresh(new (std::nothrow) State());
    if (!fresh) return GZPX_ERR_DEVICE;
    GZPX_TRY(fresh->init());
    state = fresh.release();
    return GZPX_OK;
}

// gzpx_crc32: k_init_meta cuts a chunk into 64 KiB tiles, k_crc32 takes one tile per workgroup
struct CrcState {
    Stream stream;
    Config cfg = {};       // (the two kernels read block_size alone)
    Scratch scratch = {};  // ... and meta: the tiles' BlockMeta
    CrcConsts cc;
    BlockMeta *h_meta = nullptr;  // pinned mirror
    Allocs mem;
    uint8_t *d_in = nullptr;  // staging, grown on demand
    size_t d_in_cap = 0;
    Allocs in_mem;
    int init() {
        cfg.block_size = kTile;
        cc = crc_consts();
        GZPX_TRY(stream.create());
        GZPX_TRY(mem.dev(scratch.meta, kCheckTiles * sizeof(BlockMeta)));
        return mem.pinned(h_meta, kCheckTiles * sizeof(BlockMeta));
    }
};

struct AdlerState {
    Stream stream;
    uint8_t *d_in = nullptr;
    uint32_t *d_out3 = nullptr, *h_out3 = nullptr;
    Allocs mem;
    int init() {
        GZPX_TRY(stream.create());
        GZPX_TRY(mem.dev(d_in, kCheckChunk));
        GZPX_TRY(mem.dev(d_out3, kCheckTiles * 12));
        return mem.pinned(h_out3, kCheckTiles * 12);
    }
};

}  // namespace

extern "C" {

void gzpx_config_default(gzpx_config *cfg, int format) {
    if (!cfg) return;
    cfg->device = 0;
    cfg->format = format;
    cfg->level = 3;  // ParCompressBuilder::new: Compression::new(3), src/par/compress.rs:54-62
    cfg->compat = GZPX_COMPAT_LIBDEFLATE_1_24;
    // Bgzf::DEFAULT_BUFSIZE = 65280 (src/deflate.rs:583); Mgzip and Snap keep the trait default
    // DEFAULT_BUFSIZE = BUFSIZE = 128 KiB (src/lib.rs:330, :105)
    cfg->buffer_size = format == GZPX_FORMAT_BGZF ? 65280 : 131072;
    cfg->max_slab_bytes = (size_t)1 << 30;
}

int gzpx_ctx_create(const gzpx_config *cfg, gzpx_ctx **out) {
    if (!cfg || !out) return GZPX_ERR_INVALID_ARG;
    *out = nullptr;
    const bool snap = cfg->format == GZPX_FORMAT_SNAP;
    if (cfg->format != GZPX_FORMAT_BGZF && cfg->format != GZPX_FORMAT_MGZIP && !snap) return GZPX_ERR_INVALID_ARG;
    if (cfg->buffer_size < kDictSize) return GZPX_ERR_BUFFER_SIZE;  // src/par/compress.rs:68-74
    // (Snap ignores the level and has no libdeflate rules, src/snap.rs:53-59, 91)
    if (!snap && (cfg->level < 0 || cfg->level > 12)) return GZPX_ERR_COMPRESSION_LEVEL;
    if (!snap && cfg->compat != GZPX_COMPAT_LIBDEFLATE_1_24 && cfg->compat != GZPX_COMPAT_LIBDEFLATE_1_10)
        return GZPX_ERR_INVALID_ARG;
    if (cfg->buffer_size > kMaxBlockSize) return GZPX_ERR_UNSUPPORTED;  // > 16 MiB blocks: not built
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GZPX_ERR_NO_DEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return GZPX_ERR_INVALID_ARG;
    if (hipSetDevice(cfg->device) != hipSuccess) return GZPX_ERR_DEVICE;

    gzpx_ctx *ctx = new (std::nothrow) gzpx_ctx();
    if (!ctx) return GZPX_ERR_DEVICE;
    ctx->cfg = *cfg;
    ctx->dcfg.format = (uint32_t)cfg->format;
    // (a Snap context runs none of the deflate kernels: its level and compat are kept as given and ignored)
    const int lvl = snap ? 0 : cfg->level, cmp = snap ? GZPX_COMPAT_LIBDEFLATE_1_24 : cfg->compat;
    ctx->dcfg.level = (uint32_t)lvl;
    // Levels 10-12 are libdeflate 1.10's near-optimal parser (1.24 changed it; there is nothing here to pin a port of
    // the later parser on): the 1.10 rules go with it WHATEVER the caller asked for, so the stream is exactly the
    // 1.10 binary's and never a hybrid of two versions.  gzpx_ctx_active_compat() tells which rules a context runs.
    ctx->dcfg.compat = (uint32_t)(lvl >= 10 ? GZPX_COMPAT_LIBDEFLATE_1_10 : cmp);
    if (lvl >= 10 && cmp != GZPX_COMPAT_LIBDEFLATE_1_10 && getenv("GZPX_TRACE")) {
        static std::atomic<bool> told{false};  // (once per process; ADVICE round 4: the override used to be silent)
        if (!told.exchange(true))
            fprintf(stderr, "gzpx: level %d runs libdeflate 1.10's near-optimal parser; compat %d was asked for, the 1.10 "
                            "rules are in force (gzpx_ctx_active_compat)\n", lvl, cmp);
    }
    ctx->dcfg.block_size = (uint32_t)cfg->buffer_size;
    ctx->dcfg.xfl = lvl >= 9 ? 2u : lvl <= 1 ? 4u : 0u;  // src/bgzf.rs:278-284
    ctx->dcfg.debug = 0;
    // per-block strides: padding for k_candidates' last iteration / dword-wide tile loads
    ctx->dcfg.stride = (uint32_t)((cfg->buffer_size + 2047) / 2048 * 2048 + 2048);
    // level 1 sub-blocks hold FAST_SEQ_STORE_LENGTH matches of at least four bytes; the block splitter of levels
    // 2-12 may cut every MIN_BLOCK_LENGTH bytes
    ctx->dcfg.max_sub = (uint32_t)(cfg->buffer_size / (lvl == 1 ? 4 * kFastSeqStoreLen : kMinBlockLen) + 2);
    // deflate_compress: inputs up to 55 - 4*level bytes -- and everything at level 0 -- take
    // deflate_compress_none
    ctx->dcfg.passthrough = lvl == 0 ? 0xFFFFFFFFu : (uint32_t)(55 - 4 * lvl);
    const LevelParams lp = level_params((uint32_t)lvl);  // libdeflate_alloc_compressor
    ctx->dcfg.hc_depth = lp.depth;
    ctx->dcfg.hc_nice = lp.nice;
    ctx->dcfg.lazy = lp.lazy;
    ctx->dcfg.no_passes = lp.passes;
    ctx->crc_consts = crc_consts();
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) {
        snprintf(ctx->devname, sizeof(ctx->devname), "%.150s (%.60s, %d CUs)", prop.name, prop.gcnArchName,
                 prop.multiProcessorCount);
        ctx->dcfg.n_cu = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 0u;
    }
    const uint64_t want = blocks_of(cfg->buffer_size, cfg->max_slab_bytes ? cfg->max_slab_bytes : 1);
    ctx->batch_blocks = (uint32_t)(want < kMaxBatchBlocks ? want : kMaxBatchBlocks);
    const size_t fit = kMaxScratchBytes / (snap ? snap_scratch_bytes_per_block(cfg->buffer_size) : scratch_bytes_per_block(ctx->dcfg));
    if (ctx->batch_blocks > fit) ctx->batch_blocks = (uint32_t)fit;
    if (ctx->batch_blocks == 0) ctx->batch_blocks = 1;
    const int rc = ctx_acquire(ctx);
    if (rc != GZPX_OK) {
        gzpx_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return GZPX_OK;
}

void gzpx_ctx_destroy(gzpx_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->cfg.device);
    for (const Stream *st : {&ctx->stream, &ctx->s_h2d, &ctx->s_d2h, &ctx->s_side}) st->sync();
    delete ctx;
}

int gzpx_ctx_active_compat(const gzpx_ctx *ctx) {
    if (!ctx) return GZPX_ERR_INVALID_ARG;
    return ctx->cfg.format == GZPX_FORMAT_SNAP ? ctx->cfg.compat : (int)ctx->dcfg.compat;
}

size_t gzpx_slab_bound(const gzpx_ctx *ctx, size_t in_len) {
    if (!ctx) return 0;
    const size_t blocks = (size_t)blocks_of(ctx->cfg.buffer_size, in_len) * framed_bound_per_block(ctx);
    return ctx->cfg.format == GZPX_FORMAT_SNAP ? blocks : blocks + kEofMarkerBytes + 64;
}

int gzpx_compress_slab_submit(gzpx_ctx *ctx, const uint8_t *in, size_t in_len, int mode, uint8_t *out,
                              size_t out_cap, uint64_t *ticket) {
    return submit_checked(ctx, {in, in_len, mode, out, out_cap, false}, ticket);
}

int gzpx_compress_slab_submit_device(gzpx_ctx *ctx, const void *d_in, size_t in_len, int mode, void *d_out,
                                     size_t out_cap, void *after_stream, uint64_t *ticket) {
    return submit_checked(ctx, {(const uint8_t *)d_in, in_len, mode, (uint8_t *)d_out, out_cap, true, (hipStream_t)after_stream},
                          ticket);
}

int gzpx_compress_slab_wait(gzpx_ctx *ctx, uint64_t ticket, size_t *out_len, uint32_t *block_sizes,
                            size_t max_blocks, size_t *n_blocks) {
    if (!ctx) return GZPX_ERR_INVALID_ARG;
    return wait_ticket(ctx, ticket, out_len, block_sizes, max_blocks, n_blocks);
}

int gzpx_compress_slab_event(gzpx_ctx *ctx, uint64_t ticket, void **hip_event) {
    if (!ctx || !hip_event) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int si = ticket_slot(ctx, ticket);
    if (si < 0) return GZPX_ERR_INVALID_ARG;
    *hip_event = (void *)ctx->slots[si].ev_kernels;
    return GZPX_OK;
}

int gzpx_compress_slab_device(gzpx_ctx *ctx, const void *d_in, size_t in_len, int mode,
                              void *d_out, size_t out_cap, size_t *out_len, uint32_t *block_sizes,
                              size_t max_blocks, size_t *n_blocks, void *hip_stream) {
    return run_checked(ctx, {(const uint8_t *)d_in, in_len, mode, (uint8_t *)d_out, out_cap, true, (hipStream_t)hip_stream},
                       out_len, block_sizes, max_blocks, n_blocks);
}

int gzpx_compress_slab(gzpx_ctx *ctx, const uint8_t *in, size_t in_len, int mode, uint8_t *out,
                       size_t out_cap, size_t *out_len, uint32_t *block_sizes, size_t max_blocks,
                       size_t *n_blocks) {
    return run_checked(ctx, {in, in_len, mode, out, out_cap, false}, out_len, block_sizes, max_blocks, n_blocks);
}

int gzpx_encode_block(gzpx_ctx *ctx, const uint8_t *in, size_t n, int is_last, uint8_t *out,
                      size_t out_cap, size_t *out_len) {
    if (!ctx) return GZPX_ERR_INVALID_ARG;
    if (n > ctx->cfg.buffer_size) return GZPX_ERR_INVALID_ARG;
    // Bgzf::encode runs on one block; the EOF marker is the only is_last effect
    // (src/deflate.rs:613-626).  A non-last block may be short (flush()).
    std::vector<uint8_t> tmp(gzpx_slab_bound(ctx, n));
    size_t got = 0, nb = 0;
    int rc = gzpx_compress_slab(ctx, in, n, is_last ? GZPX_SLAB_LAST : GZPX_SLAB_FLUSH, tmp.data(),
                                tmp.size(), &got, nullptr, 0, &nb);
    if (rc != GZPX_OK) return rc;
    if (got > out_cap) return GZPX_ERR_INSUFFICIENT_SPACE;
    memcpy(out, tmp.data(), got);
    *out_len = got;
    return GZPX_OK;
}

int gzpx_multi_create(const gzpx_config *cfg, const int *devices, size_t n_devices, gzpx_multi **out) {
    if (!cfg || !devices || !n_devices || !out) return GZPX_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->format == GZPX_FORMAT_SNAP) return GZPX_ERR_UNSUPPORTED;  // (multi-device Snap: not built)
    gzpx_multi *m = new (std::nothrow) gzpx_multi();
    if (!m) return GZPX_ERR_DEVICE;
    m->buffer_size = cfg->buffer_size;
    m->stage.reset(new (std::nothrow) gzpx_multi::Stage[n_devices]);
    if (!m->stage) {
        delete m;
        return GZPX_ERR_DEVICE;
    }
    for (size_t g = 0; g < n_devices; g++) {
        gzpx_config c = *cfg;
        c.device = devices[g];
        // each device sees 1/n of the largest slab (+ one block of imbalance)
        if (c.max_slab_bytes) c.max_slab_bytes = c.max_slab_bytes / n_devices + 2 * c.buffer_size;
        gzpx_ctx *ctx = nullptr;
        const int rc = gzpx_ctx_create(&c, &ctx);
        if (rc != GZPX_OK) {
            gzpx_multi_destroy(m);
            return rc;
        }
        m->ctxs.push_back(ctx);
    }
    // device-to-device copies of the gather: direct over xGMI where the devices can reach each other
    for (size_t a = 0; a < n_devices; a++)
        for (size_t b = 0; b < n_devices; b++) {
            int can = 0;
            if (devices[a] != devices[b] && hipDeviceCanAccessPeer(&can, devices[a], devices[b]) == hipSuccess && can &&
                hipSetDevice(devices[a]) == hipSuccess)
                (void)hipDeviceEnablePeerAccess(devices[b], 0);  // (already enabled: an error we ignore)
        }
    (void)hipGetLastError();
    *out = m;
    return GZPX_OK;
}

void gzpx_multi_destroy(gzpx_multi *m) {
    if (!m) return;
    for (size_t g = 0; g < m->ctxs.size(); g++)
        if (hipSetDevice(m->ctxs[g]->cfg.device) == hipSuccess) m->stage[g].mem.release();
    for (gzpx_ctx *c : m->ctxs) gzpx_ctx_destroy(c);
    delete m;
}

int gzpx_multi_shard(const gzpx_multi *m, size_t in_len, size_t g, size_t *offset, size_t *len) {
    if (!m || g >= m->ctxs.size() || !offset || !len) return GZPX_ERR_INVALID_ARG;
    MultiPart p;
    multi_part_of(in_len, m->buffer_size, m->ctxs.size(), g, p);
    *offset = p.lo;
    *len = p.n;
    return GZPX_OK;
}

// The device-resident form: north_star's write-out.  Range g of the slab already lives on device g
// (d_in[g]); every device compresses its range into its own staging buffer, the host learns the shard
// sizes and each shard then travels ONCE, device to device, into its stream offset of `d_out` on
// devices[root] -- hipMemcpyPeerAsync on the owning device's copy stream, all peers at once (every peer
// has its own xGMI link to the root); the root's own shard is a local copy.  No payload byte touches
// host memory.  In-order property: src/par/compress.rs:305-310.
int gzpx_multi_compress_slab_device(gzpx_multi *m, const void *const *d_in, size_t in_len, int mode, size_t root,
                                    void *d_out, size_t out_cap, size_t *out_len, uint32_t *block_sizes,
                                    size_t max_blocks, size_t *n_blocks) {
    if (!m || !out_len || m->ctxs.empty() || !d_in || !d_out || root >= m->ctxs.size()) return GZPX_ERR_INVALID_ARG;
    GZPX_TRY(check_slab_args(m->ctxs[0], d_in, in_len, mode, d_out));
    const int root_dev = m->ctxs[root]->cfg.device;
    return multi_compress(
        m, in_len, mode, out_cap, out_len, block_sizes, max_blocks, n_blocks,
        [&](size_t g, const MultiPart &r, SlabJob &job) -> int {
            if (r.n && !d_in[g]) return GZPX_ERR_INVALID_ARG;
            if (hipSetDevice(m->ctxs[g]->cfg.device) != hipSuccess) return GZPX_ERR_DEVICE;
            const size_t need = gzpx_slab_bound(m->ctxs[g], r.n);
            gzpx_multi::Stage &st = m->stage[g];
            GZPX_TRY(grow(st.mem, st.cap, need, need + need / 8 + 4096, [&](size_t cap) { return st.mem.dev(st.d, cap); }));
            job.in = (const uint8_t *)d_in[g];
            job.out = st.d;
            job.out_cap = st.cap;
            job.device = true;
            job.after = (hipStream_t)GZPX_STREAM_NONE;  // (the caller's contract: the ranges are ready)
            return GZPX_OK;
        },
        [&](size_t g, Slot &sl, size_t off, size_t produced) -> int {
            gzpx_ctx *ctx = m->ctxs[g];
            if (hipSetDevice(ctx->cfg.device) != hipSuccess ||
                hipMemcpyPeerAsync((uint8_t *)d_out + off, root_dev, m->stage[g].d, ctx->cfg.device, produced, ctx->s_d2h) !=
                    hipSuccess ||
                hipEventRecord(sl.ev_d2h, ctx->s_d2h) != hipSuccess)
                return GZPX_ERR_DEVICE;
            return GZPX_OK;
        });
}

size_t gzpx_multi_devices(const gzpx_multi *m) { return m ? m->ctxs.size() : 0; }

// The host form: every device copies its shard straight to its offset in `out`, each over its own PCIe link.
int gzpx_multi_compress_slab(gzpx_multi *m, const uint8_t *in, size_t in_len, int mode, uint8_t *out,
                             size_t out_cap, size_t *out_len, uint32_t *block_sizes, size_t max_blocks,
                             size_t *n_blocks) {
    if (!m || !out_len || m->ctxs.empty()) return GZPX_ERR_INVALID_ARG;
    GZPX_TRY(check_slab_args(m->ctxs[0], in, in_len, mode, out));
    return multi_compress(
        m, in_len, mode, out_cap, out_len, block_sizes, max_blocks, n_blocks,
        [&](size_t, const MultiPart &r, SlabJob &job) -> int {
            job.in = in + r.lo;  // (the stream stays in the slot's staging: its place in `out` is known after the sizes are)
            return GZPX_OK;
        },
        [&](size_t g, Slot &sl, size_t off, size_t produced) { return start_copy_out(m->ctxs[g], sl, out + off, produced); });
}

// ---------------------------------------------------------------- libdeflate-shaped ABI
struct gzpx_compressor {
    int level;
    int compat;
    gzpx_ctx *ctx;
    std::vector<uint8_t> tmp;
};

gzpx_compressor *gzpx_alloc_compressor(int level) {
    if (level < 0 || level > 12) return nullptr;
    gzpx_compressor *c = new (std::nothrow) gzpx_compressor();
    if (!c) return nullptr;
    c->level = level;
    c->compat = GZPX_COMPAT_LIBDEFLATE_1_24;
    c->ctx = nullptr;
    return c;
}

int gzpx_compressor_set_compat(gzpx_compressor *c, int compat) {
    if (!c || c->ctx) return GZPX_ERR_INVALID_ARG;
    c->compat = compat;
    return GZPX_OK;
}

static int compressor_ctx(gzpx_compressor *c, size_t n) {
    if (c->ctx && n <= c->ctx->cfg.buffer_size) return GZPX_OK;
    if (c->ctx) gzpx_ctx_destroy(c->ctx);
    c->ctx = nullptr;
    gzpx_config cfg;
    gzpx_config_default(&cfg, GZPX_FORMAT_MGZIP);  // Mgzip framing has no payload size limit
    cfg.level = c->level;
    cfg.compat = c->compat;
    size_t bs = 65536;  // one whole-buffer DEFLATE call = one "block" of that size
    while (bs < n) bs *= 2;
    cfg.buffer_size = bs;
    cfg.max_slab_bytes = bs;
    return gzpx_ctx_create(&cfg, &c->ctx);
}

size_t gzpx_deflate_compress(gzpx_compressor *c, const void *in, size_t n, void *out, size_t cap) {
    if (!c || (!in && n) || !out) return 0;
    if (n > kMaxBlockSize) return 0;  // whole-buffer inputs above 16 MiB: not built
    if (compressor_ctx(c, n) != GZPX_OK) return 0;
    c->tmp.resize(gzpx_slab_bound(c->ctx, n));
    size_t got = 0, nb = 0;
    if (gzpx_compress_slab(c->ctx, (const uint8_t *)in, n, GZPX_SLAB_LAST, c->tmp.data(), c->tmp.size(),
                           &got, nullptr, 0, &nb) != GZPX_OK)
        return 0;
    const size_t hdr = header_bytes(c->ctx->dcfg.format), payload = got - hdr - kTrailerBytes;
    if (payload > cap) return 0;  // libdeflate: 0 when the output does not fit
    memcpy(out, c->tmp.data() + hdr, payload);
    return payload;
}

size_t gzpx_deflate_compress_bound(gzpx_compressor *c, size_t n) {
    // libdeflate_deflate_compress_bound: worst case = stored blocks of MIN_BLOCK_LENGTH
    // bytes, 5 bytes of header each.  v1.10 (probed on the image's binary) adds 1 + 8 bytes of
    // slack (OUTPUT_END_PADDING); the pinned v1.24 does not.
    size_t max_blocks = (n + kMinBlockLen - 1) / kMinBlockLen;
    if (max_blocks < 1) max_blocks = 1;
    const size_t slack = (c && c->compat == GZPX_COMPAT_LIBDEFLATE_1_10) ? 9 : 0;
    return 5 * max_blocks + n + slack;
}

void gzpx_free_compressor(gzpx_compressor *c) {
    if (!c) return;
    if (c->ctx) gzpx_ctx_destroy(c->ctx);
    delete c;
}

int gzpx_crc32_checked(uint32_t crc, const void *buf, size_t n, uint32_t *out) {
    // libdeflate_crc32 semantics: crc32(crc, buf) = combine(crc, crc32(0, buf), n)
    static std::mutex mu;
    static CrcState *state = nullptr;
    if (!out || (!buf && n)) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(mu);
    GZPX_TRY(checksum_state(state));
    *out = crc;
    CrcState &st = *state;
    const uint8_t *p = (const uint8_t *)buf;
    while (n) {
        const size_t take = n < kCheckChunk ? n : kCheckChunk;
        GZPX_TRY(grow(st.in_mem, st.d_in_cap, take + 16, take + take / 8 + 4096,
                      [&](size_t cap) { return st.in_mem.dev(st.d_in, cap); }));
        const uint32_t nb = (uint32_t)((take + kTile - 1) / kTile);
        HIP_TRY(hipMemcpyAsync(st.d_in, p, take, hipMemcpyHostToDevice, st.stream));
        launch_init_meta(st.cfg, take, nb, 0, st.scratch, st.stream);
        launch_crc32(st.cfg, st.d_in, take, nb, st.scratch, st.cc, st.stream);
        HIP_TRY(hipMemcpyAsync(st.h_meta, st.scratch.meta, nb * sizeof(BlockMeta), hipMemcpyDeviceToHost, st.stream));
        HIP_TRY(hipStreamSynchronize(st.stream));
        for (uint32_t b = 0; b < nb; b++) crc = crc32_combine(crc, st.h_meta[b].crc, st.h_meta[b].n);
        p += take;
        n -= take;
    }
    *out = crc;
    return GZPX_OK;
}

uint32_t gzpx_crc32(uint32_t crc, const void *buf, size_t n) {
    // libdeflate_crc32's signature has no error channel: a device failure leaves `crc` unchanged
    // and is reported through gzpx_last_status() (thread-local); gzpx_crc32_checked returns it.
    uint32_t out = crc;
    t_last_status = gzpx_crc32_checked(crc, buf, n, &out);
    return t_last_status == GZPX_OK ? out : crc;
}

int gzpx_last_status(void) { return t_last_status; }

// ---- Crc32::combine, Adler32::update / combine (src/check.rs:85-164): the device side of Adler32::update is in gzpx_wrap.h
uint32_t gzpx_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) { return crc32_combine(crc1, crc2, len2); }

uint32_t gzpx_adler32_combine(uint32_t adler1, uint32_t adler2, uint64_t len2) {
    // zlib's adler32_combine (zlib 1.2.11 / zlib-ng 2.x: the same arithmetic), restated from its published algorithm
    const uint32_t base = 65521u;
    const uint32_t rem = (uint32_t)(len2 % base);
    uint32_t sum1 = adler1 & 0xFFFFu;
    uint32_t sum2 = (uint32_t)(((uint64_t)rem * sum1) % base);
    sum1 += (adler2 & 0xFFFFu) + base - 1;
    sum2 += ((adler1 >> 16) & 0xFFFFu) + ((adler2 >> 16) & 0xFFFFu) + base - rem;
    if (sum1 >= base) sum1 -= base;
    if (sum1 >= base) sum1 -= base;
    if (sum2 >= (base << 1)) sum2 -= (base << 1);
    if (sum2 >= base) sum2 -= base;
    return sum1 | (sum2 << 16);
}

int gzpx_adler32_checked(uint32_t adler, const void *buf, size_t n, uint32_t *out) {
    static std::mutex mu;
    static AdlerState *state = nullptr;
    if (!out || (!buf && n)) return GZPX_ERR_INVALID_ARG;
    *out = adler;
    if (n == 0) return GZPX_OK;
    std::lock_guard<std::mutex> lock(mu);
    GZPX_TRY(checksum_state(state));
    uint8_t *const d_in = state->d_in;
    uint32_t *const d_out3 = state->d_out3, *const h_out3 = state->h_out3;
    const hipStream_t stream = state->stream;
    const uint32_t base = 65521u;
    uint32_t a = adler & 0xFFFFu, b = (adler >> 16) & 0xFFFFu;
    const uint8_t *p = (const uint8_t *)buf;
    while (n) {
        const size_t take = n < kCheckChunk ? n : kCheckChunk;
        const size_t tiles = (take + 65535) / 65536;
        HIP_TRY(hipMemcpyAsync(d_in, p, take, hipMemcpyHostToDevice, stream));
        launch_adler32(d_in, take, d_out3, stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_out3, d_out3, tiles * 12, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        for (size_t t = 0; t < tiles; t++) {  // a' = a + s1, b' = b + len a + s2
            const uint32_t s1 = h_out3[3 * t], s2 = h_out3[3 * t + 1], len = h_out3[3 * t + 2];
            b = (uint32_t)((b + (uint64_t)(len % base) * a + s2) % base);
            a = (a + s1) % base;
        }
        p += take;
        n -= take;
    }
    *out = a | (b << 16);
    return GZPX_OK;
}

uint32_t gzpx_adler32(uint32_t adler, const void *buf, size_t n) {
    // zlib's adler32 signature has no error channel: a device failure leaves `adler` unchanged and is reported through
    // gzpx_last_status() (thread-local), as with gzpx_crc32
    uint32_t out = adler;
    t_last_status = gzpx_adler32_checked(adler, buf, n, &out);
    return t_last_status == GZPX_OK ? out : adler;
}

}  // extern "C"

// ---------------------------------------------------------------- ParDecompress side
namespace {

// One slab of blocks being inflated.  Everything a slab needs lives in its slot (block tables,
// staging), so up to kSlots slabs are in flight: copy-in of one, kernels of another, copy-out of
// a third, each on its own stream.
struct DSlot : NoCopy {
    int state = 0;  // 0 free, 1 submitted, 2 a thread is inside wait()
    uint64_t gen = 0;
    Event ev_h2d, ev_kernels, ev_done;  // (all seven: created with the slot's first use)
    Event ev_t0, ev_t1;  // around the inflate kernels (timing enabled)
    Event ev_tm;         // behind k_inflate_seg (the decode / copy route)
    Event ev_tc;         // behind the check kernel of gzpx_inflate_batch_device
    bool have_check = false;  // ev_t1 .. ev_tc hold the slot's last launch
    InflateScratch sc;  // match records / tile table of k_inflate_seg + k_lzcopy; sc.redo lives with the block tables
    uint64_t *h_total = nullptr;    // pinned
    uint32_t *h_summary = nullptr;  // pinned: the host's words of the launch record (kDs*, kWrRec*)
    Allocs once;  // h_total, h_summary, sc.summary: 64 bytes each, made with the events
    size_t cap_blocks = 0;
    uint64_t *d_offsets = nullptr, *d_out_off = nullptr;
    uint32_t *d_sizes = nullptr, *d_crc = nullptr;
    DBlockHost *d_blk = nullptr;
    DBlockHost *h_blk = nullptr;  // pinned
    uint32_t *h_crc = nullptr;    // pinned
    uint64_t *h_offsets = nullptr;  // pinned copies of the caller's arrays (the caller's may be pageable
    uint32_t *h_sizes = nullptr;    //  and must not be referenced after submit returns)
    Allocs tables;  // the ten arrays of cap_blocks members, sc.redo among them
    bool have_blk = false;          // h_blk holds this launch's records (debug launches only)
    uint8_t *d_in = nullptr, *d_out = nullptr;
    size_t d_in_cap = 0, d_out_cap = 0;
    Allocs in_mem, out_mem;
    size_t mlist_cap = 0, tfirst_cap = 0;
    Allocs mlist_mem, tfirst_mem;  // sc.mlist, sc.tfirst
    size_t nb = 0;
    int route = kInflateRouteSeg;  // the route of the slot's last launch (the context's may have changed since)
    int debug = 0;                 // ... and what gzpx_debug_inflate had selected for it
};

int dslot_reserve(DSlot &c, size_t nb) {
    if (!c.ev_kernels) {
        GZPX_TRY(c.ev_h2d.create());
        GZPX_TRY(c.ev_kernels.create());
        GZPX_TRY(c.ev_done.create());
        for (Event *e : {&c.ev_t0, &c.ev_t1, &c.ev_tm, &c.ev_tc}) GZPX_TRY(e->create(true));
        GZPX_TRY(c.once.pinned(c.h_total, 64));
        GZPX_TRY(c.once.pinned(c.h_summary, kDsWords * 4));
        GZPX_TRY(c.once.dev(c.sc.summary, kDsWords * 4));
        HIP_TRY(hipMemset(c.sc.summary, 0, kDsWords * 4));  // (kDsSegHint is kept from launch to launch)
    }
    Allocs &t = c.tables;
    return grow(t, c.cap_blocks, nb, nb + nb / 4 + 64, [&](size_t cap) -> int {
        GZPX_TRY(t.dev(c.d_offsets, cap * 8));
        GZPX_TRY(t.dev(c.d_out_off, (cap + 1) * 8));
        GZPX_TRY(t.dev(c.d_sizes, cap * 4));
        GZPX_TRY(t.dev(c.d_crc, cap * 4));
        GZPX_TRY(t.dev(c.d_blk, cap * sizeof(DBlockHost)));
        GZPX_TRY(t.dev(c.sc.redo, (2 * cap + 2) * 4));  // (list, ticket counter, and a debug launch's reasons)
        GZPX_TRY(t.pinned(c.h_blk, cap * sizeof(DBlockHost)));
        GZPX_TRY(t.pinned(c.h_crc, cap * 4));
        GZPX_TRY(t.pinned(c.h_offsets, cap * 8));
        return t.pinned(c.h_sizes, cap * 4);
    });
}

// What each kind of call keeps in its context: scratch, pinned mirrors, capacities, events and what the getters may
// read of them, used by one call at a time under the context's mutex.  (Destroyed last to first: memory, then events.)

// member discovery (gzpx_*_device calls that take no member table)
struct ScanState : NoCopy {
    Event ev0, ev1;  // around the scan kernels
    bool have = false;
    MemberScanScratch ms;
    uint32_t *h_rec = nullptr;  // pinned: the scan record
    Allocs once;                // ms.rec, h_rec
    size_t seg_cap = 0;
    Allocs seg;   // ms.seg_count, ms.seg_off
    Allocs cand;  // the six candidate arrays of ms.cap entries
    uint64_t *d_tab_off = nullptr;  // the walk's table for gzpx_scan_blocks_device
    uint32_t *d_tab_size = nullptr;
    size_t tab_cap = 0;
    Allocs tab_mem;
    int reserve(size_t n_seg, size_t cap) {
        if (!ms.rec) {
            GZPX_TRY(once.dev(ms.rec, 64));
            GZPX_TRY(once.pinned(h_rec, 64));
            GZPX_TRY(ev0.create(true));
            GZPX_TRY(ev1.create(true));
        }
        GZPX_TRY(grow(seg, seg_cap, n_seg, n_seg, [&](size_t n) -> int {
            GZPX_TRY(seg.dev(ms.seg_count, n * 4));
            return seg.dev(ms.seg_off, n * 4);
        }));
        return grow(cand, ms.cap, cap, cap, [&](size_t n) -> int {
            GZPX_TRY(cand.dev(ms.pos, n * 8));
            GZPX_TRY(cand.dev(ms.size, n * 4));
            GZPX_TRY(cand.dev(ms.succ, n * 4));
            GZPX_TRY(cand.dev(ms.jump[0], n * 4));
            GZPX_TRY(cand.dev(ms.jump[1], n * 4));
            return cand.dev(ms.idx, n * 4);
        });
    }
};

// reads by range (gzpx_read_ranges_device); the line searches select their members with it too
struct RangesState : NoCopy {
    Event ev[5];        // select [0..1], inflate [2..3], gather [3..4]
    bool have = false;  // ev[0..1] hold the last call's select; stages: [2..4] its inflate and gather
    bool stages = false;
    size_t last_members = 0;
    RangeScratch rr;
    uint32_t *h_rec = nullptr;  // pinned: the record of locate + select
    Allocs once;                // rr.rec, h_rec
    size_t range_cap = 0, host_cap = 0, member_cap = 0;
    uint64_t *h_ranges = nullptr;   // pinned: the caller's ranges on their way in
    uint64_t *h_out_off = nullptr;  // pinned: out_offsets on their way out
    Allocs ranges;   // rr.ranges, first, len, src, out_off
    Allocs host;     // the two pinned arrays above: a call whose tables lie in device memory needs none
    Allocs members;  // rr.diff, map, soff
    int reserve(size_t n_ranges, size_t n_members, bool host_tables = true) {
        if (!rr.rec) {
            GZPX_TRY(once.dev(rr.rec, 64));
            GZPX_TRY(once.pinned(h_rec, 64));
            for (Event &e : ev) GZPX_TRY(e.create(true));
        }
        GZPX_TRY(grow(ranges, range_cap, n_ranges, n_ranges + n_ranges / 4 + 64, [&](size_t cap) -> int {
            GZPX_TRY(ranges.dev(rr.ranges, cap * 16));
            GZPX_TRY(ranges.dev(rr.first, cap * 4));
            GZPX_TRY(ranges.dev(rr.len, cap * 8));
            GZPX_TRY(ranges.dev(rr.src, cap * 8));
            return ranges.dev(rr.out_off, (cap + 1) * 8);
        }));
        GZPX_TRY(grow(host, host_cap, host_tables ? n_ranges : 0, n_ranges + n_ranges / 4 + 64, [&](size_t cap) -> int {
            GZPX_TRY(host.pinned(h_ranges, cap * 16));
            return host.pinned(h_out_off, (cap + 1) * 8);
        }));
        return grow(members, member_cap, n_members + 1, n_members + n_members / 4 + 64, [&](size_t cap) -> int {
            GZPX_TRY(members.dev(rr.diff, cap * 4));
            GZPX_TRY(members.dev(rr.map, cap * 4));
            return members.dev(rr.soff, cap * 8);
        });
    }
};

// members inflated back to back for a read by range, a line call or a search: room for `bytes` and 64 more
struct Staging : NoCopy {
    uint8_t *d = nullptr;
    size_t cap = 0;
    Allocs mem;
    int reserve(uint64_t bytes) {
        return grow(mem, cap, (size_t)(bytes + 64), (size_t)(bytes + bytes / 8 + 4096), [&](size_t n) { return mem.dev(d, n); });
    }
};

// checksums of a table (gzpx_checksum_batch_device); the record and the events are a slot's
struct CksumState : NoCopy {
    CksumScratch ck;
    size_t entry_cap = 0, wg_cap = 0;
    Allocs entries;      // ck.prefix, ck.part
    Allocs wgs;          // ck.carry
    uint32_t width = 0;  // gzpx_dctx_set_checksum_width
    int reserve(size_t n, uint32_t workgroups) {
        GZPX_TRY(grow(entries, entry_cap, n, n + n / 4 + 64, [&](size_t cap) -> int {
            GZPX_TRY(entries.dev(ck.prefix, (cap + 1) * 8));
            return entries.dev(ck.part, cap * 4);
        }));
        return grow(wgs, wg_cap, workgroups, workgroups, [&](size_t cap) { return wgs.dev(ck.carry, cap * 8); });
    }
};

static_assert(kLnTile == GZPX_LINES_TILE, "the public constant states the kernels' tile");
constexpr size_t kLinesBatchDefault = (size_t)256 << 20;

// reads by line (gzpx_dlines_build_device and the two searches); the searches also use the ranges' state, the staging
// buffer and one slot, as a read by byte range does
struct LinesState : NoCopy {
    size_t batch = 0;  // gzpx_dctx_set_lines_batch (0: kLinesBatchDefault); the search's batches too
    Event ev[7];       // tiles + select [0..1], inflate [2..3], search [3..4], gather [5..6]; a build: [0..1..2] per batch
    int stages = 0;    // how many of the four stages of the last search ev holds
    size_t last_members = 0;
    float build_ms[2] = {0.0f, 0.0f};  // the last build's inflate and count kernels, summed over its batches
    LinesScratch ln;
    uint32_t *h_rec = nullptr;  // pinned: the search record
    Allocs once;                // ln.rec, h_rec
    size_t cap = 0, host_cap = 0;  // boundaries
    uint64_t *h_bpos = nullptr;    // pinned: the byte positions on their way out
    Allocs bounds;                 // ln.bounds, btile, bpos
    Allocs host;                   // h_bpos: a call whose tables lie in device memory needs none
    int reserve(size_t n_bounds, bool host_tables = true) {
        if (!ln.rec) {
            GZPX_TRY(once.dev(ln.rec, 64));
            GZPX_TRY(once.pinned(h_rec, 64));
            for (Event &e : ev) GZPX_TRY(e.create(true));
        }
        GZPX_TRY(grow(bounds, cap, n_bounds, n_bounds + n_bounds / 4 + 64, [&](size_t n) -> int {
            GZPX_TRY(bounds.dev(ln.bounds, n * 8));
            GZPX_TRY(bounds.dev(ln.btile, n * 4));
            return bounds.dev(ln.bpos, n * 8);
        }));
        return grow(host, host_cap, host_tables ? n_bounds : 0, n_bounds + n_bounds / 4 + 64,
                    [&](size_t n) { return host.pinned(h_bpos, n * 8); });
    }
};

// search (gzpx_find_device; the scratch and the events for a set's too): the batches, the staging buffer and one slot as a
// line-table build uses them
struct FindState : NoCopy {
    Event ev[4];                       // per batch: inflate [0..1], count + scan [1..2], write + carry [2..3]
    float ms[3] = {0.0f, 0.0f, 0.0f};  // the last gzpx_find_device's, summed over its batches
    FindScratch fd;
    uint32_t *h_pat = nullptr;  // pinned: the pattern on its way in
    uint64_t *h_rec = nullptr;  // pinned: the record on its way out
    Allocs once;                // fd.pat, fd.rec and the two pinned arrays above
    size_t piece_cap = 0;
    Allocs pieces;  // fd.cnt, fd.bases
    int reserve(size_t n_pieces) {
        if (!fd.rec) {
            GZPX_TRY(once.dev(fd.pat, kFdMaxPattern));
            GZPX_TRY(once.dev(fd.rec, kFdRecWords * 8));
            GZPX_TRY(once.pinned(h_pat, kFdMaxPattern));
            GZPX_TRY(once.pinned(h_rec, kFdRecWords * 8));
            for (Event &e : ev) GZPX_TRY(e.create(true));
        }
        return grow(pieces, piece_cap, n_pieces, n_pieces + n_pieces / 8 + 16, [&](size_t cap) -> int {
            GZPX_TRY(pieces.dev(fd.cnt, cap * 8));
            return pieces.dev(fd.bases, cap * 16);
        });
    }
};

// selection of lines by content (gzpx_select_lines_device): the search's state for the counting pass of every batch, and
// its own for the record bitmap and the runs
struct SelectState : NoCopy {
    Event ev[5];                       // per batch: inflate [0..1], count + scan + mark + carry [1..2]; the runs [3..4]
    float ms[3] = {0.0f, 0.0f, 0.0f};  // the last call's, the first two summed over its batches
    SelectScratch sl;
    uint64_t *h_rec = nullptr;  // pinned: the record on its way out
    uint64_t *h_run = nullptr;  // pinned: the one run of a call that inflates nothing, on its way in
    Allocs once;                // sl.rec and the two pinned arrays above
    size_t record_cap = 0;
    Allocs records;  // sl.bitmap, cnt, bases
    int reserve(uint64_t n_records) {
        if (!sl.rec) {
            GZPX_TRY(once.dev(sl.rec, kSlRecWords * 8));
            GZPX_TRY(once.pinned(h_rec, kSlRecWords * 8));
            GZPX_TRY(once.pinned(h_run, 16));
            for (Event &e : ev) GZPX_TRY(e.create(true));
        }
        return grow(records, record_cap, (size_t)n_records, (size_t)(n_records + n_records / 8 + 4096), [&](size_t cap) -> int {
            const size_t groups = (size_t)select_groups(cap);
            GZPX_TRY(records.dev(sl.bitmap, (cap + 31) / 32 * 4));
            GZPX_TRY(records.dev(sl.cnt, groups * 8));
            return records.dev(sl.bases, groups * 4);
        });
    }
};

// search for a set (gzpx_find_set_device, gzpx_select_lines_set_device): the compiled set and the counts per pattern.
// The pieces' counts and bases, the record and its pinned copy are the search's (c->find), as the selection uses them.
struct FindSetState : NoCopy {
    float ms[3] = {0.0f, 0.0f, 0.0f};  // the last gzpx_find_set_device's, summed over its batches (timed with c->find.ev)
    FsSet *d_set = nullptr;
    FsSet *h_set = nullptr;        // pinned: the compiled set on its way in
    uint64_t *d_counts = nullptr;  // [kFsMaxPatterns] the hits of every pattern
    Allocs once;                   // the three above
    bool ready = false;
    int reserve() {
        if (ready) return GZPX_OK;
        once.release();  // (an earlier attempt that failed half way)
        GZPX_TRY(once.dev(d_set, sizeof(FsSet)));
        GZPX_TRY(once.dev(d_counts, kFsMaxPatterns * 8));
        GZPX_TRY(once.pinned(h_set, sizeof(FsSet)));
        ready = true;
        return GZPX_OK;
    }
};

// fields of lines (gzpx_read_fields_device and its table form): the line search's state in front, then its own pieces
struct FieldsState : NoCopy {
    Event ev[4];        // carry + scan [0..1], count + scan [1..2], write [2..3]
    bool have = false;  // ev[0..2] hold the last call's two counting stages; wrote: ev[3] its writing pass
    bool wrote = false;
    FieldsScratch fl;
    FlSet *h_set = nullptr;     // pinned: the compiled field list on its way in
    uint64_t *h_rec = nullptr;  // pinned: the record on its way out
    Allocs once;                // fl.set, fl.rec and the two pinned arrays above
    size_t range_cap = 0, host_cap = 0, piece_cap = 0;
    uint64_t *h_out_off = nullptr;  // pinned: out_offsets on their way out
    Allocs ranges;  // fl.pfirst, fl.out_off
    Allocs host;    // h_out_off: a call whose tables lie in device memory needs none
    Allocs pieces;  // fl.carry, cin, cnt, obase
    int reserve(size_t n_ranges, size_t n_pieces, bool host_tables) {
        if (!fl.rec) {
            GZPX_TRY(once.dev(fl.set, sizeof(FlSet)));
            GZPX_TRY(once.dev(fl.rec, kFlRecWords * 8));
            GZPX_TRY(once.pinned(h_set, sizeof(FlSet)));
            GZPX_TRY(once.pinned(h_rec, kFlRecWords * 8));
            for (Event &e : ev) GZPX_TRY(e.create(true));
        }
        GZPX_TRY(grow(ranges, range_cap, n_ranges, n_ranges + n_ranges / 4 + 64, [&](size_t cap) -> int {
            GZPX_TRY(ranges.dev(fl.pfirst, (cap + 1) * 8));
            return ranges.dev(fl.out_off, (cap + 1) * 8);
        }));
        GZPX_TRY(grow(host, host_cap, host_tables ? n_ranges : 0, n_ranges + n_ranges / 4 + 64,
                      [&](size_t cap) { return host.pinned(h_out_off, (cap + 1) * 8); }));
        return grow(pieces, piece_cap, n_pieces + 1, n_pieces + n_pieces / 8 + 16, [&](size_t cap) -> int {
            GZPX_TRY(pieces.dev(fl.carry, cap * 4));
            GZPX_TRY(pieces.dev(fl.cin, cap * 8));
            GZPX_TRY(pieces.dev(fl.cnt, cap * 4));
            return pieces.dev(fl.obase, (cap + 1) * 8);
        });
    }
};

// numeric columns of lines (gzpx_read_columns_device and its table form): the line search's state in front, the pieces
// and carries of the fields' first pass in its own scratch, then the rows and the parse
struct ColumnsState : NoCopy {
    Event ev[3];        // carries + row scan [0..1], the parse [1..2]
    bool have = false;  // ev holds the last call's stages
    ColumnsScratch cl;
    ClCols *h_cols = nullptr;   // pinned: the column list on its way in
    uint64_t *h_rec = nullptr;  // pinned: the record on its way out
    Allocs once;                // cl.cols, cl.rec, cl.fl.rec and the two pinned arrays above
    size_t range_cap = 0, host_cap = 0, piece_cap = 0;
    uint64_t *h_row_off = nullptr;  // pinned: row_offsets on their way out
    Allocs ranges;  // cl.fl.pfirst, cl.row_off
    Allocs host;    // h_row_off: a call whose tables lie in device memory needs none
    Allocs pieces;  // cl.fl.carry, cl.fl.cin, cl.rcnt, cl.rin
    int reserve(size_t n_ranges, size_t n_pieces, bool host_tables) {
        if (!cl.rec) {
            once.release();  // (an earlier attempt that failed half way)
            GZPX_TRY(once.dev(cl.cols, sizeof(ClCols)));
            GZPX_TRY(once.dev(cl.fl.rec, kFlRecWords * 8));
            GZPX_TRY(once.pinned(h_cols, sizeof(ClCols)));
            GZPX_TRY(once.pinned(h_rec, kClRecWords * 8));
            for (Event &e : ev) GZPX_TRY(e.create(true));
            GZPX_TRY(once.dev(cl.rec, kClRecWords * 8));
        }
        GZPX_TRY(grow(ranges, range_cap, n_ranges, n_ranges + n_ranges / 4 + 64, [&](size_t cap) -> int {
            GZPX_TRY(ranges.dev(cl.fl.pfirst, (cap + 1) * 8));
            return ranges.dev(cl.row_off, (cap + 1) * 8);
        }));
        GZPX_TRY(grow(host, host_cap, host_tables ? n_ranges : 0, n_ranges + n_ranges / 4 + 64,
                      [&](size_t cap) { return host.pinned(h_row_off, (cap + 1) * 8); }));
        return grow(pieces, piece_cap, n_pieces + 1, n_pieces + n_pieces / 8 + 16, [&](size_t cap) -> int {
            GZPX_TRY(pieces.dev(cl.fl.carry, cap * 4));
            GZPX_TRY(pieces.dev(cl.fl.cin, cap * 8));
            GZPX_TRY(pieces.dev(cl.rcnt, cap * 4));
            return pieces.dev(cl.rin, cap * 8);
        });
    }
};

// selection of lines by their numbers (gzpx_where_lines_device and its table form): the line search's state in front,
// then the columns' stages in scratch of its own, the two bitmaps and the runs
struct WhereState : NoCopy {
    Event ev[4];        // carries + row scan [0..1], the parse with the predicate [1..2], the runs [2..3]
    bool have = false;  // ev holds the last call's stages
    WhereScratch wh;
    ClCols *h_cols = nullptr;     // pinned: the distinct fields on their way in
    WhTextTerms *h_terms = nullptr;  // pinned: the compiled terms on their way in
    uint64_t *h_rec = nullptr;    // pinned: the record on its way out
    Allocs once;                  // wh.cl.cols, wh.cl.rec, wh.cl.fl.rec, wh.terms, wh.rec and the three pinned arrays above
    size_t range_cap = 0, piece_cap = 0, bit_cap = 0;
    Allocs ranges;  // wh.cl.fl.pfirst, wh.cl.row_off
    Allocs pieces;  // wh.cl.fl.carry, wh.cl.fl.cin, wh.cl.rcnt, wh.cl.rin
    Allocs rows;    // wh.bitmap (wh.starts behind it), wh.cnt, wh.bases
    int reserve(size_t n_ranges, size_t n_pieces, uint64_t bits) {
        ColumnsScratch &cl = wh.cl;
        if (!wh.rec) {
            once.release();  // (an earlier attempt that failed half way)
            GZPX_TRY(once.dev(cl.cols, sizeof(ClCols)));
            GZPX_TRY(once.dev(cl.fl.rec, kFlRecWords * 8));
            GZPX_TRY(once.dev(cl.rec, kClRecWords * 8));
            GZPX_TRY(once.dev(wh.terms, sizeof(WhTextTerms)));
            GZPX_TRY(once.pinned(h_cols, sizeof(ClCols)));
            GZPX_TRY(once.pinned(h_terms, sizeof(WhTextTerms)));
            GZPX_TRY(once.pinned(h_rec, kWhRecWords * 8));
            for (Event &e : ev) GZPX_TRY(e.create(true));
            GZPX_TRY(once.dev(wh.rec, kWhRecWords * 8));
        }
        GZPX_TRY(grow(ranges, range_cap, n_ranges, n_ranges + n_ranges / 4 + 64, [&](size_t cap) -> int {
            GZPX_TRY(ranges.dev(cl.fl.pfirst, (cap + 1) * 8));
            return ranges.dev(cl.row_off, (cap + 1) * 8);
        }));
        GZPX_TRY(grow(pieces, piece_cap, n_pieces + 1, n_pieces + n_pieces / 8 + 16, [&](size_t cap) -> int {
            GZPX_TRY(pieces.dev(cl.fl.carry, cap * 4));
            GZPX_TRY(pieces.dev(cl.fl.cin, cap * 8));
            GZPX_TRY(pieces.dev(cl.rcnt, cap * 4));
            return pieces.dev(cl.rin, cap * 8);
        }));
        // (the call's bitmaps are where_bits() bits each, back to back: wh.starts is placed per call)
        return grow(rows, bit_cap, (size_t)bits, (size_t)where_bits(bits + bits / 8 + 4096), [&](size_t cap) -> int {
            const size_t groups = cap / kSlRunRecords;
            GZPX_TRY(rows.dev(wh.bitmap, cap / 8 * 2));
            GZPX_TRY(rows.dev(wh.cnt, groups * 8));
            return rows.dev(wh.bases, groups * 4);
        });
    }
};

}  // namespace

// (members are destroyed last to first: memory and events of the slots and of each kind of call, then the streams)
struct gzpx_dctx : NoCopy {
    int device = 0;
    int format = 0;
    CrcConsts cc;
    Stream stream, s_h2d, s_d2h;
    Event ev_dep;
    uint64_t next_gen = 1;
    int n_cu = 0;
    int debug = 0;  // 1: instrumented k_inflate_seg / k_inflate, 2: instrumented k_lzcopy
    int route = kInflateRouteSeg;  // GZPX_INFLATE_ROUTE=wave / gzpx_dctx_set_route: k_inflate for every member
    int last_slot = -1;  // the slot of the last completed launch (timing / debug counters)
    size_t last_nb = 0;
    ScanState scan;
    RangesState ranges;
    Staging stage;
    CksumState cksum;
    LinesState lines;
    FindState find;
    SelectState select;
    FindSetState find_set;
    FieldsState fields;
    ColumnsState columns;
    WhereState where;
    DSlot slots[kSlots];
    std::mutex mu;
    std::condition_variable cv_slot;
};

namespace {

// the 64-bit field of a record of 32-bit words that starts at `word`
uint64_t rec_u64(const uint32_t *rec, size_t word) { return (uint64_t)rec[word] | ((uint64_t)rec[word + 1] << 32); }

// what the device's walk found (dscan_run): the table itself stays in the context's scratch for launch_member_emit
struct ScanResult {
    size_t n_members = 0;  // whole members in front of the walk's end
    size_t consumed = 0;   // where it ended
    bool invalid = false;  // ... at a header that fails the checks (a cap below n_members stops the walk before it sees that)
    int slot = -1;         // the free slot dscan_run waited for in front of the walk, for the caller that goes on to use one
};

// k_inflate_seg + k_lzcopy's match records and tile table for nb members that inflate to at most out_cap bytes
int dslot_seg_scratch(DSlot &sl, size_t out_cap, size_t nb) {
    const size_t need_m = inflate_mlist_bytes(out_cap, nb), need_t = inflate_tfirst_bytes(out_cap, nb);
    GZPX_TRY(grow(sl.mlist_mem, sl.mlist_cap, need_m, need_m + need_m / 8,
                  [&](size_t cap) { return sl.mlist_mem.dev(sl.sc.mlist, cap); }));
    return grow(sl.tfirst_mem, sl.tfirst_cap, need_t, need_t + need_t / 8,
                [&](size_t cap) { return sl.tfirst_mem.dev(sl.sc.tfirst, cap); });
}

// A slot made ready for an inflate launch of nb members on `route`: what the launch reads from it, what the getters
// read after it, and on the decode / copy route that pair's scratch for `cap` bytes of output.  `in_bytes`: the
// compressed bytes that stand for the members' total (InflateScratch).  The slot then holds no member records and no
// check time: the caller that brings the records back, or runs a check kernel, says so itself.  `writes` false (the
// sizes call): nothing is inflated, so the pair's scratch is neither sized nor allocated.
int dslot_prepare(gzpx_dctx *c, DSlot &sl, size_t nb, int route, size_t cap, uint64_t in_bytes, bool writes = true) {
    sl.nb = nb;
    sl.route = route;
    sl.debug = c->debug;
    sl.have_blk = sl.have_check = false;
    sl.sc.n_cu = c->n_cu;
    sl.sc.in_bytes = in_bytes;
    return route == kInflateRouteSeg && writes ? dslot_seg_scratch(sl, cap, nb) : GZPX_OK;
}

// What an inflate launch takes from the context and from a slot that dslot_prepare has made ready (InflateLaunch): the
// caller adds where the compressed bytes lie and where the output goes (the sizes call: nowhere).
InflateLaunch inflate_launch_of(const gzpx_dctx *c, const DSlot &sl, const uint8_t *d_in, uint64_t *d_out_off, uint8_t *d_out,
                                size_t out_cap) {
    InflateLaunch l;
    l.d_in = d_in;
    l.nb = (uint32_t)sl.nb;
    l.d_blk = sl.d_blk;
    l.d_out_off = d_out_off;
    l.d_out = d_out;
    l.out_cap = out_cap;
    l.d_check = sl.d_crc;
    l.debug = sl.debug;
    l.route = sl.route;
    l.ev_begin = sl.ev_t0;
    l.ev_mid = sl.ev_tm;
    l.ev_end = sl.ev_t1;
    l.ev_check = sl.ev_tc;
    l.stream = c->stream;
    l.sc = &sl.sc;
    l.cc = &c->cc;
    return l;
}

// The framed inflate, enqueued on the context's stream: the slot made ready, nb members of d_in, listed by the device
// tables `offsets` / `sizes`, into dst[0..cap) back to back, and k_dsummary's words (what the host needs of the members'
// records: summary_verdict) on their way to sl.h_summary.  `ev_before`, if any, is recorded in front of the kernels.
int inflate_enqueue(gzpx_dctx *c, DSlot &sl, const uint8_t *d_in, const uint64_t *offsets, const uint32_t *sizes, size_t nb,
                    uint8_t *dst, size_t cap, uint64_t in_bytes, hipEvent_t ev_before = nullptr) {
    GZPX_TRY(dslot_prepare(c, sl, nb, c->route, cap, in_bytes));
    if (ev_before) HIP_TRY(hipEventRecord(ev_before, c->stream));
    launch_inflate(inflate_launch_of(c, sl, d_in, sl.d_out_off, dst, cap), header_bytes(c->format), offsets, sizes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sl.h_summary, sl.sc.summary, kDsHostWords * 4, hipMemcpyDeviceToHost, c->stream));
    return GZPX_OK;
}

// the members' records themselves, behind a launch: only for the debug counters, and only the calls that bring them back
int debug_records(gzpx_dctx *c, DSlot &sl, size_t nb) {
    if (!c->debug) return GZPX_OK;
    HIP_TRY(hipMemcpyAsync(sl.h_blk, sl.d_blk, nb * sizeof(DBlockHost), hipMemcpyDeviceToHost, c->stream));
    sl.have_blk = true;
    return GZPX_OK;
}

// Enqueue the inflate of one slab (c->mu held): copies in, kernels, copies out, as the compress side's submit_enqueue.
// `scan`: the members are the first nb of the walk dscan_run has just made over d_in, in the slot it waited for (the
// table is still in the context's scratch); what the loop below checks of a caller's table, the walk guarantees of
// its own.
int dsubmit_enqueue(gzpx_dctx *c, const uint8_t *host_in, const uint8_t *d_in, size_t in_len,
                    const uint64_t *offsets, const uint32_t *sizes, size_t nb, uint8_t *host_out, uint8_t *d_out,
                    size_t out_cap, hipStream_t after, bool block_for_slot, std::unique_lock<std::mutex> &lk,
                    uint64_t *ticket, const ScanResult *scan = nullptr) {
    if (nb && ((!scan && (!offsets || !sizes)) || (!host_in && !d_in) || (scan && !d_in))) return GZPX_ERR_INVALID_ARG;
    if (nb > 0xFFFFFFFFull) return GZPX_ERR_INVALID_ARG;
    const uint32_t hdr_len = header_bytes(c->format);
    for (size_t b = 0; b < nb && !scan; b++)
        if (sizes[b] < hdr_len + 8 || offsets[b] > in_len || sizes[b] > in_len - offsets[b]) return GZPX_ERR_INVALID_ARG;
    const int si = scan ? scan->slot : free_slot(c, lk, block_for_slot);
    if (si < 0) return GZPX_ERR_BUSY;
    // (the copy-in still reads the caller's `in`, the copy-out may still write the caller's `out`; the slot stays free)
    Drain drain{{c->s_h2d, c->stream, c->s_d2h}, 3};
    DSlot &sl = c->slots[si];
    GZPX_TRY(dslot_reserve(sl, nb ? nb : 1));
    sl.nb = nb;  // (no members: a ticket all the same, with nothing behind it)
    hipStream_t stream = c->stream;
    if (nb) {
        if (host_in) {  // staging
            GZPX_TRY(grow(sl.in_mem, sl.d_in_cap, in_len + 16, in_len + in_len / 8 + 4096,
                          [&](size_t cap) { return sl.in_mem.dev(sl.d_in, cap); }));
            GZPX_TRY(grow(sl.out_mem, sl.d_out_cap, out_cap + 16, out_cap + out_cap / 8 + 4096,
                          [&](size_t cap) { return sl.out_mem.dev(sl.d_out, cap); }));
            HIP_TRY(hipMemcpyAsync(sl.d_in, host_in, in_len, hipMemcpyHostToDevice, c->s_h2d));
            d_in = sl.d_in;
            d_out = sl.d_out;
        } else {
            GZPX_TRY(order_behind(stream, after, c->ev_dep));
        }
        uint64_t csum = 0;  // the members' compressed bytes
        if (scan) {  // the table goes from the scan's scratch to the slot's on the device
            launch_member_emit(c->scan.ms, (uint32_t)nb, sl.d_offsets, sl.d_sizes, stream);
            csum = scan->consumed;  // (the members of a walk lie back to back from offset 0)
        } else {
            memcpy(sl.h_offsets, offsets, nb * 8);
            memcpy(sl.h_sizes, sizes, nb * 4);
            HIP_TRY(hipMemcpyAsync(sl.d_offsets, sl.h_offsets, nb * 8, hipMemcpyHostToDevice, c->s_h2d));
            HIP_TRY(hipMemcpyAsync(sl.d_sizes, sl.h_sizes, nb * 4, hipMemcpyHostToDevice, c->s_h2d));
            HIP_TRY(hipEventRecord(sl.ev_h2d, c->s_h2d));
            HIP_TRY(hipStreamWaitEvent(stream, sl.ev_h2d, 0));
            for (size_t b = 0; b < nb; b++) csum += sizes[b];
        }
        // (the pair's scratch is sized by what the caller can take)
        GZPX_TRY(inflate_enqueue(c, sl, d_in, sl.d_offsets, sl.d_sizes, nb, d_out, out_cap, csum));
        GZPX_TRY(debug_records(c, sl, nb));
        HIP_TRY(hipMemcpyAsync(sl.h_total, sl.d_out_off + nb, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipEventRecord(sl.ev_kernels, stream));
        if (host_out) {
            // Blocks land back to back from offset 0 and their sizes are the footers' ISIZE fields,
            // so the bytes to bring back are known now: the copy-out is enqueued behind the kernels
            // and needs no host round trip.
            uint64_t total = 0;
            for (size_t b = 0; b < nb; b++) {
                const uint8_t *f = host_in + offsets[b] + sizes[b] - 4;
                total += (uint64_t)f[0] | ((uint64_t)f[1] << 8) | ((uint64_t)f[2] << 16) | ((uint64_t)f[3] << 24);
            }
            if (total > out_cap) total = out_cap;  // (the kernels flag the blocks that do not fit)
            HIP_TRY(hipStreamWaitEvent(c->s_d2h, sl.ev_kernels, 0));
            if (total) HIP_TRY(hipMemcpyAsync(host_out, sl.d_out, (size_t)total, hipMemcpyDeviceToHost, c->s_d2h));
            HIP_TRY(hipEventRecord(sl.ev_done, c->s_d2h));
        } else {
            HIP_TRY(hipEventRecord(sl.ev_done, stream));
        }
    }
    *ticket = issue_ticket(c, si);
    drain.armed = false;
    return GZPX_OK;
}

// The launch record of the framed paths (k_dsummary's, kDs*) as the call's return code; a failure names the first
// failing member of the launch, by its index in the launch, and the two checksums.  `lenient`: the libdeflate-shaped
// call's rule, under which fewer bytes than ISIZE are no failure.
int summary_verdict(const uint32_t *rec, bool lenient, gzpx_check_info *info) {
    const uint32_t *q = rec + (lenient ? kDsLenient : kDsStrict);
    if (q[kDsFirst] == 0xFFFFFFFFu) return GZPX_OK;
    if (info) {
        info->block = q[kDsFirst];
        info->found = q[kDsFound];
        info->expected = q[kDsExpected];
    }
    const uint32_t st = q[kDsStatus];
    return st == kInfBadData ? GZPX_ERR_BAD_DATA
           : st == kInfInsufficientSpace ? GZPX_ERR_INSUFFICIENT_SPACE
           : (st != kInfOk && !lenient) ? GZPX_ERR_BAD_DATA  // kInfShortOutput
                                        : GZPX_ERR_INVALID_CHECK;
}

// `short_ok`: the libdeflate-shaped call offers its capacity as ISIZE and accepts fewer bytes (libdeflate
// with actual_out_nbytes_ret); a framed member that inflates to fewer bytes than its footer says is
// BadData (libdeflate SHORT_OUTPUT through decode_block, src/par/decompress.rs:162-186).
int dwait_ticket(gzpx_dctx *c, uint64_t ticket, size_t *out_len, gzpx_check_info *info, bool short_ok = false) {
    const int si = claim_ticket(c, ticket);
    if (si < 0) return GZPX_ERR_INVALID_ARG;
    DSlot &sl = c->slots[si];
    int rc = GZPX_OK;
    size_t produced = 0;
    if (sl.nb) {
        if (hipSetDevice(c->device) != hipSuccess || hipEventSynchronize(sl.ev_done) != hipSuccess) {
            rc = GZPX_ERR_DEVICE;
        } else {
            // the first failing block in stream order (src/par/decompress.rs:162-186), found on the device
            rc = summary_verdict(sl.h_summary, short_ok, info);
            if (rc == GZPX_OK) produced = (size_t)*sl.h_total;
        }
    }
    if (out_len) *out_len = produced;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        sl.state = 0;
        c->last_slot = si;
        c->last_nb = sl.nb;
    }
    c->cv_slot.notify_all();
    return rc;
}

// gzpx_scan_blocks over d_in[0..in_len) on the device, without the cap: how many members the walk from offset 0
// records and where it stops.  Returns synchronised; the table stays in c->scan.ms (launch_member_emit) until the next
// scan of this context.  Called with c->mu held.  `slot_lk`: the caller goes on to use a slot and holds c->mu from
// the scan until it is done with the table: a free slot is waited for first (the wait lets go of the mutex), r->slot.
int dscan_run(gzpx_dctx *c, const uint8_t *d_in, size_t in_len, hipStream_t after, ScanResult *r,
              std::unique_lock<std::mutex> *slot_lk = nullptr) {
    *r = ScanResult();
    if (slot_lk) r->slot = free_slot(c, *slot_lk, true);
    ScanState &s = c->scan;
    s.have = false;
    const size_t hdr = header_bytes(c->format);
    if (in_len < hdr) return GZPX_OK;  // read_exact(header) finds nothing to read
    hipStream_t stream = c->stream;
    GZPX_TRY(order_behind(stream, after, c->ev_dep));
    // one wave per segment; 16 KiB each, larger where that keeps the single-workgroup scan of their counts short
    const size_t span = ((uintptr_t)d_in & 15u) + in_len;
    size_t seg_bytes = 16384;
    while ((span + seg_bytes - 1) / seg_bytes > 65536 && seg_bytes < ((size_t)1 << 30)) seg_bytes *= 2;
    const size_t n_seg = (span + seg_bytes - 1) / seg_bytes;
    if (n_seg > 0xFFFFFFFFull) return GZPX_ERR_INVALID_ARG;
    // Candidates: the members (in our own streams one per 20-odd KiB) and about one impostor per 2^17 bytes of
    // compressed data.  A stream of tiny members, or one built to look like that, finds the arrays too small: the
    // record says by how much, and the scan runs once more.
    const size_t kCapMax = 0xFFFFFFF0ull;
    size_t cap = in_len / 2048 + 4096;
    if (cap < s.ms.cap) cap = s.ms.cap;
    if (cap > kCapMax) cap = kCapMax;
    for (int attempt = 0;; attempt++) {
        const int rc = s.reserve(n_seg, cap);
        if (rc != GZPX_OK) return rc;
        // a walk has at most min(candidates, in_len / smallest member) members: that many indices to hand out
        size_t chain = in_len / (hdr + 8) + 1;
        if (chain > s.ms.cap) chain = s.ms.cap;
        uint32_t rounds = 0;
        while (rounds < 32 && ((size_t)1 << rounds) < chain) rounds++;
        if (attempt == 0) HIP_TRY(hipEventRecord(s.ev0, stream));
        launch_member_scan(c->format, d_in, in_len, (uint32_t)seg_bytes, (uint32_t)n_seg, rounds, s.ms, stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(s.ev1, stream));
        HIP_TRY(hipMemcpyAsync(s.h_rec, s.ms.rec, 32, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        const size_t n_cand = s.h_rec[0];
        if (n_cand <= s.ms.cap) break;
        if (n_cand > kCapMax || attempt) return GZPX_ERR_DEVICE;  // (more candidates than the 32-bit indices address)
        cap = n_cand + n_cand / 8 + 64;
        if (cap > kCapMax) cap = kCapMax;
    }
    s.have = true;
    r->invalid = s.h_rec[2] != 0;
    r->n_members = s.h_rec[1];
    r->consumed = (size_t)rec_u64(s.h_rec, 4);
    return GZPX_OK;
}

}  // namespace

extern "C" {

int gzpx_dctx_create(int device, int format, gzpx_dctx **out) {
    if (!out || (format != GZPX_FORMAT_BGZF && format != GZPX_FORMAT_MGZIP)) return GZPX_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GZPX_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return GZPX_ERR_INVALID_ARG;
    if (hipSetDevice(device) != hipSuccess) return GZPX_ERR_DEVICE;
    gzpx_dctx *c = new (std::nothrow) gzpx_dctx();
    if (!c) return GZPX_ERR_DEVICE;
    c->device = device;
    c->format = format;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
    }
    if (const char *e = getenv("GZPX_INFLATE_ROUTE"))
        if (!strcmp(e, "wave")) c->route = kInflateRouteWave;
    c->cc = crc_consts();
    if (c->stream.create() != GZPX_OK || c->s_h2d.create() != GZPX_OK || c->s_d2h.create() != GZPX_OK ||
        c->ev_dep.create() != GZPX_OK) {
        gzpx_dctx_destroy(c);
        return GZPX_ERR_DEVICE;
    }
    *out = c;
    return GZPX_OK;
}

void gzpx_dctx_destroy(gzpx_dctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (const Stream *st : {&c->stream, &c->s_h2d, &c->s_d2h}) st->sync();
    delete c;
}

int gzpx_scan_blocks(int format, const uint8_t *in, size_t in_len, uint64_t *offsets, uint32_t *sizes,
                     size_t max_blocks, size_t *n_blocks, size_t *consumed) {
    if ((!in && in_len) || !n_blocks || !consumed) return GZPX_ERR_INVALID_ARG;
    const size_t hdr = header_bytes(format);
    size_t pos = 0, nb = 0;
    *n_blocks = 0;
    *consumed = 0;
    while (in_len - pos >= hdr) {  // read_exact(header) succeeds
        const uint8_t *h = in + pos;
        if ((h[3] & 4) != 4) return GZPX_ERR_INVALID_HEADER;  // "Extra field flag not set"
        if (format == GZPX_FORMAT_BGZF ? (h[12] != 'B' || h[13] != 'C') : (h[12] != 'I' || h[13] != 'G'))
            return GZPX_ERR_INVALID_HEADER;  // "Bad SID"
        const size_t size = format == GZPX_FORMAT_BGZF
                                ? (size_t)(h[16] | (h[17] << 8)) + 1
                                : (size_t)h[16] | ((size_t)h[17] << 8) | ((size_t)h[18] << 16) | ((size_t)h[19] << 24);
        if (size < hdr + 8) return GZPX_ERR_INVALID_HEADER;
        if (in_len - pos < size) break;  // read_exact(remainder) would wait for more input
        if (offsets && sizes) {
            if (nb >= max_blocks) break;
            offsets[nb] = pos;
            sizes[nb] = (uint32_t)size;
        }
        nb++;
        pos += size;
    }
    *n_blocks = nb;
    *consumed = pos;
    return GZPX_OK;
}

int gzpx_decompress_blocks_submit(gzpx_dctx *c, const uint8_t *in, size_t in_len, const uint64_t *offsets,
                                  const uint32_t *sizes, size_t n_blocks, uint8_t *out, size_t out_cap,
                                  uint64_t *ticket) {
    if (!c || (!in && in_len) || (!out && out_cap) || !ticket) return GZPX_ERR_INVALID_ARG;
    std::unique_lock<std::mutex> lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    return dsubmit_enqueue(c, in, nullptr, in_len, offsets, sizes, n_blocks, out, nullptr, out_cap, nullptr, false,
                           lk, ticket);
}

int gzpx_decompress_blocks_wait(gzpx_dctx *c, uint64_t ticket, size_t *out_len, gzpx_check_info *info) {
    if (!c) return GZPX_ERR_INVALID_ARG;
    return dwait_ticket(c, ticket, out_len, info);
}

int gzpx_decompress_blocks_device(gzpx_dctx *c, const void *d_in, size_t in_len, const uint64_t *offsets,
                                  const uint32_t *sizes, size_t n_blocks, void *d_out, size_t out_cap,
                                  size_t *out_len, gzpx_check_info *info, void *hip_stream) {
    if (!c || !out_len) return GZPX_ERR_INVALID_ARG;
    *out_len = 0;
    if (n_blocks == 0) return GZPX_OK;
    uint64_t ticket = 0;
    int rc;
    {
        std::unique_lock<std::mutex> lk(c->mu);
        if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
        rc = dsubmit_enqueue(c, nullptr, (const uint8_t *)d_in, in_len, offsets, sizes, n_blocks, nullptr,
                             (uint8_t *)d_out, out_cap, (hipStream_t)hip_stream, true, lk, &ticket);
    }
    if (rc != GZPX_OK) return rc;
    return dwait_ticket(c, ticket, out_len, info);
}

int gzpx_scan_blocks_device(gzpx_dctx *c, const void *d_in, size_t in_len, uint64_t *offsets, uint32_t *sizes,
                            size_t max_blocks, size_t *n_blocks, size_t *consumed, void *hip_stream) {
    if (!c || (!d_in && in_len) || !n_blocks || !consumed) return GZPX_ERR_INVALID_ARG;
    *n_blocks = 0;
    *consumed = 0;
    std::unique_lock<std::mutex> lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    ScanResult r;
    const int rc = dscan_run(c, (const uint8_t *)d_in, in_len, (hipStream_t)hip_stream, &r);
    if (rc != GZPX_OK) return rc;
    const bool tables = offsets && sizes;  // (no tables: the cap is not looked at, as on the host)
    if (r.invalid && !(tables && max_blocks < r.n_members)) return GZPX_ERR_INVALID_HEADER;
    if (!tables || r.n_members == 0) {
        *n_blocks = r.n_members;
        *consumed = r.consumed;
        return GZPX_OK;
    }
    // with the cap reached in front of a whole member the walk stops there: that member's offset is `consumed`
    const bool capped = max_blocks < r.n_members;
    const size_t n = capped ? max_blocks : r.n_members, n_emit = capped ? n + 1 : n;
    ScanState &s = c->scan;
    GZPX_TRY(grow(s.tab_mem, s.tab_cap, n_emit, n_emit + n_emit / 4 + 64, [&](size_t cap) -> int {
        GZPX_TRY(s.tab_mem.dev(s.d_tab_off, cap * 8));
        return s.tab_mem.dev(s.d_tab_size, cap * 4);
    }));
    launch_member_emit(s.ms, (uint32_t)n_emit, s.d_tab_off, s.d_tab_size, c->stream);
    HIP_TRY(hipGetLastError());
    uint64_t stop = 0;
    if (n) HIP_TRY(hipMemcpyAsync(offsets, s.d_tab_off, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (n) HIP_TRY(hipMemcpyAsync(sizes, s.d_tab_size, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (capped) HIP_TRY(hipMemcpyAsync(&stop, s.d_tab_off + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_blocks = n;
    *consumed = capped ? (size_t)stop : r.consumed;
    return GZPX_OK;
}

int gzpx_decompress_stream_device(gzpx_dctx *c, const void *d_in, size_t in_len, void *d_out, size_t out_cap,
                                  size_t *out_len, size_t *n_blocks, size_t *consumed, gzpx_check_info *info,
                                  void *hip_stream) {
    if (!c || (!d_in && in_len) || !out_len || !n_blocks || !consumed) return GZPX_ERR_INVALID_ARG;
    *out_len = 0;
    *n_blocks = 0;
    *consumed = 0;
    uint64_t ticket = 0;
    int rc;
    {
        std::unique_lock<std::mutex> lk(c->mu);
        if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
        ScanResult r;
        rc = dscan_run(c, (const uint8_t *)d_in, in_len, (hipStream_t)hip_stream, &r, &lk);
        if (rc != GZPX_OK) return rc;
        if (r.invalid) return GZPX_ERR_INVALID_HEADER;
        *n_blocks = r.n_members;
        *consumed = r.consumed;
        if (r.n_members == 0) return GZPX_OK;
        rc = dsubmit_enqueue(c, nullptr, (const uint8_t *)d_in, in_len, nullptr, nullptr, r.n_members, nullptr,
                             (uint8_t *)d_out, out_cap, (hipStream_t)hip_stream, true, lk, &ticket, &r);
    }
    if (rc != GZPX_OK) return rc;
    return dwait_ticket(c, ticket, out_len, info);
}

int gzpx_index_device(gzpx_dctx *c, const void *d_in, size_t in_len, gzpx_index_entry *entries, size_t max_entries,
                      size_t *n_entries, size_t *consumed, uint64_t *inflated_len, void *hip_stream) {
    if (!c || (!d_in && in_len) || !n_entries || !consumed) return GZPX_ERR_INVALID_ARG;
    *n_entries = 0;
    *consumed = 0;
    if (inflated_len) *inflated_len = 0;
    std::unique_lock<std::mutex> lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    ScanResult r;
    const int rc = dscan_run(c, (const uint8_t *)d_in, in_len, (hipStream_t)hip_stream, &r, &lk);
    if (rc != GZPX_OK) return rc;
    if (r.invalid) return GZPX_ERR_INVALID_HEADER;
    *n_entries = r.n_members;
    *consumed = r.consumed;
    if (r.n_members == 0) return GZPX_OK;
    if (r.n_members > 0xFFFFFFFFull) return GZPX_ERR_INVALID_ARG;
    DSlot &sl = c->slots[r.slot];  // (its tables only; the slot stays free, the call returns synchronised under the lock)
    const int rr = dslot_reserve(sl, r.n_members);
    if (rr != GZPX_OK) return rr;
    const uint32_t nb = (uint32_t)r.n_members;
    launch_member_emit(c->scan.ms, nb, sl.d_offsets, sl.d_sizes, c->stream);
    launch_member_index((const uint8_t *)d_in, sl.d_offsets, sl.d_sizes, nb, sl.d_blk, sl.d_out_off, c->stream);
    HIP_TRY(hipGetLastError());
    const size_t n_copy = entries ? (r.n_members < max_entries ? r.n_members : max_entries) : 0;
    std::vector<uint64_t> un(n_copy);
    if (n_copy) {
        HIP_TRY(hipMemcpyAsync(sl.h_offsets, sl.d_offsets, n_copy * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(un.data(), sl.d_out_off, n_copy * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(sl.h_total, sl.d_out_off + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n_copy; i++) entries[i] = gzpx_index_entry{sl.h_offsets[i], un[i]};
    if (inflated_len) *inflated_len = *sl.h_total;
    return GZPX_OK;
}

int gzpx_dctx_last_scan_ms(gzpx_dctx *ctx, float *ms) {
    if (!ctx || !ms) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    *ms = 0.0f;
    if (!ctx->scan.have) return GZPX_OK;
    return hipEventElapsedTime(ms, ctx->scan.ev0, ctx->scan.ev1) == hipSuccess ? GZPX_OK : GZPX_ERR_DEVICE;
}

}  // extern "C"

struct gzpx_dindex : NoCopy {
    int device = 0, format = 0;
    size_t n = 0, consumed = 0;
    uint64_t inflated_len = 0;
    uint64_t *d_off = nullptr;     // [n]
    uint32_t *d_size = nullptr;    // [n]
    uint64_t *d_ustart = nullptr;  // [n + 1]
    Allocs mem;
};

extern "C" {

void gzpx_dindex_destroy(gzpx_dindex *ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    delete ix;
}

int gzpx_dindex_build_device(gzpx_dctx *c, const void *d_in, size_t in_len, gzpx_dindex **out, size_t *n_members,
                             size_t *consumed, uint64_t *inflated_len, void *hip_stream) {
    if (!c || (!d_in && in_len) || !out) return GZPX_ERR_INVALID_ARG;
    *out = nullptr;
    if (n_members) *n_members = 0;
    if (consumed) *consumed = 0;
    if (inflated_len) *inflated_len = 0;
    std::unique_lock<std::mutex> lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    ScanResult r;
    int rc = dscan_run(c, (const uint8_t *)d_in, in_len, (hipStream_t)hip_stream, &r, &lk);
    if (rc != GZPX_OK) return rc;
    if (r.invalid) return GZPX_ERR_INVALID_HEADER;
    if (r.n_members > 0xFFFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    std::unique_ptr<gzpx_dindex> ix(new (std::nothrow) gzpx_dindex());  // (c's device is current: a return frees it)
    if (!ix) return GZPX_ERR_DEVICE;
    ix->device = c->device;
    ix->format = c->format;
    ix->n = r.n_members;
    ix->consumed = r.consumed;
    const size_t n = r.n_members;
    Drain drain{{c->stream}, 1};  // (a failure: nothing still runs on the arrays when they are freed)
    GZPX_TRY(ix->mem.dev(ix->d_off, (n ? n : 1) * 8));
    GZPX_TRY(ix->mem.dev(ix->d_size, (n ? n : 1) * 4));
    GZPX_TRY(ix->mem.dev(ix->d_ustart, (n + 1) * 8));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(ix->d_ustart, 0, 8, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    } else {
        DSlot &sl = c->slots[r.slot];  // (its member records only; the slot stays free, the call returns synchronised under the lock)
        GZPX_TRY(dslot_reserve(sl, n));
        launch_member_emit(c->scan.ms, (uint32_t)n, ix->d_off, ix->d_size, c->stream);
        launch_member_index((const uint8_t *)d_in, ix->d_off, ix->d_size, (uint32_t)n, sl.d_blk, ix->d_ustart, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(sl.h_total, ix->d_ustart + n, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        ix->inflated_len = *sl.h_total;
    }
    drain.armed = false;
    if (n_members) *n_members = ix->n;
    if (consumed) *consumed = ix->consumed;
    if (inflated_len) *inflated_len = ix->inflated_len;
    *out = ix.release();
    return GZPX_OK;
}

int gzpx_dindex_entries(const gzpx_dindex *ix, gzpx_index_entry *entries, size_t max_entries, size_t *n_entries) {
    if (!ix || !n_entries) return GZPX_ERR_INVALID_ARG;
    *n_entries = ix->n;
    const size_t n_copy = entries ? (ix->n < max_entries ? ix->n : max_entries) : 0;
    if (!n_copy) return GZPX_OK;
    if (hipSetDevice(ix->device) != hipSuccess) return GZPX_ERR_DEVICE;
    std::vector<uint64_t> off(n_copy), un(n_copy);
    HIP_TRY(hipMemcpy(off.data(), ix->d_off, n_copy * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(un.data(), ix->d_ustart, n_copy * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n_copy; i++) entries[i] = gzpx_index_entry{off[i], un[i]};
    return GZPX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- indexed reads: the steps the calls below share
namespace {

// an index and a context that belong together, and a stream at least as long as the index says
bool index_matches(const gzpx_dctx *c, const gzpx_dindex *ix, size_t in_len) {
    return ix->device == c->device && ix->format == c->format && in_len >= ix->consumed;
}

// (the stream's average member stands for each of nb members of it: InflateScratch::in_bytes)
uint64_t average_in_bytes(const gzpx_dindex *ix, size_t nb) { return (uint64_t)(ix->consumed / ix->n) * nb; }

// the ranges' record behind locate + select: the first bad item (0xFFFFFFFF: none), the members the items touch, what
// those inflate to, the items' bytes
struct Selection {
    uint32_t bad;
    size_t n;
    uint64_t stage_bytes, total;
};

Selection selection_read(const gzpx_dctx *c) {
    const uint32_t *rec = c->ranges.h_rec;
    return Selection{rec[kRrRecBad], rec[kRrRecSelected], rec_u64(rec, kRrRecStage), rec_u64(rec, kRrRecTotal)};
}

// The first half of "select, then inflate the selection": `bytes` of the caller's items go through h_ranges to
// `d_items`, and between ev[0] and ev[1] the kernels `pre` enqueues (the line calls': boundaries to tile covers) and
// locate + select run, which leave the selected members' table in the slot's.  The caller copies the records it
// reads back, synchronises -- the one round trip in front of the inflate -- and reads selection_read().
// `on_device`: the items lie in device memory and come by a device-to-device copy behind whatever the context's stream
// was ordered behind; nothing of them touches the host.
template <class Pre>
int select_enqueue(gzpx_dctx *c, DSlot &sl, const gzpx_dindex *ix, const void *items, bool on_device, size_t bytes, void *d_items,
                   size_t n, int is_virtual, Event *ev, Pre &&pre) {
    RangesState &r = c->ranges;
    const RrIndex rix{ix->d_off, ix->d_size, ix->d_ustart, (uint32_t)ix->n};
    if (on_device) {
        HIP_TRY(hipMemcpyAsync(d_items, items, bytes, hipMemcpyDeviceToDevice, c->stream));
    } else {
        memcpy(r.h_ranges, items, bytes);  // (room for 16 bytes an item)
        HIP_TRY(hipMemcpyAsync(d_items, r.h_ranges, bytes, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipEventRecord(ev[0], c->stream));
    pre();
    launch_ranges_select(rix, (uint32_t)n, is_virtual, r.rr, sl.d_offsets, sl.d_sizes, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], c->stream));
    return GZPX_OK;
}

// The second half: the selected members into staging, which the caller has reserved.  (The pair's scratch is sized by
// the staging; the members' records stay on the device, under gzpx_debug_inflate too.)
int inflate_selection(gzpx_dctx *c, DSlot &sl, const gzpx_dindex *ix, const uint8_t *d_in, const Selection &s,
                      hipEvent_t ev_before = nullptr) {
    return inflate_enqueue(c, sl, d_in, sl.d_offsets, sl.d_sizes, s.n, c->stage.d, (size_t)s.stage_bytes,
                           average_in_bytes(ix, s.n), ev_before);
}

// The verdict on an inflated selection (the stream idle): a failure names the first failing member of the selection in
// stream order by its index in the stream, through the rank map.
int selection_verdict(gzpx_dctx *c, const DSlot &sl, gzpx_check_info *info) {
    gzpx_check_info failed = {0, 0, 0};
    const int verdict = summary_verdict(sl.h_summary, false, &failed);
    if (verdict == GZPX_OK) return GZPX_OK;
    uint32_t member = 0;
    HIP_TRY(hipMemcpy(&member, c->ranges.rr.map + failed.block, 4, hipMemcpyDeviceToHost));
    failed.block = member;
    if (info) *info = failed;
    return verdict;
}

// The whole members of an index in batches of at most the context's lines_batch inflated bytes, a larger member on
// its own: batch k is members [cuts[k], cuts[k + 1]).  Cut on the host from the index's prefix sums.
struct Batches {
    std::vector<uint64_t> ustart;
    std::vector<size_t> cuts;
    uint64_t max_bytes = 0;
    size_t max_members = 1;
};

int batches_of(const gzpx_dctx *c, const gzpx_dindex *ix, Batches &b) {
    const size_t n = ix->n;
    b.ustart.assign(n + 1, 0);
    if (n) HIP_TRY(hipMemcpy(b.ustart.data(), ix->d_ustart, (n + 1) * 8, hipMemcpyDeviceToHost));
    const uint64_t batch = c->lines.batch ? c->lines.batch : kLinesBatchDefault;
    b.cuts.assign(1, 0);
    for (size_t m0 = 0; m0 < n;) {
        size_t m1 = m0 + 1;
        while (m1 < n && b.ustart[m1 + 1] - b.ustart[m0] <= batch) m1++;
        if (b.ustart[m1] - b.ustart[m0] > b.max_bytes) b.max_bytes = b.ustart[m1] - b.ustart[m0];
        if (m1 - m0 > b.max_members) b.max_members = m1 - m0;
        b.cuts.push_back(m1);
        m0 = m1;
    }
    return GZPX_OK;
}

// One pass over every member of an index, batch by batch through staging (c->mu held, slot `si` free and the caller's
// for the call, `drain` the caller's on the context's stream).  Slot and staging are reserved for the largest batch,
// `pad` bytes in front of where the inflate writes.  Per batch: the caller's ev[0] is recorded, the batch inflated, and
// enqueue(base, bytes, is_last) puts the caller's kernels behind it, each followed by the next of ev[1..n_ms] --
// without asking how the inflate went: whatever staging holds, they stay inside it.  Then the stream is synchronised
// (staging is the next batch's too; the verdict decides whether there is one), the n_ms times between the events are
// added to the caller's sums (all of them or none), and a failing verdict ends the pass with the member's index in
// the stream.
template <class Enqueue>
int batched_pass(gzpx_dctx *c, int si, const gzpx_dindex *ix, const Batches &b, const uint8_t *d_in, size_t pad,
                 const Event *ev, int n_ms, float *ms_sums, gzpx_check_info *info, Drain &drain, Enqueue &&enqueue) {
    DSlot &sl = c->slots[si];
    GZPX_TRY(dslot_reserve(sl, b.max_members));
    GZPX_TRY(c->stage.reserve(pad + b.max_bytes));
    for (size_t k = 0; k + 1 < b.cuts.size(); k++) {
        const size_t m0 = b.cuts[k], nb = b.cuts[k + 1] - m0;
        const uint64_t base = b.ustart[m0], bytes = b.ustart[m0 + nb] - base;
        GZPX_TRY(inflate_enqueue(c, sl, d_in, ix->d_off + m0, ix->d_size + m0, nb, c->stage.d + pad, (size_t)bytes,
                                 average_in_bytes(ix, nb), ev[0]));
        GZPX_TRY(enqueue(base, bytes, k + 2 == b.cuts.size()));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->last_slot = si;
        c->last_nb = nb;
        float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int timed = 0;
        while (timed < n_ms && hipEventElapsedTime(&ms[timed], ev[timed], ev[timed + 1]) == hipSuccess) timed++;
        for (int j = 0; timed == n_ms && j < n_ms; j++) ms_sums[j] += ms[j];
        gzpx_check_info failed = {0, 0, 0};
        const int verdict = summary_verdict(sl.h_summary, false, &failed);
        if (verdict != GZPX_OK) {
            failed.block += m0;
            if (info) *info = failed;
            drain.armed = false;
            return verdict;
        }
    }
    return GZPX_OK;
}

// The record of a call on a table of members (kWrRec*: k_dresult's, k_dresult_sizes', k_cksum_record's) as the call's
// return code: how many failed, the total where the call has one, and the first failing member with its two
// checksums -- `sums` false (the sizes call, which verifies none): 0 and 0.
int result_verdict(const uint32_t *q, size_t *n_failed, uint64_t *total, gzpx_check_info *info, bool sums = true) {
    if (total) *total = rec_u64(q, kWrRecTotal);
    *n_failed = q[kWrRecFailed];
    if (q[kWrRecFirst] == 0xFFFFFFFFu) return GZPX_OK;
    if (info) *info = gzpx_check_info{q[kWrRecFirst], sums ? q[kWrRecFound] : 0u, sums ? q[kWrRecExpected] : 0u};
    return (int)q[kWrRecStatus];
}

}  // namespace

extern "C" {

int gzpx_read_ranges_device(gzpx_dctx *c, const gzpx_dindex *ix, const void *d_in, size_t in_len,
                            const gzpx_range *ranges, size_t n_ranges, int coords, void *d_out, size_t out_cap,
                            size_t *out_len, uint64_t *out_offsets, size_t *bad_range, gzpx_check_info *info,
                            void *hip_stream) {
    if (!c || !ix || !out_len || (!ranges && n_ranges) || (!d_in && in_len) || (!d_out && out_cap))
        return GZPX_ERR_INVALID_ARG;
    *out_len = 0;
    if (bad_range) *bad_range = (size_t)-1;
    if (coords != GZPX_RANGE_UNCOMPRESSED && coords != GZPX_RANGE_VIRTUAL) return GZPX_ERR_INVALID_ARG;
    if (coords == GZPX_RANGE_VIRTUAL && c->format != GZPX_FORMAT_BGZF) return GZPX_ERR_INVALID_ARG;
    if (!index_matches(c, ix, in_len)) return GZPX_ERR_INVALID_ARG;
    if (n_ranges > 0xFFFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    std::unique_lock<std::mutex> lk(c->mu);
    RangesState &r = c->ranges;
    r.have = r.stages = false;
    r.last_members = 0;
    if (n_ranges == 0) {
        if (out_offsets) out_offsets[0] = 0;
        return GZPX_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    const int si = free_slot(c, lk, true);
    DSlot &sl = c->slots[si];  // (stays free: the call returns synchronised under the lock)
    GZPX_TRY(dslot_reserve(sl, ix->n ? ix->n : 1));
    GZPX_TRY(r.reserve(n_ranges, ix->n));
    hipStream_t stream = c->stream;
    GZPX_TRY(order_behind(stream, (hipStream_t)hip_stream, c->ev_dep));
    Drain drain{{stream}, 1};
    GZPX_TRY(select_enqueue(c, sl, ix, ranges, false, n_ranges * sizeof(gzpx_range), r.rr.ranges, n_ranges,
                            coords == GZPX_RANGE_VIRTUAL, r.ev, [] {}));
    HIP_TRY(hipMemcpyAsync(r.h_rec, r.rr.rec, 32, hipMemcpyDeviceToHost, stream));
    if (out_offsets)
        HIP_TRY(hipMemcpyAsync(r.h_out_off, r.rr.out_off, (n_ranges + 1) * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // the record: the one round trip in front of the inflate
    r.have = true;
    const Selection sel = selection_read(c);
    if (sel.bad != 0xFFFFFFFFu) {
        if (bad_range) *bad_range = sel.bad;
        return GZPX_ERR_INVALID_ARG;
    }
    if (sel.total > out_cap) {
        *out_len = (size_t)sel.total;
        return GZPX_ERR_INSUFFICIENT_SPACE;
    }
    if (sel.total >> 44) return GZPX_ERR_INVALID_ARG;  // (the gather's grid)
    if (out_offsets) memcpy(out_offsets, r.h_out_off, (n_ranges + 1) * 8);
    r.last_members = sel.n;
    if (sel.n == 0) {  // empty ranges only
        drain.armed = false;
        return GZPX_OK;
    }
    GZPX_TRY(c->stage.reserve(sel.stage_bytes));
    GZPX_TRY(inflate_selection(c, sl, ix, (const uint8_t *)d_in, sel, r.ev[2]));
    HIP_TRY(hipEventRecord(r.ev[3], stream));
    // (enqueued behind the inflate without asking how it went: after a failed check d_out holds nothing of use)
    launch_ranges_gather(c->stage.d, (uint32_t)n_ranges, r.rr, (uint8_t *)d_out, sel.total, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r.ev[4], stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    r.stages = true;
    c->last_slot = si;
    c->last_nb = sel.n;
    GZPX_TRY(selection_verdict(c, sl, info));
    *out_len = (size_t)sel.total;
    return GZPX_OK;
}

int gzpx_inflate_batch_device(gzpx_dctx *c, int wrap, unsigned flags, const void *d_in, size_t in_len,
                              const uint64_t *d_in_offsets, const uint32_t *d_in_sizes, const uint32_t *d_out_sizes,
                              size_t n, void *d_out, size_t out_cap, uint64_t *d_out_offsets,
                              gzpx_member_result *d_results, size_t *out_len, size_t *n_failed, gzpx_check_info *info,
                              void *hip_stream) {
    static_assert(sizeof(gzpx_member_result) == 16, "k_dresult writes this layout");
    if (!c || !out_len || !n_failed || (!d_in && in_len) || (!d_out && out_cap)) return GZPX_ERR_INVALID_ARG;
    *out_len = 0;
    *n_failed = 0;
    if (wrap != GZPX_WRAP_RAW && wrap != GZPX_WRAP_ZLIB && wrap != GZPX_WRAP_GZIP) return GZPX_ERR_INVALID_ARG;
    if (flags & ~GZPX_BATCH_SHORT_OK) return GZPX_ERR_INVALID_ARG;
    const bool short_ok = (flags & GZPX_BATCH_SHORT_OK) != 0;
    if (short_ok && (wrap == GZPX_WRAP_GZIP || !d_out_sizes)) return GZPX_ERR_INVALID_ARG;
    if (!d_out_sizes && wrap != GZPX_WRAP_GZIP) return GZPX_ERR_INVALID_ARG;  // (only a gzip trailer states a size)
    if (n && (!d_in_offsets || !d_in_sizes)) return GZPX_ERR_INVALID_ARG;
    if (n > 0xFFFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    std::unique_lock<std::mutex> lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    hipStream_t stream = c->stream;
    if (n == 0) {
        if (d_out_offsets) {
            HIP_TRY(hipMemsetAsync(d_out_offsets, 0, 8, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        return GZPX_OK;
    }
    const int si = free_slot(c, lk, true);
    DSlot &sl = c->slots[si];  // (stays free: the call returns synchronised under the lock)
    GZPX_TRY(dslot_reserve(sl, n));
    GZPX_TRY(order_behind(stream, (hipStream_t)hip_stream, c->ev_dep));
    Drain drain{{stream}, 1};
    // (fewer bytes than the slot are k_inflate's to see; the sizes are on the device: the input stands for their sum)
    GZPX_TRY(dslot_prepare(c, sl, n, short_ok ? (int)kInflateRouteWave : c->route, out_cap, in_len));
    // the slot's own size table is free here (the caller's is read where it lies): it holds the members' slots
    launch_inflate_batch(inflate_launch_of(c, sl, (const uint8_t *)d_in, sl.d_out_off, (uint8_t *)d_out, out_cap), wrap,
                         short_ok ? 1 : 0, in_len, d_in_offsets, d_in_sizes, d_out_sizes, sl.d_sizes, d_out_offsets, d_results);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sl.h_summary, sl.sc.summary, kWrRecHostWords * 4, hipMemcpyDeviceToHost, stream));
    GZPX_TRY(debug_records(c, sl, n));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    sl.have_check = true;
    c->last_slot = si;
    c->last_nb = n;
    uint64_t total = 0;
    const int verdict = result_verdict(sl.h_summary, n_failed, &total, info);  // k_dresult's record
    *out_len = (size_t)total;
    return verdict;
}

int gzpx_inflate_batch_sizes_device(gzpx_dctx *c, int wrap, const void *d_in, size_t in_len, const uint64_t *d_in_offsets,
                                    const uint32_t *d_in_sizes, size_t n, uint32_t max_out_size, uint32_t *d_out_sizes,
                                    uint32_t *d_in_used, gzpx_member_result *d_results, uint64_t *total_out, size_t *n_failed,
                                    gzpx_check_info *info, void *hip_stream) {
    if (!c || !total_out || !n_failed || (!d_in && in_len)) return GZPX_ERR_INVALID_ARG;
    *total_out = 0;
    *n_failed = 0;
    if (wrap != GZPX_WRAP_RAW && wrap != GZPX_WRAP_ZLIB && wrap != GZPX_WRAP_GZIP) return GZPX_ERR_INVALID_ARG;
    if (n && (!d_in_offsets || !d_in_sizes || !d_out_sizes)) return GZPX_ERR_INVALID_ARG;
    if (n > 0xFFFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    std::unique_lock<std::mutex> lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    hipStream_t stream = c->stream;
    if (n == 0) return GZPX_OK;
    const int si = free_slot(c, lk, true);
    DSlot &sl = c->slots[si];  // (stays free: the call returns synchronised under the lock)
    GZPX_TRY(dslot_reserve(sl, n));
    GZPX_TRY(order_behind(stream, (hipStream_t)hip_stream, c->ev_dep));
    Drain drain{{stream}, 1};
    // (nothing is inflated: a capacity of 0 and no scratch of the decode / copy pair; the input stands for the members' sum)
    GZPX_TRY(dslot_prepare(c, sl, n, c->route, 0, in_len, false));
    launch_inflate_sizes(inflate_launch_of(c, sl, (const uint8_t *)d_in, nullptr, nullptr, 0), wrap, in_len, d_in_offsets,
                         d_in_sizes, max_out_size, d_out_sizes, d_in_used, d_results);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sl.h_summary, sl.sc.summary, kWrRecHostWords * 4, hipMemcpyDeviceToHost, stream));
    GZPX_TRY(debug_records(c, sl, n));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    c->last_slot = si;
    c->last_nb = n;
    return result_verdict(sl.h_summary, n_failed, total_out, info, false);  // k_dresult_sizes' record
}

int gzpx_checksum_batch_device(gzpx_dctx *c, int kind, const void *d_in, size_t in_len, const uint64_t *d_offsets,
                               const uint32_t *d_sizes, size_t n, const uint32_t *d_seeds, const uint32_t *d_expected,
                               uint32_t *d_sums, gzpx_member_result *d_results, size_t *n_failed, gzpx_check_info *info,
                               void *hip_stream) {
    static_assert(sizeof(gzpx_member_result) == 16, "k_cksum_finish writes this layout");
    if (!c || !n_failed || !info || (!d_in && in_len) || !d_offsets) return GZPX_ERR_INVALID_ARG;
    *n_failed = 0;
    if (kind != GZPX_CHECK_CRC32 && kind != GZPX_CHECK_ADLER32 && kind != GZPX_CHECK_CRC32C) return GZPX_ERR_INVALID_ARG;
    if (!d_sums && !d_expected) return GZPX_ERR_INVALID_ARG;
    if (n > 0xFFFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    std::unique_lock<std::mutex> lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    if (n == 0) return GZPX_OK;
    hipStream_t stream = c->stream;
    const int si = free_slot(c, lk, true);
    DSlot &sl = c->slots[si];  // (stays free: the call returns synchronised under the lock; its events and record serve)
    GZPX_TRY(dslot_reserve(sl, 1));
    const uint32_t wgs = cksum_workgroups(c->n_cu, c->cksum.width);
    GZPX_TRY(c->cksum.reserve(n, wgs));
    c->cksum.ck.rec = sl.sc.summary;
    GZPX_TRY(order_behind(stream, (hipStream_t)hip_stream, c->ev_dep));
    Drain drain{{stream}, 1};
    sl.have_blk = sl.have_check = false;
    HIP_TRY(hipEventRecord(sl.ev_t1, stream));
    launch_cksum_batch(kind, (const uint8_t *)d_in, in_len, d_offsets, d_sizes, (uint32_t)n, d_seeds, d_expected, d_sums,
                       d_results, c->cksum.ck, wgs, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sl.ev_tc, stream));
    HIP_TRY(hipMemcpyAsync(sl.h_summary, sl.sc.summary, kWrRecHostWords * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    sl.have_check = true;
    c->last_slot = si;
    c->last_nb = 0;  // (no member was inflated: the inflate getters answer 0)
    return result_verdict(sl.h_summary, n_failed, nullptr, info);  // k_cksum_record's record
}

int gzpx_dctx_set_checksum_width(gzpx_dctx *ctx, unsigned workgroups) {
    if (!ctx || workgroups > 65536u) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->cksum.width = workgroups;
    return GZPX_OK;
}

int gzpx_dctx_last_check_ms(gzpx_dctx *ctx, float *ms) {
    if (!ctx || !ms) return GZPX_ERR_INVALID_ARG;
    *ms = 0.0f;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (ctx->last_slot < 0 || !ctx->slots[ctx->last_slot].have_check) return GZPX_OK;
    const DSlot &sl = ctx->slots[ctx->last_slot];
    if (hipEventElapsedTime(ms, sl.ev_t1, sl.ev_tc) != hipSuccess) return GZPX_ERR_DEVICE;
    return GZPX_OK;
}

int gzpx_dctx_last_ranges_members(gzpx_dctx *ctx, size_t *n_members_read) {
    if (!ctx || !n_members_read) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    *n_members_read = ctx->ranges.last_members;
    return GZPX_OK;
}

int gzpx_dctx_last_ranges_ms(gzpx_dctx *ctx, float ms[3]) {
    if (!ctx || !ms) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    ms[0] = ms[1] = ms[2] = 0.0f;
    const RangesState &r = ctx->ranges;
    if (!r.have) return GZPX_OK;
    if (hipEventElapsedTime(&ms[0], r.ev[0], r.ev[1]) != hipSuccess) return GZPX_ERR_DEVICE;
    if (!r.stages) return GZPX_OK;
    if (hipEventElapsedTime(&ms[1], r.ev[2], r.ev[3]) != hipSuccess || hipEventElapsedTime(&ms[2], r.ev[3], r.ev[4]) != hipSuccess)
        return GZPX_ERR_DEVICE;
    return GZPX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- reads by line (gzpx_lines.h)
struct gzpx_dlines : NoCopy {
    int device = 0, format = 0;  // the index the table was built for
    size_t n = 0, consumed = 0;
    uint64_t inflated_len = 0;
    uint32_t delim = 0, tiles = 0;
    uint64_t n_delims = 0, n_lines = 0;
    uint64_t *d_prefix = nullptr;  // [tiles + 1] P
    uint32_t *d_rec = nullptr;     // [8] kLnRec*: D, L, whether the last byte is a delimiter
    Allocs mem;
};

namespace {

// a table, an index and a context that belong together, and a stream at least as long as the index says
bool lines_match(const gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, size_t in_len) {
    return index_matches(c, ix, in_len) && lt->device == ix->device && lt->format == ix->format && lt->n == ix->n &&
           lt->consumed == ix->consumed && lt->inflated_len == ix->inflated_len;
}

// What the two line calls share (c->mu held, slot `si` free and the caller's for the call): n items of `per`
// boundaries each -- line numbers, or (a, b) of line ranges -- are validated, the covers of their tiles located and
// selected, the selected members inflated into staging and the boundary tiles walked there.  Two round trips: the
// record in front of the inflate, the positions behind the walk.  Returns with the stream idle; l.h_bpos then holds
// start() of every boundary and, per == 2, c->ranges (rr, h_out_off) and *total describe the gather that is still to run.
// `on_device`: `bounds` lies in device memory and is read where it lies, behind `after`; l.h_bpos and r.h_out_off stay
// unwritten (the caller copies l.ln.bpos and r.rr.out_off on the device), so no table sized by n touches the host.  The
// two records and their round trips are the same.
int lines_search(gzpx_dctx *c, int si, const gzpx_dindex *ix, const gzpx_dlines *lt, const uint8_t *d_in, const uint64_t *bounds,
                 size_t n, uint32_t per, size_t *bad, gzpx_check_info *info, hipStream_t after, uint64_t *total,
                 bool on_device = false) {
    DSlot &sl = c->slots[si];
    RangesState &r = c->ranges;
    LinesState &l = c->lines;
    GZPX_TRY(dslot_reserve(sl, ix->n ? ix->n : 1));
    GZPX_TRY(r.reserve(n, ix->n, !on_device));
    GZPX_TRY(l.reserve(n * per, !on_device));
    hipStream_t stream = c->stream;
    GZPX_TRY(order_behind(stream, after, c->ev_dep));
    Drain drain{{stream}, 1};
    const LnTable tb{lt->d_prefix, lt->tiles, lt->n_delims, lt->n_lines, lt->inflated_len};
    GZPX_TRY(select_enqueue(c, sl, ix, bounds, on_device, n * per * 8, l.ln.bounds, n, 0, l.ev,
                            [&] { launch_lines_tiles(tb, (uint32_t)n, per, l.ln, r.rr, stream); }));
    HIP_TRY(hipMemcpyAsync(l.h_rec, l.ln.rec, 32, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(r.h_rec, r.rr.rec, 32, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // the record: the round trip in front of the inflate
    l.stages = 1;
    const Selection sel = selection_read(c);
    if (l.h_rec[kLnRecBad] != 0xFFFFFFFFu || sel.bad != 0xFFFFFFFFu) {
        if (bad) *bad = l.h_rec[kLnRecBad] != 0xFFFFFFFFu ? l.h_rec[kLnRecBad] : sel.bad;
        return GZPX_ERR_INVALID_ARG;
    }
    GZPX_TRY(c->stage.reserve(sel.stage_bytes));
    HIP_TRY(hipEventRecord(l.ev[2], stream));  // (recorded with nothing selected too, unlike a read by byte range)
    if (sel.n) GZPX_TRY(inflate_selection(c, sl, ix, d_in, sel));
    HIP_TRY(hipEventRecord(l.ev[3], stream));
    // (enqueued behind the inflate without asking how it went: whatever staging holds, the walk stays inside its tiles)
    launch_lines_find(tb, (uint32_t)n, per, lt->delim, l.ln, r.rr, c->stage.d, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(l.ev[4], stream));
    if (!on_device) HIP_TRY(hipMemcpyAsync(l.h_bpos, l.ln.bpos, n * per * 8, hipMemcpyDeviceToHost, stream));
    if (per == 2u) {
        HIP_TRY(hipMemcpyAsync(l.h_rec, l.ln.rec, 32, hipMemcpyDeviceToHost, stream));
        if (!on_device) HIP_TRY(hipMemcpyAsync(r.h_out_off, r.rr.out_off, (n + 1) * 8, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));  // the positions: the total is known only now
    drain.armed = false;
    l.stages = 3;
    if (sel.n) {
        c->last_slot = si;
        c->last_nb = sel.n;
        GZPX_TRY(selection_verdict(c, sl, info));
    }
    l.last_members = sel.n;
    if (total) *total = rec_u64(l.h_rec, kLnRecTotal);
    return GZPX_OK;
}

}  // namespace

extern "C" {

void gzpx_dlines_destroy(gzpx_dlines *lt) {
    if (!lt) return;
    (void)hipSetDevice(lt->device);
    delete lt;
}

int gzpx_dlines_build_device(gzpx_dctx *c, const gzpx_dindex *ix, const void *d_in, size_t in_len, unsigned delim,
                             gzpx_dlines **out, uint64_t *n_delims, uint64_t *n_lines, gzpx_check_info *info, void *hip_stream) {
    if (!c || !ix || !out || (!d_in && in_len)) return GZPX_ERR_INVALID_ARG;
    *out = nullptr;
    if (n_delims) *n_delims = 0;
    if (n_lines) *n_lines = 0;
    if (delim > 255u) return GZPX_ERR_INVALID_ARG;
    if (!index_matches(c, ix, in_len)) return GZPX_ERR_INVALID_ARG;
    const uint64_t total = ix->inflated_len;
    const uint64_t tiles = (total + kLnTile - 1u) / kLnTile;
    if (tiles > 0xFFFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    std::unique_lock<std::mutex> lk(c->mu);
    LinesState &l = c->lines;
    l.build_ms[0] = l.build_ms[1] = 0.0f;
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    const int si = free_slot(c, lk, true);  // (stays free: the call returns synchronised under the lock)
    std::unique_ptr<gzpx_dlines> lt(new (std::nothrow) gzpx_dlines());  // (c's device is current: a return frees it)
    if (!lt) return GZPX_ERR_DEVICE;
    lt->device = ix->device;
    lt->format = ix->format;
    lt->n = ix->n;
    lt->consumed = ix->consumed;
    lt->inflated_len = total;
    lt->delim = delim;
    lt->tiles = (uint32_t)tiles;
    uint32_t *d_cnt = nullptr;  // [tiles] the tiles' counters: the build's own
    Allocs tmp;
    hipStream_t stream = c->stream;
    Drain drain{{stream}, 1};  // (a failure: nothing still runs on the arrays when they are freed)
    GZPX_TRY(lt->mem.dev(lt->d_prefix, (size_t)(tiles + 1) * 8));
    GZPX_TRY(lt->mem.dev(lt->d_rec, 64));
    GZPX_TRY(tmp.dev(d_cnt, (size_t)(tiles ? tiles : 1) * 4));
    GZPX_TRY(l.reserve(1));  // (the events)
    Batches b;
    GZPX_TRY(batches_of(c, ix, b));
    GZPX_TRY(order_behind(stream, (hipStream_t)hip_stream, c->ev_dep));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, (size_t)(tiles ? tiles : 1) * 4, stream));
    HIP_TRY(hipMemsetAsync(lt->d_rec, 0, 64, stream));
    GZPX_TRY(batched_pass(
        c, si, ix, b, (const uint8_t *)d_in, 0, l.ev, 2, l.build_ms, info, drain, [&](uint64_t base, uint64_t bytes, bool) -> int {
            HIP_TRY(hipEventRecord(l.ev[1], stream));
            launch_lines_count(c->stage.d, base, bytes, total, delim, d_cnt, lt->d_rec, stream);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(l.ev[2], stream));
            return GZPX_OK;
        }));
    launch_lines_prefix(d_cnt, (uint32_t)tiles, total, lt->d_prefix, lt->d_rec, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(l.h_rec, lt->d_rec, 32, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    lt->n_delims = rec_u64(l.h_rec, kLnRecD);
    lt->n_lines = rec_u64(l.h_rec, kLnRecL);
    if (n_delims) *n_delims = lt->n_delims;
    if (n_lines) *n_lines = lt->n_lines;
    *out = lt.release();
    return GZPX_OK;
}

int gzpx_dlines_prefix(const gzpx_dlines *lt, uint64_t *prefix, size_t max_entries, size_t *n_entries) {
    if (!lt || !n_entries) return GZPX_ERR_INVALID_ARG;
    *n_entries = (size_t)lt->tiles + 1;
    const size_t n_copy = prefix ? (*n_entries < max_entries ? *n_entries : max_entries) : 0;
    if (!n_copy) return GZPX_OK;
    if (hipSetDevice(lt->device) != hipSuccess) return GZPX_ERR_DEVICE;
    HIP_TRY(hipMemcpy(prefix, lt->d_prefix, n_copy * 8, hipMemcpyDeviceToHost));
    return GZPX_OK;
}

int gzpx_line_offsets_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                             const uint64_t *lines, size_t n, uint64_t *offsets, size_t *bad, gzpx_check_info *info,
                             void *hip_stream) {
    if (!c || !ix || !lt || (!lines && n) || (!offsets && n) || (!d_in && in_len)) return GZPX_ERR_INVALID_ARG;
    if (bad) *bad = (size_t)-1;
    if (!lines_match(c, ix, lt, in_len) || n > 0x7FFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    std::unique_lock<std::mutex> lk(c->mu);
    c->lines.stages = 0;
    c->lines.last_members = 0;
    if (n == 0) return GZPX_OK;
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    const int si = free_slot(c, lk, true);  // (stays free: the call returns synchronised under the lock)
    GZPX_TRY(lines_search(c, si, ix, lt, (const uint8_t *)d_in, lines, n, 1u, bad, info, (hipStream_t)hip_stream, nullptr));
    memcpy(offsets, c->lines.h_bpos, n * 8);
    return GZPX_OK;
}

}  // extern "C"

namespace {

// gzpx_read_lines_device, and with `on_device` gzpx_read_lines_table_device: line_ranges, out_offsets and byte_ranges
// are then device arrays, and the two that are written are filled by device-to-device copies on the context's stream.
int read_lines(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
               const gzpx_range *line_ranges, bool on_device, size_t n_ranges, void *d_out, size_t out_cap, size_t *out_len,
               uint64_t *out_offsets, gzpx_range *byte_ranges, size_t *bad_range, gzpx_check_info *info, void *hip_stream) {
    static_assert(sizeof(gzpx_range) == 16, "the kernels read and write (begin, end) pairs");
    if (!c || !ix || !lt || !out_len || (!line_ranges && n_ranges) || (!d_in && in_len) || (!d_out && out_cap))
        return GZPX_ERR_INVALID_ARG;
    *out_len = 0;
    if (bad_range) *bad_range = (size_t)-1;
    if (!lines_match(c, ix, lt, in_len) || n_ranges > 0x7FFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    std::unique_lock<std::mutex> lk(c->mu);
    c->lines.stages = 0;
    c->lines.last_members = 0;
    if (n_ranges == 0) {
        if (out_offsets && !on_device) out_offsets[0] = 0;
        if (out_offsets && on_device) {
            if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
            HIP_TRY(hipMemset(out_offsets, 0, 8));
        }
        return GZPX_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    const int si = free_slot(c, lk, true);  // (stays free: the call returns synchronised under the lock)
    uint64_t total = 0;
    GZPX_TRY(lines_search(c, si, ix, lt, (const uint8_t *)d_in, (const uint64_t *)line_ranges, n_ranges, 2u, bad_range, info,
                          (hipStream_t)hip_stream, &total, on_device));
    hipStream_t stream = c->stream;
    Drain drain{{stream}, 1, on_device && byte_ranges};  // (armed while a copy to the caller's device arrays may run)
    if (byte_ranges && !on_device) memcpy(byte_ranges, c->lines.h_bpos, n_ranges * 16);
    if (byte_ranges && on_device)
        HIP_TRY(hipMemcpyAsync(byte_ranges, c->lines.ln.bpos, n_ranges * 16, hipMemcpyDeviceToDevice, stream));
    if (total > out_cap) {
        *out_len = (size_t)total;
        return GZPX_ERR_INSUFFICIENT_SPACE;
    }
    if (total >> 44) return GZPX_ERR_INVALID_ARG;  // (the gather's grid)
    drain.armed = true;
    if (out_offsets && !on_device) memcpy(out_offsets, c->ranges.h_out_off, (n_ranges + 1) * 8);
    if (out_offsets && on_device)
        HIP_TRY(hipMemcpyAsync(out_offsets, c->ranges.rr.out_off, (n_ranges + 1) * 8, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipEventRecord(c->lines.ev[5], stream));
    launch_ranges_gather(c->stage.d, (uint32_t)n_ranges, c->ranges.rr, (uint8_t *)d_out, total, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->lines.ev[6], stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    c->lines.stages = 4;
    *out_len = (size_t)total;
    return GZPX_OK;
}

}  // namespace

extern "C" {

int gzpx_read_lines_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                           const gzpx_range *line_ranges, size_t n_ranges, void *d_out, size_t out_cap, size_t *out_len,
                           uint64_t *out_offsets, gzpx_range *byte_ranges, size_t *bad_range, gzpx_check_info *info,
                           void *hip_stream) {
    return read_lines(c, ix, lt, d_in, in_len, line_ranges, false, n_ranges, d_out, out_cap, out_len, out_offsets, byte_ranges,
                      bad_range, info, hip_stream);
}

int gzpx_read_lines_table_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                                 const gzpx_range *d_line_ranges, size_t n_ranges, void *d_out, size_t out_cap, size_t *out_len,
                                 uint64_t *d_out_offsets, gzpx_range *d_byte_ranges, size_t *bad_range, gzpx_check_info *info,
                                 void *hip_stream) {
    return read_lines(c, ix, lt, d_in, in_len, d_line_ranges, true, n_ranges, d_out, out_cap, out_len, d_out_offsets,
                      d_byte_ranges, bad_range, info, hip_stream);
}

}  // extern "C"

// ---------------------------------------------------------------- fields of lines (gzpx_fields.h)
namespace {

// The field list and the flags as the kernels take them: the field numbers at which membership in S changes, ascending
// (ranges that touch are one), field 0 outside S, UINT64_MAX behind them.  False: the list breaks a rule of gzpx.h.
bool fields_compile(const gzpx_range *fields, size_t n_fields, unsigned flags, FlSet &s) {
    static_assert(kFlMaxRanges == GZPX_FIELDS_MAX_RANGES, "the public constant states the kernels' limit");
    if (!fields || n_fields == 0 || n_fields > kFlMaxRanges || (flags & ~GZPX_FIELDS_COMPLEMENT)) return false;
    size_t n = 0;
    for (size_t i = 0; i < n_fields; i++) {
        const uint64_t b = fields[i].begin, e = fields[i].end;
        if (b >= e || (i && fields[i - 1].end > b) || (e == GZPX_FIELDS_TO_END && i + 1 != n_fields)) return false;
        if (n && s.b[n - 1] == b) n--;
        else s.b[n++] = b;
        if (e != GZPX_FIELDS_TO_END) s.b[n++] = e;
    }
    if (flags & GZPX_FIELDS_COMPLEMENT) {
        if (n && s.b[0] == 0) {
            for (size_t i = 1; i < n; i++) s.b[i - 1] = s.b[i];
            n--;
        } else {
            for (size_t i = n; i > 0; i--) s.b[i] = s.b[i - 1];
            s.b[0] = 0;
            n++;
        }
    }
    s.n = n;
    for (size_t i = n; i < kFlBounds; i++) s.b[i] = UINT64_MAX;
    return true;
}

// gzpx_read_fields_device, and with `on_device` gzpx_read_fields_table_device: line_ranges and out_offsets are then
// device arrays.  The line search of read_lines, then the three passes of gzpx_fields.h in place of the gather, enqueued
// together: whether the output fits is decided on the device, and one record comes back behind the last of them.
int read_fields(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                const gzpx_range *line_ranges, bool on_device, size_t n_ranges, unsigned field_delim, const gzpx_range *fields,
                size_t n_fields, unsigned flags, void *d_out, size_t out_cap, size_t *out_len, uint64_t *out_offsets,
                size_t *bad_range, gzpx_check_info *info, void *hip_stream) {
    if (!c || !ix || !lt || !out_len || (!line_ranges && n_ranges) || (!d_in && in_len) || (!d_out && out_cap))
        return GZPX_ERR_INVALID_ARG;
    *out_len = 0;
    if (bad_range) *bad_range = (size_t)-1;
    std::unique_lock<std::mutex> lk(c->mu);
    FieldsState &f = c->fields;
    c->lines.stages = 0;
    c->lines.last_members = 0;
    f.have = f.wrote = false;
    if (!lines_match(c, ix, lt, in_len) || n_ranges > 0x7FFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    if (field_delim > 255u || field_delim == lt->delim) return GZPX_ERR_INVALID_ARG;
    FlSet set;
    if (!fields_compile(fields, n_fields, flags, set)) return GZPX_ERR_INVALID_ARG;
    if (n_ranges == 0) {
        if (out_offsets && !on_device) out_offsets[0] = 0;
        if (out_offsets && on_device) {
            if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
            HIP_TRY(hipMemset(out_offsets, 0, 8));
        }
        return GZPX_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    const int si = free_slot(c, lk, true);  // (stays free: the call returns synchronised under the lock)
    uint64_t bytes = 0;  // of the ranges, in staging
    GZPX_TRY(lines_search(c, si, ix, lt, (const uint8_t *)d_in, (const uint64_t *)line_ranges, n_ranges, 2u, bad_range, info,
                          (hipStream_t)hip_stream, &bytes, on_device));
    const uint64_t grid = fields_pieces(bytes, n_ranges);
    if (grid > 0x7FFFFFF0ull) return GZPX_ERR_INVALID_ARG;  // (the passes' grid)
    GZPX_TRY(f.reserve(n_ranges, (size_t)grid, !on_device));
    hipStream_t stream = c->stream;
    Drain drain{{stream}, 1};
    const RangeScratch &rr = c->ranges.rr;
    uint64_t *d_off = on_device && out_offsets ? out_offsets : f.fl.out_off;
    *f.h_set = set;
    HIP_TRY(hipMemcpyAsync(f.fl.set, f.h_set, sizeof(FlSet), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(f.ev[0], stream));
    launch_fields_carry(c->stage.d, (uint32_t)n_ranges, rr, f.fl, lt->delim, field_delim, (uint32_t)grid, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f.ev[1], stream));
    launch_fields_count(c->stage.d, (uint32_t)n_ranges, rr, f.fl, lt->delim, field_delim, (uint32_t)grid, d_off, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f.ev[2], stream));
    if (d_out) {
        launch_fields_write(c->stage.d, (uint32_t)n_ranges, rr, f.fl, lt->delim, field_delim, (uint32_t)grid, (uint8_t *)d_out,
                            out_cap, stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(f.ev[3], stream));
    }
    HIP_TRY(hipMemcpyAsync(f.h_rec, f.fl.rec, kFlRecWords * 8, hipMemcpyDeviceToHost, stream));
    if (out_offsets && !on_device) HIP_TRY(hipMemcpyAsync(f.h_out_off, d_off, (n_ranges + 1) * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    f.have = true;
    const uint64_t total = f.h_rec[kFlRecTotal];
    f.wrote = d_out && total <= out_cap;
    *out_len = (size_t)total;
    if (out_offsets && !on_device) memcpy(out_offsets, f.h_out_off, (n_ranges + 1) * 8);
    return d_out && total > out_cap ? GZPX_ERR_INSUFFICIENT_SPACE : GZPX_OK;
}

}  // namespace

extern "C" {

int gzpx_read_fields_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                            const gzpx_range *line_ranges, size_t n_ranges, unsigned field_delim, const gzpx_range *fields,
                            size_t n_fields, unsigned flags, void *d_out, size_t out_cap, size_t *out_len, uint64_t *out_offsets,
                            size_t *bad_range, gzpx_check_info *info, void *hip_stream) {
    return read_fields(c, ix, lt, d_in, in_len, line_ranges, false, n_ranges, field_delim, fields, n_fields, flags, d_out, out_cap,
                       out_len, out_offsets, bad_range, info, hip_stream);
}

int gzpx_read_fields_table_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                                  const gzpx_range *d_line_ranges, size_t n_ranges, unsigned field_delim, const gzpx_range *fields,
                                  size_t n_fields, unsigned flags, void *d_out, size_t out_cap, size_t *out_len,
                                  uint64_t *d_out_offsets, size_t *bad_range, gzpx_check_info *info, void *hip_stream) {
    return read_fields(c, ix, lt, d_in, in_len, d_line_ranges, true, n_ranges, field_delim, fields, n_fields, flags, d_out, out_cap,
                       out_len, d_out_offsets, bad_range, info, hip_stream);
}

int gzpx_dctx_last_fields_ms(gzpx_dctx *ctx, float ms[3]) {
    if (!ctx || !ms) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    ms[0] = ms[1] = ms[2] = 0.0f;
    const FieldsState &f = ctx->fields;
    if (!f.have) return GZPX_OK;
    if (hipEventElapsedTime(&ms[0], f.ev[0], f.ev[1]) != hipSuccess || hipEventElapsedTime(&ms[1], f.ev[1], f.ev[2]) != hipSuccess)
        return GZPX_ERR_DEVICE;
    if (f.wrote && hipEventElapsedTime(&ms[2], f.ev[2], f.ev[3]) != hipSuccess) return GZPX_ERR_DEVICE;
    return GZPX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- numeric columns of lines (gzpx_columns.h)
namespace {

// the column list as the kernels take it; false: it breaks a rule of gzpx.h
bool columns_compile(const gzpx_column *cols, size_t n_cols, ClCols &s) {
    static_assert(kClMaxCols == GZPX_COLUMNS_MAX && kClMaxBytes == GZPX_CELL_MAX_BYTES, "the public constants state the kernels' limits");
    if (!cols || n_cols == 0 || n_cols > kClMaxCols) return false;
    for (size_t i = 0; i < kClMaxCols; i++) {
        s.field[i] = UINT64_MAX;
        s.type[i] = 0;
    }
    for (size_t i = 0; i < n_cols; i++) {
        if ((i && cols[i - 1].field >= cols[i].field) || cols[i].reserved) return false;
        if (cols[i].type != GZPX_COL_INT64 && cols[i].type != GZPX_COL_FLOAT64) return false;
        s.field[i] = cols[i].field;
        s.type[i] = cols[i].type;
    }
    s.n = (uint32_t)n_cols;
    s.pad = 0;
    return true;
}

// gzpx_read_columns_device, and with `on_device` gzpx_read_columns_table_device: line_ranges and row_offsets are then
// device arrays.  The line search of read_lines, then the carries of gzpx_fields.h, the rows and the parse of
// gzpx_columns.h, enqueued together: whether the rows fit is decided on the device, and one record comes back.
int read_columns(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                 const gzpx_range *line_ranges, bool on_device, size_t n_ranges, unsigned field_delim, const gzpx_column *cols,
                 size_t n_cols, void *d_values, uint8_t *d_status, size_t rows_cap, uint64_t *n_rows, uint64_t *n_not_ok,
                 uint64_t *d_col_not_ok, uint64_t *row_offsets, size_t *bad_range, gzpx_check_info *info, void *hip_stream) {
    if (!c || !ix || !lt || !n_rows || (!line_ranges && n_ranges) || (!d_in && in_len)) return GZPX_ERR_INVALID_ARG;
    *n_rows = 0;
    if (n_not_ok) *n_not_ok = 0;
    if (bad_range) *bad_range = (size_t)-1;
    std::unique_lock<std::mutex> lk(c->mu);
    ColumnsState &f = c->columns;
    c->lines.stages = 0;
    c->lines.last_members = 0;
    f.have = false;
    if (!lines_match(c, ix, lt, in_len) || n_ranges > 0x7FFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    if (field_delim > 255u || field_delim == lt->delim || ((uintptr_t)d_values & 7u)) return GZPX_ERR_INVALID_ARG;
    ClCols list;
    if (!columns_compile(cols, n_cols, list)) return GZPX_ERR_INVALID_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    if (n_ranges == 0) {
        if (row_offsets && !on_device) row_offsets[0] = 0;
        if ((row_offsets && on_device) || d_col_not_ok) {  // (device arrays: behind the caller's stream, as every other call)
            hipStream_t stream = c->stream;
            GZPX_TRY(order_behind(stream, (hipStream_t)hip_stream, c->ev_dep));
            Drain drain{{stream}, 1};
            if (row_offsets && on_device) HIP_TRY(hipMemsetAsync(row_offsets, 0, 8, stream));
            if (d_col_not_ok) HIP_TRY(hipMemsetAsync(d_col_not_ok, 0, n_cols * 8, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            drain.armed = false;
        }
        return GZPX_OK;
    }
    const int si = free_slot(c, lk, true);  // (stays free: the call returns synchronised under the lock)
    uint64_t bytes = 0;  // of the ranges, in staging
    GZPX_TRY(lines_search(c, si, ix, lt, (const uint8_t *)d_in, (const uint64_t *)line_ranges, n_ranges, 2u, bad_range, info,
                          (hipStream_t)hip_stream, &bytes, on_device));
    const uint64_t grid = fields_pieces(bytes, n_ranges);
    if (grid > 0x7FFFFFF0ull) return GZPX_ERR_INVALID_ARG;  // (the passes' grid)
    GZPX_TRY(f.reserve(n_ranges, (size_t)grid, !on_device));
    hipStream_t stream = c->stream;
    Drain drain{{stream}, 1};
    const RangeScratch &rr = c->ranges.rr;
    uint64_t *d_off = on_device && row_offsets ? row_offsets : f.cl.row_off;
    const bool stores = d_values || d_status;
    *f.h_cols = list;
    HIP_TRY(hipMemcpyAsync(f.cl.cols, f.h_cols, sizeof(ClCols), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(f.ev[0], stream));
    launch_fields_carry(c->stage.d, (uint32_t)n_ranges, rr, f.cl.fl, lt->delim, field_delim, (uint32_t)grid, stream);
    launch_columns_rows(c->stage.d, (uint32_t)n_ranges, rr, c->lines.ln, f.cl, lt->delim, field_delim, (uint32_t)grid, d_off, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f.ev[1], stream));
    launch_columns_parse(c->stage.d, (uint32_t)n_ranges, rr, f.cl, lt->delim, field_delim, (uint32_t)grid, d_off, (uint64_t *)d_values,
                         d_status, stores ? rows_cap : 0, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f.ev[2], stream));
    HIP_TRY(hipMemcpyAsync(f.h_rec, f.cl.rec, kClRecWords * 8, hipMemcpyDeviceToHost, stream));
    if (d_col_not_ok) HIP_TRY(hipMemcpyAsync(d_col_not_ok, f.cl.rec + kClRecCol, n_cols * 8, hipMemcpyDeviceToDevice, stream));
    if (row_offsets && !on_device) HIP_TRY(hipMemcpyAsync(f.h_row_off, d_off, (n_ranges + 1) * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    f.have = true;
    *n_rows = f.h_rec[kClRecRows];
    if (n_not_ok) *n_not_ok = f.h_rec[kClRecNotOk];
    if (row_offsets && !on_device) memcpy(row_offsets, f.h_row_off, (n_ranges + 1) * 8);
    return stores && f.h_rec[kClRecRows] > rows_cap ? GZPX_ERR_INSUFFICIENT_SPACE : GZPX_OK;
}

}  // namespace

extern "C" {

int gzpx_read_columns_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                             const gzpx_range *line_ranges, size_t n_ranges, unsigned field_delim, const gzpx_column *cols,
                             size_t n_cols, void *d_values, uint8_t *d_status, size_t rows_cap, uint64_t *n_rows, uint64_t *n_not_ok,
                             uint64_t *d_col_not_ok, uint64_t *row_offsets, size_t *bad_range, gzpx_check_info *info,
                             void *hip_stream) {
    return read_columns(c, ix, lt, d_in, in_len, line_ranges, false, n_ranges, field_delim, cols, n_cols, d_values, d_status, rows_cap,
                        n_rows, n_not_ok, d_col_not_ok, row_offsets, bad_range, info, hip_stream);
}

int gzpx_read_columns_table_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                                   const gzpx_range *d_line_ranges, size_t n_ranges, unsigned field_delim, const gzpx_column *cols,
                                   size_t n_cols, void *d_values, uint8_t *d_status, size_t rows_cap, uint64_t *n_rows,
                                   uint64_t *n_not_ok, uint64_t *d_col_not_ok, uint64_t *d_row_offsets, size_t *bad_range,
                                   gzpx_check_info *info, void *hip_stream) {
    return read_columns(c, ix, lt, d_in, in_len, d_line_ranges, true, n_ranges, field_delim, cols, n_cols, d_values, d_status,
                        rows_cap, n_rows, n_not_ok, d_col_not_ok, d_row_offsets, bad_range, info, hip_stream);
}

int gzpx_dctx_last_columns_ms(gzpx_dctx *ctx, float ms[2]) {
    if (!ctx || !ms) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    ms[0] = ms[1] = 0.0f;
    const ColumnsState &f = ctx->columns;
    if (!f.have) return GZPX_OK;
    if (hipEventElapsedTime(&ms[0], f.ev[0], f.ev[1]) != hipSuccess || hipEventElapsedTime(&ms[1], f.ev[1], f.ev[2]) != hipSuccess)
        return GZPX_ERR_DEVICE;
    return GZPX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- selection of lines by their numbers (gzpx_where.h)
namespace {

// The terms as the kernels take them: the distinct fields as a column list, the terms grouped by column, and the pool of
// the TEXT terms' constants as the caller gave it.  `with_text` false (gzpx_where_lines_device): a TEXT term and the two
// prefix ops break the rules like any unknown code.  *has_text: a term is on a TEXT column.  False: they break a rule of
// gzpx.h.
bool where_compile(const gzpx_where_term *terms, size_t n_terms, unsigned flags, const void *text, size_t text_len, bool with_text,
                   ClCols &list, WhTextTerms &tt, bool *has_text) {
    static_assert(kWhMaxTerms == GZPX_WHERE_MAX_TERMS && kWhLt == GZPX_WHERE_LT && kWhLe == GZPX_WHERE_LE && kWhEq == GZPX_WHERE_EQ &&
                      kWhNe == GZPX_WHERE_NE && kWhGe == GZPX_WHERE_GE && kWhGt == GZPX_WHERE_GT && kWhIsOk == GZPX_WHERE_IS_OK &&
                      kWhNotOk == GZPX_WHERE_NOT_OK && kWhPrefix == GZPX_WHERE_PREFIX && kWhNotPrefix == GZPX_WHERE_NOT_PREFIX &&
                      kClText == GZPX_COL_TEXT && kWhTextMax == GZPX_WHERE_TEXT_MAX && kWhPoolMax == GZPX_WHERE_TEXT_POOL_MAX &&
                      GZPX_WHERE_TEXT_MAX == GZPX_CELL_MAX_BYTES,
                  "the public constants state the kernels' limits and codes");
    WhTerms &t = tt.t;
    *has_text = false;
    if (!terms || n_terms == 0 || n_terms > kWhMaxTerms || (flags & ~(GZPX_WHERE_ANY | GZPX_WHERE_INVERT))) return false;
    if (text_len > kWhPoolMax || (!text && text_len) || (!with_text && text_len)) return false;
    for (size_t i = 0; i < kClMaxCols; i++) {
        list.field[i] = UINT64_MAX;
        list.type[i] = 0;
    }
    memset(&tt, 0, offsetof(WhTextTerms, pool));
    uint32_t n = 0;  // distinct fields so far
    for (size_t i = 0; i < n_terms; i++) {
        const gzpx_where_term &m = terms[i];
        const bool is_text = with_text && m.type == GZPX_COL_TEXT;
        if (m.type != GZPX_COL_INT64 && m.type != GZPX_COL_FLOAT64 && !is_text) return false;
        if (m.op > (is_text ? GZPX_WHERE_NOT_PREFIX : GZPX_WHERE_NOT_OK)) return false;  // (the prefix ops: on TEXT alone)
        const bool status_op = m.op == GZPX_WHERE_IS_OK || m.op == GZPX_WHERE_NOT_OK;
        if (status_op && m.value) return false;
        if (is_text && !status_op) {  // the constant text[offset, offset + len)
            const uint64_t off = m.value & 0xFFFFFFFFull, len = m.value >> 32;
            if (len > kWhTextMax || off + len > text_len) return false;
        }
        if (is_text) *has_text = true;
        if (!status_op && m.type == GZPX_COL_FLOAT64 && (m.value & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return false;  // a NaN
        if (i && terms[i - 1].field > m.field) return false;
        if (i && terms[i - 1].field == m.field) {
            if (terms[i - 1].type != m.type) return false;
        } else {
            if (n == kClMaxCols) return false;
            list.field[n] = m.field;
            list.type[n] = m.type;
            t.first[n++] = (uint32_t)i;
        }
        t.value[i] = m.value;
        t.op[i] = m.op;
    }
    for (uint32_t c = n; c <= kClMaxCols; c++) t.first[c] = (uint32_t)n_terms;
    t.any = (flags & GZPX_WHERE_ANY) ? 1u : 0u;
    tt.pool_len = *has_text ? (uint32_t)text_len : 0u;
    if (tt.pool_len) memcpy(tt.pool, text, text_len);
    list.n = n;
    list.pad = 0;
    return true;
}

// gzpx_where_lines_device and gzpx_where_text_device (`with_text`: TEXT terms and their pool of constants are allowed),
// and with `on_device` their table forms: line_ranges is then a device array.  The
// line search of read_lines, then the carries of gzpx_fields.h, the rows of gzpx_columns.h, the parse with the predicate
// and the runs of gzpx_where.h, enqueued together; one record comes back.  The bitmaps are sized by a bound on the rows
// that the host knows: the rows themselves in the host form, the ranges' bytes in the table form.
int where_lines(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                const gzpx_range *line_ranges, bool on_device, size_t n_ranges, unsigned field_delim, const gzpx_where_term *terms,
                size_t n_terms, unsigned flags, const void *text, size_t text_len, bool with_text, gzpx_range *d_runs, size_t runs_cap,
                uint64_t *n_runs, uint64_t *n_selected, uint64_t *n_rows, uint64_t *n_not_ok, size_t *bad_range, gzpx_check_info *info,
                void *hip_stream) {
    if (!c || !ix || !lt || !n_runs || !n_selected || !n_rows || (!line_ranges && n_ranges) || (!d_in && in_len))
        return GZPX_ERR_INVALID_ARG;
    *n_runs = *n_selected = *n_rows = 0;
    if (n_not_ok) *n_not_ok = 0;
    if (bad_range) *bad_range = (size_t)-1;
    std::unique_lock<std::mutex> lk(c->mu);
    WhereState &f = c->where;
    c->lines.stages = 0;
    c->lines.last_members = 0;
    f.have = false;
    if (!lines_match(c, ix, lt, in_len) || n_ranges > 0x7FFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    if (field_delim > 255u || field_delim == lt->delim || ((uintptr_t)d_runs & 7u)) return GZPX_ERR_INVALID_ARG;
    ClCols list;
    WhTextTerms compiled;
    bool has_text;
    if (!where_compile(terms, n_terms, flags, text, text_len, with_text, list, compiled, &has_text)) return GZPX_ERR_INVALID_ARG;
    if (n_ranges == 0) return GZPX_OK;
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    const int si = free_slot(c, lk, true);  // (stays free: the call returns synchronised under the lock)
    uint64_t bytes = 0;  // of the ranges, in staging
    GZPX_TRY(lines_search(c, si, ix, lt, (const uint8_t *)d_in, (const uint64_t *)line_ranges, n_ranges, 2u, bad_range, info,
                          (hipStream_t)hip_stream, &bytes, on_device));
    // every line of a range holds at least one byte of it: R <= bytes
    uint64_t bound = bytes;
    if (!on_device) {
        bound = 0;
        for (size_t r = 0; r < n_ranges; r++) bound += line_ranges[r].end - line_ranges[r].begin;  // (valid: the search said so)
    }
    if (bound > 0xFFFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    if (bound == 0) return GZPX_OK;  // every range is empty
    const uint64_t grid = fields_pieces(bytes, n_ranges), bits = where_bits(bound);
    if (grid > 0x7FFFFFF0ull) return GZPX_ERR_INVALID_ARG;  // (the passes' grid)
    GZPX_TRY(f.reserve(n_ranges, (size_t)grid, bits));
    f.wh.starts = f.wh.bitmap + bits / 32u;
    hipStream_t stream = c->stream;
    Drain drain{{stream}, 1};
    const RangeScratch &rr = c->ranges.rr;
    const ColumnsScratch &cl = f.wh.cl;
    const uint64_t cap = d_runs ? runs_cap : 0;
    const int invert = ((flags & GZPX_WHERE_ANY) ? 0 : 1) ^ ((flags & GZPX_WHERE_INVERT) ? 1 : 0);  // without ANY the bits say "rejected"
    *f.h_cols = list;
    // (the terms, and with TEXT terms the pool's bytes in use behind them)
    const size_t terms_bytes = has_text ? offsetof(WhTextTerms, pool) + ((compiled.pool_len + 3u) & ~(size_t)3u) : sizeof(WhTerms);
    memcpy(f.h_terms, &compiled, offsetof(WhTextTerms, pool) + compiled.pool_len);
    HIP_TRY(hipMemcpyAsync(cl.cols, f.h_cols, sizeof(ClCols), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(f.wh.terms, f.h_terms, terms_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(f.ev[0], stream));
    launch_fields_carry(c->stage.d, (uint32_t)n_ranges, rr, cl.fl, lt->delim, field_delim, (uint32_t)grid, stream);
    launch_columns_rows(c->stage.d, (uint32_t)n_ranges, rr, c->lines.ln, cl, lt->delim, field_delim, (uint32_t)grid, cl.row_off, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f.ev[1], stream));
    launch_where_parse(c->stage.d, (uint32_t)n_ranges, rr, f.wh, lt->delim, field_delim, (uint32_t)grid, cl.row_off, bits, has_text, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f.ev[2], stream));
    launch_where_runs((uint32_t)n_ranges, c->lines.ln, f.wh, cl.row_off, bits, invert, (uint64_t *)d_runs, cap, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f.ev[3], stream));
    HIP_TRY(hipMemcpyAsync(f.h_rec, f.wh.rec, kWhRecWords * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    f.have = true;
    *n_runs = f.h_rec[kWhRecRuns];
    *n_selected = f.h_rec[kWhRecSelected];
    *n_rows = f.h_rec[kWhRecRows];
    if (n_not_ok) *n_not_ok = f.h_rec[kWhRecNotOk];
    if (*n_rows > bits) return GZPX_ERR_INVALID_ARG;  // (the table and the stream do not belong together: nothing was marked)
    return d_runs && *n_runs > cap ? GZPX_ERR_INSUFFICIENT_SPACE : GZPX_OK;
}

}  // namespace

extern "C" {

int gzpx_where_lines_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                            const gzpx_range *line_ranges, size_t n_ranges, unsigned field_delim, const gzpx_where_term *terms,
                            size_t n_terms, unsigned flags, gzpx_range *d_runs, size_t runs_cap, uint64_t *n_runs,
                            uint64_t *n_selected, uint64_t *n_rows, uint64_t *n_not_ok, size_t *bad_range, gzpx_check_info *info,
                            void *hip_stream) {
    return where_lines(c, ix, lt, d_in, in_len, line_ranges, false, n_ranges, field_delim, terms, n_terms, flags, nullptr, 0, false,
                       d_runs, runs_cap, n_runs, n_selected, n_rows, n_not_ok, bad_range, info, hip_stream);
}

int gzpx_where_lines_table_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                                  const gzpx_range *d_line_ranges, size_t n_ranges, unsigned field_delim,
                                  const gzpx_where_term *terms, size_t n_terms, unsigned flags, gzpx_range *d_runs, size_t runs_cap,
                                  uint64_t *n_runs, uint64_t *n_selected, uint64_t *n_rows, uint64_t *n_not_ok, size_t *bad_range,
                                  gzpx_check_info *info, void *hip_stream) {
    return where_lines(c, ix, lt, d_in, in_len, d_line_ranges, true, n_ranges, field_delim, terms, n_terms, flags, nullptr, 0, false,
                       d_runs, runs_cap, n_runs, n_selected, n_rows, n_not_ok, bad_range, info, hip_stream);
}

int gzpx_where_text_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                           const gzpx_range *line_ranges, size_t n_ranges, unsigned field_delim, const gzpx_where_term *terms,
                           size_t n_terms, const void *text, size_t text_len, unsigned flags, gzpx_range *d_runs, size_t runs_cap,
                           uint64_t *n_runs, uint64_t *n_selected, uint64_t *n_rows, uint64_t *n_not_ok, size_t *bad_range,
                           gzpx_check_info *info, void *hip_stream) {
    return where_lines(c, ix, lt, d_in, in_len, line_ranges, false, n_ranges, field_delim, terms, n_terms, flags, text, text_len, true,
                       d_runs, runs_cap, n_runs, n_selected, n_rows, n_not_ok, bad_range, info, hip_stream);
}

int gzpx_where_text_table_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                                 const gzpx_range *d_line_ranges, size_t n_ranges, unsigned field_delim,
                                 const gzpx_where_term *terms, size_t n_terms, const void *text, size_t text_len, unsigned flags,
                                 gzpx_range *d_runs, size_t runs_cap, uint64_t *n_runs, uint64_t *n_selected, uint64_t *n_rows,
                                 uint64_t *n_not_ok, size_t *bad_range, gzpx_check_info *info, void *hip_stream) {
    return where_lines(c, ix, lt, d_in, in_len, d_line_ranges, true, n_ranges, field_delim, terms, n_terms, flags, text, text_len, true,
                       d_runs, runs_cap, n_runs, n_selected, n_rows, n_not_ok, bad_range, info, hip_stream);
}

int gzpx_dctx_last_where_ms(gzpx_dctx *ctx, float ms[3]) {
    if (!ctx || !ms) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    ms[0] = ms[1] = ms[2] = 0.0f;
    const WhereState &f = ctx->where;
    if (!f.have) return GZPX_OK;
    for (int j = 0; j < 3; j++)
        if (hipEventElapsedTime(&ms[j], f.ev[j], f.ev[j + 1]) != hipSuccess) return GZPX_ERR_DEVICE;
    return GZPX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- search and selection, for one pattern or a set of them
// (gzpx_find.h, gzpx_select.h, gzpx_findset.h)
namespace {

// what the entry points check of a set before anything else happens
struct SetShape {
    uint32_t K = 0, longest = 0, shortest = 0;
};

bool findset_shape(const void *patterns, const uint32_t *off, size_t n_patterns, SetShape &sh) {
    static_assert(kFsMaxPatterns == GZPX_FINDSET_MAX_PATTERNS && kFsMaxBytes == GZPX_FINDSET_MAX_BYTES,
                  "the public constants state the kernels' limits");
    if (!patterns || !off || n_patterns == 0 || n_patterns > kFsMaxPatterns) return false;
    sh.K = (uint32_t)n_patterns;
    sh.shortest = kFdMaxPattern;
    for (size_t k = 0; k < n_patterns; k++) {
        if (off[k + 1] <= off[k] || off[k + 1] - off[k] > kFdMaxPattern) return false;  // (empty, too long, or decreasing)
        const uint32_t m = off[k + 1] - off[k];
        if (m > sh.longest) sh.longest = m;
        if (m < sh.shortest) sh.shortest = m;
    }
    return off[n_patterns] - off[0] <= kFsMaxBytes;
}

// The set in the form the kernels stage into LDS; returns the bytes of it that are in use (bytes is the last table).
size_t findset_compile(const uint8_t *patterns, const uint32_t *off, const SetShape &sh, FsSet *h) {
    const uint32_t K = sh.K, q = sh.shortest < 4u ? sh.shortest : 4u;
    uint32_t window[kFsMaxPatterns], order[kFsMaxPatterns];
    memset(h->hdr, 0, sizeof(h->hdr));
    const uint32_t bitmap_words = q == 1u ? 8u : kFsBitmapWords;
    memset(h->bitmap, 0, bitmap_words * 4u);
    uint32_t words = 0;
    for (uint32_t k = 0; k < K; k++) {
        const uint8_t *p = patterns + off[k];
        const uint32_t m = off[k + 1] - off[k];
        window[k] = 0;
        for (uint32_t j = 0; j < q; j++) window[k] |= (uint32_t)p[j] << (8u * j);
        const uint32_t bit = fs_gram_index(window[k], q);
        h->bitmap[bit >> 5] |= 1u << (bit & 31u);
        h->meta[k] = (words << 16) | m;
        h->bytes[words + (m - 1u) / 4u] = 0;  // (the tail of the last dword)
        memcpy(&h->bytes[words], p, m);
        words += (m + 3u) / 4u;
        order[k] = k;
    }
    // buckets: the ids sorted by window, ascending inside one window
    std::stable_sort(order, order + K, [&](uint32_t x, uint32_t y) { return window[x] < window[y]; });
    uint32_t grams = 0;
    for (uint32_t j = 0; j < K; j++) {
        if (j == 0 || window[order[j]] != window[order[j - 1]]) {
            h->keys[grams] = window[order[j]];
            h->bstart[grams++] = j;
        }
        h->ids[j] = order[j];
    }
    h->bstart[grams] = K;
    while (words % 4u) h->bytes[words++] = 0;  // (staged as 16-byte words)
    h->hdr[kFsHdrK] = K;
    h->hdr[kFsHdrQ] = q;
    h->hdr[kFsHdrM] = sh.longest;
    h->hdr[kFsHdrGrams] = grams;
    h->hdr[kFsHdrBitmapWords] = bitmap_words;
    h->hdr[kFsHdrByteWords] = words;
    return offsetof(FsSet, bytes) + (size_t)words * 4u;
}

// What a call searches for: one pattern (off null; sh.K = 1, sh.longest = sh.shortest = its length) or a set.
struct Wanted {
    const void *bytes;    // the pattern, or the set's patterns back to back
    const uint32_t *off;  // the set's offsets into them
    SetShape sh;
};

// What a batch of a search does.
struct SearchBatch {
    FindBatch fb;
    bool search;     // the region is not empty and is either new or the last word on its starts
    uint32_t carry;  // bytes to keep for the next batch (0: none, or the carry stays as it is)
};

// One pattern of m bytes.  Hits are owned by their LAST byte: a batch searches its bytes with the last min(m - 1, bytes
// in front of it) bytes of the earlier batches in front of them, and keeps the last min(m - 1, bytes seen) bytes for the
// next batch (a batch shorter than that appends to the carry).
SearchBatch batch_by_last_byte(uint8_t *stage, uint64_t base, uint64_t bytes, bool is_last, uint32_t m, int delim) {
    const uint64_t seen = base + bytes;
    SearchBatch s;
    s.fb = FindBatch{stage, base, bytes, (uint32_t)(base < m - 1u ? base : m - 1u), m, delim};
    s.search = bytes != 0;
    s.carry = bytes && !is_last ? (uint32_t)(seen < m - 1u ? seen : m - 1u) : 0u;
    return s;
}

// A set whose longest pattern has M bytes.  Hits are owned by their START: a batch that is not the last owns the starts
// p of its region with p + M <= the region's end, the last min(M - 1, bytes seen) bytes wait in the carry, and the last
// batch owns every start that is left -- also when it holds no byte itself.
SearchBatch batch_by_start(uint8_t *stage, uint64_t base, uint64_t bytes, bool is_last, uint32_t M, int delim) {
    const uint32_t waiting = (uint32_t)(base < M - 1u ? base : M - 1u);
    const uint64_t seen = base + bytes;
    SearchBatch s;
    s.fb = FindBatch{stage, base, bytes, waiting, is_last ? 1u : M, delim};
    s.search = bytes || (is_last && waiting);
    s.carry = bytes && !is_last ? (uint32_t)(seen < M - 1u ? seen : M - 1u) : 0u;
    return s;
}

SearchBatch search_batch(const Wanted &w, uint8_t *stage, uint64_t base, uint64_t bytes, bool is_last, int delim) {
    return w.off ? batch_by_start(stage, base, bytes, is_last, w.sh.longest, delim)
                 : batch_by_last_byte(stage, base, bytes, is_last, w.sh.longest, delim);
}

// the search's scratch for the batches of b (and the events both kinds of search time with)
int search_reserve(gzpx_dctx *c, const Wanted &w, const Batches &b) {
    GZPX_TRY(c->find.reserve((size_t)find_pieces(b.max_bytes)));
    return w.off ? c->find_set.reserve() : GZPX_OK;
}

// In front of the first batch: the pattern or the compiled set, and cleared records, on their way to the device.
// `mt`: what the launchers take for it.
int search_begin(gzpx_dctx *c, const Wanted &w, FindMatcher &mt) {
    FindState &f = c->find;
    FindSetState &fs = c->find_set;
    mt = FindMatcher{};
    HIP_TRY(hipMemsetAsync(f.fd.rec, 0, kFdRecWords * 8, c->stream));
    if (!w.off) {
        memset(f.h_pat, 0, kFdMaxPattern);
        memcpy(f.h_pat, w.bytes, w.sh.longest);
        HIP_TRY(hipMemcpyAsync(f.fd.pat, f.h_pat, kFdMaxPattern, hipMemcpyHostToDevice, c->stream));
        return GZPX_OK;
    }
    const size_t used = findset_compile((const uint8_t *)w.bytes, w.off, w.sh, fs.h_set);
    HIP_TRY(hipMemcpyAsync(fs.d_set, fs.h_set, used, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(fs.d_counts, 0, kFsMaxPatterns * 8, c->stream));
    mt = FindMatcher{fs.d_set, fs.d_counts};
    return GZPX_OK;
}

// gzpx_find_device and gzpx_find_set_device behind their argument checks.  `ms`: the kind's own three sums.
int search_hits(gzpx_dctx *c, const gzpx_dindex *ix, const void *d_in, const Wanted &w, int delim, uint64_t *d_positions,
                uint32_t *d_ids, uint64_t *d_lines, size_t hits_cap, uint64_t *d_counts, float *ms, uint64_t *n_hits,
                gzpx_check_info *info, void *hip_stream) {
    const bool writes = d_positions || d_ids || d_lines;
    const uint64_t cap = writes ? hits_cap : 0;
    std::unique_lock<std::mutex> lk(c->mu);
    FindState &f = c->find;
    ms[0] = ms[1] = ms[2] = 0.0f;
    hipStream_t stream = c->stream;
    if (!ix->n || w.sh.shortest > ix->inflated_len) {  // no position can hold a pattern: nothing is inflated, every count is zero
        if (!d_counts) return GZPX_OK;
        if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
        GZPX_TRY(order_behind(stream, (hipStream_t)hip_stream, c->ev_dep));
        Drain drain{{stream}, 1};
        HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)w.sh.K * 8, stream));
        return GZPX_OK;  // (the drain synchronises)
    }
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    const int si = free_slot(c, lk, true);  // (stays free: the call returns synchronised under the lock)
    Drain drain{{stream}, 1};
    Batches b;
    GZPX_TRY(batches_of(c, ix, b));
    GZPX_TRY(search_reserve(c, w, b));
    GZPX_TRY(order_behind(stream, (hipStream_t)hip_stream, c->ev_dep));
    FindMatcher mt;
    GZPX_TRY(search_begin(c, w, mt));
    GZPX_TRY(batched_pass(
        c, si, ix, b, (const uint8_t *)d_in, kFdPad /* the inflate writes behind the pad */, f.ev, 3, ms, info, drain,
        [&](uint64_t base, uint64_t bytes, bool is_last) -> int {
            const SearchBatch sb = search_batch(w, c->stage.d, base, bytes, is_last, d_lines ? delim : GZPX_FIND_NO_LINES);
            HIP_TRY(hipEventRecord(f.ev[1], stream));
            if (sb.search) launch_find_count(sb.fb, f.fd, mt, stream);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(f.ev[2], stream));
            if (sb.search && cap) launch_find_write(sb.fb, f.fd, mt, d_positions, d_ids, d_lines, cap, stream);
            if (sb.carry) launch_find_carry(sb.fb, f.fd, sb.carry, stream);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(f.ev[3], stream));
            return GZPX_OK;
        }));
    HIP_TRY(hipMemcpyAsync(f.h_rec, f.fd.rec, kFdRecWords * 8, hipMemcpyDeviceToHost, stream));
    if (d_counts) HIP_TRY(hipMemcpyAsync(d_counts, mt.d_counts, (size_t)w.sh.K * 8, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    *n_hits = f.h_rec[kFdRecHits];
    return writes && *n_hits > cap ? GZPX_ERR_INSUFFICIENT_SPACE : GZPX_OK;
}

// gzpx_select_lines_device and gzpx_select_lines_set_device behind their argument checks.
int select_lines(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, const Wanted &w, uint64_t group,
                 unsigned flags, gzpx_range *d_runs, size_t runs_cap, uint64_t *n_runs, uint64_t *n_records, uint64_t *n_hits,
                 gzpx_check_info *info, void *hip_stream) {
    const uint64_t L = lt->n_lines;
    const uint64_t R = L / group + (L % group ? 1u : 0u);
    if (R > 0xFFFFFFF0ull) return GZPX_ERR_INVALID_ARG;
    const int invert = (flags & GZPX_SELECT_INVERT) ? 1 : 0;
    const uint64_t cap = d_runs ? runs_cap : 0;
    std::unique_lock<std::mutex> lk(c->mu);
    SelectState &s = c->select;
    FindState &f = c->find;
    s.ms[0] = s.ms[1] = s.ms[2] = 0.0f;
    if (L == 0) return GZPX_OK;
    if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
    hipStream_t stream = c->stream;
    if (w.sh.shortest > ix->inflated_len) {  // no position can hold a pattern: nothing is inflated, and every record is one run under INVERT
        if (!invert) return GZPX_OK;
        *n_runs = 1;
        *n_records = R;
        if (!d_runs) return GZPX_OK;
        if (!cap) return GZPX_ERR_INSUFFICIENT_SPACE;
        GZPX_TRY(s.reserve(1));
        GZPX_TRY(order_behind(stream, (hipStream_t)hip_stream, c->ev_dep));
        Drain drain{{stream}, 1};
        s.h_run[0] = 0;
        s.h_run[1] = L;
        HIP_TRY(hipMemcpyAsync(d_runs, s.h_run, 16, hipMemcpyHostToDevice, stream));
        return GZPX_OK;  // (the drain synchronises)
    }
    const int si = free_slot(c, lk, true);  // (stays free: the call returns synchronised under the lock)
    Drain drain{{stream}, 1};
    Batches b;
    GZPX_TRY(batches_of(c, ix, b));
    GZPX_TRY(search_reserve(c, w, b));
    GZPX_TRY(s.reserve(R));
    GZPX_TRY(order_behind(stream, (hipStream_t)hip_stream, c->ev_dep));
    FindMatcher mt;
    GZPX_TRY(search_begin(c, w, mt));
    HIP_TRY(hipMemsetAsync(s.sl.bitmap, 0, (size_t)((R + 31) / 32 * 4), stream));
    GZPX_TRY(batched_pass(
        c, si, ix, b, (const uint8_t *)d_in, kFdPad /* the inflate writes behind the pad */, s.ev, 2, s.ms, info, drain,
        [&](uint64_t base, uint64_t bytes, bool is_last) -> int {
            const SearchBatch sb = search_batch(w, c->stage.d, base, bytes, is_last, (int)lt->delim);
            HIP_TRY(hipEventRecord(s.ev[1], stream));
            if (sb.search) {
                launch_find_count(sb.fb, f.fd, mt, stream);
                launch_select_mark(sb.fb, f.fd, mt, s.sl, group, R, stream);
            }
            if (sb.carry) launch_find_carry(sb.fb, f.fd, sb.carry, stream);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(s.ev[2], stream));
            return GZPX_OK;
        }));
    HIP_TRY(hipEventRecord(s.ev[3], stream));
    launch_select_runs(s.sl, f.fd, R, group, L, invert, (uint64_t *)d_runs, cap, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.ev[4], stream));
    HIP_TRY(hipMemcpyAsync(s.h_rec, s.sl.rec, kSlRecWords * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    if (hipEventElapsedTime(&s.ms[2], s.ev[3], s.ev[4]) != hipSuccess) s.ms[2] = 0.0f;
    *n_runs = s.h_rec[kSlRecRuns];
    *n_records = s.h_rec[kSlRecRecords];
    if (n_hits) *n_hits = s.h_rec[kSlRecHits];
    return d_runs && *n_runs > cap ? GZPX_ERR_INSUFFICIENT_SPACE : GZPX_OK;
}

// the three sums of the last call of one kind
template <class State>
int last_ms(gzpx_dctx *ctx, State gzpx_dctx::*kind, float ms[3]) {
    if (!ctx || !ms) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    for (int j = 0; j < 3; j++) ms[j] = (ctx->*kind).ms[j];
    return GZPX_OK;
}

}  // namespace

extern "C" {

int gzpx_find_device(gzpx_dctx *c, const gzpx_dindex *ix, const void *d_in, size_t in_len, const void *pattern,
                     size_t pattern_len, int delim, uint64_t *d_positions, uint64_t *d_lines, size_t hits_cap, uint64_t *n_hits,
                     gzpx_check_info *info, void *hip_stream) {
    static_assert(kFdMaxPattern == GZPX_FIND_MAX_PATTERN, "the public constant states the kernels' limit");
    if (!c || !ix || !n_hits || !pattern || (!d_in && in_len)) return GZPX_ERR_INVALID_ARG;
    *n_hits = 0;
    if (pattern_len == 0 || pattern_len > kFdMaxPattern || delim < GZPX_FIND_NO_LINES || delim > 255) return GZPX_ERR_INVALID_ARG;
    if (d_lines && delim == GZPX_FIND_NO_LINES) return GZPX_ERR_INVALID_ARG;
    if (!index_matches(c, ix, in_len)) return GZPX_ERR_INVALID_ARG;
    const uint32_t m = (uint32_t)pattern_len;
    return search_hits(c, ix, d_in, Wanted{pattern, nullptr, SetShape{1u, m, m}}, delim, d_positions, nullptr, d_lines, hits_cap, nullptr,
                       c->find.ms, n_hits, info, hip_stream);
}

int gzpx_find_set_device(gzpx_dctx *c, const gzpx_dindex *ix, const void *d_in, size_t in_len, const void *patterns,
                         const uint32_t *pattern_offsets, size_t n_patterns, int delim, uint64_t *d_positions, uint32_t *d_ids,
                         uint64_t *d_lines, size_t hits_cap, uint64_t *d_counts, uint64_t *n_hits, gzpx_check_info *info,
                         void *hip_stream) {
    if (!c || !ix || !n_hits || (!d_in && in_len)) return GZPX_ERR_INVALID_ARG;
    *n_hits = 0;
    SetShape sh;
    if (!findset_shape(patterns, pattern_offsets, n_patterns, sh)) return GZPX_ERR_INVALID_ARG;
    if (delim < GZPX_FIND_NO_LINES || delim > 255 || (d_lines && delim == GZPX_FIND_NO_LINES)) return GZPX_ERR_INVALID_ARG;
    if (!index_matches(c, ix, in_len)) return GZPX_ERR_INVALID_ARG;
    return search_hits(c, ix, d_in, Wanted{patterns, pattern_offsets, sh}, delim, d_positions, d_ids, d_lines, hits_cap, d_counts,
                       c->find_set.ms, n_hits, info, hip_stream);
}

int gzpx_select_lines_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                             const void *pattern, size_t pattern_len, uint64_t group, unsigned flags, gzpx_range *d_runs,
                             size_t runs_cap, uint64_t *n_runs, uint64_t *n_records, uint64_t *n_hits, gzpx_check_info *info,
                             void *hip_stream) {
    if (!c || !ix || !lt || !n_runs || !n_records || !pattern || (!d_in && in_len)) return GZPX_ERR_INVALID_ARG;
    *n_runs = *n_records = 0;
    if (n_hits) *n_hits = 0;
    if (group == 0 || (flags & ~GZPX_SELECT_INVERT) || pattern_len == 0 || pattern_len > kFdMaxPattern) return GZPX_ERR_INVALID_ARG;
    if (!lines_match(c, ix, lt, in_len)) return GZPX_ERR_INVALID_ARG;
    const uint32_t m = (uint32_t)pattern_len;
    return select_lines(c, ix, lt, d_in, Wanted{pattern, nullptr, SetShape{1u, m, m}}, group, flags, d_runs, runs_cap, n_runs,
                        n_records, n_hits, info, hip_stream);
}

int gzpx_select_lines_set_device(gzpx_dctx *c, const gzpx_dindex *ix, const gzpx_dlines *lt, const void *d_in, size_t in_len,
                                 const void *patterns, const uint32_t *pattern_offsets, size_t n_patterns, uint64_t group,
                                 unsigned flags, gzpx_range *d_runs, size_t runs_cap, uint64_t *n_runs, uint64_t *n_records,
                                 uint64_t *n_hits, gzpx_check_info *info, void *hip_stream) {
    if (!c || !ix || !lt || !n_runs || !n_records || (!d_in && in_len)) return GZPX_ERR_INVALID_ARG;
    *n_runs = *n_records = 0;
    if (n_hits) *n_hits = 0;
    SetShape sh;
    if (group == 0 || (flags & ~GZPX_SELECT_INVERT) || !findset_shape(patterns, pattern_offsets, n_patterns, sh))
        return GZPX_ERR_INVALID_ARG;
    if (!lines_match(c, ix, lt, in_len)) return GZPX_ERR_INVALID_ARG;
    return select_lines(c, ix, lt, d_in, Wanted{patterns, pattern_offsets, sh}, group, flags, d_runs, runs_cap, n_runs, n_records,
                        n_hits, info, hip_stream);
}

int gzpx_dctx_last_find_ms(gzpx_dctx *ctx, float ms[3]) { return last_ms(ctx, &gzpx_dctx::find, ms); }
int gzpx_dctx_last_find_set_ms(gzpx_dctx *ctx, float ms[3]) { return last_ms(ctx, &gzpx_dctx::find_set, ms); }
int gzpx_dctx_last_select_ms(gzpx_dctx *ctx, float ms[3]) { return last_ms(ctx, &gzpx_dctx::select, ms); }

int gzpx_dctx_set_lines_batch(gzpx_dctx *ctx, size_t inflated_bytes) {
    if (!ctx) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->lines.batch = inflated_bytes;
    return GZPX_OK;
}

int gzpx_dctx_last_lines_members(gzpx_dctx *ctx, size_t *n_members_read) {
    if (!ctx || !n_members_read) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    *n_members_read = ctx->lines.last_members;
    return GZPX_OK;
}

int gzpx_dctx_last_lines_ms(gzpx_dctx *ctx, float ms[4]) {
    if (!ctx || !ms) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    ms[0] = ms[1] = ms[2] = ms[3] = 0.0f;
    const Event *ev = ctx->lines.ev;
    const int have = ctx->lines.stages;
    if (have >= 1 && hipEventElapsedTime(&ms[0], ev[0], ev[1]) != hipSuccess) return GZPX_ERR_DEVICE;
    if (have >= 3 && (hipEventElapsedTime(&ms[1], ev[2], ev[3]) != hipSuccess || hipEventElapsedTime(&ms[2], ev[3], ev[4]) != hipSuccess))
        return GZPX_ERR_DEVICE;
    if (have >= 4 && hipEventElapsedTime(&ms[3], ev[5], ev[6]) != hipSuccess) return GZPX_ERR_DEVICE;
    return GZPX_OK;
}

int gzpx_dctx_last_lines_build_ms(gzpx_dctx *ctx, float ms[2]) {
    if (!ctx || !ms) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    ms[0] = ctx->lines.build_ms[0];
    ms[1] = ctx->lines.build_ms[1];
    return GZPX_OK;
}

int gzpx_decompress_blocks(gzpx_dctx *c, const uint8_t *in, size_t in_len, const uint64_t *offsets,
                           const uint32_t *sizes, size_t n_blocks, uint8_t *out, size_t out_cap,
                           size_t *out_len, gzpx_check_info *info) {
    if (!c || (!in && in_len) || (!out && out_cap) || !out_len) return GZPX_ERR_INVALID_ARG;
    *out_len = 0;
    if (n_blocks == 0) return GZPX_OK;
    uint64_t ticket = 0;
    int rc;
    {
        std::unique_lock<std::mutex> lk(c->mu);
        if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
        uint8_t dummy = 0;
        rc = dsubmit_enqueue(c, in, nullptr, in_len, offsets, sizes, n_blocks, out ? out : &dummy, nullptr, out_cap,
                             nullptr, true, lk, &ticket);
    }
    if (rc != GZPX_OK) return rc;
    return dwait_ticket(c, ticket, out_len, info);
}

struct gzpx_decompressor {
    gzpx_dctx *ctx;
    std::vector<uint8_t> framed;
};

gzpx_decompressor *gzpx_alloc_decompressor(void) {
    gzpx_decompressor *d = new (std::nothrow) gzpx_decompressor();
    if (d) d->ctx = nullptr;
    return d;
}

int gzpx_deflate_decompress(gzpx_decompressor *d, const void *in, size_t n, void *out, size_t cap, size_t *actual) {
    if (!d || (!in && n) || (!out && cap)) return GZPX_ERR_INVALID_ARG;
    if (cap > 0xFFFFFFFFull || n > 0xFFFFFFFFull - 64) return GZPX_ERR_UNSUPPORTED;  // one member: 32-bit sizes
    if (!d->ctx) {
        const int rc = gzpx_dctx_create(0, GZPX_FORMAT_MGZIP, &d->ctx);
        if (rc != GZPX_OK) return rc;
    }
    // the kernels work on framed members: wrap the raw stream with a header and a footer whose
    // ISIZE is the caller's capacity (libdeflate semantics: at most `cap` bytes may come out).  With
    // cap == 0 one byte of room is offered, so that a stream with output is told apart from an
    // empty one (libdeflate: INSUFFICIENT_SPACE).
    const size_t room = cap ? cap : 1;
    d->framed.assign(20 + n + 8, 0);
    memcpy(d->framed.data() + 20, in, n);
    uint8_t *f = d->framed.data() + 20 + n;
    const uint32_t isz = (uint32_t)room;
    f[4] = (uint8_t)isz;
    f[5] = (uint8_t)(isz >> 8);
    f[6] = (uint8_t)(isz >> 16);
    f[7] = (uint8_t)(isz >> 24);
    const uint64_t off = 0;
    const uint32_t size = (uint32_t)d->framed.size();
    std::vector<uint8_t> tmp(room);
    gzpx_dctx *c = d->ctx;
    uint64_t ticket = 0;
    int rc;
    size_t got = 0;
    {
        std::unique_lock<std::mutex> lk(c->mu);
        if (hipSetDevice(c->device) != hipSuccess) return GZPX_ERR_DEVICE;
        rc = dsubmit_enqueue(c, d->framed.data(), nullptr, d->framed.size(), &off, &size, 1, tmp.data(), nullptr, room,
                             nullptr, true, lk, &ticket);
    }
    if (rc != GZPX_OK) return rc;
    const DSlot &sl = c->slots[ticket & 0xFF];
    gzpx_check_info info = {0, 0, 0};
    rc = dwait_ticket(c, ticket, nullptr, &info, true);
    if (rc == GZPX_ERR_INVALID_CHECK) rc = GZPX_OK;  // a raw stream carries no checksum
    if (rc != GZPX_OK) return rc;
    {
        std::lock_guard<std::mutex> lk(c->mu);  // (this handle is single-threaded like libdeflate's: the
        got = sl.h_summary[kDsProduced0];       //  slot has not been reused since the wait)
    }
    if (got > cap) return GZPX_ERR_INSUFFICIENT_SPACE;  // cap == 0 and the stream has output
    if (got) memcpy(out, tmp.data(), got);
    if (actual) *actual = got;
    return GZPX_OK;
}

void gzpx_free_decompressor(gzpx_decompressor *d) {
    if (!d) return;
    if (d->ctx) gzpx_dctx_destroy(d->ctx);
    delete d;
}

}  // extern "C"

// ---------------------------------------------------------------- measurement / debug hooks
extern "C" {

int gzpx_ctx_set_profiling(gzpx_ctx *ctx, int on) {
    if (!ctx) return GZPX_ERR_INVALID_ARG;
    ctx->profiling = on == 2 ? 2 : on != 0 ? 1 : 0;
    return GZPX_OK;
}

int gzpx_ctx_last_stage_ms(const gzpx_ctx *ctx, float ms[GZPX_N_STAGES]) {
    if (!ctx || !ms) return GZPX_ERR_INVALID_ARG;
    for (int i = 0; i < GZPX_N_STAGES; i++) ms[i] = ctx->stage_ms[i];
    return GZPX_OK;
}

const char *gzpx_stage_name(int stage) {
    switch (stage) {
    case kStInitMeta: return "k_init_meta";
    case kStCandidates: return "k_candidates";
    case kStMatch: return "k_match";
    case kStParse: return "k_parse";
    case kStHist: return "k_hist";
    case kStHuffman: return "k_huffman";
    case kStCrc32: return "k_crc32";
    case kStScan: return "k_scan";
    case kStEmit: return "k_emit";
    default: return "?";
    }
}

const char *gzpx_ctx_stage_kernel(const gzpx_ctx *ctx, int stage) {
    if (ctx && ctx->cfg.format == GZPX_FORMAT_SNAP)  // (the CRC-32C is computed inside k_snap_chunk)
        return stage == kStMatch ? "k_snap_chunk" : stage == kStScan ? "k_snap_frame+k_scan" : stage == kStEmit ? "k_snap_emit" : "-";
    // the kernels behind the match and parse stages depend on the level (and, at level 1, on the block size)
    if (ctx && stage == kStMatch) {
        const Config &c = ctx->dcfg;
        if (c.level <= 1) return (c.block_size <= kTile && !(c.debug & 2u)) ? "k_mparse" : "k_match";
        if (c.level >= 10) return "k_near_optimal";
        return c.lazy ? "k_match_hc+k_parse_lazy" : "k_match_hc+k_parse_hc";
    }
    if (ctx && stage == kStParse && ctx->dcfg.level > 1) return "-";
    return gzpx_stage_name(stage);
}

int gzpx_debug_tokens(gzpx_ctx *ctx, size_t block, uint32_t *tokens, size_t max_tokens,
                      size_t *n_tokens, uint32_t *sub_first_token, size_t *n_sub) {
    if (!ctx || !n_tokens || block >= ctx->last_nb || ctx->cfg.format == GZPX_FORMAT_SNAP)
        return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return GZPX_ERR_DEVICE;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(ctx->h_meta, ctx->scratch.meta + block, sizeof(BlockMeta), hipMemcpyDeviceToHost));
    const BlockMeta m = ctx->h_meta[0];
    const uint32_t max_sub = ctx->dcfg.max_sub;
    *n_tokens = m.ntok;
    if (n_sub) *n_sub = m.nsub;
    if (sub_first_token && m.nsub) {
        HIP_TRY(hipMemcpy(ctx->h_sub, ctx->scratch.sub + block * (size_t)max_sub,
                          (size_t)(m.nsub < max_sub ? m.nsub : max_sub) * sizeof(SubMeta), hipMemcpyDeviceToHost));
        for (uint32_t s = 0; s < m.nsub && s < max_sub; s++) sub_first_token[s] = ctx->h_sub[s].tok_begin;
    }
    const size_t ncopy = m.ntok < max_tokens ? m.ntok : max_tokens;
    if (tokens && ncopy)
        HIP_TRY(hipMemcpy(tokens, ctx->scratch.tok + block * (size_t)ctx->dcfg.stride, ncopy * 4,
                          hipMemcpyDeviceToHost));
    return GZPX_OK;
}

int gzpx_debug_snap(gzpx_ctx *ctx, int enable, uint64_t sums[8]) {
    if (!ctx || ctx->cfg.format != GZPX_FORMAT_SNAP) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return GZPX_ERR_DEVICE;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t chunks = (size_t)ctx->batch_blocks * snap_chunks_per_buffer((uint32_t)ctx->cfg.buffer_size);
    SnapScratch &ss = ctx->snap;
    if (sums) {
        for (int k = 0; k < 8; k++) sums[k] = 0;
        const size_t used = (size_t)ctx->last_nb * snap_chunks_per_buffer((uint32_t)ctx->cfg.buffer_size);
        if (ss.dbg && used) {
            std::vector<uint64_t> h(used * 8);
            HIP_TRY(hipMemcpy(h.data(), ss.dbg, h.size() * 8, hipMemcpyDeviceToHost));
            for (size_t c = 0; c < used; c++)
                for (int k = 0; k < 8; k++) sums[k] += h[c * 8 + k];
        }
    }
    if (enable && !ss.dbg) {
        GZPX_TRY(ctx->snap_dbg.dev(ss.dbg, chunks * 8 * sizeof(uint64_t)));
        HIP_TRY(hipMemset(ss.dbg, 0, chunks * 8 * sizeof(uint64_t)));
    } else if (!enable) {
        ctx->snap_dbg.release();
    }
    return GZPX_OK;
}

int gzpx_debug_set_flags(gzpx_ctx *ctx, uint32_t flags) {
    if (!ctx) return GZPX_ERR_INVALID_ARG;
    ctx->dcfg.debug = flags;
    return GZPX_OK;
}

int gzpx_debug_redo_count(gzpx_ctx *ctx, uint32_t *count) {
    if (!ctx || !count || ctx->cfg.format == GZPX_FORMAT_SNAP) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return GZPX_ERR_DEVICE;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(count, ctx->scratch.redo, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return GZPX_OK;
}

void *gzpx_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void gzpx_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

int gzpx_dctx_last_inflate_ms(gzpx_dctx *ctx, float *ms) {
    if (!ctx || !ms) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    *ms = 0.0f;
    if (!ctx->last_nb || ctx->last_slot < 0) return GZPX_OK;
    const DSlot &sl = ctx->slots[ctx->last_slot];
    return hipEventElapsedTime(ms, sl.ev_t0, sl.ev_t1) == hipSuccess ? GZPX_OK : GZPX_ERR_DEVICE;
}

int gzpx_dctx_last_inflate_stage_ms(gzpx_dctx *ctx, float ms[2]) {
    if (!ctx || !ms) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    ms[0] = ms[1] = 0.0f;
    if (!ctx->last_nb || ctx->last_slot < 0 || ctx->slots[ctx->last_slot].route != kInflateRouteSeg) return GZPX_OK;
    const DSlot &sl = ctx->slots[ctx->last_slot];
    if (hipEventElapsedTime(&ms[0], sl.ev_t0, sl.ev_tm) != hipSuccess || hipEventElapsedTime(&ms[1], sl.ev_tm, sl.ev_t1) != hipSuccess)
        return GZPX_ERR_DEVICE;
    return GZPX_OK;
}

int gzpx_dctx_set_route(gzpx_dctx *ctx, int route) {
    if (!ctx || (route != GZPX_INFLATE_SEG && route != GZPX_INFLATE_WAVE)) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->route = route == GZPX_INFLATE_WAVE ? kInflateRouteWave : kInflateRouteSeg;
    return GZPX_OK;
}

int gzpx_dctx_last_redo_count(gzpx_dctx *ctx, uint32_t *count) {
    if (!ctx || !count) return GZPX_ERR_INVALID_ARG;
    *count = 0;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (ctx->last_slot < 0 || !ctx->slots[ctx->last_slot].sc.redo || ctx->slots[ctx->last_slot].route != kInflateRouteSeg)
        return GZPX_OK;
    if (hipSetDevice(ctx->device) != hipSuccess) return GZPX_ERR_DEVICE;
    if (hipMemcpy(count, ctx->slots[ctx->last_slot].sc.redo, 4, hipMemcpyDeviceToHost) != hipSuccess) return GZPX_ERR_DEVICE;
    return GZPX_OK;
}

int gzpx_debug_inflate(gzpx_dctx *ctx, int enable, uint64_t sums[8]) {
    if (!ctx) return GZPX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->debug = enable < 0 ? 0 : enable > 2 ? 1 : enable;
    if (sums) {
        for (int k = 0; k < 8; k++) sums[k] = 0;
        if (ctx->last_slot >= 0 && ctx->slots[ctx->last_slot].have_blk)
            for (size_t b = 0; b < ctx->last_nb; b++)
                for (int k = 0; k < 8; k++) sums[k] += ctx->slots[ctx->last_slot].h_blk[b].cyc[k];
    }
    return GZPX_OK;
}

static_assert(kHbNone == GZPX_HANDBACK_NONE && kHbHeader == GZPX_HANDBACK_HEADER && kHbStored == GZPX_HANDBACK_STORED &&
                  kHbNoEob == GZPX_HANDBACK_NO_EOB && kHbResync == GZPX_HANDBACK_RESYNC && kHbSpanSymbol == GZPX_HANDBACK_SPAN_SYMBOL &&
                  kHbSpanOverrun == GZPX_HANDBACK_SPAN_OVERRUN && kHbDistance == GZPX_HANDBACK_DISTANCE &&
                  kHbOffsetSymbol == GZPX_HANDBACK_OFFSET_SYMBOL && kHbCodeword == GZPX_HANDBACK_CODEWORD &&
                  kHbCountMismatch == GZPX_HANDBACK_COUNT_MISMATCH && kHbFinal == GZPX_HANDBACK_FINAL &&
                  kHbLzcopy == GZPX_HANDBACK_LZCOPY, "the kernels' reasons are the header's");
int gzpx_debug_inflate_handback(gzpx_dctx *ctx, uint32_t *reasons, size_t n) {
    if (!ctx || (n && !reasons)) return GZPX_ERR_INVALID_ARG;
    for (size_t b = 0; b < n; b++) reasons[b] = GZPX_HANDBACK_NONE;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (ctx->last_slot < 0 || !ctx->last_nb) return GZPX_OK;
    const DSlot &sl = ctx->slots[ctx->last_slot];
    if (!sl.debug || !sl.sc.redo || sl.route != kInflateRouteSeg) return GZPX_OK;
    if (hipSetDevice(ctx->device) != hipSuccess) return GZPX_ERR_DEVICE;
    const size_t nb = sl.nb;  // (the launch's own count: it says where the reasons lie)
    if (!nb || nb > sl.cap_blocks) return GZPX_OK;
    std::vector<uint32_t> h(2 + 2 * nb);
    if (hipMemcpy(h.data(), sl.sc.redo, h.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return GZPX_ERR_DEVICE;
    const uint32_t *why = h.data() + 2 + nb;
    for (size_t b = 0; b < n && b < nb; b++) reasons[b] = why[b];
    // k_lzcopy carries no instrumentation under enable 1: a member on the list that k_inflate_seg did not put there is its
    if (sl.debug == 1)
        for (size_t i = 0; i < h[0] && i < nb; i++) {
            const uint32_t b = h[1 + i];
            if (b < n && b < nb && why[b] == kHbNone) reasons[b] = kHbLzcopy;
        }
    return GZPX_OK;
}

const char *gzpx_strerror(int code) {
    switch (code) {
        case GZPX_OK: return "ok";
        case GZPX_ERR_INVALID_ARG: return "invalid argument";
        case GZPX_ERR_BUFFER_SIZE: return "buffer size must be >= 32768 (GzpError::BufferSize)";
        case GZPX_ERR_COMPRESSION_LEVEL: return "invalid compression level (GzpError::LibDeflaterCompressionLvl)";
        case GZPX_ERR_INSUFFICIENT_SPACE: return "insufficient output space (GzpError::LibDeflaterCompress)";
        case GZPX_ERR_BLOCK_SIZE_EXCEEDED: return "compressed block >= 65536 bytes (GzpError::BlockSizeExceeded)";
        case GZPX_ERR_DEVICE: return "HIP runtime error";
        case GZPX_ERR_NO_DEVICE: return "no HIP device (no CPU fallback exists)";
        case GZPX_ERR_UNSUPPORTED: return "configuration valid in gzp but not built yet";
        case GZPX_ERR_NUM_THREADS: return "number of threads must be > 0 (GzpError::NumThreads)";
        case GZPX_ERR_IO: return "the wrapped writer failed (GzpError::Io)";
        case GZPX_ERR_CHANNEL: return "compression pipeline already closed (GzpError::ChannelSend)";
        case GZPX_ERR_INVALID_HEADER: return "invalid block header (GzpError::InvalidHeader)";
        case GZPX_ERR_INVALID_CHECK: return "checksum mismatch (GzpError::InvalidCheck)";
        case GZPX_ERR_BAD_DATA: return "invalid DEFLATE stream (GzpError::LibDelfaterDecompress(BadData))";
        case GZPX_ERR_BUSY: return "every slab slot of the context is in flight: wait for one first";
        default: return "unknown error";
    }
}

const char *gzpx_device_name(const gzpx_ctx *ctx) { return ctx ? ctx->devname : ""; }
const char *gzpx_version(void) { return "gzpx 0.1 (gfx950)"; }
#ifndef GZPX_BUILD_ID
#define GZPX_BUILD_ID "unknown"
#endif
const char *gzpx_build_id(void) { return GZPX_BUILD_ID; }

}  // extern "C"
