// gzpx_wave.h -- what more than one stage or more than one header of gzpx_kernels.hip uses: the measurement switch
// GZPX_EXP and the GZPX_EXPERIMENT counter tables, wave_sync, rdlane / uniform, the pinning macros,
// load_le32_global, the wave and workgroup scans, dword4, length_entry / build_length_table.  It also brings in the
// three headers of shared arithmetic, gzpx_policy.h (libdeflate's parsing rules: lz_hash, where a sub-block ends, which
// matches count), gzpx_deflate.h (with its wave routines, behind wave_sync) and gzpx_crc.h (with its device half,
// behind dword4), so that every stage of gzpx_kernels.hip and every decode header finds all of this in front of it.
//
// Nothing here replaces a routine of the reference: these are the lane-level idioms its scalar loops turn into on a
// 64-lane wave.
//
// Included once by gzpx_kernels.hip inside namespace gzpx, in front of the first kernel.  Needs gzpx_device.h (Config)
// and <hip/hip_runtime.h> alone.

// Measurement-only switches (tools/exp_bounds.py builds a second library with -DGZPX_EXPERIMENT; the
// product build compiles them away): parts of a kernel are skipped -- the results are wrong on purpose
// -- to see which resource bounds it.
#ifdef GZPX_EXPERIMENT
#define GZPX_EXP(cfg, bit) (((cfg).debug >> (bit)) & 1u)
#else
#define GZPX_EXP(cfg, bit) 0u
#endif

// libdeflate's parsing rules: lz_hash, the block-end constants, the split check, the minimum match length
#include "gzpx_policy.h"

// ------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------

// Rendezvous + ordering point for the lanes of ONE wave that communicate through LDS.  LDS
// operations of a wave execute in issue order, so no hardware wait is needed -- only the
// compiler must not move LDS accesses across it.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// a value that is the same in every lane, moved to a scalar register (wave-uniform state that
// comes out of LDS would otherwise occupy a VGPR in every lane)
__device__ __forceinline__ uint32_t rdlane(uint32_t v, uint32_t l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l);
}
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// keep a finished value in a VGPR here (stops the compiler from sinking its computation to the use)
#if defined(__HIP_DEVICE_COMPILE__)
#define GZPX_PIN_VGPR(x) asm volatile("" : "+v"(x))
#else
#define GZPX_PIN_VGPR(x) ((void)0)
#endif

// a value that a load brings is complete here: the compiler's wait for that load goes in front of this statement and,
// the register not being written, in front of no later use (the value itself stays what and where it is)
#if defined(__HIP_DEVICE_COMPILE__)
#define GZPX_HERE_VGPR(x) asm volatile("" ::"v"(x))
#else
#define GZPX_HERE_VGPR(x) ((void)0)
#endif

// last statement of one arm of a branch whose arms end alike: keeps the compiler from sinking the like
// tails into one copy behind the branch (which would turn this arm's immediate offsets into selected addresses)
#if defined(__HIP_DEVICE_COMPILE__)
#define GZPX_KEEP_ARM_APART() asm volatile("")
#else
#define GZPX_KEEP_ARM_APART() ((void)0)
#endif

// little-endian u32 at an arbitrary byte address of global memory via two aligned loads
__device__ __forceinline__ uint32_t load_le32_global(const uint8_t *p) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t *w = (const uint32_t *)(a & ~(uintptr_t)3);
    return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(a & 3));
}

__device__ __forceinline__ uint32_t wave_reduce_add(uint32_t v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, unsigned lane) {
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d);
        if (lane >= (unsigned)d) v += t;
    }
    return v;
}

// wave-wide inclusive scans on the DPP network (row shifts, then the row broadcasts of gfx9)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_zero(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v) {
    v += dpp_zero<0x111, 0xf>(v);
    v += dpp_zero<0x112, 0xf>(v);
    v += dpp_zero<0x114, 0xf>(v);
    v += dpp_zero<0x118, 0xf>(v);
    v += dpp_zero<0x142, 0xa>(v);
    v += dpp_zero<0x143, 0xc>(v);
    return v;
}
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v) {
    v = umax32(v, dpp_zero<0x111, 0xf>(v));
    v = umax32(v, dpp_zero<0x112, 0xf>(v));
    v = umax32(v, dpp_zero<0x114, 0xf>(v));
    v = umax32(v, dpp_zero<0x118, 0xf>(v));
    v = umax32(v, dpp_zero<0x142, 0xa>(v));
    v = umax32(v, dpp_zero<0x143, 0xc>(v));
    return v;
}

// Exclusive scan of one value per thread over a workgroup of NW waves; `wsum` is NW words of LDS.
// Returns the exclusive prefix; *total receives the workgroup sum.  Two barriers.
template <unsigned NW>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wsum, uint32_t *total) {
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t inc = wave_incl_add(v);
    __syncthreads();  // protect wsum from the previous use
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    // the wave totals: one LDS read per lane and a second DPP scan (NW <= 64) instead of NW reads and
    // 2 NW additions in every lane
    const uint32_t mine = lane < NW ? wsum[lane] : 0u;
    const uint32_t winc = wave_incl_add(mine);
    *total = rdlane(winc, NW - 1);
    const uint32_t base = wave ? rdlane(winc, wave - 1) : 0u;
    return base + inc - v;
}

// Exclusive scan of one 64-bit value per thread over a 256-thread workgroup; `wsum` is 4 words of
// LDS.  Returns the exclusive prefix; *total receives the workgroup sum.  Two barriers.  (64-bit:
// 256 Mgzip blocks of 16 MiB, or foreign ISIZE fields, sum to 2^32 and more.)
__device__ __forceinline__ uint64_t block_exclusive_scan256(uint64_t v, uint64_t *wsum, uint64_t *total) {
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(inc, d);
        if (lane >= (unsigned)d) inc += t;
    }
    __syncthreads();  // protect wsum from the previous use
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint64_t base = 0, tot = 0;
    for (unsigned w = 0; w < 4; w++) {
        const uint64_t s = wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}

// RFC 1951's alphabets, the precode order, the fixed code, the dynamic header's fields and the canonical-code steps
#define GZPX_DEFLATE_WAVE
#include "gzpx_deflate.h"

// The two token consumers (k_hist, k_emit) look lengths up in a 256-entry LDS table of length - 3.  k_hist keeps
// slot | extra-bit count << 5 (length_entry); k_emit builds, from the same entries, the codeword and extra bits of
// every length for each sub-block.
__device__ __forceinline__ uint32_t length_entry(uint32_t x) {
    const DeflateSlot s = length_slot(x + 3);
    return s.slot | (s.xbits << 5);
}
__device__ __forceinline__ void build_length_table(uint8_t *lslot, uint32_t tid) {
    if (tid < 256) lslot[tid] = (uint8_t)length_entry(tid);
}

// four dwords that are only dword-aligned in global memory (the hardware takes such 16-byte loads)
struct __attribute__((aligned(4))) dword4 {
    uint32_t x, y, z, w;
};

// CRC-32 / CRC-32C: the one product, the power table, the slice-by-4 steps (crc_seg256 loads dword4)
#define GZPX_CRC_KERNELS
#include "gzpx_crc.h"

#ifdef GZPX_EXPERIMENT
// k_huffman: setup, litlen code, offset code, precode RLE, precode code, costs, header + tables (rows as below)
__device__ unsigned long long g_exp_huff[1024 * 8];
// k_mparse: stage, first walk, later rounds, settle, build, barrier rounds, re-walks (x 1024 rows, a
// block adds to row blockIdx & 1023: same-address atomics serialise at the L2)
__device__ unsigned long long g_exp_cycles[1024 * 8];
// k_match_hc_sparse: window, first nodes, walks, lists, searches (cycles); rounds, listed searches, tiles (counts)
__device__ unsigned long long g_exp_sparse[1024 * 8];
#endif
