// Reads stay inside the slab: the product kernels on the CPU emulator under AddressSanitizer, with the input in a heap
// buffer of exactly the slab's length (under the emulator a device pointer is a host pointer), so that a load behind
// the slab's last byte is a heap-buffer-overflow.  BGZF at levels 1 and 3 (k_candidates modes 0-3), with the interior
// body, with Config.debug bit 7 (every iteration clamped) and with bit 0 (the fallback); lengths that end a block at
// each residue of its last iteration, n mod 1024 in {0, 1, 15, 16, 17, 1023}, for a slab of one block and of three.
// A stand-alone program, CPU only; from the repository root:
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Wno-unknown-pragmas -Wno-unused-function -I tests/emu -I include \
//       -x c++ gzp_amd/csrc/gzpx_kernels.hip gzp_amd/csrc/gzpx_nearopt.hip gzp_amd/csrc/gzpx_synth.hip \
//       gzp_amd/csrc/gzpx_api.cpp gzp_amd/csrc/gzpx_par.cpp tests/emu/emu_runtime.cpp tools/asan_cand_reads.cpp \
//       -o /tmp/asan_cand_reads && /tmp/asan_cand_reads
//
// The kernels load aligned dwords, and the dword that holds a slab's last byte is read whole (cand_fetch's clamp, the
// CRC kernel): with `--round-up` the buffer is the slab's length rounded up to a dword, which allows exactly that and
// nothing behind it.  Prints one line per run and "clean" at the end; AddressSanitizer ends the program at the first
// bad access.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gzpx.h"

static uint32_t rng_state = 20250927u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

int main(int argc, char **argv) {
    const bool round_up = argc > 1 && !strcmp(argv[1], "--round-up");
    const size_t kBlock = 65280;
    const size_t tails[] = {0, 1, 15, 16, 17, 1023};
    const uint32_t flags[] = {0u, 128u, 1u};
    const char *words[] = {"the ", "candidate ", "table ", "of ", "a ", "block ", "turn ", "wave ", "and ", "lane "};
    int runs = 0;
    for (int level : {1, 3}) {
        for (size_t blocks : {(size_t)1, (size_t)3}) {
            for (size_t tail : tails) {
                // the last block: seven iterations and `tail` bytes
                const size_t last = 7 * 1024 + tail, n = (blocks - 1) * kBlock + last;
                uint8_t *in = (uint8_t *)malloc(round_up ? (n + 3) & ~(size_t)3 : n);
                for (size_t i = 0; i < n;) {
                    const char *w = words[rnd() % 10];
                    for (; *w && i < n; w++) in[i++] = (uint8_t)*w;
                }
                for (uint32_t f : flags) {
                    gzpx_config cfg;
                    gzpx_config_default(&cfg, GZPX_FORMAT_BGZF);
                    cfg.level = level;
                    cfg.compat = GZPX_COMPAT_LIBDEFLATE_1_24;
                    cfg.buffer_size = kBlock;
                    cfg.max_slab_bytes = n;
                    gzpx_ctx *ctx = nullptr;
                    int rc = gzpx_ctx_create(&cfg, &ctx);
                    if (rc) return fprintf(stderr, "gzpx_ctx_create: %s\n", gzpx_strerror(rc)), 1;
                    if ((rc = gzpx_debug_set_flags(ctx, f))) return fprintf(stderr, "flags: %s\n", gzpx_strerror(rc)), 1;
                    const size_t cap = gzpx_slab_bound(ctx, n);
                    std::vector<uint8_t> out(cap);
                    size_t out_len = 0, nb = 0;
                    rc = gzpx_compress_slab_device(ctx, in, n, GZPX_SLAB_LAST, out.data(), cap, &out_len, nullptr, 0, &nb, nullptr);
                    if (rc) return fprintf(stderr, "compress: %s\n", gzpx_strerror(rc)), 1;
                    printf("level %d  slab %zu, last block %zu (mod 1024 = %zu)  debug %u  -> %zu bytes, %zu blocks\n", level, n, last,
                           last % 1024, f, out_len, nb);
                    gzpx_ctx_destroy(ctx);
                    runs++;
                }
                free(in);
            }
        }
    }
    printf("clean: %d runs, no read outside the input buffer (%s)\n", runs, round_up ? "length rounded up to a dword" : "exact length");
    return 0;
}
