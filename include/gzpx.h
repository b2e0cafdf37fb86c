/*
 * gzpx.h -- C ABI of the MI355X-native per-block encoder behind gzp's ParCompress<Bgzf/Mgzip>.
 *
 * This is the drop-in boundary: the entry points are what gzp's FFI for this path binds today
 * (libdeflater -> libdeflate-sys), plus one slab-level call that lets the orchestration layer
 * hand thousands of blocks to the GPU at once.  Plain pointers and sizes only.
 *
 * Reference interfaces replaced (paths relative to the gzp tree, v2.0.1):
 *
 *   gzpx_alloc_compressor      libdeflater::Compressor::new            src/deflate.rs:596-599 (Bgzf::create_compressor)
 *                              = libdeflate_alloc_compressor            /opt/conda/include/libdeflate.h:62-69
 *   gzpx_deflate_compress      Compressor::deflate_compress            src/bgzf.rs:214-216, src/mgzip.rs:201-203
 *                              = libdeflate_deflate_compress            libdeflate.h:88-91
 *   gzpx_deflate_compress_bound  Compressor::deflate_compress_bound    libdeflate.h:93-95
 *   gzpx_free_compressor       Drop for Compressor                     libdeflate.h:117
 *   gzpx_crc32                 libdeflater::Crc::update / sum          src/bgzf.rs:224-225, src/check.rs:62,70
 *                              = libdeflate_crc32                       libdeflate.h:343-344
 *   gzpx_encode_block          FormatSpec::encode for Bgzf / Mgzip     src/lib.rs:351-358, src/deflate.rs:613-626, 463-472
 *                              (= bgzf::compress src/bgzf.rs:204-237 + BGZF_EOF src/bgzf.rs:24-38)
 *                              FormatSpec::encode for Snap              src/snap.rs:61-74 (FrameEncoder over the buffer)
 *   gzpx_compress_slab*        the worker loop of ParCompress::run     src/par/compress.rs:279-294, applied to every
 *                              block of a slab cut by ParCompress::write / flush_last (src/par/compress.rs:413-463, 332-362)
 *   error codes                GzpError variants on this path          src/lib.rs:114-163
 *
 * Results are byte-identical to the reference's libdeflate path at the same level (see
 * DESIGN.md for the one libdeflate-version-dependent rule selected by `compat`).
 */
#ifndef GZPX_H
#define GZPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (GzpError classes reachable on the path, src/lib.rs:114-163) ---- */
#define GZPX_OK 0
#define GZPX_ERR_INVALID_ARG 1         /* null pointer, non-multiple slab, ...                       */
#define GZPX_ERR_BUFFER_SIZE 2         /* GzpError::BufferSize: buffer_size < DICT_SIZE (32768)       */
#define GZPX_ERR_COMPRESSION_LEVEL 3   /* GzpError::LibDeflaterCompressionLvl                         */
#define GZPX_ERR_INSUFFICIENT_SPACE 4  /* GzpError::LibDeflaterCompress(InsufficientSpace)            */
#define GZPX_ERR_BLOCK_SIZE_EXCEEDED 5 /* GzpError::BlockSizeExceeded(c, 65536), src/bgzf.rs:218-223  */
#define GZPX_ERR_DEVICE 6              /* HIP runtime error (the Io-like class)                       */
#define GZPX_ERR_NO_DEVICE 7           /* no MI355X / HIP device: there is NO CPU fallback            */
#define GZPX_ERR_UNSUPPORTED 8         /* valid in the reference, not built yet (blocks > 64 MiB) */
#define GZPX_ERR_NUM_THREADS 9         /* GzpError::NumThreads(0), src/par/compress.rs:84-90          */
#define GZPX_ERR_IO 10                 /* GzpError::Io: the wrapped writer failed                     */
#define GZPX_ERR_CHANNEL 11            /* GzpError::ChannelSend/Receive: pipeline already closed      */
#define GZPX_ERR_INVALID_HEADER 12     /* GzpError::InvalidHeader (src/deflate.rs:555-565, 405-415)    */
#define GZPX_ERR_INVALID_CHECK 13      /* GzpError::InvalidCheck{found, expected}                      */
#define GZPX_ERR_BAD_DATA 14           /* GzpError::LibDelfaterDecompress(BadData)                     */
#define GZPX_ERR_BUSY 15               /* submit: every slab slot of the context is in flight          */

/* how a slab is cut (the `mode` argument of gzpx_compress_slab*) */
#define GZPX_SLAB_FULL_BLOCKS 0 /* write(): only whole buffer_size blocks, in_len a non-zero multiple   */
#define GZPX_SLAB_LAST 1        /* flush_last(true): final piece may be short/empty; BGZF EOF appended  */
#define GZPX_SLAB_FLUSH 2       /* flush_last(false): final piece may be short/empty; no EOF marker     */

#define GZPX_FORMAT_BGZF 0
#define GZPX_FORMAT_MGZIP 1
/* Snap (src/snap.rs:38-83): every buffer_size piece is snap::read::FrameEncoder's frame stream of that piece alone --
 * the stream identifier, then per 64 KiB chunk a header, the masked CRC-32C of the chunk and its raw Snappy encoding
 * (or the chunk itself where that is not shorter than n - n/8); an empty piece encodes to nothing.  gzp ignores the
 * level for Snap (src/snap.rs:53-59, 91): level and compat are accepted whatever they are.  Snap has no end-of-stream
 * marker, so GZPX_SLAB_LAST and GZPX_SLAB_FLUSH produce the same bytes.  Compression only: gzp has no
 * ParDecompress<Snap> (gzpx_dctx_create refuses it), and the multi-device entry points and gzpx_par_index refuse it
 * too.  Raw chunk bodies are snappy 1.1.8's (DESIGN.md "Snap"). */
#define GZPX_FORMAT_SNAP 2

/* libdeflate behaviour pinned by Cargo.lock is 1.24; the image's binary oracle is 1.10.  The two
 * differ (for levels 1-4) only in how a Huffman code with no used symbol is emitted and in
 * min_len for scans shorter than 512 bytes; levels 5-9 are pinned against 1.10 only (no 1.24 binary or
 * source here to compare the lazy parsers with), with the same two rules applied. */
#define GZPX_COMPAT_LIBDEFLATE_1_24 0
#define GZPX_COMPAT_LIBDEFLATE_1_10 1

typedef struct gzpx_config {
    int device;                /* HIP device ordinal                                              */
    int format;                /* GZPX_FORMAT_*                                                   */
    int level;                 /* flate2::Compression level, 0..12 as libdeflate accepts (src/deflate.rs:596-599); 10..12: the near-optimal
                                * parser as in libdeflate 1.10 -- later versions changed it, so at these levels `compat` is
                                * ignored, the 1.10 rules apply throughout (gzpx_ctx_active_compat) and the stream equals the
                                * 1.10 binary's, not 1.24's */
    int compat;                /* GZPX_COMPAT_*                                                   */
    size_t buffer_size;        /* ParCompressBuilder::buffer_size (65280 default for BGZF)        */
    size_t max_slab_bytes;     /* largest slab a single gzpx_compress_slab* call will be given    */
} gzpx_config;

typedef struct gzpx_ctx gzpx_ctx;

/* Fills *cfg with the reference's defaults for `format` (Bgzf: buffer_size 65280, Mgzip / Snap 131072, level 3 ->
 * callers set the level they use; compat 1.24; device 0; max_slab_bytes 1 GiB). */
void gzpx_config_default(gzpx_config *cfg, int format);

/* Validates like ParCompressBuilder (src/par/compress.rs:68-74) + CompressionLvl::new and
 * allocates device scratch.  Fails with GZPX_ERR_NO_DEVICE when no GPU is present. */
int gzpx_ctx_create(const gzpx_config *cfg, gzpx_ctx **out);
void gzpx_ctx_destroy(gzpx_ctx *ctx);

/* The GZPX_COMPAT_* rules this context really runs: cfg->compat at levels 0-9; at levels 10-12 always
 * GZPX_COMPAT_LIBDEFLATE_1_10 -- the near-optimal parser built here is libdeflate 1.10's (the one binary there is to
 * pin it on), so its stream is the 1.10 binary's bit for bit and never a mix of two versions' rules. */
int gzpx_ctx_active_compat(const gzpx_ctx *ctx);

/* Upper bound of the bytes gzpx_compress_slab* can produce for in_len input bytes. */
size_t gzpx_slab_bound(const gzpx_ctx *ctx, size_t in_len);

/*
 * Compress one slab held in HOST memory.  The slab is cut into buffer_size blocks exactly as
 * ParCompress::write does; `mode` is one of GZPX_SLAB_*: with FULL_BLOCKS, in_len must be a
 * non-zero multiple of buffer_size (the caller keeps the remainder, as write() does); with LAST
 * or FLUSH the final piece may be short or empty (flush_last), and LAST appends the BGZF EOF
 * marker after it.
 * out receives the framed blocks back to back; block_sizes[i] (optional) the framed size of
 * block i.  On GZPX_ERR_BLOCK_SIZE_EXCEEDED, *n_blocks holds the index of the failing block.
 */
int gzpx_compress_slab(gzpx_ctx *ctx, const uint8_t *in, size_t in_len, int mode, uint8_t *out,
                       size_t out_cap, size_t *out_len, uint32_t *block_sizes, size_t max_blocks,
                       size_t *n_blocks);

/* For the hip_stream / after_stream arguments below: "the caller has already synchronized -- no dependency":
 * nothing is recorded on any stream (NULL, the legacy default stream, waits behind ALL blocking streams of the
 * device and may not be recorded on while a stream capture is running). */
#define GZPX_STREAM_NONE ((void *)(intptr_t)-1)

/* Same, with the slab and the output already resident in DEVICE memory (d_in, d_out are device
 * pointers).  hip_stream (a hipStream_t; NULL = the legacy default stream, which is also PyTorch's
 * current stream unless told otherwise): the slab is read only after everything enqueued on that stream
 * so far has completed -- the context's own streams are non-blocking, so the dependency is always made
 * explicit with an event, also for NULL; GZPX_STREAM_NONE: no dependency at all, the slab is ready now.
 * Synchronous with respect to the host on return. */
int gzpx_compress_slab_device(gzpx_ctx *ctx, const void *d_in, size_t in_len, int mode,
                              void *d_out, size_t out_cap, size_t *out_len, uint32_t *block_sizes,
                              size_t max_blocks, size_t *n_blocks, void *hip_stream);

/*
 * Asynchronous form ("async variant with stream/event handles for H2D || kernel || D2H
 * overlap").  A context owns a copy-in stream, a compute stream and a copy-out stream and up to
 * GZPX_SLOTS slabs in flight, each with its own device staging buffers:
 *
 *   gzpx_compress_slab_submit   enqueues the copy-in of `in` (page-locked memory makes it a DMA
 *                               transfer: gzpx_host_alloc) and every kernel of the slab, and returns
 *                               without waiting for the device, at every level.  GZPX_ERR_BUSY when all
 *                               slots are taken.  `in` and `out` must stay valid until the wait.
 *   gzpx_compress_slab_wait     blocks until that slab's kernels are done, copies exactly the
 *                               produced bytes to `out`, reports like gzpx_compress_slab, frees the slot.
 *
 * Submitting slab k+1 before waiting for slab k overlaps k+1's copy-in with k's kernels and k's
 * copy-out with k+1's kernels; results come back in submission order if waited for in that order.
 * The _device form works on device pointers (no copies); `after_stream` as above.
 * gzpx_compress_slab_event hands out the hipEvent_t that fires when the slab's kernels and result
 * records are complete, for callers that chain their own streams (valid until the wait).
 */
#define GZPX_SLOTS 3
int gzpx_compress_slab_submit(gzpx_ctx *ctx, const uint8_t *in, size_t in_len, int mode, uint8_t *out,
                              size_t out_cap, uint64_t *ticket);
int gzpx_compress_slab_submit_device(gzpx_ctx *ctx, const void *d_in, size_t in_len, int mode, void *d_out,
                                     size_t out_cap, void *after_stream, uint64_t *ticket);
int gzpx_compress_slab_wait(gzpx_ctx *ctx, uint64_t ticket, size_t *out_len, uint32_t *block_sizes,
                            size_t max_blocks, size_t *n_blocks);
int gzpx_compress_slab_event(gzpx_ctx *ctx, uint64_t ticket, void **hip_event);

/*
 * Multi-device form: one context per entry of devices[]; a slab is cut into
 * that many contiguous block ranges (balanced to one block; only the range holding the slab's end
 * takes `mode`), every device compresses its range concurrently, and once the shard sizes are known
 * each device copies its shard straight to its offset in `out` -- the in-order write-out without any
 * payload crossing between GPUs.  Same result, byte for byte, as gzpx_compress_slab on one device.
 * (One process per GPU + an RCCL gather of the shards: gzp_amd/shard.py, bench.py --gpus N.)
 */
typedef struct gzpx_multi gzpx_multi;
int gzpx_multi_create(const gzpx_config *cfg, const int *devices, size_t n_devices, gzpx_multi **out);
void gzpx_multi_destroy(gzpx_multi *m);
size_t gzpx_multi_devices(const gzpx_multi *m);
int gzpx_multi_compress_slab(gzpx_multi *m, const uint8_t *in, size_t in_len, int mode, uint8_t *out,
                             size_t out_cap, size_t *out_len, uint32_t *block_sizes, size_t max_blocks,
                             size_t *n_blocks);

/* The same with every range already resident on its own device -- north_star's "shard of the input slab
 * across 8 GPUs with a gather of compressed blocks over xGMI for in-order write-out": d_in[g] is a device
 * pointer ON devices[g] to range g of the slab (gzpx_multi_shard tells offset and length of range g for a
 * slab of in_len bytes), every device compresses its range into its own staging, and each shard is then
 * copied once, device to device (hipMemcpyPeerAsync, all peers at once), into its stream offset of d_out on
 * devices[root].  No payload passes through host memory; only the 16-byte result records and the
 * per-block sizes do.  Byte for byte the stream of gzpx_compress_slab.  Replaces the writer thread's
 * in-order collection, src/par/compress.rs:305-310.
 * Caller contract: the ranges d_in[g] are complete and d_out is IDLE on entry (no work of the caller still reads
 * or writes it on any stream of devices[root]) -- the call orders its kernels and peer copies among themselves
 * and returns when all of them are done, but takes no stream or event of the caller to wait behind. */
int gzpx_multi_shard(const gzpx_multi *m, size_t in_len, size_t g, size_t *offset, size_t *len);
int gzpx_multi_compress_slab_device(gzpx_multi *m, const void *const *d_in, size_t in_len, int mode, size_t root,
                                    void *d_out, size_t out_cap, size_t *out_len, uint32_t *block_sizes,
                                    size_t max_blocks, size_t *n_blocks);

/* FormatSpec::encode: one framed block (is_last => BGZF_EOF appended for BGZF; ignored for Snap, src/snap.rs:61-74). */
int gzpx_encode_block(gzpx_ctx *ctx, const uint8_t *in, size_t n, int is_last, uint8_t *out,
                      size_t out_cap, size_t *out_len);

/* ---- libdeflate-shaped per-block ABI (what libdeflater binds) ---- */
typedef struct gzpx_compressor gzpx_compressor;
gzpx_compressor *gzpx_alloc_compressor(int level); /* NULL: bad level / no device / unsupported */
size_t gzpx_deflate_compress(gzpx_compressor *c, const void *in, size_t n, void *out, size_t cap);
size_t gzpx_deflate_compress_bound(gzpx_compressor *c, size_t n);
void gzpx_free_compressor(gzpx_compressor *c);
/* compat / device knobs for the handle above (before first use) */
int gzpx_compressor_set_compat(gzpx_compressor *c, int compat);
uint32_t gzpx_crc32(uint32_t crc, const void *buf, size_t n);
/* libdeflate_crc32's signature cannot report a failure: on a device error gzpx_crc32 returns `crc`
 * unchanged and records the status for the calling thread; gzpx_crc32_checked returns it directly. */
int gzpx_crc32_checked(uint32_t crc, const void *buf, size_t n, uint32_t *out);
int gzpx_last_status(void);

/* The checks of gzp's Gzip / Zlib formats (src/check.rs:85-164) as helpers; the encoders of those formats are not
 * built (zlib-ng's output cannot be pinned in this image), so nothing inside the library calls these.
 *   gzpx_crc32_combine    Crc32::combine (flate2::Crc::combine, src/check.rs:160-163): the CRC-32 of A || B from crc(A),
 *                         crc(B) and |B|.  Arithmetic only.  (Crc32::update is gzpx_crc32 above.)
 *   gzpx_adler32          Adler32::update (libz_ng_sys::adler32, src/check.rs:112-119): start with 1.  On the device;
 *                         errors as gzpx_crc32 (gzpx_last_status), gzpx_adler32_checked returns them.
 *   gzpx_adler32_combine  Adler32::combine (adler32_combine, src/check.rs:121-127).  Arithmetic only. */
uint32_t gzpx_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);
uint32_t gzpx_adler32(uint32_t adler, const void *buf, size_t n);
int gzpx_adler32_checked(uint32_t adler, const void *buf, size_t n, uint32_t *out);
uint32_t gzpx_adler32_combine(uint32_t adler1, uint32_t adler2, uint64_t len2);

/* ---- ParCompress<Bgzf/Mgzip> twin: Write + ZWriter::finish over device lanes (C++ class
 * gzp::ParCompress in gzp_amd/csrc/gzpx_par.hpp; src/par/compress.rs:33-469) ---- */
typedef struct gzpx_par gzpx_par;
typedef int (*gzpx_write_fn)(void *user, const uint8_t *data, size_t n); /* 0 = ok (the `W: Write`) */
typedef struct gzpx_par_config {
    int format;          /* GZPX_FORMAT_*                                               */
    int level;           /* ParCompressBuilder::compression_level                       */
    int compat;          /* GZPX_COMPAT_*                                               */
    int device;          /* HIP device                                                  */
    size_t buffer_size;  /* ParCompressBuilder::buffer_size (>= 32768)                  */
    size_t num_threads;  /* ParCompressBuilder::num_threads (> 0); > 1 adds copy helpers */
    size_t batch_blocks; /* blocks per slab handed to the device (0 = default 1024; a slab is capped at 128 MiB) */
} gzpx_par_config;
int gzpx_par_create(const gzpx_par_config *cfg, gzpx_write_fn write_fn, void *user, gzpx_par **out);
/* the same with ParCompressBuilder::pin_threads(Some(first_core)) (src/par/compress.rs:99-107): the
 * twin's device thread and copy helpers are pinned to consecutive cores the process may run on */
int gzpx_par_create_pinned(const gzpx_par_config *cfg, size_t first_core, gzpx_write_fn write_fn, void *user,
                           gzpx_par **out);
int gzpx_par_write(gzpx_par *p, const uint8_t *buf, size_t n);
/* The loop of the reference's own benchmark (benches/bench.rs:36-45: read 64 KiB, write_all it) on the
 * native side of the boundary: n bytes through write() calls of `chunk` bytes each.  What a Rust caller
 * of gzpx_par_write sees without this binding's per-call cost; same stream as one write() of n bytes. */
int gzpx_par_write_chunked(gzpx_par *p, const uint8_t *buf, size_t n, size_t chunk);
/* In-place form of write() for producers that can fill memory they are handed (read(2) into the
 * slab, a decoder's output): reserve returns room (>= buffer_size bytes) inside the page-locked slab
 * that is being filled, commit appends the first n bytes of it to the stream.  Same cut rule as
 * write(), no copy on the way to the device. */
int gzpx_par_reserve(gzpx_par *p, uint8_t **ptr, size_t *cap);
int gzpx_par_commit(gzpx_par *p, size_t n);
int gzpx_par_flush(gzpx_par *p);
int gzpx_par_finish(gzpx_par *p);
void gzpx_par_destroy(gzpx_par *p);
const char *gzpx_par_last_error(const gzpx_par *p);

/* ---- block index side-product (README.md:161 "Return an auto-generated index for BGZF / Mgzip
 * formats"): where every block written so far starts in the compressed and in the uncompressed
 * stream, in stream order; complete after gzpx_par_finish.  gzpx_gzi_write serialises it in
 * htslib's .gzi layout (u64 count, then (compressed, uncompressed) u64 pairs of every block but
 * the first, little-endian). */
typedef struct gzpx_index_entry {
    uint64_t compressed_offset;
    uint64_t uncompressed_offset;
} gzpx_index_entry;
int gzpx_par_index(gzpx_par *p, gzpx_index_entry *entries, size_t max_entries, size_t *n_entries);
size_t gzpx_gzi_size(size_t n_entries);
int gzpx_gzi_write(const gzpx_index_entry *entries, size_t n_entries, uint8_t *out, size_t out_cap,
                   size_t *out_len);

/* ---- ParDecompress<Bgzf/Mgzip> (src/par/decompress.rs:132-337; BlockFormatSpec src/lib.rs:411-448) ----
 *   gzpx_scan_blocks            the reader thread's header walk: check_header + get_block_size
 *                               (src/deflate.rs:555-570 / 405-422) over a host buffer
 *   gzpx_decompress_blocks*     the worker loop (src/par/decompress.rs:162-186) for every block of a
 *                               slab: get_footer_values, decode_block = libdeflate_deflate_decompress
 *                               into ISIZE bytes, LibDeflateCrc check (src/check.rs:38-82)
 *   gzpx_*_decompressor         libdeflater::Decompressor (libdeflate.h: libdeflate_alloc_decompressor,
 *                               libdeflate_deflate_decompress, libdeflate_free_decompressor)
 */
typedef struct gzpx_dctx gzpx_dctx;
typedef struct gzpx_check_info {
    size_t block;            /* index of the block that failed (any error)          */
    uint32_t found, expected; /* InvalidCheck { found, expected }                    */
} gzpx_check_info;
int gzpx_dctx_create(int device, int format, gzpx_dctx **out);
void gzpx_dctx_destroy(gzpx_dctx *ctx);
/* Walks the block headers in in[0..in_len).  offsets[i] / sizes[i]: start and total size of block
 * i; *consumed: bytes covered by complete blocks (a trailing partial block is left to the caller,
 * as read_exact would block on it).  GZPX_ERR_INVALID_HEADER for a header that fails check_header. */
int gzpx_scan_blocks(int format, const uint8_t *in, size_t in_len, uint64_t *offsets, uint32_t *sizes,
                     size_t max_blocks, size_t *n_blocks, size_t *consumed);
int gzpx_decompress_blocks(gzpx_dctx *ctx, const uint8_t *in, size_t in_len, const uint64_t *offsets,
                           const uint32_t *sizes, size_t n_blocks, uint8_t *out, size_t out_cap,
                           size_t *out_len, gzpx_check_info *info);
/* asynchronous form (same slots / streams scheme as gzpx_compress_slab_submit): the copy-in, the
 * kernels and the copy-out of the inflated bytes (their count is the sum of the footers' ISIZE fields,
 * known at submit time) are all enqueued by submit; wait blocks for them and reports the first
 * failing block in stream order.  offsets / sizes are copied by submit. */
int gzpx_decompress_blocks_submit(gzpx_dctx *ctx, const uint8_t *in, size_t in_len, const uint64_t *offsets,
                                  const uint32_t *sizes, size_t n_blocks, uint8_t *out, size_t out_cap,
                                  uint64_t *ticket);
int gzpx_decompress_blocks_wait(gzpx_dctx *ctx, uint64_t ticket, size_t *out_len, gzpx_check_info *info);
/* d_in / d_out are device pointers; offsets / sizes stay host arrays */
int gzpx_decompress_blocks_device(gzpx_dctx *ctx, const void *d_in, size_t in_len, const uint64_t *offsets,
                                  const uint32_t *sizes, size_t n_blocks, void *d_out, size_t out_cap,
                                  size_t *out_len, gzpx_check_info *info, void *hip_stream);
/* ---- the same for a stream that lies in device memory: the members are found on the device (gzpx_mscan.h), no
 * member table and no byte of the stream crosses to the host first.  hip_stream as for gzpx_decompress_blocks_device. */
/* gzpx_scan_blocks for a stream in device memory.  offsets / sizes: optional HOST arrays (both or neither);
 * result identical to gzpx_scan_blocks on the same bytes, for every input and every max_blocks. */
int gzpx_scan_blocks_device(gzpx_dctx *ctx, const void *d_in, size_t in_len, uint64_t *offsets, uint32_t *sizes,
                            size_t max_blocks, size_t *n_blocks, size_t *consumed, void *hip_stream);
/* scan + inflate with no member table crossing to the host: every complete member of d_in[0..in_len) is inflated
 * to d_out back to back; *consumed as above (a trailing partial member is the caller's).  An invalid header:
 * GZPX_ERR_INVALID_HEADER, nothing inflated.  Otherwise as gzpx_decompress_blocks_device with the walk's table. */
int gzpx_decompress_stream_device(gzpx_dctx *ctx, const void *d_in, size_t in_len, void *d_out, size_t out_cap,
                                  size_t *out_len, size_t *n_blocks, size_t *consumed, gzpx_check_info *info,
                                  void *hip_stream);
/* the block index of a stream nobody here wrote: one entry per member as a reader sees them (so the BGZF EOF
 * marker is an entry; gzpx_par_index, the writer's view, has none for it), compressed offset = member start,
 * uncompressed offset = exclusive prefix sum of the footers' ISIZE; *inflated_len = the total.  entries: host array
 * (may be NULL), the first max_entries are written, *n_entries = how many there are. */
int gzpx_index_device(gzpx_dctx *ctx, const void *d_in, size_t in_len, gzpx_index_entry *entries,
                      size_t max_entries, size_t *n_entries, size_t *consumed, uint64_t *inflated_len,
                      void *hip_stream);
/* HIP-event duration of the member-discovery kernels in the last of these three calls on this context (a scan whose
 * candidate arrays were too small ran twice: both runs and the reallocation between them are inside) */
int gzpx_dctx_last_scan_ms(gzpx_dctx *ctx, float *ms);
/* ---- random access by range (gzpx_ranges.h): the index of a device-resident stream kept ON the device, and reads of
 * a batch of byte ranges of the inflated stream that inflate only the members the ranges touch.
 * gzpx_dindex_build_device: the walk of gzpx_index_device (same *consumed / *inflated_len, same
 * GZPX_ERR_INVALID_HEADER, a trailing partial member left out); the member offsets, the member sizes and the
 * exclusive prefix sum of ISIZE stay in device memory owned by *out, only the scan record and the total cross to the
 * host.  An empty stream gives a valid index of 0 members.  gzpx_dindex_entries copies the tables out: identical to
 * what gzpx_index_device returns on the same bytes.  An index belongs to the device and the format of its context.
 * (A .gzi file cannot be imported: it has no member sizes and no entry for the first or the EOF member.) */
typedef struct gzpx_dindex gzpx_dindex;
int gzpx_dindex_build_device(gzpx_dctx *ctx, const void *d_in, size_t in_len, gzpx_dindex **out, size_t *n_members,
                             size_t *consumed, uint64_t *inflated_len, void *hip_stream);
int gzpx_dindex_entries(const gzpx_dindex *ix, gzpx_index_entry *entries, size_t max_entries, size_t *n_entries);
void gzpx_dindex_destroy(gzpx_dindex *ix);
typedef struct gzpx_range {
    uint64_t begin, end; /* [begin, end) */
} gzpx_range;
#define GZPX_RANGE_UNCOMPRESSED 0 /* offsets into the inflated stream                            */
#define GZPX_RANGE_VIRTUAL 1      /* BGZF virtual offsets: member start << 16 | offset in member */
/* Reads n_ranges ranges of the inflated stream into d_out, back to back in the order given: the bytes of range r
 * land at d_out + out_offsets[r], *out_len is the total (out_offsets: optional HOST array of n_ranges + 1).
 * `ranges` is a host array; d_in / in_len are the bytes the index was built from (the address may differ; in_len
 * below the index's `consumed`: GZPX_ERR_INVALID_ARG); hip_stream as for gzpx_decompress_blocks_device.  Returns
 * synchronised; runs under the context's lock and uses one slot, like gzpx_decompress_stream_device.
 *   Ranges may overlap or repeat (their bytes are repeated in the output) and may be empty; n_ranges == 0 is OK with
 *   0 bytes.  GZPX_RANGE_UNCOMPRESSED: begin <= end <= inflated_len.  GZPX_RANGE_VIRTUAL (BGZF contexts only, else
 *   GZPX_ERR_INVALID_ARG): the upper 48 bits are exactly a member start of the index, the lower 16 are <= that
 *   member's ISIZE (equal: the position in front of the next member), and begin does not lie behind end in stream
 *   order.  A range that breaks these rules: GZPX_ERR_INVALID_ARG with *bad_range = the first such range, nothing
 *   inflated.  The total is known before anything is inflated: above out_cap the call returns
 *   GZPX_ERR_INSUFFICIENT_SPACE with *out_len = the bytes needed, nothing inflated.
 *   Members read: for a non-empty range, `first` = the last member whose uncompressed start is <= begin, `last` =
 *   the last member whose uncompressed start is < end; the union of [first, last] over the non-empty ranges is
 *   read, every member once however many ranges touch it, and no byte of any other member
 *   (gzpx_dctx_last_ranges_members: the size of that union in the last call).  Every member read is inflated whole
 *   and its CRC and ISIZE are checked as everywhere else: GZPX_ERR_BAD_DATA / GZPX_ERR_INVALID_CHECK /
 *   GZPX_ERR_INSUFFICIENT_SPACE (an ISIZE that lies) for the first failing member in stream order, info->block = its
 *   index IN THE STREAM (after such a failure d_out[0..total) holds nothing of use: the slices are cut behind the
 *   inflate without a round trip in between).  Both inflate routes (gzpx_dctx_set_route) serve it.
 * gzpx_dctx_last_ranges_ms: HIP-event durations of the last call's stages: [0] locate + select, [1] inflate into the
 * context's staging buffer, [2] gather. */
int gzpx_read_ranges_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const void *d_in, size_t in_len,
                            const gzpx_range *ranges, size_t n_ranges, int coords, void *d_out, size_t out_cap,
                            size_t *out_len, uint64_t *out_offsets, size_t *bad_range, gzpx_check_info *info,
                            void *hip_stream);
int gzpx_dctx_last_ranges_members(gzpx_dctx *ctx, size_t *n_members_read);
int gzpx_dctx_last_ranges_ms(gzpx_dctx *ctx, float ms[3]);
/* ---- reads by line (gzpx_lines.h): text in a device-resident BGZF / Mgzip stream -- FASTQ, VCF, CSV, JSONL -- is
 * fetched by LINE numbers, without the detour of inflating everything and searching it on the host.  A table of
 * delimiter counts is built once per stream; a read then inflates only the members that hold its boundaries' tiles
 * and its bytes.
 * Definitions.  `delim` is one byte (default '\n'; '\r' is an ordinary byte).  T = GZPX_LINES_TILE.  D = the number
 *   of delimiter bytes in the inflated stream.  L = the number of lines: L = D when the stream is empty or its last
 *   byte is `delim`, else L = D + 1 (the last line is unterminated).  A line includes its delimiter.
 *   start(k) for 0 <= k <= L: start(0) = 0; start(k) = 1 + the position of the k-th delimiter (counting from 1) for
 *   1 <= k <= D; start(D + 1) = inflated_len when L = D + 1.  The line range [a, b), a <= b <= L, is the bytes
 *   [start(a), start(b)).
 *   Tile t is the inflated bytes [T t, min(T (t + 1), inflated_len)): a grid fixed on the inflated stream, independent
 *   of the members.  P[t] = the number of delimiters in tiles 0..t-1, uint64, tiles + 1 entries, P[tiles] = D.  The
 *   tile of boundary k, 1 <= k <= D, is the t with P[t] < k <= P[t + 1].
 * gzpx_dlines_build_device inflates EVERY member of the index into the context's staging buffer (CRC and ISIZE checked
 *   as everywhere), in batches of whole members of at most gzpx_dctx_set_lines_batch inflated bytes (0 = the default,
 *   256 MiB; a larger member is a batch of its own; the value serves gzpx_find_device too), counts the delimiters of every tile behind each batch (a tile that
 *   two batches share gets both parts) and forms P.  P and a record (D, L, whether the last byte is a delimiter) stay
 *   in device memory owned by *out; *n_delims = D, *n_lines = L (both optional).  A failing member: the inflate's
 *   error, info->block = its index in the stream, *out = NULL.  An empty stream or an index of 0 members: a valid table
 *   with D = L = 0.  delim > 255: GZPX_ERR_INVALID_ARG.  gzpx_dlines_prefix copies P out (gzpx_dindex_entries' shape).
 *   A table remembers the index it was built for (device, format, members, consumed, inflated_len): with another
 *   index or context the calls below return GZPX_ERR_INVALID_ARG.
 * gzpx_read_lines_device follows gzpx_read_ranges_device: the ranges' bytes back to back in the order given, overlaps
 *   and duplicates repeated, empty ranges allowed ([L, L) among them), n_ranges == 0 OK; hip_stream, the lock and the
 *   slot likewise; it returns synchronised.  A range with a > b or b > L: GZPX_ERR_INVALID_ARG, *bad_range = the
 *   first such range, nothing inflated.
 *   Members read.  The cover of a non-empty range [a, b) is the inflated bytes from (a == 0 ? 0 : T tile(a)) to
 *   (b > D ? inflated_len : min(T (tile(b) + 1), inflated_len)).  The members read are the union over the covers of
 *   [first, last] by gzpx_read_ranges_device's rule, each once, and no byte of any other member
 *   (gzpx_dctx_last_lines_members: the size of that union in the last call).  An empty range reads nothing; its
 *   boundary is not searched for, and byte_ranges reports it as {0, 0}.
 *   The total is known only behind the search: above out_cap the call returns GZPX_ERR_INSUFFICIENT_SPACE with
 *   *out_len = the bytes needed and nothing written to d_out.  A member that fails its check: the error as for
 *   gzpx_read_ranges_device, info->block = its index in the stream, d_out holds nothing of use.  out_offsets
 *   (n_ranges + 1) and byte_ranges (n_ranges: [start(a), start(b)) of every range) are optional HOST arrays.
 * gzpx_line_offsets_device is the same search without the gather: offsets[i] = start(lines[i]) (host arrays),
 *   lines[i] <= L, else GZPX_ERR_INVALID_ARG with *bad = i.  lines[i] == 0 or > D needs no member; the members read
 *   are the union over the other boundaries' own tiles [T t, min(T (t + 1), inflated_len)).
 * gzpx_dctx_last_lines_ms: HIP-event durations of the last search's stages: [0] boundary tiles + locate + select,
 *   [1] inflate, [2] boundary search, [3] gather.  gzpx_dctx_last_lines_build_ms: the last build's [0] inflate and
 *   [1] count kernels, summed over its batches. */
#define GZPX_LINES_TILE 16384
typedef struct gzpx_dlines gzpx_dlines;
int gzpx_dlines_build_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const void *d_in, size_t in_len, unsigned delim,
                             gzpx_dlines **out, uint64_t *n_delims, uint64_t *n_lines, gzpx_check_info *info,
                             void *hip_stream);
int gzpx_dlines_prefix(const gzpx_dlines *lines, uint64_t *prefix, size_t max_entries, size_t *n_entries);
void gzpx_dlines_destroy(gzpx_dlines *lines);
int gzpx_line_offsets_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in, size_t in_len,
                             const uint64_t *line_numbers, size_t n, uint64_t *offsets, size_t *bad, gzpx_check_info *info,
                             void *hip_stream);
int gzpx_read_lines_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in, size_t in_len,
                           const gzpx_range *line_ranges, size_t n_ranges, void *d_out, size_t out_cap, size_t *out_len,
                           uint64_t *out_offsets, gzpx_range *byte_ranges, size_t *bad_range, gzpx_check_info *info,
                           void *hip_stream);
int gzpx_dctx_set_lines_batch(gzpx_dctx *ctx, size_t inflated_bytes);
int gzpx_dctx_last_lines_members(gzpx_dctx *ctx, size_t *n_members_read);
int gzpx_dctx_last_lines_ms(gzpx_dctx *ctx, float ms[4]);
int gzpx_dctx_last_lines_build_ms(gzpx_dctx *ctx, float ms[2]);
/* ---- search (gzpx_find.h): WHERE a byte string occurs in a device-resident BGZF / Mgzip stream -- the records whose
 * name starts with a prefix, the lines of one contig ("\nchr7\t"), an adapter sequence -- as byte positions for
 * gzpx_read_ranges_device and line numbers for gzpx_read_lines_device, with nothing but a table of hits leaving the
 * device.
 * Definitions.  `plain` is the inflated stream of the index, n = inflated_len.  The pattern is a HOST array of m bytes,
 *   1 <= m <= GZPX_FIND_MAX_PATTERN, any byte values.  A HIT is a position p, 0 <= p <= n - m, with
 *   plain[p .. p + m) == pattern.  Overlapping hits all count ("aa" in "aaaa": 0, 1, 2); hits are reported in
 *   ascending p.  Where in the stream a hit lies plays no part: it may straddle 16-byte words, members (empty members
 *   between them included) and the batches of the inflate.
 *   The LINE of a hit is the number of `delim` bytes in plain[0 .. p): the line that holds the hit's FIRST byte, in the
 *   numbering of the reads by line, start(line) <= p < start(line + 1).  A pattern may contain the delimiter
 *   ("\n@SRR" anchors at a line start; its hits lie in the line that the "\n" ends).  No gzpx_dlines table is needed.
 * gzpx_find_device inflates EVERY member of the index once into the context's staging buffer (CRC and ISIZE checked as
 *   everywhere), in the batches of gzpx_dlines_build_device -- gzpx_dctx_set_lines_batch serves both calls -- and
 *   searches each batch behind its inflate: a batch finds the hits whose last byte lies in it, from the last m - 1
 *   bytes of the earlier batches kept in front of it.  A count-only call and a writing call inflate once each.
 *   d_positions and d_lines are DEVICE arrays of hits_cap uint64 entries; each is optional.  Both NULL: count only,
 *   hits_cap is ignored, GZPX_OK.  *n_hits is always the number of hits in the whole stream.  When it exceeds hits_cap
 *   and an output array was given, the first hits_cap hits are written, nothing behind hits_cap entries is touched and
 *   the call returns GZPX_ERR_INSUFFICIENT_SPACE: call again with the size now known.
 *   delim is a byte value, or GZPX_FIND_NO_LINES; outside -1..255, or GZPX_FIND_NO_LINES with d_lines given:
 *   GZPX_ERR_INVALID_ARG.  pattern_len 0 or above GZPX_FIND_MAX_PATTERN: GZPX_ERR_INVALID_ARG.  m > n, an empty stream
 *   or an index of 0 members: GZPX_OK with 0 hits and nothing inflated.
 *   Index and context as for gzpx_dlines_build_device: device, format and in_len >= consumed are checked, the
 *   context's lock is taken, one slot is used, hip_stream is ordered in front, the call returns synchronised.  A
 *   failing member ends the call with the inflate's error, info->block = its index in the stream, *n_hits = 0, and
 *   the output arrays hold nothing of use.
 * gzpx_dctx_last_find_ms: HIP-event durations of the last call, summed over its batches: [0] inflate, [1] counting
 *   pass + scan, [2] writing pass + carry. */
#define GZPX_FIND_MAX_PATTERN 256
#define GZPX_FIND_NO_LINES (-1)
int gzpx_find_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const void *d_in, size_t in_len, const void *pattern,
                     size_t pattern_len, int delim, uint64_t *d_positions, uint64_t *d_lines, size_t hits_cap, uint64_t *n_hits,
                     gzpx_check_info *info, void *hip_stream);
int gzpx_dctx_last_find_ms(gzpx_dctx *ctx, float ms[3]);
/* ---- selection of lines by content (gzpx_select.h): grep, grep -v and record-wise grep on a device-resident BGZF /
 * Mgzip stream -- the FASTQ records whose name starts with a prefix, the VCF rows of one contig, every line that does
 * not hold a string -- as a table of LINE RANGES that stays in device memory, and a form of the read by line that takes
 * such a table where it lies.  Only fixed-size records cross to the host.
 * Definitions.  `plain`, n, the pattern, m and HIT are exactly as for gzpx_find_device.  `delim`, D, L, start(k) and
 *   "line" are exactly as for the reads by line, taken from the gzpx_dlines table that is passed in: the selection has
 *   no delimiter argument of its own.
 *   The LINE of a hit is the line of its first byte (gzpx_find_device's rule).  A pattern may hold the delimiter:
 *   "\nchr7\t" selects the line that the "\n" ends, as the search reports it.
 *   `group` = g >= 1 lines form a RECORD: record r is the lines [g r, min(g (r + 1), L)); R = ceil(L / g); the last
 *   record may be short.  A record is HIT when the line of at least one hit lies in it.  The selected set S is the hit
 *   records; with GZPX_SELECT_INVERT it is the records of [0, R) that are not hit.
 *   A RUN is a maximal interval [r0, r1) of consecutive selected records.  Runs are reported in ascending order as LINE
 *   ranges {g r0, min(g r1, L)} in gzpx_range.  There are at most ceil(R / 2) runs, so a table can always be sized in
 *   advance.
 * gzpx_select_lines_device.  Context, lock, slot, hip_stream, "returns synchronised", the batches
 *   (gzpx_dctx_set_lines_batch) and the report of a failing member (the inflate's error, info->block = its index in the
 *   stream) are as for gzpx_find_device; on a failing member *n_runs = *n_records = 0.  Every member is inflated once
 *   per call, whatever runs_cap is.  The pattern is a HOST array; d_runs is a DEVICE array of runs_cap entries.
 *   *n_runs and *n_records (the selected records) are always the totals; *n_hits (optional) is what gzpx_find_device
 *   reports.  d_runs == NULL: count only, runs_cap is ignored.  Otherwise, when there are more than runs_cap runs, the
 *   first runs_cap are written, nothing behind runs_cap entries is touched and the call returns
 *   GZPX_ERR_INSUFFICIENT_SPACE.
 *   GZPX_ERR_INVALID_ARG: group == 0; a flag bit other than GZPX_SELECT_INVERT; pattern_len 0 or above
 *   GZPX_FIND_MAX_PATTERN; a lines table that does not belong to the index and context (gzpx_read_lines_device's
 *   check); R > 0xFFFFFFF0.
 *   L == 0: GZPX_OK, 0 runs, nothing inflated.  m > n: no hit can exist and nothing is inflated; without INVERT that is
 *   0 runs, with INVERT the one run {0, L}.
 *   gzpx_dctx_last_select_ms: HIP-event durations of the last call: [0] inflate and [1] counting pass + scan + marking
 *   pass, summed over its batches, [2] the runs.
 * gzpx_read_lines_table_device is gzpx_read_lines_device with its tables in device memory: validation and *bad_range,
 *   the covers and the members read, GZPX_ERR_INSUFFICIENT_SPACE with *out_len = the bytes needed and d_out untouched,
 *   empty ranges reported as {0, 0}, gzpx_dctx_last_lines_members and gzpx_dctx_last_lines_ms are the same, word for
 *   word.  d_line_ranges (n_ranges entries) is read where it lies, ordered behind hip_stream like d_in;
 *   d_out_offsets (n_ranges + 1) and d_byte_ranges (n_ranges), both optional, are written in device memory, by the
 *   time the call returns, under the conditions under which gzpx_read_lines_device writes its host arrays.  No table
 *   sized by n_ranges crosses to the host in either direction: two 32-byte records do. */
#define GZPX_SELECT_INVERT 1u
int gzpx_select_lines_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in, size_t in_len,
                             const void *pattern, size_t pattern_len, uint64_t group, unsigned flags, gzpx_range *d_runs,
                             size_t runs_cap, uint64_t *n_runs, uint64_t *n_records, uint64_t *n_hits, gzpx_check_info *info,
                             void *hip_stream);
int gzpx_dctx_last_select_ms(gzpx_dctx *ctx, float ms[3]);
int gzpx_read_lines_table_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in,
                                 size_t in_len, const gzpx_range *d_line_ranges, size_t n_ranges, void *d_out, size_t out_cap,
                                 size_t *out_len, uint64_t *d_out_offsets, gzpx_range *d_byte_ranges, size_t *bad_range,
                                 gzpx_check_info *info, void *hip_stream);
/* ---- fields of lines (gzpx_fields.h): the column half of "rows and columns of a compressed table in HBM" -- the
 * eight fixed columns of a VCF without its thousands of sample columns, one column of a TSV, the name field of a
 * SAM-like line -- cut -f with -d on the lines of a device-resident BGZF / Mgzip stream.  The table that
 * gzpx_select_lines_device leaves in device memory goes straight in; the output is bytes in device memory.
 * Lines, delimiter and covers.  `plain`, `delim`, D, L, start(k), "line", line ranges, the covers and the members read
 *   are those of gzpx_read_lines_device, word for word, and so are validation and *bad_range, empty ranges, overlapping
 *   and repeated ranges (their output is repeated), the context's lock, the slot, hip_stream, "returns synchronised",
 *   both inflate routes and the report of a failing member (the inflate's error, info->block = its index in the stream).
 * Field delimiter and field list.  `field_delim` is one byte, any value; above 255, or equal to the lines table's
 *   delimiter: GZPX_ERR_INVALID_ARG.  The BODY of a line is the line without its delimiter; the unterminated last line
 *   is all body.  The body splits at every field_delim byte into F = (the number of such bytes) + 1 FIELDS, numbered
 *   from 0: an empty body is one empty field, consecutive delimiters give empty fields.
 *   `fields` is a HOST array of 1..GZPX_FIELDS_MAX_RANGES half-open ranges [begin, end) of field numbers, each with
 *   begin < end, ascending and disjoint (fields[i].end <= fields[i + 1].begin); end == GZPX_FIELDS_TO_END (through the
 *   line's last field) is allowed in the last range only.  S is the union of the ranges, or with
 *   GZPX_FIELDS_COMPLEMENT its complement in [0, infinity); an empty S is legal.  A list that breaks a rule, or a flag bit
 *   other than GZPX_FIELDS_COMPLEMENT: GZPX_ERR_INVALID_ARG with nothing inflated.
 * Output of one line.  The fields k in S with k < F, ascending, joined by one field_delim; then the line's delimiter,
 *   if and only if the line has one.  A line in which no selected field exists yields just its delimiter.  Field order
 *   is never changed and nothing is repeated within a line.  This is cut -f with -d (--complement), WITHOUT cut's special
 *   case for lines that hold no delimiter: such a line is one field, number 0, and is kept or dropped like any other.
 *   The same rule per byte, as the kernels apply it -- every output byte is an input byte, in input order; s0 = min S:
 *   a body byte of field k is kept iff k is in S; the j-th field delimiter of a line (j >= 1, the one in front of field
 *   j) is kept iff j is in S and j > s0; the line delimiter is always kept.  Field numbers are counted and compared as
 *   64-bit values from the range's first byte to its last, across pieces of any number: nothing saturates.
 * Output of the call.  The lines of range 0, then those of range 1, and so on; *out_len = the total; out_offsets[r] =
 *   where range r's output starts, out_offsets[n_ranges] = *out_len (optional; n_ranges + 1 entries; written whenever
 *   the call returns GZPX_OK or GZPX_ERR_INSUFFICIENT_SPACE).  d_out == NULL (out_cap 0) is a size query: GZPX_OK, *out_len
 *   and the offsets are written, and the writing pass does not run.  With d_out given and the total above out_cap the
 *   call returns GZPX_ERR_INSUFFICIENT_SPACE with *out_len = the bytes needed and no byte of d_out written.  Bytes of
 *   d_out at and behind *out_len are never written.  n_ranges == 0 is OK with 0 bytes.  The result is the same bit for
 *   bit from run to run: no atomics place it.
 * gzpx_read_fields_device takes line_ranges and out_offsets as HOST arrays, gzpx_read_fields_table_device as DEVICE
 *   arrays (d_line_ranges is read where it lies, ordered behind hip_stream like d_in).  In the table form only
 *   fixed-size records cross to the host: no table sized by n_ranges or by the output does.
 * gzpx_dctx_last_fields_ms: HIP-event durations of the last call's three stages behind the search: [0] the field-carry
 *   pass and its scan, [1] the counting pass and its scan, [2] the writing pass (0 when it did not run).  The search's
 *   stages stay readable through gzpx_dctx_last_lines_ms, whose [3], the gather, is 0 for these calls;
 *   gzpx_dctx_last_lines_members answers as for a read by line. */
#define GZPX_FIELDS_MAX_RANGES 64
#define GZPX_FIELDS_COMPLEMENT 1u     /* cut --complement: every field NOT listed */
#define GZPX_FIELDS_TO_END UINT64_MAX /* as a range's `end`: through the line's last field */
int gzpx_read_fields_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in, size_t in_len,
                            const gzpx_range *line_ranges, size_t n_ranges, unsigned field_delim, const gzpx_range *fields,
                            size_t n_fields, unsigned flags, void *d_out, size_t out_cap, size_t *out_len, uint64_t *out_offsets,
                            size_t *bad_range, gzpx_check_info *info, void *hip_stream);
int gzpx_read_fields_table_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in,
                                  size_t in_len, const gzpx_range *d_line_ranges, size_t n_ranges, unsigned field_delim,
                                  const gzpx_range *fields, size_t n_fields, unsigned flags, void *d_out, size_t out_cap,
                                  size_t *out_len, uint64_t *d_out_offsets, size_t *bad_range, gzpx_check_info *info,
                                  void *hip_stream);
int gzpx_dctx_last_fields_ms(gzpx_dctx *ctx, float ms[3]);
/* ---- numeric columns of lines (gzpx_columns.h): the last step of grep ... | cut -f ... | <numbers> -- POS and QUAL
 * of a VCF, a column of measurements of a TSV -- one value per line and column as int64 / float64 arrays in device
 * memory, with a status byte per value.  gzpx_read_fields_device and everything in front of it are untouched.
 * Lines, delimiters, fields.  `plain`, `delim`, line ranges, covers and members read, validation and *bad_range, the
 *   context's lock, the slot, hip_stream, "returns synchronised", both inflate routes and the report of a failing member
 *   are gzpx_read_fields_device's, word for word.  So are field_delim (one byte, not the lines table's delimiter) and
 *   the split of a line's body at every field_delim into F fields numbered from 0.  '\r' is an ordinary byte.
 * Columns.  `cols` is a HOST array of 1..GZPX_COLUMNS_MAX entries: field numbers strictly ascending, `type` one of
 *   GZPX_COL_INT64 and GZPX_COL_FLOAT64, `reserved` 0.  Anything else: GZPX_ERR_INVALID_ARG with nothing inflated.
 * Rows.  Line i of range r is row rbase[r] + i, rbase the exclusive sum of (end - begin) over the ranges as given:
 *   overlapping and repeated ranges repeat their rows, empty ranges add none.  R is the total.  *n_rows = R always.
 *   row_offsets[r] = rbase[r], row_offsets[n_ranges] = R (optional; n_ranges + 1 entries; written whenever the call
 *   returns GZPX_OK or GZPX_ERR_INSUFFICIENT_SPACE).
 * Cells.  Column c, row i is the 8-byte cell d_values[c * rows_cap + i] (int64_t or double by the column's type) with
 *   its status byte at d_status[c * rows_cap + i].  d_values must be 8-byte aligned.  Either array may be NULL; with
 *   both NULL the call still counts and rows_cap is ignored.  With an array given and R > rows_cap:
 *   GZPX_ERR_INSUFFICIENT_SPACE, *n_rows = R, no byte of either array is written and the counts are 0.  Otherwise every
 *   cell with i < R is written exactly once and no cell with i >= R is touched in any column.  *n_not_ok is the number of
 *   cells whose status is not GZPX_CELL_OK; d_col_not_ok, an optional DEVICE array of n_cols entries, holds the same
 *   count per column.  A cell that is not OK holds 0 (INT64) or the quiet NaN 0x7FF8000000000000 (FLOAT64).
 * Status of the cell for field number f; the first rule that applies decides.  f >= F: MISSING.  A field of 0 bytes:
 *   EMPTY.  More than GZPX_CELL_MAX_BYTES bytes: INVALID, and its bytes are not looked at.  Not matched in full by the
 *   type's grammar: INVALID.  Otherwise RANGE or OK:
 *   INT64    [+-]?[0-9]+ ; OK iff the value lies in [-2^63, 2^63 - 1] (leading zeros do not count against it).
 *   FLOAT64  [+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)? or, case-insensitively, [+-]?(nan|inf|infinity).
 *            nan gives the quiet NaN above whatever its sign, inf the signed infinity.  A decimal number: join the
 *            integer and fraction digits and strip leading and trailing zeros; w = the value of what is left (0 if
 *            nothing is); q = exponent - (fraction digits) + (trailing zeros stripped).  w == 0: the signed zero, OK.
 *            w <= 2^53 and -22 <= q <= 22: OK, and the value is the ONE IEEE operation double(w) * 10^q or
 *            double(w) / 10^-q on two exact operands, negated for '-': the correctly rounded value (Clinger).
 *            Everything else is RANGE, an exponent of any number of digits included.  Plainly: numbers of up to 15
 *            significant digits with small exponents convert; the 16- and 17-digit output of repr() is mostly RANGE.
 *            A later version may convert RANGE cells in full; the status code keeps the ABI stable for it.
 * The result is the same bit for bit from run to run: scans place every cell, and the two counts are integer sums.
 * gzpx_read_columns_device takes line_ranges and row_offsets as HOST arrays, gzpx_read_columns_table_device as DEVICE
 *   arrays (d_line_ranges is read where it lies, ordered behind hip_stream like d_in).  In the table form only
 *   fixed-size records cross to the host.  n_ranges == 0 is OK with 0 rows.
 * gzpx_dctx_last_columns_ms: HIP-event durations of the last call's stages behind the search: [0] the field carries,
 *   the pieces' line counts and their scans, [1] the parsing pass.  gzpx_dctx_last_lines_ms and
 *   gzpx_dctx_last_lines_members answer as for gzpx_read_fields_device. */
#define GZPX_COLUMNS_MAX 16
#define GZPX_CELL_MAX_BYTES 64
#define GZPX_COL_INT64 0
#define GZPX_COL_FLOAT64 1
#define GZPX_CELL_OK 0      /* the value is the field's number */
#define GZPX_CELL_MISSING 1 /* the line has no field of that number */
#define GZPX_CELL_EMPTY 2   /* the field has no bytes */
#define GZPX_CELL_INVALID 3 /* longer than GZPX_CELL_MAX_BYTES, or not in the grammar */
#define GZPX_CELL_RANGE 4   /* in the grammar, outside what this call converts exactly */
typedef struct gzpx_column {
    uint64_t field;
    uint32_t type;
    uint32_t reserved;
} gzpx_column;
int gzpx_read_columns_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in, size_t in_len,
                             const gzpx_range *line_ranges, size_t n_ranges, unsigned field_delim, const gzpx_column *cols,
                             size_t n_cols, void *d_values, uint8_t *d_status, size_t rows_cap, uint64_t *n_rows,
                             uint64_t *n_not_ok, uint64_t *d_col_not_ok, uint64_t *row_offsets, size_t *bad_range,
                             gzpx_check_info *info, void *hip_stream);
int gzpx_read_columns_table_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in,
                                   size_t in_len, const gzpx_range *d_line_ranges, size_t n_ranges, unsigned field_delim,
                                   const gzpx_column *cols, size_t n_cols, void *d_values, uint8_t *d_status, size_t rows_cap,
                                   uint64_t *n_rows, uint64_t *n_not_ok, uint64_t *d_col_not_ok, uint64_t *d_row_offsets,
                                   size_t *bad_range, gzpx_check_info *info, void *hip_stream);
int gzpx_dctx_last_columns_ms(gzpx_dctx *ctx, float ms[2]);
/* ---- selection of lines by their numbers (gzpx_where.h): awk '$6 >= 30' between grep and cut -- the VCF rows with
 * QUAL >= 30 and 1000000 <= POS < 2000000, the TSV rows whose measurement is above a threshold -- as a table of line
 * ranges in device memory that gzpx_read_lines_table_device, gzpx_read_fields_table_device and
 * gzpx_read_columns_table_device take where it lies.  No cell array is materialised and only fixed-size records cross
 * to the host.  gzpx_read_columns_device and everything in front of it are untouched.
 * Lines, delimiters, fields, cells, rows.  `plain`, `delim`, line ranges, covers and members read, validation and
 *   *bad_range, empty, overlapping and repeated ranges, field_delim, the split of a line into fields, the cell grammar
 *   of both types and the five statuses, the rows (line i of range r is row rbase[r] + i, R the total), the context's
 *   lock, the slot, hip_stream, "returns synchronised", both inflate routes and the report of a failing member are
 *   gzpx_read_columns_device's, word for word: the two calls share the code that parses a cell.
 * Terms.  `terms` is a HOST array of 1..GZPX_WHERE_MAX_TERMS entries with `field` non-descending.  Several terms may
 *   name one field (100 <= POS, POS < 200); their `type` must then agree.  At most GZPX_COLUMNS_MAX distinct fields.
 *   `type` is GZPX_COL_INT64 or GZPX_COL_FLOAT64, `op` one of the eight GZPX_WHERE_*; `value` holds the bits of an
 *   int64_t or of a double by the type, must be 0 for IS_OK and NOT_OK, and for FLOAT64 must not be a NaN.  No flag bit
 *   beyond GZPX_WHERE_ANY and GZPX_WHERE_INVERT.  Anything else: GZPX_ERR_INVALID_ARG with nothing inflated.
 * Truth of a term on a row.  Take the row's cell for `field` by the type's rules.  IS_OK / NOT_OK look at the status
 *   alone.  A comparison on a cell that is not OK (MISSING, EMPTY, INVALID, RANGE) is FALSE, NE included.  On an OK cell
 *   INT64 compares as signed 64-bit integers and FLOAT64 by IEEE rules: -0.0 == 0.0, an OK cell that is NaN (the text
 *   "nan") is false for everything but NE, infinities order as usual.
 * Selected rows.  A row PASSES when all terms hold, with GZPX_WHERE_ANY when at least one does.  The selected set is the
 *   rows that pass, with GZPX_WHERE_INVERT the rows of [0, R) that do not -- so inversion selects rows whose cells are
 *   not OK: it negates the predicate, not each comparison.
 * Runs.  A RUN is a maximal interval of consecutive selected rows OF ONE RANGE: runs never join across two ranges, even
 *   if the ranges are adjacent or overlap ({0, 5}, {5, 9} all selected gives two runs).  Runs are written in row order
 *   as LINE ranges {ranges[r].begin + i0, ranges[r].begin + i1}; there are at most (R + n_ranges) / 2, so a table can be
 *   sized in advance.  With the one range {0, L} this is the table gzpx_select_lines_device writes with group 1.
 * Outputs.  *n_runs, *n_selected and *n_rows (= R) are always the totals; *n_not_ok (optional) is the number of cells of
 *   the distinct fields whose status is not OK, what gzpx_read_columns_device reports for the same columns.  d_runs ==
 *   NULL: count only, runs_cap is ignored.  d_runs (8-byte aligned) with more runs than runs_cap: the first runs_cap are
 *   written, nothing behind them is touched, and the call returns GZPX_ERR_INSUFFICIENT_SPACE.  n_ranges == 0, or all
 *   ranges empty: GZPX_OK, all counts 0.  On a failing member all counts are 0.  More than 0xFFFFFFF0 rows:
 *   GZPX_ERR_INVALID_ARG, behind the search; gzpx_where_lines_device decides by R itself, gzpx_where_lines_table_device,
 *   where R is known on the device only, by the bound the host knows: the bytes the ranges hold (every line holds at
 *   least one byte, so R is never above them), which also sizes its row bitmaps.  The result is the same bit for bit
 *   from run to run: bits set with atomicOr do not depend on order, scans place every run, the counts are integer sums.
 * gzpx_where_lines_device takes line_ranges as a HOST array, gzpx_where_lines_table_device as a DEVICE array (read
 *   where it lies, ordered behind hip_stream like d_in): the table gzpx_select_lines_device wrote, for one.
 * gzpx_dctx_last_where_ms: HIP-event durations of the last call's stages behind the search: [0] the field carries, the
 *   pieces' row counts and their scans, [1] the parse with the predicate, [2] the runs.  gzpx_dctx_last_lines_ms and
 *   gzpx_dctx_last_lines_members answer as for gzpx_read_columns_device. */
#define GZPX_WHERE_MAX_TERMS 32
#define GZPX_WHERE_LT 0
#define GZPX_WHERE_LE 1
#define GZPX_WHERE_EQ 2
#define GZPX_WHERE_NE 3
#define GZPX_WHERE_GE 4
#define GZPX_WHERE_GT 5
#define GZPX_WHERE_IS_OK 6   /* the cell's status is GZPX_CELL_OK; value must be 0 */
#define GZPX_WHERE_NOT_OK 7  /* it is not; value must be 0 */
#define GZPX_WHERE_ANY 1u    /* flags: a row passes when at least one term holds (default: when all hold) */
#define GZPX_WHERE_INVERT 2u /* flags: select the rows that do not pass */
typedef struct gzpx_where_term {
    uint64_t field; /* field number, as gzpx_column.field */
    uint32_t type;  /* GZPX_COL_INT64 / GZPX_COL_FLOAT64 */
    uint32_t op;    /* GZPX_WHERE_* */
    uint64_t value; /* the bits of an int64_t or of a double, by type */
} gzpx_where_term;
int gzpx_where_lines_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in, size_t in_len,
                            const gzpx_range *line_ranges, size_t n_ranges, unsigned field_delim, const gzpx_where_term *terms,
                            size_t n_terms, unsigned flags, gzpx_range *d_runs, size_t runs_cap, uint64_t *n_runs,
                            uint64_t *n_selected, uint64_t *n_rows, uint64_t *n_not_ok, size_t *bad_range, gzpx_check_info *info,
                            void *hip_stream);
int gzpx_where_lines_table_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in,
                                  size_t in_len, const gzpx_range *d_line_ranges, size_t n_ranges, unsigned field_delim,
                                  const gzpx_where_term *terms, size_t n_terms, unsigned flags, gzpx_range *d_runs,
                                  size_t runs_cap, uint64_t *n_runs, uint64_t *n_selected, uint64_t *n_rows, uint64_t *n_not_ok,
                                  size_t *bad_range, gzpx_check_info *info, void *hip_stream);
int gzpx_dctx_last_where_ms(gzpx_dctx *ctx, float ms[3]);
/* ---- selection of lines by the TEXT of their fields (gzpx_where.h): awk '$1 == "chr7" && $7 == "PASS" && $6 >= 30' --
 * the query a VCF is really asked -- with the constant anchored to its field: "PASS" inside an INFO string selects
 * nothing.  gzpx_where_lines_device and gzpx_where_lines_table_device are untouched: they still answer type 2 and ops 8
 * and 9 with GZPX_ERR_INVALID_ARG, and gzpx_read_columns_device still refuses GZPX_COL_TEXT.
 * Everything but the third cell type.  Lines, delimiters, line ranges and their validation, fields, the numeric cells,
 *   rows, runs ("never leave their range", at most (R + n_ranges) / 2 of them), selected rows, ANY and INVERT, the
 *   outputs, counts and capacity (count-only with d_runs == NULL, the first runs_cap runs and
 *   GZPX_ERR_INSUFFICIENT_SPACE), *bad_range, the context's lock, the slot, hip_stream, "returns synchronised", both
 *   inflate routes, the report of a failing member (all counts 0), the bound of 0xFFFFFFF0 rows and bit-reproducibility
 *   are gzpx_where_lines_device's, word for word; the four calls are one function.  gzpx_where_term is unchanged.  With
 *   numeric terms only the two calls give what gzpx_where_lines_device gives, from the same kernel.
 * The pool.  `text` is a HOST array of text_len <= GZPX_WHERE_TEXT_POOL_MAX constant bytes (NULL when text_len is 0).
 *   A TEXT term's `value` is offset | (uint64_t)len << 32: its constant is text[offset, offset + len), len <=
 *   GZPX_WHERE_TEXT_MAX, offset + len <= text_len.  Constants may overlap or share bytes; they may hold any byte.
 *   GZPX_WHERE_TEXT_MAX equals GZPX_CELL_MAX_BYTES for a reason: a constant of c bytes is decided by the field's first
 *   c + 1 bytes, and the walk keeps 65 bytes behind whatever byte opens a field in fast memory -- the guarantee the
 *   numeric cells already rest on.  The pool is 32 terms x 64 bytes.
 * Terms.  The rules of gzpx_where_lines_device, and: `type` may be GZPX_COL_TEXT; `op` may be GZPX_WHERE_PREFIX or
 *   GZPX_WHERE_NOT_PREFIX on a TEXT term (on a numeric type: GZPX_ERR_INVALID_ARG); IS_OK and NOT_OK take value 0 on
 *   every type; all terms of one field agree in their type.  len > 64, offset + len > text_len, text_len above the
 *   maximum, text == NULL with text_len > 0: GZPX_ERR_INVALID_ARG with nothing inflated and nothing written.
 * A TEXT cell.  Field f of a line with F fields is MISSING when f >= F.  Otherwise it is OK and its value is the field's
 *   bytes: of any length, 0 included (an empty field is the OK empty string), of any value ('\r' and NUL are ordinary
 *   bytes).  EMPTY, INVALID and RANGE do not occur.  *n_not_ok counts the MISSING cells of TEXT fields together with the
 *   numeric cells that are not OK.
 * Truth of a TEXT term.  IS_OK / NOT_OK look at the status alone.  Every other op is FALSE on a MISSING cell, NE and
 *   NOT_PREFIX included.  On an OK cell LT .. GT compare as unsigned bytes, memcmp over the common length and then the
 *   shorter first: Python's ordering of bytes, LC_ALL=C string comparison for NUL-free text.  PREFIX: the field begins
 *   with the constant (the empty constant: every OK cell).  NOT_PREFIX: it does not.
 * Mixing and chaining.  INT64, FLOAT64 and TEXT terms mix freely in one call under ALL, ANY and INVERT.  "CHROM in {a, b,
 *   c} AND QUAL >= 30" is two chained calls: three EQ terms on CHROM under GZPX_WHERE_ANY write a table, and
 *   gzpx_where_text_table_device (or gzpx_where_lines_table_device) takes it with the term on QUAL.
 * gzpx_dctx_last_where_ms, gzpx_dctx_last_lines_ms and gzpx_dctx_last_lines_members answer for these calls too. */
#define GZPX_COL_TEXT 2
#define GZPX_WHERE_PREFIX 8      /* TEXT only: the field begins with the constant */
#define GZPX_WHERE_NOT_PREFIX 9  /* TEXT only: it does not (false on a MISSING cell) */
#define GZPX_WHERE_TEXT_MAX 64   /* bytes of one constant; == GZPX_CELL_MAX_BYTES */
#define GZPX_WHERE_TEXT_POOL_MAX 2048 /* bytes of the pool: GZPX_WHERE_MAX_TERMS x GZPX_WHERE_TEXT_MAX */
int gzpx_where_text_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in, size_t in_len,
                           const gzpx_range *line_ranges, size_t n_ranges, unsigned field_delim, const gzpx_where_term *terms,
                           size_t n_terms, const void *text, size_t text_len, unsigned flags, gzpx_range *d_runs, size_t runs_cap,
                           uint64_t *n_runs, uint64_t *n_selected, uint64_t *n_rows, uint64_t *n_not_ok, size_t *bad_range,
                           gzpx_check_info *info, void *hip_stream);
int gzpx_where_text_table_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in,
                                 size_t in_len, const gzpx_range *d_line_ranges, size_t n_ranges, unsigned field_delim,
                                 const gzpx_where_term *terms, size_t n_terms, const void *text, size_t text_len, unsigned flags,
                                 gzpx_range *d_runs, size_t runs_cap, uint64_t *n_runs, uint64_t *n_selected, uint64_t *n_rows,
                                 uint64_t *n_not_ok, size_t *bad_range, gzpx_check_info *info, void *hip_stream);
/* ---- search for a SET of byte strings (gzpx_findset.h): grep -F -e A -e B -f list on a device-resident BGZF / Mgzip
 * stream -- the VCF rows of a handful of contigs, the FASTQ records that carry any of 96 barcodes, the log lines with
 * any of a list of error codes -- in ONE inflate and one pass over it, the hits of all patterns already merged by
 * position.  gzpx_find_device and gzpx_select_lines_device are untouched by it.
 * Definitions.  `plain`, n, `delim` and the LINE of a hit are exactly as for gzpx_find_device.  The set is a HOST
 *   array: pattern k is patterns[pattern_offsets[k] .. pattern_offsets[k + 1]), m_k bytes; there are n_patterns + 1
 *   offsets, non-decreasing; pattern_offsets[0] may be non-zero.  1 <= n_patterns <= GZPX_FINDSET_MAX_PATTERNS;
 *   1 <= m_k <= GZPX_FIND_MAX_PATTERN for every k; the sum of the lengths, pattern_offsets[n_patterns] -
 *   pattern_offsets[0], is at most GZPX_FINDSET_MAX_BYTES.  Bytes may have any value; patterns may be equal to,
 *   prefixes of, or contained in one another.  A violation of any of these rules (a NULL array, an empty or too long
 *   pattern, offsets that decrease, too many patterns or bytes) is GZPX_ERR_INVALID_ARG with nothing inflated and
 *   nothing written.
 *   A HIT is a pair (p, k) with plain[p .. p + m_k) == pattern k, 0 <= p <= n - m_k: gzpx_find_device's rule for every
 *   pattern.  Equal patterns each hit under their own id.  Hits are reported in ascending p and, at equal p, in
 *   ascending k -- the order a stable merge by position of the results of n_patterns calls of gzpx_find_device gives,
 *   so the result is reproducible bit for bit and d_ids can be cut by position.
 * gzpx_find_set_device.  d_positions (uint64), d_ids (uint32) and d_lines (uint64) are DEVICE arrays of hits_cap
 *   entries, each optional: entry r describes hit r.  All three NULL: count only, hits_cap is ignored, GZPX_OK.
 *   *n_hits is always the number of hits of all patterns in the whole stream.  When it exceeds hits_cap and an output
 *   array was given, the first hits_cap hits are written, nothing behind hits_cap entries is touched and the call
 *   returns GZPX_ERR_INSUFFICIENT_SPACE.  delim outside -1..255, or GZPX_FIND_NO_LINES with d_lines given:
 *   GZPX_ERR_INVALID_ARG.
 *   d_counts is an optional DEVICE array of n_patterns uint64: entry k is the number of hits of pattern k in the whole
 *   stream, whatever hits_cap is, in count-only calls too.  Whenever the call returns GZPX_OK or
 *   GZPX_ERR_INSUFFICIENT_SPACE the entries sum to *n_hits -- also when nothing is inflated, where all are zero.
 *   An index of 0 members, or every m_k > n: GZPX_OK, 0 hits, nothing inflated.  A set in which only some patterns are
 *   longer than the stream is searched for the others.
 *   Every member is inflated once per call, in the batches of gzpx_dctx_set_lines_batch.  Hits are owned by the batch
 *   in which they START: a batch that is not the last reports the starts p with p + M <= the end of what it holds,
 *   M = the longest pattern, and keeps its last M - 1 bytes in front of the next batch; the last batch -- also an empty
 *   one, such as the BGZF EOF member at a batch size of 1 -- reports every start that is left.  That keeps the order
 *   above across batches for patterns of different lengths.
 *   Index and context checks, the context's lock, the slot, hip_stream, "returns synchronised" and the report of a
 *   failing member are gzpx_find_device's: the inflate's error, info->block = the member's index in the stream,
 *   *n_hits = 0, and the output arrays, d_counts included, hold nothing of use.
 * gzpx_dctx_last_find_set_ms: HIP-event durations of the last gzpx_find_set_device, summed over its batches:
 *   [0] inflate, [1] counting pass + scan, [2] writing pass + carry.
 * gzpx_select_lines_set_device is gzpx_select_lines_device with "a hit" meaning a hit of any pattern of the set:
 *   definitions, `group`, GZPX_SELECT_INVERT, runs, runs_cap, errors and the report of a failing member are unchanged;
 *   *n_hits (optional) is the set's total as above; the rules of the set are those above, a violation is
 *   GZPX_ERR_INVALID_ARG.  Every m_k > n: nothing is inflated; 0 runs, with INVERT the one run {0, L}.  The table feeds
 *   gzpx_read_lines_table_device as it is; the timings are read with gzpx_dctx_last_select_ms. */
#define GZPX_FINDSET_MAX_PATTERNS 256
#define GZPX_FINDSET_MAX_BYTES 16384 /* sum of the patterns' lengths */
int gzpx_find_set_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const void *d_in, size_t in_len, const void *patterns,
                         const uint32_t *pattern_offsets, size_t n_patterns, int delim, uint64_t *d_positions, uint32_t *d_ids,
                         uint64_t *d_lines, size_t hits_cap, uint64_t *d_counts, uint64_t *n_hits, gzpx_check_info *info,
                         void *hip_stream);
int gzpx_dctx_last_find_set_ms(gzpx_dctx *ctx, float ms[3]);
int gzpx_select_lines_set_device(gzpx_dctx *ctx, const gzpx_dindex *ix, const gzpx_dlines *lines, const void *d_in,
                                 size_t in_len, const void *patterns, const uint32_t *pattern_offsets, size_t n_patterns,
                                 uint64_t group, unsigned flags, gzpx_range *d_runs, size_t runs_cap, uint64_t *n_runs,
                                 uint64_t *n_records, uint64_t *n_hits, gzpx_check_info *info, void *hip_stream);
/* ---- batches of independent DEFLATE members that this library did not write (gzpx_wrap.h): GZIP pages of Parquet,
 * zlib chunks of HDF5 / Zarr / ORC, PNG IDAT streams, members of a multi-member gzip file whose extents are known.
 * The counterpart of libdeflate_deflate_decompress / libdeflate_zlib_decompress / libdeflate_gzip_decompress for a
 * table of members in device memory: member i is d_in[in_offsets[i], in_offsets[i] + in_sizes[i]), wrapper included;
 * the members are inflated back to back by the kernels that inflate BGZF, each is checked with the checksum its
 * wrapper carries, and the call reports a status per member.
 *   Context: any gzpx_dctx, whatever format it was created for.  Runs under the context's lock, uses one slot,
 *   honours gzpx_dctx_set_route, returns synchronised; hip_stream as for gzpx_decompress_stream_device.
 *   Tables: d_in_offsets / d_in_sizes / d_out_sizes / d_out_offsets / d_results are DEVICE arrays; none crosses to the
 *   host in either direction (what comes back is one 32-byte record).  n == 0 is OK with 0 bytes.
 *   Placement: member i's slot is out_sizes[i] bytes (d_out_sizes == NULL, GZIP only: its trailer's ISIZE; 0 for a
 *   member whose table entry is invalid); the slots lie back to back in table order, d_out_offsets (n + 1 entries) is
 *   their exclusive prefix sum with [n] = *out_len, and no offset depends on whether a member failed.  A failed
 *   member's slot holds nothing of use.  Bytes of d_out at and behind min(*out_len, out_cap) are never written.
 *   Sizes: out_sizes[i] is the exact number of bytes member i inflates to (libdeflate without actual_out_nbytes_ret).
 *   With GZPX_BATCH_SHORT_OK it is a capacity, `produced` says how much came out, and the rest of the slot is zeroed;
 *   every member of such a call goes through the one-wave-per-member kernel (GZPX_INFLATE_WAVE), so it is NOT the
 *   fast case.  The flag is refused (GZPX_ERR_INVALID_ARG) with GZIP, whose trailer states the size, and with
 *   d_out_sizes == NULL.  GZIP with d_out_sizes: an ISIZE that differs from out_sizes[i] fails the member with
 *   GZPX_ERR_INVALID_CHECK (found = ISIZE, expected = out_sizes[i]); nothing is decoded for it.  A slot of 0 bytes is
 *   not decoded (as an ISIZE of 0 on the BGZF path); its check, taken over no bytes, still has to match.
 *   Status of one member, the first that applies:
 *     GZPX_ERR_INVALID_ARG         the table entry reaches outside [0, in_len), or the member is shorter than its
 *                                  wrapper (ZLIB 6 bytes, GZIP 18)
 *     GZPX_ERR_INVALID_HEADER      ZLIB: CM != 8, CINFO > 7, (CMF << 8 | FLG) % 31 != 0, or FDICT set (preset
 *                                  dictionaries are not supported).  GZIP: wrong magic, CM != 8, a reserved flag bit
 *                                  (5-7) set, or an FEXTRA / FNAME / FCOMMENT / FHCRC field that does not end in front
 *                                  of the member's last 8 bytes.  FTEXT is ignored; FHCRC's two bytes are skipped and
 *                                  not verified (libdeflate does not verify them either).
 *     GZPX_ERR_INSUFFICIENT_SPACE  the slot ends behind out_cap, or the stream has more output than the slot
 *     GZPX_ERR_BAD_DATA            the DEFLATE stream is invalid, or ends short of the slot without SHORT_OK
 *     GZPX_ERR_INVALID_CHECK       Adler-32 (ZLIB) or CRC-32 (GZIP) over the `produced` bytes differs from the trailer
 *   RAW has no check.
 *   Trailer: the member's last 4 (ZLIB) or 8 (GZIP) bytes AS THE TABLE GIVES THEM; payload bytes between the final
 *   block and the trailer are ignored, as on the BGZF path.  This is where the call is stricter than libdeflate about
 *   extents: libdeflate finds the trailer behind the final block and ignores what follows it, so a member has to be
 *   cut exactly here.
 *   Returns the status of the first failing member in table order with info->block = its index (found / expected
 *   for GZPX_ERR_INVALID_CHECK); every other member is still inflated and checked in full, d_results says which
 *   failed, *n_failed how many.  *out_len is the sum of the slots in every case.
 * gzpx_dctx_last_check_ms: HIP-event duration of the last batch call's check kernel (Adler-32 or the CRC-32 pass
 * behind the copy kernel's own; 0 for RAW bar the event pair); gzpx_dctx_last_kernel_ms gives the inflate kernels. */
#define GZPX_WRAP_RAW  0  /* RFC 1951: no header, no trailer, no check                          */
#define GZPX_WRAP_ZLIB 1  /* RFC 1950: CMF/FLG, Adler-32 (big endian) behind the stream         */
#define GZPX_WRAP_GZIP 2  /* RFC 1952: any legal header fields, CRC-32 + ISIZE behind the stream */
#define GZPX_BATCH_SHORT_OK 1u  /* flags: out_sizes are capacities, fewer bytes are accepted (RAW, ZLIB) */
typedef struct gzpx_member_result {
    uint32_t status;          /* GZPX_OK or the GZPX_ERR_* of this member            */
    uint32_t produced;        /* bytes inflated into the member's slot                */
    uint32_t found, expected; /* GZPX_ERR_INVALID_CHECK: the two values               */
} gzpx_member_result;
int gzpx_inflate_batch_device(gzpx_dctx *ctx, int wrap, unsigned flags,
                              const void *d_in, size_t in_len,
                              const uint64_t *d_in_offsets, const uint32_t *d_in_sizes, /* DEVICE arrays [n] */
                              const uint32_t *d_out_sizes,   /* DEVICE [n]; may be NULL for GZIP: the footers' ISIZE */
                              size_t n, void *d_out, size_t out_cap,
                              uint64_t *d_out_offsets,       /* DEVICE [n + 1], optional: written */
                              gzpx_member_result *d_results, /* DEVICE [n], optional: written */
                              size_t *out_len, size_t *n_failed, gzpx_check_info *info, void *hip_stream);
int gzpx_dctx_last_check_ms(gzpx_dctx *ctx, float *ms);
/* ---- the size query of such a batch: what every member inflates to and how long it is, for callers whose metadata
 * is missing or untrusted (raw DEFLATE containers, PNG IDAT, zlib chunks) and for tables whose entries are not cut
 * exactly.  The counterpart of libdeflate's *_decompress_ex with both actual_*_ret pointers, without an output buffer:
 * the inflate kernels run in a count-only form that decodes the Huffman symbols and adds up lengths -- no literal is
 * stored, no match source read, no byte of output written -- so the call reads the compressed bytes once and writes
 * 4 to 24 bytes per member.
 *   Context, lock, slot, hip_stream, "returns synchronised", n == 0 and n > 0xFFFFFFF0: as gzpx_inflate_batch_device.
 *   Honours gzpx_dctx_set_route; both routes give the same answers.  Every table is a DEVICE array and none crosses to
 *   the host; what comes back is one 32-byte record.  No output-sized scratch is allocated.
 *   Extents: in_sizes[i] is an UPPER BOUND here.  Member i begins at in_offsets[i] and ends no later than
 *   in_offsets[i] + in_sizes[i]; no byte behind that bound or behind in_len is read (bytes between the member's end
 *   and the bound may be).  A bound that leaves more than 0x1FFFFF00 bytes behind the wrapper's header is cut there.
 *   Per member, on success: out_sizes[i] = the exact number of bytes the DEFLATE stream inflates to; in_used[i] = the
 *   member's length as libdeflate reports it in actual_in_nbytes_ret: the wrapper's header, the stream through the
 *   byte that holds the last bit of the final block, and the trailer (RAW 0, ZLIB 4, GZIP 8 bytes);
 *   d_results[i] = {GZPX_OK, out_size, in_used, 0}.
 *   On failure out_sizes[i] = in_used[i] = 0 and d_results[i].status is the first that applies:
 *     GZPX_ERR_INVALID_ARG         the entry leaves [0, in_len) or is shorter than its wrapper (ZLIB 6, GZIP 18)
 *     GZPX_ERR_INVALID_HEADER      the ZLIB / GZIP header rules of gzpx_inflate_batch_device, FDICT included (a GZIP
 *                                  header field has to end in front of the ENTRY's last 8 bytes)
 *     GZPX_ERR_INSUFFICIENT_SPACE  the stream has more output than max_out_size (0: 0xFFFFFFFF): the guard against a
 *                                  decompression bomb -- counting stops at the symbol that crosses the cap
 *     GZPX_ERR_BAD_DATA            the stream is invalid by libdeflate's rules (a match that reaches in front of the
 *                                  member's first byte included: the running count decides, no window is needed), or
 *                                  the stream or its trailer does not end inside the entry
 *   Checks: none.  No Adler-32 / CRC-32 is verified and ISIZE is not read -- there are no bytes to check; the inflate
 *   call that follows verifies them.
 *   Returns the first failing member's status with info->block = its index (found = expected = 0); *n_failed = how
 *   many failed; *total_out = the sum of out_sizes, i.e. of the good members' sizes.
 *   gzpx_dctx_last_inflate_ms (and _stage_ms: [0] the count-only k_inflate_seg, [1] the hand-backs) answer for this
 *   call as for the batch call; gzpx_dctx_last_redo_count likewise.
 *   Intended use: this call, then allocate *total_out bytes, then gzpx_inflate_batch_device with d_out_sizes as this
 *   call wrote them -- and, if the table's entries were loose, with d_in_used as its d_in_sizes.  The second call is
 *   unchanged: the fast route, Adler-32 / CRC-32 verified.  A member that failed here has a slot of 0 bytes there and
 *   is not decoded; for RAW, which has no check, the second call then reports nothing about it (ZLIB / GZIP members
 *   with in_used = 0 fail there as GZPX_ERR_INVALID_ARG): this call's results are where its failure is recorded. */
int gzpx_inflate_batch_sizes_device(gzpx_dctx *ctx, int wrap,
                                    const void *d_in, size_t in_len,
                                    const uint64_t *d_in_offsets, const uint32_t *d_in_sizes, size_t n, /* DEVICE [n] */
                                    uint32_t max_out_size,         /* cap per member; 0 = 0xFFFFFFFF */
                                    uint32_t *d_out_sizes,         /* DEVICE [n], written */
                                    uint32_t *d_in_used,           /* DEVICE [n], optional, written */
                                    gzpx_member_result *d_results, /* DEVICE [n], optional, written */
                                    uint64_t *total_out, size_t *n_failed, gzpx_check_info *info, void *hip_stream);
/* ---- checksums of a table of device-resident buffers: CRC-32, CRC-32C and Adler-32 of n entries of one input, for the
 * callers whose checksum lies outside the DEFLATE stream -- ZIP entries (CRC-32 in the directory), PNG chunks, Parquet
 * pages (CRC-32 in the page header), Zarr's crc32c codec, and gzp's whole-stream checks (src/check.rs:85-164) -- and so
 * for what gzpx_inflate_batch_device leaves in device memory from a GZPX_WRAP_RAW batch.  The counterpart of zlib's
 * crc32(seed, buf, len) / adler32(seed, buf, len) (libdeflate_crc32 / libdeflate_adler32) for a table of buffers in
 * device memory: tables in, sums out, and nothing crosses to the host but one 32-byte record.
 *   Context: any gzpx_dctx, whatever format it was created for.  Runs under the context's lock, returns synchronised;
 *   hip_stream as for gzpx_inflate_batch_device, GZPX_STREAM_NONE included.  gzpx_dctx_last_check_ms answers for this
 *   call too: the HIP-event duration of its kernels.
 *   Entries: with d_sizes, entry i is d_in[off[i], off[i] + size[i]) -- an (in_offsets, in_sizes) pair.  With
 *   d_sizes == NULL (the span form) d_offsets has n + 1 entries and entry i is d_in[off[i], off[i + 1]): the
 *   d_out_offsets array gzpx_inflate_batch_device writes, taken as it is; such an entry may be longer than 4 GiB.
 *   Entries may overlap, repeat, nest, be empty and come in any order.
 *   Value: sums[i] = zlib's crc32(seed, buf, len) (GZPX_CHECK_CRC32), adler32(seed, buf, len) (GZPX_CHECK_ADLER32), or
 *   the same CRC with the Castagnoli polynomial (GZPX_CHECK_CRC32C: iSCSI / RFC 3720, NOT the masked form of Snappy
 *   frames).  seed = d_seeds[i]: the sum of what lies in front, for a buffer that is hashed in pieces; without d_seeds
 *   0 for both CRCs and 1 for Adler-32.  An empty entry yields its seed.
 *   Verify: with d_expected, a valid entry whose sum differs from d_expected[i] is a failed entry.
 *   Status of one entry, the first that applies:
 *     GZPX_ERR_INVALID_ARG    the entry leaves [0, in_len), or in the span form off[i + 1] < off[i]; sums[i] = 0 and no
 *                             byte is read for it
 *     GZPX_ERR_INVALID_CHECK  the sum differs from d_expected[i]
 *   d_results[i] = {status, the entry's length saturated at 0xFFFFFFFF (0 for an invalid entry), found = sums[i],
 *   expected = d_expected[i], or 0 without d_expected}.
 *   Returns the status of the first failing entry in table order with info->block = its index and found / expected
 *   filled in; every other entry is still computed, *n_failed says how many failed.
 *   GZPX_ERR_INVALID_ARG for the call, with nothing launched: a null ctx, d_in (with in_len > 0), d_offsets,
 *   n_failed or info; an unknown kind; neither d_sums nor d_expected; n > 0xFFFFFFF0.  n == 0 is OK.
 *   Memory: scratch is 12 bytes per entry and 8 bytes per workgroup launched, kept by the context; nothing is sized by
 *   in_len or by the sum of the sizes (overlapping entries make that sum unbounded); no table crosses to the host, and
 *   there is no host round trip between the kernels.
 *   Reads: the bytes of valid entries and the aligned 4-byte words that hold an entry's first and last byte -- never a
 *   byte in front of the aligned 16-byte word that holds d_in[0] or behind the one that holds d_in[in_len - 1].
 * gzpx_dctx_set_checksum_width: diagnostics -- the number of persistent workgroups of the call's tile kernel (0, the
 * default: six per compute unit; at most 65536).  The sums do not depend on it; tests move the workgroups' edges
 * with it. */
#define GZPX_CHECK_CRC32   0  /* zlib / gzip crc32: reflected 0xEDB88320, init and xor-out all ones          */
#define GZPX_CHECK_ADLER32 1  /* zlib adler32                                                                 */
#define GZPX_CHECK_CRC32C  2  /* Castagnoli, reflected 0x82F63B78, init and xor-out all ones, NOT Snappy-masked */
int gzpx_checksum_batch_device(gzpx_dctx *ctx, int kind,
                               const void *d_in, size_t in_len,
                               const uint64_t *d_offsets,     /* DEVICE [n], or [n + 1] when d_sizes == NULL */
                               const uint32_t *d_sizes,       /* DEVICE [n], or NULL: the span form          */
                               size_t n,
                               const uint32_t *d_seeds,       /* DEVICE [n], optional: running values         */
                               const uint32_t *d_expected,    /* DEVICE [n], optional: verify                 */
                               uint32_t *d_sums,              /* DEVICE [n], optional if d_expected is given  */
                               gzpx_member_result *d_results, /* DEVICE [n], optional                         */
                               size_t *n_failed, gzpx_check_info *info, void *hip_stream);
int gzpx_dctx_set_checksum_width(gzpx_dctx *ctx, unsigned workgroups);
typedef struct gzpx_decompressor gzpx_decompressor;
gzpx_decompressor *gzpx_alloc_decompressor(void);
/* 0 = ok (short output allowed, *actual = bytes produced), GZPX_ERR_BAD_DATA, GZPX_ERR_INSUFFICIENT_SPACE */
int gzpx_deflate_decompress(gzpx_decompressor *d, const void *in, size_t n, void *out, size_t cap, size_t *actual);
void gzpx_free_decompressor(gzpx_decompressor *d);

/* ParDecompress twin: `Read` over a block stream (C++ class gzp::ParDecompress, gzpx_par.hpp) */
typedef struct gzpx_pard gzpx_pard;
typedef long (*gzpx_read_fn)(void *user, uint8_t *buf, size_t cap); /* bytes read, 0 = EOF, < 0 = error */
int gzpx_pard_create(int format, int device, size_t batch_bytes, gzpx_read_fn read_fn, void *user,
                     gzpx_pard **out);
int gzpx_pard_read(gzpx_pard *p, uint8_t *buf, size_t n, size_t *got);
/* std::io::BufRead's fill_buf / consume for the same stream: *ptr = the inflated bytes where they lie (the current slab's
 * page-locked buffer, valid until the next fill_buf / read that follows a consume of all of them), *len = how many
 * (0 at the end of the stream).  gzp's ParDecompress is `Read` only (src/par/decompress.rs:241-352); a binding that
 * wants no copy between the slab and its own buffer implements BufRead over these two. */
int gzpx_pard_fill_buf(gzpx_pard *p, const uint8_t **ptr, size_t *len);
int gzpx_pard_consume(gzpx_pard *p, size_t n);
void gzpx_pard_destroy(gzpx_pard *p);
const char *gzpx_pard_last_error(const gzpx_pard *p);

/* Page-locked host memory for slab staging.  A caller that fills its slabs in such buffers (the
 * twin does) turns the library's copies to and from the device into DMA transfers that overlap
 * with the other lane's kernels: 12 GiB/s host to host instead of 6 with pageable memory. */
void *gzpx_host_alloc(size_t bytes);
void gzpx_host_free(void *p);

/* ---- workload support: the synthetic FASTQ stream of BASELINE configs[3] (32 GiB sharded over 8
 * GPUs), generated in HBM.  Fills d_out[0..n) with bytes [stream_offset, stream_offset + n) of the
 * stream with this seed (oracle/synth_fastq.c states the stream on the CPU). ---- */
int gzpx_synth_fastq_device(void *d_out, uint64_t stream_offset, uint64_t n, uint64_t seed, void *hip_stream);
/* the printable-ASCII noise of BASELINE configs[2] (byte i = 0x20 + (splitmix64 output i >> 56) % 95) */
int gzpx_synth_ascii_device(void *d_out, uint64_t stream_offset, uint64_t n, uint64_t seed, void *hip_stream);

/* ---- measurement hooks (HIP events on the launching stream; bench.py roofline leg) ---- */
#define GZPX_N_STAGES 9
/* stage order: init_meta, candidates, match, parse, hist, huffman, crc32, scan, emit */
/* on: 0 off, 1 HIP events around every stage, 2 around the dominant stage (2: match) only -- two markers in the
 * stream instead of thirteen, for a timed region that wants the kernel's duration without paying for the rest */
int gzpx_ctx_set_profiling(gzpx_ctx *ctx, int on);
int gzpx_ctx_last_stage_ms(const gzpx_ctx *ctx, float ms[GZPX_N_STAGES]);
const char *gzpx_stage_name(int stage);
/* the kernel(s) behind a stage for THIS context: stage 2 is k_mparse (level 1, blocks <= 64 KiB: match
 * on demand; k_match / k_parse then only see the blocks it hands back), k_match (level 1, larger
 * blocks), k_match_hc + k_parse_hc (levels 2-4) or k_match_hc + k_parse_lazy (levels 5-9) */
const char *gzpx_ctx_stage_kernel(const gzpx_ctx *ctx, int stage);

/* ---- test hooks: intermediate products of the last slab call (device -> host copies) ---- */
int gzpx_debug_tokens(gzpx_ctx *ctx, size_t block, uint32_t *tokens, size_t max_tokens,
                      size_t *n_tokens, uint32_t *sub_first_token, size_t *n_sub);

/* Diagnostics switches (0 in production): bit 0 = k_candidates takes its order-independent
 * fallback (cand_block_safe) on every block instead of the atomic-chain form; bit 1 = level 1 through the
 * dense k_match / k_parse pair instead of the match-on-demand kernel k_mparse; bit 2 = k_mparse
 * hands every block back to the dense pair (exercises the redo list); bit 3 = k_mparse's walks search at
 * every position instead of stepping over the runs that have no hash candidate (same stream; A/B timing);
 * bit 7 = k_candidates takes every iteration through its clamped body instead of the interior one (same
 * stream; A/B timing). */
int gzpx_debug_set_flags(gzpx_ctx *ctx, uint32_t flags);
/* Level 1: how many blocks of the last batch k_mparse handed back to the dense kernels. */
int gzpx_debug_redo_count(gzpx_ctx *ctx, uint32_t *count);
/* Snap contexts: switch k_snap_chunk's phase clocks on (1) / off (0); sums[] = the clocks of the last batch of the
 * last launch summed over its chunks: [0] cycles of k_snap_chunk, [1] CRC-32C, [2] literal scans, [3] match
 * extension and the table updates between copies, [4] literal and copy emission, [5] scan steps (64 probes each),
 * [6] copies, [7] bytes.  Stage times of a Snap context: slot 2 = k_snap_chunk, 7 = k_snap_frame + k_scan,
 * 8 = k_snap_emit (gzpx_ctx_stage_kernel). */
int gzpx_debug_snap(gzpx_ctx *ctx, int enable, uint64_t sums[8]);

/* HIP-event duration of the inflate kernels (k_inflate_seg + k_lzcopy + k_inflate over the redo list, or
 * k_inflate alone) in the last decompress launch of this context */
int gzpx_dctx_last_inflate_ms(gzpx_dctx *ctx, float *ms);
/* GZPX_INFLATE_SEG: the same split in two, ms[0] = k_inflate_seg (Huffman decode), ms[1] = k_lzcopy + k_inflate over the
 * hand-backs (zeros on the other route) */
int gzpx_dctx_last_inflate_stage_ms(gzpx_dctx *ctx, float ms[2]);
/* Which kernels inflate (decode_block, src/par/decompress.rs:162-186): GZPX_INFLATE_SEG (default) = the decode /
 * LZ-copy pair, members they cannot take handed to k_inflate; GZPX_INFLATE_WAVE = k_inflate (one wave per member,
 * window in HBM) for every member.  Same bytes, same error classes either way. */
#define GZPX_INFLATE_SEG 0
#define GZPX_INFLATE_WAVE 1
int gzpx_dctx_set_route(gzpx_dctx *ctx, int route);
/* How many members of the last launch the decode / copy pair handed to k_inflate (diagnostics). */
int gzpx_dctx_last_redo_count(gzpx_dctx *ctx, uint32_t *count);
/* inflate: switch the instrumented kernels on (1, or 2 on the GZPX_INFLATE_SEG route for k_lzcopy's clocks instead
 * of k_inflate_seg's) / off (0); sums[] = per-member counters of the last instrumented launch summed over its members.
 * enable = 1, GZPX_INFLATE_SEG: [0] cycles of k_inflate_seg, [1] headers + tables, [2] pass 1, [3] pass 2, [4] pass 3,
 * [5] spans, [6] pass-2 iterations, [7] symbol steps of passes 1 and 3.  enable = 2: [0] cycles of k_lzcopy, [1] tile
 * staged in, [2] chunk set-up, [3] polling, [4] CRC + tile written out, [5] polling iterations, [6] of them without
 * progress, [7] matches.  GZPX_INFLATE_WAVE: [0] cycles, [1] headers + tables, [2] round set-up, [3] stores + copies,
 * [4] rounds, [5] literals, [6] matches, [7] flushes */
int gzpx_debug_inflate(gzpx_dctx *ctx, int enable, uint64_t sums[8]);
/* Why the decode / copy pair handed members of the last launch to k_inflate: reasons[b] for members b < n of it,
 * GZPX_HANDBACK_NONE for a member the pair decoded (or never looked at: ISIZE 0) and for every member when the last
 * launch was not an instrumented one on the GZPX_INFLATE_SEG route.  Only the instrumented kernels record a reason
 * (gzpx_debug_inflate's enable 1: k_inflate_seg's, and GZPX_HANDBACK_LZCOPY for a member on the list that k_inflate_seg
 * did not put there; enable 2: k_lzcopy's alone); the production kernels carry none of this.  Where several lanes of a
 * span trip in pass 3, the reason is the first such lane's: the earliest on the true path. */
#define GZPX_HANDBACK_NONE 0
#define GZPX_HANDBACK_HEADER 1          /* block header refused: type 3, a code's shape, the header's runs, no end-of-block code, stored LEN / NLEN, payload ends inside it */
#define GZPX_HANDBACK_STORED 2          /* a stored block reaches past the payload or past ISIZE */
#define GZPX_HANDBACK_NO_EOB 3          /* the payload ends before the block does */
#define GZPX_HANDBACK_RESYNC 4          /* the lanes did not re-synchronise within the iteration limit of pass 2 */
#define GZPX_HANDBACK_SPAN_SYMBOL 5     /* the span's true path stops at something that is no end-of-block code */
#define GZPX_HANDBACK_SPAN_OVERRUN 6    /* the span's output overruns ISIZE, or its exit lies behind the payload */
#define GZPX_HANDBACK_DISTANCE 7        /* pass 3: a distance reaches in front of the output's start */
#define GZPX_HANDBACK_OFFSET_SYMBOL 8   /* pass 3: an invalid offset codeword */
#define GZPX_HANDBACK_CODEWORD 9        /* pass 3: an invalid litlen codeword (litlen symbols 286 and 287 among them) */
#define GZPX_HANDBACK_COUNT_MISMATCH 10 /* pass 3 of the count-only form disagrees with pass 2 */
#define GZPX_HANDBACK_FINAL 11          /* behind the final block: fewer bytes than ISIZE, or the stream ends behind the payload */
#define GZPX_HANDBACK_LZCOPY 12         /* k_lzcopy gave up */
int gzpx_debug_inflate_handback(gzpx_dctx *ctx, uint32_t *reasons, size_t n);

const char *gzpx_strerror(int code);
const char *gzpx_device_name(const gzpx_ctx *ctx);
const char *gzpx_version(void);
/* Identifies the sources this library was built from (gzp_amd/build.py: source_id()); "unknown" for builds made
 * another way.  profiles/pmc_traffic.json carries the id of the build its counters were collected with. */
const char *gzpx_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* GZPX_H */
