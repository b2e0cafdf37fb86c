// gzpx_check.hip -- the checks of gzp's streaming formats as helpers behind the C ABI (src/check.rs:85-164):
// Adler32::update (zlib's adler32 over a buffer) on the device, Adler32::combine / Crc32::combine as plain arithmetic
// (gzpx_api.cpp; Crc32::update is gzpx_crc32).  The checks are pinned on Python's zlib module (tests/test_checks.py,
// tests/test_gpu_checks.py).
//
// The Adler-32 kernel lives in gzpx_wrap.h since the zlib wrapper of gzpx_inflate_batch_device needs the same sum over
// every inflated member: adler_workgroup is the one device routine, k_adler32_tiles (one (s1, s2, n) per 64 KiB tile,
// combined on the host) and k_dadler32 (a workgroup per member) are its two callers, and launch_adler32 is with the
// other launchers in gzpx_kernels.hip.  Nothing is left to compile here.
