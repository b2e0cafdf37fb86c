"""The Snap format through the product sources on the CPU emulator: raw vectors (one-chunk buffers) and framed
vectors through gzpx_compress_slab in all three modes, gzpx_encode_block and the twin, against
tests/golden/snap_vectors.json; and the refusals of the C ABI.  (Sizes kept small: the emulator runs every lane.)"""
import ctypes

import pytest

import snap_cases as sc
from gzp_amd import _native, par

G = sc.golden()
GEN = sc.generator()
RAW = [v for v in G["raw"] if v["spec"][1] <= 4096 or v["spec"][0] in ("echo", "literal", "period")]
FRAMED = [v for v in G["framed"] if v["spec"][1] <= 140000 and v["spec"][3] <= 131072]


def test_raw_vectors(emu_lib):
    sc.run_raw(emu_lib, RAW, GEN)


def test_framed_vectors_every_slab_mode(emu_lib):
    sc.run_framed(emu_lib, FRAMED, GEN)


def test_encode_block(emu_lib):
    sc.run_encode_block(emu_lib, FRAMED[::3], GEN)


def test_twin_ragged_writes(emu_lib):
    sc.run_twin(emu_lib, [v for v in FRAMED if v["spec"][1] > 0][::4], GEN)


def test_twin_flush(emu_lib):
    raw = GEN.load_snappy() or GEN.snappy_raw
    sc.run_twin_flush(emu_lib, GEN, raw, [("text", 100000, 3, 32768), ("mixed", 70000, 4, 65537)])


def _create(lib, **kw):
    cfg = _native.GzpxConfig()
    lib.L.gzpx_config_default(ctypes.byref(cfg), _native.FORMAT_SNAP)
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    rc = lib.L.gzpx_ctx_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc == _native.OK:
        lib.L.gzpx_ctx_destroy(h)
    return rc, cfg


def test_config_and_refusals(emu_lib):
    L = emu_lib.L
    rc, cfg = _create(emu_lib, max_slab_bytes=1 << 20)
    assert rc == _native.OK and cfg.buffer_size == 131072
    # the level and compat are ignored (src/snap.rs:53-59, 91)
    for lvl in (-1, 0, 13, 99):
        assert _create(emu_lib, level=lvl, compat=7, max_slab_bytes=1 << 20)[0] == _native.OK
    assert _create(emu_lib, buffer_size=32767)[0] == _native.ERR_BUFFER_SIZE
    assert _create(emu_lib, buffer_size=(64 << 20) + 1)[0] == _native.ERR_UNSUPPORTED
    # multi-device, ParDecompress and the block index refuse Snap
    cfg = _native.GzpxConfig()
    L.gzpx_config_default(ctypes.byref(cfg), _native.FORMAT_SNAP)
    devs = (ctypes.c_int * 1)(0)
    h = ctypes.c_void_p()
    assert L.gzpx_multi_create(ctypes.byref(cfg), devs, 1, ctypes.byref(h)) == _native.ERR_UNSUPPORTED
    assert L.gzpx_dctx_create(0, _native.FORMAT_SNAP, ctypes.byref(h)) == _native.ERR_INVALID_ARG
    with pytest.raises(_native.GzpxError):
        par.ParDecompressBuilder(par.Snap, lib=emu_lib)
    sink = sc._Sink()
    w = par.ParCompressBuilder(par.Snap, lib=emu_lib).buffer_size(65536).num_threads(1).batch_blocks(2).from_writer(sink)
    w.write(b"abc" * 1000)
    w.finish()
    with pytest.raises(_native.GzpxError) as e:
        w.index()
    assert e.value.code == _native.ERR_INVALID_ARG
    assert sc.decode_frames(sink.value())[0] == b"abc" * 1000
    # a Snap context has no deflate debug state; its stages are named after its own kernels
    with _native.Context(format=_native.FORMAT_SNAP, buffer_size=65536, lib=emu_lib, max_slab_bytes=65536) as c:
        c.compress_slab(b"x" * 100, True)
        with pytest.raises(_native.GzpxError):
            c.debug_tokens(0)
        with pytest.raises(_native.GzpxError):
            c.debug_redo_count()
        c.set_profiling(True)
        c.compress_slab(b"y" * 70000, True)
        assert sorted(c.last_stage_ms()) == ["k_snap_chunk", "k_snap_emit", "k_snap_frame+k_scan"]
        c.debug_snap(True)
        got = c.compress_slab(GEN.make_input(["text", 70000, 3]), True)
        sums = c.debug_snap(False)
        # bytes, copies, scan steps of the last batch (one 64 KiB buffer per batch here: the last holds 4,464 bytes)
        assert sums[7] == 70000 - 65536 and sums[6] > 0 and sums[5] > 0
        assert sc.decode_frames(got)[0] == GEN.make_input(["text", 70000, 3]).tobytes()
    # a Snap context refuses the debug hooks of the other formats, and they refuse it
    with _native.Context(format=_native.FORMAT_BGZF, level=1, lib=emu_lib, max_slab_bytes=65280) as c:
        with pytest.raises(_native.GzpxError):
            c.debug_snap(True)
