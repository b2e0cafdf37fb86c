"""The profiling modes of a compress context (gzpx_ctx_set_profiling: 0 off, 1 HIP events around every stage, 2 around
the dominant stage only), shared by the emulator and the GPU run: what a mode measures never changes the stream, the
stages that read a time are the ones the context's kernels stand behind, and mode 2 reads stage 2 alone -- from the
per-batch wait of a multi-batch slab, and from the job's own pair of events when a one-batch slab is waited for.

One slab of text, cut so that it is one batch or two; three contexts.  The streams are checked as the other tests check
them: BGZF against the oracle, Snap decoded back to the input."""
import ctypes
import functools

import numpy as np

import snap_cases
from gzp_amd import _native, synth

BS = 65280
N = 3 * BS + 100  # four blocks, the last one short
KINDS = ("bgzf1", "bgzf3", "snap")
SLABS = {"one_batch": N, "two_batches": 2 * BS}  # max_slab_bytes: the whole slab / two blocks of it (synchronous measurement)
MATCH = 2  # the dominant stage, the only one mode 2 reads

# The stages gzpx_ctx_stage_kernel names for the context (include/gzpx.h: the stage order, stage 3 is "-" above level
# 1, a Snap context has 2, 7 and 8).  Stage 0, k_init_meta, keeps its name at every level but is a launch of its own
# at level 0 only: from level 1 on the first k_candidates launch cuts the slab itself (gzpx_kernels.hip, above
# k_init_meta), so it reads exactly 0 there and is left out of LAUNCHED, the stages that must read a time on the GPU.
NAMED = {"bgzf1": {0, 1, 2, 3, 4, 5, 6, 7, 8}, "bgzf3": {0, 1, 2, 4, 5, 6, 7, 8}, "snap": {2, 7, 8}}
LAUNCHED = {k: v - {0} for k, v in NAMED.items()}


@functools.lru_cache(maxsize=None)
def data():
    a = synth.make("text", N, 7)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _want(oracle, level):
    return oracle.compress_stream(data(), oracle.FMT_BGZF, level, oracle.COMPAT_1_24, BS)


def context(lib, kind, slab):
    if kind == "snap":
        return _native.Context(format=_native.FORMAT_SNAP, buffer_size=BS, lib=lib, max_slab_bytes=SLABS[slab])
    return _native.Context(format=_native.FORMAT_BGZF, level=int(kind[-1]), buffer_size=BS, lib=lib,
                           max_slab_bytes=SLABS[slab])


def stage_ms(c):
    ms = (ctypes.c_float * _native.N_STAGES)()
    c.lib.check(c.lib.L.gzpx_ctx_last_stage_ms(c.h, ms))
    return [float(v) for v in ms]


def named_stages(c):
    return {i for i in range(_native.N_STAGES) if c.lib.L.gzpx_ctx_stage_kernel(c.h, i) != b"-"}


def check_stream(oracle, kind, got, what):
    if kind == "snap":
        assert snap_cases.decode_frames(got)[0] == data().tobytes(), what
    else:
        assert got == _want(oracle, int(kind[-1])), what


def submit_wait(c):
    """The slab through submit + wait: (stream, stage times between the two calls, stage times after the wait)."""
    a = data()
    out = np.empty(c.slab_bound(a.size), dtype=np.uint8)
    t = c.submit(a.ctypes.data, a.size, out.ctypes.data, out.size, _native.SLAB_LAST)
    assert t is not None
    between = stage_ms(c)
    got, _ = c.wait(t)
    return out[:got].tobytes(), between, stage_ms(c)


def run(lib, oracle, kind, slab, gpu, records=None):
    """Modes 0, 1, 2 (and, one batch: mode 2 through submit + wait) on one context.  `records`: a function that reads
    the emulator's event-record counter; the records of every call are returned, in that order."""
    counted = []
    count = records or (lambda: 0)
    with context(lib, kind, slab) as c:
        assert named_stages(c) == NAMED[kind]
        streams = {}
        for mode in (0, 1, 2):
            c.set_profiling(mode)
            n0 = count()
            streams[mode] = c.compress_slab(data(), True)
            counted.append(count() - n0)
            ms = stage_ms(c)
            what = "%s, %s, mode %d: %s" % (kind, slab, mode, ms)
            assert streams[mode] == streams[0], what
            on = set() if mode == 0 else NAMED[kind] if mode == 1 else {MATCH}
            assert all(ms[i] == 0.0 for i in range(_native.N_STAGES) if i not in on), what
            assert all(v >= 0.0 for v in ms), what
            if gpu and mode == 1:
                assert all(ms[i] > 0.0 for i in LAUNCHED[kind]) and ms[0] == 0.0, what
            if gpu and mode == 2:
                assert ms[MATCH] > 0.0, what
        check_stream(oracle, kind, streams[0], "%s, %s" % (kind, slab))
        if slab == "one_batch":  # mode 2 is still set: the job carries its own pair of events, read by the wait
            n0 = count()
            got, between, ms = submit_wait(c)
            counted.append(count() - n0)
            what = "%s, submit + wait in mode 2: %s / %s" % (kind, between, ms)
            assert got == streams[0], what
            assert all(v == 0.0 for v in between), what  # (nothing of the job before: submit cleared it)
            assert all(ms[i] == 0.0 for i in range(_native.N_STAGES) if i != MATCH) and ms[MATCH] >= 0.0, what
            if gpu:
                assert ms[MATCH] > 0.0, what
    return counted


if __name__ == "__main__":  # the counting helper: python tests/prof_cases.py prints the emulator's table of event records
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import build_emu
    from oracle import oracle as o
    o.build()
    lib = _native.GzpxLib(build_emu.build())
    lib.L.emu_event_record_count.restype = ctypes.c_long
    for kind in KINDS:
        for slab in SLABS:
            print('    ("%s", "%s"): %s,' % (kind, slab, run(lib, o, kind, slab, False, lib.L.emu_event_record_count)))
