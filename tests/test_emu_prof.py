"""tests/prof_cases.py through the product sources on the CPU emulator, and what the GPU run cannot see: how many
event records each call puts on its streams.  Every record is a marker a stream has to process (the comment above
ProfPairs in gzpx_api.cpp prices them), so a host-side change that adds or drops one is a change of the work
submitted, whatever the bytes say.  Emulated events may read 0 ms: the times are only checked for where they land."""
import ctypes

import pytest

import prof_cases as pc

# hipEventRecord calls per call, in the order prof_cases.run makes them: compress_slab in modes 0, 1, 2, then (one
# batch) submit + wait in mode 2.  Not worked out by hand: counted by `python tests/prof_cases.py` on the commit before
# the encode side of gzpx_api.cpp was reorganised (c3d345d plus the counter in tests/emu/emu_runtime.cpp alone).  The
# emulator is deterministic, so the numbers carry no margin.
EVENT_RECORDS = {
    ("bgzf1", "one_batch"): [5, 16, 7, 7],
    ("bgzf1", "two_batches"): [7, 29, 11],
    ("bgzf3", "one_batch"): [5, 15, 7, 7],
    ("bgzf3", "two_batches"): [7, 27, 11],
    ("snap", "one_batch"): [3, 7, 5, 5],
    ("snap", "two_batches"): [3, 11, 7],
}


@pytest.mark.parametrize("slab", list(pc.SLABS))
@pytest.mark.parametrize("kind", pc.KINDS)
def test_profiling_modes(emu_lib, oracle, kind, slab):
    emu_lib.L.emu_event_record_count.restype = ctypes.c_long
    assert pc.run(emu_lib, oracle, kind, slab, False, emu_lib.L.emu_event_record_count) == EVENT_RECORDS[kind, slab]
