"""Inflate conformance through the emulated kernels (tests/inflate_cases.py): libdeflate's recorded verdict on every
crafted stream, on Decompressor.deflate_decompress and on both DContext routes; the record itself; and the hostile
encoder's differential run at a small seed count.  No GPU."""
import os
import sys

import numpy as np
import pytest

import inflate_cases as ic


@pytest.fixture(scope="module")
def verdicts():
    return ic.load_verdicts()


def test_record_matches_the_crafted_streams(verdicts):
    ic.check_record_matches_streams(verdicts)


def test_record_regenerates_from_the_boxs_libdeflate():
    """The committed record is what the recorder writes today, byte for byte."""
    ld = ic.box_libdeflate()
    if ld is None:
        pytest.skip("no libdeflate.so.0 on this box")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_inflate_verdicts
    with open(ic.VERDICTS) as f:
        assert f.read() == make_inflate_verdicts.render(ic.record(ld))


def test_bit_writer_speed_and_paths():
    """The two ways into the bit writer agree, and a 64 KiB member builds in well under a second."""
    import time
    import deflate_craft as dc
    rng = np.random.default_rng(1)
    v = rng.integers(0, 1 << 15, 5000)
    n = rng.integers(0, 16, 5000)
    v &= (1 << n) - 1
    a, b = dc.BitWriter(), dc.BitWriter()
    for w in (a, b):
        w.bits(5, 3)
    for x, k in zip(v.tolist(), n.tolist()):
        a.bits(x, k)
    b.fields(v[:1234], n[:1234])
    b.fields(v[1234:], n[1234:])
    assert a.getvalue() == b.getvalue() and a.bitpos == b.bitpos
    from gzp_amd import synth
    data = synth.make("text", 65280, 1).tobytes()
    took = []
    for _ in range(2):  # (the better of two: a busy box must not fail this)
        t0 = time.perf_counter()
        dc.encode(data, np.random.default_rng(2), max_payload=ic.BGZF_MAX_PAYLOAD)
        took.append(time.perf_counter() - t0)
    assert min(took) < 1.0, took


@pytest.mark.parametrize("name", ic.case_names())
def test_verdict_decompressor(emu_lib, verdicts, name):
    ic.check_decompressor(emu_lib, verdicts, name)


@pytest.mark.parametrize("route", sorted(ic.ROUTES))
@pytest.mark.parametrize("name", ic.case_names())
def test_verdict_member(emu_lib, verdicts, name, route):
    ic.check_member(emu_lib, verdicts, name, route)


# ---- the differential run: 40 BGZF members and the three Mgzip ones (measured on the CPU: 10 s for both routes and both
# formats, 8 s to build and check the seeds of this file and of the GPU file, which runs 200 members; the whole file: 55 s)
@pytest.fixture(scope="module")
def hostile():
    return ic.hostile_bgzf(40, 7100)


@pytest.fixture(scope="module")
def hostile_big():
    return ic.hostile_mgzip(7200)


def test_hostile_seeds_reach_the_edges(hostile, hostile_big):
    """The seeds of BOTH files (this one's 40 members, the GPU file's 200) hold every edge the run is about."""
    ic.check_stats(hostile[2])
    ic.check_stats(ic.hostile_bgzf(ic.GPU_MEMBERS, ic.GPU_SEED)[2])


@pytest.mark.parametrize("route", sorted(ic.ROUTES))
def test_hostile_bgzf(emu_lib, hostile, route):
    ic.check_hostile_bgzf(emu_lib, route, hostile[0], hostile[1])


@pytest.mark.parametrize("route", sorted(ic.ROUTES))
def test_hostile_mgzip(emu_lib, hostile_big, route):
    ic.check_hostile_mgzip(emu_lib, route, hostile_big[0])
