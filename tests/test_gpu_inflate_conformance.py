"""Inflate conformance on the MI355X (tests/inflate_cases.py): libdeflate's recorded verdict on every crafted stream, on
Decompressor.deflate_decompress and on both DContext routes, and the hostile encoder's differential run."""
import pytest

import inflate_cases as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def verdicts():
    return ic.load_verdicts()


@pytest.mark.parametrize("name", ic.case_names())
def test_verdict_decompressor(hip_lib, verdicts, name):
    ic.check_decompressor(hip_lib, verdicts, name)


@pytest.mark.parametrize("route", sorted(ic.ROUTES))
@pytest.mark.parametrize("name", ic.case_names())
def test_verdict_member(hip_lib, verdicts, name, route):
    ic.check_member(hip_lib, verdicts, name, route)


@pytest.fixture(scope="module")
def hostile():
    streams, raws, stats = ic.hostile_bgzf(ic.GPU_MEMBERS, ic.GPU_SEED)
    ic.check_stats(stats)
    return streams, raws


@pytest.fixture(scope="module")
def hostile_big():
    return ic.hostile_mgzip(7200)[0]


@pytest.mark.parametrize("route", sorted(ic.ROUTES))
def test_hostile_bgzf(hip_lib, hostile, route):
    ic.check_hostile_bgzf(hip_lib, route, hostile[0], hostile[1])


@pytest.mark.parametrize("route", sorted(ic.ROUTES))
def test_hostile_mgzip(hip_lib, hostile_big, route):
    ic.check_hostile_mgzip(hip_lib, route, hostile_big)
