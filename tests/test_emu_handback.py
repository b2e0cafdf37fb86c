"""What the decode / copy pair hands back to k_inflate, and why, through the emulated kernels (tests/handback_cases.py).
No GPU."""
import pytest

import handback_cases as hc
import inflate_cases as ic


@pytest.fixture(scope="module")
def verdicts():
    return ic.load_verdicts()


@pytest.fixture(scope="module")
def cx(emu_lib):
    c = hc.Contexts(emu_lib)
    yield c
    c.close()


def test_table_agrees_with_libdeflates_verdicts(verdicts):
    hc.check_table(verdicts)


@pytest.mark.parametrize("name", hc.crafted_names())
def test_crafted(cx, verdicts, name):
    hc.check_crafted(cx, verdicts, name)


@pytest.mark.parametrize("name", hc.RAW_NAMES)
def test_crafted_count_mode(cx, name):
    hc.check_crafted_raw(cx, name)


def test_hostile_encoder(cx):
    hc.check_valid(cx, hc.hostile(), hc.HOSTILE_RESYNC)


def test_zlib_strategies(cx):
    hc.check_valid(cx, hc.zlib_members(), hc.ZLIB_RESYNC)


def test_every_symbol(cx):
    hc.check_valid(cx, hc.alphabet_members(), hc.ALPHABET_RESYNC)


def test_hostile_encoder_count_mode(cx):
    hc.check_valid_raw(cx, hc.hostile(), hc.HOSTILE_RESYNC)


def test_zlib_strategies_count_mode(cx):
    hc.check_valid_raw(cx, hc.zlib_members(), hc.ZLIB_RESYNC)


def test_every_symbol_count_mode(cx):
    hc.check_valid_raw(cx, hc.alphabet_members(), hc.ALPHABET_RESYNC)


def test_eight_waves_a_member(cx):
    hc.check_big(cx)
