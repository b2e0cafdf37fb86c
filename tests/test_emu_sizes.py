"""gzpx_inflate_batch_sizes_device through the CPU emulator (a device pointer is a host pointer there): the shared
bodies of tests/size_cases.py with members of at most a few tens of KiB."""
import pytest

import size_cases
from size_cases import WRAPS


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_sizes_right(emu_lib, wrap):
    size_cases.sizes_right(emu_lib, WRAPS[wrap], small=True)


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_loose_extents(emu_lib, wrap):
    size_cases.loose_extents(emu_lib, WRAPS[wrap], small=True)


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_round_trip(emu_lib, wrap):
    size_cases.round_trip(emu_lib, WRAPS[wrap], small=True)


def test_big_launch(emu_lib):
    size_cases.big_launch(emu_lib, size_cases.ZLIB, n=20000)


@pytest.mark.parametrize("wrap", ["raw", "zlib"])
def test_crafted_streams(emu_lib, wrap):
    size_cases.crafted(emu_lib, WRAPS[wrap], sample=4)


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_failures_stay_local(emu_lib, wrap):
    size_cases.failures_stay_local(emu_lib, WRAPS[wrap])


def test_max_out_size(emu_lib):
    size_cases.max_out_size(emu_lib, count_steps=True)


def test_debug_two_counts_alike(emu_lib):
    size_cases.debug_two_counts_alike(emu_lib)


def test_arguments(emu_lib):
    size_cases.arguments(emu_lib)


def test_no_read_past_the_input(emu_lib):
    size_cases.no_read_past_input(emu_lib)
