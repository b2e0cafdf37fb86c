"""gzpx_inflate_batch_device through the CPU emulator (a device pointer is a host pointer there): the shared bodies
of tests/batch_cases.py with members of at most a few tens of KiB."""
import pytest

import batch_cases
from batch_cases import WRAPS


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_bytes(emu_lib, wrap):
    batch_cases.bytes_right(emu_lib, WRAPS[wrap], small=True)


def test_big_launch(emu_lib):
    batch_cases.big_launch(emu_lib, batch_cases.ZLIB, n=20000)


def test_one_stream_two_doors(emu_lib, oracle):
    batch_cases.two_doors(emu_lib, oracle, n=150000)


def test_gzip_headers(emu_lib):
    batch_cases.headers(emu_lib, batch_cases.GZIP)


def test_zlib_headers(emu_lib):
    batch_cases.headers(emu_lib, batch_cases.ZLIB)


def test_adler_edges(emu_lib):
    batch_cases.adler_edges(emu_lib, big=70000)


def test_adler32_host_call(emu_lib):
    batch_cases.adler_host_call(emu_lib, big=70000)


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_failures_stay_local(emu_lib, wrap):
    batch_cases.failures_stay_local(emu_lib, WRAPS[wrap])


def test_sizes_and_flags(emu_lib):
    batch_cases.sizes_and_flags(emu_lib)


@pytest.mark.parametrize("wrap", ["raw", "zlib"])
def test_crafted_streams(emu_lib, wrap):
    batch_cases.crafted(emu_lib, WRAPS[wrap], sample=4)


def test_no_read_past_the_input(emu_lib):
    batch_cases.no_read_past_input(emu_lib)
