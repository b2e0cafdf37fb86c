"""gzpx_inflate_batch_device on the MI355X: the shared bodies of tests/batch_cases.py through the real library."""
import pytest

import batch_cases
from batch_cases import WRAPS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_bytes(hip_lib, wrap):
    batch_cases.bytes_right(hip_lib, WRAPS[wrap])


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_big_launch(hip_lib, wrap):
    batch_cases.big_launch(hip_lib, WRAPS[wrap])


def test_one_stream_two_doors(hip_lib, oracle):
    batch_cases.two_doors(hip_lib, oracle)


def test_gzip_headers(hip_lib):
    batch_cases.headers(hip_lib, batch_cases.GZIP)


def test_zlib_headers(hip_lib):
    batch_cases.headers(hip_lib, batch_cases.ZLIB)


def test_adler_edges(hip_lib):
    batch_cases.adler_edges(hip_lib, big=1 << 20)


def test_adler32_host_call(hip_lib):
    batch_cases.adler_host_call(hip_lib, big=1 << 20)


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_failures_stay_local(hip_lib, wrap):
    batch_cases.failures_stay_local(hip_lib, WRAPS[wrap])


def test_sizes_and_flags(hip_lib):
    batch_cases.sizes_and_flags(hip_lib)


@pytest.mark.parametrize("wrap", ["raw", "zlib"])
def test_crafted_streams(hip_lib, wrap):
    batch_cases.crafted(hip_lib, WRAPS[wrap])
