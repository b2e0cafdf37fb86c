"""gzpx_inflate_batch_sizes_device on the MI355X: the shared bodies of tests/size_cases.py through the real library."""
import pytest

import size_cases
from size_cases import WRAPS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_sizes_right(hip_lib, wrap):
    size_cases.sizes_right(hip_lib, WRAPS[wrap])


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_loose_extents(hip_lib, wrap):
    size_cases.loose_extents(hip_lib, WRAPS[wrap])


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_round_trip(hip_lib, wrap):
    size_cases.round_trip(hip_lib, WRAPS[wrap])


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_big_launch(hip_lib, wrap):
    size_cases.big_launch(hip_lib, WRAPS[wrap])


@pytest.mark.parametrize("wrap", ["raw", "zlib"])
def test_crafted_streams(hip_lib, wrap):
    size_cases.crafted(hip_lib, WRAPS[wrap])


@pytest.mark.parametrize("wrap", sorted(WRAPS))
def test_failures_stay_local(hip_lib, wrap):
    size_cases.failures_stay_local(hip_lib, WRAPS[wrap])


def test_max_out_size(hip_lib):
    size_cases.max_out_size(hip_lib, count_steps=True)


def test_debug_two_counts_alike(hip_lib):
    size_cases.debug_two_counts_alike(hip_lib)


def test_arguments(hip_lib):
    size_cases.arguments(hip_lib)
