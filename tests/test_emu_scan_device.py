"""Member discovery on the device through the CPU emulator (a device pointer is a host pointer there): the shared
bodies of tests/scan_cases.py, every comparison exact against gzpx_scan_blocks on the same bytes."""
import scan_cases


def test_well_formed_streams(emu_lib, oracle):
    scan_cases.well_formed(emu_lib, oracle)


def test_foreign_members(emu_lib):
    scan_cases.foreign_members(emu_lib)


def test_truncation(emu_lib):
    scan_cases.truncation(emu_lib)


def test_max_blocks(emu_lib, oracle):
    scan_cases.max_blocks(emu_lib, oracle)


def test_invalid_headers(emu_lib):
    scan_cases.invalid_headers(emu_lib)


def test_impostors(emu_lib, oracle):
    scan_cases.impostors(emu_lib, oracle)


def test_stream_decompress(emu_lib, oracle):
    scan_cases.stream_decompress(emu_lib, oracle)


def test_index(emu_lib, oracle):
    scan_cases.index(emu_lib, oracle)
