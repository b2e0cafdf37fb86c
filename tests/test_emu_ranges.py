"""Random-access reads by range through the CPU emulator (a device pointer is a host pointer there): the shared bodies
of tests/range_cases.py, every byte compared with zlib's inflate of the same members."""
import range_cases


def test_index(emu_lib, oracle):
    range_cases.index(emu_lib, oracle)


def test_empty_stream(emu_lib):
    range_cases.empty_stream(emu_lib)


def test_ranges(emu_lib, oracle):
    range_cases.ranges(emu_lib, oracle)


def test_virtual_offsets(emu_lib, oracle):
    range_cases.virtual(emu_lib, oracle)


def test_errors(emu_lib):
    range_cases.errors(emu_lib)


def test_only_needed_members_are_touched(emu_lib):
    range_cases.touched(emu_lib)


def test_members_around_the_several_waves_size(emu_lib):
    range_cases.big_members(emu_lib)
