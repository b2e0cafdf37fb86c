"""The search for a set of patterns through the CPU emulator (a device pointer is a host pointer there): the shared
bodies of tests/findset_cases.py, every count, position, id, line and run compared with what bytes.find and numpy give on
zlib's inflate of the same members."""
import findset_cases


def test_one_pattern(emu_lib):
    findset_cases.one_pattern(emu_lib)


def test_mixed_lengths(emu_lib):
    findset_cases.mixed_lengths(emu_lib)


def test_same_position(emu_lib):
    findset_cases.same_position(emu_lib)


def test_buckets(emu_lib):
    findset_cases.buckets(emu_lib)


def test_order_every_split(emu_lib):
    findset_cases.order_every_split(emu_lib)


def test_waiting_carry(emu_lib):
    findset_cases.waiting_carry(emu_lib)


def test_dense_overlaps(emu_lib):
    findset_cases.dense_overlaps(emu_lib)


def test_special_bytes(emu_lib):
    findset_cases.special_bytes(emu_lib)


def test_lines(emu_lib):
    findset_cases.lines(emu_lib)


def test_lines_close_the_loop(emu_lib):
    findset_cases.lines_close_the_loop(emu_lib)


def test_capacity(emu_lib):
    findset_cases.capacity(emu_lib)


def test_errors(emu_lib):
    findset_cases.errors(emu_lib)


def test_damaged_member(emu_lib):
    findset_cases.damaged(emu_lib)


def test_selection(emu_lib):
    findset_cases.selection(emu_lib)


def test_selection_errors(emu_lib):
    findset_cases.selection_errors(emu_lib)


def test_selection_damaged_member(emu_lib):
    findset_cases.selection_damaged(emu_lib)
