"""The selection of lines by content and the read by table through the CPU emulator (a device pointer is a host pointer
there): the shared bodies of tests/select_cases.py, every run, count and byte compared with what bytes.find, numpy and
the joined lines give on zlib's inflate of the same members."""
import select_cases


def test_edge_sets(emu_lib):
    select_cases.edge_sets(emu_lib)


def test_scan_step(emu_lib):
    select_cases.scan_step(emu_lib)


def test_records(emu_lib):
    select_cases.records(emu_lib)


def test_attribution_every_split(emu_lib):
    select_cases.attribution_every_split(emu_lib)


def test_attribution_tiny_members(emu_lib):
    select_cases.attribution_tiny_members(emu_lib)


def test_attribution_delimiters(emu_lib):
    select_cases.attribution_delimiters(emu_lib)


def test_lost_updates(emu_lib):
    select_cases.lost_updates(emu_lib)


def test_capacity(emu_lib):
    select_cases.capacity(emu_lib)


def test_errors(emu_lib):
    select_cases.errors(emu_lib)


def test_damaged_member(emu_lib):
    select_cases.damaged(emu_lib)


def test_table_reads(emu_lib, oracle):
    select_cases.table_reads(emu_lib, oracle)


def test_table_errors(emu_lib, oracle):
    select_cases.table_errors(emu_lib, oracle)


def test_close_the_loop(emu_lib):
    select_cases.close_the_loop(emu_lib)
