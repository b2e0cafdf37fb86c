"""tests/read_call_cases.py through the product sources on the CPU emulator: every call of the script hands back what it
handed back before the indexed reads of gzpx_api.cpp were given one home per step, and puts the same host-side work
around its kernels -- event records, stream synchronisations, allocations."""
import read_call_cases as rc

# Per call: the return code, the out-values in the order read_call_cases.run lists them, and (hipEventRecord calls,
# stream synchronisations, allocations).  Not worked out by hand: printed by `python tests/read_call_cases.py` on the
# commit before the reorganisation (6d95975).  The emulator is deterministic, so the numbers carry no margin.
EXPECTED = [
    ("index build", (0, 6, 41333, 100100, (2, 2, 26))),
    ("ranges: one", (0, 777, True, 3256634083, 2175769796, (777, 17, 34), 1, (8, 2, 15))),
    ("ranges: 200", (0, 20000, True, 1753904774, 4042092092, (777, 17, 34), 5, (8, 2, 10))),
    ("ranges: empty only", (0, 0, True, 420107693, 2204801007, (777, 17, 34), 0, (2, 1, 0))),
    ("ranges: bad range", (1, 0, 1, 3262946108, 2204801007, (777, 17, 34), 0, (2, 2, 0))),
    ("ranges: one byte short", (4, 20000, True, 2496215465, 2204801007, (777, 17, 34), 0, (2, 2, 0))),
    ("ranges: damaged member", (13, 0, True, 4226472697, 3470588445, (3, 2599008278, 2599008342), 3, (8, 2, 0))),
    ("lines build", (0, True, 849, 850, (777, 17, 34), True, (18, 4, 9))),
    ("lines build: damaged member", (13, False, 0, 0, (3, 2599008278, 2599008342), True, (12, 2, 3))),
    ("line offsets", (0, True, 3287974643, (777, 17, 34), 5, (8, 2, 0))),
    ("read lines", (0, 1473, True, 4012196195, 1501785933, 1729111168, (777, 17, 34), 5, (10, 3, 0))),
    ("read lines: one byte short", (4, 1473, True, 1931345528, 1501785933, 2204801007, (777, 17, 34), 5, (8, 2, 0))),
    ("read lines: damaged member", (13, 0, True, 1672798330, 3262946108, 2204801007, (3, 2599008278, 2599008342), 0, (8, 2, 0))),
    ("find: count only", (0, 1908, 2743463053, 2743463053, (777, 17, 34), True, (21, 4, 6))),
    ("find: positions + lines", (0, 1908, 994461814, 3286930372, (777, 17, 34), True, (21, 4, 0))),
    ("find: hits_cap too small", (4, 1908, 807462612, 3661989346, (777, 17, 34), True, (21, 4, 0))),
    ("find: damaged member", (13, 0, 1223625442, 2394936202, (3, 2599008278, 2599008342), True, (14, 2, 0))),
    ("inflate batch", (0, 45000, 0, (777, 17, 34), (4, 1, 0))),
    ("inflate batch sizes", (0, 45000, 0, [5000, 0, 40000], (777, 17, 34), (3, 1, 0))),
    ("checksum batch", (0, 0, True, (777, 17, 34), (2, 1, 3))),
    ("checksum batch: one wrong", (13, 1, True, (2, 2134047741, 2134047740), (2, 1, 0))),
]


def test_read_calls_do_the_same_host_side_work(emu_lib, oracle):
    got = rc.run(emu_lib, oracle)
    assert [name for name, _ in got] == [name for name, _ in EXPECTED]
    for (name, row), (_, want) in zip(got, EXPECTED):
        assert row == want, name
