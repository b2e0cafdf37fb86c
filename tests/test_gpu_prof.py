"""tests/prof_cases.py on the MI355X through the real library: the same streams and the same placement of the stage
times as on the emulator, and real events besides -- every stage the context launches reads a time in mode 1, the
dominant stage reads one in mode 2, through the per-batch wait and through submit + wait."""
import pytest

import prof_cases as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("slab", list(pc.SLABS))
@pytest.mark.parametrize("kind", pc.KINDS)
def test_profiling_modes(hip_lib, oracle, kind, slab):
    pc.run(hip_lib, oracle, kind, slab, True)
