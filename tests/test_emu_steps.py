"""The steps of the single-workgroup scans through the CPU emulator (a device pointer is a host pointer there): the shared
bodies of tests/step_cases.py.  A call with 4,096 ranges takes seconds on the emulator, so the pieces cross their step
at three places only; tests/test_gpu_steps.py sweeps every place.  The steps of k_ln_prefix, k_fd_scan and of where's
grid-stride sweep take streams that the emulator cannot hold: they are crossed on the GPU alone."""
import step_cases
from step_cases import FL_STEP


def test_piece_steps(emu_lib):
    step_cases.piece_steps(emu_lib, ks=(FL_STEP - 5, FL_STEP - 2, FL_STEP), table_ks=(FL_STEP - 2,), mgzip_ks=(FL_STEP - 2,))


def test_member_steps(emu_lib):
    step_cases.member_steps(emu_lib, light=True)
