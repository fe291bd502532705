"""Every launch switch and every run-time kernel instantiation on the gfx950 build (the cases: tests/parity_matrix.py, SWITCH_CASES; the
emulation twin: tests/test_emu_switches.py).  Laplace and Color equal the oracle bit for bit; Riesz calls acosf / sinf / cosf, so its cases
give the float frames and bytes of the default kernels on the same GPU (tests/test_gpu_exact.py, (3)).  Every case asserts the report
name and variant of the kernel it is there for.  No case sets a value the switches' validators refuse."""
import pytest

import parity_matrix as M
from helpers import TorchMem
from test_emu_switches import EMU_SIZES, zero_copy_off_child

pytestmark = pytest.mark.gpu

REFERENCE = {k: "default" for k, c in M.SWITCH_CASES.items() if c["idx"] == 2}
# (the largest case, deep10 -- 3072 x 2564, ten levels, three frames, most of it the oracle's share -- takes 1.4 s on an MI355X host, every
# other case under 0.6 s)


@pytest.fixture(scope="module")
def dev():
    return TorchMem()


@pytest.mark.parametrize("key", list(M.SWITCH_CASES))
def test_switch_case_gpu(lvm, po, hip, dev, key):
    M.switch_case(lvm, po, hip, dev, "gpu", key, REFERENCE.get(key, "oracle"))


def test_every_runtime_instantiation_is_reached(lvm, po, hip, dev):
    seen = M.ledger(lvm, po, hip, dev, "gpu", M.LEDGER_KEYS, REFERENCE)
    assert M.REQUIRED <= seen, sorted(M.REQUIRED - seen)


def test_zero_copy_off_gpu(hip):
    """one more process with the GPU open, under its own time limit"""
    zero_copy_off_child("", EMU_SIZES, 120)
