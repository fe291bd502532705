"""LVM_RZ_PORTABLE_TRIG on the CPU emulation build: the exact-flavour Riesz kernels with csrc/rz_trig.h in place of the host libm,
against the oracle under LVMO_VAR_PORTABLE_TRIG -- one case per instantiation that calls the header (tests/parity_matrix.py,
PTRIG_CASES; the gfx950 twin: tests/test_gpu_riesz_exact.py).  Every case: the bytes of every frame and the float frame of every
call's first frame equal the oracle's bit for bit, and every phase and blur / amplify launch is reported as a `ptrig` variant.  One
more case has the switch on and the exact flavour off: the default flavour's bytes, and no `ptrig` anywhere."""
import numpy as np
import pytest

import parity_matrix as M
from helpers import HostMem

HOST = HostMem()


@pytest.fixture
def ptrig(monkeypatch, po):
    def on(oracle_bits=()):
        return M.portable_trig(monkeypatch, po, oracle_bits)
    yield on
    po.set_variant(0)


@pytest.mark.parametrize("key", list(M.PTRIG_CASES))
def test_portable_trig_case_emu(lvm, po, emu, ptrig, key):
    ptrig(M.PTRIG_CASES[key]["oracle_bits"])
    M.switch_case(lvm, po, emu, HOST, "emu-ptrig", key)


@pytest.mark.parametrize("size", [(264, 150, 3), (134, 78, 2)])
def test_the_oracle_bit_is_alive_on_these_frames(lvm, po, size):
    """oracle(bit) differs from oracle(0) in the float frames of these very clips: equality with oracle(bit) cannot be had by a
    library, or an oracle, that ignores its switch"""
    ck, pk = lvm.synth.config(2, size)
    clip = lvm.synth.Clip(**ck)
    P = po.make_params(**pk)
    floats = []
    try:
        for mask in (0, po.VARIANTS["portable_trig"]):
            po.set_variant(mask)
            orc = po.Oracle()
            try:
                for t in range(4):
                    _, pr = orc.process(clip.frame(t), P)
                floats.append(orc.last_float().copy())
            finally:
                orc.close()
    finally:
        po.set_variant(0)
    share = float((floats[0] != floats[1]).mean())
    assert share > 0.01, share


def test_switch_on_in_the_default_flavour_changes_nothing(lvm, emu):
    for size in ((264, 150, 3), (134, 78, 2)):
        on_names, on, _ = M.profiled_call(lvm, emu, HOST, *size, env={"LVM_RZ_PORTABLE_TRIG": "1"}, exact_lab=False)
        off_names, off, _ = M.profiled_call(lvm, emu, HOST, *size, env={"LVM_RZ_PORTABLE_TRIG": "0"}, exact_lab=False)
        M.no_ptrig_launches(on_names)
        assert on_names == off_names and any(n.startswith("rz_blur_amp") for n in on_names), (on_names, off_names)
        assert np.array_equal(on, off), "%d bytes differ" % int((on != off).sum())
