"""Every colour once.  content.cube_frames lays all triples (B, G, R) of a value set out as one square frame, in natural order and
in a seeded permutation.  Laplace with amplification 0 makes a clip's first frame a function of the pixel's colour alone, Lab2BGR(Lab(in)):
the forward table path (csrc/lab_lut.h) and the inverse conversion (csrc/lvm_internal.h) on the whole cube, with arbitrary colours
in the neighbouring lanes.

  gfx950 build   : the 256 values 0 .. 255, two 4096 x 4096 frames -- all 2^24 colours;
  emulation build: 64 values that take every cell of the table and the weights 0 and 15, two 512 x 512 frames."""
import numpy as np
import pytest

import content
from helpers import TorchMem, c_params

LEVELS = 2


def _config(lvm, side, amplification=None):
    ck, pk = lvm.synth.config(0, (side, side, LEVELS))
    if amplification is not None:
        pk["amplification"] = amplification
    return pk


def _cube(po, lvm, values, seed=9):
    """frames, the permutation, and the oracle's round trip (amplification 0) of the natural frame: computed once per module"""
    nat, per = content.cube_frames(values, seed)
    perm = content.cube_permutation(len(values) ** 3, seed)
    assert np.array_equal(per.reshape(-1, 3), nat.reshape(-1, 3)[perm])
    assert len(np.unique(nat.reshape(-1, 3).astype(np.uint32) @ np.array([1, 256, 65536], np.uint32))) == len(values) ** 3
    orc = po.Oracle()
    try:
        ref, pr = orc.process(nat, po.make_params(**_config(lvm, nat.shape[0], 0.0)))
        assert pr
        ref_float = orc.last_float().copy()
    finally:
        orc.close()
    for a in (nat, per, perm, ref, ref_float):
        a.setflags(write=False)
    return nat, per, perm, ref, ref_float


def _round_trip(lvm, lib, cube):
    """lvm_process, amplification 0: exact flavour with keep_float bit-equal to the oracle; shipped configuration: the permuted
    frame gives the permuted bytes of the natural frame (no reference needed), and the natural frame the oracle's bytes within the
    project's bars.  Returns the shipped configuration's [worst LSB difference, identical fraction] against the oracle."""
    nat, per, perm, ref, ref_float = cube
    cp = c_params(lvm, _config(lvm, nat.shape[0], 0.0))
    ctx = lvm.Context(0, 1, lib)
    ctx.keep_float(True)
    ctx.exact_lab(True)
    try:
        out, pr = ctx.process(nat, cp)
        assert pr
        got_float = ctx.read_float(ref_float.shape)
        bad = np.flatnonzero((got_float.view(np.uint32) != ref_float.view(np.uint32)).reshape(-1, 3).any(axis=1))
        assert bad.size == 0, "exact flavour: %d colours differ in the float frame, first (B, G, R) = %s: %s vs the oracle's %s" % (
            bad.size, nat.reshape(-1, 3)[bad[0]], got_float.reshape(-1, 3)[bad[0]], ref_float.reshape(-1, 3)[bad[0]])
        bad = np.flatnonzero((out != ref).reshape(-1, 3).any(axis=1))
        assert bad.size == 0, "exact flavour: %d colours differ in the bytes, first (B, G, R) = %s: %s vs the oracle's %s" % (
            bad.size, nat.reshape(-1, 3)[bad[0]], out.reshape(-1, 3)[bad[0]], ref.reshape(-1, 3)[bad[0]])
    finally:
        ctx.close()
    ctx = lvm.Context(0, 1, lib)
    try:
        out_nat, pr = ctx.process(nat, cp)
        assert pr
        out_nat = out_nat.copy()
        ctx.reset()                                     # (a second frame adds the temporally filtered top level: no function of the pixel alone)
        out_per, pr = ctx.process(per, cp)
        assert pr
        bad = np.flatnonzero((out_per.reshape(-1, 3) != out_nat.reshape(-1, 3)[perm]).any(axis=1))
        assert bad.size == 0, "shipped configuration: %d colours come out differently in another place, first (B, G, R) = %s: %s vs %s" % (
            bad.size, per.reshape(-1, 3)[bad[0]], out_per.reshape(-1, 3)[bad[0]], out_nat.reshape(-1, 3)[perm[bad[0]]])
    finally:
        ctx.close()
    du = np.abs(out_nat.astype(np.int16) - ref.astype(np.int16))
    worst = [int(du.max()), float((du == 0).mean())]
    print("cube of %d colours, shipped configuration vs oracle: worst LSB difference %d, identical fraction %.6f" % (
        nat.shape[0] * nat.shape[1], worst[0], worst[1]))
    assert worst[0] <= 1 and worst[1] >= 0.999, worst
    return worst


# ---- emulation build: 64 values ---------------------------------------------------------------------------------------------------
def test_cube_values_take_every_cell_and_both_end_weights():
    v = content.cube_values(64).astype(np.int64)
    assert len(np.unique(v)) == 64 and {0, 1, 254, 255} <= set(v.tolist())
    fine = (514 * v + 4) >> 8                         # lab_lut.h: cell << 4 | weight (tests/test_lab_lut.py: the closed form)
    assert set((fine >> 4).tolist()) == set(range(33))
    assert {0, 15} <= set((fine & 15).tolist())


def test_cube_frames_hold_every_triple_once():
    nat, per = content.cube_frames(content.cube_values(64))
    assert nat.shape == per.shape == (512, 512, 3) and nat.dtype == np.uint8
    key = lambda f: np.sort(f.reshape(-1, 3).astype(np.uint32) @ np.array([1, 256, 65536], np.uint32))
    assert np.array_equal(key(nat), key(per)) and len(np.unique(key(nat))) == 64 ** 3
    assert not np.array_equal(nat, per)


def test_emu_cube_64_values_round_trip(lvm, po, emu):
    _round_trip(lvm, emu, _cube(po, lvm, content.cube_values(64)))


# ---- gfx950 build: all 2^24 colours ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube256(lvm, po):
    return _cube(po, lvm, np.arange(256, dtype=np.uint8))


@pytest.fixture(scope="module")
def dev():
    return TorchMem()


@pytest.mark.gpu
def test_gpu_cube_round_trip_of_every_colour(lvm, hip, cube256):
    _round_trip(lvm, hip, cube256)


@pytest.mark.gpu
def test_gpu_cube_batched_frames_exact(lvm, po, hip, dev, cube256):
    """lvm_process_device_frames on [natural, permuted], exact flavour, default amplification: the oracle's bytes frame by frame,
    through the fused table + first pyramid kernel (lap_down0_lut), which the launch code picks at this size."""
    nat, per = cube256[:2]
    side = nat.shape[0]
    pk = _config(lvm, side)
    fb = side * side * 3
    ctx = lvm.Context(0, 1, hip)
    ctx.exact_lab(True)
    ctx.profile(True)
    try:
        d_in = dev.upload(np.stack([nat, per]))
        d_out = dev.zeros_like(d_in)
        prod = ctx.process_device_frames(c_params(lvm, pk), 2, dev.ptr(d_in), side, side, 3, side * 3, fb, fb, dev.ptr(d_out), side * 3, fb, fb,
                                         dev.stream())
        dev.sync(ctx)
        got = dev.download(d_out)
        names = ctx.profile_collect()
    finally:
        ctx.close()
    assert "lap_down0_lut" in names and "lab_lut" not in names, sorted(names)
    orc = po.Oracle()
    try:
        for t, f in enumerate((nat, per)):
            ref, pr = orc.process(f, po.make_params(**pk))
            assert pr == prod[t]
            bad = np.flatnonzero((got[t] != ref).reshape(-1, 3).any(axis=1))
            assert bad.size == 0, "frame %d: %d pixels differ, first (B, G, R) = %s: %s vs the oracle's %s" % (
                t, bad.size, f.reshape(-1, 3)[bad[0]], got[t].reshape(-1, 3)[bad[0]], ref.reshape(-1, 3)[bad[0]])
    finally:
        orc.close()


@pytest.mark.gpu
def test_gpu_cube_byte_kernels_exact(lvm, hip, dev, cube256):
    """lvm_process_device from a view whose input and output base pointers are odd: the byte forms of the table kernel and of the
    first and last Laplace kernels on every colour, exact flavour, amplification 0 -- the oracle's bytes of the round trip."""
    nat, _, _, ref, _ = cube256
    side = nat.shape[0]
    fb = side * side * 3
    buf = np.full(fb + 16, 0xAB, np.uint8)
    buf[1:1 + fb] = nat.reshape(-1)
    ctx = lvm.Context(0, 1, hip)
    ctx.exact_lab(True)
    ctx.profile(True)
    try:
        d_in = dev.upload(buf)
        d_out = dev.upload(np.full(fb + 16, 0xCD, np.uint8))
        p_in, p_out = dev.ptr_at(d_in, 1), dev.ptr_at(d_out, 1)
        assert p_in % 2 == 1 and p_out % 2 == 1
        assert ctx.process_device(c_params(lvm, _config(lvm, side, 0.0)), p_in, side, side, 3, side * 3, fb, p_out, side * 3, fb, dev.stream())
        dev.sync(ctx)
        got = dev.download(d_out)
        variants = ctx.profile_variants()
    finally:
        ctx.close()
    assert variants.get("lab_lut") == {"bytes"} and variants.get("lap_down0") == {"bytes"} and variants.get("lap_final") == {"bytes"}, variants
    assert (got[:1] == 0xCD).all() and (got[1 + fb:] == 0xCD).all(), "bytes outside the output view were written"
    out = got[1:1 + fb].reshape(side, side, 3)
    bad = np.flatnonzero((out != ref).reshape(-1, 3).any(axis=1))
    assert bad.size == 0, "%d colours differ, first (B, G, R) = %s: %s vs the oracle's %s" % (
        bad.size, nat.reshape(-1, 3)[bad[0]], out.reshape(-1, 3)[bad[0]], ref.reshape(-1, 3)[bad[0]])
