"""The persistent grid of the last Laplace kernel (k_lap_final_v4) must not show in the output.

Its default size is a multiple of the workgroups the device really holds (laplace.hip, lap_fin_resident: the runtime's occupancy answer
for the launched instance x the CUs), so it changes with the kernel's register budget and with the part.  Which wave walks which strips --
and how many strips a wave walks -- follows from it; every strip is computed from global memory alone, so another partition must not change
a byte.  Both flavours of the Lab arithmetic: the shipped one (table + u8 steps: the instance held to six waves per SIMD) and the
OpenCV-order one.
  (a) 328 x 109, 3 levels, calls of (1, 4, 3) frames, strips of 8 rows: a second strip column with 18 live lanes, a short last strip row.
      Default grid against one workgroup that walks everything.
  (b) 1920 x 1080, 6 levels, a first frame and one call of 12 frames: 8 x 135 x 12 = 12 960 strips of 8 rows, more than the 12 288 waves
      of 2 x 768 workgroups -- the smallest count at which the waves of such a grid loop.  Default grid against 7 workgroups and against
      1024, the partition this launch had before the grid followed the occupancy."""
import os

import numpy as np
import pytest

from helpers import TorchMem

pytestmark = pytest.mark.gpu

_FIN = {"LVM_FIN_ROWS": "8", "LVM_FIN_MIN_TASKS": "0"}
_FRAMES = {}


@pytest.fixture(scope="module")
def dev():
    return TorchMem()


def _frames(lvm, size, n):
    """the first n frames of the synthetic clip at this size, generated once and left unchanged"""
    if size not in _FRAMES:
        ck, pk = lvm.synth.config(0, size)
        clip = lvm.synth.Clip(seed=1234, **ck)
        _FRAMES[size] = (pk, np.stack([clip.frame(t) for t in range(n)]))
    pk, fr = _FRAMES[size]
    assert len(fr) >= n
    return pk, fr


def _run(lvm, lib, mem, size, calls, env, exact):
    """per call: (produced flags, output bytes, {report name: variants})"""
    w, h, levels = size
    pk, frames = _frames(lvm, size, sum(calls))
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    ctx, res, t, fb = None, [], 0, w * h * 3
    try:
        ctx = lvm.Context(0, 1, lib)
        ctx.exact_lab(exact)
        ctx.profile(True)
        cp = lvm.LvmParams(pk["mode"], pk["levels"], pk["amplification"], pk["coWavelength"], pk["coLow"], pk["coHigh"], pk["chromAttenuation"],
                           pk["framerate"], 0)
        for nf in calls:
            fin = np.array(frames[t:t + nf][:, None], copy=True)          # [frame][stream][h][w][3]: the shared frames stay as they are
            d_in = mem.upload(fin)
            d_out = mem.zeros_like(d_in)
            prod = ctx.process_device_frames(cp, nf, mem.ptr(d_in), w, h, 3, w * 3, fb, fb, mem.ptr(d_out), w * 3, fb, fb, mem.stream())
            mem.sync(ctx)
            out = np.array(mem.download(d_out), copy=True)
            variants = ctx.profile_variants()
            names = {n: variants.get(n, set()) for n in ctx.profile_collect()}
            ctx.profile_only(None)
            res.append((list(prod), out, names))
            t += nf
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if ctx is not None:
            ctx.close()
    return res


def _same(a, b, what):
    assert len(a) == len(b)
    for k, ((pa, oa, _), (pb, ob, _)) in enumerate(zip(a, b)):
        assert pa == pb, (what, k, pa, pb)
        assert np.array_equal(oa, ob), "%s, call %d: %d bytes differ" % (what, k, int((oa != ob).sum()))
    assert any(p for r in a for p in r[0]), what


@pytest.mark.parametrize("exact", [False, True], ids=["shipped", "opencv-order"])
def test_small_frame_default_grid_equals_one_workgroup(lvm, hip, dev, exact):
    size, calls = (328, 109, 3), (1, 4, 3)
    base = _run(lvm, hip, dev, size, calls, dict(_FIN), exact)
    one = _run(lvm, hip, dev, size, calls, dict(_FIN, LVM_FIN_GROUPS="1"), exact)
    for res in (base, one):
        for k, (_, _, names) in enumerate(res):
            assert names.get("lap_final") == {"strips"}, (k, sorted(names), names.get("lap_final"))
    _same(base, one, "default grid vs. LVM_FIN_GROUPS=1")


def test_full_hd_default_grid_equals_other_partitions(lvm, hip, dev):
    size, calls = (1920, 1080, 6), (1, 12)
    base = _run(lvm, hip, dev, size, calls, dict(_FIN), False)
    for k, (_, _, names) in enumerate(base):
        assert names.get("lap_final") == {"strips"}, (k, sorted(names), names.get("lap_final"))
    for g in ("7", "1024"):
        other = _run(lvm, hip, dev, size, calls, dict(_FIN, LVM_FIN_GROUPS=g), False)
        _same(base, other, "default grid vs. LVM_FIN_GROUPS=" + g)
