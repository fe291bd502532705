"""Riesz (Phase mode) on the gfx950 build held to the CPU oracle BIT FOR BIT.

Exact-flavour Riesz is IEEE arithmetic in the oracle's order except for three library calls -- acosf in the phase kernels, cosf / sinf
in the blur / amplify kernels -- where device libm and glibc differ in the last ulp (tests/test_gpu_exact.py, (3)).  Under
LVM_RZ_PORTABLE_TRIG=1 the kernels call csrc/rz_trig.h, and under LVMO_VAR_PORTABLE_TRIG the oracle calls the same header: float64
arithmetic rounded once, no libm on either side.  Then the GPU owes the oracle every float value and every byte, and a wrong border
lane, a dropped halo row, a store hazard or a buffer range off by one in a GPU-only primitive (DPP exchanges, buffer resources, LDS
staging) has no 0.1 % of the bytes to hide in.

The bodies and parameter lists are those of the emulation matrix (tests/parity_matrix.py, tests/test_emu_parity.py) and of the GPU
modules that hold Riesz to the bars; here each runs under the `ptrig` fixture with the comparison set to equality.  First in the file:
the three functions themselves, device against oracle on the input set of tests/test_rz_trig.py."""
import numpy as np
import pytest

import parity_matrix as M
import phase_gray as pg
import rz_trig_set as T
from helpers import TorchMem, c_params, frames_clip, padded_strides_clip
from test_emu_phase_gray import _batched as gray_batched, _per_frame as gray_per_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return TorchMem()


@pytest.fixture
def ptrig(monkeypatch, po):
    """LVM_RZ_PORTABLE_TRIG=1 and the oracle's LVMO_VAR_PORTABLE_TRIG for one test; both restored when it ends"""
    def on(oracle_bits=()):
        return M.portable_trig(monkeypatch, po, oracle_bits)
    on()
    yield on
    po.set_variant(0)


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


# ---- the functions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", T.FNS)
def test_device_functions_equal_the_oracle(lvm, po, hip, dev, fn):
    x, want = T.inputs(fn), T.oracle_values(po, fn)
    got = np.empty_like(want)
    ctx = lvm.Context(0, 1, hip)
    try:
        for i in range(0, x.size, T.BATCH):
            d_x = dev.upload(np.array(x[i:i + T.BATCH]))               # (a writable copy: the shared input set is read-only)
            d_y = dev.zeros_like(d_x)
            ctx.trig_eval(po.TRIG_FNS[fn], d_x.data_ptr(), d_y.data_ptr(), d_x.numel(), dev.stream())
            dev.sync(ctx)
            got[i:i + T.BATCH] = dev.download(d_y)
    finally:
        ctx.close()
    ok, n, first = T.same_bits(got, want)
    assert ok, "rz_%sf: %d of %d values differ, first at x = %r (bits %#010x): device %r, oracle %r" % (
        fn, n, x.size, x[first], int(x.view(np.uint32)[first]), got[first], want[first])


# ---- one profiled call per instantiation: the kernels that ran are the `ptrig` ones ----------------------------------------------
@pytest.mark.parametrize("key", list(M.PTRIG_CASES))
def test_portable_trig_case_gpu(lvm, po, hip, dev, ptrig, key):
    """(also the OpenCV build kinds: LVM_CV_FILTER_UNFUSED / LVM_CV_MUL_F32 against the oracle under the matching LVMO_VAR_* bits plus
    the new one, on 67 x 131 -- the smallest shape of tests/test_gpu_opencv_build.py -- and on the two sizes of the other cases)"""
    ptrig(M.PTRIG_CASES[key]["oracle_bits"])
    M.switch_case(lvm, po, hip, dev, "gpu-ptrig", key)


def test_switch_on_in_the_default_flavour_changes_nothing_gpu(lvm, hip, dev):
    for size in ((264, 150, 3), (134, 78, 2)):
        on_names, on, _ = M.profiled_call(lvm, hip, dev, *size, env={"LVM_RZ_PORTABLE_TRIG": "1"}, exact_lab=False)
        off_names, off, _ = M.profiled_call(lvm, hip, dev, *size, env={"LVM_RZ_PORTABLE_TRIG": "0"}, exact_lab=False)
        M.no_ptrig_launches(on_names)
        assert on_names == off_names, (on_names, off_names)
        assert np.array_equal(on, off), "%d bytes differ" % int((on != off).sum())


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,levels", M.RIESZ_SHAPES)
def test_riesz_exact(lvm, po, hip, ptrig, w, h, levels):
    M.riesz_shape(lvm, po, hip, w, h, levels)


# ---- kernel families forced onto small frames --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,levels,calls", M.RIESZ_TILE_KERNELS)
@pytest.mark.parametrize("wide", ["1", "0"])
def test_riesz_wide_and_narrow_tile_kernels_exact(lvm, po, hip, dev, ptrig, w, h, levels, calls, wide, monkeypatch):
    M.riesz_wide_and_narrow_tile_kernels(lvm, po, hip, dev, monkeypatch, w, h, levels, calls, wide)


@pytest.mark.parametrize("blur4", ["1", "0"])
def test_riesz_register_blocked_blur_exact(lvm, po, hip, ptrig, blur4, monkeypatch):
    M.riesz_register_blocked_blur(lvm, po, hip, monkeypatch, blur4)


@pytest.mark.parametrize("w,h,levels,rows,exact", [c for c in M.RIESZ_STRIP_BLUR if c[4]])
def test_riesz_strip_blur_exact(lvm, po, hip, ptrig, w, h, levels, rows, exact, monkeypatch):
    M.riesz_strip_blur(lvm, po, hip, monkeypatch, w, h, levels, rows, exact)


def test_riesz_strip_blur_in_temporal_batches_exact(lvm, po, hip, dev, ptrig, monkeypatch):
    M.riesz_strip_blur_in_temporal_batches(lvm, po, hip, dev, monkeypatch)


def test_riesz_tiled_blur_exact(lvm, po, hip, ptrig, monkeypatch):
    M.riesz_tiled_blur(lvm, po, hip, monkeypatch)


@pytest.mark.parametrize("compact", ["1", "0"])
def test_riesz_collapse_tile_variants_exact(lvm, po, hip, ptrig, compact, monkeypatch):
    M.riesz_collapse_tile_variants(lvm, po, hip, monkeypatch, compact)


@pytest.mark.parametrize("strip", M.RIESZ_SPLIT_STRIPS[0])
@pytest.mark.parametrize("w,h,levels", M.RIESZ_SPLIT_STRIPS[1])
def test_riesz_wave_strip_stencils_exact(lvm, po, hip, ptrig, w, h, levels, strip, monkeypatch):
    M.riesz_wave_strip_stencils(lvm, po, hip, monkeypatch, w, h, levels, strip)


@pytest.mark.parametrize("strip", M.RIESZ_COLLAPSE_STRIPS[0])
@pytest.mark.parametrize("w,h,levels", M.RIESZ_COLLAPSE_STRIPS[1])
def test_riesz_wave_strip_collapse_and_output_exact(lvm, po, hip, ptrig, w, h, levels, strip, monkeypatch):
    M.riesz_wave_strip_collapse_and_output(lvm, po, hip, monkeypatch, w, h, levels, strip)


# ---- state machine ------------------------------------------------------------------------------------------------------------------
def test_riesz_cutoff_change_gray_and_reset_exact(lvm, po, hip, ptrig):
    M.riesz_cutoff_change_gray_and_reset(lvm, po, hip)


@pytest.mark.parametrize("w,h,levels,ns,calls", M.RIESZ_BATCHES)
def test_riesz_temporal_batches_exact(lvm, po, hip, dev, ptrig, w, h, levels, ns, calls):
    frames_clip(lvm, po, hip, dev, 2, w, h, levels, ns, calls)


def _riesz(cases):
    return [c for c in cases if c[0] == 2]


@pytest.mark.parametrize("idx,pad_in,pad_out", _riesz(M.PADDED_STRIDES))
def test_riesz_padded_row_strides_exact(lvm, po, hip, dev, ptrig, idx, pad_in, pad_out):
    padded_strides_clip(lvm, po, hip, dev, idx, pad_in, pad_out)


@pytest.mark.parametrize("idx,const_from,size", _riesz(M.FLAT_REGIONS))
def test_riesz_flat_regions_and_constant_frames_exact(lvm, po, hip, ptrig, idx, const_from, size):
    """(200 x 120: a black block wider than the 9 x 9 + 13 x 13 supports -- its 0/0 patches must become the oracle's zeros)"""
    M.flat_regions(lvm, po, hip, idx, const_from, size)


def test_riesz_fully_constant_clip_exact(lvm, po, hip, ptrig):
    M.fully_constant_clip(lvm, po, hip, 2)


@pytest.mark.parametrize("idx,over", _riesz(M.EXTREME_PARAMETERS))
def test_riesz_extreme_parameters_exact(lvm, po, hip, ptrig, idx, over):
    M.extreme_parameters(lvm, po, hip, idx, over)


def test_riesz_size_and_channel_changes_exact(lvm, po, hip, ptrig):
    M.size_and_channel_changes(lvm, po, hip, 2)


# ---- content ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,idx,w,h,levels", [c for c in M.CHROMA_CASES if c[1] == 2])
def test_riesz_chroma_exact(lvm, po, hip, ptrig, kind, idx, w, h, levels):
    M.chroma_shape(lvm, po, hip, kind, idx, w, h, levels)


@pytest.mark.parametrize("idx,w,h,levels,ns,calls,over,clip_over", _riesz(M.CHROMA_BATCHES))
def test_riesz_chroma_temporal_batches_exact(lvm, po, hip, dev, ptrig, idx, w, h, levels, ns, calls, over, clip_over):
    M.chroma_batches(lvm, po, hip, dev, idx, w, h, levels, ns, calls, over, clip_over)


@pytest.mark.parametrize("idx,w,h,levels,name", _riesz(M.CHROMA_LAYOUTS))
def test_riesz_chroma_layouts_exact(lvm, po, hip, dev, ptrig, idx, w, h, levels, name):
    M.chroma_layout(lvm, po, hip, dev, idx, w, h, levels, name)


@pytest.mark.parametrize("kind", M.CHROMA_FORCED_KINDS)
def test_riesz_chroma_forced_strip_kernels_exact(lvm, po, hip, dev, ptrig, kind):
    M.chroma_forced(lvm, po, hip, dev, kind, "rz_strips", ptrig=True)


# ---- layouts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx,w,h,levels,ns,name", _riesz(M.LAYOUT_CASES), ids=_ids(_riesz(M.LAYOUT_CASES)))
def test_riesz_layout_exact(lvm, po, hip, dev, ptrig, idx, w, h, levels, ns, name):
    M.layout_case(lvm, po, hip, dev, idx, w, h, levels, ns, name)


@pytest.mark.parametrize("name", ["B", "C", "D"])
def test_riesz_layout_forced_strip_kernels_exact(lvm, po, hip, dev, ptrig, name):
    M.layout_forced_case(lvm, po, hip, dev, "rz_strips", name, ptrig=True)


# ---- many streams, full-length batches, surfaces that lie far apart (parity_matrix.MANY_*, FAR_*) -------------------------------------------
_MANY_RZ = _riesz(M.MANY_CASES)


@pytest.mark.parametrize("idx,w,h,levels,ns", _MANY_RZ, ids=_ids(_MANY_RZ))
def test_riesz_many_streams_full_batches_exact(lvm, po, hip, dev, ptrig, idx, w, h, levels, ns):
    M.many_streams_case(lvm, po, hip, dev, idx, w, h, levels, ns, refs="ptrig")


def test_riesz_many_streams_kernels_chosen_without_forcing(lvm, po, hip, dev, ptrig):
    """16 streams x 32 frames once more with the call of 32 frames profiled: the printed record says which kernels these small frames
    reached unforced (the choice counts the CUs: no assertion on it)"""
    _, w, h, levels = _MANY_RZ[0][:4]
    calls = M.many_calls(2)
    names = M.many_streams_case(lvm, po, hip, dev, 2, w, h, levels, 16, refs="ptrig", profile_call=calls.index(32))
    print("unforced at 16 streams x 32 frames, mode 2", (w, h, levels), {n: sorted(v) for n, v in sorted(names.items())})


@pytest.mark.parametrize("idx,ns", _riesz(M.MANY_PER_FRAME), ids=_ids(_riesz(M.MANY_PER_FRAME)))
def test_riesz_many_streams_per_frame_schedule_exact(lvm, po, hip, dev, ptrig, idx, ns):
    M.many_per_frame(lvm, po, hip, dev, idx, ns, refs="ptrig")


def test_riesz_five_streams_forced_strip_kernels_exact(lvm, po, hip, dev, ptrig):
    _, launched = M.many_forced(lvm, po, hip, dev, "rz_strips", ptrig=True)
    print("five streams, forced rz_strips launched as asserted:", launched)


def test_riesz_many_streams_default_flavour_within_the_bars(lvm, po, hip, dev):
    """what bench.py runs is the default flavour (device sine / cosine, the oracle on libm): 16 streams x 16 frames at the bars of
    helpers.layout_clip (1 LSB, >= 0.999 identical)"""
    _, w, h, levels = _MANY_RZ[0][:4]
    ns, nf = M.MANY_DEFAULT
    worst = M.many_streams_case(lvm, po, hip, dev, 2, w, h, levels, ns, tail=(nf,), exact=False)
    print("default flavour, mode 2 %d streams x %d frames vs oracle: worst u8 diff %d, worst identical fraction %.6f" % ((ns, nf) + tuple(worst)))


@pytest.mark.parametrize("key", [k for k, c in M.FAR_CASES.items() if c[0] == 2])
def test_riesz_far_surfaces_exact(lvm, po, hip, dev, ptrig, key):
    print("far surfaces", key, "launched:", M.far_case(lvm, po, hip, dev, key, refs="ptrig", ptrig=M.FAR_CASES[key][4] is not None))


# ---- switches -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [k for k, c in M.SWITCH_CASES.items() if c["idx"] == 2])
def test_riesz_switch_case_against_the_oracle(lvm, po, hip, dev, ptrig, key):
    """(tests/test_gpu_switches.py keeps the comparison against the default kernels; the ledger key differs, so neither run stands in
    for the other)"""
    M.switch_case(lvm, po, hip, dev, "gpu-ptrig", key, reference="oracle")


# ---- phase on gray ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strips", [False, True], ids=["default", "strips"])
@pytest.mark.parametrize("w,h,levels", pg.SHAPES)
def test_gray_phase_is_the_oracle_on_the_expanded_frames_exact(lvm, po, hip, dev, ptrig, w, h, levels, strips, monkeypatch):
    """BGR2GRAY(oracle(expand(g))) with equality: per frame, in batches, two streams; the strip output kernel forced"""
    if strips:
        monkeypatch.setenv("LVM_RZ_COLLAPSE_STRIPS_MIN", "1")
    frames, pk = pg.gray_clip(lvm, po, w, h, levels), pg.params(lvm, w, h, levels)
    refs = pg.clip_reference(lvm, po, w, h, levels, portable_trig=True)
    pg.assert_not_vacuous(frames, refs)
    ctx = pg.context(lvm, hip, 1, "exact")
    try:
        gray_per_frame(lvm, ctx, frames, pk, refs)
    finally:
        ctx.close()
    gray_batched(lvm, hip, [frames], pk, [refs], mem=dev)
    other = pg.gray_clip(lvm, po, w, h, levels, seed=1235)
    gray_batched(lvm, hip, [frames, other], pk, [refs, pg.clip_reference(lvm, po, w, h, levels, seed=1235, portable_trig=True)], mem=dev)


# ---- one production size --------------------------------------------------------------------------------------------------------------
PRODUCTION = (1920, 1080, 6)
PRODUCTION_CALLS = (1, 5)


def test_production_size_picks_the_strip_kernels_and_equals_the_oracle(lvm, po, hip, dev, ptrig):
    """1920 x 1080, six levels, one stream, lvm_process_device_frames: without forcing, the launch heuristics pick the strip kernels only
    at such sizes -- the strip output kernel from 10^7 plane-pixels per launch (LVM_RZ_COLLAPSE_STRIPS_MIN's default), which five frames
    of 1080p are and four are not: calls of (1, 5) frames, the oracle renders six.  The second call is profiled: rz_final ran as
    `strips`, the strip form of the blur / amplify stage as `ptrig`.  The shipped build of the output kernels (no float frame kept) owes
    the bytes of every frame, a float-keeping context the float frame at the head of the batch.  A store hazard that leaves a few
    hundred wrong pixels in a frame of this size fails here."""
    w, h, levels = PRODUCTION
    ck, pk = lvm.synth.config(2, PRODUCTION)
    clip = lvm.synth.Clip(**ck)
    n = sum(PRODUCTION_CALLS)
    fin = np.stack([clip.frame(t) for t in range(n)])
    P, cp = po.make_params(**pk), c_params(lvm, pk)
    orc = po.Oracle()
    refs = []
    try:
        for t in range(n):
            ref, pr = orc.process(fin[t], P)
            refs.append((pr, np.array(ref, copy=True), orc.last_float().copy() if pr else None))
    finally:
        orc.close()
    assert [r[0] for r in refs] == [False] + [True] * (n - 1)
    fb = w * h * 3
    d_in = dev.upload(fin)
    for keep in (False, True):
        ctx = lvm.Context(0, 1, hip)
        try:
            ctx.exact_lab(True)
            ctx.keep_float(keep)
            d_out = dev.zeros_like(d_in)
            t = 0
            for k, nf in enumerate(PRODUCTION_CALLS):
                ctx.profile(k == 1)
                prod = ctx.process_device_frames(cp, nf, dev.ptr(d_in, t), w, h, 3, w * 3, fb, fb, dev.ptr(d_out, t), w * 3, fb, fb, dev.stream())
                dev.sync(ctx)
                assert list(prod) == [r[0] for r in refs[t:t + nf]], (k, prod)
                if keep and prod[0]:
                    fg = ctx.read_float((h, w, 3))
                    assert np.array_equal(refs[t][2], fg), "frame %d: %d float values differ from the oracle" % (t, int((refs[t][2] != fg).sum()))
                t += nf
            variants = ctx.profile_variants()
            names = {nm: variants.get(nm, set()) for nm in ctx.profile_collect()}
            assert names.get("rz_final") == {"strips"}, names
            assert names.get("rz_blur_amp") == {"ptrig"} and "rz_blur_amp_tiles" not in names, names
            M.ptrig_launches(names)
            got = dev.download(d_out)
            for t in range(1, n):
                assert np.array_equal(refs[t][1], got[t]), "keep_float=%s frame %d: %d bytes differ from the oracle" % (
                    keep, t, int((refs[t][1] != got[t]).sum()))
        finally:
            ctx.close()
