"""The gfx950 build held to bit-exact parity where its arithmetic allows it.

Every translation unit is built with -ffp-contract=off and IEEE division / sqrt, every fused multiply-add is spelled, and the
Laplace and Color paths call no transcendental function in the exact flavour (lvm_debug_exact_lab), the forward Lab conversion
is integer arithmetic.  So on the MI355X, as in the emulation build, those modes must give the oracle's float frames and bytes
exactly:
  (1) the Laplace and Color cases of the emulation matrix (tests/parity_matrix.py), the Laplace and Color seeds of the random
      sweep at both scales, the analytic flavour, and the big frames where the default heuristics pick other kernels;
  (2) in the default (shipped) flavour the GPU must give the emulation build's bytes and floats -- the only bit-level check the
      shipped flavour can have (the oracle has no fast mode), and a check that results do not depend on the grid size (the
      emulation reports 3 CUs);
  (3) Riesz calls acosf / sinf / cosf, where device library and glibc need not agree to the last ulp: every kernel variant must
      give the default kernels' float frames and bytes on the same GPU, in both flavours;
  (4) the variant switches really select the kernels they name (profiling report names)."""
import numpy as np
import pytest

import content
import parity_matrix as M
from helpers import STEPS_U8_FRAC, TorchMem, c_params, frames_clip, padded_strides_clip, pipelined_clip, run_pair, two_streams_clip
from test_emu_random import configure, draw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return TorchMem()


# ---- (1) exact flavour: Laplace and Color equal the oracle bit for bit --------------------------------------------------------
@pytest.mark.parametrize("w,h,levels,ch", M.LAPLACE_SHAPES)
def test_laplace_exact(lvm, po, hip, w, h, levels, ch):
    M.laplace_shape(lvm, po, hip, w, h, levels, ch)


@pytest.mark.parametrize("idx,w,h,levels", M.no_riesz(M.ANALYTIC))
def test_laplace_analytic_flavour_exact(lvm, po, hip, idx, w, h, levels, monkeypatch):
    M.analytic_flavour(lvm, po, hip, monkeypatch, idx, w, h, levels)


def test_laplace_param_changes_and_reset_exact(lvm, po, hip):
    M.laplace_param_changes_and_reset(lvm, po, hip)


def test_laplace_two_streams_exact(lvm, po, hip, dev):
    two_streams_clip(lvm, po, hip, dev)


@pytest.mark.parametrize("w,h,levels", M.PIPELINED)
def test_laplace_pipelined_exact(lvm, po, hip, dev, w, h, levels):
    pipelined_clip(lvm, po, hip, dev, w, h, levels, 11)


@pytest.mark.parametrize("w,h,levels", M.FUSED_MULTI)
def test_laplace_fused_multi_level_pyrdown_exact(lvm, po, hip, w, h, levels):
    M.laplace_shape_3_frames(lvm, po, hip, w, h, levels)


@pytest.mark.parametrize("rows", M.FIN_ROWS)
def test_laplace_final_kernel_strip_heights_exact(lvm, po, hip, rows, monkeypatch):
    M.laplace_final_strip_height(lvm, po, hip, monkeypatch, rows)


@pytest.mark.parametrize("w,h,levels", M.ROWS_PYRDOWN)
def test_laplace_wave_strip_pyrdown_exact(lvm, po, hip, w, h, levels, monkeypatch):
    M.laplace_wave_strip_pyrdown(lvm, po, hip, monkeypatch, w, h, levels)


@pytest.mark.parametrize("idx,w,h,levels", M.FIRST_KERNEL)
def test_wave_strip_first_kernel_exact(lvm, po, hip, idx, w, h, levels, monkeypatch):
    M.wave_strip_first_kernel(lvm, po, hip, monkeypatch, idx, w, h, levels)


@pytest.mark.parametrize("w,h,levels,exact", M.FUSED_TABLE)
def test_fused_table_conversion_and_first_kernel_exact(lvm, po, hip, w, h, levels, exact, monkeypatch):
    M.fused_table_first_kernel(lvm, po, hip, monkeypatch, w, h, levels, exact)


def test_unfused_conversion_in_batches_exact(lvm, po, hip, dev, monkeypatch):
    M.unfused_conversion_in_batches(lvm, po, hip, dev, monkeypatch)


@pytest.mark.parametrize("w,h,levels,ns,calls", M.LEVEL1_GEOMETRIES)
def test_laplace_level1_step_and_last_kernel_geometries_exact(lvm, po, hip, dev, w, h, levels, ns, calls):
    frames_clip(lvm, po, hip, dev, 0, w, h, levels, ns, calls)


def test_laplace_parameter_change_between_calls_exact(lvm, po, hip):
    M.laplace_param_change_between_calls(lvm, po, hip)


def test_fused_conversion_in_batches_two_streams_exact(lvm, po, hip, dev, monkeypatch):
    M.fused_conversion_two_streams(lvm, po, hip, dev, monkeypatch)


@pytest.mark.parametrize("w,h,levels,ns,calls", M.LAPLACE_BATCHES)
def test_laplace_temporal_batches_exact(lvm, po, hip, dev, w, h, levels, ns, calls):
    frames_clip(lvm, po, hip, dev, 0, w, h, levels, ns, calls)


@pytest.mark.parametrize("w,h,levels,ns,calls", M.SPLIT_LEVELS)
def test_laplace_split_levels_iir_and_collapse_exact(lvm, po, hip, dev, w, h, levels, ns, calls):
    frames_clip(lvm, po, hip, dev, 0, w, h, levels, ns, calls)


@pytest.mark.parametrize("w,h,levels,ns,calls", M.SPLIT_FROM_2)
def test_laplace_split_from_level_2_exact(lvm, po, hip, dev, w, h, levels, ns, calls, monkeypatch):
    M.laplace_split_from_2(lvm, po, hip, dev, monkeypatch, w, h, levels, ns, calls)


def test_laplace_level_chain_exact(lvm, po, hip, dev, monkeypatch):
    M.laplace_level_chain(lvm, po, hip, dev, monkeypatch)


@pytest.mark.parametrize("w,h,levels,calls", M.BLOCK_UP)
def test_laplace_block_up_kernel_variants_exact(lvm, po, hip, dev, w, h, levels, calls):
    frames_clip(lvm, po, hip, dev, 0, w, h, levels, 1, calls)


def test_laplace_tiled_up_kernel_exact(lvm, po, hip, dev, monkeypatch):
    M.laplace_tiled_up(lvm, po, hip, dev, monkeypatch)


@pytest.mark.parametrize("w,h,levels,ch,fps", M.COLOR_SHAPES)
def test_color_exact(lvm, po, hip, w, h, levels, ch, fps):
    M.color_shape(lvm, po, hip, w, h, levels, ch, fps)


@pytest.mark.parametrize("w,h,levels,rows", M.COL_OUT_ROWS)
def test_color_output_kernel_variants_exact(lvm, po, hip, w, h, levels, rows, monkeypatch):
    M.color_12_frames(lvm, po, hip, monkeypatch, w, h, levels, {"LVM_COL_OUT_ROWS": rows, "LVM_COL_OUT_MIN_TASKS": "0"})


@pytest.mark.parametrize("w,h,levels", M.COL_STRIP_BORDERS)
def test_color_strip_kernel_border_lanes_exact(lvm, po, hip, w, h, levels, monkeypatch):
    M.color_12_frames(lvm, po, hip, monkeypatch, w, h, levels, {"LVM_COL_OUT_MIN_TASKS": "0"})


@pytest.mark.parametrize("w,h,levels", M.COL_PREVIOUS_STRIPS)
def test_color_previous_strip_kernels_exact(lvm, po, hip, w, h, levels, monkeypatch):
    M.color_12_frames(lvm, po, hip, monkeypatch, w, h, levels, {"LVM_COL_OUT_LEAN": "0", "LVM_COL_OUT_MIN_TASKS": "0"})


def test_color_one_level_exact(lvm, po, hip, monkeypatch):
    M.color_12_frames(lvm, po, hip, monkeypatch, 128, 48, 1, {"LVM_COL_OUT_MIN_TASKS": "0"})


@pytest.mark.parametrize("w,h,levels,rows", M.COL_DOWN01_ROWS)
def test_color_first_two_levels_in_one_pass_exact(lvm, po, hip, w, h, levels, rows, monkeypatch):
    M.color_12_frames(lvm, po, hip, monkeypatch, w, h, levels,
                      {"LVM_D0_MIN_TASKS": "0", "LVM_COL_DOWN01_ROWS": rows, "LVM_COL_OUT_MIN_TASKS": "0"})


def test_color_two_level_pass_switched_off_exact(lvm, po, hip, monkeypatch):
    M.color_12_frames(lvm, po, hip, monkeypatch, 264, 90, 3, {"LVM_D0_MIN_TASKS": "0", "LVM_COL_DOWN01": "0"})


def test_color_wide_band_and_fps_change_exact(lvm, po, hip):
    M.color_wide_band_and_fps_change(lvm, po, hip)


@pytest.mark.parametrize("w,h,levels,ns,calls", M.COLOR_BATCHES)
def test_color_temporal_batches_exact(lvm, po, hip, dev, w, h, levels, ns, calls):
    frames_clip(lvm, po, hip, dev, 3, w, h, levels, ns, calls, *M.COLOR_BATCH_PARAMS)


@pytest.mark.parametrize("lo,hi", M.NARROW_DFT_BANDS)
@pytest.mark.parametrize("thin8", ["1", "0"])
def test_color_narrow_band_dft_exact(lvm, po, hip, dev, lo, hi, thin8, monkeypatch):
    M.color_narrow_band_dft(lvm, po, hip, dev, monkeypatch, lo, hi, thin8)


def test_color_frames_api_falls_back_frame_by_frame_exact(lvm, po, hip, dev):
    frames_clip(lvm, po, hip, dev, 3, 96, 64, 3, 1, (4, 3))


@pytest.mark.parametrize("idx,pad_in,pad_out", M.no_riesz(M.PADDED_STRIDES))
def test_padded_row_strides_exact(lvm, po, hip, dev, idx, pad_in, pad_out):
    padded_strides_clip(lvm, po, hip, dev, idx, pad_in, pad_out)


@pytest.mark.parametrize("idx,const_from,size", M.no_riesz(M.FLAT_REGIONS))
def test_flat_regions_and_constant_frames_exact(lvm, po, hip, idx, const_from, size):
    M.flat_regions(lvm, po, hip, idx, const_from, size)


@pytest.mark.parametrize("idx", [0, 3])
def test_fully_constant_clip_exact(lvm, po, hip, idx):
    M.fully_constant_clip(lvm, po, hip, idx)


@pytest.mark.parametrize("idx,over", M.no_riesz(M.EXTREME_PARAMETERS))
def test_extreme_parameters_exact(lvm, po, hip, idx, over):
    M.extreme_parameters(lvm, po, hip, idx, over)


@pytest.mark.parametrize("idx", [0, 3])
def test_size_and_channel_changes_exact(lvm, po, hip, idx):
    M.size_and_channel_changes(lvm, po, hip, idx)


def test_laplace_color_mode_switch_exact(lvm, po, hip):
    ck, pk0 = lvm.synth.config(0, (96, 64, 3))
    _, pk3 = lvm.synth.config(3, (96, 64, 3))
    run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk0, 12, 0.0, exact=True, param_fn=lambda t, p: dict([pk0, pk3, pk0][(t // 4) % 3]))


# chromatic content (tests/content.py): Laplace and Color bit for bit; the Riesz entries of the forced, batched and layout cases at the
# bars of helpers.layout_clip, as tests/test_layouts.py holds them (the Riesz shapes: tests/test_gpu_parity.py)
@pytest.mark.parametrize("kind,idx,w,h,levels", [c for c in M.CHROMA_CASES if c[1] != 2])
def test_chroma_exact(lvm, po, hip, kind, idx, w, h, levels):
    M.chroma_shape(lvm, po, hip, kind, idx, w, h, levels)


def test_chroma_gray_frames_exact(lvm, po, hip):
    M.chroma_gray(lvm, po, hip)


@pytest.mark.parametrize("kind,force", M.CHROMA_FORCED_CASES)
def test_chroma_forced_strip_kernels(lvm, po, hip, dev, kind, force):
    riesz = M.LAYOUT_FORCED[force][0] == 2
    worst, launched = M.chroma_forced(lvm, po, hip, dev, kind, force, exact=not riesz)
    print("chroma forced", kind, force, "launched as asserted:", launched)
    if riesz:
        print("chroma forced", kind, force, "vs oracle: worst u8 diff %d, worst identical fraction %.6f" % tuple(worst))


@pytest.mark.parametrize("kind", M.CHROMA_FORCED_KINDS)
def test_chroma_final_kernel_strips_of_8_rows_exact(lvm, po, hip, kind, monkeypatch):
    M.laplace_final_strip_height(lvm, po, hip, monkeypatch, 8, kind=kind)


@pytest.mark.parametrize("kind,idx,w,h,levels", M.CHROMA_ANALYTIC)
def test_chroma_analytic_flavour(lvm, po, hip, kind, idx, w, h, levels, monkeypatch):
    worst = M.analytic_flavour(lvm, po, hip, monkeypatch, idx, w, h, levels, kind=kind, exact=idx != 2)
    if idx == 2:
        print("chroma analytic riesz", kind, (w, h, levels), "worst rel/u8/frac, shipped u8/frac", worst)


@pytest.mark.parametrize("idx,w,h,levels,ns,calls,over,clip_over", M.CHROMA_BATCHES)
def test_chroma_temporal_batches(lvm, po, hip, dev, idx, w, h, levels, ns, calls, over, clip_over):
    worst = M.chroma_batches(lvm, po, hip, dev, idx, w, h, levels, ns, calls, over, clip_over, exact=idx != 2)
    if idx == 2:
        print("chroma riesz batches vs oracle: worst u8 diff %d, worst identical fraction %.6f" % tuple(worst))


@pytest.mark.parametrize("idx,w,h,levels,name", M.CHROMA_LAYOUTS)
def test_chroma_layouts(lvm, po, hip, dev, idx, w, h, levels, name):
    worst, _ = M.chroma_layout(lvm, po, hip, dev, idx, w, h, levels, name, exact=idx != 2)
    if idx == 2:
        print("chroma riesz layout", name, "vs oracle: worst u8 diff %d, worst identical fraction %.6f" % tuple(worst))


def test_chroma_far_out_of_gamut_exact(lvm, po, hip):
    M.chroma_out_of_gamut(lvm, po, hip)


# many streams, full-length batches, surfaces that lie far apart (parity_matrix.MANY_*, FAR_*): the schedules bench.py runs -- 4 and 16 streams,
# calls of 16 and 32 frames, the per-frame loop, the 4-stream depth-1 pipeline -- and 5 and 17 streams, on grids, LDS and 64-bit address
# arithmetic of the gfx950 build.  Laplace and Color here, Riesz in tests/test_gpu_riesz_exact.py.
def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


_MANY_LC = M.no_riesz(M.MANY_CASES)


@pytest.mark.parametrize("idx,w,h,levels,ns", _MANY_LC, ids=_ids(_MANY_LC))
def test_many_streams_full_batches_exact(lvm, po, hip, dev, idx, w, h, levels, ns):
    M.many_streams_case(lvm, po, hip, dev, idx, w, h, levels, ns)


@pytest.mark.parametrize("idx", [0, 3])
def test_many_streams_kernels_chosen_without_forcing(lvm, po, hip, dev, idx):
    """16 streams x 32 frames once more with the call of 32 frames profiled: the printed record says which kernels these small frames
    reached unforced (the choice counts the CUs: no assertion on it)"""
    _, w, h, levels = [s for s in M.MANY_SHAPES if s[0] == idx and s[1] % 4 == 0][-1]
    calls = M.many_calls(idx)
    names = M.many_streams_case(lvm, po, hip, dev, idx, w, h, levels, 16, profile_call=calls.index(32))
    print("unforced at 16 streams x 32 frames, mode", idx, (w, h, levels), {n: sorted(v) for n, v in sorted(names.items())})


@pytest.mark.parametrize("idx,ns", M.no_riesz(M.MANY_PER_FRAME), ids=_ids(M.no_riesz(M.MANY_PER_FRAME)))
def test_many_streams_per_frame_schedule_exact(lvm, po, hip, dev, idx, ns):
    M.many_per_frame(lvm, po, hip, dev, idx, ns)


@pytest.mark.parametrize("nframes,ring", M.MANY_PIPELINE, ids=_ids(M.MANY_PIPELINE))
def test_four_streams_pipelined_exact(lvm, po, hip, dev, nframes, ring):
    pipelined_clip(lvm, po, hip, dev, 64, 48, 3, nframes, ring=ring, n_streams=4)


@pytest.mark.parametrize("force", [f for f, c in M.LAYOUT_FORCED.items() if c[0] != 2])
def test_five_streams_forced_strip_kernels_exact(lvm, po, hip, dev, force):
    _, launched = M.many_forced(lvm, po, hip, dev, force)
    print("five streams, forced", force, "launched as asserted:", launched)


@pytest.mark.parametrize("idx", [0, 3])
def test_many_streams_default_flavour_within_the_bars(lvm, po, hip, dev, idx):
    """what bench.py runs is the default flavour: 16 streams x 16 frames at the bars of helpers.layout_clip (1 LSB, >= 0.999 identical)"""
    _, w, h, levels = [s for s in M.MANY_SHAPES if s[0] == idx][-1]
    ns, nf = M.MANY_DEFAULT
    worst = M.many_streams_case(lvm, po, hip, dev, idx, w, h, levels, ns, tail=(nf,), exact=False)
    print("default flavour, mode", idx, "%d streams x %d frames vs oracle: worst u8 diff %d, worst identical fraction %.6f" % ((ns, nf) + tuple(worst)))


@pytest.mark.parametrize("key", [k for k, c in M.FAR_CASES.items() if c[0] != 2])
def test_far_surfaces_exact(lvm, po, hip, dev, key):
    print("far surfaces", key, "launched:", M.far_case(lvm, po, hip, dev, key))


@pytest.mark.parametrize("surface", list(M.FAR_SURFACES))
def test_far_units_of_the_other_device_surfaces(lvm, po, hip, dev, surface):
    M.FAR_SURFACES[surface](lvm, po, hip, dev)


LC_SEEDS = [s for s in range(24) if draw(s)[1] != 2]


@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("seed", LC_SEEDS)
def test_random_laplace_color_exact(lvm, po, hip, seed, scale):
    """the Laplace and Color seeds of tests/test_emu_random.py, at the emulation's size and at four times it"""
    ck, pk, vary = configure(lvm, seed, scale)
    run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 7, 0.0, exact=True, param_fn=vary)


@pytest.mark.parametrize("w,h,levels", [(640, 360, 4), (323, 211, 5), (1920, 1080, 6)])
def test_laplace_analytic_flavour_default_kernels_exact(lvm, po, hip, w, h, levels):
    """the analytic flavour with the launch code's own kernel choice (the matrix above forces the strip first kernel)"""
    ck, pk = lvm.synth.config(0, (w, h, levels))
    run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 4 if w > 1000 else 8, 0.0, exact=True, analytic=True)


def test_laplace_1080p_exact(lvm, po, hip, dev):
    """1080p, 6 levels, default heuristics: per-frame calls (float frame and bytes), then a call of 32 frames (lap_down0_lut,
    pyr_down_rows, the split IIR / collapse levels, k_lap_final_v4)."""
    ck, pk = lvm.synth.config(0, (1920, 1080, 6))
    run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 3, 0.0, exact=True)
    frames_clip(lvm, po, hip, dev, 0, 1920, 1080, 6, 1, (1, 32))


def test_laplace_4k_8_levels_exact(lvm, po, hip, dev):
    """3840 x 2160, 8 levels, temporal batches (test_gpu_schedules.py::test_laplace_4k_8_levels_temporal_batches at the exact bar)"""
    frames_clip(lvm, po, hip, dev, 0, 3840, 2160, 8, 1, (1, 5, 5))


def test_color_1080p_window_and_batches_exact(lvm, po, hip, dev):
    """1080p, 6 levels, 60 fps (a window of 128 columns): per-frame calls and batches until the window is full, then batches of 32
    (k_down01_rows, the _u2 minmax / output kernels unforced)."""
    frames_clip(lvm, po, hip, dev, 3, 1920, 1080, 6, 1, (1, 1, 30, 32, 32, 32, 32))


# ---- (2) default flavour: the GPU gives the emulation build's bytes and floats ------------------------------------------------
def _run_lib(lvm, lib, clip, pk, nframes, keep_float, param_fn=None):
    ctx = lvm.Context(0, 1, lib)
    ctx.keep_float(keep_float)
    got = []
    try:
        for t in range(nframes):
            p = param_fn(t, dict(pk)) if param_fn else pk
            f = clip.frame(t)
            out, pr = ctx.process(f, c_params(lvm, p))
            got.append((pr, np.array(out, copy=True), ctx.read_float(f.shape).copy() if pr and keep_float else None))
    finally:
        ctx.close()
    return got


def _assert_same(a, b, what):
    for t, ((pa, ua, fa), (pb, ub, fb)) in enumerate(zip(a, b)):
        assert pa == pb, "%s frame %d: produced %s vs %s" % (what, t, pa, pb)
        if not pa:
            continue
        bad = np.argwhere(ua != ub)
        assert len(bad) == 0, "%s frame %d: %d bytes differ, first at %s (%d vs %d)" % (
            what, t, len(bad), tuple(bad[0]), int(ua[tuple(bad[0])]), int(ub[tuple(bad[0])]))
        if fa is not None:
            bad = np.argwhere(fa.view(np.uint32) != fb.view(np.uint32))
            assert len(bad) == 0, "%s frame %d: %d float values differ, first at %s (%r vs %r)" % (
                what, t, len(bad), tuple(bad[0]), float(fa[tuple(bad[0])]), float(fb[tuple(bad[0])]))


SHIPPED_CASES = [(0, (640, 360, 5), {}), (0, (323, 211, 4), {}), (0, (135, 77, 4), {}), (0, (100, 64, 2), {"channels": 1}),
                 (0, (328, 109, 3), {"LVM_D0_MIN_TASKS": "0"}), (0, (328, 109, 3), {"LVM_D0_FUSED_WAVES": "1"}),
                 (0, (328, 109, 3), {"LVM_ROWS_MIN_ELEMS": "0"}), (0, (328, 125, 3), {"LVM_FIN_ROWS": "8", "LVM_FIN_MIN_TASKS": "0"}),
                 (3, (320, 180, 4), {}), (3, (264, 90, 3), {"LVM_COL_OUT_ROWS": "8", "LVM_COL_OUT_MIN_TASKS": "0"}),
                 (3, (520, 52, 3), {"LVM_D0_MIN_TASKS": "0", "LVM_COL_DOWN01_ROWS": "7", "LVM_COL_OUT_MIN_TASKS": "0"}),
                 (3, (264, 90, 3), {"LVM_COL_OUT_LEAN": "0", "LVM_COL_OUT_MIN_TASKS": "0"})]


def _shipped_case(lvm, hip, emu, idx, size, env, monkeypatch, kind=None):
    chans = env.get("channels", 3)
    for k, v in env.items():
        if k.startswith("LVM_"):
            monkeypatch.setenv(k, v)
    ck, pk = lvm.synth.config(idx, size)
    ck["channels"] = chans
    if idx == 3:
        ck["fps"] = 15.0; pk["framerate"] = 15.0
    clip = lvm.synth.Clip(**ck) if kind is None else content.chroma_clip(lvm, ck, kind)
    n = 14 if idx == 3 else 6
    for keep in (False, True):
        _assert_same(_run_lib(lvm, hip, clip, pk, n, keep), _run_lib(lvm, emu, clip, pk, n, keep), "keep_float=%s" % keep)


@pytest.mark.parametrize("idx,size,env", SHIPPED_CASES)
def test_shipped_flavour_gpu_equals_emulation(lvm, hip, emu, idx, size, env, monkeypatch):
    """Same frames through both builds in the shipped configuration (identical u8 frames) and with keep_float (identical float
    frames and bytes); a few forced variants."""
    _shipped_case(lvm, hip, emu, idx, size, env, monkeypatch)


CHROMA_SHIPPED_CASES = [SHIPPED_CASES[1], SHIPPED_CASES[5], SHIPPED_CASES[7], SHIPPED_CASES[11]]


@pytest.mark.parametrize("kind", ["noise", "hue"])
@pytest.mark.parametrize("idx,size,env", CHROMA_SHIPPED_CASES)
def test_shipped_flavour_gpu_equals_emulation_on_chromatic_content(lvm, hip, emu, idx, size, env, kind, monkeypatch):
    """The same on saturated colours: the only bit-level check the shipped flavour's colour arithmetic (reciprocal multiplies, packed
    Lab2BGR, the gfx950 spellings of lvm_gfx950.h against the C of the emulation header) can have."""
    _shipped_case(lvm, hip, emu, idx, size, env, monkeypatch, kind=kind)


class _Frames:
    def __init__(self, *frames):
        self.frames = frames

    def frame(self, t):
        return self.frames[t]


def test_shipped_flavour_gpu_equals_emulation_on_the_colour_cube(lvm, hip, emu):
    """Every triple of 64 values that take every cell of the table (content.cube_values): natural, permuted, natural as three frames
    of a Laplace clip, 3 levels."""
    nat, per = content.cube_frames(content.cube_values(64))
    clip = _Frames(nat, per, nat)
    _, pk = lvm.synth.config(0, (nat.shape[1], nat.shape[0], 3))
    for keep in (False, True):
        _assert_same(_run_lib(lvm, hip, clip, pk, 3, keep), _run_lib(lvm, emu, clip, pk, 3, keep), "keep_float=%s" % keep)


@pytest.mark.parametrize("idx,size,calls", [(0, (320, 180, 4), (1, 5, 3)), (0, (264, 74, 3), (1, 6, 1, 2)), (3, (80, 52, 3), (17, 16, 9))])
def test_shipped_flavour_batches_gpu_equals_emulation(lvm, hip, emu, dev, idx, size, calls):
    """short ragged temporal batches through lvm_process_device_frames, shipped configuration: identical bytes"""
    from helpers import HostMem
    ck, pk = lvm.synth.config(idx, size)
    if idx == 3:
        ck["fps"] = 7.0; pk.update(framerate=7.0, coLow=0.4, coHigh=2.0)
    clip = lvm.synth.Clip(**ck)
    frames = np.stack([clip.frame(t) for t in range(sum(calls))])
    w, h = ck["w"], ck["h"]
    fb = w * h * 3
    outs = []
    for lib, mem in ((hip, dev), (emu, HostMem())):
        ctx = lvm.Context(0, 1, lib)
        try:
            d_in = mem.upload(frames)
            d_out = mem.zeros_like(d_in)
            prod, t = [], 0
            for nf in calls:
                prod += ctx.process_device_frames(c_params(lvm, pk), nf, mem.ptr(d_in, t), w, h, 3, w * 3, fb, fb, mem.ptr(d_out, t), w * 3,
                                                  fb, fb, mem.stream())
                t += nf
            mem.sync(ctx)
            outs.append((prod, mem.download(d_out)))
        finally:
            ctx.close()
    (pa, a), (pb, b) = outs
    assert pa == pb and any(pa)
    for t in range(len(pa)):
        if pa[t]:
            assert np.array_equal(a[t], b[t]), "frame %d: %d bytes differ" % (t, int((a[t] != b[t]).sum()))


@pytest.mark.parametrize("seed", [s for s in LC_SEEDS if s < 12])
def test_random_shipped_flavour_gpu_equals_emulation(lvm, hip, emu, seed):
    ck, pk, vary = configure(lvm, seed)
    clip = lvm.synth.Clip(**ck)
    for keep in (False, True):
        _assert_same(_run_lib(lvm, hip, clip, pk, 7, keep, vary), _run_lib(lvm, emu, clip, pk, 7, keep, vary), "keep_float=%s" % keep)


# ---- (3) Riesz: every variant against the default kernels on the same GPU ----------------------------------------------------
RZ_VARIANTS = {
    "split_rows_10": {"LVM_RZ_SPLIT_ROWS_MIN": "1", "LVM_RZ_SPLIT_STRIP": "10"},
    "split_rows_54": {"LVM_RZ_SPLIT_ROWS_MIN": "1", "LVM_RZ_SPLIT_STRIP": "54"},
    "split_tiled": {"LVM_RZ_SPLIT_ROWS": "0", "LVM_RZ_SPLIT2_MIN": "1000000000"},
    "split2_phase4": {"LVM_RZ_SPLIT_ROWS": "0", "LVM_RZ_SPLIT2_MIN": "0", "LVM_RZ_PHASE4_MIN_FRAMES": "1"},
    "phase_narrow": {"LVM_RZ_PHASE4_MIN_FRAMES": "1000"},
    "blur4": {"LVM_RZ_BLUR_STRIPS": "0", "LVM_RZ_BLUR4": "1"},
    "blur_scalar": {"LVM_RZ_BLUR_STRIPS": "0", "LVM_RZ_BLUR4": "0"},
    "blur_strips_16": {"LVM_RZ_BLUR_STRIPS_MIN": "0", "LVM_RZ_BLUR_STRIP_ROWS": "16"},
    "blur_strips_64": {"LVM_RZ_BLUR_STRIPS_MIN": "0", "LVM_RZ_BLUR_STRIP_ROWS": "64"},
    "compact": {"LVM_RZ_COLLAPSE_STRIPS": "0", "LVM_RZ_COMPACT": "1"},
    "full_tile": {"LVM_RZ_COLLAPSE_STRIPS": "0", "LVM_RZ_COMPACT": "0"},
    "collapse_strips_10": {"LVM_RZ_COLLAPSE_STRIPS_MIN": "1", "LVM_RZ_COLLAPSE_STRIP": "10"},
    "collapse_strips_64": {"LVM_RZ_COLLAPSE_STRIPS_MIN": "1", "LVM_RZ_COLLAPSE_STRIP": "64"},
}
RZ_SHAPES = [(8, 4, 2), (128, 5, 2), (1000, 24, 2), (520, 70, 3), (256, 41, 2), (134, 78, 2), (67, 131, 2), (264, 150, 3), (512, 64, 4)]
RZ_CALLS = (1, 2, 1, 3)
_RZ_ENV = sorted({k for v in RZ_VARIANTS.values() for k in v})


def _riesz_run(lvm, lib, mem, monkeypatch, frames, pk, env, keep_float, exact):
    for k in _RZ_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n, h, w, _ = frames.shape
    fb = w * h * 3
    ctx = lvm.Context(0, 1, lib)
    ctx.keep_float(keep_float)
    ctx.exact_lab(exact)
    try:
        d_in = mem.upload(frames)
        d_out = mem.zeros_like(d_in)
        prod, floats, t = [], [], 0
        for nf in RZ_CALLS:
            prod += ctx.process_device_frames(c_params(lvm, pk), nf, mem.ptr(d_in, t), w, h, 3, w * 3, fb, fb, mem.ptr(d_out, t), w * 3,
                                              fb, fb, mem.stream())
            t += nf
            mem.sync(ctx)
            floats.append(ctx.read_float((h, w, 3)).copy() if keep_float and prod[t - nf] else None)   # the call's first frame
        return prod, mem.download(d_out), floats
    finally:
        ctx.close()


@pytest.mark.parametrize("w,h,levels", RZ_SHAPES)
def test_riesz_variants_equal_the_default_kernels(lvm, po, hip, dev, w, h, levels, monkeypatch):
    _riesz_variants(lvm, po, hip, dev, monkeypatch, w, h, levels)


@pytest.mark.parametrize("w,h,levels", [(264, 150, 3), (67, 131, 2)])
def test_riesz_variants_equal_the_default_kernels_on_chromatic_content(lvm, po, hip, dev, w, h, levels, monkeypatch):
    """the same on `noise` (tests/content.py): every variant's Lab planes and output kernels on saturated colours, both flavours"""
    _riesz_variants(lvm, po, hip, dev, monkeypatch, w, h, levels, kind="noise")


def _riesz_variants(lvm, po, hip, dev, monkeypatch, w, h, levels, kind=None):
    """Per shape: the default kernels and every LVM_RZ_* variant on the same frames and the same GPU, in temporal batches of 1 ... 3
    frames.  With keep_float: identical float frames (the first frame of every call) and identical bytes, in the exact and the
    default flavour.  Shipped configuration (u8 step table): identical bytes among the variants; against the float-keeping build
    of the same flavour at most 1 LSB with >= STEPS_U8_FRAC identical (the quantiser paragraph; bar of
    tests/helpers.py:3-6).  Every variant of the exact flavour also meets the oracle bars; the worst gap is printed."""
    ck, pk = lvm.synth.config(2, (w, h, levels))
    clip = lvm.synth.Clip(**ck) if kind is None else content.chroma_clip(lvm, ck, kind)
    n = sum(RZ_CALLS)
    frames = np.stack([clip.frame(t) for t in range(n)])
    orc = po.Oracle()
    P = po.make_params(**pk)
    refs = []
    try:
        for t in range(n):
            ref, pr = orc.process(frames[t], P)
            refs.append((pr, ref, orc.last_float().copy() if pr else None))
    finally:
        orc.close()
    first = np.cumsum((0,) + RZ_CALLS[:-1])
    base = {(kf, ex): _riesz_run(lvm, hip, dev, monkeypatch, frames, pk, {}, kf, ex) for kf in (True, False) for ex in (True, False)}
    worst = [0.0, 1.0]
    for name, env in [("default", {})] + list(RZ_VARIANTS.items()):
        for ex in (True, False):
            prod, u8, fl = base[(True, ex)] if name == "default" else _riesz_run(lvm, hip, dev, monkeypatch, frames, pk, env, True, ex)
            bprod, bu8, bfl = base[(True, ex)]
            assert prod == bprod == [r[0] for r in refs], (name, ex, prod)
            for t in range(n):
                if prod[t]:
                    assert np.array_equal(u8[t], bu8[t]), "%s exact=%s frame %d: %d bytes differ from the default kernels" % (
                        name, ex, t, int((u8[t] != bu8[t]).sum()))
            for c, t in enumerate(first):
                if fl[c] is not None:
                    assert np.array_equal(fl[c], bfl[c]), "%s exact=%s frame %d: %d float values differ from the default kernels" % (
                        name, ex, t, int((fl[c] != bfl[c]).sum()))
                    if ex:
                        fr = refs[t][2]
                        rel = float(np.abs(fr - fl[c]).max() / max(float(np.abs(fr).max()), 1e-30))
                        assert rel <= 1e-4, (name, t, rel)
                        worst[0] = max(worst[0], rel)
            for t in range(n):
                if prod[t]:
                    du = np.abs(refs[t][1].astype(np.int32) - u8[t].astype(np.int32))
                    assert du.max() <= 1 and (du == 0).mean() >= 0.999, (name, ex, t, int(du.max()), float((du == 0).mean()))
                    if ex:
                        worst[1] = min(worst[1], float((du == 0).mean()))
            sprod, su8, _ = base[(False, ex)] if name == "default" else _riesz_run(lvm, hip, dev, monkeypatch, frames, pk, env, False, ex)
            bsprod, bsu8, _ = base[(False, ex)]
            assert sprod == bsprod == prod, (name, ex)
            for t in range(n):
                if not sprod[t]:
                    continue
                assert np.array_equal(su8[t], bsu8[t]), "%s exact=%s shipped frame %d: %d bytes differ from the default kernels" % (
                    name, ex, t, int((su8[t] != bsu8[t]).sum()))
                dd = np.abs(su8[t].astype(np.int32) - u8[t].astype(np.int32))
                assert dd.max() <= 1 and (dd == 0).mean() >= STEPS_U8_FRAC, (name, ex, t, int(dd.max()), float((dd == 0).mean()))
    print("riesz", kind or "synth", (w, h, levels), "exact flavour vs oracle (acosf / sinf / cosf of the device library): worst float rel %.3e, "
          "worst identical u8 fraction %.6f" % tuple(worst))


# ---- (4) the variant switches select the kernels they name ---------------------------------------------------------------------
PROFILE_CASES = [
    (0, (328, 109, 3), 1, {"LVM_D0_FUSED_WAVES": "1"}, ["lap_down0_lut"], ["lap_down0", "lab_lut"]),
    (0, (328, 109, 3), 1, {"LVM_D0_FUSED": "0"}, ["lap_down0", "lab_lut"], ["lap_down0_lut"]),
    (0, (1920, 1080, 6), 4, {}, ["pyr_down_rows_l1"], []),
    (0, (328, 109, 3), 1, {"LVM_ROWS_MIN_ELEMS": "0"}, ["pyr_down_rows_l1"], ["pyr_down_l1", "pyr_down3_l1", "pyr_down2_l1"]),
    (0, (640, 360, 5), 6, {}, ["lap_iir", "lap_collapse"], ["lap_tail"]),
    (0, (320, 180, 4), 6, {"LVM_LAP_SPLIT": "0"}, [], ["lap_iir", "lap_collapse"]),
    (2, (264, 150, 3), 1, {"LVM_RZ_PHASE4_MIN_FRAMES": "1000"}, ["rz_phase_small"], ["rz_phase"]),
    (2, (1920, 1080, 6), 2, {}, ["rz_phase"], ["rz_phase_small"]),
    (2, (264, 150, 3), 1, {"LVM_RZ_BLUR_STRIPS": "0", "LVM_RZ_BLUR4": "0"}, ["rz_blur_amp_small"], ["rz_blur_amp"]),
    (3, (1920, 1080, 6), 2, {}, ["col_out_u2", "col_minmax_u2"], ["col_out"]),
    (3, (264, 90, 3), 1, {"LVM_COL_OUT_LEAN": "0", "LVM_COL_OUT_MIN_TASKS": "0"}, ["col_out"], ["col_out_u2"]),
]


def _launched(lvm, lib, mem, monkeypatch, idx, size, nf, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ck, pk = lvm.synth.config(idx, size)
    if idx == 3:
        ck["fps"] = 15.0; pk["framerate"] = 15.0
    clip = lvm.synth.Clip(**ck)
    w, h = ck["w"], ck["h"]
    fb = w * h * 3
    frames = np.stack([clip.frame(t) for t in range(1 + nf)])
    ctx = lvm.Context(0, 1, lib)
    ctx.profile(True)
    try:
        d_in = mem.upload(frames)
        d_out = mem.zeros_like(d_in)
        for t, k in ((0, 1), (1, nf)):
            ctx.process_device_frames(c_params(lvm, pk), k, mem.ptr(d_in, t), w, h, 3, w * 3, fb, fb, mem.ptr(d_out, t), w * 3, fb, fb,
                                      mem.stream())
        mem.sync(ctx)
        return set(ctx.profile_collect())
    finally:
        ctx.close()


@pytest.mark.parametrize("idx,size,nf,env,present,absent", PROFILE_CASES)
def test_variant_switches_select_the_named_kernels(lvm, hip, dev, idx, size, nf, env, present, absent, monkeypatch):
    names = _launched(lvm, hip, dev, monkeypatch, idx, size, nf, env)
    for p in present:
        assert p in names, (p, sorted(names))
    for a in absent:
        assert a not in names, (a, sorted(names))
