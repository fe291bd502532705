"""Kernel-logic parity on CPU: the product sources (csrc/*.hip) compiled against the HIP
emulation header (tests/emu) vs the CPU oracle, through the same C ABI.  Because the kernels
follow the oracle's operation order, the float frames must be BIT-IDENTICAL wherever no
transcendental is involved (the emulation build uses the host libm like the oracle does).
This validates tiling, border rules, odd sizes and state handling without a GPU; the real
gfx950 build is checked by tests/test_gpu_parity.py (-m gpu)."""
import numpy as np
import pytest

import parity_matrix as M
from helpers import HostMem, frames_clip, padded_strides_clip, pipelined_clip, run_pair, two_streams_clip

HOST = HostMem()


@pytest.mark.parametrize("w,h,levels,ch", M.LAPLACE_SHAPES)
def test_laplace_emu_bit_exact(lvm, po, emu, w, h, levels, ch):
    M.laplace_shape(lvm, po, emu, w, h, levels, ch)


@pytest.mark.parametrize("idx,w,h,levels", M.ANALYTIC)
def test_analytic_flavour_emu_bit_exact(lvm, po, emu, idx, w, h, levels, monkeypatch):
    M.analytic_flavour(lvm, po, emu, monkeypatch, idx, w, h, levels)


def test_laplace_emu_param_changes_and_reset(lvm, po, emu):
    M.laplace_param_changes_and_reset(lvm, po, emu)


def test_laplace_emu_two_streams_are_independent(lvm, po, emu):
    two_streams_clip(lvm, po, emu, HOST)


# ---- Riesz (phase) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,levels", M.RIESZ_SHAPES)
def test_riesz_emu_bit_exact(lvm, po, emu, w, h, levels):
    M.riesz_shape(lvm, po, emu, w, h, levels)


@pytest.mark.parametrize("w,h,levels,calls", M.RIESZ_TILE_KERNELS)
@pytest.mark.parametrize("wide", ["1", "0"])
def test_riesz_emu_wide_and_narrow_tile_kernels(lvm, po, emu, w, h, levels, calls, wide, monkeypatch):
    """Round 5 picks the tile kernels by launch size: k_rz_split2 (4 x 2 outputs per thread) from 600 000 plane-pixels per launch, else
    k_rz_split (one output per thread); k_rz_phase4 (four pixels per thread) from two frames x streams per launch, else k_rz_phase.  Both
    choices forced onto small frames -- per-frame calls between temporal batches, so that the state written by one phase kernel is read
    by the other."""
    M.riesz_wide_and_narrow_tile_kernels(lvm, po, emu, HOST, monkeypatch, w, h, levels, calls, wide)


@pytest.mark.parametrize("blur4", ["1", "0"])
def test_riesz_emu_register_blocked_blur(lvm, po, emu, blur4, monkeypatch):
    """k_rz_blur_amp4 (64 x 32 tiles, vector staging of interior tiles, 4 x 2 outputs per thread) against the
    scalar kernel's arithmetic: a frame with interior, edge and partial tiles on two levels."""
    M.riesz_register_blocked_blur(lvm, po, emu, monkeypatch, blur4)


@pytest.mark.parametrize("w,h,levels,rows,exact", M.RIESZ_STRIP_BLUR)
def test_riesz_emu_strip_blur(lvm, po, emu, w, h, levels, rows, exact, monkeypatch):
    """k_rz_blur_strips (three 13-tap Gaussians + amplify as wave strips: DPP halo exchange over three lanes either side, a
    13-row register window per plane) forced onto small levels: several strips per row with mirrored edge columns, a last
    strip ending short of the wave, strips shorter than the 12 halo rows, odd heights, level widths 2 mod 4.
    exact=False: the default flavour (hardware sine / cosine) against the parity bars."""
    M.riesz_strip_blur(lvm, po, emu, monkeypatch, w, h, levels, rows, exact)


def test_riesz_emu_strip_blur_in_temporal_batches(lvm, po, emu, monkeypatch):
    """Batched frames with the strip form forced onto every level: the phase kernel then stores no per-frame Riesz pair for
    those levels and the amplify stage recomputes it from the band (two streams, calls of several lengths)."""
    M.riesz_strip_blur_in_temporal_batches(lvm, po, emu, HOST, monkeypatch)


def test_riesz_emu_tiled_blur_still_matches(lvm, po, emu, monkeypatch):
    M.riesz_tiled_blur(lvm, po, emu, monkeypatch)


@pytest.mark.parametrize("compact", ["1", "0"])
def test_riesz_emu_collapse_tile_variants(lvm, po, emu, compact, monkeypatch):
    """The collapse kernels' zero-injected tile, compact (even rows / columns only; planes with even width and height) and
    full: interior (vector-staged) and border tiles on level 0, a plane with an odd height on level 1."""
    M.riesz_collapse_tile_variants(lvm, po, emu, monkeypatch, compact)


def test_riesz_emu_cutoff_change_gray_and_reset(lvm, po, emu):
    M.riesz_cutoff_change_gray_and_reset(lvm, po, emu)


# ---- Colour ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,levels,ch,fps", M.COLOR_SHAPES)
def test_color_emu_bit_exact(lvm, po, emu, w, h, levels, ch, fps):
    M.color_shape(lvm, po, emu, w, h, levels, ch, fps)


@pytest.mark.parametrize("w,h,levels,rows", M.COL_OUT_ROWS)
def test_color_emu_output_kernel_variants(lvm, po, emu, w, h, levels, rows, monkeypatch):
    """The vectorised output kernels: tiled (rows = 0) and wave strips of 2 ... 36 rows (k_col_out_strips: both pyrUps inside, window
    positions of two row slots each, U2 window in an LDS ring, buffer loads / stores), on heights the up chain overshoots (the
    bilinear row map skips source rows) and widths with a partly filled wave."""
    M.color_12_frames(lvm, po, emu, monkeypatch, w, h, levels, {"LVM_COL_OUT_ROWS": rows, "LVM_COL_OUT_MIN_TASKS": "0"})


@pytest.mark.parametrize("w,h,levels", M.COL_STRIP_BORDERS)
def test_color_emu_strip_kernel_border_lanes(lvm, po, emu, w, h, levels, monkeypatch):
    """k_col_out_strips: widths whose last strip holds one group (516: the U2 border column vw - 4 sits in the strip BEFORE the last
    one), interior strips (772), an exact multiple of the strip width."""
    M.color_12_frames(lvm, po, emu, monkeypatch, w, h, levels, {"LVM_COL_OUT_MIN_TASKS": "0"})


@pytest.mark.parametrize("w,h,levels", M.COL_PREVIOUS_STRIPS)
def test_color_emu_previous_strip_kernels_still_match(lvm, po, emu, w, h, levels, monkeypatch):
    """LVM_COL_OUT_LEAN=0: k_col_out_rows (the fallback for row maps that are not strictly increasing / one-level pyramids)."""
    M.color_12_frames(lvm, po, emu, monkeypatch, w, h, levels, {"LVM_COL_OUT_LEAN": "0", "LVM_COL_OUT_MIN_TASKS": "0"})


def test_color_emu_one_level_uses_the_single_pyrup_kernels(lvm, po, emu, monkeypatch):
    """levels = 1: no level-2 image exists, the strip kernels with one pyrUp inside run."""
    M.color_12_frames(lvm, po, emu, monkeypatch, 128, 48, 1, {"LVM_COL_OUT_MIN_TASKS": "0"})


@pytest.mark.parametrize("w,h,levels,rows", M.COL_DOWN01_ROWS)
def test_color_emu_first_two_levels_in_one_pass(lvm, po, emu, w, h, levels, rows, monkeypatch):
    """k_down01_rows (u8 -> level 2 without writing level 1; large launches only in production, forced here): strips of 1 ... 17
    level-2 rows -- top strip (mirrored level-1 rows -2, -1), interior strips, bottom rows with an even and an odd number of level-1
    rows (rows h1, h1 + 1 are window copies), one and several strips per row, the level-1 border columns."""
    M.color_12_frames(lvm, po, emu, monkeypatch, w, h, levels,
                      {"LVM_D0_MIN_TASKS": "0", "LVM_COL_DOWN01_ROWS": rows, "LVM_COL_OUT_MIN_TASKS": "0"})


def test_color_emu_two_level_pass_can_be_switched_off(lvm, po, emu, monkeypatch):
    M.color_12_frames(lvm, po, emu, monkeypatch, 264, 90, 3, {"LVM_D0_MIN_TASKS": "0", "LVM_COL_DOWN01": "0"})


def test_color_emu_wide_band_and_fps_change(lvm, po, emu):
    M.color_wide_band_and_fps_change(lvm, po, emu)


def test_mode_switch_drops_state(lvm, po, emu):
    ck, pk0 = lvm.synth.config(0, (96, 64, 3))
    _, pk2 = lvm.synth.config(2, (96, 64, 3))
    _, pk3 = lvm.synth.config(3, (96, 64, 3))

    def vary(t, p):
        return dict([pk0, pk2, pk3, pk0][(t // 3) % 4])
    run_pair(lvm, po, emu, lvm.synth.Clip(**ck), pk0, 12, 0.0, exact=True, param_fn=vary)


def test_fast_lab_flavour_stays_within_tolerance(lvm, po, emu):
    """Default arithmetic (float32 cube root, reciprocal multiplies) vs the oracle: within the
    1e-4 / 1 LSB parity bar for every mode."""
    for idx in (0, 2, 3):
        ck, pk = lvm.synth.config(idx, (96, 64, 3))
        run_pair(lvm, po, emu, lvm.synth.Clip(**ck), pk, 8, 1e-4, exact=False, exact_lab=False)


@pytest.mark.parametrize("w,h,levels", M.PIPELINED)
def test_laplace_emu_pipelined_schedule(lvm, po, emu, w, h, levels):
    pipelined_clip(lvm, po, emu, HOST, w, h, levels, 11)


@pytest.mark.parametrize("w,h,levels", M.FUSED_MULTI)
def test_laplace_emu_fused_multi_level_pyrdown(lvm, po, emu, w, h, levels):
    """Sizes large enough that the tail starts at level 3-4, so G_1 -> G_2..G_4 goes through the
    fused k_pyr_down_multi<2|3> kernel (vector and generic first/last kernels)."""
    M.laplace_shape_3_frames(lvm, po, emu, w, h, levels)


@pytest.mark.parametrize("rows", M.FIN_ROWS)
def test_laplace_emu_final_kernel_strip_heights(lvm, po, emu, rows, monkeypatch):
    M.laplace_final_strip_height(lvm, po, emu, monkeypatch, rows)


@pytest.mark.parametrize("w,h,levels", M.ROWS_PYRDOWN)
def test_laplace_emu_wave_strip_pyrdown(lvm, po, emu, w, h, levels, monkeypatch):
    """k_pyr_down_rows (the pyrDown of large planes) forced onto every level whose width allows it:
    edge lanes, partial strips, odd heights."""
    M.laplace_wave_strip_pyrdown(lvm, po, emu, monkeypatch, w, h, levels)


@pytest.mark.parametrize("idx,w,h,levels", M.FIRST_KERNEL)
def test_emu_wave_strip_first_kernel(lvm, po, emu, idx, w, h, levels, monkeypatch):
    """k_down0_rows (u8 -> Lab / float -> pyrDown with DPP halo exchange between lanes) forced onto small frames:
    several strips per row (mirrored left / right edge groups, a strip ending exactly at the image edge), partly
    filled last strips, odd heights; Laplace (Lab) and Color (unscaled planes)."""
    M.wave_strip_first_kernel(lvm, po, emu, monkeypatch, idx, w, h, levels)


@pytest.mark.parametrize("w,h,levels,exact", M.FUSED_TABLE)
def test_emu_fused_table_conversion_and_first_kernel(lvm, po, emu, w, h, levels, exact, monkeypatch):
    """k_down0_lut_rows (OpenCV's forward Lab table + pyrDown + the integer planes of the owned pixels in one pass)
    forced onto small frames: mirrored edge groups, a strip ending at the image edge, partly filled last strips, odd
    heights (the last source row owned by the last strip); per-frame calls, so the output kernel of every frame reads the
    planes this kernel stored.  exact=False: the default flavour's fma tap sums against the 1e-4 bar."""
    M.fused_table_first_kernel(lvm, po, emu, monkeypatch, w, h, levels, exact)


def test_emu_unfused_conversion_in_batches(lvm, po, emu, monkeypatch):
    M.unfused_conversion_in_batches(lvm, po, emu, HOST, monkeypatch)


@pytest.mark.parametrize("w,h,levels,ns,calls", M.LEVEL1_GEOMETRIES)
def test_laplace_emu_level1_step_and_last_kernel_geometries(lvm, po, emu, w, h, levels, ns, calls):
    """k_lap_up at level 1 + k_lap_final_v4 over the geometries that the (deleted, round 5) fused level-1 kernel was checked on:
    bit-identical to the oracle over several calls, per-frame calls between temporal batches included."""
    frames_clip(lvm, po, emu, HOST, 0, w, h, levels, ns, calls)


def test_laplace_emu_parameter_change_between_calls(lvm, po, emu):
    M.laplace_param_change_between_calls(lvm, po, emu)


def test_emu_fused_conversion_in_batches_two_streams(lvm, po, emu, monkeypatch):
    M.fused_conversion_two_streams(lvm, po, emu, HOST, monkeypatch)


@pytest.mark.parametrize("w,h,levels,ns,calls", M.LAPLACE_BATCHES)
def test_laplace_emu_temporal_batches(lvm, po, emu, w, h, levels, ns, calls):
    frames_clip(lvm, po, emu, HOST, 0, w, h, levels, ns, calls)


@pytest.mark.parametrize("w,h,levels,ns,calls", M.SPLIT_LEVELS)
def test_laplace_emu_split_levels_iir_and_collapse(lvm, po, emu, w, h, levels, ns, calls):
    """Temporal batches of >= 4 frames: levels 2 .. L-1 as ONE k_lap_iir_levels launch + ONE k_lap_collapse launch
    (several 64 x 32 tiles of level 2, odd level heights, levels of a few pixels, two streams, every ring depth)."""
    frames_clip(lvm, po, emu, HOST, 0, w, h, levels, ns, calls)


@pytest.mark.parametrize("w,h,levels,ns,calls", M.SPLIT_FROM_2)
def test_laplace_emu_split_from_level_2_still_matches(lvm, po, emu, w, h, levels, ns, calls, monkeypatch):
    """LVM_LAP_SPLIT_FROM=2: levels 2 .. L-1 all in the IIR + collapse launches (the default until round 6; since then level 2 is a fused
    band / IIR / collapse step when the pyramid has >= 5 levels and the two launches start at level 3)."""
    M.laplace_split_from_2(lvm, po, emu, HOST, monkeypatch, w, h, levels, ns, calls)


def test_laplace_emu_level_chain_still_matches(lvm, po, emu, monkeypatch):
    M.laplace_level_chain(lvm, po, emu, HOST, monkeypatch)


@pytest.mark.parametrize("w,h,levels,calls", M.BLOCK_UP)
def test_laplace_emu_block_up_kernel_variants(lvm, po, emu, w, h, levels, calls):
    """k_lap_up_rows over batch lengths that select every ring depth (4, 2, 1), on odd heights
    (half-filled last block row)."""
    frames_clip(lvm, po, emu, HOST, 0, w, h, levels, 1, calls)


def test_laplace_emu_tiled_up_kernel_still_matches(lvm, po, emu, monkeypatch):
    M.laplace_tiled_up(lvm, po, emu, HOST, monkeypatch)


def test_frames_api_other_modes_fall_back_frame_by_frame(lvm, po, emu):
    frames_clip(lvm, po, emu, HOST, 2, 96, 64, 3, 1, (4, 3))
    frames_clip(lvm, po, emu, HOST, 3, 96, 64, 3, 1, (4, 3))


@pytest.mark.parametrize("w,h,levels,ns,calls", M.RIESZ_BATCHES)
def test_riesz_emu_temporal_batches(lvm, po, emu, w, h, levels, ns, calls):
    frames_clip(lvm, po, emu, HOST, 2, w, h, levels, ns, calls)


@pytest.mark.parametrize("w,h,levels,ns,calls", M.COLOR_BATCHES)
def test_color_emu_temporal_batches(lvm, po, emu, w, h, levels, ns, calls):
    """fps 7 -> the window caps at 16 columns: once it is full the remaining frames of a call share
    launches (every frame of a batch sees the ring shifted by one column)."""
    frames_clip(lvm, po, emu, HOST, 3, w, h, levels, ns, calls, *M.COLOR_BATCH_PARAMS)


@pytest.mark.parametrize("lo,hi", M.NARROW_DFT_BANDS)
@pytest.mark.parametrize("thin8", ["1", "0"])
def test_color_emu_narrow_band_dft_eight_lanes_per_row(lvm, po, emu, lo, hi, thin8, monkeypatch):
    """k_col_dft_thin8 (at most four spectrum entries: eight lanes per window row) on temporal batches: three complex bins (0.8-1.6 Hz
    at 7 fps, 16-frame window), one complex bin + the Nyquist element (2.9-3.5 Hz), a single bin (0.8-0.95 Hz); LVM_COL_THIN8_DFT=0
    runs the one-thread-per-row kernel on the same clips.  Bit-exact against the oracle either way."""
    M.color_narrow_band_dft(lvm, po, emu, HOST, monkeypatch, lo, hi, thin8)


# ---- ragged rows: strides larger than the row ---------------------------------------------------------
@pytest.mark.parametrize("idx,pad_in,pad_out", M.PADDED_STRIDES)
def test_emu_padded_row_strides(lvm, po, emu, idx, pad_in, pad_out):
    """lvm_process_device on frames whose rows are padded (a cv::Mat ROI view has step > cols * channels):
    dword-aligned paddings keep the vectorised kernels, odd ones select the generic byte kernels; the padding
    bytes of the output must stay untouched."""
    padded_strides_clip(lvm, po, emu, HOST, idx, pad_in, pad_out)


# ---- degenerate content: flat black / white regions and constant frames -----------------------------------
@pytest.mark.parametrize("idx,const_from,size", M.FLAT_REGIONS)
def test_emu_flat_regions_and_constant_frames(lvm, po, emu, idx, const_from, size):
    M.flat_regions(lvm, po, emu, idx, const_from, size)


@pytest.mark.parametrize("idx", [0, 2, 3])
def test_emu_fully_constant_clip(lvm, po, emu, idx):
    M.fully_constant_clip(lvm, po, emu, idx)


@pytest.mark.parametrize("idx,over", M.EXTREME_PARAMETERS)
def test_emu_extreme_parameters(lvm, po, emu, idx, over):
    M.extreme_parameters(lvm, po, emu, idx, over)


@pytest.mark.parametrize("idx", [0, 2, 3])
def test_emu_size_and_channel_changes(lvm, po, emu, idx):
    M.size_and_channel_changes(lvm, po, emu, idx)


@pytest.mark.parametrize("w,h,levels", [(520, 40, 3), (260, 36, 2), (256, 34, 2), (772, 22, 2)])
def test_fast_final_kernel_strips_and_shortcut_paths(lvm, po, emu, w, h, levels):
    """Default-flavour last Laplace kernel (k_lap_final_fast): several wave strips per row, a last strip with a
    single lane / a half wave, DPP halo exchange with the halo loads of the first and last lane; a clip with very
    dark and saturated patches so that the general (select / spline) paths and the wave-uniform shortcuts both run,
    strong amplification so that outputs clamp at 0 and 255."""
    ck, pk = lvm.synth.config(0, (w, h, levels))
    pk["amplification"] = 60.0
    base = lvm.synth.Clip(**ck)

    class Patched:
        def frame(self, t):
            f = base.frame(t).copy()
            f[2:h // 2, 8:w // 4] = (f[2:h // 2, 8:w // 4] // 12)           # values 0..20: below the CIE threshold
            f[h // 2:h - 1, w // 2:w - 5] = 255 - (255 - f[h // 2:h - 1, w // 2:w - 5]) // 16
            f[:, w - 4:] = f[:, w - 4:] // 3
            return f
    worst = run_pair(lvm, po, emu, Patched(), pk, 7, 1e-4, exact=False, exact_lab=False, u8_frac=0.998)
    print("fast final kernel", (w, h, levels), worst)


@pytest.mark.parametrize("strip", M.RIESZ_SPLIT_STRIPS[0])
@pytest.mark.parametrize("w,h,levels", M.RIESZ_SPLIT_STRIPS[1])
def test_riesz_emu_wave_strip_stencils(lvm, po, emu, w, h, levels, strip, monkeypatch):
    """The LDS-free 9x9 strip kernels (forced onto these small planes): several 248-column strips per row (a full one, a
    partial one, a strip whose last lane owns the image's last column group), strips cut by the image height, odd heights,
    the strip height chosen by the launch code (0) or forced (10 rows: several strips per column; 54: the 1080p choice), a
    plane of five rows (the row index of the loads bounces off both edges inside one group of steps), bit-exact against the oracle."""
    M.riesz_wave_strip_stencils(lvm, po, emu, monkeypatch, w, h, levels, strip)


@pytest.mark.parametrize("strip", M.RIESZ_COLLAPSE_STRIPS[0])
@pytest.mark.parametrize("w,h,levels", M.RIESZ_COLLAPSE_STRIPS[1])
def test_riesz_emu_wave_strip_collapse_and_output(lvm, po, emu, w, h, levels, strip, monkeypatch):
    """k_rz_collapse_strips forced onto small planes with even sizes: the collapse of levels 1 and 2 and the output kernel of a
    512 x 64 frame, several 248-column strips per row, strips cut by the image height, the smallest plane the kernel accepts
    (two column groups, four rows: every row index is a reflection), strip height chosen by the launch code or forced;
    OpenCV-order Lab arithmetic: bit-exact against the oracle."""
    M.riesz_wave_strip_collapse_and_output(lvm, po, emu, monkeypatch, w, h, levels, strip)


def test_riesz_emu_strip_output_fast_flavour_equals_the_tiled_kernel(lvm, emu, monkeypatch):
    """The default flavour (reciprocal multiplies, packed Lab2BGR) of the strip output kernel against the tiled k_rz_final on the
    same frames: identical bytes and identical float frames (both evaluate the same operations per pixel)."""
    ck, pk = lvm.synth.config(2, (256, 48, 3))
    clip = lvm.synth.Clip(**ck)
    from helpers import c_params
    outs = []
    for strips in ("1", "0"):
        monkeypatch.setenv("LVM_RZ_COLLAPSE_STRIPS_MIN", "1")
        monkeypatch.setenv("LVM_RZ_COLLAPSE_STRIPS", strips)
        ctx = lvm.Context(0, 1, emu)
        ctx.keep_float(True)
        try:
            got = []
            for t in range(5):
                out, produced = ctx.process(clip.frame(t), c_params(lvm, pk))
                got.append((np.array(out, copy=True), ctx.read_float((48, 256, 3)).copy() if produced else None))
        finally:
            ctx.close()
        outs.append(got)
    for (a, fa), (b, fb) in zip(*outs):
        assert np.array_equal(a, b)
        assert (fa is None and fb is None) or np.array_equal(fa, fb)


# ---- chromatic content: saturated colours through the same kernels (tests/content.py, parity_matrix.CHROMA_*) -----------------------
@pytest.mark.parametrize("kind,idx,w,h,levels", M.CHROMA_CASES)
def test_emu_chroma_bit_exact(lvm, po, emu, kind, idx, w, h, levels):
    M.chroma_shape(lvm, po, emu, kind, idx, w, h, levels)


@pytest.mark.parametrize("kind,idx,w,h,levels", M.CHROMA_CASES)
def test_emu_chroma_default_flavour_within_the_bars(lvm, po, emu, kind, idx, w, h, levels):
    worst = M.chroma_shape(lvm, po, emu, kind, idx, w, h, levels, flavour_exact=False)
    print("chroma default flavour", kind, (idx, w, h, levels), "worst rel/u8/frac, shipped u8/frac", worst)


def test_emu_chroma_gray_frames_bit_exact(lvm, po, emu):
    M.chroma_gray(lvm, po, emu)


@pytest.mark.parametrize("kind,force", M.CHROMA_FORCED_CASES)
def test_emu_chroma_forced_strip_kernels_bit_exact(lvm, po, emu, kind, force):
    M.chroma_forced(lvm, po, emu, HOST, kind, force)


@pytest.mark.parametrize("kind", M.CHROMA_FORCED_KINDS)
def test_emu_chroma_final_kernel_strips_of_8_rows(lvm, po, emu, kind, monkeypatch):
    M.laplace_final_strip_height(lvm, po, emu, monkeypatch, 8, kind=kind)


@pytest.mark.parametrize("kind,idx,w,h,levels", M.CHROMA_ANALYTIC)
def test_emu_chroma_analytic_flavour_bit_exact(lvm, po, emu, kind, idx, w, h, levels, monkeypatch):
    M.analytic_flavour(lvm, po, emu, monkeypatch, idx, w, h, levels, kind=kind)


@pytest.mark.parametrize("idx,w,h,levels,ns,calls,over,clip_over", M.CHROMA_BATCHES)
def test_emu_chroma_temporal_batches(lvm, po, emu, idx, w, h, levels, ns, calls, over, clip_over):
    M.chroma_batches(lvm, po, emu, HOST, idx, w, h, levels, ns, calls, over, clip_over)


@pytest.mark.parametrize("idx,w,h,levels,name", M.CHROMA_LAYOUTS)
def test_emu_chroma_layouts(lvm, po, emu, idx, w, h, levels, name):
    M.chroma_layout(lvm, po, emu, HOST, idx, w, h, levels, name)


def test_emu_chroma_far_out_of_gamut(lvm, po, emu):
    M.chroma_out_of_gamut(lvm, po, emu)
