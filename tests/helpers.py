"""Shared helpers of the parity tests (test infrastructure)."""
import numpy as np

# The shipped build against the float-keeping one where the output kernels quantise through the u8 step table (fin_steps in
# csrc/lvm_internal.h): the step table is OpenCV's unfused spline + scale + round, the float-keeping kernels evaluate the spline as
# an fma chain -- the two round apart on a few pixels (the bar of tests/test_u8_steps.py).
STEPS_U8_FRAC = 0.9999


def c_params(lvm, pk, key=0):
    return lvm.LvmParams(pk["mode"], pk["levels"], pk["amplification"], pk["coWavelength"], pk["coLow"],
                         pk["coHigh"], pk["chromAttenuation"], pk["framerate"], key)


def _channels(f):
    return 1 if f.ndim == 2 else f.shape[2]


def run_pair(lvm, po, lib, clip, pk, nframes, float_tol, n_streams=1, u8_max=1, u8_frac=0.999, exact=False,
             param_fn=None, exact_lab=None, analytic=False, lab_lut=None, shipped=True):
    """Feeds the same frames to the CPU oracle and to the library behind the C ABI `lib`
    (gfx950 build or the CPU emulation build) and checks, frame by frame:
      (i)   produced / passthrough flags identical,
      (ii)  pre-quantisation float frame: max|d| / max|ref| <= float_tol  (exact => bit-equal),
      (iii) u8 frame: max abs diff <= u8_max LSB and >= u8_frac identical pixels.
    Both sides run OpenCV 4's default forward Lab (the interpolated 33^3 table) unless analytic=True (the cube-root form
    OpenCV computes with its interpolation switched off: oracle lvmo_set_lab_lut(0), library lvm_debug_lab_analytic).

    Reading the float frame (lvm_debug_keep_float) selects other builds of the output kernels (DBG = true, spline quantiser).
    So a second context of the same library, `shipped`, runs the same frames in the configuration that process(), the chain,
    export and bench.py run: keep_float off, exact_lab off, lab_analytic as asked.  Per frame it must give
      (iv)  the oracle's produced flags, and a u8 frame within the u8_max / u8_frac bars of the oracle's
            (exact=True: the parity bars, 1 LSB / 0.999, since the shipped build is the fast flavour);
      (v)   against the first context's u8 frame, when both run the same flavour (always in Color mode, which has no Lab):
            identical bytes where the step table does not apply (Color, gray, the analytic flavour), else <= 1 LSB and
            >= STEPS_U8_FRAC identical.
    shipped=False opts out (callers give the reason on the same line).
    Returns the worst observed figures: [float rel, u8 diff, identical fraction] of the first context, then
    [u8 diff, identical fraction] of the shipped context against the oracle."""
    P = po.make_params(**pk)
    exact_lab = exact if exact_lab is None else exact_lab
    ctx = lvm.Context(0, n_streams, lib)
    ctx.keep_float(True)
    ctx.exact_lab(exact_lab)   # bit-exact checks need OpenCV-order Lab math
    ctx.lab_analytic(analytic)
    ship = None
    if shipped:
        ship = lvm.Context(0, n_streams, lib)
        ship.lab_analytic(analytic)
    if lab_lut is not None:
        ctx.set_lab_lut(lab_lut)
        if ship is not None:
            ship.set_lab_lut(lab_lut)
    po.lib().lvmo_set_lab_lut(0 if analytic else 1)
    orc = po.Oracle()
    same_flavour = analytic or not exact_lab
    ship_max, ship_frac = (1, 0.999) if exact else (u8_max, u8_frac)
    worst = [0.0, 0, 1.0, 0, 1.0]
    try:
        for t in range(nframes):
            mode = pk["mode"]
            if param_fn:
                pk2 = param_fn(t, dict(pk))
                P = po.make_params(**pk2)
                cp = c_params(lvm, pk2)
                mode = pk2["mode"]
            else:
                cp = c_params(lvm, pk)
            f = clip.frame(t)
            ref, pr = orc.process(f, P)
            out, pg = ctx.process(f, cp)
            assert pr == pg, "produced flag differs at frame %d: oracle %s, lib %s" % (t, pr, pg)
            if ship is not None:
                out_s, ps = ship.process(f, cp)
                assert pr == ps, "shipped build: produced flag differs at frame %d: oracle %s, lib %s" % (t, pr, ps)
            if not pr:
                assert out is f or np.array_equal(out, f)
                if ship is not None:
                    assert out_s is f or np.array_equal(out_s, f), "shipped build: passthrough frame %d changed" % t
                continue
            fr = orc.last_float()
            fg = ctx.read_float(fr.shape)
            assert np.isfinite(fg).all(), "non-finite values in frame %d" % t
            rel = float(np.abs(fr - fg).max() / max(float(np.abs(fr).max()), 1e-30))
            du = np.abs(ref.astype(np.int32) - out.astype(np.int32))
            worst[:3] = [max(worst[0], rel), max(worst[1], int(du.max())), min(worst[2], float((du == 0).mean()))]
            if exact:
                assert np.array_equal(fr, fg), "frame %d: float frames differ (max rel %.3e)" % (t, rel)
                assert np.array_equal(ref, out)
            else:
                assert rel <= float_tol, "frame %d: float rel err %.3e > %.1e" % (t, rel, float_tol)
                assert du.max() <= u8_max, "frame %d: u8 diff %d" % (t, du.max())
                assert (du == 0).mean() >= u8_frac, "frame %d: identical fraction %.5f" % (t, (du == 0).mean())
            if ship is None:
                continue
            ds = np.abs(ref.astype(np.int32) - out_s.astype(np.int32))
            worst[3:] = [max(worst[3], int(ds.max())), min(worst[4], float((ds == 0).mean()))]
            assert ds.max() <= ship_max, "shipped build, frame %d: u8 diff %d against the oracle" % (t, ds.max())
            assert (ds == 0).mean() >= ship_frac, "shipped build, frame %d: identical fraction %.5f" % (t, (ds == 0).mean())
            if same_flavour or mode == 2:
                steps = mode in (0, 1) and _channels(f) == 3 and not analytic
                dd = np.abs(out.astype(np.int32) - out_s.astype(np.int32))
                if steps:
                    assert dd.max() <= 1 and (dd == 0).mean() >= STEPS_U8_FRAC, \
                        "frame %d: shipped build vs float-keeping build: max %d, identical %.6f" % (t, dd.max(), (dd == 0).mean())
                else:
                    assert dd.max() == 0, "frame %d: shipped build vs float-keeping build differ on %d bytes" % (t, int((dd != 0).sum()))
    finally:
        po.lib().lvmo_set_lab_lut(1)
        ctx.close()
        if ship is not None:
            ship.close()
        orc.close()
    return worst


# ---- exact-flavour bodies shared by the emulation and the gfx950 matrices (tests/parity_matrix.py) --------------------------
def _clip_of(lvm, clip_fn, ck, stream):
    """the clip of one stream: clip_fn(ck, stream) where a case brings its own content (tests/content.py), else the synthetic
    texture with the stream's seed"""
    return clip_fn(ck, stream) if clip_fn else lvm.synth.Clip(seed=1234 + stream, **ck)


_REFERENCES = {}       # clip_reference: key -> [frames [n][h][w][3] (read-only), produced flags [n], oracle frames [n][h][w][3] (read-only)]


def clip_reference(lvm, po, refs, idx, w, h, levels, stream, n, over=None, clip_over=None):
    """The first n frames of the synthetic clip of stream `stream` (seed 1234 + stream) and what the oracle makes of them, computed once
    per process and shared, read-only, by every case that asks: (input frames, produced flags, oracle frames).  The clip of a stream and
    the oracle's frames do not depend on how many streams run beside it or on how the frames are cut into calls.  `refs` names the
    oracle configuration in force ("libm": none; "ptrig": parity_matrix.portable_trig) and is part of the key."""
    key = (refs, idx, w, h, levels, stream, tuple(sorted((over or {}).items())), tuple(sorted((clip_over or {}).items())))
    have = _REFERENCES.get(key)
    if have is None or len(have[1]) < n:
        ck, pk = lvm.synth.config(idx, (w, h, levels))
        pk.update(over or {})
        ck.update(clip_over or {})
        clip = lvm.synth.Clip(seed=1234 + stream, **ck)
        P = po.make_params(**pk)
        orc = po.Oracle()
        try:
            fin = np.stack([clip.frame(t) for t in range(n)])
            out, prod = np.zeros_like(fin), []
            for t in range(n):
                ref, pr = orc.process(fin[t], P)
                prod.append(bool(pr))
                if pr:
                    out[t] = ref
        finally:
            orc.close()
        fin.setflags(write=False)
        out.setflags(write=False)
        have = _REFERENCES[key] = (fin, prod, out)
    return have[0][:n], have[1][:n], have[2][:n]


class _CachedOracle:
    """the part of po.Oracle that frames_clip uses, answered from clip_reference (the frames must come in the clip's order)"""

    def __init__(self, fin, prod, out):
        self.fin, self.prod, self.out, self.t = fin, prod, out, 0

    def process(self, frame, P):
        t = self.t
        assert np.array_equal(frame, self.fin[t]), "frame %d is not the clip's" % t
        self.t += 1
        return self.out[t], self.prod[t]

    def close(self):
        pass


def frames_clip(lvm, po, lib, mem, idx, w, h, levels, n_streams, calls, over=None, clip_over=None, clip_fn=None, refs=None, device=False,
                exact=True, profile_call=None):
    """lvm_process_device_frames: batches of consecutive frames (sizes in `calls`) of n_streams streams, OpenCV-order Lab
    (lvm_debug_exact_lab), must give exactly the bytes the oracle produces frame by frame.
    refs ("libm" / "ptrig", see clip_reference): the oracle's frames come from the per-process cache instead of n_streams live oracles.
    device: every frame of a call goes through lvm_process_device on its own (the per-frame schedule).
    exact=False: the default flavour, held to the parity bars (1 LSB, >= 0.999 identical bytes per frame); returns the worst figures.
    profile_call=k: returns {report name: variants} of what call k launched (lvm_profile_variants)."""
    ck, pk = lvm.synth.config(idx, (w, h, levels))
    pk.update(over or {})
    ck.update(clip_over or {})
    P = po.make_params(**pk)
    cp = c_params(lvm, pk)
    total = sum(calls)
    if refs is None:
        clips = [_clip_of(lvm, clip_fn, ck, s) for s in range(n_streams)]
        orcs = [po.Oracle() for _ in range(n_streams)]
        frame_of = lambda s_, t_: clips[s_].frame(t_)
    else:
        assert clip_fn is None
        cached = [clip_reference(lvm, po, refs, idx, w, h, levels, s, total, over, clip_over) for s in range(n_streams)]
        orcs = [_CachedOracle(*c) for c in cached]
        frame_of = lambda s_, t_: cached[s_][0][t_]
    ctx = lvm.Context(0, n_streams, lib)
    ctx.exact_lab(exact)
    t = 0
    fb = w * h * 3
    worst, names = [0, 1.0], None
    try:
        for k, nf in enumerate(calls):
            fin = np.stack([np.stack([frame_of(s_, t + f) for s_ in range(n_streams)]) for f in range(nf)])      # [frame][stream][h][w][3]
            d_in = mem.upload(fin)
            d_out = mem.zeros_like(d_in)
            if profile_call == k:
                ctx.profile(True)
            if device:
                produced = [ctx.process_device(cp, mem.ptr(d_in, f), w, h, 3, w * 3, fb, mem.ptr(d_out, f), w * 3, fb, mem.stream()) for f in range(nf)]
            else:
                produced = ctx.process_device_frames(cp, nf, mem.ptr(d_in), w, h, 3, w * 3, fb, fb * n_streams,
                                                     mem.ptr(d_out), w * 3, fb, fb * n_streams, mem.stream())
            mem.sync(ctx)
            if profile_call == k:
                variants = ctx.profile_variants()
                names = {n: variants.get(n, set()) for n in ctx.profile_collect()}
                ctx.profile(False)
            fout = mem.download(d_out)
            for f in range(nf):
                for s_ in range(n_streams):
                    ref, pr = orcs[s_].process(fin[f, s_], P)
                    assert produced[f] == pr, (t + f, produced[f], pr)
                    if pr and exact:
                        assert np.array_equal(ref, fout[f, s_]), "frame %d stream %d: %d bytes differ" % (
                            t + f, s_, int((ref != fout[f, s_]).sum()))
                    elif pr:
                        du = np.abs(ref.astype(np.int32) - fout[f, s_].astype(np.int32))
                        worst = [max(worst[0], int(du.max())), min(worst[1], float((du == 0).mean()))]
                        assert du.max() <= 1 and (du == 0).mean() >= 0.999, "frame %d stream %d: u8 diff %d, identical %.6f" % (
                            t + f, s_, int(du.max()), float((du == 0).mean()))
            t += nf
    finally:
        ctx.close()
        for o in orcs:
            o.close()
    return names if profile_call is not None else (None if exact else worst)


LAYOUT_GUARD = 64        # bytes behind the last rectangle of every allocation: part of the output's untouched area


def _layout_geometry(w, h, n_streams, nf, layout):
    """byte geometry of one call of nf frames in `layout` = (extra canvas columns, rx, ry, ox, oy, stream gap bytes, order):
    (row stride, stream stride, frame stride, offset of the input view, offset of the output view, allocation size).
    order "fs": a canvas of (w + extra) pixels by h + max(ry, oy) + 1 rows (h rows when both are 0) per (frame, stream), laid out
                [frame][stream], gap bytes behind each;
    order "sf": the same canvases laid out [stream][frame];
    order "mosaic" / "mosaic_device": the streams side by side in one canvas per frame (stream stride = w * 3 bytes)."""
    extra, rx, ry, ox, oy, gap, order = layout
    assert max(rx, ox) <= extra
    H = h + max(ry, oy) + (1 if max(ry, oy) else 0)
    if order in ("mosaic", "mosaic_device"):
        row = (n_streams * w + extra) * 3
        ss, fs = w * 3, H * row + gap
    else:
        row = (w + extra) * 3
        canvas = H * row + gap
        ss, fs = (canvas, n_streams * canvas) if order == "fs" else (nf * canvas, canvas)
        assert order in ("fs", "sf")
    total = (nf - 1) * fs + (n_streams - 1) * ss + H * row + gap + LAYOUT_GUARD
    return row, ss, fs, ry * row + rx * 3, oy * row + ox * 3, total


def _view_index(w, h, n_streams, nf, row, ss, fs, off):
    """flat byte indices [frame][stream][h][w * 3] of the rectangles of a call inside its allocation"""
    f, s_, y, x = np.ogrid[:nf, :n_streams, :h, :w * 3]
    return off + f * fs + s_ * ss + y * row + x


def layout_clip(lvm, po, lib, mem, idx, w, h, levels, n_streams, calls, layout, env=None, over=None, clip_over=None, exact=True,
                profile=False, clip_fn=None):
    """lvm_process_device_frames (order "mosaic_device": lvm_process_device, frame by frame) on frames that are rectangles inside
    larger canvases -- what a cv::Mat ROI or the export's ROI view of a decoded frame hands to the magnifier.  `layout` as in
    _layout_geometry (tests/parity_matrix.py: LAYOUTS); input canvases are filled with 0xAB, output canvases with 0xCD, the two
    rectangles sit at different offsets.  `env`: forcing switches, set while the contexts are created and run.
    The context runs OpenCV-order Lab (lvm_debug_exact_lab).  Per frame and stream:
      - the produced flags are the oracle's;
      - exact=True: the output rectangle is the oracle's frame, bit for bit;
        exact=False (Riesz on the GPU: device acosf / sinf / cosf): within the parity bars of the oracle (1 LSB, >= 0.999 identical)
        AND byte-equal to a second context of the same library that gets the same frames in packed layout (w * 3, w * h * 3,
        [frame][stream]) in the same flavour -- the arithmetic of the exact flavour does not depend on the kernel family;
      - every other byte of the output allocation is still 0xCD (between rows, streams and frames, before the first rectangle,
        behind the last one); a frame that was not produced leaves its rectangle untouched too.
    Returns ([worst u8 diff, worst identical fraction] against the oracle, and with profile=True {report name launched: set of the
    kernel variants that ran under it (lvm_profile_variants), empty for names with one kernel}, else None)."""
    import os
    ck, pk = lvm.synth.config(idx, (w, h, levels))
    pk.update(over or {})
    ck.update(clip_over or {})
    clips = [_clip_of(lvm, clip_fn, ck, s) for s in range(n_streams)]
    P = po.make_params(**pk)
    cp = c_params(lvm, pk)
    order = layout[6]
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    ctx = packed = None
    orcs = []
    worst, names = [0, 1.0], None
    try:
        ctx = lvm.Context(0, n_streams, lib)
        ctx.exact_lab(True)
        if profile:
            ctx.profile(True)
        if not exact:
            packed = lvm.Context(0, n_streams, lib)
            packed.exact_lab(True)
        orcs = [po.Oracle() for _ in range(n_streams)]
        t = 0
        for nf in calls:
            row, ss, fs, off_in, off_out, total = _layout_geometry(w, h, n_streams, nf, layout)
            fin = np.stack([np.stack([c.frame(t + f) for c in clips]) for f in range(nf)])      # [frame][stream][h][w][3]
            ii = _view_index(w, h, n_streams, nf, row, ss, fs, off_in)
            io = _view_index(w, h, n_streams, nf, row, ss, fs, off_out)
            assert ii.max() < total - LAYOUT_GUARD and io.max() < total - LAYOUT_GUARD and np.unique(io).size == io.size
            buf_in = np.full(total, 0xAB, np.uint8)
            buf_in[ii] = fin.reshape(nf, n_streams, h, w * 3)
            d_in = mem.upload(buf_in)
            d_out = mem.upload(np.full(total, 0xCD, np.uint8))
            assert mem.ptr_at(d_in, 0) % 16 == 0 and mem.ptr_at(d_out, 0) % 16 == 0       # the offsets alone decide the alignment
            p_in, p_out = mem.ptr_at(d_in, off_in), mem.ptr_at(d_out, off_out)
            if order == "mosaic_device":
                produced = [ctx.process_device(cp, p_in + f * fs, w, h, 3, row, ss, p_out + f * fs, row, ss, mem.stream()) for f in range(nf)]
            else:
                produced = ctx.process_device_frames(cp, nf, p_in, w, h, 3, row, ss, fs, p_out, row, ss, fs, mem.stream())
            mem.sync(ctx)
            buf_out = mem.download(d_out)
            got = buf_out[io].reshape(nf, n_streams, h, w, 3)
            if packed is not None:
                fb = w * h * 3
                q_in = mem.upload(fin)
                q_out = mem.zeros_like(q_in)
                prod_p = packed.process_device_frames(cp, nf, mem.ptr(q_in), w, h, 3, w * 3, fb, fb * n_streams, mem.ptr(q_out), w * 3, fb,
                                                      fb * n_streams, mem.stream())
                mem.sync(packed)
                got_p = mem.download(q_out)
                assert list(prod_p) == list(produced), (t, prod_p, produced)
            untouched = np.ones(total, bool)
            for f in range(nf):
                for s_ in range(n_streams):
                    ref, pr = orcs[s_].process(fin[f, s_], P)
                    assert produced[f] == pr, (t + f, produced[f], pr)
                    if not pr:
                        continue
                    untouched[io[f, s_].reshape(-1)] = False
                    if exact:
                        assert np.array_equal(ref, got[f, s_]), "frame %d stream %d: %d bytes differ from the oracle" % (
                            t + f, s_, int((ref != got[f, s_]).sum()))
                        continue
                    du = np.abs(ref.astype(np.int32) - got[f, s_].astype(np.int32))
                    worst = [max(worst[0], int(du.max())), min(worst[1], float((du == 0).mean()))]
                    assert du.max() <= 1 and (du == 0).mean() >= 0.999, "frame %d stream %d: u8 diff %d, identical %.6f" % (
                        t + f, s_, int(du.max()), float((du == 0).mean()))
                    assert np.array_equal(got_p[f, s_], got[f, s_]), "frame %d stream %d: %d bytes differ from the packed layout" % (
                        t + f, s_, int((got_p[f, s_] != got[f, s_]).sum()))
            bad = np.flatnonzero(untouched & (buf_out != 0xCD))
            assert bad.size == 0, "call at frame %d: %d bytes outside the output rectangles were written, first at offset %d" % (
                t, bad.size, int(bad[0]))
            t += nf
        if profile:
            variants = ctx.profile_variants()
            names = {n: variants.get(n, set()) for n in ctx.profile_collect()}
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        for c_ in (ctx, packed):
            if c_ is not None:
                c_.close()
        for o in orcs:
            o.close()
    return worst, names


# ---- surfaces that lie far apart: stream and frame strides beyond 2^31 and 2^32 bytes ---------------------------------------------------
# include/lvm_hip.h promises stream and frame strides of any size, and every kernel forms base + b * stride itself.  One allocation
# of FAR_* geometry holds all rectangles of a call; the pointers handed to the library start FAR_BASE bytes into it, so that every
# address a 32-bit truncation of an offset could produce -- zero-extended or sign-extended, of the whole offset or of its frame and
# stream terms -- still lies inside the allocation: such a bug shows as wrong bytes, never as a fault (far_layout asserts it).
FAR_STREAM = 2**31 + 64          # stream stride of the [frame][stream] call; the frame stride is twice that
FAR_FRAME = 2**32 + 128          # = 2 * FAR_STREAM: the batch leg's rule.  Also the stream stride of the per-frame call
FAR_BASE = 2**31 + 4096          # offset of the first input rectangle in the allocation
FAR_OUT = 2**20                  # an output rectangle lies this far behind the input rectangle of the same frame and stream
FAR_CAP = 10 * 2**30             # no allocation above this


def _trunc32(v):
    """v, its low 32 bits zero-extended, and sign-extended"""
    z = v & 0xFFFFFFFF
    return {v, z, z - 2**32 if z >= 2**31 else z}


def far_layout(span, terms, shift=0, guard=LAYOUT_GUARD, slots=(0, FAR_OUT)):
    """Geometry of far surfaces in one allocation.  `span`: bytes from the first to the last byte of one rectangle; `terms`: per
    rectangle the addends of its offset from the pointer that is passed (such as (f * frame stride, s * stream stride)); `shift`: extra
    bytes on every pointer (an odd base); `slots`: where the pointers that are passed lie behind the first one, at least span + 2 guards
    apart.  Returns (offsets of the pointers in the allocation, allocation size) after asserting the safety property from the numbers:
    with any addend, or the sum, cut to 32 bits either way, the rectangle and its guards still lie inside the allocation."""
    slots = sorted(slots)
    assert slots[0] == 0 and all(b - a >= span + 2 * guard for a, b in zip(slots, slots[1:]))
    ptrs = [FAR_BASE + shift + s for s in slots]
    total = ptrs[-1] + max(sum(t) for t in terms) + span + guard
    assert total <= FAR_CAP, total
    for t in terms:
        cands = _trunc32(sum(t))
        partial = {0}
        for a in t:
            partial = {p + c for p in partial for c in _trunc32(a)}
        for c in cands | partial:
            for p in ptrs:
                assert 0 <= p + c - guard and p + c + span + guard <= total, (t, c, p, total)
    return ptrs, total


def _far_rows(w, h, row, ch=3):
    """indices of the pixels' bytes [h][w * ch] inside one rectangle of row stride `row`"""
    return np.arange(h)[:, None] * row + np.arange(w * ch)[None, :]


def far_put(mem, buf, at, rows, frame, fill=0xAB):
    """one frame into its rectangle at byte `at` of the allocation, the row padding filled with `fill`"""
    h, wb = rows.shape
    region = np.full(int(rows.max()) + 1, fill, np.uint8)
    region[rows] = frame.reshape(h, wb)
    mem.put(buf, at, region)


def far_arm(mem, buf, at, rows, guard=LAYOUT_GUARD):
    """an output rectangle, its row padding and `guard` bytes either side of it: 0xCD"""
    mem.put(buf, at - guard, np.full(int(rows.max()) + 1 + 2 * guard, 0xCD, np.uint8))


def far_get(mem, buf, at, rows, what, guard=LAYOUT_GUARD):
    """the bytes [h][w * ch] of an output rectangle, after checking that its row padding and the guards are still 0xCD"""
    region = mem.get(buf, at - guard, int(rows.max()) + 1 + 2 * guard)
    got = region[guard:][rows]
    rest = np.ones(region.size, bool)
    rest[guard + rows.reshape(-1)] = False
    bad = np.flatnonzero(rest & (region != 0xCD))
    assert bad.size == 0, "%s: %d bytes outside the rectangle were written, first %d bytes from its start" % (what, bad.size, int(bad[0]) - guard)
    return got


def far_clip(lvm, po, lib, mem, idx, w, h, levels, seed_frames, over=None, clip_over=None, env=None, odd=False, refs="libm"):
    """Two streams whose frames lie FAR_STREAM and FAR_FRAME bytes apart, in one allocation (far_layout), rows padded by 4 bytes,
    OpenCV-order Lab, every produced frame the oracle's bit for bit (`refs` as in clip_reference):
      - `seed_frames` lvm_process_device calls on small packed buffers build the state;
      - ONE lvm_process_device_frames call of 2 frames in [frame][stream] order (frame stride == 2 * stream stride: the batch leg), the
        rectangles at 0, FAR_STREAM, FAR_FRAME and FAR_FRAME + FAR_STREAM from the pointers passed;
      - ONE lvm_process_device call with stream stride FAR_FRAME on the same allocation.
    Only the rectangles are written and read; the row padding and LAYOUT_GUARD bytes either side of every output rectangle must stay
    0xCD.  `env`: forcing switches, set while the context exists.  odd: both pointers one byte on (the byte kernels).
    Returns {report name: variants} of the two far calls (lvm_profile_variants)."""
    import os
    ns, nf, ch = 2, 2, 3
    row = w * ch + 4
    rows = _far_rows(w, h, row)
    span = int(rows.max()) + 1
    batch = {(f, s): (f * FAR_FRAME, s * FAR_STREAM) for f in range(nf) for s in range(ns)}
    single = {(0, s): (0, s * FAR_FRAME) for s in range(ns)}
    (p_in, p_out), total = far_layout(span, list(batch.values()) + list(single.values()), shift=1 if odd else 0)
    n = seed_frames + nf + 1
    cached = [clip_reference(lvm, po, refs, idx, w, h, levels, s, n, over, clip_over) for s in range(ns)]
    ck, pk = lvm.synth.config(idx, (w, h, levels))
    pk.update(over or {})
    cp = c_params(lvm, pk)
    fb = w * h * ch
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    ctx = buf = None
    try:
        ctx = lvm.Context(0, ns, lib)
        ctx.exact_lab(True)
        for t in range(seed_frames):
            d_in = mem.upload(np.stack([c[0][t] for c in cached]))
            d_out = mem.zeros_like(d_in)
            pr = ctx.process_device(cp, mem.ptr(d_in), w, h, ch, w * ch, fb, mem.ptr(d_out), w * ch, fb, mem.stream())
            mem.sync(ctx)
            got = mem.download(d_out)
            for s in range(ns):
                assert pr == cached[s][1][t], (t, s)
                if pr:
                    assert np.array_equal(got[s], cached[s][2][t]), "seeding frame %d stream %d" % (t, s)
        buf = mem.empty(total)
        assert mem.ptr_at(buf, 0) % 16 == 0
        ctx.profile(True)

        def run(t0, layout, call, what):
            for (f, s), terms in layout.items():
                far_put(mem, buf, p_in + sum(terms), rows, cached[s][0][t0 + f])
                far_arm(mem, buf, p_out + sum(terms), rows)
            produced = call()
            mem.sync(ctx)
            for (f, s), terms in layout.items():
                assert produced[f] and cached[s][1][t0 + f], (what, f, s, produced)
                got = far_get(mem, buf, p_out + sum(terms), rows, "%s frame %d stream %d" % (what, f, s)).reshape(h, w, ch)
                ref = cached[s][2][t0 + f]
                if not np.array_equal(got, ref):
                    twins = [(f2, s2) for (f2, s2) in layout if np.array_equal(got, cached[s2][2][t0 + f2])]
                    raise AssertionError("%s frame %d stream %d: %d bytes differ from the oracle (the oracle's frame, stream of: %s; still 0xCD: %s)" % (
                        what, f, s, int((got != ref).sum()), twins, bool((got == 0xCD).all())))
        t = seed_frames
        run(t, batch, lambda: ctx.process_device_frames(cp, nf, mem.ptr_at(buf, p_in), w, h, ch, row, FAR_STREAM, FAR_FRAME, mem.ptr_at(buf, p_out), row,
                                                        FAR_STREAM, FAR_FRAME, mem.stream()), "far batch")
        run(t + nf, single, lambda: [ctx.process_device(cp, mem.ptr_at(buf, p_in), w, h, ch, row, FAR_FRAME, mem.ptr_at(buf, p_out), row, FAR_FRAME,
                                                        mem.stream())], "far per-frame call")
        variants = ctx.profile_variants()
        return {nm: variants.get(nm, set()) for nm in ctx.profile_collect()}
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if ctx is not None:
            ctx.close()
        del buf
        mem.release()


def far_units(lvm, lib, mem, n_streams, inputs, out_bytes, call, out_init=None, setup=None):
    """A device surface that takes a stream or frame stride, on two units (streams or frames) FAR_FRAME bytes apart in one allocation
    (far_layout), against what the same surface gives on packed buffers.  inputs: uint8 arrays [2][...], one per input pointer of the
    surface; out_bytes: bytes of one unit of its device output (0: none), which starts as 0xCD or as out_init [2][out_bytes] (a surface
    that works in place).  call(ctx, [(address, unit stride) per input], (address, unit stride) of the output or None) makes the call
    and returns what the surface returns to the host.  Asserts that the far call returns the same and writes the same bytes, and that
    LAYOUT_GUARD bytes either side of every far output unit stay 0xCD.  Returns (host result, packed output [2][out_bytes] or None)."""
    n, G = 2, LAYOUT_GUARD
    ins = [np.ascontiguousarray(a, np.uint8).reshape(n, -1) for a in inputs]
    init = None
    if out_bytes:
        init = np.full((n, out_bytes), 0xCD, np.uint8) if out_init is None else np.ascontiguousarray(out_init, np.uint8).reshape(n, out_bytes)
    sizes = [a.shape[1] for a in ins] + ([out_bytes] if out_bytes else [])
    slot = FAR_OUT // 4
    assert len(sizes) <= 4 and max(sizes) + 2 * G <= slot
    ptrs, total = far_layout(max(sizes), [(k * FAR_FRAME,) for k in range(n)], slots=[j * slot for j in range(len(sizes))])
    ctx = lvm.Context(0, n_streams, lib)
    buf = None
    try:
        if setup:
            setup(ctx)
        d_ins = [mem.upload(a.reshape(-1)) for a in ins]
        d_out = mem.upload(init.reshape(-1)) if out_bytes else None
        ret = call(ctx, [(mem.ptr_at(d, 0), a.shape[1]) for d, a in zip(d_ins, ins)], (mem.ptr_at(d_out, 0), out_bytes) if out_bytes else None)
        mem.sync(ctx)
        want = np.array(mem.download(d_out), copy=True).reshape(n, out_bytes) if out_bytes else None
        assert want is None or (want != init).any(), "the surface wrote nothing"
        buf = mem.empty(total)
        for k in range(n):
            for j, a in enumerate(ins):
                mem.put(buf, ptrs[j] + k * FAR_FRAME, a[k])
            if out_bytes:
                mem.put(buf, ptrs[-1] + k * FAR_FRAME - G, np.concatenate([np.full(G, 0xCD, np.uint8), init[k], np.full(G, 0xCD, np.uint8)]))
        far_ret = call(ctx, [(mem.ptr_at(buf, p), FAR_FRAME) for p in ptrs[:len(ins)]], (mem.ptr_at(buf, ptrs[-1]), FAR_FRAME) if out_bytes else None)
        mem.sync(ctx)
        assert far_ret == ret, "the far call returned something else than the packed one"
        for k in range(n if out_bytes else 0):
            region = mem.get(buf, ptrs[-1] + k * FAR_FRAME - G, out_bytes + 2 * G)
            got = region[G:G + out_bytes]
            assert (region[:G] == 0xCD).all() and (region[G + out_bytes:] == 0xCD).all(), "unit %d: bytes beside the output were written" % k
            if not np.array_equal(got, want[k]):
                raise AssertionError("unit %d: %d bytes differ from the packed call (equal to the packed unit %s; untouched: %s)" % (
                    k, int((got != want[k]).sum()), [k2 for k2 in range(n) if np.array_equal(got, want[k2])], bool(np.array_equal(got, init[k]))))
        return ret, want
    finally:
        ctx.close()
        del buf
        mem.release()


def pipelined_clip(lvm, po, lib, mem, w, h, levels, nframes, ring=4, clip_fn=None, n_streams=1):
    """lvm_process_device with pipeline depth 1 over a ring of in/out buffers + flush, OpenCV-order Lab: every frame's
    output must equal the oracle's (and therefore the depth-0 schedule's) bit for bit.  n_streams > 1: every slot of the ring holds
    one frame of each stream ([stream][h][w][3]), each stream with a clip and an oracle of its own."""
    ck, pk = lvm.synth.config(0, (w, h, levels))
    clips = [_clip_of(lvm, clip_fn, ck, s) for s in range(n_streams)]
    P = po.make_params(**pk)
    cp = c_params(lvm, pk)
    ctx = lvm.Context(0, n_streams, lib)
    ctx.exact_lab(True)
    ctx.set_pipeline(1)
    orcs = [po.Oracle() for _ in range(n_streams)]
    d_in = mem.upload(np.zeros((ring, n_streams, h, w, 3), np.uint8))
    d_out = mem.zeros_like(d_in)
    st = mem.stream()
    refs = {}

    def same(got, t):
        bad = [s for s in range(n_streams) if not np.array_equal(got[s], refs[t][s])]
        assert not bad, "frame %d: streams %s differ from the oracle" % (t, bad)
    try:
        for t in range(nframes):
            k = t % ring
            if t >= ring:        # slot k is about to be reused: frame t-ring must already be complete
                mem.sync(ctx)
                same(mem.download(d_out)[k], t - ring)
            f = np.stack([c.frame(t) for c in clips])
            mem.write(d_in, k, f)
            refs[t] = np.stack([orcs[s].process(f[s], P)[0] for s in range(n_streams)])
            assert ctx.process_device(cp, mem.ptr(d_in, k), w, h, 3, w * 3, w * h * 3, mem.ptr(d_out, k), w * 3, w * h * 3, st)
        ctx.flush(st)
        mem.sync(ctx)
        got = mem.download(d_out)
        for t in range(max(0, nframes - ring), nframes):
            same(got[t % ring], t)
    finally:
        ctx.close()
        for o in orcs:
            o.close()


def two_streams_clip(lvm, po, lib, mem, w=96, h=64, levels=3, nframes=5, clip_fn=None):
    """A two-stream context through lvm_process_device, OpenCV-order Lab: each stream equals its own oracle bit for bit."""
    ck, pk = lvm.synth.config(0, (w, h, levels))
    clips = [_clip_of(lvm, clip_fn, ck, s) for s in range(2)]
    ctx = lvm.Context(0, 2, lib)
    ctx.exact_lab(True)
    orcs = [po.Oracle(), po.Oracle()]
    P = po.make_params(**pk)
    cp = c_params(lvm, pk)
    try:
        for t in range(nframes):
            fin = np.stack([c.frame(t) for c in clips])
            d_in = mem.upload(fin)
            d_out = mem.zeros_like(d_in)
            produced = ctx.process_device(cp, mem.ptr(d_in), w, h, 3, w * 3, w * h * 3, mem.ptr(d_out), w * 3, w * h * 3, mem.stream())
            mem.sync(ctx)
            assert produced
            fout = mem.download(d_out)
            for s in range(2):
                ref, _ = orcs[s].process(fin[s], P)
                assert np.array_equal(ref, fout[s]), "frame %d stream %d" % (t, s)
    finally:
        ctx.close()
        for o in orcs:
            o.close()


def padded_strides_clip(lvm, po, lib, mem, idx, pad_in, pad_out, w=96, h=64, levels=3, nframes=6, clip_fn=None):
    """lvm_process_device on frames whose rows are padded (a cv::Mat ROI view has step > cols * channels), OpenCV-order
    Lab: dword-aligned paddings keep the vectorised kernels, odd ones select the generic byte kernels; the padding bytes
    of the output must stay untouched and the frame must equal the oracle's bit for bit."""
    ck, pk = lvm.synth.config(idx, (w, h, levels))
    clip = _clip_of(lvm, clip_fn, ck, 0)
    P = po.make_params(**pk)
    cp = c_params(lvm, pk)
    ctx = lvm.Context(0, 1, lib)
    ctx.exact_lab(True)
    orc = po.Oracle()
    si, so = w * 3 + pad_in, w * 3 + pad_out
    try:
        for t in range(nframes):
            f = clip.frame(t)
            buf_in = np.full((h, si), 0xAB, np.uint8)
            buf_in[:, :w * 3] = f.reshape(h, w * 3)
            d_in = mem.upload(buf_in)
            d_out = mem.upload(np.full((h, so), 0xCD, np.uint8))
            ref, pr = orc.process(f, P)
            pg = ctx.process_device(cp, mem.ptr(d_in), w, h, 3, si, si * h, mem.ptr(d_out), so, so * h, mem.stream())
            mem.sync(ctx)
            assert pr == pg
            buf_out = mem.download(d_out)
            assert (buf_out[:, w * 3:] == 0xCD).all(), "padding bytes of the output were written"
            if pr:
                assert np.array_equal(buf_out[:, :w * 3].reshape(h, w, 3), ref), "frame %d" % t
    finally:
        ctx.close()
        orc.close()


# ---- schedule equivalence: one clip through every surface of the library ------------------------------------------------------
class HostMem:
    """'Device' buffers of the emulation build: host arrays."""
    def upload(self, a):
        return np.ascontiguousarray(a).copy()

    def zeros_like(self, a):
        return np.zeros_like(a)

    def ptr(self, a, i=0):
        return a[i].ctypes.data

    def ptr_at(self, a, byte_offset):
        """address of byte `byte_offset` of the uint8 buffer a"""
        assert a.dtype == np.uint8 and 0 <= byte_offset < a.size
        return a.ctypes.data + byte_offset

    def write(self, a, i, v):
        a[i][...] = v

    def empty(self, n):
        """n bytes, untouched: the pages are committed as they are written"""
        return np.empty(n, np.uint8)

    def put(self, a, byte_offset, v):
        a[byte_offset:byte_offset + v.size] = v

    def get(self, a, byte_offset, n):
        return a[byte_offset:byte_offset + n].copy()

    def release(self):
        """after the last reference to a large buffer is gone"""

    def download(self, a):
        return np.asarray(a)

    def stream(self):
        return None

    def call_stream(self):
        """the stream of the next device-surface call of a plan (run_plan)"""
        return None

    def quiesce(self):
        """run_plan: the caller waits for the device (the emulation has run everything already)"""

    def sync(self, ctx):
        ctx.synchronize()


class TorchMem:
    """Device buffers of the gfx950 build: torch tensors on the current HIP stream."""
    def __init__(self):
        import torch
        self.torch = torch

    def upload(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def zeros_like(self, a):
        return self.torch.zeros_like(a)

    def ptr(self, a, i=0):
        return a[i].data_ptr()

    def ptr_at(self, a, byte_offset):
        """address of byte `byte_offset` of the uint8 buffer a"""
        assert a.dtype == self.torch.uint8 and 0 <= byte_offset < a.numel()
        return a.data_ptr() + byte_offset

    def write(self, a, i, v):
        a[i].copy_(self.torch.from_numpy(np.ascontiguousarray(v)))

    def empty(self, n):
        """n bytes, untouched"""
        return self.torch.empty(n, dtype=self.torch.uint8, device="cuda")

    def put(self, a, byte_offset, v):
        a[byte_offset:byte_offset + v.size].copy_(self.torch.from_numpy(np.ascontiguousarray(v)))

    def get(self, a, byte_offset, n):
        self.torch.cuda.synchronize()
        return a[byte_offset:byte_offset + n].cpu().numpy()

    def release(self):
        """after the last reference to a large buffer is gone: hand it back to the device"""
        self.torch.cuda.synchronize()
        self.torch.cuda.empty_cache()

    def download(self, a):
        self.torch.cuda.synchronize()
        return a.cpu().numpy()

    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def call_stream(self):
        """the stream of the next device-surface call of a plan (run_plan): torch's current stream"""
        return self.stream()

    def quiesce(self):
        self.torch.cuda.synchronize()

    def sync(self, ctx):
        self.torch.cuda.synchronize()


def run_schedules(lvm, lib, mem, frames, other, pk, calls, pipeline=False):
    """The same clip (`frames`, [n][h][w][3] uint8) through the surfaces include/lvm_hip.h calls equivalent, shipped configuration
    (no keep_float, default flavour), packed rows (the layout lvm_process stages host frames in) in every schedule:
      host       lvm_process on host frames
      device     lvm_process_device, one frame per call
      frames     lvm_process_device_frames with the call lengths `calls`
      frames_max the same after lvm_set_max_frames(max(calls))
      pipelined  lvm_process_device at pipeline depth 1 + lvm_flush (pipeline=True: Laplace)
      stream1    lvm_process_device_frames on a 2-stream context, the clip as stream 1 and `other` as stream 0
      chain      lvm_chain_process_batch_ex with preprocessing off (Preprocess -> Grayscale -> Magnification)
    Returns {schedule: (produced flags, output frames)}; outputs of frames that were not produced are zeroed."""
    n, h, w, ch = frames.shape
    assert sum(calls) == n and other.shape == frames.shape
    fb = w * h * ch
    cp = c_params(lvm, pk)
    res = {}

    def finish(produced, out):
        out = out.copy()
        out[~np.asarray(produced, bool)] = 0
        return list(produced), out

    ctx = lvm.Context(0, 1, lib)
    try:
        outs, prod = np.zeros_like(frames), []
        for t in range(n):
            o, p = ctx.process(frames[t], cp)
            prod.append(p)
            if p:
                outs[t] = o
        res["host"] = finish(prod, outs)
    finally:
        ctx.close()

    d_in = mem.upload(frames)
    st = mem.stream()
    for name in ("device", "pipelined") if pipeline else ("device",):
        ctx = lvm.Context(0, 1, lib)
        try:
            if name == "pipelined":
                ctx.set_pipeline(1)
            d_out = mem.zeros_like(d_in)
            prod = [ctx.process_device(cp, mem.ptr(d_in, t), w, h, ch, w * ch, fb, mem.ptr(d_out, t), w * ch, fb, st) for t in range(n)]
            if name == "pipelined":
                ctx.flush(st)
            mem.sync(ctx)
            res[name] = finish(prod, mem.download(d_out))
        finally:
            ctx.close()

    for name, hint in (("frames", 0), ("frames_max", max(calls))):
        ctx = lvm.Context(0, 1, lib)
        try:
            if hint:
                ctx.set_max_frames(hint)
            d_out = mem.zeros_like(d_in)
            prod, t = [], 0
            for nf in calls:
                prod += ctx.process_device_frames(cp, nf, mem.ptr(d_in, t), w, h, ch, w * ch, fb, fb, mem.ptr(d_out, t), w * ch, fb, fb, st)
                t += nf
            mem.sync(ctx)
            res[name] = finish(prod, mem.download(d_out))
        finally:
            ctx.close()
    del d_in

    d_in2 = mem.upload(np.stack([other, frames], axis=1))          # [frame][stream][h][w][ch]: the clip is stream 1
    ctx = lvm.Context(0, 2, lib)
    try:
        d_out2 = mem.zeros_like(d_in2)
        prod, t = [], 0
        for nf in calls:
            prod += ctx.process_device_frames(cp, nf, mem.ptr(d_in2, t), w, h, ch, w * ch, fb, 2 * fb, mem.ptr(d_out2, t), w * ch, fb, 2 * fb, st)
            t += nf
        mem.sync(ctx)
        res["stream1"] = finish(prod, mem.download(d_out2)[:, 1])
    finally:
        ctx.close()
    del d_in2

    ctx = lvm.Context(0, 1, lib)
    pre = lvm.to_c_preprocess(lvm.PreprocessParams(), False)
    try:
        outs, prod = np.zeros_like(frames), []
        for t in range(n):
            o, _, p = ctx.chain_process_batch_ex([frames[t]], pre, cp)
            prod.append(p)
            if p:
                outs[t] = o[0]
        res["chain"] = finish(prod, outs)
    finally:
        ctx.close()
    return res


def assert_schedules_identical(res):
    """every schedule: the same produced flags and the same bytes as `host`, frame by frame"""
    prod0, out0 = res["host"]
    assert any(prod0), "no frame produced"
    for name, (prod, out) in res.items():
        assert prod == prod0, "%s: produced flags differ from lvm_process: %s" % (name, [t for t, (a, b) in enumerate(zip(prod, prod0)) if a != b])
        bad = [(t, int((out[t] != out0[t]).sum())) for t in range(len(prod0)) if prod0[t] and not np.array_equal(out[t], out0[t])]
        assert not bad, "%s differs from lvm_process: (frame, bytes) %s" % (name, bad[:8])


def oracle_bars(po, frames, pk, prod, outs, n_compare, u8_max=1, u8_frac=0.999):
    """the first n_compare frames of one schedule against the oracle at the parity bars; returns (worst diff, worst identical)"""
    P = po.make_params(**pk)
    orc = po.Oracle()
    worst = [0, 1.0]
    try:
        for t in range(n_compare):
            ref, pr = orc.process(frames[t], P)
            assert pr == prod[t], (t, pr, prod[t])
            if pr:
                du = np.abs(ref.astype(np.int32) - outs[t].astype(np.int32))
                worst = [max(worst[0], int(du.max())), min(worst[1], float((du == 0).mean()))]
                assert du.max() <= u8_max and (du == 0).mean() >= u8_frac, (t, int(du.max()), float((du == 0).mean()))
    finally:
        orc.close()
    return worst


def color_shrink_in_batches(lvm, po, lib, mem, size, calls, change_at, fps_to, u8_max, u8_frac):
    """Color mode through lvm_process_device_frames in the call lengths `calls`; the framerate falls from the clip's 60 to fps_to at
    the call that starts at frame change_at (SpatialFilter.cpp:80-83: the window cap shrinks, one column dropped per frame), so the
    following calls cross the shrink.  Every frame against the oracle."""
    ck, pk = lvm.synth.config(3, size)
    pk["coLow"], pk["coHigh"] = 0.5, 2.0
    clip = lvm.synth.Clip(**ck)
    w, h = ck["w"], ck["h"]
    n = sum(calls)
    frames = np.stack([clip.frame(t) for t in range(n)])
    assert change_at in np.cumsum((0,) + tuple(calls))
    fb = w * h * 3
    ctx = lvm.Context(0, 1, lib)
    d_in = mem.upload(frames)
    d_out = mem.zeros_like(d_in)
    prod, t, pks = [], 0, []
    try:
        for nf in calls:
            p = dict(pk, framerate=fps_to) if t >= change_at else pk
            pks += [p] * nf
            prod += ctx.process_device_frames(c_params(lvm, p), nf, mem.ptr(d_in, t), w, h, 3, w * 3, fb, fb, mem.ptr(d_out, t), w * 3, fb, fb,
                                              mem.stream())
            t += nf
        mem.sync(ctx)
        got = mem.download(d_out)
    finally:
        ctx.close()
    orc = po.Oracle()
    worst = [0, 1.0]
    try:
        for t in range(n):
            ref, pr = orc.process(frames[t], po.make_params(**pks[t]))
            assert pr == prod[t], (t, pr, prod[t])
            if pr:
                du = np.abs(ref.astype(np.int32) - got[t].astype(np.int32))
                worst = [max(worst[0], int(du.max())), min(worst[1], float((du == 0).mean()))]
                assert du.max() <= u8_max and (du == 0).mean() >= u8_frac, (t, int(du.max()), float((du == 0).mean()))
    finally:
        orc.close()
    return worst


# ---- surface mix: ONE context through a seeded interleaving of its surfaces (tests/test_surface_mix.py) -----------------------------
def _chain_key():
    """What lvm_chain_process_batch_ex and lvm_export_frames put into lvm_params.preprocess_key for "preprocessing off" (csrc/lvm_api.hip
    preprocess_key_of: FNV-1a over downscale, roi_enabled, roiX, roiY, roiW, roiH).  The device surfaces of a plan pass the same value, so
    that every surface drives the SAME magnifier state; a wrong value here shows as a structural reset the oracle does not make."""
    import struct
    k = 1469598103934665603
    for b in struct.pack("<iiffff", 1, 0, 0.0, 0.0, 1.0, 1.0):
        k = ((k ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return k


CHAIN_KEY = _chain_key()
# lengths of lvm_process_device_frames calls and how often each is drawn (cut to the frames that are left: the long ones end a plan)
PLAN_BATCHES = (1, 2, 3, 4, 5, 7, 9, 16, 33)
PLAN_BATCH_P = (0.15, 0.25, 0.2, 0.12, 0.1, 0.08, 0.05, 0.03, 0.02)
FRAME_OPS = ("host", "device", "frames", "chain", "export")


class StreamMem(TorchMem):
    """TorchMem for plans whose device-surface calls go to real caller streams: `n_streams` torch.cuda.Stream() objects and, with
    own=True, None (the context's own stream), drawn per call from `seed` (cycle=True: the streams in turn).

    The caller's duties and nothing more: the chosen stream waits for the upload of its input (wait_stream), buffers live until the
    end, results are read after torch.cuda.synchronize() (download).  Nothing orders one call of the context behind the previous one:
    that is the library's job.  To make the order impossible to get right by luck, every other call (a "late" one) first puts a
    device-side delay on its stream -- long enough that the stream is free DELAY_MS after every other stream, by this class's own
    account of the delays it has issued -- and the call after it (an "early" one) goes undelayed to ANOTHER stream or to a host
    surface: without cross-stream ordering it runs at least 20 ms before the call it follows."""
    DELAY_MS = 25.0
    _cycles_per_ms = None

    def __init__(self, seed, n_streams=4, own=True, cycle=False):
        super().__init__()
        t = self.torch
        self.pool = [t.cuda.Stream() for _ in range(n_streams)]
        self.own, self.cycle = own, cycle
        self.rng = np.random.default_rng(seed)
        self.busy = [0.0] * n_streams            # ms of delay issued to each stream since the last quiesce
        self.prev, self.late, self.turn = None, True, 0
        self.log = []                            # (stream index or -1 for the own stream, late) per call
        self._calibrate()

    def _time_sleep(self, cycles):
        t = self.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        t.cuda._sleep(int(cycles))
        e1.record()
        t.cuda.synchronize()
        return e0.elapsed_time(e1)

    def _calibrate(self):
        """torch.cuda._sleep counts ticks of a clock whose rate is the device's business: measured once, and the delay the plans use
        is measured to be the 20 ms they rely on"""
        cls = StreamMem
        if cls._cycles_per_ms is None:
            self._time_sleep(1000)               # (loads the kernel)
            n, ms = 1000000, 0.0
            for _ in range(4):
                ms = self._time_sleep(n)
                if ms >= 5.0:
                    break
                n *= 8
            assert ms >= 5.0, "torch.cuda._sleep(%d) took %.3f ms" % (n, ms)
            cls._cycles_per_ms = n / ms
            got = self._time_sleep(self.DELAY_MS * cls._cycles_per_ms)
            assert got >= 20.0, "a delay meant to take %.0f ms took %.2f ms" % (self.DELAY_MS, got)

    def handles(self):
        return [s.cuda_stream for s in self.pool]

    def call_stream(self):
        t, n = self.torch, len(self.pool)
        if self.cycle:
            k = self.turn % n
            self.turn += 1
        else:
            choices = [i for i in range(-1 if self.own else 0, n) if self.late or i != self.prev]
            k = int(self.rng.choice(choices))
        if k >= 0:
            self.pool[k].wait_stream(t.cuda.current_stream())          # the upload of the call's input
            if self.late:
                target = max(self.busy) + self.DELAY_MS
                with t.cuda.stream(self.pool[k]):
                    t.cuda._sleep(int((target - self.busy[k]) * self._cycles_per_ms))
                self.busy[k] = target
        self.log.append((k, self.late))
        self.prev, self.late = k, not self.late
        return self.pool[k].cuda_stream if k >= 0 else 0

    def quiesce(self):
        self.torch.cuda.synchronize()
        self.busy = [0.0] * len(self.pool)


def draw_plan(seed, n_frames, mode, n_streams=1, warm=0, fps=30.0):
    """A seeded interleaving of the operations one context takes, consuming n_frames consecutive frames:
      ("host",) lvm_process    ("device",) lvm_process_device    ("frames", n) lvm_process_device_frames, n of PLAN_BATCHES
      ("chain",) lvm_chain_process_batch_ex, preprocessing off    ("export", n) ONE lvm_export_frames segment, split None
      ("pipeline", 0 | 1) lvm_set_pipeline    ("flush",) lvm_flush    ("max_frames", n) lvm_set_max_frames
      ("set", {...}) an amplification or cutoff change from the next frame on    ("reset",) lvm_reset
    The first `warm` frames go one per call (Color: the window fills before the first batch).  lvm_reset discards an owed pipelined
    frame by contract, so a flush stands in front of every reset that could meet one, and at the end.  n_streams > 1 leaves out the
    surfaces that take 1-stream contexts only (lvm_process, lvm_export_frames)."""
    r = np.random.default_rng(7000 + seed)
    kinds = ["device", "frames", "host", "chain", "export", "pipeline", "flush", "max_frames", "set", "reset"]
    weights = np.array([0.22, 0.28, 0.12, 0.08, 0.05, 0.06, 0.05, 0.04, 0.07, 0.03])
    if n_streams > 1:
        weights[[2, 4]] = 0.0
    weights = weights / weights.sum()
    plan, t, depth, owed, exported = [], 0, 0, False, False
    while t < n_frames:
        k = str(r.choice(kinds, p=weights))
        left = n_frames - t
        if k == "device":
            plan.append((k,)); t += 1; owed = depth == 1
        elif k == "frames":
            n = 1 if t < warm else min(left, int(r.choice(PLAN_BATCHES, p=PLAN_BATCH_P)))
            plan.append((k, n)); t += n; owed = depth == 1           # (at depth 1 Laplace takes the frames one by one and owes the last)
        elif k in ("host", "chain"):
            plan.append((k,)); t += 1; owed = False                  # the synchronous surfaces complete what is owed
        elif k == "export":
            if exported or t < warm or left < 2:
                continue
            n = min(left, int(r.integers(2, 8)))
            plan.append((k, n)); t += n; owed, exported = False, True
        elif k == "pipeline":
            depth = depth ^ int(r.random() < 0.75)                   # (mostly a change; setting the depth it has is a call too)
            plan.append((k, depth)); owed = owed and depth == 1      # (a change flushes)
        elif k == "flush":
            plan.append((k,)); owed = False
        elif k == "max_frames":
            plan.append((k, int(r.choice([1, 2, 4, 8, 16, 33]))))
        elif k == "set":
            if r.random() < 0.5:
                plan.append((k, {"amplification": float(r.uniform(1.0, 80.0))}))
            elif mode == 0:          # Laplace: IIR blend factors
                lo = float(r.uniform(0.01, 0.5))
                plan.append((k, {"coLow": lo, "coHigh": float(r.uniform(lo + 0.05, 0.999))}))
            elif mode == 1:          # Riesz: Butterworth band in Hz
                lo = float(r.uniform(0.1, 0.3 * fps))
                plan.append((k, {"coLow": lo, "coHigh": float(r.uniform(lo + 0.1, 0.49 * fps))}))
            else:                    # Color: ideal band in Hz
                lo = float(r.uniform(0.1, 0.2 * fps))
                plan.append((k, {"coLow": lo, "coHigh": float(r.uniform(lo + 0.05, 0.45 * fps))}))
        else:
            if owed:
                plan.append(("flush",))
            plan.append((k,)); owed = False
    if owed:
        plan.append(("flush",))
    return plan


def plan_frames(plan):
    return sum(op[1] if op[0] in ("frames", "export") else 1 for op in plan if op[0] in FRAME_OPS)


def plan_reference(po, plan, frames, pk, key=CHAIN_KEY):
    """The oracle over the frames of a plan ([n][stream][h][w][ch]), one oracle per stream: frame after frame with the parameters in
    force, reset where the plan resets.  Returns (produced flags [n], frames [n][stream]...; a frame that was not produced: zeros)."""
    n, S = frames.shape[:2]
    assert plan_frames(plan) == n
    orcs = [po.Oracle() for _ in range(S)]
    prod, out = [], np.zeros_like(frames)
    cur, t = dict(pk), 0
    try:
        for op in plan:
            if op[0] == "set":
                cur.update(op[1])
            elif op[0] == "reset":
                for o in orcs:
                    o.reset()
            elif op[0] in FRAME_OPS:
                P = po.make_params(preprocess_key=key, **cur)
                for _ in range(op[1] if len(op) > 1 else 1):
                    flags = set()
                    for s in range(S):
                        ref, pr = orcs[s].process(frames[t, s], P)
                        flags.add(bool(pr))
                        if pr:
                            out[t, s] = ref
                    assert len(flags) == 1
                    prod.append(flags.pop())
                    t += 1
    finally:
        for o in orcs:
            o.close()
    return prod, out


def run_plan(lvm, lib, mem, plan, frames, pk, key=CHAIN_KEY, exact_lab=True):
    """One context through `plan` (draw_plan) on `frames` ([n][stream][h][w][3]); device-surface calls and flushes go to
    mem.call_stream().  All buffers live until the end and every output is read once, after the last operation (in pipelined mode:
    after the flush that completes it).  Before lvm_reset, before a temporal batch longer than any since the state was built (its
    buffers grow: a free) and before the context is destroyed the caller waits for the device (mem.quiesce): whether those paths wait
    for every caller stream by themselves is not this function's question.
    Returns {"prod": flags [n], "out": [n][stream][h][w][3], "op": index of the operation that took frame t, "crop": {t: (rows, cols)}
    for frames that came back as export canvases, "pass": what a frame that was not produced must hold (zeros = untouched, or the input)}."""
    n, S, h, w, ch = frames.shape
    assert plan_frames(plan) == n and ch == 3
    fb = w * h * ch
    ctx = lvm.Context(0, S, lib)
    res = {"prod": [None] * n, "op": [None] * n, "crop": {}, "pass": np.zeros_like(frames)}
    host_out = {}
    pre = lvm.to_c_preprocess(lvm.PreprocessParams(), False)
    try:
        ctx.exact_lab(exact_lab)
        d_in = mem.upload(frames)
        d_out = mem.zeros_like(d_in)
        cur, t, hint, cap = dict(pk), 0, 0, 0
        for k, op in enumerate(plan):
            cp = c_params(lvm, cur, key)
            nf = (op[1] if len(op) > 1 else 1) if op[0] in FRAME_OPS else 0
            res["op"][t:t + nf] = [k] * nf
            if op[0] == "set":
                cur.update(op[1])
            elif op[0] == "reset":
                mem.quiesce()
                ctx.reset()
                cap = hint
            elif op[0] == "pipeline":
                ctx.set_pipeline(op[1])
            elif op[0] == "flush":
                ctx.flush(mem.call_stream())
            elif op[0] == "max_frames":
                ctx.set_max_frames(op[1])
                hint = op[1]
            elif op[0] == "device":
                res["prod"][t] = ctx.process_device(cp, mem.ptr(d_in, t), w, h, ch, w * ch, fb, mem.ptr(d_out, t), w * ch, fb, mem.call_stream())
            elif op[0] == "frames":
                if nf > cap:
                    mem.quiesce()
                    cap = max(nf, hint)
                res["prod"][t:t + nf] = ctx.process_device_frames(cp, nf, mem.ptr(d_in, t), w, h, ch, w * ch, fb, fb * S, mem.ptr(d_out, t),
                                                                  w * ch, fb, fb * S, mem.call_stream())
            elif op[0] == "host":
                o, p = ctx.process(frames[t, 0], cp)
                res["prod"][t], host_out[t] = p, np.array(o, copy=True)[None]
                res["pass"][t] = frames[t]
            elif op[0] == "chain":
                outs, _, p = ctx.chain_process_batch_ex(list(frames[t]), pre, cp)
                res["prod"][t], host_out[t] = p, np.stack(outs)
                res["pass"][t] = frames[t]                 # passthrough: the frame the magnifier saw
            elif op[0] == "export":
                if nf > cap:                               # (the export hands its frames on in sub-batches; the rule above, whatever their length)
                    mem.quiesce()
                    cap = max(nf, hint)
                canv, prods = ctx.export_frames(list(frames[t:t + nf, 0]), pre, cp, 0)
                for f in range(nf):
                    res["prod"][t + f] = prods[f]
                    hh, ww = canv[f].shape[:2]
                    res["crop"][t + f] = (hh, ww)          # Exporter::compose crops to even sizes
                    full = np.zeros((1, h, w, ch), np.uint8)
                    full[0, :hh, :ww] = canv[f]
                    host_out[t + f] = full
                    res["pass"][t + f] = frames[t + f]
            else:
                raise ValueError(op)
            t += nf
        out = mem.download(d_out).copy()
        for t_, o in host_out.items():
            out[t_] = o
        res["out"] = out
        mem.quiesce()
    finally:
        ctx.close()
    return res


def _plan_fail(plan, res, t, msg):
    k = res["op"][t]
    raise AssertionError("frame %d (operation %d of %d, %r): %s\nthe operations up to it: %s" % (t, k, len(plan), plan[k], msg, plan[max(0, k - 9):k + 1]))


def check_plan(plan, ref, res, exact=True, u8_max=1, u8_frac=0.999):
    """Every frame of a plan's run against plan_reference: the produced flags; a produced frame byte for byte (exact) or at the
    parity bars; a frame that was not produced is the input (host surfaces) or untouched.  A failure names the frame, the byte count
    and the last ten operations.  Returns [worst u8 diff, worst identical fraction]."""
    prod_r, out_r = ref
    worst = [0, 1.0]
    for t in range(len(prod_r)):
        if res["prod"][t] != prod_r[t]:
            _plan_fail(plan, res, t, "produced flag %s, the oracle's %s" % (res["prod"][t], prod_r[t]))
        hh, ww = res["crop"].get(t, out_r.shape[2:4])
        for s in range(out_r.shape[1]):
            got = res["out"][t, s, :hh, :ww]
            want = (out_r if prod_r[t] else res["pass"])[t, s, :hh, :ww]
            du = np.abs(want.astype(np.int32) - got.astype(np.int32))
            worst = [max(worst[0], int(du.max())), min(worst[1], float((du == 0).mean()))]
            if (exact or not prod_r[t]) and du.max() != 0:
                _plan_fail(plan, res, t, "stream %d: %d of %d bytes differ from the oracle (max %d)" % (s, int((du != 0).sum()), du.size, int(du.max())))
            if du.max() > u8_max or (du == 0).mean() < u8_frac:
                _plan_fail(plan, res, t, "stream %d: u8 diff %d, identical %.6f: outside the bars (%d bytes differ)" % (
                    s, int(du.max()), float((du == 0).mean()), int((du != 0).sum())))
    return worst


def check_plans_identical(plan, res_a, res_b):
    """two runs of one plan, byte for byte"""
    assert res_a["prod"] == res_b["prod"], (res_a["prod"], res_b["prod"])
    for t in range(len(res_a["prod"])):
        if not np.array_equal(res_a["out"][t], res_b["out"][t]):
            _plan_fail(plan, res_a, t, "%d bytes differ between the two runs" % int((res_a["out"][t] != res_b["out"][t]).sum()))
