#!/usr/bin/env python3
"""Motion-JPEG encode on the device, measured (run on a GPU box: `gpurun -- 'python tools/mjpeg_bench.py > gpurun_out/mjpeg.txt'`):
  1. lvm_mjpeg_encode_device on device-resident 3840 x 1080 canvases (the export's side-by-side shape): frames/s, bytes per frame, the
     five kernels (HIP events, lvm_profile_*);
  2. the export surface host -> host: lvm_export_frames (canvases down, 12.4 MB each) against lvm_export_frames_mjpeg (JPEG frames down),
     page-locked buffers, 32 frames per call;
  3. libjpeg (Pillow) encoding the same canvas on one host core, for scale.
With --parent LIB (a liblvm_hip.so built from the parent commit) it instead alternates that library and this one on the two encode cases: against_parent().
"""
import ctypes as C
import importlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lvm = importlib.import_module("live-video-magnification_amd")


def main():
    import torch
    lib = lvm.load()
    q = int(os.environ.get("MJ_QUALITY", "85"))
    ck, pk = lvm.synth.config(1)                      # 1080p Laplace clip
    clip = lvm.synth.Clip(seed=1234, **ck)
    w, h = ck["w"], ck["h"]
    frames = np.stack([clip.frame(t) for t in range(8)])
    canvas = np.concatenate([frames, frames[::-1]], axis=2)          # 3840 x 1080 side by side
    cw, chh = 2 * w, h
    T = 8
    d = torch.from_numpy(canvas).cuda()
    ctx = lvm.Context(0, 1)
    out = ctx.mjpeg_encode_device(C.c_void_p(d.data_ptr()), cw, chh, T, quality=q)
    sizes = [len(x) for x in out]
    print("canvas %dx%d quality %d: %.0f KB per frame (%.2f bits/pixel, %.1f x smaller than the 12.4 MB canvas)" % (
        cw, chh, q, np.mean(sizes) / 1e3, 8 * np.mean(sizes) / (cw * chh), cw * chh * 3 / np.mean(sizes)))
    cap = int(lib.lvm_mjpeg_bound(cw, chh)) * T
    buf = np.empty(cap, np.uint8)
    offs = (C.c_size_t * (T + 1))()
    for _ in range(3):
        ctx._check(lib.lvm_mjpeg_encode_device(ctx.h, d.data_ptr(), cw, chh, cw * 3, cw * 3 * chh, T, q, buf.ctypes.data, cap, offs))
    K = 20
    t0 = time.perf_counter()
    for _ in range(K):
        ctx._check(lib.lvm_mjpeg_encode_device(ctx.h, d.data_ptr(), cw, chh, cw * 3, cw * 3 * chh, T, q, buf.ctypes.data, cap, offs))
    dt = time.perf_counter() - t0
    print("lvm_mjpeg_encode_device (device frames in, JPEG on the host out, %d frames per call, pageable output): %.0f frames/s, %.1f us per frame" % (
        T, K * T / dt, 1e6 * dt / (K * T)))
    ctx.profile(True)
    for _ in range(5):
        ctx._check(lib.lvm_mjpeg_encode_device(ctx.h, d.data_ptr(), cw, chh, cw * 3, cw * 3 * chh, T, q, buf.ctypes.data, cap, offs))
    prof = ctx.profile_collect()
    ctx.profile(False)
    tot = 0.0
    for name, (ms, cnt) in prof.items():
        if name.startswith("mj_"):
            print("  %-14s %8.1f us per launch of %d frames (%d launches)" % (name, 1e3 * ms / max(cnt, 1), T, cnt))
            tot += 1e3 * ms / max(cnt, 1)
    print("  kernels: %.1f us per %d frames = %.1f us per frame" % (tot, T, tot / T))
    ctx.close()

    # host -> host export, canvases against JPEG frames
    Te = 32
    host = np.stack([clip.frame(t) for t in range(16)])
    fb, cb = h * w * 3, cw * chh * 3
    cpre = lvm.LvmPreprocessParams(1, 0, 0.0, 0.0, 1.0, 1.0, 0)
    from tests_helpers_shim import c_params  # noqa
    cp = c_params(lvm, pk)
    pin, pout, pj = C.c_void_p(), C.c_void_p(), C.c_void_p()
    jcap = int(np.max(sizes) * 1.5) * Te
    assert lib.lvm_host_alloc(fb * Te, C.byref(pin)) == 0 and lib.lvm_host_alloc(cb * Te, C.byref(pout)) == 0 and lib.lvm_host_alloc(jcap, C.byref(pj)) == 0
    src = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), shape=(Te, h, w, 3))
    for i in range(Te):
        src[i] = host[i % 16]
    vp = C.c_void_p
    pi = (vp * Te)(*[pin.value + i * fb for i in range(Te)])
    pc = (vp * Te)(*[pout.value + i * cb for i in range(Te)])
    prod = (C.c_int * Te)()
    joffs = (C.c_size_t * (Te + 1))()
    for name in ("canvases", "mjpeg chunk 2", "mjpeg chunk 4", "mjpeg chunk 8", "mjpeg chunk 16"):
        if name.startswith("mjpeg"):
            os.environ["LVM_EXPORT_MJPEG_CHUNK"] = name.split()[-1]
        ex = lvm.Context(0, 1)
        ex.set_max_frames(Te)

        def call():
            if name == "canvases":
                ex._check(lib.lvm_export_frames(ex.h, C.byref(cpre), C.byref(cp), 1, Te, pi, w, h, 3, w * 3, pc, cw * 3, prod))
            else:
                ex._check(lib.lvm_export_frames_mjpeg(ex.h, C.byref(cpre), C.byref(cp), 1, Te, pi, w, h, 3, w * 3, q, pj, jcap, joffs, prod))
        for _ in range(2):
            call()
        Kx = 6
        t0 = time.perf_counter()
        for _ in range(Kx):
            call()
        dx = time.perf_counter() - t0
        down = cb if name == "canvases" else joffs[Te] / Te
        print("export host -> host, %-14s: %7.0f frames/s (%.1f us per frame; %.2f MB up + %.2f MB down per frame)" % (
            name, Kx * Te / dx, 1e6 * dx / (Kx * Te), fb / 1e6, down / 1e6))
        ex.close()
    # the decode half: 1080p frames as this repository's encoder writes them (68 restart intervals each) and as libjpeg writes them (none)
    dctx = lvm.Context(0, 1)
    dsrc = torch.from_numpy(frames).cuda()
    own8 = dctx.mjpeg_encode_device(C.c_void_p(dsrc.data_ptr()), w, h, 8, quality=90)              # the default: restart intervals of 8 MCUs
    dctx.mjpeg_set_restart_interval((w + 15) // 16)
    own = dctx.mjpeg_encode_device(C.c_void_p(dsrc.data_ptr()), w, h, 8, quality=90)               # one interval per MCU row
    dctx.mjpeg_set_restart_interval(0)
    print("restart intervals of 8 MCUs (default) against one per MCU row: %.0f KB per frame against %.0f (+%.2f %%)" % (
        np.mean([len(x) for x in own8]) / 1e3, np.mean([len(x) for x in own]) / 1e3, 100.0 * (sum(len(x) for x in own8) / sum(len(x) for x in own) - 1)))
    kinds = [("this encoder's frames, restart interval = 8 MCUs, the default (1020 lanes per frame)", own8), ("this encoder's frames, restart interval = MCU row (68 lanes per frame)", own)]
    try:
        from PIL import Image
        lj = []
        for k in range(8):
            b = io.BytesIO()
            Image.fromarray(frames[k][..., ::-1]).save(b, "JPEG", quality=90, subsampling=2)
            lj.append(b.getvalue())
        kinds.append(("libjpeg's frames (no restart markers: self-synchronising lanes of 1024 bits)", lj))
    except Exception:
        pass
    # (Huffman decoding is serial inside a restart interval: a call's time is the latency of ONE interval, whatever the number of frames)
    for label, js8 in kinds:
        for nd in (8, 64):
            js = (js8 * 8)[:nd]
            dout = torch.zeros((nd, h, w, 3), dtype=torch.uint8, device="cuda")
            blob = np.frombuffer(b"".join(js), np.uint8)
            offsn = (C.c_size_t * (nd + 1))(*np.concatenate([[0], np.cumsum([len(j) for j in js])]).tolist())
            dctx._check(lib.lvm_mjpeg_decode_device(dctx.h, blob.ctypes.data, offsn, nd, w, h, dout.data_ptr(), w * 3, w * 3 * h))
            Kd = 3
            t0 = time.perf_counter()
            for _ in range(Kd):
                dctx._check(lib.lvm_mjpeg_decode_device(dctx.h, blob.ctypes.data, offsn, nd, w, h, dout.data_ptr(), w * 3, w * 3 * h))
            dt = time.perf_counter() - t0
            print("lvm_mjpeg_decode_device, %2d x 1080p, %s: %.0f frames/s (%.1f ms per call, %.0f KB per frame)" % (
                nd, label, Kd * nd / dt, 1e3 * dt / Kd, len(blob) / nd / 1e3))
            del dout
    dctx.close()
    # file -> file: JPEG frames in, JPEG frames of the composed canvases out
    for label, ownk in (("inputs with restart intervals of 8 MCUs (this encoder's default)", own8), ("inputs with one restart interval per MCU row", own)):
        jin = (ownk * 4)[:Te]
        blob = np.frombuffer(b"".join(jin), np.uint8)
        pjin = C.c_void_p()
        assert lib.lvm_host_alloc(len(blob), C.byref(pjin)) == 0
        C.memmove(pjin, blob.ctypes.data, len(blob))
        ioffs = (C.c_size_t * (Te + 1))(*np.concatenate([[0], np.cumsum([len(j) for j in jin])]).tolist())
        os.environ["LVM_EXPORT_MJPEG_CHUNK"] = "4"
        ex = lvm.Context(0, 1)
        ex.set_max_frames(Te)
        for _ in range(2):
            ex._check(lib.lvm_export_mjpeg_frames(ex.h, C.byref(cpre), C.byref(cp), 1, Te, pjin, ioffs, w, h, q, pj, jcap, joffs, prod))
        t0 = time.perf_counter()
        for _ in range(6):
            ex._check(lib.lvm_export_mjpeg_frames(ex.h, C.byref(cpre), C.byref(cp), 1, Te, pjin, ioffs, w, h, q, pj, jcap, joffs, prod))
        dx = time.perf_counter() - t0
        print("export JPEG -> JPEG (lvm_export_mjpeg_frames), %s: %7.0f frames/s (%.1f us per frame; %.2f MB up + %.2f MB down per frame)" % (
            label, 6 * Te / dx, 1e6 * dx / (6 * Te), len(blob) / Te / 1e6, joffs[Te] / Te / 1e6))
        ex.close()
        lib.lvm_host_free(pjin)
    try:
        from PIL import Image
        im = Image.fromarray(canvas[0][..., ::-1])
        t0 = time.perf_counter()
        for _ in range(5):
            b = io.BytesIO()
            im.save(b, "JPEG", quality=q, subsampling=2)
        dt = (time.perf_counter() - t0) / 5
        print("libjpeg-turbo (Pillow %s) on one host core, the same canvas: %.1f frames/s (%.1f ms per frame, %d KB)" % (
            importlib.import_module("PIL").__version__, 1 / dt, 1e3 * dt, len(b.getvalue()) // 1000))
    except Exception as e:
        print("Pillow not available:", e)


def against_parent(parent):
    """--parent LIB: the parent commit's library and this one, each on a fresh context of its own, alternating call by call in one process (who goes
    first alternates too) after warm-up calls, on two cases: lvm_mjpeg_encode_device on eight 3840 x 1080 canvases (page-locked output), and
    lvm_export_frames_mjpeg at 1080p side by side, 32 page-locked frames per call.  Per case: both sides' call times (host clock around the synchronous
    call), whether the output bytes are identical, and the per-launch times of the mj_* rows (HIP events, lvm_profile_*: one figure per profiled call,
    the two sides alternating again).  The bar for the call time and for every row: this library's median inside the parent's own min .. max."""
    import torch
    from tests_helpers_shim import c_params
    lib, old = lvm.load(), lvm.bind(C.CDLL(parent))
    q, reps, passes = int(os.environ.get("MJ_QUALITY", "85")), int(os.environ.get("MJ_REPS", "20")), int(os.environ.get("MJ_PASSES", "10"))
    ck, pk = lvm.synth.config(1)
    clip = lvm.synth.Clip(seed=1234, **ck)
    w, h = ck["w"], ck["h"]
    frames = np.stack([clip.frame(t) for t in range(16)])
    cw, chh, T, Te = 2 * w, h, 8, 32
    d = torch.from_numpy(np.concatenate([frames[:8], frames[:8][::-1]], axis=2)).cuda()
    fb = h * w * 3
    jcap, jcap_e = (3 << 20) * T, (3 << 20) * Te       # (these canvases take 1.2 MB each at quality 85; a buffer too small is an error, not a figure)
    pin, pj = C.c_void_p(), C.c_void_p()
    assert lib.lvm_host_alloc(fb * Te, C.byref(pin)) == 0 and lib.lvm_host_alloc(jcap_e, C.byref(pj)) == 0
    src = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), shape=(Te, h, w, 3))
    for i in range(Te):
        src[i] = frames[i % 16]
    out = np.ctypeslib.as_array(C.cast(pj, C.POINTER(C.c_uint8)), shape=(jcap_e,))
    pi = (C.c_void_p * Te)(*[pin.value + i * fb for i in range(Te)])
    prod = (C.c_int * Te)()
    cpre, cp = lvm.LvmPreprocessParams(1, 0, 0.0, 0.0, 1.0, 1.0, 0), c_params(lvm, pk)
    offs = (C.c_size_t * (Te + 1))()

    def encode(cx, lb):
        cx._check(lb.lvm_mjpeg_encode_device(cx.h, d.data_ptr(), cw, chh, cw * 3, cw * 3 * chh, T, q, pj, jcap, offs))
        return T

    def export(cx, lb):
        cx._check(lb.lvm_export_frames_mjpeg(cx.h, C.byref(cpre), C.byref(cp), 1, Te, pi, w, h, 3, w * 3, q, pj, jcap_e, offs, prod))
        return Te

    print("the parent commit's library against this one, alternating call by call (%d timed calls each after 3 warm-up calls, then %d profiled calls each), fresh contexts per case:" % (2 * reps, passes))
    for label, call in (("lvm_mjpeg_encode_device, %d canvases of %d x %d, quality %d" % (T, cw, chh, q), encode),
                        ("lvm_export_frames_mjpeg, %d x %d side by side, %d page-locked frames per call, quality %d" % (w, h, Te, q), export)):
        sides = (("parent", lvm.Context(0, 1, old), old), ("this", lvm.Context(0, 1), lib))
        for _n, cx, _l in sides:
            cx.set_max_frames(Te)
        ms = {name: [] for name, _c, _l in sides}
        for it in range(3 + 2 * reps):
            for name, cx, lb in sides[::1 - 2 * (it & 1)]:
                t0 = time.perf_counter()
                call(cx, lb)
                if it >= 3:
                    ms[name].append(1e3 * (time.perf_counter() - t0))
        print("  " + label + ":")
        for name, _c, _l in sides:
            v = np.sort(ms[name])
            print("    %-6s median %.3f ms per call (min %.3f, max %.3f)" % (name, np.median(v), v[0], v[-1]))
        po, med = np.sort(ms["parent"]), float(np.median(ms["this"]))
        print("    this library's median lies %s the parent's min .. max (%+.1f %% against the parent's median)" % (
            "INSIDE" if po[0] <= med <= po[-1] else "OUTSIDE", 100 * (med / np.median(po) - 1)))
        got = []
        for name, cx, lb in sides:
            out[:] = 0xEE
            n = call(cx, lb)
            got.append((out[:offs[n]].tobytes(), list(offs[:n + 1])))
        print("    output: %s (%d bytes)" % ("byte-identical on both sides" if got[0] == got[1] else "DIFFERENT", len(got[1][0])))
        rows = {name: {} for name, _c, _l in sides}
        for it in range(passes):
            for name, cx, lb in sides[::1 - 2 * (it & 1)]:
                cx.profile_only(None)                  # (clears the totals)
                cx.profile(True)
                call(cx, lb)
                prof = cx.profile_collect()
                cx.profile(False)
                for kn, (t, cnt) in prof.items():
                    if kn.startswith("mj_") and cnt:
                        rows[name].setdefault(kn, []).append(1e3 * t / cnt)
        for kn in sorted(rows["this"]):
            a, b = np.sort(rows["parent"].get(kn, [0.0])), np.sort(rows["this"][kn])
            print("      %-18s parent median %8.2f us per launch (min %.2f, max %.2f), this %8.2f (min %.2f, max %.2f): %s" % (
                kn, np.median(a), a[0], a[-1], np.median(b), b[0], b[-1], "INSIDE" if a[0] <= np.median(b) <= a[-1] else "OUTSIDE"))
        for _n, cx, _l in sides:
            cx.close()
    lib.lvm_host_free(pin)
    lib.lvm_host_free(pj)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as tests_helpers_shim
    sys.modules["tests_helpers_shim"] = tests_helpers_shim
    if "--parent" in sys.argv:
        against_parent(sys.argv[sys.argv.index("--parent") + 1])
    else:
        main()
