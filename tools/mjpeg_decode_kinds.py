#!/usr/bin/env python3
"""The two decode arithmetics of lvm_mjpeg_decode_device side by side on the GPU (lvm_mjpeg_set_decoder): LVM_MJPEG_DECODER_REPLICATE (k_mjd_pixels)
against LVM_MJPEG_DECODER_LIBJPEG (k_mjd_chroma_islow + k_mjd_pixels_libjpeg), in ONE process on ONE context, alternating:
  1. per-launch times of the pixel stage (HIP events around the launches, lvm_profile_*), 32 frames of 1920 x 1080, quality 90, per call;
  2. the whole call (host clock around the synchronous call), median of repeated calls, for streams with one restart interval per MCU row
     and with the encoder's default of 8 MCUs (the entropy stage in front is shared and dominates the first).
Prints to stdout; profiles/r07_mjpeg_decode_kinds.txt is a run of it."""
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lvm = importlib.import_module("live-video-magnification_amd")

KINDS = ((lvm.MJPEG_DECODER_REPLICATE, "replicate"), (lvm.MJPEG_DECODER_LIBJPEG, "libjpeg"))


def main():
    import torch
    lib = lvm.load()
    n, reps = int(os.environ.get("MJD_FRAMES", "32")), int(os.environ.get("MJD_REPS", "15"))
    ck, _ = lvm.synth.config(1)                       # the 1080p clip
    clip = lvm.synth.Clip(seed=1234, **ck)
    w, h = ck["w"], ck["h"]
    frames = np.stack([clip.frame(t) for t in range(8)])
    ctx = lvm.Context(0, 1)
    src = torch.from_numpy(frames).cuda()
    own8 = ctx.mjpeg_encode_device(C.c_void_p(src.data_ptr()), w, h, 8, quality=90)
    ctx.mjpeg_set_restart_interval((w + 15) // 16)
    row = ctx.mjpeg_encode_device(C.c_void_p(src.data_ptr()), w, h, 8, quality=90)
    ctx.mjpeg_set_restart_interval(0)
    out = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    print("%d frames of %d x %d, quality 90, per call; %d timed calls per figure after 3 warm-up calls, kinds alternating" % (n, w, h, reps))
    for label, js8 in (("one restart interval per MCU row (68 lanes per frame)", row), ("restart intervals of 8 MCUs, the encoder's default (1020 lanes per frame)", own8)):
        js = (js8 * ((n + 7) // 8))[:n]
        blob = np.frombuffer(b"".join(js), np.uint8)
        offs = (C.c_size_t * (n + 1))(*np.concatenate([[0], np.cumsum([len(j) for j in js])]).tolist())

        def call(kind):
            ctx.mjpeg_set_decoder(kind)
            t0 = time.perf_counter()
            ctx._check(lib.lvm_mjpeg_decode_device(ctx.h, blob.ctypes.data, offs, n, w, h, out.data_ptr(), w * 3, w * 3 * h))
            return 1e3 * (time.perf_counter() - t0)
        for _ in range(3):
            for kind, _name in KINDS:
                call(kind)
        ms = {kind: [] for kind, _ in KINDS}
        for _ in range(reps):
            for kind, _name in KINDS:
                ms[kind].append(call(kind))
        print(label + ":")
        for kind, name in KINDS:
            v = np.sort(ms[kind])
            print("  lvm_mjpeg_decode_device, %-9s: median %.2f ms per call (min %.2f, max %.2f) = %.0f frames/s" % (name, np.median(v), v[0], v[-1], 1e3 * n / np.median(v)))
        ctx.profile_only(None)                   # (clears the totals)
        ctx.profile(True)
        for _ in range(5):
            for kind, _name in KINDS:
                call(kind)
        prof = ctx.profile_collect()
        ctx.profile(False)
        for name, (t, cnt) in sorted(prof.items()):
            if name.startswith("mjd_") or name.startswith("mjp_"):
                print("  %-20s %9.1f us per launch of %d frames (%d launches)" % (name, 1e3 * t / max(cnt, 1), n, cnt))
        us = {k: 1e3 * prof[k][0] / max(prof[k][1], 1) for k in ("mjd_pixels", "mjd_chroma_islow", "mjd_pixels_libjpeg")}
        pair = us["mjd_chroma_islow"] + us["mjd_pixels_libjpeg"]
        print("  pixel stage: mjd_pixels %.1f us, mjd_chroma_islow + mjd_pixels_libjpeg %.1f us (%.2f x); %.1f / %.1f us per frame" % (
            us["mjd_pixels"], pair, pair / us["mjd_pixels"], us["mjd_pixels"] / n, pair / n))
    ctx.close()


if __name__ == "__main__":
    main()
