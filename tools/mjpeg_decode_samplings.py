#!/usr/bin/env python3
"""The samplings of lvm_mjpeg_decode_device side by side on the GPU (lvm_mjpeg_set_samplings, libjpeg kind): libjpeg-turbo's (Pillow's) 4:2:0, 4:2:2,
4:4:4 and one-component streams of the 1080p clip at quality 90, without restart markers (the self-synchronising kernels) and with restart intervals
of one MCU row (a lane per interval), 32 frames per call, in ONE process on ONE context:
  1. the whole call (host clock around the synchronous call): median, min, max of repeated calls;
  2. per-launch times (HIP events around the launches, lvm_profile_*) and the mjp_sync launches per call: 1 guessing pass + the passes that changed
     an exit + 1 that confirmed -- the look-back of the first pass (MJP_LOOKBACK) was tuned on 4:2:0, this is where the other samplings are recorded.
With --parent LIB (a liblvm_hip.so built from the parent commit) it then alternates that library and this one, each on a fresh context of its own and taking turns to go
first: every sampling under the libjpeg kind and 4:2:0 under the replicating kind, each without restart markers and with one interval per MCU row, 4:2:0
also with the encoder's default intervals of 8 MCUs.  Per case: both sides' call times, whether this library's median lies inside the parent's own
min .. max, whether the decoded frames are byte-identical, and both sides' per-launch times (to locate a difference, not to judge one).
Prints to stdout."""
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

SAMPLINGS = (("4:2:0", lvm.MJPEG_SAMPLING_420, 2), ("4:2:2", lvm.MJPEG_SAMPLING_422, 1), ("4:4:4", lvm.MJPEG_SAMPLING_444, 0), ("gray", lvm.MJPEG_SAMPLING_GRAY, None))


def pil_encode(f, q, subsampling, **kw):
    from PIL import Image
    buf = io.BytesIO()
    if subsampling is None:
        Image.fromarray(np.ascontiguousarray(f[..., 1])).save(buf, "JPEG", quality=q, **kw)
    else:
        Image.fromarray(f[..., ::-1]).save(buf, "JPEG", quality=q, subsampling=subsampling, **kw)
    return buf.getvalue()


def packed(js8, n):
    js = (js8 * ((n + 7) // 8))[:n]
    return np.frombuffer(b"".join(js), np.uint8), (C.c_size_t * (n + 1))(*np.concatenate([[0], np.cumsum([len(j) for j in js])]).tolist())


def main():
    import torch
    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
    lib = lvm.load()
    n, reps = int(os.environ.get("MJD_FRAMES", "32")), int(os.environ.get("MJD_REPS", "15"))
    ck, _ = lvm.synth.config(1)                       # the 1080p clip
    clip = lvm.synth.Clip(seed=1234, **ck)
    w, h = ck["w"], ck["h"]
    frames = np.stack([clip.frame(t) for t in range(8)])
    ctx = lvm.Context(0, 1)
    ctx.mjpeg_set_decoder(lvm.MJPEG_DECODER_LIBJPEG)
    ctx.mjpeg_set_samplings(lvm.MJPEG_SAMPLING_ALL)
    out = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    print("%d frames of %d x %d, quality 90, libjpeg-turbo's streams, libjpeg kind, per call; %d timed calls per figure after 3 warm-up calls" % (n, w, h, reps))

    def timed(cx, lb, blob, offs):
        t0 = time.perf_counter()
        cx._check(lb.lvm_mjpeg_decode_device(cx.h, blob.ctypes.data, offs, n, w, h, out.data_ptr(), w * 3, w * 3 * h))
        return 1e3 * (time.perf_counter() - t0)

    for label, kw in (("no restart markers (self-synchronising lanes of 1024 bits)", {}), ("one restart interval per MCU row (a lane per interval)", dict(restart_marker_rows=1))):
        print(label + ":")
        for name, _mask, sub in SAMPLINGS:
            js8 = [pil_encode(frames[k], 90, sub, **kw) for k in range(8)]
            blob, offs = packed(js8, n)
            for _ in range(3):
                timed(ctx, lib, blob, offs)
            v = np.sort([timed(ctx, lib, blob, offs) for _ in range(reps)])
            print("  %-5s %7.0f KB per frame: median %.2f ms per call (min %.2f, max %.2f) = %.0f frames/s" % (
                name, np.mean([len(j) for j in js8]) / 1e3, np.median(v), v[0], v[-1], 1e3 * n / np.median(v)))
            ctx.profile_only(None)                   # (clears the totals)
            ctx.profile(True)
            for _ in range(5):
                timed(ctx, lib, blob, offs)
            prof = ctx.profile_collect()
            ctx.profile(False)
            for kn, (t, cnt) in sorted(prof.items()):
                if (kn.startswith("mjd_") or kn.startswith("mjp_")) and cnt:
                    print("      %-20s %9.1f us per launch (%.1f launches per call)" % (kn, 1e3 * t / cnt, cnt / 5))
            if "mjp_sync" in prof and prof["mjp_sync"][1]:
                print("      mjp_sync passes that changed an exit: %.1f per call" % (prof["mjp_sync"][1] / 5 - 2))

    ctx.close()                                      # (the comparison below runs on fresh contexts: no buffer of the runs above is kept)
    if parent:
        old = lvm.bind(C.CDLL(parent))
        enc_ctx = lvm.Context(0, 1)
        src = torch.from_numpy(frames).cuda()
        own8 = enc_ctx.mjpeg_encode_device(C.c_void_p(src.data_ptr()), w, h, 8, quality=90)       # restart intervals of 8 MCUs, the encoder's default
        enc_ctx.close()
        cases = []
        for kind_name, kind in (("libjpeg kind", lvm.MJPEG_DECODER_LIBJPEG), ("replicating kind", lvm.MJPEG_DECODER_REPLICATE)):
            for name, mask, sub in SAMPLINGS if kind == lvm.MJPEG_DECODER_LIBJPEG else SAMPLINGS[:1]:
                cases.append((kind, mask, "%s, %s, no restart markers" % (name, kind_name), [pil_encode(frames[k], 90, sub) for k in range(8)]))
                cases.append((kind, mask, "%s, %s, one restart interval per MCU row" % (name, kind_name), [pil_encode(frames[k], 90, sub, restart_marker_rows=1) for k in range(8)]))
                if sub == 2:
                    cases.append((kind, mask, "%s, %s, restart intervals of 8 MCUs (this encoder's stream)" % (name, kind_name), own8))
        print("the parent commit's library against this one, alternating call by call (%d timed calls each after 3 warm-up calls), fresh contexts per case:" % (2 * reps))
        for kind, mask, label, js8 in cases:
            sides = (("parent", lvm.Context(0, 1, old), old), ("this", lvm.Context(0, 1), lib))
            for _n, cx, _l in sides:
                cx.mjpeg_set_decoder(kind)
                cx.mjpeg_set_samplings(mask)
            blob, offs = packed(js8, n)
            ms = {name: [] for name, _c, _l in sides}
            for it in range(3 + 2 * reps):
                for name, cx, lb in sides[::1 - 2 * (it & 1)]:          # (who goes first alternates as well)
                    t = timed(cx, lb, blob, offs)
                    if it >= 3:
                        ms[name].append(t)
            print("  " + label + ":")
            for name, _c, _l in sides:
                v = np.sort(ms[name])
                print("    %-6s median %.3f ms per call (min %.3f, max %.3f)" % (name, np.median(v), v[0], v[-1]))
            po, med = np.sort(ms["parent"]), float(np.median(ms["this"]))
            print("    this library's median lies %s the parent's min .. max (%+.1f %% against the parent's median)" % (
                "INSIDE" if po[0] <= med <= po[-1] else "OUTSIDE", 100 * (med / np.median(po) - 1)))
            decoded = []
            for name, cx, lb in sides:
                out.fill_(0xEE)
                timed(cx, lb, blob, offs)
                decoded.append(out.clone())
            print("    decoded frames: %s" % ("byte-identical on both sides" if torch.equal(decoded[0], decoded[1]) else "DIFFERENT"))
            del decoded
            prof = {}
            for name, cx, lb in sides:
                cx.profile_only(None)
                cx.profile(True)
                for _ in range(5):
                    timed(cx, lb, blob, offs)
                prof[name] = cx.profile_collect()
                cx.profile(False)
            for kn in sorted(prof["this"]):
                (t, cnt), (to, co) = prof["this"][kn], prof["parent"].get(kn, (0.0, 0))
                if (kn.startswith("mjd_") or kn.startswith("mjp_")) and cnt and co:
                    print("      %-20s parent %9.1f us per launch (%.1f launches per call), this %9.1f us (%.1f)" % (kn, 1e3 * to / co, co / 5, 1e3 * t / cnt, cnt / 5))
            for _n, cx, _l in sides:
                cx.close()


if __name__ == "__main__":
    main()
