#!/usr/bin/env python3
"""Chain input in raw camera formats (lvm_set_source_format) on one MI355X: 1920 x 1080, one stream, Laplace with the parameters of
BASELINE configs[1] (cfg 2 of 5: synth.config(1, ...)), page-locked frames (lvm_host_alloc).
  (a) lvm_chain_process frames/s on BGR frames -- the code of the parent commit, the baseline;
  (b) the same on YUYV and on NV12 frames of the same clip (the upload shrinks from 3 to 2 and 1.5 bytes per pixel);
      all three in this process, windows alternating, host clock around CALLS synchronous calls, profiling off; then, in passes of their
      own, HIP events around every launch (lvm_profile_enable): kernel microseconds per frame, and what is left of a frame's time -- the
      copies over PCIe, their hand-offs and the host side;
  (c) the conversion-only launch (lvm_preprocess_device, crop-only, colour out) on device-resident frames: microseconds per launch from
      device events around LAUNCHES launches that rotate over ROT frame pairs (more bytes than the 256 MB of memory-side cache), the bytes
      it moves per second (raw bytes read + 3 bytes per pixel written), for both kernels ("yuv4"; "yuv" through a base pointer offset by 2).
      tools/ubench_stream (run in the same session by the caller) gives the copy ceiling of the box to put beside it.
The outputs of (b) are compared with (a)'s on the converted frames: identical bytes, or the count that differs.
usage: tools/yuv_source.py [--out profiles/r13_yuv_source.txt] [--width W --height H --levels L]"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

lvm = importlib.import_module("live-video-magnification_amd")
WARM, CALLS, REPS, PROF_CALLS, PROF_REPS = 20, 400, 5, 50, 3
ROT, LAUNCHES = 32, 640
NFRAMES = 8                     # distinct frames of the clip, cycled: the work does not depend on the content


def yuv2bgr(Y, U, V):
    """OpenCV 4 color_yuv (include/lvm_hip.h)"""
    Y, U, V = (a.astype(np.int32) for a in (Y, U, V))
    y = np.maximum(0, Y - 16) * 1220542 + (1 << 19)
    u, v = U - 128, V - 128
    return np.clip(np.stack([(y + 2116026 * u) >> 20, (y - 852492 * v - 409993 * u) >> 20, (y + 1673527 * v) >> 20], axis=-1), 0, 255).astype(np.uint8)


def raw_of(f, fmt):
    """a raw frame with the content of BGR frame f (Y = G, U = B, V = R of the pair's / block's first pixel) and the BGR frame it converts to"""
    h, w = f.shape[:2]
    if fmt == 1:
        q = np.empty((h, w // 2, 4), np.uint8)
        q[:, :, 0], q[:, :, 2], q[:, :, 1], q[:, :, 3] = f[:, 0::2, 1], f[:, 1::2, 1], f[:, 0::2, 0], f[:, 0::2, 2]
        return q.reshape(h, 2 * w), yuv2bgr(f[:, :, 1], np.repeat(q[:, :, 1], 2, 1), np.repeat(q[:, :, 3], 2, 1))
    raw = np.empty((h * 3 // 2, w), np.uint8)
    raw[:h] = f[:, :, 1]
    uv = raw[h:].reshape(h // 2, w // 2, 2)
    uv[:, :, 0], uv[:, :, 1] = f[0::2, 0::2, 0], f[0::2, 0::2, 2]
    up = lambda p: np.repeat(np.repeat(p, 2, 0), 2, 1)
    return raw, yuv2bgr(raw[:h], up(uv[:, :, 0]), up(uv[:, :, 1]))


class Pinned:
    def __init__(self, lib, arr):
        self.lib, self.p = lib, C.c_void_p()
        assert lib.lvm_host_alloc(arr.size, C.byref(self.p)) == 0
        self.a = np.ctypeslib.as_array(C.cast(self.p, C.POINTER(C.c_uint8)), shape=arr.shape)
        self.a[...] = arr

    def free(self):
        self.lib.lvm_host_free(self.p)


class Path:
    """one context fed the clip in one format through lvm_chain_process, frames and output page-locked"""
    def __init__(self, fmt, frames, cp, w, h):
        self.fmt, self.w, self.h, self.cp = fmt, w, h, cp
        self.ctx = lvm.Context(0, 1)
        self.ctx.set_source_format(fmt)
        self.lib = self.ctx.lib
        self.frames = [Pinned(self.lib, f) for f in frames]
        self.out = Pinned(self.lib, np.zeros((h, w, 3), np.uint8))
        self.row = frames[0].shape[1] * (3 if fmt == 0 else 1)
        self.pre = lvm.to_c_preprocess(lvm.PreprocessParams(), False)
        self.produced = C.c_int(0)
        self.t = 0

    def call(self):
        f = self.frames[self.t % len(self.frames)]
        self.t += 1
        rc = self.lib.lvm_chain_process(self.ctx.h, C.byref(self.pre), C.byref(self.cp), f.p, self.w, self.h, 3, self.row, self.out.p, self.w * 3, C.byref(self.produced))
        assert rc == 0, self.lib.lvm_last_error(self.ctx.h)

    def window(self):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            self.call()                                               # (synchronous: complete on return)
        return CALLS / (time.perf_counter() - t0)

    def kernels(self):
        self.ctx.profile_only(None)
        self.ctx.profile(True)
        for _ in range(PROF_CALLS):
            self.call()
        prof, var = self.ctx.profile_collect(), self.ctx.profile_variants()
        self.ctx.profile(False)
        return {k: (1e3 * ms / PROF_CALLS, ",".join(sorted(var.get(k, ())))) for k, (ms, n) in prof.items()}

    def close(self):
        self.ctx.close()
        for f in self.frames + [self.out]:
            f.free()


def convert_only(fmt, raw, w, h, offset):
    """(variant, us per launch, GB/s) of lvm_preprocess_device, crop-only, on ROT device-resident frame pairs"""
    ctx = lvm.Context(0, 1)
    ctx.set_source_format(fmt)
    rh, rb = raw.shape
    d_in = torch.zeros((ROT, rh * rb + 16), dtype=torch.uint8, device="cuda")
    d_in[:, offset:offset + rh * rb] = torch.from_numpy(raw.reshape(-1)).cuda()
    d_out = torch.zeros((ROT, h * w * 3), dtype=torch.uint8, device="cuda")
    pre = lvm.to_c_preprocess(lvm.PreprocessParams(), False)
    stream = torch.cuda.Stream()                 # (a stream of the caller's: handle 0 would mean the context's own stream, which torch's events do not see)
    st = stream.cuda_stream
    torch.cuda.synchronize()

    def launch(k):
        ctx.preprocess_device(pre, C.c_void_p(d_in[k % ROT].data_ptr() + offset), w, h, 3, rb, rh * rb, C.c_void_p(d_out[k % ROT].data_ptr()), w * 3, w * h * 3, st)
    ctx.profile(True)
    launch(0)
    torch.cuda.synchronize()
    variant = ",".join(sorted(ctx.profile_variants()["preprocess"]))
    ctx.profile(False)
    for k in range(ROT):
        launch(k)
    best = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        for k in range(LAUNCHES):
            launch(k)
        e1.record(stream)
        torch.cuda.synchronize()
        best.append(1e3 * e0.elapsed_time(e1) / LAUNCHES)
    got = d_out[0].cpu().numpy().reshape(h, w, 3)
    ctx.close()
    us = statistics.median(best)
    return variant, us, min(best), (rh * rb + w * h * 3) / us / 1e3, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--levels", type=int, default=6)
    a = ap.parse_args()
    w, h = a.width, a.height
    ck, pk = lvm.synth.config(1, (w, h, a.levels))
    clip = lvm.synth.Clip(**ck)
    src = [clip.frame(t) for t in range(NFRAMES)]
    cp = lvm.LvmParams(pk["mode"], pk["levels"], pk["amplification"], pk["coWavelength"], pk["coLow"], pk["coHigh"], pk["chromAttenuation"], pk["framerate"], 0)
    yuyv, nv12 = [raw_of(f, 1) for f in src], [raw_of(f, 4) for f in src]
    lines = ["Chain input in raw camera formats (lvm_set_source_format): %d x %d, 1 stream, Laplace (synth.config(1): %d levels), page-locked frames" % (w, h, pk["levels"]),
             "device: %s; %s" % (torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none", time.strftime("%Y-%m-%d %H:%M:%S %Z")), ""]
    # (a), (b): the BGR baseline is fed the frames the raw ones convert to, so that the outputs can be compared
    for name, clipset, fmt in (("YUYV", yuyv, 1), ("NV12", nv12, 4)):
        paths = {"BGR": Path(0, [b for _, b in clipset], cp, w, h), name: Path(fmt, [r for r, _ in clipset], cp, w, h)}
        differ = 0
        for t in range(WARM):
            outs = []
            for p in paths.values():
                p.call()
                outs.append(p.out.a.copy())
            differ += int((outs[0] != outs[1]).sum())
        fps = {k: [] for k in paths}
        for _ in range(REPS):
            for k, p in paths.items():
                fps[k].append(p.window())
        passes = {k: [] for k in paths}
        for _ in range(PROF_REPS):
            for k, p in paths.items():
                passes[k].append(p.kernels())
        lines.append("(a) / (b) lvm_chain_process, BGR against %s frames of the same clip, windows of %d calls alternating (%d each), profiling off:" % (name, CALLS, REPS))
        for k in paths:
            lines.append("  %-4s frames/s: best %.0f  median %.0f  (windows: %s)" % (k, max(fps[k]), statistics.median(fps[k]), " ".join("%.0f" % v for v in fps[k])))
        mb, mr = statistics.median(fps["BGR"]), statistics.median(fps[name])
        up_b, up_r = w * h * 3, clipset[0][0].size
        lines.append("  %s / BGR (medians): %.3f; us per frame %.1f -> %.1f; upload %.2f -> %.2f MB per frame; bytes that differ on %d warm-up frames: %d" % (
            name, mr / mb, 1e6 / mb, 1e6 / mr, up_b / 1e6, up_r / 1e6, WARM, differ))
        lines.append("  kernels, HIP events around every launch (median of %d alternating passes of %d frames), microseconds per frame:" % (PROF_REPS, PROF_CALLS))
        kern = {k: {n: (statistics.median(q[n][0] for q in v), v[0][n][1]) for n in v[0]} for k, v in passes.items()}
        for n in list(kern[name]):
            b, r = kern["BGR"].get(n), kern[name][n]
            lines.append("    %-20s %8s %8.1f %s" % (n, "%.1f" % b[0] if b else "-", r[0], r[1]))
        sb, sr = sum(v[0] for v in kern["BGR"].values()), sum(v[0] for v in kern[name].values())
        lines.append("    %-20s %8.1f %8.1f   (BGR, %s)" % ("sum", sb, sr, name))
        lines.append("    %-20s %8.1f %8.1f   (frame time of the windows above minus the kernels: copies over PCIe, hand-offs, host)" % ("rest", 1e6 / mb - sb, 1e6 / mr - sr))
        lines.append("")
        for p in paths.values():
            p.close()
    lines.append("(c) conversion-only launch (lvm_preprocess_device, crop-only) on device-resident frames, %d launches rotating over %d frame pairs, device events," % (LAUNCHES, ROT))
    lines.append("    median (best) of %d windows; bytes = raw bytes read + 3 bytes per pixel written:" % REPS)
    # (at 1920 x 1080 a launch moves ~10 MB: microseconds, the cadence of back-to-back launches as much as the kernel; the frame tiled 2 x 2 shows the rate)
    for tiles in (1, 2):
        for name, fmt in (("YUYV", 1), ("NV12", 4)):
            raw, bgr = raw_of(np.tile(src[0], (tiles, tiles, 1)), fmt)
            for offset in (0, 2):
                variant, us, best, gbs, got = convert_only(fmt, raw, w * tiles, h * tiles, offset)
                lines.append("  %4d x %4d %-4s %-5s %8.1f us (%.1f)  %7.1f GB/s  %.2f MB per launch  output == restatement: %s" % (
                    w * tiles, h * tiles, name, variant, us, best, gbs, (raw.size + w * h * tiles * tiles * 3) / 1e6, bool(np.array_equal(got, bgr))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
