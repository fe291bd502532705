#!/usr/bin/env python3
"""Export canvases as 4:2:0 surfaces (lvm_set_canvas_format) on one MI355X: 1920 x 1080, Laplace with the parameters of BASELINE configs[1]
(synth.config(1, ...)), lvm_export_frames host -> host in batches of BATCH page-locked frames (lvm_host_alloc), split None and LeftRight.
  (a) frames/s of four contexts in ONE process, windows of CALLS calls alternating:
        BGR    BGR frames in, BGR canvases out -- the parent commit's path, the baseline;
        NV12c  BGR frames in, NV12 canvases out (the download shrinks from 3 to 1.5 bytes per pixel);
        NV12sc NV12 frames in (lvm_set_source_format) and NV12 canvases out (1.5 bytes per pixel each way);
        BGR'   the BGR line again, a context of its own: the difference between the two BGR lines is the run-to-run spread of this run.
      The acceptance: NV12c is not slower than BGR by more than that spread.  The canvases of NV12c are compared with the restatement
      (OpenCV 4's COLOR_BGR2YUV_I420, interleaved) of BGR's on one batch: identical bytes, or the count that differs.
  (b) the conversion launch alone (lvm_canvas_convert_device) on device-resident canvases: microseconds per launch from device events around
      LAUNCHES launches that rotate over ROT canvases (more bytes than the 256 MB of memory-side cache), and the bytes it moves per second
      (3 bytes per pixel read + 1.5 written), for both kernels ("vec8"; "bytes" through a base pointer offset by 2).  tools/ubench_stream
      (run in the same session by the caller) gives the copy ceiling of the box to put beside it.
usage: tools/yuv_canvas.py [--out profiles/r15_yuv_canvas.txt] [--width W --height H --levels L]"""
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
BATCH, WARM, CALLS, REPS = 32, 3, 25, 5
ROT, LAUNCHES = 32, 640
NFRAMES = 8                     # distinct frames of the clip, cycled: the work does not depend on the content
BGR, NV12, I420 = 0, 4, 6


def yuv_of(f):
    """OpenCV 4 color_yuv, BGR -> Y, U, V per pixel (include/lvm_hip.h)"""
    b, g, r = (f[..., k].astype(np.int32) for k in range(3))
    return ((269484 * r + 528482 * g + 102760 * b + (1 << 19) + (16 << 20)) >> 20,
            (-155188 * r - 305135 * g + 460324 * b + (1 << 19) + (128 << 20)) >> 20,
            (460324 * r - 385875 * g - 74448 * b + (1 << 19) + (128 << 20)) >> 20)


def surface(f, fmt):
    """the (3h/2, w) surface of BGR canvas f: NV12 or I420"""
    h, w = f.shape[:2]
    y = yuv_of(f)[0]
    _, u, v = yuv_of(f[0::2, 0::2])
    out = np.empty((h * 3 // 2, w), np.uint8)
    out[:h] = y
    if fmt == NV12:
        c = out[h:].reshape(h // 2, w // 2, 2)
        c[:, :, 0], c[:, :, 1] = u, v
    else:
        c = out[h:].reshape(2, h // 2, w // 2)
        c[0], c[1] = u, v
    return out


def nv12_source(f):
    """an NV12 frame with the content of BGR frame f (Y = G, U = B, V = R of the block's first pixel)"""
    h, w = f.shape[:2]
    raw = np.empty((h * 3 // 2, w), np.uint8)
    raw[:h] = f[:, :, 1]
    uv = raw[h:].reshape(h // 2, w // 2, 2)
    uv[:, :, 0], uv[:, :, 1] = f[0::2, 0::2, 0], f[0::2, 0::2, 2]
    return raw


class Pinned:
    def __init__(self, lib, nbytes):
        self.lib, self.p = lib, C.c_void_p()
        assert lib.lvm_host_alloc(nbytes, C.byref(self.p)) == 0
        self.a = np.ctypeslib.as_array(C.cast(self.p, C.POINTER(C.c_uint8)), shape=(nbytes,))

    def free(self):
        self.lib.lvm_host_free(self.p)


class Path:
    """one context, BATCH page-locked frames in one format and BATCH page-locked canvases in another, through lvm_export_frames"""
    def __init__(self, src_fmt, canvas_fmt, frames, cp, w, h, split):
        self.ctx = lvm.Context(0, 1)
        self.ctx.set_source_format(src_fmt)
        self.ctx.set_canvas_format(canvas_fmt)
        self.lib, self.w, self.h, self.cp, self.split = self.ctx.lib, w, h, cp, split
        self.pre = lvm.to_c_preprocess(lvm.PreprocessParams(), False)
        cw, chh = C.c_int(0), C.c_int(0)
        assert self.lib.lvm_export_geometry(C.byref(self.pre), split, w, h, 3, C.byref(cw), C.byref(chh)) == 0
        self.cw, self.chh = cw.value, chh.value
        self.row = w * (3 if src_fmt == BGR else 1)
        self.cstride = self.cw * (3 if canvas_fmt == BGR else 1)
        self.cbytes = self.ctx.canvas_layout(canvas_fmt, self.cw, self.chh, self.cstride)[0]
        fbytes = frames[0].size
        self.fin, self.out = Pinned(self.lib, fbytes * BATCH), Pinned(self.lib, self.cbytes * BATCH)
        for k in range(BATCH):
            self.fin.a[k * fbytes:(k + 1) * fbytes] = frames[k % len(frames)].reshape(-1)
        self.pin = (C.c_void_p * BATCH)(*[self.fin.p.value + k * fbytes for k in range(BATCH)])
        self.pout = (C.c_void_p * BATCH)(*[self.out.p.value + k * self.cbytes for k in range(BATCH)])
        self.produced = (C.c_int * BATCH)()
        self.down = self.cbytes

    def call(self):
        rc = self.lib.lvm_export_frames(self.ctx.h, C.byref(self.pre), C.byref(self.cp), self.split, BATCH, self.pin, self.w, self.h, 3, self.row, self.pout, self.cstride,
                                        self.produced)
        assert rc == 0, self.lib.lvm_last_error(self.ctx.h)

    def canvas(self, k):
        return self.out.a[k * self.cbytes:(k + 1) * self.cbytes].copy()

    def window(self):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            self.call()                                               # (synchronous: the canvases are in host memory on return)
        return CALLS * BATCH / (time.perf_counter() - t0)

    def variants(self):
        self.ctx.profile_only("canvas_yuv")
        self.ctx.profile(True)
        self.call()
        v = self.ctx.profile_variants().get("canvas_yuv", set())
        self.ctx.profile(False)
        return ",".join(sorted(v)) or "-"

    def close(self):
        self.ctx.close()
        self.fin.free(); self.out.free()


def convert_only(fmt, canvas, offset):
    """(variant, median us per launch, best, GB/s, output of launch 0) of lvm_canvas_convert_device on ROT device-resident canvases"""
    h, w = canvas.shape[:2]
    ctx = lvm.Context(0, 1)
    d_in = torch.zeros((ROT, h * w * 3 + 16), dtype=torch.uint8, device="cuda")
    d_in[:, offset:offset + h * w * 3] = torch.from_numpy(canvas.reshape(-1)).cuda()
    nbytes = w * h * 3 // 2
    d_out = torch.zeros((ROT, nbytes + 16), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()                 # (a stream of the caller's: handle 0 would mean the context's own stream, which torch's events do not see)
    st = stream.cuda_stream
    torch.cuda.synchronize()

    def launch(k):
        ctx.canvas_convert_device(fmt, C.c_void_p(d_in[k % ROT].data_ptr() + offset), w, h, w * 3, w * h * 3, 1, C.c_void_p(d_out[k % ROT].data_ptr() + offset), w, nbytes, st)
    ctx.profile(True)
    launch(0)
    torch.cuda.synchronize()
    variant = ",".join(sorted(ctx.profile_variants()["canvas_yuv"]))
    ctx.profile(False)
    for k in range(ROT):
        launch(k)
    times = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        for k in range(LAUNCHES):
            launch(k)
        e1.record(stream)
        torch.cuda.synchronize()
        times.append(1e3 * e0.elapsed_time(e1) / LAUNCHES)
    got = d_out[0].cpu().numpy()[offset:offset + nbytes].reshape(h * 3 // 2, w)
    ctx.close()
    us = statistics.median(times)
    return variant, us, min(times), (w * h * 3 + nbytes) / us / 1e3, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--levels", type=int, default=6)
    a = ap.parse_args()
    w, h = a.width, a.height
    if not torch.cuda.is_available():
        raise SystemExit("tools/yuv_canvas.py measures on the GPU: no device here")
    ck, pk = lvm.synth.config(1, (w, h, a.levels))
    clip = lvm.synth.Clip(**ck)
    src = [clip.frame(t) for t in range(NFRAMES)]
    cp = lvm.LvmParams(pk["mode"], pk["levels"], pk["amplification"], pk["coWavelength"], pk["coLow"], pk["coHigh"], pk["chromAttenuation"], pk["framerate"], 0)
    raws = [nv12_source(f) for f in src]
    lines = ["Export canvases as 4:2:0 surfaces (lvm_set_canvas_format): %d x %d, Laplace (synth.config(1): %d levels), lvm_export_frames host -> host," % (w, h, pk["levels"]),
             "batches of %d page-locked frames; device: %s; %s" % (BATCH, torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d %H:%M:%S %Z")), ""]
    for split, sname in ((0, "None"), (1, "LeftRight")):
        paths = {"BGR": Path(BGR, BGR, src, cp, w, h, split), "NV12c": Path(BGR, NV12, src, cp, w, h, split), "NV12sc": Path(NV12, NV12, raws, cp, w, h, split),
                 "BGR'": Path(BGR, BGR, src, cp, w, h, split)}
        for p in paths.values():
            for _ in range(WARM):
                p.call()
        # the same frames through the same schedule: NV12c's canvases against the restatement of BGR's (the last warm-up batch of each)
        b, n = paths["BGR"], paths["NV12c"]
        differ = 0
        for k in (0, 1, BATCH - 1):
            differ += int((surface(b.canvas(k).reshape(b.chh, b.cw, 3), NV12).reshape(-1) != n.canvas(k)).sum())
        fps = {k: [] for k in paths}
        for _ in range(REPS):
            for k, p in paths.items():
                fps[k].append(p.window())
        med = {k: statistics.median(v) for k, v in fps.items()}
        lines.append("(a) split %s, canvas %d x %d; windows of %d calls of %d frames, alternating, %d each, profiling off; frames/s:" % (sname, b.cw, b.chh, CALLS, BATCH, REPS))
        for k, p in paths.items():
            lines.append("  %-7s best %6.0f  median %6.0f  (windows: %s)  download %.2f MB per canvas  canvas_yuv: %s" % (
                k, max(fps[k]), med[k], " ".join("%.0f" % v for v in fps[k]), p.down / 1e6, p.variants()))
        spread = abs(med["BGR"] - med["BGR'"]) / max(med["BGR"], med["BGR'"])
        base = max(med["BGR"], med["BGR'"])
        lines.append("  spread between the two BGR lines (medians): %.2f %%;  NV12c / BGR: %.3f, %.3f;  NV12sc / BGR: %.3f, %.3f  (against BGR, against the faster BGR line)" % (
            100 * spread, med["NV12c"] / med["BGR"], med["NV12c"] / base, med["NV12sc"] / med["BGR"], med["NV12sc"] / base))
        lines.append("  acceptance (NV12c not slower than BGR by more than the spread): %s;  bytes of three NV12c canvases that differ from the restatement of BGR's: %d" % (
            "met" if med["NV12c"] >= med["BGR"] * (1 - spread) else "NOT met", differ))
        lines.append("")
        for p in paths.values():
            p.close()
    lines.append("(b) conversion launch alone (lvm_canvas_convert_device) on device-resident canvases, %d launches rotating over %d canvases, device events," % (LAUNCHES, ROT))
    lines.append("    median (best) of %d windows; bytes = 3 bytes per pixel read + 1.5 written:" % REPS)
    # (at 1920 x 1080 a launch moves ~9 MB: microseconds, the cadence of back-to-back launches as much as the kernel; the canvas tiled 2 x 2 shows the rate)
    for tiles in (1, 2):
        canvas = np.ascontiguousarray(np.tile(src[0], (tiles, tiles, 1)))
        for name, fmt in (("NV12", NV12), ("I420", I420)):
            want = surface(canvas, fmt)
            for offset in (0, 2):
                variant, us, best, gbs, got = convert_only(fmt, canvas, offset)
                lines.append("  %4d x %4d %-4s %-5s %8.1f us (%.1f)  %7.1f GB/s  %.2f MB per launch  output == restatement: %s" % (
                    w * tiles, h * tiles, name, variant, us, best, gbs, canvas.size * 1.5 / 1e6, bool(np.array_equal(got, want))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
