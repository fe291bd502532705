#!/usr/bin/env python3
"""Phase mode on gray frames (lvm_set_phase_on_gray) against the BGR path on the expanded frames, on one MI355X: 1920 x 1080, 6 levels,
one stream, 32 frames per lvm_process_device_frames call, device-resident frames.  Both paths run in this process, alternating:
  - frames/s: host clock around CALLS calls that end in a device synchronise, profiling off, best and median of REPS windows each;
  - per-kernel times: HIP events around every launch (lvm_profile_enable) in passes of their own, again alternating (the kernels between
    the two ends are the same code in both paths: where they differ, the passes differ), median microseconds per launch of 32 frames;
  - the bytes of the gray path against BGR2GRAY of the BGR path's on the timed clip (identical, or the count that differs).
usage: tools/riesz_gray.py [--out profiles/r13_riesz_gray.txt] [--width W --height H --levels L --frames T]"""
import argparse
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
WARM, CALLS, REPS, PROF_CALLS, PROF_REPS = 3, 100, 5, 4, 3          # a window: 3200 frames, ~0.2 s
BGR2GRAY = np.array([3735, 19235, 9798], np.int64)               # GrayscaleProcessor.cpp:13 (RGB2Gray<uchar>, 15-bit fixed point)


def bgr2gray(a):
    return ((a.astype(np.int64) * BGR2GRAY).sum(-1) + (1 << 14) >> 15).astype(np.uint8)


class Path:
    def __init__(self, frames, cp, gray):
        self.ch = 1 if gray else 3
        src = frames if gray else np.repeat(frames[..., None], 3, axis=-1)
        self.n, self.h, self.w = frames.shape
        self.fb = self.w * self.h * self.ch
        self.d_in = torch.from_numpy(np.ascontiguousarray(src)).cuda()
        self.d_out = torch.zeros_like(self.d_in)
        self.cp = cp
        self.ctx = lvm.Context(0, 1)
        self.ctx.set_phase_on_gray(gray)
        self.ctx.set_max_frames(self.n - 1)
        assert self.frames(0, 1) == [False]                          # the first frame of a clip seeds the state
        assert all(self.frames(1, self.n - 1))

    def frames(self, t, nf):
        w, h, ch, fb = self.w, self.h, self.ch, self.fb
        return self.ctx.process_device_frames(self.cp, nf, self.d_in[t].data_ptr(), w, h, ch, w * ch, fb, fb, self.d_out[t].data_ptr(), w * ch, fb, fb,
                                              torch.cuda.current_stream().cuda_stream)

    def call(self):
        self.frames(1, self.n - 1)

    def window(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            self.call()
        torch.cuda.synchronize()
        return CALLS * (self.n - 1) / (time.perf_counter() - t0)

    def kernels(self):
        self.ctx.profile_only(None)                                  # (clears the totals of the previous pass)
        self.ctx.profile(True)
        for _ in range(PROF_CALLS):
            self.call()
        prof, var = self.ctx.profile_collect(), self.ctx.profile_variants()
        self.ctx.profile(False)
        return {k: (1e3 * ms / max(n, 1), ",".join(sorted(var.get(k, ())))) for k, (ms, n) in prof.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--frames", type=int, default=32)
    a = ap.parse_args()
    ck, pk = lvm.synth.config(2, (a.width, a.height, a.levels))
    clip = lvm.synth.Clip(**ck)
    distinct = [bgr2gray(clip.frame(t)) for t in range(8)]           # the clip's first frames, repeated: the kernels' work does not depend on the content
    frames = np.stack([distinct[t % 8] for t in range(a.frames + 1)])
    cp = lvm.LvmParams(pk["mode"], pk["levels"], pk["amplification"], pk["coWavelength"], pk["coLow"], pk["coHigh"], pk["chromAttenuation"], pk["framerate"], 0)
    paths = {"gray": Path(frames, cp, True), "bgr": Path(frames, cp, False)}
    for p in paths.values():
        for _ in range(WARM):
            p.call()
    fps = {k: [] for k in paths}
    for _ in range(REPS):                                            # alternating: both see the same machine
        for k, p in paths.items():
            fps[k].append(p.window())
    torch.cuda.synchronize()
    og, ob = paths["gray"].d_out.cpu().numpy()[1:], bgr2gray(paths["bgr"].d_out.cpu().numpy()[1:])
    differ = int((og != ob).sum())
    passes = {k: [] for k in paths}
    for _ in range(PROF_REPS):
        for k, p in paths.items():
            passes[k].append(p.kernels())
    kern = {k: {n: (statistics.median(q[n][0] for q in v), v[0][n][1]) for n in v[0]} for k, v in passes.items()}
    lines = ["Phase mode, gray frames (lvm_set_phase_on_gray) against the BGR path on the expanded frames: %d x %d, %d levels, 1 stream, %d frames per call,"
             % (a.width, a.height, a.levels, a.frames),
             "device-resident frames, both paths in one process, windows of %d calls alternating (%d each), profiling off" % (CALLS, REPS), ""]
    for k in ("gray", "bgr"):
        lines.append("%-4s frames/s: best %.0f  median %.0f  (windows: %s)" % (k, max(fps[k]), statistics.median(fps[k]), " ".join("%.0f" % v for v in fps[k])))
    lines += ["gray / bgr (medians): %.3f" % (statistics.median(fps["gray"]) / statistics.median(fps["bgr"])),
              "bytes of the gray path that differ from BGR2GRAY(BGR path) on the %d produced frames: %d of %d" % (a.frames, differ, og.size), "",
              "per launch of %d frames, HIP events around every launch (median of %d alternating passes of %d calls), microseconds:" % (a.frames, PROF_REPS, PROF_CALLS),
              "%-22s %10s %-12s %10s %-12s" % ("kernel", "gray", "", "bgr", "")]
    names = list(kern["bgr"]) + [n for n in kern["gray"] if n not in kern["bgr"]]
    for n in names:
        g, b = kern["gray"].get(n), kern["bgr"].get(n)
        lines.append("%-22s %10s %-12s %10s %-12s" % (n, "%.1f" % g[0] if g else "-", g[1] if g else "", "%.1f" % b[0] if b else "-", b[1] if b else ""))
    lines.append("%-22s %10.1f %-12s %10.1f" % ("sum", sum(v[0] for v in kern["gray"].values()), "", sum(v[0] for v in kern["bgr"].values())))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    for p in paths.values():
        p.ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
