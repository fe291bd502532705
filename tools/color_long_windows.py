#!/usr/bin/env python3
"""Color mode at the window lengths of high-speed footage, on the GPU: 1080p, 6 levels, rolling windows of 2048 frames (framerate 1024) and
4096 frames (framerate 2048), filled from a ring of 8 device frames, in ONE process:
  1. warm-up: milliseconds per frame while the window fills (per-frame calls, a band of one entry), for the default build, for
     LVM_COL_LONG_DFT=0 (the serial kernel, frame by frame: what these windows had before) and, with --parent LIB (a liblvm_hip.so built
     from the parent commit), for the parent -- whose warm-up frames also synchronise, free, allocate and copy a twiddle table each;
  2. the full window: bands of 1, 91 and all n / 2 entries, per-frame calls and 32-frame calls, the default (k_col_dft_long, one launch
     per call) against LVM_COL_LONG_DFT=0, alternating call by call on a context each; median of 7 calls (3 for the serial kernel; its
     32-frame calls are 32 per-frame launches and are run once, or not at all, where one would take more than 20 s);
  3. the scale: the same cells at a full 1024-frame window (framerate 512), the longest window of the kernels that were there before.
The serial kernel's cost per frame grows with n^2 whatever the band (38 ms per warm-up frame on the way to 2048 frames, 131 ms on the full window):
filling a 4096-frame window with it takes some ten minutes per context, so windows above CLW_SERIAL_MAX (default 2048) run the default side alone.
Host clock around call + synchronisation.  Prints to stdout."""
import contextlib
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lvm = importlib.import_module("live-video-magnification_amd")

W, H, LEVELS, NB = 1920, 1080, 6, 32
BANDS = (("1 entry", 1.0, 1.2), ("91 entries", 10.0, 55.0), ("all", 0.0, None))       # Hz; window = 2 framerate, so element x passes for 4 lo <= x <= 4 hi


def entries(n, fps, lo, hi):
    """entries of the packed spectrum the 0/1 mask lets through (csrc/color.hip col_filter)"""
    lo = lo + 0.01 if lo == 0.0 else lo
    fl, fh = 2 * lo * float(np.float32(n)) / fps, 2 * hi * float(np.float32(n)) / fps
    m = lambda x: fl <= x <= fh
    return int(m(0)) + sum(1 for k in range(1, (n - 1) // 2 + 1) if m(2 * k - 1) or m(2 * k)) + int(n % 2 == 0 and m(n - 1))


def params(fps, lo, hi):
    return lvm.LvmParams(2, LEVELS, 50.0, 0.0, lo, hi if hi is not None else fps / 2, 0.0, float(fps), 0)


class Side:
    """one context of one library under one setting of the switch, with its window"""
    def __init__(self, name, lib, env, torch, src, dst):
        self.name, self.torch, self.src, self.dst = name, torch, src, dst
        self.env = env
        with self.switch():
            self.ctx = lvm.Context(0, 1, lib)
            self.ctx.set_max_frames(NB)

    @contextlib.contextmanager
    def switch(self):
        """the library reads its switches when it builds the mode's state (the first frame, or the first one after a structural change): every
        call of this side runs with the side's setting in the environment"""
        saved = os.environ.get("LVM_COL_LONG_DFT")
        if self.env is not None:
            os.environ["LVM_COL_LONG_DFT"] = self.env
        try:
            yield
        finally:
            os.environ.pop("LVM_COL_LONG_DFT", None)
            if saved is not None:
                os.environ["LVM_COL_LONG_DFT"] = saved

    def call(self, cp, nf):
        fb = W * H * 3
        with self.switch():
            t0 = time.perf_counter()
            self.ctx.process_device_frames(cp, nf, self.src.data_ptr(), W, H, 3, W * 3, fb, fb, self.dst.data_ptr(), W * 3, fb, fb, 0)
            self.torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0)

    def fill(self, cp, n):
        """n per-frame calls, synchronised once at the end: ms per frame"""
        fb = W * H * 3
        self.torch.cuda.synchronize()
        with self.switch():
            t0 = time.perf_counter()
            for t in range(n):
                k = t % 8
                self.ctx.process_device_frames(cp, 1, self.src.data_ptr() + k * fb, W, H, 3, W * 3, fb, fb, self.dst.data_ptr() + k * fb, W * 3, fb, fb, 0)
                if t % 256 == 255 and time.perf_counter() - t0 > 60:          # a sign of life on the slow sides
                    print("    (%s: %d frames in %.0f s)" % (self.name, t + 1, time.perf_counter() - t0), flush=True)
            self.torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / n

    def variants(self):
        return ",".join(sorted(self.ctx.profile_variants().get("col_dft", set()))) or "-"


def cells(sides, fps, n, serial_names):
    for label, lo, hi in BANDS:
        cp = params(fps, lo, hi)
        ne = entries(n, fps, lo, hi if hi is not None else fps / 2)
        for nf in (1, NB):
            ms = {s.name: [] for s in sides}
            reps = {s.name: (3 if s.name in serial_names else 7) for s in sides}
            note = {}
            for s in sides:                                  # one untimed call each: the band's first call; sizes the serial kernel's 32-frame calls
                first = s.call(cp, 1)
                if s.name in serial_names and nf > 1:
                    if first * nf > 20e3:
                        reps[s.name], note[s.name] = 0, "not run: 32 per-frame launches of %.0f ms" % first
                    elif first * nf > 1e3:
                        reps[s.name] = 1
            for it in range(max(reps.values())):
                for s in sides[::1 - 2 * (it & 1)]:          # (who goes first alternates as well)
                    if it < reps[s.name]:
                        ms[s.name].append(s.call(cp, nf))
            line = "  window %4d, %-10s (%4d entries), %2d-frame calls:" % (n, label, ne, nf)
            for s in sides:
                v = np.sort(ms[s.name])
                line += "  %s %s" % (s.name, note.get(s.name) or "median %.3f ms (min %.3f, max %.3f, %d calls) = %.3f ms per frame" % (
                    np.median(v), v[0], v[-1], len(v), np.median(v) / nf))
            if len(sides) > 1 and ms[sides[0].name] and ms[sides[1].name]:
                line += "  => %.1f x" % (np.median(ms[sides[1].name]) / np.median(ms[sides[0].name]))
            print(line, flush=True)


def main():
    import torch
    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
    windows = [int(x) for x in os.environ.get("CLW_WINDOWS", "2048,4096").split(",")]
    serial_max = int(os.environ.get("CLW_SERIAL_MAX", "2048"))
    lib = lvm.load()
    old = lvm.bind(C.CDLL(parent)) if parent else None
    ck, _ = lvm.synth.config(1)                              # the 1080p clip
    clip = lvm.synth.Clip(seed=1234, **ck)
    ring = np.stack([clip.frame(t) for t in range(8)])
    src = torch.from_numpy(np.concatenate([ring] * (NB // 8))).cuda()
    dst = torch.zeros_like(src)
    print("%d x %d, %d levels, Color mode, amplification 50; frames from a ring of 8 on the device; host clock around call + synchronisation" % (W, H, LEVELS))

    print("scale: a full window of 1024 frames (framerate 512), the kernels for windows up to 1024 frames:")
    s0 = Side("default", lib, None, torch, src, dst)
    print("  warm-up, 1024 per-frame calls, band of 1 entry: %.3f ms per frame" % s0.fill(params(512.0, 1.0, 1.2), 1024))
    cells([s0], 512.0, 1024, ())
    s0.ctx.close()

    for n in windows:
        fps = n / 2.0
        cp = params(fps, 1.0, 1.2)
        print("window of %d frames (framerate %.0f):" % (n, fps))
        sides = [Side("long", lib, "1", torch, src, dst)]
        if n <= serial_max:
            sides.append(Side("serial", lib, "0", torch, src, dst))
        if old is not None and n <= serial_max:
            sides.append(Side("parent", old, None, torch, src, dst))
        for s in sides:
            ms = s.fill(cp, n)
            s.ctx.profile(True)
            s.ctx.profile_only("col_dft")
            s.call(cp, 1)                                    # (one profiled frame on the full window: which kernel this side runs)
            last = s.variants()
            s.ctx.profile(False)
            print("  warm-up, %d per-frame calls, band of 1 entry, %-7s %8.3f ms per frame (col_dft variants: %s)" % (n, s.name + ":", ms, last), flush=True)
        if sides[-1].name == "parent":
            sides.pop().ctx.close()
        cells(sides, fps, n, ("serial",))
        for s in sides:
            s.ctx.close()


if __name__ == "__main__":
    main()
