#!/usr/bin/env python3
"""What the build kinds of lvm_set_opencv_build cost on the GPU: Riesz 1920 x 1080, 6 levels, lvm_process_device_frames calls of 32 frames over a
64-frame input ring, ONE context per kind, every kind's timed calls alternating with those of a mask-0 context in the same process:
  1. frames/s of whole calls (host clock around the call and lvm_synchronize), median of repeated calls, beside the mask-0 context's
     figure from the same alternation;
  2. the per-launch HIP-event times (lvm_profile_*) of the launches the kind replaced -- the 9 x 9 split and collapse / output stage, the
     phase kernels, the blur stage -- beside mask 0's times of the same stages from a pass right in front of the kind's (one profiled call
     discarded, two counted), and which kernel ran (lvm_profile_variants).
The kinds are opt-in parity modes: no throughput target.  Prints to stdout; profiles/r11_opencv_build_kinds.txt holds a run of it."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lvm = importlib.import_module("live-video-magnification_amd")

KINDS = ((lvm.CV_FILTER_UNFUSED, "unfused"), (lvm.CV_FILTER_DFT, "dft"), (lvm.CV_MUL_F32, "mul_f32"),
         (lvm.CV_FILTER_DFT | lvm.CV_MUL_F32, "dft|mul_f32"), (lvm.CV_FILTER_DFT | lvm.CV_FILTER_UNFUSED, "dft|unfused"))
STAGES = (("split", ("rz_split_",)), ("phase", ("rz_phase",)), ("blur", ("rz_blur_amp",)), ("collapse + output", ("rz_collapse_", "rz_final")))


def main():
    import torch
    lvm.load()
    T, ring = int(os.environ.get("CVB_FRAMES", "32")), 64
    reps, warm = int(os.environ.get("CVB_REPS", "9")), 3
    ck, pk = lvm.synth.config(2)                       # Riesz, the 1080p clip, 6 levels
    clip = lvm.synth.Clip(seed=1234, **ck)
    w, h = ck["w"], ck["h"]
    fb = w * h * 3
    cp = lvm.LvmParams(pk["mode"], pk["levels"], pk["amplification"], pk["coWavelength"], pk["coLow"], pk["coHigh"], pk["chromAttenuation"],
                       pk["framerate"], 0)
    d_in = torch.from_numpy(np.stack([clip.frame(t) for t in range(ring)])).cuda()
    d_out = torch.zeros((T, h, w, 3), dtype=torch.uint8, device="cuda")
    stream = None                                      # the context's own stream

    def context(kind):
        ctx = lvm.Context(0, 1)
        ctx.set_max_frames(T)
        ctx.set_opencv_build(kind)
        # the first frame initialises the state (a pass-through frame); the warm-up calls below run in the steady state already
        ctx.process_device(cp, d_in[0].data_ptr(), w, h, 3, w * 3, fb, d_out[0].data_ptr(), w * 3, fb, stream)
        return ctx

    pos = {}

    def call(ctx):
        t = pos.get(ctx, 0)
        pos[ctx] = (t + T) % ring
        t0 = time.perf_counter()
        ctx.process_device_frames(cp, T, d_in[t].data_ptr(), w, h, 3, w * 3, fb, fb, d_out.data_ptr(), w * 3, fb, fb, stream)
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def stage_times(ctx):
        ctx.profile(True)
        call(ctx)
        ctx.profile_only(None)                   # (clears the totals: the first profiled call is not counted)
        for _ in range(2):
            call(ctx)
        variants = ctx.profile_variants()
        prof = ctx.profile_collect()
        ctx.profile(False)
        out = {}
        for stage, prefixes in STAGES:
            names = sorted(n for n in prof if n.startswith(prefixes))
            out[stage] = (sum(prof[n][0] for n in names) / 2.0,
                          ", ".join("%s %.0f us%s" % (n, 1e3 * prof[n][0] / max(prof[n][1], 1), (" [" + ",".join(sorted(variants[n])) + "]") if n in variants else "")
                                    for n in names))
        return out

    print("Riesz %d x %d, %d levels, calls of %d frames over a %d-frame ring; %d timed calls per figure after %d warm-up calls, each kind alternating with mask 0" % (
        w, h, pk["levels"], T, ring, reps, warm))
    base = context(0)
    base_stages = None
    for kind, name in KINDS:
        ctx = context(kind)
        for _ in range(warm):
            call(base), call(ctx)
        ms = {base: [], ctx: []}
        for _ in range(reps):
            for c in (base, ctx):
                ms[c].append(call(c))
        m0, mk = float(np.median(ms[base])), float(np.median(ms[ctx]))
        print("kind %-12s (mask %d): median %.2f ms per call = %.0f frames/s   | mask 0 in the same run: %.2f ms = %.0f frames/s   | %.2f x" % (
            name, kind, mk, 1e3 * T / mk, m0, 1e3 * T / m0, mk / m0))
        base_stages = stage_times(base)
        st = stage_times(ctx)
        for stage, _ in STAGES:
            t0, tk = base_stages[stage][0], st[stage][0]
            print("    %-18s %8.2f ms per call (mask 0: %.2f ms, %.2f x)   %s" % (stage, tk, t0, tk / t0, st[stage][1]))
        ctx.close()
    print("mask 0 stages (the pass in front of the last kind):")
    for stage, _ in STAGES:
        print("    %-18s %8.2f ms per call   %s" % (stage, base_stages[stage][0], base_stages[stage][1]))
    base.close()


if __name__ == "__main__":
    main()
