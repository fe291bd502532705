#!/usr/bin/env python3
"""Generates tests/golden/color_long_window.npz: Color-mode output frames of the CPU oracle (oracle.pyoracle.Oracle) at the true
window lengths of high-speed footage, 2048 frames (framerate 600) and 4096 frames (framerate 1200).

The oracle's ideal filter costs O(window^2) per row and frame, so a clip that fills a 4096-frame window takes minutes: the clips run
ONCE, here, and tests/test_color_long_window.py compares the library with the stored frames.  (A CPU test of that file re-runs the
oracle over the head of clip A and compares it with this file, which ties the file to the oracle as it stands.)

Frames: 6 x 6 gray, 1 level (9 window rows: the smallest size the reference accepts).  Frame t, pixel i = y * 6 + x:
    4 + (((t * 36 + i) * 1103515245 + 12345) >> 16) % 248
in plain integers -- no RNG stream whose implementation could drift.

    python tests/golden/make_color_long.py            # both clips (about three minutes on 8 cores)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402

W = H = 6
BASE = {"mode": po.MODE_COLOR, "levels": 1, "amplification": 50.0, "coWavelength": 0.0, "chromAttenuation": 0.0}
# per clip: framerate, frames, first stored frame, segments (first frame, frame count, frames per call, coLow, coHigh)
CLIPS = {
    "a": {"framerate": 600.0, "frames": 2100, "keep_from": 1000,
          "segments": [[0, 2048, 1, 0.83, 1.0], [2048, 32, 32, 20.0, 45.0], [2080, 8, 8, 0.0, 300.0], [2088, 12, 1, 20.0, 45.0]]},
    "b": {"framerate": 1200.0, "frames": 4130, "keep_from": 4000,
          "segments": [[0, 4096, 1, 1.66, 2.0], [4096, 32, 32, 40.0, 90.0], [4128, 2, 1, 0.0, 600.0]]},
}


def frame(t):
    i = np.arange(W * H, dtype=np.int64)
    return (4 + (((t * 36 + i) * 1103515245 + 12345) >> 16) % 248).astype(np.uint8).reshape(H, W)


def run(clip, upto=None):
    """the oracle over frames 0 .. upto-1 of a clip: (produced flags, output frames from keep_from on)"""
    n = clip["frames"] if upto is None else upto
    orc = po.Oracle()
    prod, kept = [], []
    try:
        for t0, cnt, _, lo, hi in clip["segments"]:
            P = po.make_params(framerate=clip["framerate"], coLow=lo, coHigh=hi, **BASE)
            for t in range(t0, min(t0 + cnt, n)):
                f = frame(t)
                out, pr = orc.process(f, P)
                prod.append(bool(pr))
                if t >= clip["keep_from"]:
                    assert pr, "frame %d was not produced" % t
                    assert np.unique(out).size >= 16, "frame %d is degenerate: %d distinct values" % (t, np.unique(out).size)
                    kept.append(np.array(out, copy=True))
    finally:
        orc.close()
    return np.array(prod, np.uint8), np.stack(kept)


def main():
    out = {"params": np.array(json.dumps({"w": W, "h": H, "base": BASE, "clips": CLIPS}, sort_keys=True))}
    for name, clip in CLIPS.items():
        assert sum(s[1] for s in clip["segments"]) == clip["frames"]
        t0 = time.time()
        prod, kept = run(clip)
        assert kept.shape == (clip["frames"] - clip["keep_from"], H, W)
        out[name + "_produced"], out[name + "_frames"] = prod, kept
        print("clip %s: %d frames in %.0f s, %d stored" % (name, clip["frames"], time.time() - t0, kept.shape[0]), flush=True)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "color_long_window.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
