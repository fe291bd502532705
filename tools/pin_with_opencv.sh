#!/bin/bash
# Pins the oracle at the OpenCV boundary.  Run ONCE on any box that has an OpenCV 4 development install, a C++20 g++ and the
# reference checkout (REF=/path/to/Live-Video-Magnification, default /root/reference):
#     bash tools/pin_with_opencv.sh
#   1. builds oracle/_ref/libref_magnify.so = the reference's own MagnificationProcessor.cpp + magnification/*.cpp compiled WHERE THEY LIE
#      + oracle/ref_driver.cpp, linked with this box's OpenCV (oracle/Makefile target ref_full);
#   2. recovers the build's forward Lab table and renders BASELINE configs 0-3 with the real reference (tools/pin_generate.py)
#      -> tests/golden/frames_cfg{0,1,2,3}.npz (a few MB: commit them);
#   2b. where the box has the cv2 module: cv2.cvtColor(COLOR_YUV2BGR_*) of one fixed raw frame per format -> tests/golden/yuv_cvtcolor.npz
#      (the raw source formats of lvm_set_source_format, tests/test_yuv_source.py);
#   2c. likewise cv2.cvtColor(COLOR_BGR2YUV_I420 / _YV12) of one fixed BGR frame -> tests/golden/bgr2yuv_420.npz (the canvas formats of
#      lvm_set_canvas_format, tests/test_yuv_canvas.py);
#   3. runs the pin tests: oracle AND library (emulation build; the gfx950 library where a GPU exists) against those files.
# From then on `pytest -m refpin` is a parity gate that needs no OpenCV.
set -e
cd "$(dirname "$0")/.."
REF=${REF:-/root/reference}
make -C oracle REF="$REF" liblvm_oracle.so ref_full
test -f oracle/_ref/libref_magnify.so || { echo "no OpenCV 4 found (pkg-config opencv4 / /usr/include/opencv4): nothing pinned"; exit 2; }
python3 tools/pin_generate.py
# 2b. cv2.cvtColor(COLOR_YUV2BGR_*) of one fixed raw frame per format (tests/test_yuv_source.py: golden_raw) -> tests/golden/yuv_cvtcolor.npz
python3 - <<'PY' || echo "no cv2 module: the raw source formats stay unpinned"
import sys
import cv2
import numpy as np
sys.path.insert(0, "tests")
from test_yuv_source import FORMATS, NAMES, golden_raw
CODES = {"YUYV": cv2.COLOR_YUV2BGR_YUYV, "UYVY": cv2.COLOR_YUV2BGR_UYVY, "YVYU": cv2.COLOR_YUV2BGR_YVYU, "NV12": cv2.COLOR_YUV2BGR_NV12, "NV21": cv2.COLOR_YUV2BGR_NV21}
out = {}
for fmt in FORMATS:
    raw = golden_raw(fmt)
    src = raw.reshape(raw.shape[0], raw.shape[1] // 2, 2) if NAMES[fmt] in ("YUYV", "UYVY", "YVYU") else raw
    out["raw_" + NAMES[fmt]], out["bgr_" + NAMES[fmt]] = raw, cv2.cvtColor(src, CODES[NAMES[fmt]])
np.savez("tests/golden/yuv_cvtcolor.npz", **out)
PY
# 2c. cv2.cvtColor(COLOR_BGR2YUV_I420 / _YV12) of one fixed BGR frame (tests/test_yuv_canvas.py: golden_bgr) -> tests/golden/bgr2yuv_420.npz
python3 - <<'PY' || echo "no cv2 module: the canvas formats stay unpinned"
import sys
import cv2
import numpy as np
sys.path.insert(0, "tests")
from test_yuv_canvas import golden_bgr
f = golden_bgr()
np.savez("tests/golden/bgr2yuv_420.npz", bgr=f, i420=cv2.cvtColor(f, cv2.COLOR_BGR2YUV_I420), yv12=cv2.cvtColor(f, cv2.COLOR_BGR2YUV_YV12))
PY
python3 -m pytest tests/test_refpin.py tests/test_yuv_source.py tests/test_yuv_canvas.py -m refpin -q -s
