"""live-video-magnification_amd: MI355X-native Eulerian video magnification core.

The product is liblvm_hip.so (csrc/, C ABI in include/lvm_hip.h); this package is the
Python-side mirror of the reference's operator interface plus bench/test input generators.
Import with importlib (the directory name contains a hyphen):

    lvm = importlib.import_module("live-video-magnification_amd")
"""
from .binding import (CV_ALL, CV_FILTER_DFT, CV_FILTER_UNFUSED, CV_MUL_F32, MJPEG_DECODER_LIBJPEG, MJPEG_DECODER_REPLICATE, MJPEG_SAMPLING_420, MJPEG_SAMPLING_422, MJPEG_SAMPLING_444, MJPEG_SAMPLING_ALL, MJPEG_SAMPLING_GRAY, PIX_BGR, PIX_I420, PIX_NV12, PIX_NV21, PIX_UYVY, PIX_YV12, PIX_YUYV, PIX_YVYU, Context, LvmError, LvmOverlayLabel, LvmParams, LvmPreprocessParams, MagnificationMode, MagnificationParams,  # noqa: F401
                      MagnificationProcessor, PreprocessParams, ProcessingChain, ProcessorConfig, bind, load, to_c_params,
                      to_c_preprocess)
from . import sharding, synth, tiling  # noqa: F401
