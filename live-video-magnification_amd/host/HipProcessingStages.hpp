// HipProcessingStages.hpp -- the reference's three per-frame stages as ONE device-side stage.
//
// The reference builds its chain in buildProcessors() (src/processing/ChainBuilder.cpp:9-17):
//
//     procs.push_back(std::make_unique<PreprocessProcessor>());
//     procs.push_back(std::make_unique<GrayscaleProcessor>());
//     procs.push_back(std::make_unique<MagnificationProcessor>());
//
// Replacing the three lines by
//
//     procs.push_back(std::make_unique<HipProcessingStages>());
//
// keeps runChainOnce / ProcessingChain / Exporter unchanged and moves crop + INTER_AREA decimation + gray +
// magnification onto the GPU: only the ROI rows are uploaded and only the (decimated) result comes back.
// Contracts mirrored:
//   * PreprocessProcessor.cpp:10-51: identity when no ROI and divisor 1; output Frame carries the new
//     width/height (:46-49);
//   * GrayscaleProcessor.cpp:7-16: identity unless cfg.grayscale and a 3-channel frame; format Gray8;
//   * MagnificationProcessor.cpp:17-67: passthrough hands the magnifier's INPUT on (here: the preprocessed
//     frame); state reset when PreprocessParams change (MagnifyCore.hpp:55-56);
//   * errors surface as std::runtime_error for ProcessingChain.cpp:50-62.
#pragma once
#include <memory>

#include <opencv2/core.hpp>

#include "lvm.hpp"
#include "processing/IProcessor.hpp"

namespace livim {

class HipProcessingStages : public IProcessor {
public:
    explicit HipProcessingStages(int device = 0) : mag_(device, 1) {}

    FrameRef process(const FrameRef& in, const ProcessorConfig& cfg) override {
        const cv::Mat& src = in->image;
        if (src.empty()) return in;                                   // every stage returns `in` on an empty image
        lvm_preprocess_params pre{};
        pre.downscale = cfg.preprocess.downscale;
        pre.roi_enabled = cfg.preprocess.roiEnabled ? 1 : 0;
        pre.roiX = cfg.preprocess.roiX; pre.roiY = cfg.preprocess.roiY;
        pre.roiW = cfg.preprocess.roiW; pre.roiH = cfg.preprocess.roiH;
        pre.grayscale = cfg.grayscale ? 1 : 0;
        const MagnificationParams& p = cfg.magnification;
        lvm::MagnificationParams q;
        q.mode = static_cast<lvm::MagnificationMode>(static_cast<int>(p.mode));
        q.amplification = p.amplification; q.coWavelength = p.coWavelength; q.coLow = p.coLow; q.coHigh = p.coHigh;
        q.chromAttenuation = p.chromAttenuation; q.levels = p.levels; q.framerate = p.framerate;
        // a raw camera frame (setRawFormat): CV_8UC2, w x h, for the packed 4:2:2 formats -- what a V4L2 capture with CAP_PROP_CONVERT_RGB = 0
        // delivers -- or CV_8UC1, w x 3h/2, for NV12 / NV21; the chain behind the conversion sees a BGR frame of w x h
        int w = src.cols, h = src.rows, channels = src.channels(), fmt = LVM_PIX_BGR;
        const bool nv = raw_format_ == LVM_PIX_NV12 || raw_format_ == LVM_PIX_NV21;
        if (raw_format_ != LVM_PIX_BGR && !nv && src.type() == kCv8UC2) { fmt = raw_format_; channels = 3; }
        if (nv && src.type() == CV_8UC1 && src.rows % 3 == 0) { fmt = raw_format_; h = src.rows / 3 * 2; channels = 3; }
        if (fmt != source_format_) { mag_.set_source_format(fmt); source_format_ = fmt; }
        int ow = 0, oh = 0, och = 0;
        lvm::Magnifier::chain_geometry(pre, w, h, channels, &ow, &oh, &och);
        const bool stage_identity = fmt == LVM_PIX_BGR && ow == w && oh == h && och == channels;
        // (output in a recycled page-locked buffer: the download is a plain DMA, no runtime-side pinning per frame)
        const std::size_t row = static_cast<std::size_t>(ow) * static_cast<std::size_t>(och);
        std::shared_ptr<std::uint8_t> buf = pool_.acquire(row * static_cast<std::size_t>(oh));
        const int type = och == 1 ? CV_8UC1 : CV_8UC3;
        cv::Mat dst = buf ? cv::Mat(oh, ow, type, buf.get(), row) : cv::Mat(oh, ow, type);
        const bool produced = mag_.chain_process(pre, q, src.data, w, h, channels,
                                                 static_cast<std::ptrdiff_t>(src.step), dst.data,
                                                 static_cast<std::ptrdiff_t>(dst.step));
        if (!produced && stage_identity) return in;                   // all three stages were identities
        auto out = std::make_shared<PinnedFrame>(*in);
        out->keep = std::move(buf);                                   // returns to the pool with the frame
        out->image = std::move(dst);
        out->width = ow; out->height = oh;                            // PreprocessProcessor.cpp:46-49
        out->format = och >= 3 ? PixelFormat::BGR8 : PixelFormat::Gray8;   // GrayscaleProcessor.cpp:14
        return out;
    }

    void reset() override { mag_.reset(); }

    // Phase mode with the Grayscale toggle (PreprocessParams::grayscale) -- an extension beyond the reference, off by default
    // (lvm_set_phase_on_gray; INTEGRATION.md "Phase mode with the Grayscale toggle"): the gray frames behind GrayscaleProcessor are
    // magnified as BGR2GRAY(Riesz(expand(g))) instead of passing through unchanged (MagnifyCore.hpp:212).
    void setPhaseOnGray(bool on) { mag_.set_phase_on_gray(on); }

    // Raw camera frames in front of the chain -- an extension beyond the reference, off by default (lvm_set_source_format; INTEGRATION.md 3b'):
    // fmt = LVM_PIX_YUYV / _UYVY / _YVYU / _NV12 / _NV21, the pixel format the capture was opened with (rawFormatOfFourcc maps V4L2's code).
    // Frames of the matching raw shape (CV_8UC2 of w x h; CV_8UC1 of w x 3h/2 for NV12 / NV21) are then converted on the device with
    // cv::cvtColor(COLOR_YUV2BGR_*)'s arithmetic; BGR / gray frames keep today's path, so a source may switch between the two.  Only for
    // captures whose own conversion is OpenCV's (V4L2 backend), not FFmpeg's swscale.
    void setRawFormat(int fmt) { raw_format_ = (fmt >= LVM_PIX_BGR && fmt <= LVM_PIX_NV21) ? fmt : LVM_PIX_BGR; }
    static int rawFormatOfFourcc(std::uint32_t fourcc) {
        auto cc = [](char a, char b, char c, char d) { return std::uint32_t(std::uint8_t(a)) | std::uint32_t(std::uint8_t(b)) << 8 | std::uint32_t(std::uint8_t(c)) << 16 | std::uint32_t(std::uint8_t(d)) << 24; };
        if (fourcc == cc('Y', 'U', 'Y', 'V') || fourcc == cc('Y', 'U', 'Y', '2')) return LVM_PIX_YUYV;
        if (fourcc == cc('U', 'Y', 'V', 'Y')) return LVM_PIX_UYVY;
        if (fourcc == cc('Y', 'V', 'Y', 'U')) return LVM_PIX_YVYU;
        if (fourcc == cc('N', 'V', '1', '2')) return LVM_PIX_NV12;
        if (fourcc == cc('N', 'V', '2', '1')) return LVM_PIX_NV21;
        return LVM_PIX_BGR;
    }

private:
    static constexpr int kCv8UC2 = 8;     // CV_8UC2 == CV_MAKETYPE(CV_8U, 2), spelled out: the headers this is checked against define CV_8UC1 / CV_8UC3 only
    struct PinnedFrame : Frame { explicit PinnedFrame(const Frame& f) : Frame(f) {} std::shared_ptr<std::uint8_t> keep; };
    lvm::Magnifier mag_;
    lvm::PinnedPool pool_;
    int raw_format_ = LVM_PIX_BGR;        // setRawFormat: what raw-shaped frames hold
    int source_format_ = LVM_PIX_BGR;     // what the context was told last
};

}  // namespace livim
