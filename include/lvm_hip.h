/*
 * lvm_hip.h -- C ABI of liblvm_hip.so, the MI355X (gfx950) Eulerian video-magnification core.
 *
 * Drop-in boundary for the reference's magnification stage.  Every entry point cites the
 * reference interface it replaces (paths relative to the reference's src/):
 *
 *   processing/IProcessor.hpp:50-60            IProcessor::process / reset   (the surface)
 *   processing/MagnificationProcessor.cpp:17-67  process(): clamp levels, structural reset,
 *                                              dispatch by mode, passthrough on !produced
 *   processing/MagnificationProcessor.cpp:10-15  reset()
 *   processing/magnification/MagnifyCore.hpp:83,163,209  magnifyMotion/Color/Riesz
 *
 * Plain pointers and sizes only; no torch / OpenCV / Qt types.  A context is
 * thread-compatible (one thread at a time per context, any number of contexts concurrently --
 * the reference runs a live chain and an export chain side by side, export/Exporter.cpp:204).
 * All entry points return 0 on success, a negative lvm_status otherwise;
 * lvm_last_error(ctx) gives the message.  After an error the context accepts lvm_reset()
 * and continues (the reference's recovery path: processing/ProcessingChain.cpp:50-62).
 */
#ifndef LVM_HIP_H
#define LVM_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* processing/IProcessor.hpp:10 -- numeric order of `enum class MagnificationMode` */
enum lvm_mode { LVM_MODE_LAPLACE = 0, LVM_MODE_PHASE = 1, LVM_MODE_COLOR = 2, LVM_MODE_NONE = 3 };

enum lvm_status {
    LVM_OK = 0,
    LVM_ERR_INVALID = -1,   /* bad argument */
    LVM_ERR_HIP = -2,       /* HIP runtime error (message in lvm_last_error) */
    LVM_ERR_NO_DEVICE = -3, /* no gfx950 device / HIP runtime unavailable */
    LVM_ERR_OOM = -4
};

/* processing/IProcessor.hpp:14-23 (MagnificationParams, algorithm units) plus a key that
 * stands for PreprocessParams equality (IProcessor.hpp:26-41): the reference drops temporal
 * state when the ROI/downscale changes even at equal size (MagnifyCore.hpp:55-56).          */
typedef struct lvm_params {
    int32_t  mode;              /* lvm_mode */
    int32_t  levels;            /* clamped to [1, maxLevels(w,h)] like MagnificationProcessor.cpp:34 */
    double   amplification;     /* alpha */
    double   coWavelength;      /* Laplace: lambda_c (UI% * 10); Phase: 100 - UI% */
    double   coLow;             /* Laplace: IIR blend in [0,1]; Phase/Color: Hz */
    double   coHigh;
    double   chromAttenuation;  /* Laplace only: gain on Lab a,b of the motion image */
    double   framerate;         /* Color ideal filter + Riesz Butterworth: the true capture rate, any value (high-speed
                                 * footage: e.g. 1000).  Color's rolling window is getOptimalBufferSize(framerate) frames:
                                 * windows of up to 4096 frames (framerate <= 2048) run the parallel ideal filter and
                                 * share launches in temporal batches (lvm_process_device_frames); longer windows are
                                 * processed frame by frame by a serial kernel (one thread per window row) */
    uint64_t preprocess_key;    /* any value that changes iff PreprocessParams changes */
} lvm_params;

typedef struct lvm_ctx lvm_ctx;

/* Replaces constructing a MagnificationProcessor (processing/ChainBuilder.cpp:15).
 * n_streams >= 1 independent streams share one context: every per-stream buffer (temporal
 * state, pyramids) is laid out [stream][...] and every kernel launch covers all of them.
 * n_streams == 1 is the drop-in case.                                                       */
int  lvm_create(int device, int n_streams, lvm_ctx** out);
void lvm_destroy(lvm_ctx* ctx);

/* IProcessor::reset (MagnificationProcessor.cpp:10-15): next frame behaves as the first. */
int  lvm_reset(lvm_ctx* ctx);

/* IProcessor::process on host memory (MagnificationProcessor.cpp:17-67), n_streams == 1.
 * in : h rows of w*channels uint8 (BGR interleaved or gray), in_stride bytes per row.
 * out: caller-allocated, same geometry; written only when *produced != 0.
 * *produced == 0 <=> the reference returns the INPUT frame (mode None, frame too small,
 * Color warm-up < 2 columns, Riesz first frame / re-init, Riesz on < 3 channels).
 * Synchronous: H2D, kernels and D2H have completed on return; `in` is not retained.        */
int  lvm_process(lvm_ctx* ctx, const lvm_params* p, const uint8_t* in, int w, int h,
                 int channels, ptrdiff_t in_stride, uint8_t* out, ptrdiff_t out_stride,
                 int* produced);

/* Same contract on DEVICE memory for all n_streams streams at once: stream s reads
 * d_in + s*in_stream_stride and writes d_out + s*out_stream_stride (bytes).  Work is enqueued
 * on `hip_stream` (a hipStream_t; NULL = the context's own stream) and NOT synchronised:
 * *produced is decided on the host before any kernel runs.
 * Call order: the calls of one context take effect in the order they are made, on whatever streams
 * they are given -- this call, lvm_process_device_frames, lvm_flush, the preprocess / compose / overlay
 * surfaces and the synchronous host surfaces (lvm_process, the chain, present, export and codec calls)
 * alike.  The temporal state lives in the context, so the library orders it: a call whose stream is
 * not the one of the context's previous call makes its stream wait for that call with an event, on
 * the device; a call on the same stream adds nothing.  The caller orders only its own buffers: d_in
 * is ready on `hip_stream`, and d_out is read behind the stream of the call that completes it
 * (`hip_stream`; at pipeline depth 1 the stream of the next call or of lvm_flush).
 * Legal layouts: any base pointer (no alignment asked: a view into a larger image, such as a
 * cv::Mat ROI, is fine); in_stride and out_stride >= w*channels; stream strides of any size,
 * smaller than a frame included (two streams side by side in one mosaic frame: stride = 2*w*channels,
 * stream stride = w*channels), but with n_streams > 1 out_stream_stride must be > 0 and the output
 * rectangles of the streams must not overlap.  Bytes outside the w*channels x h rectangles are never
 * written.  Dword-aligned pointers and strides with w % 4 == 0 select the vector kernels, everything
 * else the byte kernels; in the bit-exact flavour the bytes do not depend on that choice.
 * One frame spans at most 2 GiB: (h - 1) * stride + w*channels <= INT32_MAX for in_stride and for
 * out_stride (the kernels address inside a frame with 32 bits); streams and frames may lie any
 * distance apart.
 * A row stride that cannot hold its pixels (negative ones included), a frame whose rows span more
 * than that, or a non-positive output stream stride is refused with LVM_ERR_INVALID before any state
 * changes or any kernel runs: the next valid frame continues the clip.                      */
int  lvm_process_device(lvm_ctx* ctx, const lvm_params* p, const uint8_t* d_in, int w, int h,
                        int channels, ptrdiff_t in_stride, ptrdiff_t in_stream_stride,
                        uint8_t* d_out, ptrdiff_t out_stride, ptrdiff_t out_stream_stride,
                        int* produced, void* hip_stream);

/* n_frames CONSECUTIVE frames of every stream in one call -- the export / offline case
 * (export/Exporter.cpp:216-259 feeds its chain frame after frame from a file).  Frame f of stream s
 * is read at d_in + f*in_frame_stride + s*in_stream_stride and written likewise.  Semantically this
 * IS n_frames calls of lvm_process_device in order (produced[f] per frame); when the mode has a
 * temporally batched schedule (Laplace: stateless kernels take the frames as a batch dimension, the
 * IIR kernels walk over them in order with their state in registers) the frames share launches.
 * Byte for byte: for the same frames in the same memory layout every schedule (this call in any
 * lengths, per-frame calls, lvm_process, pipeline depth 1, any stream) writes the same bytes.
 * Layouts as for lvm_process_device, frame strides of any size; the frames share launches only when
 * they are laid out [frame][stream] (frame stride == n_streams * stream stride, in and out), every
 * other order (such as [stream][frame]) is processed frame by frame.  A refused layout fails the call
 * at the first frame it reaches; produced[] of the frames before it stand.
 * Color: the frames share launches (up to 32 at a time) once the rolling window is full, for windows
 * of up to 4096 frames (framerate <= 2048); the frames of a longer window are processed one by one.  */
int  lvm_process_device_frames(lvm_ctx* ctx, const lvm_params* p, int n_frames, const uint8_t* d_in,
                               int w, int h, int channels, ptrdiff_t in_stride,
                               ptrdiff_t in_stream_stride, ptrdiff_t in_frame_stride, uint8_t* d_out,
                               ptrdiff_t out_stride, ptrdiff_t out_stream_stride,
                               ptrdiff_t out_frame_stride, int* produced, void* hip_stream);

/* Largest n_frames the caller will pass to lvm_process_device_frames: the per-batch pyramids are then
 * allocated once when a mode's state is created, never inside a steady-state call (an export knows its
 * batch size up front, export/Exporter.cpp:216-259).  Without the hint the buffers grow on demand.   */
int  lvm_set_max_frames(lvm_ctx* ctx, int n_frames);

/* Page-locked host memory for frame buffers (what the reference's core/FramePool.cpp:29-36 would allocate
 * its pooled cv::Mat storage from).  lvm_process takes NO staging copy for such frames: the first kernel reads
 * the input and the last kernel writes the output frame directly over PCIe (the input alias only where exactly
 * one kernel reads the u8 frame: Laplace / Riesz on BGR frames); lvm_export_frames / lvm_chain_process copy them
 * by DMA at link speed.  Pageable frames work everywhere (staged copies; the HIP runtime pins them on the fly). */
int  lvm_host_alloc(size_t bytes, void** out);
void lvm_host_free(void* p);

/* ---- the two uint8 stages in front of the magnifier -------------------------
 * processing/IProcessor.hpp:26-41 PreprocessParams + ProcessorConfig::grayscale (IProcessor.hpp:45).  */
typedef struct lvm_preprocess_params {
    int32_t downscale;      /* 1 / 2 / 4 / 8, clamped to [1, 8] like PreprocessProcessor.cpp:14 */
    int32_t roi_enabled;
    float   roiX, roiY, roiW, roiH;   /* fractions of the full frame */
    int32_t grayscale;      /* ProcessorConfig::grayscale: BGR -> Gray8 after the decimation */
} lvm_preprocess_params;

/* Geometry of PreprocessProcessor::process + GrayscaleProcessor::process for a w x h x channels frame:
 * the clamped ROI rectangle (PreprocessProcessor.cpp:19-31) and the size / channel count of the frame
 * handed to the magnifier (:36-39, GrayscaleProcessor.cpp:8-15).                                      */
int  lvm_preprocess_geometry(const lvm_preprocess_params* pp, int w, int h, int channels, int* roi_x,
                             int* roi_y, int* roi_w, int* roi_h, int* out_w, int* out_h, int* out_channels);
/* PreprocessProcessor::process (processing/PreprocessProcessor.cpp:10-51: crop + cv::resize INTER_AREA)
 * followed by GrayscaleProcessor::process (processing/GrayscaleProcessor.cpp:7-16) on DEVICE memory, all
 * n_streams streams, one kernel: the full frame is read once, the small frame written once.  d_out has
 * the geometry lvm_preprocess_geometry reports.  Enqueued on hip_stream, not synchronised.            */
int  lvm_preprocess_device(lvm_ctx* ctx, const lvm_preprocess_params* pp, const uint8_t* d_in, int w, int h,
                           int channels, ptrdiff_t in_stride, ptrdiff_t in_stream_stride, uint8_t* d_out,
                           ptrdiff_t out_stride, ptrdiff_t out_stream_stride, void* hip_stream);
/* runChainOnce (processing/ChainBuilder.cpp:19-29) for the three stages Preprocess -> Grayscale ->
 * Magnification on host memory, n_streams == 1: only the ROI rows cross PCIe, crop / decimation / gray /
 * magnification run on the device, the (small) result comes back.  `out` must hold out_h rows of
 * out_w * out_channels bytes (lvm_preprocess_geometry).  It is always written: the magnified frame
 * when *produced != 0, otherwise the preprocessed frame (the reference's passthrough hands the
 * magnifier's INPUT on, MagnificationProcessor.cpp:61).  The structural key of the magnifier follows
 * the PreprocessParams (MagnifyCore.hpp:55-56), p->preprocess_key is ignored here.                  */
int  lvm_chain_process(lvm_ctx* ctx, const lvm_preprocess_params* pp, const lvm_params* p, const uint8_t* in,
                       int w, int h, int channels, ptrdiff_t in_stride, uint8_t* out, ptrdiff_t out_stride,
                       int* produced);

/* The same for all n_streams streams of a context at once (one processing thread feeding N
 * cameras): in[s] / out[s] are the host frames of stream s, all with the same geometry and parameters; one
 * preprocess launch and one launch per magnifier stage cover every stream.  *produced applies to all streams
 * (they share mode, geometry and history length).                                                     */
int  lvm_chain_process_batch(lvm_ctx* ctx, const lvm_preprocess_params* pp, const lvm_params* p,
                             const uint8_t* const* in, int w, int h, int channels, ptrdiff_t in_stride,
                             uint8_t* const* out, ptrdiff_t out_stride, int* produced);

/* The same plus runChainOnce's `original` (processing/ChainBuilder.cpp:19-29: the tap after chain[0] = PreprocessProcessor,
 * BEFORE GrayscaleProcessor; what the display shows in its left pane, core/LatestFrameMailbox.hpp:13-16): pre_out[s] (may
 * be NULL, entries may be NULL) receives the cropped / decimated frame of stream s -- out_w x out_h like out[s], but with
 * the SOURCE's channel count: with grayscale on a BGR source the tap is the colour frame (3 bytes per pixel,
 * pre_stride >= 3 * out_w) while out[s] is gray.                                                                 */
int  lvm_chain_process_batch_ex(lvm_ctx* ctx, const lvm_preprocess_params* pp, const lvm_params* p,
                                const uint8_t* const* in, int w, int h, int channels, ptrdiff_t in_stride,
                                uint8_t* const* out, ptrdiff_t out_stride, uint8_t* const* pre_out,
                                ptrdiff_t pre_stride, int* produced);

/* ---- display hand-off on the device (the display half) ---------------------------------
 * runChainOnce (processing/ChainBuilder.cpp:19-29) for the LIVE path, n_streams == 1: host frame in, the two frames the display
 * shows left in DEVICE memory.  The reference's ProcessingChain publishes {processed, original} (ProcessingChain.cpp:46-49) and
 * DisplayWidget::uploadFrame (ui/DisplayWidget.cpp:133-152) uploads both from host memory to GL textures on every frame; here
 *   d_proc  (out_w x out_h x out_channels, lvm_preprocess_geometry) receives the magnified frame or, on passthrough
 *           (*produced == 0), the frame the magnifier saw -- i.e. always what the display's main pane shows
 *           (MagnificationProcessor.cpp:61);
 *   d_orig  (out_w x out_h x the SOURCE's channels) receives runChainOnce's `original`: PreprocessProcessor's output, tapped before
 *           GrayscaleProcessor (ChainBuilder.cpp:25);
 * either may be NULL.  Both are caller-owned device pointers -- e.g. the mapped pointers of two GL pixel-unpack buffers registered
 * with hipGraphicsGLRegisterBuffer (host/HipDisplayPresenter.hpp does that), from which glTexSubImage2D then copies device to
 * device: only the ROI rows of the input cross PCIe, nothing comes back.  Synchronous (complete on return).            */
int  lvm_chain_present(lvm_ctx* ctx, const lvm_preprocess_params* pp, const lvm_params* p, const uint8_t* in, int w, int h,
                       int channels, ptrdiff_t in_stride, uint8_t* d_proc, ptrdiff_t proc_stride, uint8_t* d_orig,
                       ptrdiff_t orig_stride, int* produced);

/* ---- export hand-off on the device ---------------------------------------------------
 * export/ExportTypes.hpp:11 -- numeric order of `enum class SplitMode`                                        */
enum lvm_split { LVM_SPLIT_NONE = 0, LVM_SPLIT_LEFT_RIGHT = 1, LVM_SPLIT_TOP_BOTTOM = 2 };
/* Pane and canvas size of Exporter::compose (export/Exporter.cpp:53-88) for an original of ow x oh and a processed
 * frame of pw x ph: panes are cropped to the common EVEN size (:63-64; split None: the processed frame's own even
 * size, :56).  Returns LVM_OK; all four outputs are 0 when the reference returns an empty Mat (:57, :65).     */
int  lvm_compose_geometry(int split, int ow, int oh, int pw, int ph, int* pane_w, int* pane_h, int* canvas_w,
                          int* canvas_h);
/* Exporter::compose on DEVICE memory for all n_streams streams: toBgr (gray -> b = g = r, Exporter.cpp:22-34), crop,
 * and the side-by-side / stacked / single-pane BGR canvas (3 bytes per pixel, canvas_stride >= 3 * canvas_w).  d_orig
 * may be NULL (the reference falls back to the processed frame, :62).  Enqueued on hip_stream, not synchronised.  The
 * text overlay (:36-50) is lvm_overlay_device's job (below). */
int  lvm_compose_device(lvm_ctx* ctx, int split, const uint8_t* d_orig, int ow, int oh, int och,
                        ptrdiff_t orig_stride, ptrdiff_t orig_stream_stride, const uint8_t* d_proc, int pw, int ph,
                        int pch, ptrdiff_t proc_stride, ptrdiff_t proc_stream_stride, uint8_t* d_canvas,
                        ptrdiff_t canvas_stride, ptrdiff_t canvas_stream_stride, void* hip_stream);

/* Spatial tiling of ONE Riesz stream over several devices: a CORRECTNESS DEMONSTRATOR, not a throughput path (DESIGN.md section 7:
 * a frame needs a handful of small exchanges, each a latency, against ~230 us of work on one MI355X -- independent streams, one per GPU, are
 * the production answer).  The frame is cut into horizontal stripes; rank r runs a stripe context on its rows extended by a halo (tiling.py:
 * 64 rows for 2 fine levels) with `levels` = F + 1, F = the fine levels it owns entirely:
 *   lvm_tile_riesz_stage1   Lab, pyramid, phase, temporal filters, normalize + amplify of the stripe (MagnifyCore.hpp:218-267, RieszPyramid.cpp
 *                           :114-144) -- everything up to the collapse; copies the stripe's residual octave (octave F of the full pyramid,
 *                           residual_w x residual_h floats) to d_residual_out.  The owned rows of it go to the rank that holds the coarse levels
 *                           (RCCL send / hipMemcpyPeer: the caller's exchange).
 *   lvm_tile_riesz_planes   that rank: the Riesz chain on a FLOAT PLANE -- the gathered octave F as level 0 of a pyramid with the remaining
 *                           levels -- collapsed back into a float plane: res_F of the full pyramid (RieszPyramid.cpp:304-325).  Rows of it go back.
 *   lvm_tile_riesz_stage2   collapse of the fine levels from the received rows of res_F instead of the stripe's own residual, Lab2BGR, u8
 *                           (MagnifyCore.hpp:269-277) for the extended stripe; the owned rows are the result.
 * Rows closer than the halo to an artificial stripe edge are computed from reflected instead of real neighbours and discarded; with the halo
 * of tiling.py the owned rows are BIT-IDENTICAL to the unsplit context's (tests/test_tiling.py).  produced follows the per-frame rules (first
 * frame: 0 -- every rank passes its rows through).  All calls enqueue on hip_stream without synchronising.                          */
int  lvm_tile_riesz_stage1(lvm_ctx* ctx, const lvm_params* p, const uint8_t* d_in, int w, int h, ptrdiff_t in_stride, int* produced,
                           float* d_residual_out, int* residual_w, int* residual_h, void* hip_stream);
int  lvm_tile_riesz_planes(lvm_ctx* ctx, const lvm_params* p, const float* d_plane_in, int w, int h, float* d_plane_out, int* produced,
                           void* hip_stream);
int  lvm_tile_riesz_stage2(lvm_ctx* ctx, const lvm_params* p, const uint8_t* d_in, int w, int h, ptrdiff_t in_stride,
                           const float* d_residual_in, uint8_t* d_out, ptrdiff_t out_stride, void* hip_stream);

/* The export's text overlay (drawLabel, export/Exporter.cpp:36-50: the rectangle behind a caption darkened with
 * cv::addWeighted(roi, 0.35, black, 0.65), then cv::putText(FONT_HERSHEY_SIMPLEX, white, LINE_AA); called from compose, :74-77 / :82-85)
 * as PER-PIXEL TABLES.  Both steps read-modify-write single pixels with the same arithmetic for B, G and R, so what a label does to a
 * canvas pixel is a function of that pixel's byte; the label itself depends only on the canvas size, i.e. it is fixed for an export.
 * The reference-side shim renders each label ONCE with the reference's own calls onto 256 constant canvases
 * (value v = 0..255) and reads the function off them -- exact for whatever the linked OpenCV draws; nothing of cv::putText is restated
 * in this library.  Pixels with equal functions share a class:
 *   x, y, w, h   the rectangle on the canvas (`bg` of drawLabel after its clip, :43-44)
 *   cls[h][w]    class of every pixel;   fn[n_classes][256]   new byte = fn[cls][old byte]
 * lvm_export_set_overlay copies up to 4 labels into device memory (0 labels: overlay off); lvm_export_frames / _mjpeg /
 * lvm_export_mjpeg_frames then apply them to every composed canvas ON THE DEVICE, so an export with `textOverlay` keeps the device and the
 * Motion-JPEG paths.  A label that does not fit the canvas of a later call fails that call (LVM_ERR_INVALID: it was rendered for another
 * canvas size).  lvm_overlay_device: the same on caller-owned device canvases (enqueued, not synchronised).                        */
typedef struct lvm_overlay_label {
    int32_t x, y, w, h;
    int32_t n_classes;
    const uint16_t* cls;
    const uint8_t* fn;
} lvm_overlay_label;
int  lvm_export_set_overlay(lvm_ctx* ctx, int n_labels, const lvm_overlay_label* labels);
int  lvm_overlay_device(lvm_ctx* ctx, uint8_t* d_canvas, int canvas_w, int canvas_h, ptrdiff_t canvas_stride, ptrdiff_t frame_stride,
                        int n_frames, void* hip_stream);

/* The loop body of Exporter::run (export/Exporter.cpp:216-259) for n_frames CONSECUTIVE host frames of a 1-stream context:
 *   runChainOnce (ChainBuilder.cpp:19-29: PreprocessProcessor -> GrayscaleProcessor -> MagnificationProcessor) on every frame in
 *   order, then Exporter::compose(original, processed, split) (Exporter.cpp:53-88) -- `original` = PreprocessProcessor's output
 *   (the tap of ChainBuilder.cpp:25 sits BEFORE GrayscaleProcessor: a colour pane even when the chain grays), `processed` = the
 *   magnifier's output or, on passthrough (produced[i] == 0), the frame it saw (MagnificationProcessor.cpp:61).
 * frames[i] -> canvases[i]: canvas_w x canvas_h x 3 bytes (lvm_export_geometry), row stride canvas_stride.  Only the ROI rows of
 * the inputs and the canvases cross PCIe, in both directions at once: the frames go through in sub-batches of 8 (each ONE temporal
 * batch of the magnifier, lvm_process_device_frames), sub-batch k + 1 uploading and sub-batch k - 1 downloading while sub-batch k is
 * magnified and composed on the device (lvm_compose_device), the labels of lvm_export_set_overlay applied there too.
 * cv::VideoWriter::write (:259) stays on the host: host/HipExportRunner.hpp is the reference-side loop around this call.  Synchronous. */
int  lvm_export_geometry(const lvm_preprocess_params* pp, int split, int w, int h, int channels, int* canvas_w, int* canvas_h);
int  lvm_export_frames(lvm_ctx* ctx, const lvm_preprocess_params* pp, const lvm_params* p, int split, int n_frames,
                       const uint8_t* const* frames, int w, int h, int channels, ptrdiff_t in_stride,
                       uint8_t* const* canvases, ptrdiff_t canvas_stride, int* produced);

/* Motion-JPEG encode on the device (the encode half): what cv::VideoWriter::write(canvas) does for
 * ExportFormat::AviMjpg, the reference's AVI export format and the fallback of every other one (export/Exporter.cpp:107-117, :259).
 * Baseline JPEG (ITU-T T.81), 8 bit, YCbCr 4:2:0 (JFIF), Annex K Huffman tables, restart intervals of 8 MCUs, libjpeg's quality scale
 * (1..100).  Frames: BGR, 1..8192 x 1..16384.
 *   lvm_mjpeg_bound            bytes that always suffice for ONE encoded frame of this size (a bound; typical frames are 5-20 % of it)
 *   lvm_mjpeg_encode_device    n_frames device-resident BGR frames -> out[offsets[i] .. offsets[i + 1]) = frame i, a complete JPEG;
 *                              offsets has n_frames + 1 entries.  LVM_ERR_INVALID when out_capacity is too small.  Synchronous.
 *   lvm_export_frames_mjpeg    lvm_export_frames with the canvases encoded on the device: only the ROI rows go up and only the compressed
 *                              frames come down.  host/HipMjpegWriter.hpp wraps the frames into the AVI container.                       */
/*   lvm_mjpeg_decode_device    the other direction (cv::VideoCapture::read on an AVI / Motion-JPEG file, source/FileSource.cpp:99): n_frames
 *                              JPEG frames in host memory (jpegs[offsets[i] .. offsets[i + 1])) -> BGR frames of w x h in DEVICE memory.
 *                              Baseline 4:2:0 in one scan (4:2:2, 4:4:4 and one-component frames too where lvm_mjpeg_set_samplings allows them;
 *                              all frames of a call share one sampling), any tables; frames with restart intervals decode a lane per interval, frames
 *                              without through self-synchronising lanes of 1024 bits (a call's time is mostly latency: pass many frames); anything else, a size other
 *                              than w x h or a malformed stream is LVM_ERR_INVALID (lvm_last_error says which frame and why).  Synchronous. */
/*   lvm_export_mjpeg_frames    lvm_export_frames_mjpeg with JPEG frames IN as well (an AVI / Motion-JPEG source file): decode, chain, compose and
 *                              encode all on the device, only compressed bytes cross PCIe in either direction (file -> file export).           */
/*   lvm_mjpeg_set_restart_interval   MCUs (16 x 16 pixels, raster order) per restart interval of the frames this context encodes from now on;
 *                              0 = the default, 8 (pass (w + 15) / 16 for one interval per MCU row).  Entropy coding is serial inside an
 *                              interval: short intervals cost < 0.5 % of bytes and make the frames decode in parallel --
 *                              lvm_mjpeg_decode_device gives every interval a lane.                                                              */
/*   lvm_mjpeg_set_decoder      the arithmetic behind the entropy layer of lvm_mjpeg_decode_device and lvm_export_mjpeg_frames, from the next call on
 *                              (the entropy layer itself is exact by the standard and shared):
 *                                LVM_MJPEG_DECODER_REPLICATE (0, the default)  matrix IDCT, 4:2:0 chroma replicated: bit-identical to
 *                                    oracle/mjpeg_oracle.py::decode_frame, what this library always decoded;
 *                                LVM_MJPEG_DECODER_LIBJPEG (1)  libjpeg's / libjpeg-turbo's defaults -- JDCT_ISLOW, do_fancy_upsampling (the 9 : 3 : 3 : 1
 *                                    triangle filter of the chroma planes), no clamp behind the dequantiser: BYTE-identical to what a libjpeg-backed
 *                                    cv::VideoCapture (or Pillow) hands out, for every stream an encoder makes from 8-bit samples; on others (damaged
 *                                    streams, where libjpeg builds differ among themselves) the arithmetic wraps in 32 bits.  FFmpeg's own mjpeg
 *                                    decoder (another IDCT, swscale chroma) is NOT what this kind restates.
 *                              Any other kind: LVM_ERR_INVALID.  Frames other than 4:2:0 (lvm_mjpeg_set_samplings) have libjpeg's arithmetic only:
 *                              under LVM_MJPEG_DECODER_REPLICATE they are refused ("frame 0: 4:2:2 needs LVM_MJPEG_DECODER_LIBJPEG").  The frames of a
 *                              call share frame 0's sampling, so this is decided at frame 0, before the later frames are parsed: it is reported
 *                              even where a later frame is malformed.                                                                            */
enum { LVM_MJPEG_DECODER_REPLICATE = 0, LVM_MJPEG_DECODER_LIBJPEG = 1 };
int  lvm_mjpeg_set_decoder(lvm_ctx* ctx, int kind);
/*   lvm_mjpeg_set_samplings    the samplings lvm_mjpeg_decode_device and lvm_export_mjpeg_frames accept from the next call on, a mask of
 *                                LVM_MJPEG_SAMPLING_420 (Y 2x2, the default mask: every refusal and message stays what it was), LVM_MJPEG_SAMPLING_422
 *                                (Y 2x1: UVC cameras, capture cards, FFmpeg's yuvj422p), LVM_MJPEG_SAMPLING_444 (FFmpeg's yuvj444p) and
 *                                LVM_MJPEG_SAMPLING_GRAY (one component; its sampling factors are ignored, T.81 A.2.2; decoded to b = g = r).
 *                              Cb and Cr are 1x1 in every one.  4:2:2, 4:4:4 and gray frames are byte-identical to libjpeg's (h2v1 fancy upsampling
 *                              for 4:2:2) and need LVM_MJPEG_DECODER_LIBJPEG.  Still refused: 4:4:0, 4:1:1, four components, progressive,
 *                              arithmetic-coded and 12-bit frames.  A mask of 0 or with other bits: LVM_ERR_INVALID, nothing changes.             */
enum { LVM_MJPEG_SAMPLING_420 = 1, LVM_MJPEG_SAMPLING_422 = 2, LVM_MJPEG_SAMPLING_444 = 4, LVM_MJPEG_SAMPLING_GRAY = 8, LVM_MJPEG_SAMPLING_ALL = 15 };
int  lvm_mjpeg_set_samplings(lvm_ctx* ctx, unsigned mask);
size_t lvm_mjpeg_bound(int w, int h);
int  lvm_mjpeg_set_restart_interval(lvm_ctx* ctx, int mcus);
int  lvm_export_mjpeg_frames(lvm_ctx* ctx, const lvm_preprocess_params* pp, const lvm_params* p, int split, int n_frames, const uint8_t* jpegs,
                             const size_t* in_offsets, int w, int h, int quality, uint8_t* out, size_t out_capacity, size_t* offsets, int* produced);
int  lvm_mjpeg_decode_device(lvm_ctx* ctx, const uint8_t* jpegs, const size_t* offsets, int n_frames, int w, int h, uint8_t* d_bgr,
                             ptrdiff_t stride, ptrdiff_t frame_stride);
int  lvm_mjpeg_encode_device(lvm_ctx* ctx, const uint8_t* d_bgr, int w, int h, ptrdiff_t stride, ptrdiff_t frame_stride, int n_frames,
                             int quality, uint8_t* out, size_t out_capacity, size_t* offsets);
int  lvm_export_frames_mjpeg(lvm_ctx* ctx, const lvm_preprocess_params* pp, const lvm_params* p, int split, int n_frames,
                             const uint8_t* const* frames, int w, int h, int channels, ptrdiff_t in_stride, int quality,
                             uint8_t* out, size_t out_capacity, size_t* offsets, int* produced);

/* Which OpenCV build the arithmetic of the RIESZ mode reproduces.  cv::filter2D / cv::sepFilter2D / `Mat * double` do not round alike in
 * every build of OpenCV, and the ill-conditioned acos(q0 / |q|) of RieszPyramid.cpp:93-97 turns their last-bit differences into ~1.2e-4 of
 * the output.  Mask 0 -- the default: every launch, kernel and byte is what it is without this call -- is the AVX2 / AVX-512
 * dispatch of an x86-64 build: fused taps (v_fma) and a float64 scalar product.  The bits, each the oracle's switch of the same name
 * (oracle/lvm_oracle.h, LVMO_VAR_*):
 *   LVM_CV_FILTER_UNFUSED  a build whose filter loops dispatch to SSE2 only (CPU_BASELINE=SSE2 without AVX2 dispatch, or a host without
 *                          FMA3): every tap of filter2D (the 9 x 9 kernels of RieszPyramid.cpp:227-232, :314-319 and the 1 x 5 / 5 x 1
 *                          Riesz pair of :74-76) and of sepFilter2D / GaussianBlur (the 13-tap blurs of :110, :121-126) is a multiply, then an add.
 *   LVM_CV_FILTER_DFT      a build without SSE3 -- every ARM build, macOS on Apple silicon included: filter2D sends kernels of >= 50 elements
 *                          through crossCorr, so the 9 x 9 kernels (:227-232, :314-319) are the float64 sum of the exact products, rounded
 *                          once.  The 5-tap pair and the separable blurs keep the direct path (fused there, unless _UNFUSED is set as well).
 *   LVM_CV_MUL_F32         a build whose `Mat * double` narrows the scalar to float first: the five products of each Butterworth step
 *                          (TemporalFilter.cpp:343-350) are x * (float)s.
 * Takes effect from the next frame of the context, for all of its streams; the temporal state is kept (as the oracle's switch keeps it)
 * and lvm_reset keeps the kind.  Laplace, Color, preprocess, compose and the codec ignore it (they meet the parity bar under every build,
 * DESIGN.md 5); it applies in every flavour (default, lvm_debug_exact_lab, lvm_debug_lab_analytic) and to lvm_tile_riesz_*.  A mask with
 * other bits: LVM_ERR_INVALID, nothing changes.  INTEGRATION.md says which kind goes with which OpenCV build.                        */
enum { LVM_CV_FILTER_UNFUSED = 1,   /* filter2D / sepFilter2D taps as multiply, then add (SSE2-only dispatch) */
       LVM_CV_FILTER_DFT     = 2,   /* filter2D kernels of >= 50 elements through crossCorr: float64 sum of the exact
                                       products, rounded once (builds without SSE3 = every ARM / macOS build) */
       LVM_CV_MUL_F32        = 4,   /* Riesz IIR `Mat * double` with the scalar narrowed to float first */
       LVM_CV_ALL            = 7 };
int  lvm_set_opencv_build(lvm_ctx* ctx, unsigned mask);
int  lvm_get_opencv_build(lvm_ctx* ctx, unsigned* mask);

/* Phase (Riesz) magnification of GRAY frames -- an EXTENSION beyond the reference, off by default.  The reference's magnifyRiesz returns
 * "produced no frame" for every 1-channel frame (MagnifyCore.hpp:212), and so does LVM_MODE_PHASE here while the option is 0: every launch,
 * byte and `produced` flag is what it is without this call.  With the option 1 a Phase context fed the gray frames g_t gives, frame by frame,
 *     produced_t, out_t  ==  produced'_t, BGR2GRAY( Riesz( expand(g_t) ) )
 * where expand(g) is the BGR frame with b = g = r = g, Riesz the 3-channel Phase mode with the same parameters, flavour and build kind, and
 * BGR2GRAY the conversion of GrayscaleProcessor (GrayscaleProcessor.cpp:13: (3735 B + 19235 G + 9798 R + 16384) >> 15 on the u8 frame) --
 * the reference chain with GrayscaleProcessor moved behind the magnifier.  The weights add up to 32768, so BGR2GRAY(expand(g)) == g and
 * the passthrough frames (first frame, re-init on NaN coefficients, frame too small) follow the same rule; cutoff change, construction-time
 * framerate, lvm_reset and the structural reset are unchanged.  L, a, b of a gray pixel are functions of its byte: a 256-entry table,
 * filled on the device by the forward conversion of the context's flavour, replaces the 33^3 table kernel and the (ia, ib) plane.
 * Every surface that processes frames takes part (lvm_process*, lvm_chain_* with grayscale = 1, lvm_chain_present, the export calls);
 * lvm_tile_riesz_* stay BGR-only.  With lvm_debug_keep_float the kept frame is the THREE-channel BGR float frame in front of the quantiser
 * (w*h*3 floats).  A change while the tracked state is Phase on 1-channel frames is a structural change (flush, synchronise, drop the
 * state: the next frame is a first frame); otherwise the value is only stored.  lvm_reset keeps it.  A value other than 0 / 1:
 * LVM_ERR_INVALID, nothing changes.                                                                                                      */
int  lvm_set_phase_on_gray(lvm_ctx* ctx, int on);
int  lvm_get_phase_on_gray(lvm_ctx* ctx, int* on);

/* Chain input in RAW CAMERA FORMATS -- an opt-in extension; with LVM_PIX_BGR (the default) every launch, byte, error message and `produced`
 * flag is what it is without this call.  The reference opens cameras with cv::CAP_V4L2 (source/CameraSource.cpp:36,53), whose backend prefers
 * the raw formats: every cap_.read() ends in cv::cvtColor(COLOR_YUV2BGR_*) on the grab thread.  With format F != LVM_PIX_BGR the frames given
 * to the surfaces below are in F and the result is, frame by frame and byte for byte, what the same call gives on
 * cvtColor(frame, COLOR_YUV2BGR_F) -- the reference chain behind a cv::VideoCapture that converted the frame itself.
 * Per pixel (OpenCV 4 color_yuv: ITU-R BT.601, limited range, 20-bit fixed point; int32, nothing overflows; `>>` arithmetic: negative
 * sums floor; sat_u8 clamps to 0..255):
 *     y = max(0, Y - 16) * 1220542
 *     R = sat_u8((y + (1 << 19) + 1673527 * (V - 128)) >> 20)
 *     G = sat_u8((y + (1 << 19) -  852492 * (V - 128) - 409993 * (U - 128)) >> 20)
 *     B = sat_u8((y + (1 << 19) + 2116026 * (U - 128)) >> 20)
 * Chroma is replicated, never interpolated: pixels 2k and 2k + 1 of a row share (U, V) in the 4:2:2 formats, a 2 x 2 block shares the pair at
 * UV row y >> 1, byte pair x >> 1 in NV12 / NV21 -- by ABSOLUTE frame coordinates: an ROI that starts at an odd x or y keeps the chroma of the
 * pair / block it cuts through.  Order: convert, crop, INTER_AREA, BGR2GRAY -- block sums add converted B, G, R bytes and the gray frame is
 * gray15(B, G, R) of the converted, decimated pixel, not Y.  The stage is never the identity: crop-only at full size is the plain conversion.
 * Arguments with F != LVM_PIX_BGR (anything else: LVM_ERR_INVALID with a message that names the rule, refused before any state changes):
 *   channels   must be 3: it describes the frame the chain sees (also for lvm_preprocess_geometry / lvm_export_geometry, which are unchanged);
 *   w          must be even; h too for NV12 / NV21 (OpenCV's own preconditions);
 *   in_stride  >= 2 * w for the packed formats, >= w for NV12 / NV21;
 *   NV12 / NV21 frames are ONE buffer: the UV plane starts at row h with the same stride (OpenCV's (3h/2) x w single-channel layout, what V4L2
 *   hands out); a stream stride covers the whole buffer.
 * Surfaces that take part: lvm_preprocess_device (device frames, all streams), lvm_chain_process / _batch / _batch_ex (the tap / `original` is
 * the converted colour frame), lvm_chain_present, lvm_export_frames, lvm_export_frames_mjpeg.  Only the ROI's raw bytes cross PCIe: 2 B / pixel
 * (4:2:2) or 1.5 B / pixel (NV12 / NV21) instead of 3.  Surfaces that do NOT: lvm_process* (IProcessor::process: a processor input is BGR / gray,
 * core/Frame.hpp:12), lvm_export_mjpeg_frames and lvm_mjpeg_decode_device (JPEG in), lvm_tile_riesz_*.  An FFmpeg-backed VideoCapture converts
 * with swscale, which is other arithmetic and NOT what this restates (INTEGRATION.md 3b').
 * The setter only stores the value -- it is read by the next call that takes frames, in call order like everything else of the context: the
 * magnifier sees BGR / gray frames of the same geometry either way, so its temporal state, the tracked structural key and preprocess_key are
 * untouched.  lvm_reset keeps the format.  An unknown format: LVM_ERR_INVALID, nothing changes.  lvm_profile_variants reports the kernel that
 * ran under "preprocess": "yuv4" (four pixels per thread, dword-wide frame I/O: crop-only, colour out, dword-aligned pointers and strides, an
 * ROI that starts at an even x, a width that is a multiple of 4) or "yuv" (byte I/O, everything else); both give identical bytes.       */
enum lvm_pixel_format { LVM_PIX_BGR = 0,      /* BGR8 or Gray8 by `channels`: today's behaviour */
                        LVM_PIX_YUYV = 1,     /* Y0 U Y1 V   (V4L2 YUYV / YUY2) */
                        LVM_PIX_UYVY = 2,     /* U Y0 V Y1 */
                        LVM_PIX_YVYU = 3,     /* Y0 V Y1 U */
                        LVM_PIX_NV12 = 4,     /* h rows of Y, then h/2 rows of interleaved U V, same row stride */
                        LVM_PIX_NV21 = 5 };   /* ... of interleaved V U */
int  lvm_set_source_format(lvm_ctx* ctx, int fmt);
int  lvm_get_source_format(lvm_ctx* ctx, int* fmt);

/* Export canvases as 4:2:0 SURFACES -- NV12 / NV21 / I420 / YV12, converted on the device; an opt-in extension, with LVM_PIX_BGR (the default)
 * every launch, byte, error message and `produced` flag is what it is without this call.  The reference's default export format is
 * ExportFormat::Mp4H264 (export/ExportTypes.hpp:23), and every H.264 / HEVC / AV1 encoder behind this library (VCN through VA-API or AMF, an FFmpeg
 * rawvideo pipe) takes 4:2:0 surfaces: 1.5 B / pixel come down instead of 3, or the surface stays on the device.  With canvas format F != LVM_PIX_BGR
 * a participating surface gives cvtColor(canvas, COLOR_BGR2YUV_I420) (OpenCV 4 color_yuv) of the BGR canvas it gives under LVM_PIX_BGR, byte for
 * byte, in the layout of F; the text overlay of lvm_export_set_overlay is applied to the BGR pixels FIRST.  Per pixel (ITU-R BT.601, limited range,
 * 20-bit fixed point, int32: every sum is positive and below 2^31 and every result lies in 0..255, so no saturation or sign rule is exercised):
 *     Y = ( 269484 R + 528482 G + 102760 B + (1 << 19) + ( 16 << 20)) >> 20
 *     U = (-155188 R - 305135 G + 460324 B + (1 << 19) + (128 << 20)) >> 20
 *     V = ( 460324 R - 385875 G -  74448 B + (1 << 19) + (128 << 20)) >> 20
 * Y at every pixel; U and V from the TOP-LEFT pixel (even x, even y, canvas coordinates) of each 2 x 2 block -- OpenCV subsamples, it does not
 * average.  The U and V rows each sum to 1: OpenCV's quirk, kept.  OpenCV 4 has no COLOR_BGR2YUV_NV12: NV12 / NV21 are the I420 samples interleaved.
 * An FFmpeg-backed cv::VideoWriter converts BGR to yuv420p with swscale, which is other arithmetic and NOT what this restates (INTEGRATION.md 3d'').
 * Layouts (canvas_w and canvas_h are even: lvm_compose_geometry crops the panes to even sizes; canvas_stride is the Y row stride):
 *   LVM_PIX_NV12 / LVM_PIX_NV21   canvas_h rows of Y; the interleaved U V (V U) plane starts at row canvas_h with the same stride: canvas_h / 2 rows of
 *                                 canvas_w bytes -- ONE buffer, the convention of the source formats.  canvas_stride >= canvas_w.
 *   LVM_PIX_I420 / LVM_PIX_YV12   canvas_h rows of Y; the first chroma plane (U for I420, V for YV12) starts at byte canvas_stride * canvas_h, the
 *                                 second at canvas_stride * canvas_h * 5 / 4; each has canvas_h / 2 rows of canvas_w / 2 bytes, row stride
 *                                 canvas_stride / 2.  canvas_stride even and >= canvas_w; with canvas_stride == canvas_w this is OpenCV's
 *                                 (3h/2) x w single-channel Mat and FFmpeg's contiguous yuv420p.
 *   The packed 4:2:2 formats (1..3) are refused as canvas formats.
 * lvm_set_canvas_format   only stores the value: the next participating call reads it, in call order.  lvm_reset keeps it; the temporal state, the
 *                         tracked structural key and the overlay tables are left alone.  Any value other than 0, 4, 5, 6, 7: LVM_ERR_INVALID with a
 *                         message that names the allowed values, nothing changes.
 * lvm_canvas_layout       a pure function of the rules above: the bytes of one canvas, the offsets of the chroma planes and their row stride.  BGR:
 *                         bytes = canvas_stride * canvas_h (canvas_stride >= 3 * canvas_w), no chroma planes (0, 0, 0).  NV12 / NV21: plane2_offset = 0.
 *                         Outputs may be NULL.  A refused format, size or stride: LVM_ERR_INVALID.
 * lvm_canvas_convert_device   n_frames device-resident BGR canvases (w x h, row stride bgr_stride >= 3 * w, frame i at d_bgr + i * bgr_frame_stride) ->
 *                         format fmt (one of the four YUV formats, whatever lvm_set_canvas_format says) at d_out + i * out_frame_stride, Y row stride
 *                         out_stride.  Enqueued on hip_stream, not synchronised; it takes its place in the context's call order like
 *                         lvm_overlay_device.  Any base pointers are legal.  w or h odd or < 2, short strides, overlapping output frames
 *                         (out_frame_stride smaller than the layout's bytes when n_frames > 1): LVM_ERR_INVALID before anything runs.  The surface for
 *                         callers that compose on the device (lvm_compose_device, lvm_overlay_device) and encode there.
 * lvm_export_frames       with F != LVM_PIX_BGR canvases[k] receives format F; canvas_stride obeys F's rule (>= canvas_w; 3 * canvas_w is no longer
 *                         required).  produced[], batching, sub-batches and the three-queue pipeline stay as they are; stage 3 downloads 1.5 B / pixel.
 *                         lvm_export_geometry is unchanged.
 * Surfaces that do NOT take part: lvm_export_frames_mjpeg, lvm_export_mjpeg_frames, lvm_mjpeg_encode_device (BGR in, JPEG out), lvm_chain_* and
 * lvm_chain_present (frames, not canvases), lvm_compose_device (always BGR), lvm_overlay_device (BGR canvases).
 * Work unit: 2 rows x 8 pixels per thread.  lvm_profile_variants reports under "canvas_yuv" the kernel that ran: "vec8" (dword-wide loads and stores:
 * every pointer, stride and plane offset involved dword-aligned, w a multiple of 8 -- and, reading panes, a pane-1 column that is a multiple of 8) or
 * "bytes" (everything else); both give identical bytes.  lvm_export_frames without labels reads the panes directly and never writes the BGR canvas:
 * that route reports "fused" as well (LVM_CANVAS_FUSED=0 forces compose, then convert); with labels it composes, overlays, then converts.      */
enum { LVM_PIX_I420 = 6,      /* canvas formats only: h rows of Y, h/2 rows of U, h/2 rows of V (FFmpeg yuv420p) */
       LVM_PIX_YV12 = 7 };    /* ... V before U */
int  lvm_set_canvas_format(lvm_ctx* ctx, int fmt);
int  lvm_get_canvas_format(lvm_ctx* ctx, int* fmt);
int  lvm_canvas_layout(int fmt, int canvas_w, int canvas_h, ptrdiff_t canvas_stride, size_t* bytes, size_t* plane1_offset, size_t* plane2_offset,
                       ptrdiff_t* chroma_stride);
int  lvm_canvas_convert_device(lvm_ctx* ctx, int fmt, const uint8_t* d_bgr, int w, int h, ptrdiff_t bgr_stride, ptrdiff_t bgr_frame_stride, int n_frames,
                               uint8_t* d_out, ptrdiff_t out_stride, ptrdiff_t out_frame_stride, void* hip_stream);

/* Cross-frame software pipeline for lvm_process_device (throughput mode, default depth 0).
 * depth 1 (implemented for the Laplace mode; other modes ignore it): a call enqueues the
 * down-sweep of ITS frame on an internal second stream concurrently with the up-sweep + output of
 * the PREVIOUS frame, so the output of call t is written (into the d_out given at call t) when
 * call t+1 -- or lvm_flush -- has been enqueued.  d_in / d_out of a call must stay valid until
 * then.  Results are identical to depth 0; only the schedule differs.  lvm_process (host path) and
 * the reference shim always run at depth 0.                                                   */
int  lvm_set_pipeline(lvm_ctx* ctx, int depth);
/* Enqueue whatever the pipeline still holds on `hip_stream` (NULL = the context's own stream). */
int  lvm_flush(lvm_ctx* ctx, void* hip_stream);

/* Wait for everything enqueued by lvm_process_device on the context's own stream. */
int  lvm_synchronize(lvm_ctx* ctx);

const char* lvm_last_error(lvm_ctx* ctx);

/* processing/magnification/SpatialFilter.cpp:5-11 calculateMaxLevels */
int  lvm_max_levels(int w, int h);
/* processing/magnification/TemporalFilter.cpp:82-94 getOptimalBufferSize */
int  lvm_optimal_buffer_size(int fps);
/* processing/magnification/TemporalFilter.cpp:280-297 butterworth(N = 2, Wn) */
void lvm_butterworth2(double Wn, double a[3], double b[3]);

/* ---- instrumentation (not part of the reference surface) -------------------------------- */
/* Keep the pre-quantisation float frame of stream 0 (parity metric).
 * lvm_debug_read_float copies w*h*channels floats (interleaved like the u8 output); for a
 * gray Phase frame under lvm_set_phase_on_gray the kept frame has three channels (w*h*3).  */
int  lvm_debug_keep_float(lvm_ctx* ctx, int on);
int  lvm_debug_read_float(lvm_ctx* ctx, float* dst, size_t count);
/* Colour arithmetic.  The forward conversion is what cv::cvtColor(COLOR_BGR2Lab) on CV_32F computes in OpenCV 4
 * (MagnifyCore.hpp:90,219): RGB2Labfloat's trilinear interpolation in a 33 x 33 x 33 int16 table -- integer work, bit-exact.
 * lvm_debug_exact_lab(1): every float operation around it (inverse conversion, pyramid taps, Riesz amplify) in OpenCV's
 * operation order with true divisions -- bit-faithful to the CPU oracle on the emulation build, used by the kernel-logic
 * tests; 0 (default): reciprocal multiplies / fma chains / hardware transcendentals where the value feeds
 * well-conditioned math.  lvm_debug_lab_analytic(1): the cube-root form RGB2Lab_f computes when OpenCV's interpolation is
 * switched off (implies the exact operation order).                                                                    */
int  lvm_debug_exact_lab(lvm_ctx* ctx, int on);
/* The output quantiser of the Lab modes -- u8 = saturate_cast<uchar>(cvRound(255 * invGamma(clip01(c)) + 1/255)) per channel
 * (Lab2RGBfloat + convertTo, MagnifyCore.hpp:152-153, :275-276) -- runs as a 4096-slice step table in the default flavour
 * (lab_tables.cpp build_u8_steps).  This entry compares the table with the operations it replaces for every float whose bit
 * pattern lies in [first_bits, first_bits + count) ON THE DEVICE: *mismatches = patterns where the bytes differ, *first_bad_bits =
 * the smallest of them.  (0, 1 << 32) sweeps every binary32 value: negative, above 1, infinities, NaN included.             */
/* Measurement aid (bench.py `clock_mhz`): a one-lane kernel on the context's auxiliary stream reads the shader-clock counter
 * (s_memtime) and the constant 100 MHz counter (s_memrealtime), waits -- beside whatever runs on the other streams -- until _stop is
 * called (or max_seconds, <= 5, have passed), and reads them again: *mhz = the AVERAGE shader clock over that interval, *seconds its
 * length.  One probe at a time per context.                                                                                        */
int  lvm_debug_clock_probe_start(lvm_ctx* ctx, double max_seconds);
int  lvm_debug_clock_probe_stop(lvm_ctx* ctx, double* mhz, double* seconds);
int  lvm_debug_sweep_u8_steps(lvm_ctx* ctx, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint32_t* first_bad_bits);
int  lvm_debug_lab_analytic(lvm_ctx* ctx, int on);
/* The portable transcendental functions of the Riesz mode (csrc/rz_trig.h: what the exact flavour calls under LVM_RZ_PORTABLE_TRIG=1 and
 * the oracle under LVMO_VAR_PORTABLE_TRIG) ON THE DEVICE: d_y[i] = fn(d_x[i]) for n floats in device memory, fn 0 = rz_acosf, 1 = rz_sinf,
 * 2 = rz_cosf.  Asynchronous on `stream` (null: the context's own).                                                                   */
int  lvm_debug_trig_eval(lvm_ctx* ctx, int fn, const float* d_x, float* d_y, size_t n, void* stream);
/* The forward table: LVM_LAB_LUT_ENTRIES int16 values in OpenCV's RGB2Labprev order, index 3 (p + 33 q + 1089 r) + channel
 * with p, q, r the R, G, B grid indices and entries L / 100 * 16384, (a + 128) / 256 * 16384, (b + 128) / 256 * 16384.
 * lvm_create builds it by restating initLabTabs (color_lab.cpp); lvm_set_lab_lut installs another one, e.g. the table of
 * a real OpenCV build recovered by converting the 33^3 node colours (oracle/ref_driver.cpp) -- the context must be idle. */
#define LVM_LAB_LUT_ENTRIES (33 * 33 * 33 * 3)
int  lvm_get_lab_lut(lvm_ctx* ctx, int16_t* dst);
int  lvm_set_lab_lut(lvm_ctx* ctx, const int16_t* src);
/* Per-kernel timing with HIP events recorded on the launch stream.  While enabled every
 * kernel launch is bracketed by two events; lvm_profile_collect synchronises and folds them
 * into per-kernel totals, readable with lvm_profile_entry (idx = 0..n-1).                   */
int  lvm_profile_enable(lvm_ctx* ctx, int on);
int  lvm_profile_collect(lvm_ctx* ctx);
/* Clears the totals and restricts the bracketing to launches with this report name (NULL or "": all launches).  With
 * one kernel bracketed its neighbours run back to back, as they do outside the profiling pass: the VALU-bound kernels
 * take ~10 % longer that way than with an event gap on both sides (the clock recovers in the gaps), and that is the
 * duration rocprofv3 reports for them.                                                                              */
int  lvm_profile_only(lvm_ctx* ctx, const char* name);
int  lvm_profile_entry(lvm_ctx* ctx, int idx, char* name, size_t name_cap, double* total_ms,
                       long long* launches);
/* Which kernels ran under entry idx's report name, comma-separated, where several share one (lap_down0, lap_final,
 * lab_lut, rz_lab, rz_final, col_down0, col_minmax, col_out): "strips" = the wave-strip kernel, "vec4" = the tiled kernel
 * with dword-wide frame I/O, "bytes" = the tiled kernel with byte I/O; under a build kind of lvm_set_opencv_build the Riesz launches it changes add "unfused", "f64", "mulf32" or
 * "unfused+mulf32"; gray Phase frames (lvm_set_phase_on_gray) run "gray4" / "gray" (dword / byte frame I/O) under lab_lut, rz_lab and
 * rz_final, and "gray-strips" under rz_final.  Empty for names with one kernel.  The frame's
 * layout picks among them (see lvm_process_device); the tests use this to see that it picked what the launch code says. */
int  lvm_profile_variants(lvm_ctx* ctx, int idx, char* variants, size_t cap);
/* Algorithmic bytes per frame per stream for the current geometry/mode. */
double lvm_algorithmic_bytes(int mode, int w, int h, int channels, int levels, double framerate);

#ifdef __cplusplus
}
#endif
#endif
