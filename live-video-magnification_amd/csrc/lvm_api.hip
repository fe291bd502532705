// lvm_api.hip -- C ABI of liblvm_hip.so (see include/lvm_hip.h) and the host-side logic of
// the reference's MagnificationProcessor (processing/MagnificationProcessor.cpp:10-67):
// level clamping, structural-change reset (MagnifyCore.hpp:45-80), dispatch by mode and the
// passthrough rules.  No CPU fallback exists: without a usable HIP device every entry point
// fails with LVM_ERR_NO_DEVICE.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "lvm_internal.h"

struct lvm_ctx : lvm::Ctx {};

namespace lvm {

void prof_begin(Ctx* c, const char* name, hipStream_t s) {
    c->prof_skip = !c->prof_only.empty() && c->prof_only != name;     // lvm_profile_only: every other launch runs unbracketed
    if (c->prof_skip) return;
    int id = -1;
    for (size_t i = 0; i < c->prof_totals.size(); ++i)
        if (c->prof_totals[i].name == name) { id = (int)i; break; }
    if (id < 0) { ProfTotal t; t.name = name; c->prof_totals.push_back(t); id = (int)c->prof_totals.size() - 1; }
    ProfEvent e; e.name = id;
    (void)hipEventCreate(&e.e0); (void)hipEventCreate(&e.e1);
    (void)hipEventRecord(e.e0, s);
    c->prof_events.push_back(e);
}
void prof_variant(Ctx* c, const char* variant) {      // of the launch prof_begin has just opened
    if (c->prof_skip) return;
    auto& v = c->prof_totals[c->prof_events.back().name].variants;
    for (const auto& x : v) if (x == variant) return;
    v.emplace_back(variant);
}
void prof_end(Ctx* c, hipStream_t s) { if (!c->prof_skip) (void)hipEventRecord(c->prof_events.back().e1, s); }

// Waits for everything this context has enqueued -- on its own two streams and on caller streams: one event PER DISTINCT
// caller stream, re-recorded after every enqueue on it (an event outlives the stream it was recorded on).  Not a
// device-wide synchronisation: the reference runs a live chain and an export chain side by side
// (export/Exporter.cpp:204,231) and one context's reset must not stall the other.  A caller that cycles through more
// than kMaxCallerStreams streams gets hipDeviceSynchronize instead (correct, just wider).
constexpr size_t kMaxCallerStreams = 8;
void sync_streams(Ctx* c) {
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    if (c->aux_stream) (void)hipStreamSynchronize(c->aux_stream);
    if (c->up_stream) (void)hipStreamSynchronize(c->up_stream);
    if (c->down_stream) (void)hipStreamSynchronize(c->down_stream);
    for (auto& e : c->caller_events) (void)hipEventSynchronize(e.second);
    // the device-wide wait has covered everything enqueued so far, on any stream: the flag starts afresh (it is not sticky)
    if (c->caller_overflow) { (void)hipDeviceSynchronize(); c->caller_overflow = false; }
    (void)hipGetLastError();
}
// Re-records the event of s's slot in caller_events behind the enqueue and leaves it in *behind; false where the stream has no slot (or the
// record failed): sync_streams then covers it with the device-wide wait.
static bool mark_slot(Ctx* c, hipStream_t s, hipEvent_t* behind) {
    for (auto& e : c->caller_events)
        if (e.first == s) { if (hipEventRecord(e.second, s) != hipSuccess) { (void)hipGetLastError(); return false; } *behind = e.second; return true; }
    hipEvent_t ev = nullptr;
    if (c->caller_events.size() >= kMaxCallerStreams) {
        // full: recycle a slot whose event has completed (its stream's work is done -- the stream may not even exist any
        // more; stream-per-call callers and framework stream pools would otherwise fill the list for good)
        for (size_t i = 0; i < c->caller_events.size(); ++i) {
            auto& e = c->caller_events[i];
            if (hipEventQuery(e.second) == hipSuccess) {
                (void)hipGetLastError();    // hipErrorNotReady of the earlier slots' queries must not surface as the next call's error
                if (hipEventRecord(e.second, s) != hipSuccess) {
                    // the slot no longer describes a live enqueue: drop it (its event with it) instead of keeping a stale stream
                    (void)hipGetLastError();
                    (void)hipEventDestroy(e.second);
                    c->caller_events.erase(c->caller_events.begin() + (ptrdiff_t)i);
                    return false;
                }
                e.first = s;
                *behind = e.second;
                return true;
            }
        }
        (void)hipGetLastError();        // hipErrorNotReady of the queries
        return false;
    }
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (hipEventRecord(ev, s) != hipSuccess) { (void)hipGetLastError(); (void)hipEventDestroy(ev); return false; }
    c->caller_events.emplace_back(s, ev);
    *behind = ev;
    return true;
}
void mark_enqueued(Ctx* c, hipStream_t s) {
    c->last_stream = s;
    if (s == c->own_stream) return;                       // the own stream is synchronised directly; it records ev_own only when a call leaves it
    c->last_marked = mark_slot(c, s, &c->ev_last);
    if (c->last_marked) return;
    // no slot: the next call on another stream (order_after_previous) waits for the spare event -- or, should this record fail too, for the device
    c->caller_overflow = true;
    c->ev_last = c->ev_spill;
    c->last_marked = hipEventRecord(c->ev_spill, s) == hipSuccess;
    if (!c->last_marked) (void)hipGetLastError();
}

// Calls of one context take effect in call order on whatever streams they are given (include/lvm_hip.h): the temporal state -- IIR planes,
// filter state, Color's ring, the parity-buffered pyramids -- lives in the context, where no caller can order it.  A call whose stream is
// not the one of the previous enqueue makes its stream wait, ON THE DEVICE, for the event behind that enqueue before it enqueues anything;
// waits chain, so everything older is covered too.  A call on the same stream as the previous one makes no HIP call here.
int order_after_previous(Ctx* c, hipStream_t s) {
    const hipStream_t prev = c->last_stream;
    if (!prev || prev == s) return LVM_OK;
    if (prev == c->own_stream) {
        LVM_HIP_TRY(c, hipEventRecord(c->ev_own, prev));            // behind everything the own stream has been given so far
        LVM_HIP_TRY(c, hipStreamWaitEvent(s, c->ev_own, 0));
    } else if (c->last_marked) {
        LVM_HIP_TRY(c, hipStreamWaitEvent(s, c->ev_last, 0));
    } else {
        LVM_HIP_TRY(c, hipDeviceSynchronize());                      // no event could be recorded behind that enqueue
    }
    return LVM_OK;
}

static void drop_state(Ctx* c) { delete c->state; c->state = nullptr; }

// (re)build the device layouts of the forward Lab table from c->lab_lut_compact
int upload_lab_lut(Ctx* c) {
    std::vector<uint32_t> ab; std::vector<int16_t> lcells;
    lab_lut_device_tables(c->lab_lut_compact.data(), ab, lcells);
    if (!c->d_lab_ab && hipMalloc((void**)&c->d_lab_ab, ab.size() * sizeof(uint32_t)) != hipSuccess) { c->d_lab_ab = nullptr; c->err = "hipMalloc (Lab table) failed"; return LVM_ERR_OOM; }
    if (!c->d_lab_Lcells && hipMalloc((void**)&c->d_lab_Lcells, lcells.size() * sizeof(int16_t)) != hipSuccess) { c->d_lab_Lcells = nullptr; c->err = "hipMalloc (Lab table) failed"; return LVM_ERR_OOM; }
    LVM_HIP_TRY(c, hipMemcpy(c->d_lab_ab, ab.data(), ab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    LVM_HIP_TRY(c, hipMemcpy(c->d_lab_Lcells, lcells.data(), lcells.size() * sizeof(int16_t), hipMemcpyHostToDevice));
    c->lab_lut.ab = c->d_lab_ab; c->lab_lut.Lcells = c->d_lab_Lcells;
    return LVM_OK;
}

// lazy, per mode (MagnificationProcessor.cpp:48-60); Riesz on gray frames creates nothing and the frame passes through
static int create_state(Ctx* c, int mode, int levels, const FrameIO& io, hipStream_t s) {
    switch (mode) {
    case LVM_MODE_LAPLACE: return laplace_create(c, levels, io, s);
    case LVM_MODE_PHASE:   return riesz_create(c, levels, io, s);
    case LVM_MODE_COLOR:   return color_create(c, levels, io, s);
    default: break;
    }
    return LVM_OK;
}

// A failed call (allocation failure, launch error) must not leave a half-built state installed: the next call
// would launch kernels on null buffers.  Drop it and disarm the tracker so that the next frame starts afresh,
// which is also what the reference's recovery path does (ProcessingChain.cpp:50-62 resets every stage).
static void tracker_disable(Ctx* c);
void fail_state(Ctx* c, hipStream_t s) {
    (void)hipStreamSynchronize(s);
    sync_streams(c);
    drop_state(c);
    tracker_disable(c);
}
static void tracker_disable(Ctx* c) { const uint64_t pre = c->tracked.pre; c->tracked = StructKey{}; c->tracked.pre = pre; }

// channels of the float frame lvm_debug_keep_float keeps: the frame's own, except that a gray Phase frame under lvm_set_phase_on_gray keeps the
// three-channel BGR frame in front of the quantiser (what the oracle holds for the expanded frame)
static size_t float_channels(const Ctx* c, int mode, int channels) { return (c->phase_on_gray && mode == LVM_MODE_PHASE && channels == 1) ? 3 : (size_t)channels; }

int ensure_float(Ctx* c, size_t count) {
    if (count * sizeof(float) > c->d_float.cap) {
        sync_streams(c);            // kernels of earlier calls may still be writing the kept frame
        const int rc = c->d_float.reserve(c, count * sizeof(float));
        if (rc != LVM_OK) return rc;
    }
    c->float_count = count;
    return LVM_OK;
}

// The layouts the device surfaces take (include/lvm_hip.h): rows that hold their pixels (compose_device's rule); stream strides are
// free -- two streams side by side in one mosaic frame have a stream stride of one row -- except that the outputs of several
// streams must not land on each other.  Inside one frame the kernels address with 32 bits -- unsigned row offsets, buffer resources of
// stride * (h - 1) + w * channels bytes, the signed offsets of the buffer intrinsics -- so the rows of a frame, first byte to last, span
// at most INT32_MAX bytes; streams and frames of a call may lie any distance apart (64-bit bases).  Null: fine.
static const char* layout_error(const FrameIO& io, int nstreams) {
    const ptrdiff_t row = (ptrdiff_t)io.w * io.channels, span_max = INT32_MAX;
    if (io.in_stride < row || io.out_stride < row) return "frame stride too small";
    if (nstreams > 1 && io.out_sstride <= 0) return "stream stride too small";
    // (h - 1) * stride + row > span_max, without the product
    auto too_far = [&](ptrdiff_t stride) { return row > span_max || (io.h > 1 && stride > (span_max - row) / (io.h - 1)); };
    if (too_far(io.in_stride) || too_far(io.out_stride)) return "frame rows span more than 2 GiB";
    return nullptr;
}

// A source frame as an entry point is given it, checked before any state changes: BGR / gray frames, and the rules of include/lvm_hip.h for the
// raw camera formats (lvm_set_source_format).  Null: fine.
static const char* source_frame_error(int fmt, int w, int h, int channels, ptrdiff_t in_stride) {
    if (fmt == LVM_PIX_BGR) return (w <= 0 || h <= 0 || (channels != 1 && channels != 3) || in_stride < (ptrdiff_t)w * channels) ? "bad frame arguments" : nullptr;
    const bool nv = fmt == LVM_PIX_NV12 || fmt == LVM_PIX_NV21;
    if (channels != 3) return "raw source format: channels must be 3 (it describes the frame the chain sees)";
    if (w <= 0 || h <= 0) return "bad frame arguments";
    if (w % 2) return "raw source format: w must be even";
    if (nv && h % 2) return "raw source format: h must be even for NV12 / NV21";
    if (in_stride < (ptrdiff_t)w * (nv ? 1 : 2)) return nv ? "raw source format: in_stride must be >= w for NV12 / NV21" : "raw source format: in_stride must be >= 2 * w for the packed formats";
    return nullptr;
}

// MagnificationProcessor::process (MagnificationProcessor.cpp:17-67) on device buffers
static int process_device(Ctx* c, const lvm_params* p, const FrameIO& io, hipStream_t s, int* produced) {
    *produced = 0;
    { const int rc = order_after_previous(c, s); if (rc != LVM_OK) return rc; }
    if (p->mode == LVM_MODE_NONE || io.d_in == nullptr || io.w <= 0 || io.h <= 0) {      // :21-29
        if (c->tracked.mode != LVM_MODE_NONE) {
            // pipelined mode: the pending frame's output is owed to its caller (same rule as on a structural change)
            if (c->state) (void)c->state->flush(c, s);
            LVM_HIP_TRY(c, hipStreamSynchronize(s));
            sync_streams(c);
            drop_state(c); tracker_disable(c);
        }
        return LVM_OK;
    }
    if (p->mode < 0 || p->mode > LVM_MODE_NONE) { c->err = "invalid mode"; return LVM_ERR_INVALID; }
    if (io.channels != 1 && io.channels != 3) { c->err = "channels must be 1 or 3"; return LVM_ERR_INVALID; }
    if (io.d_out == nullptr) { c->err = "null output"; return LVM_ERR_INVALID; }
    const StructKey key = struct_key(*p, io.w, io.h, io.channels);                      // :32-34
    if (key.levels < 1) return LVM_OK;
    // the kernels address the rows of a frame with 32-bit offsets: refuse what they cannot walk (layout_error) before any state is touched
    if (const char* why = layout_error(io, c->nstreams)) { c->err = why; return LVM_ERR_INVALID; }
    if (key != c->tracked) {                                                            // MagnifyCore.hpp:53-65
        // buffers of the old geometry may still be in use by queued kernels
        if (c->state) (void)c->state->flush(c, s);                       // pipelined mode: do not lose the pending frame
        LVM_HIP_TRY(c, hipStreamSynchronize(s));
        sync_streams(c);                                                 // earlier calls may have used other streams
        c->tracked = key;
        drop_state(c);                                                                  // :39-43
    }
    if (c->keep_float) {
        const int rc = ensure_float(c, (size_t)io.w * io.h * float_channels(c, p->mode, io.channels));
        if (rc != LVM_OK) return rc;
    }
    int rc = c->state ? LVM_OK : create_state(c, p->mode, key.levels, io, s);
    if (rc == LVM_OK && c->state) rc = c->state->process(c, *p, io, s, produced);
    mark_enqueued(c, s);
    if (rc != LVM_OK) fail_state(c, s);
    return rc;
}

// run the magnifier with pipeline depth 0: the synchronous surfaces complete their own frames
template <class Run>
static int at_depth0(Ctx* c, Run&& run) {
    const int depth = c->pipeline_depth;
    c->pipeline_depth = 0;
    const int rc = run();
    c->pipeline_depth = depth;
    return rc;
}

// What an entry point that enqueues on the caller's stream does around its call: the device, the stream of the call (null: the context's own), the
// wait that orders it behind the previous call, the call, and the mark the next call orders itself behind -- set whether or not `run` succeeded:
// a failed call may have enqueued part of its work.
template <class Run>
static int on_stream(Ctx* c, void* hip_stream, Run&& run) {
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    int rc = order_after_previous(c, s);
    if (rc != LVM_OK) return rc;
    rc = run(s);
    mark_enqueued(c, s);
    return rc;
}

}  // namespace lvm

using lvm::Ctx;

extern "C" {

int lvm_create(int device, int n_streams, lvm_ctx** out) {
    if (!out || n_streams < 1) return LVM_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return LVM_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return LVM_ERR_NO_DEVICE;
    lvm_ctx* c = new (std::nothrow) lvm_ctx();
    if (!c) return LVM_ERR_OOM;
    c->device = device;
    c->nstreams = n_streams;
    { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) c->num_cus = n; }
    float g[256] = {}, ig[4096] = {};
    lvm::build_lab_tables(g, ig, c->lab.fwd, c->lab.inv);
    for (int i = 0; i < 9; ++i) { c->lab.inv1024[i] = c->lab.inv[i] * 1024.0f; c->lab.inv4096[i] = c->lab.inv[i] * 4096.0f; }
    std::vector<uint32_t> steps(2 * lvm::kU8StepSlices);
    if (!lvm::build_u8_steps(ig, steps.data())) { delete c; return LVM_ERR_INVALID; }      // (cannot happen with OpenCV's spline: checked by the tests)
    bool ok = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_own, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_spill, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->d_gamma_u8, sizeof(g)) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->d_invgamma, sizeof(ig)) == hipSuccess;
    ok = ok && hipMemcpy(c->d_gamma_u8, g, sizeof(g), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(c->d_invgamma, ig, sizeof(ig), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->d_u8steps, steps.size() * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMemcpy(c->d_u8steps, steps.data(), steps.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        // OpenCV's forward Lab table (lab_tables.cpp) and the closed form of its cell index (lab_lut.h)
        if (!lvm::lab_lut_fine_index_ok()) { lvm_destroy(c); return LVM_ERR_INVALID; }
        lvm::build_lab_lut_compact(c->lab_lut_compact);
        const int rc = lvm::upload_lab_lut(c);
        if (rc != LVM_OK) { lvm_destroy(c); return rc; }                 // LVM_ERR_OOM stays LVM_ERR_OOM
    }
    if (!ok) { lvm_destroy(c); return LVM_ERR_HIP; }
    c->lab.gamma_u8 = c->d_gamma_u8;
    c->lab.invgamma = c->d_invgamma;
    c->lab.u8steps = c->d_u8steps;
    c->lab.a255 = (float)(1.0 / 255.0f);
    *out = c;
    return LVM_OK;
}

void lvm_destroy(lvm_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    lvm::sync_streams(c);
    delete c->state; c->state = nullptr;
    for (auto& e : c->prof_events) { (void)hipEventDestroy(e.e0); (void)hipEventDestroy(e.e1); }
    if (c->d_gamma_u8) (void)hipFree(c->d_gamma_u8);
    if (c->d_invgamma) (void)hipFree(c->d_invgamma);
    if (c->d_u8steps) (void)hipFree(c->d_u8steps);
    lvm::overlay_release(c);
    if (c->probe_running) { double m = 0; (void)lvm::clock_probe_stop(c, &m, nullptr); }
    if (c->h_probe) (void)hipHostFree(c->h_probe);
    if (c->d_lab_ab) (void)hipFree(c->d_lab_ab);
    if (c->d_lab_Lcells) (void)hipFree(c->d_lab_Lcells);
    lvm::preprocess_release(c);
    lvm::mjpeg_release(c);
    lvm::mjpeg_decode_release(c);
    for (auto e : c->ev_up) (void)hipEventDestroy(e);
    for (auto e : c->ev_done) (void)hipEventDestroy(e);
    if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
    if (c->down_stream) (void)hipStreamDestroy(c->down_stream);
    for (auto& e : c->caller_events) (void)hipEventDestroy(e.second);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_own) (void)hipEventDestroy(c->ev_own);
    if (c->ev_spill) (void)hipEventDestroy(c->ev_spill);
    if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;                       // (the staging buffers go with it: DevBuf)
}

int lvm_reset(lvm_ctx* c) {                       // MagnificationProcessor.cpp:10-15
    if (!c) return LVM_ERR_INVALID;
    (void)hipSetDevice(c->device);
    // (an owed pipelined frame is discarded: reset() means "forget everything", MagnificationProcessor.cpp:10-15)
    lvm::sync_streams(c);
    lvm::drop_state(c);
    c->tracked = lvm::StructKey{};
    c->err.clear();
    return LVM_OK;
}

int lvm_process_device(lvm_ctx* c, const lvm_params* p, const uint8_t* d_in, int w, int h, int channels,
                       ptrdiff_t in_stride, ptrdiff_t in_stream_stride, uint8_t* d_out, ptrdiff_t out_stride,
                       ptrdiff_t out_stream_stride, int* produced, void* hip_stream) {
    if (!c || !p || !produced) return LVM_ERR_INVALID;
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    lvm::FrameIO io{d_in, in_stride, in_stream_stride, d_out, out_stride, out_stream_stride, w, h, channels};
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return lvm::process_device(c, p, io, s, produced);
}

int lvm_process_device_frames(lvm_ctx* c, const lvm_params* p, int n_frames, const uint8_t* d_in, int w, int h, int channels,
                              ptrdiff_t in_stride, ptrdiff_t in_stream_stride, ptrdiff_t in_frame_stride, uint8_t* d_out,
                              ptrdiff_t out_stride, ptrdiff_t out_stream_stride, ptrdiff_t out_frame_stride, int* produced,
                              void* hip_stream) {
    if (!c || !p || !produced || n_frames < 1) return LVM_ERR_INVALID;
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    if (c->keep_float && w > 0 && h > 0 && (channels == 1 || channels == 3) &&         // the batched schedules keep the first frame of a batch
        !lvm::layout_error(lvm::FrameIO{d_in, in_stride, in_stream_stride, d_out, out_stride, out_stream_stride, w, h, channels}, c->nstreams)) {   // (a refused layout reserves nothing)
        const int rc = lvm::ensure_float(c, (size_t)w * h * lvm::float_channels(c, p->mode, channels));
        if (rc != LVM_OK) return rc;
    }
    int f = 0;
    while (f < n_frames) {
        lvm::FrameIO io{d_in ? d_in + (size_t)f * in_frame_stride : nullptr, in_stride, in_stream_stride,
                        d_out ? d_out + (size_t)f * out_frame_stride : nullptr, out_stride, out_stream_stride, w, h, channels};
        // temporal batch: same structural key as the tracked state, a state that is steady for these parameters, frames laid
        // out [frame][stream]; everything else (first frames, odd layouts) goes frame by frame
        const int left = n_frames - f;
        const bool same = d_in && d_out && lvm::struct_key(*p, w, h, channels) == c->tracked;
        const bool layout = in_frame_stride == in_stream_stride * c->nstreams && out_frame_stride == out_stream_stride * c->nstreams;
        // (a layout the per-frame path refuses is left to it: it reports the error)
        const int nb = (left >= 2 && same && layout && c->state && !lvm::layout_error(io, c->nstreams)) ? c->state->batch_frames(c, *p, io, left) : 0;
        if (nb > 0) {
            int rc = lvm::order_after_previous(c, s);
            if (rc != LVM_OK) return rc;
            rc = c->state->process_frames(c, *p, io, nb, s);
            lvm::mark_enqueued(c, s);
            if (rc != LVM_OK) { lvm::fail_state(c, s); return rc; }
            for (int k = f; k < f + nb; ++k) produced[k] = 1;
            f += nb;
            continue;
        }
        const int rc = lvm::process_device(c, p, io, s, &produced[f]);
        if (rc != LVM_OK) return rc;
        ++f;
    }
    return LVM_OK;
}


int lvm_preprocess_geometry(const lvm_preprocess_params* pp, int w, int h, int channels, int* rx, int* ry, int* rw, int* rh,
                            int* ow, int* oh, int* och) {
    if (!pp || w <= 0 || h <= 0 || (channels != 1 && channels != 3)) return LVM_ERR_INVALID;
    int v[7];
    lvm::preprocess_geometry(*pp, w, h, channels, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]);
    int* dst[7] = {rx, ry, rw, rh, ow, oh, och};
    for (int i = 0; i < 7; ++i) if (dst[i]) *dst[i] = v[i];
    return LVM_OK;
}

int lvm_preprocess_device(lvm_ctx* c, const lvm_preprocess_params* pp, const uint8_t* d_in, int w, int h, int channels,
                          ptrdiff_t in_stride, ptrdiff_t in_stream_stride, uint8_t* d_out, ptrdiff_t out_stride,
                          ptrdiff_t out_stream_stride, void* hip_stream) {
    if (!c || !pp) return LVM_ERR_INVALID;
    const int fmt = c->source_format;
    // (a BGR / gray frame is checked by preprocess_device, with its own text and without a rule for in_stride: only the raw rules are checked here)
    if (fmt != LVM_PIX_BGR) {
        if (const char* why = lvm::source_frame_error(fmt, w, h, channels, in_stride)) { c->err = why; return LVM_ERR_INVALID; }
    }
    // the whole raw frame is on the device: its pixel (0, 0) starts a chroma pair / block, the UV plane starts at row h (NV12 / NV21)
    const lvm::RawSource raw{fmt, 0, 0, (ptrdiff_t)h * in_stride};
    // (the area tables are the context's: preprocess.hip replaces them behind a wait for the call's stream alone)
    return lvm::on_stream(c, hip_stream, [&](hipStream_t s) {
        return lvm::preprocess_device(c, *pp, lvm::Image{d_in, w, h, channels, in_stride, in_stream_stride}, lvm::ImageOut{d_out, 0, 0, 0, out_stride, out_stream_stride}, s,
                                      lvm::ImageOut(), fmt != LVM_PIX_BGR ? &raw : nullptr);
    });
}

int lvm_compose_geometry(int split, int ow, int oh, int pw, int ph, int* pane_w, int* pane_h, int* canvas_w, int* canvas_h) {
    if (split < LVM_SPLIT_NONE || split > LVM_SPLIT_TOP_BOTTOM) return LVM_ERR_INVALID;
    int v[4];
    (void)lvm::compose_geometry(split, ow, oh, pw, ph, &v[0], &v[1], &v[2], &v[3]);
    int* dst[4] = {pane_w, pane_h, canvas_w, canvas_h};
    for (int i = 0; i < 4; ++i) if (dst[i]) *dst[i] = v[i];
    return LVM_OK;
}

int lvm_compose_device(lvm_ctx* c, int split, const uint8_t* d_orig, int ow, int oh, int och, ptrdiff_t orig_stride,
                       ptrdiff_t orig_stream_stride, const uint8_t* d_proc, int pw, int ph, int pch, ptrdiff_t proc_stride,
                       ptrdiff_t proc_stream_stride, uint8_t* d_canvas, ptrdiff_t canvas_stride, ptrdiff_t canvas_stream_stride,
                       void* hip_stream) {
    if (!c) return LVM_ERR_INVALID;
    return lvm::on_stream(c, hip_stream, [&](hipStream_t s) {
        return lvm::compose_device(c, split, lvm::Image{d_orig, ow, oh, och, orig_stride, orig_stream_stride}, lvm::Image{d_proc, pw, ph, pch, proc_stride, proc_stream_stride},
                                   lvm::ImageOut{d_canvas, 0, 0, 3, canvas_stride, canvas_stream_stride}, s);
    });
}

// ---- spatial tiling of ONE Riesz stream (demonstrator; the production answer to several GPUs is one stream per GPU) ----------------------
static int tile_check(lvm_ctx* c, const lvm_params* p, int w, int h) {
    if (!c || !p) return LVM_ERR_INVALID;
    if (p->mode != LVM_MODE_PHASE || c->nstreams != 1 || w < 1 || h < 1) { c->err = "tiling: the Riesz mode on a 1-stream context"; return LVM_ERR_INVALID; }
    return LVM_OK;
}

int lvm_tile_riesz_stage1(lvm_ctx* c, const lvm_params* p, const uint8_t* d_in, int w, int h, ptrdiff_t in_stride, int* produced,
                          float* d_residual_out, int* residual_w, int* residual_h, void* hip_stream) {
    int rc = tile_check(c, p, w, h);
    if (rc != LVM_OK) return rc;
    if (!d_in || !produced || lvm::source_frame_error(LVM_PIX_BGR, w, h, 3, in_stride)) { c->err = "tiling: bad frame arguments"; return LVM_ERR_INVALID; }
    // by hand: process_device orders and marks the call itself, and runs between the two settings of tile_mode
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    // (no output in this stage: the frame argument stands in for the output pointer the per-frame path asks for and is never written)
    lvm::FrameIO io{d_in, in_stride, in_stride * h, const_cast<uint8_t*>(d_in), in_stride, in_stride * h, w, h, 3};
    c->tile_mode = 1;
    rc = lvm::process_device(c, p, io, s, produced);
    c->tile_mode = 0;
    if (rc != LVM_OK) return rc;
    return lvm::riesz_tile_residual(c, d_residual_out, residual_w, residual_h, s);
}

int lvm_tile_riesz_stage2(lvm_ctx* c, const lvm_params* p, const uint8_t* d_in, int w, int h, ptrdiff_t in_stride, const float* d_residual_in,
                          uint8_t* d_out, ptrdiff_t out_stride, void* hip_stream) {
    int rc = tile_check(c, p, w, h);
    if (rc != LVM_OK) return rc;
    if (!d_in || !d_out || !d_residual_in || lvm::source_frame_error(LVM_PIX_BGR, w, h, 3, in_stride) || out_stride < (ptrdiff_t)w * 3) { c->err = "tiling: bad frame arguments"; return LVM_ERR_INVALID; }
    if (c->tracked.mode != LVM_MODE_PHASE || c->tracked.w != w || c->tracked.h != h || c->tracked.channels != 3) { c->err = "tiling: stage 2 without a matching stage 1"; return LVM_ERR_INVALID; }
    const lvm::FrameIO io{d_in, in_stride, in_stride * h, d_out, out_stride, out_stride * h, w, h, 3};
    return lvm::on_stream(c, hip_stream, [&](hipStream_t s) { return lvm::riesz_tile_finish(c, *p, io, d_residual_in, s); });
}

int lvm_tile_riesz_planes(lvm_ctx* c, const lvm_params* p, const float* d_plane_in, int w, int h, float* d_plane_out, int* produced, void* hip_stream) {
    int rc = tile_check(c, p, w, h);
    if (rc != LVM_OK) return rc;
    if (!d_plane_in || !d_plane_out || !produced || p->levels < 2) { c->err = "tiling: planes in and out, at least two levels"; return LVM_ERR_INVALID; }
    // by hand, like stage 1: process_device orders and marks, between the two settings of tile_mode
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    // the per-frame path with a plane where the frame would be: three "channels" so that the Riesz mode accepts it (MagnifyCore.hpp:212);
    // neither pointer is touched as bytes (tile_mode 2: riesz.hip rz_build / rz_collapse_out)
    lvm::FrameIO io{reinterpret_cast<const uint8_t*>(d_plane_in), (ptrdiff_t)w * 3, (ptrdiff_t)w * 3 * h, reinterpret_cast<uint8_t*>(d_plane_out), (ptrdiff_t)w * 3,
                    (ptrdiff_t)w * 3 * h, w, h, 3};
    c->tile_mode = 2; c->tile_plane_in = d_plane_in; c->tile_plane_out = d_plane_out;
    rc = lvm::process_device(c, p, io, s, produced);
    c->tile_mode = 0; c->tile_plane_in = nullptr; c->tile_plane_out = nullptr;
    return rc;
}

int lvm_export_set_overlay(lvm_ctx* c, int n_labels, const lvm_overlay_label* labels) {
    if (!c) return LVM_ERR_INVALID;
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    return lvm::overlay_set(c, n_labels, labels);
}

int lvm_overlay_device(lvm_ctx* c, uint8_t* d_canvas, int canvas_w, int canvas_h, ptrdiff_t canvas_stride, ptrdiff_t frame_stride, int n_frames, void* hip_stream) {
    if (!c) return LVM_ERR_INVALID;
    return lvm::on_stream(c, hip_stream, [&](hipStream_t s) { return lvm::overlay_device(c, lvm::ImageOut{d_canvas, canvas_w, canvas_h, 3, canvas_stride, frame_stride}, n_frames, s); });
}

// FNV-1a over the PreprocessParams fields the reference compares (IProcessor.hpp:36-39)
static uint64_t preprocess_key_of(const lvm_preprocess_params& pp) {
    uint64_t k = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; ++i) { k ^= b[i]; k *= 1099511628211ull; } };
    const int32_t en = pp.roi_enabled ? 1 : 0;
    mix(&pp.downscale, 4); mix(&en, 4); mix(&pp.roiX, 4); mix(&pp.roiY, 4); mix(&pp.roiW, 4); mix(&pp.roiH, 4);
    return k;
}

// The host chain in front of the magnifier (PreprocessProcessor + GrayscaleProcessor) for one source geometry: what the chain and export
// entry points share.
struct ChainGeom {
    int channels, rx, ry, rw, rh, ow, oh, och;
    size_t roi_row, roi_bytes;      // the cropped source frame
    // raw source formats: the staged frame is the ROI widened to whole chroma pairs -- pixel columns [rx & ~1, (rx + rw - 1) | 1] of the ROI's
    // rows (2 bytes each: packed formats), or that many Y bytes per ROI row followed by the UV rows (ry >> 1) .. ((ry + rh - 1) >> 1) (NV12 / NV21)
    int fmt, h, uv_rows;
    lvm::RawSource raw;             // what the kernel needs to know about it: the parities of the ROI's origin, where the UV rows start
    size_t out_row, out_bytes;      // the frame the magnifier sees and the one it writes
    bool identity;                  // nothing to do in front of the magnifier (PreprocessProcessor.cpp:15, GrayscaleProcessor.cpp:8-9)
    // runChainOnce's `original` is chain[0]'s output (ChainBuilder.cpp:25: the tap sits BEFORE GrayscaleProcessor): with grayscale on
    // a BGR source it is the cropped / decimated COLOUR frame, not the gray frame the magnifier sees
    bool gray;
    size_t tap_row, tap_bytes;      // a frame of the tap: 3 channels with `gray`, the magnifier's input frame otherwise
};
static ChainGeom chain_geometry(const lvm_preprocess_params& pp, int w, int h, int channels, int fmt = LVM_PIX_BGR) {
    ChainGeom g{};
    g.channels = channels; g.fmt = fmt; g.h = h;
    lvm::preprocess_geometry(pp, w, h, channels, &g.rx, &g.ry, &g.rw, &g.rh, &g.ow, &g.oh, &g.och);
    g.roi_row = (size_t)g.rw * channels; g.roi_bytes = g.roi_row * g.rh;
    g.out_row = (size_t)g.ow * g.och; g.out_bytes = g.out_row * g.oh;
    g.identity = g.ow == g.rw && g.oh == g.rh && g.och == channels;
    g.gray = g.och == 1 && channels == 3;
    g.tap_row = g.gray ? (size_t)g.ow * 3 : g.out_row; g.tap_bytes = g.tap_row * g.oh;
    if (fmt != LVM_PIX_BGR) {
        const size_t cols = (size_t)(((g.rx + g.rw - 1) | 1) + 1 - (g.rx & ~1));
        const bool nv = fmt == LVM_PIX_NV12 || fmt == LVM_PIX_NV21;
        g.uv_rows = nv ? ((g.ry + g.rh - 1) >> 1) - (g.ry >> 1) + 1 : 0;
        g.roi_row = nv ? cols : cols * 2; g.roi_bytes = g.roi_row * ((size_t)g.rh + g.uv_rows);
        g.raw = lvm::RawSource{fmt, g.rx & 1, nv ? (g.ry & 1) : 0, (ptrdiff_t)(g.roi_row * g.rh)};
        g.identity = false;         // crop-only at full size is the plain conversion: it writes the BGR frame the magnifier reads
    }
    return g;
}
// only the ROI rows cross PCIe (the crop is the pitch of the 2-D copy)
static hipError_t chain_upload(const ChainGeom& g, uint8_t* d_dst, const uint8_t* frame, ptrdiff_t in_stride, hipStream_t s) {
    if (g.fmt != LVM_PIX_BGR) {     // the ROI's raw bytes: whole chroma pairs; NV12 / NV21: two 2-D copies
        const size_t x0 = (size_t)(g.rx & ~1) * (g.uv_rows ? 1 : 2);
        const hipError_t e = hipMemcpy2DAsync(d_dst, g.roi_row, frame + (size_t)g.ry * in_stride + x0, (size_t)in_stride, g.roi_row, (size_t)g.rh, hipMemcpyHostToDevice, s);
        if (e != hipSuccess || !g.uv_rows) return e;
        return hipMemcpy2DAsync(d_dst + g.raw.uv_offset, g.roi_row, frame + ((size_t)g.h + (size_t)(g.ry >> 1)) * in_stride + x0, (size_t)in_stride, g.roi_row,
                                (size_t)g.uv_rows, hipMemcpyHostToDevice, s);
    }
    return hipMemcpy2DAsync(d_dst, g.roi_row, frame + (size_t)g.ry * in_stride + (size_t)g.rx * g.channels, (size_t)in_stride, g.roi_row, (size_t)g.rh,
                            hipMemcpyHostToDevice, s);
}
static lvm_params chain_params(const lvm_params& p, const lvm_preprocess_params& pp) {
    lvm_params mp = p;
    mp.preprocess_key = preprocess_key_of(pp);
    return mp;
}

// The front end the chain and export entry points share: n source frames of one geometry staged in front of the magnifier.  stage_plan checks the
// frame and works the geometry out (no HIP call); begin() orders the call behind the previous one, waits for the context's stream and sizes the
// staging buffers; then frame k is uploaded (or decoded into place), preprocessed, and seen(k) / tap(k) are views of what the magnifier reads and
// of runChainOnce's `original`.
struct Staged {
    Ctx* c; lvm_preprocess_params pp; ChainGeom g; int n; ptrdiff_t in_stride;
    // the pane Exporter::compose labels "Original" is runChainOnce's tap (ChainGeom::gray): kept in d_pre_tap when the caller wants it
    bool gray_tap;
    // where stage 1 leaves frame k in d_pre_in: the cropped copy (host frames), or -- `decoded` -- the ROI inside the whole decoded frame (JPEG frames)
    size_t src_off, src_row, src_fbytes;
    const char* error;              // of stage_plan; null: fine

    lvm::Image src(int k) const { return {c->d_pre_in + src_off + (size_t)k * src_fbytes, g.rw, g.rh, g.channels, (ptrdiff_t)src_row, (ptrdiff_t)src_fbytes}; }
    // what the magnifier sees: the preprocessed frame, or the staged one itself where there is nothing to do (ChainGeom::identity)
    lvm::ImageOut pre(int k) const { return {c->d_pre_out + (size_t)k * g.out_bytes, g.ow, g.oh, g.och, (ptrdiff_t)g.out_row, (ptrdiff_t)g.out_bytes}; }
    lvm::Image seen(int k) const { return g.identity ? src(k) : (lvm::Image)pre(k); }
    lvm::ImageOut out(int k) const { return {c->d_chain_out + (size_t)k * g.out_bytes, g.ow, g.oh, g.och, (ptrdiff_t)g.out_row, (ptrdiff_t)g.out_bytes}; }
    // the colour frame in front of GrayscaleProcessor (ChainBuilder.cpp:25); without a gray stage in between the tap IS the frame the magnifier sees
    lvm::ImageOut own_tap(int k) const {
        if (!gray_tap) return lvm::ImageOut();
        return {c->d_pre_tap + (size_t)k * g.tap_bytes, g.ow, g.oh, 3, (ptrdiff_t)g.tap_row, (ptrdiff_t)g.tap_bytes};
    }
    lvm::Image tap(int k) const { return gray_tap ? (lvm::Image)own_tap(k) : seen(k); }

    int begin(hipStream_t s) const {
        { const int orc = lvm::order_after_previous(c, s); if (orc != LVM_OK) return orc; }
        LVM_HIP_TRY(c, hipStreamSynchronize(s));      // staging buffers may be replaced below
        int rc = c->d_pre_in.reserve(c, src_fbytes * n);
        if (rc == LVM_OK) rc = c->d_pre_out.reserve(c, g.out_bytes * n);
        if (rc == LVM_OK) rc = c->d_chain_out.reserve(c, g.out_bytes * n);
        if (rc == LVM_OK && gray_tap) rc = c->d_pre_tap.reserve(c, g.tap_bytes * n);
        return rc;
    }
    // only the ROI rows cross PCIe (the crop is the pitch of the 2-D copy)
    hipError_t upload(int k, const uint8_t* frame, hipStream_t s) const { return chain_upload(g, c->d_pre_in + (size_t)k * g.roi_bytes, frame, in_stride, s); }
    // Preprocess + Grayscale of the staged frames k .. k + nstreams - 1 (one launch: the context's streams are its z dimension), the tap to `to`
    int preprocess(int k, hipStream_t s, const lvm::ImageOut& to) const {
        if (g.identity) return LVM_OK;
        return lvm::preprocess_device(c, pp, src(k), pre(k), s, to, g.fmt != LVM_PIX_BGR ? &g.raw : nullptr);
    }
};
static Staged stage_plan(Ctx* c, const lvm_preprocess_params& pp, int fmt, int w, int h, int channels, ptrdiff_t in_stride, int n_frames, bool want_tap, bool decoded = false) {
    Staged st{};
    st.c = c; st.n = n_frames; st.in_stride = in_stride;
    st.error = lvm::source_frame_error(fmt, w, h, channels, in_stride);
    if (st.error) return st;
    st.g = chain_geometry(pp, w, h, channels, fmt);
    st.pp = pp; st.pp.roi_enabled = 0;             // the staged frames are cropped already (by the upload, or as a view into a decoded frame)
    st.gray_tap = want_tap && st.g.gray;
    st.src_row = st.g.roi_row; st.src_fbytes = st.g.roi_bytes;
    if (decoded) {
        st.src_row = (size_t)w * channels; st.src_fbytes = st.src_row * h;
        st.src_off = (size_t)st.g.ry * st.src_row + (size_t)st.g.rx * channels;
    }
    return st;
}
// the magnifier's arguments for staged frame k (and the context's further streams behind it), writing to `out`
static lvm::FrameIO stage_io(const Staged& st, int k, const lvm::ImageOut& out) {
    const lvm::Image in = st.seen(k);
    return lvm::FrameIO{in.p, in.stride, in.sstride, out.p, out.stride, out.sstride, in.w, in.h, in.cn};
}
static hipError_t frame_copy(uint8_t* dst, ptrdiff_t dst_stride, const lvm::Image& f, hipMemcpyKind kind, hipStream_t s) {
    return hipMemcpy2DAsync(dst, (size_t)dst_stride, f.p, (size_t)f.stride, (size_t)f.w * f.cn, (size_t)f.h, kind, s);
}

int lvm_chain_process_batch(lvm_ctx* c, const lvm_preprocess_params* pp, const lvm_params* p, const uint8_t* const* in, int w, int h,
                            int channels, ptrdiff_t in_stride, uint8_t* const* out, ptrdiff_t out_stride, int* produced) {
    return lvm_chain_process_batch_ex(c, pp, p, in, w, h, channels, in_stride, out, out_stride, nullptr, 0, produced);
}

int lvm_chain_process_batch_ex(lvm_ctx* c, const lvm_preprocess_params* pp, const lvm_params* p, const uint8_t* const* in, int w, int h,
                               int channels, ptrdiff_t in_stride, uint8_t* const* out, ptrdiff_t out_stride, uint8_t* const* pre_out,
                               ptrdiff_t pre_stride, int* produced) {
    if (!c || !pp || !p || !produced || !in || !out) return LVM_ERR_INVALID;
    *produced = 0;
    const int NS = c->nstreams;
    const Staged st = stage_plan(c, *pp, c->source_format, w, h, channels, in_stride, NS, pre_out != nullptr);
    if (st.error) { c->err = st.error; return LVM_ERR_INVALID; }
    for (int s = 0; s < NS; ++s) if (!in[s] || !out[s]) { c->err = "null frame pointer"; return LVM_ERR_INVALID; }
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    if (out_stride < (ptrdiff_t)st.g.out_row) { c->err = "output stride too small"; return LVM_ERR_INVALID; }
    hipStream_t s = c->own_stream;
    int rc = st.begin(s);
    if (rc != LVM_OK) return rc;
    for (int k = 0; k < NS; ++k) LVM_HIP_TRY(c, st.upload(k, in[k], s));
    rc = st.preprocess(0, s, st.own_tap(0));
    if (rc != LVM_OK) { (void)hipStreamSynchronize(s); return rc; }
    const lvm_params mp = chain_params(*p, *pp);
    const lvm::FrameIO io = stage_io(st, 0, st.out(0));
    rc = lvm::at_depth0(c, [&] { return lvm::process_device(c, &mp, io, s, produced); });
    if (rc != LVM_OK) { (void)hipStreamSynchronize(s); return rc; }
    for (int k = 0; k < NS; ++k)        // passthrough: the chain hands the magnifier's INPUT on (MagnificationProcessor.cpp:61)
        LVM_HIP_TRY(c, frame_copy(out[k], out_stride, *produced ? (lvm::Image)st.out(k) : st.seen(k), hipMemcpyDeviceToHost, s));
    if (pre_out) {     // the pre-magnification tap (runChainOnce's `original`, ChainBuilder.cpp:19-29): the display's left pane
        if (pre_stride < (ptrdiff_t)st.g.tap_row) { c->err = "pre_out stride too small"; (void)hipStreamSynchronize(s); return LVM_ERR_INVALID; }
        for (int k = 0; k < NS; ++k)
            if (pre_out[k]) LVM_HIP_TRY(c, frame_copy(pre_out[k], pre_stride, st.tap(k), hipMemcpyDeviceToHost, s));
    }
    LVM_HIP_TRY(c, hipStreamSynchronize(s));
    return LVM_OK;
}

// runChainOnce for the LIVE DISPLAY (display half): host frame in, both frames the display shows left in DEVICE
// memory -- see include/lvm_hip.h.  The reference publishes {processed, original} to the display's mailbox (ProcessingChain.cpp:46-49)
// and DisplayWidget::uploadFrame (ui/DisplayWidget.cpp:133-152) sends both to GL textures from HOST memory every frame; with the two
// destinations being mapped GL pixel-unpack buffers (host/HipDisplayPresenter.hpp) the frames never come back over PCIe.
int lvm_chain_present(lvm_ctx* c, const lvm_preprocess_params* pp, const lvm_params* p, const uint8_t* in, int w, int h, int channels,
                      ptrdiff_t in_stride, uint8_t* d_proc, ptrdiff_t proc_stride, uint8_t* d_orig, ptrdiff_t orig_stride, int* produced) {
    if (!c || !pp || !p || !produced || !in) return LVM_ERR_INVALID;
    *produced = 0;
    if (c->nstreams != 1) { c->err = "lvm_chain_present needs a 1-stream context"; return LVM_ERR_INVALID; }
    const Staged st = stage_plan(c, *pp, c->source_format, w, h, channels, in_stride, 1, false);      // (no tap of the context's: see below)
    if (st.error) { c->err = st.error; return LVM_ERR_INVALID; }
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    const ChainGeom& g = st.g;
    if (d_proc && proc_stride < (ptrdiff_t)g.out_row) { c->err = "proc stride too small"; return LVM_ERR_INVALID; }
    if (d_orig && orig_stride < (ptrdiff_t)g.tap_row) { c->err = "orig stride too small"; return LVM_ERR_INVALID; }      // (the tap keeps the source's channel count)
    hipStream_t s = c->own_stream;
    int rc = st.begin(s);
    if (rc != LVM_OK) return rc;
    LVM_HIP_TRY(c, st.upload(0, in, s));
    // special case 1: with grayscale on a BGR source the kernel writes the colour tap straight into the caller's `original` buffer
    const bool gray_tap = d_orig && g.gray;
    rc = st.preprocess(0, s, gray_tap ? lvm::ImageOut{d_orig, g.ow, g.oh, 3, orig_stride, orig_stride * g.oh} : lvm::ImageOut());
    if (rc != LVM_OK) { (void)hipStreamSynchronize(s); return rc; }
    if (d_orig && !gray_tap)        // no gray stage in between: the tap IS the frame the magnifier sees
        LVM_HIP_TRY(c, frame_copy(d_orig, orig_stride, st.seen(0), hipMemcpyDeviceToDevice, s));
    const lvm_params mp = chain_params(*p, *pp);
    // special case 2: the last kernel writes the processed frame straight into the caller's buffer
    const lvm::FrameIO io = stage_io(st, 0, d_proc ? lvm::ImageOut{d_proc, g.ow, g.oh, g.och, proc_stride, proc_stride * g.oh} : st.out(0));
    rc = lvm::at_depth0(c, [&] { return lvm::process_device(c, &mp, io, s, produced); });
    if (rc != LVM_OK) { (void)hipStreamSynchronize(s); return rc; }
    if (!*produced && d_proc)       // passthrough: the chain hands the magnifier's INPUT on (MagnificationProcessor.cpp:61) -- that is what the display shows
        LVM_HIP_TRY(c, frame_copy(d_proc, proc_stride, st.seen(0), hipMemcpyDeviceToDevice, s));
    LVM_HIP_TRY(c, hipStreamSynchronize(s));
    return LVM_OK;
}

int lvm_export_geometry(const lvm_preprocess_params* pp, int split, int w, int h, int channels, int* cw, int* ch) {
    if (!pp || w <= 0 || h <= 0 || (channels != 1 && channels != 3) || !cw || !ch) return LVM_ERR_INVALID;
    if (split < LVM_SPLIT_NONE || split > LVM_SPLIT_TOP_BOTTOM) return LVM_ERR_INVALID;
    const ChainGeom g = chain_geometry(*pp, w, h, channels);
    int pw, ph;
    (void)lvm::compose_geometry(split, g.ow, g.oh, g.ow, g.oh, &pw, &ph, cw, ch);      // 0 x 0 where Exporter::compose returns an empty Mat
    return LVM_OK;
}

// Exporter::run's loop body for a batch of host frames (export/Exporter.cpp:216-259); see include/lvm_hip.h.
// Round 5: a three-stage pipeline over three queues -- the frames go through in sub-batches of LVM_EXPORT_CHUNK (2) frames, and while
// sub-batch k is preprocessed / magnified / composed on the context's stream, sub-batch k + 1 is uploaded on `up_stream` and the
// canvases of sub-batch k - 1 are downloaded on `down_stream`: PCIe runs in both directions at once (measured on this box,
// tools/ubench_pcie.hip: 52-57 GB/s one way, 90-97 GB/s with both directions busy).  The magnifier still sees every frame in order
// with the state of its predecessor; a sub-batch is one temporal batch (lvm_process_device_frames), so the frames are the ones a
// single 32-frame batch -- or 32 per-frame calls -- gives.
// The three public entry points are one loop (export_run) between a SOURCE -- host frames, or JPEG frames decoded on the device by the upload
// queue, the ROI a view into the decoded frame instead of the pitch of a copy -- and a SINK: canvases to the host as BGR or as 4:2:0 surfaces, or
// the canvases encoded on the device (Motion-JPEG).  Each is a small tagged struct with its few functions below; a new source or sink is one more
// tag and one more case in each of them.
struct ExportSource {
    enum Kind { HostFrames, Jpeg } kind;
    const uint8_t* const* frames; ptrdiff_t in_stride;      // HostFrames
    const uint8_t* jpegs; const size_t* offsets;            // Jpeg: all frames of the call
};
struct ExportSink {
    enum Kind { Bgr, Yuv, Mjpeg } kind;
    uint8_t* const* canvases; ptrdiff_t canvas_stride;      // Bgr, Yuv: one host canvas per frame
    int quality; uint8_t* out; size_t capacity; size_t* offsets;   // Mjpeg
};

// Everything an export call decides before it touches the device: the staged front end, the canvas and its layouts, how the canvases are made,
// the sub-batches.
struct ExportPlan {
    Staged st; int split, n;
    int cw, chh; size_t can_row, can_bytes;         // the BGR canvas, rows packed on the device
    int cfmt; lvm::CanvasLayout host_l, dev_l;      // canvases as 4:2:0 surfaces: the caller's layout, and the device's -- rows packed, the same plane order
    bool fused;                                     // the conversion reads the panes, the BGR canvas is never written
    int chunk, nchunks;
    lvm::ImageOut canvas(int k) const { return {st.c->d_canvas + (size_t)k * can_bytes, cw, chh, 3, (ptrdiff_t)can_row, (ptrdiff_t)can_bytes}; }
    lvm::ImageOut surface(int k) const { return {st.c->d_canvas_yuv + (size_t)k * dev_l.bytes, cw, chh, 1, (ptrdiff_t)cw, (ptrdiff_t)dev_l.bytes}; }
};
static int export_plan(lvm_ctx* c, const lvm_preprocess_params* pp, int split, int n_frames, int w, int h, int channels, const ExportSource& src, const ExportSink& sink,
                       int* produced, ExportPlan* out) {
    const bool js = src.kind == ExportSource::Jpeg, mj = sink.kind == ExportSink::Mjpeg;
    if (mj && (!sink.out || !sink.offsets)) return LVM_ERR_INVALID;
    if (js && (!src.jpegs || !src.offsets || channels != 3)) return LVM_ERR_INVALID;
    if (c->nstreams != 1) { c->err = "lvm_export_frames needs a 1-stream context"; return LVM_ERR_INVALID; }
    ExportPlan& P = *out;
    P.split = split; P.n = n_frames;
    // (JPEG frames decode to BGR: lvm_export_mjpeg_frames does not take part in lvm_set_source_format)
    P.st = stage_plan(c, *pp, js ? LVM_PIX_BGR : c->source_format, w, h, channels, js ? (ptrdiff_t)w * 3 : src.in_stride, n_frames, split != LVM_SPLIT_NONE, js);
    if (P.st.error) { c->err = P.st.error; return LVM_ERR_INVALID; }
    for (int k = 0; k < n_frames; ++k) { produced[k] = 0; if ((!js && !src.frames[k]) || (!mj && !sink.canvases[k])) { c->err = "null frame pointer"; return LVM_ERR_INVALID; } }
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    const ChainGeom& g = P.st.g;
    int pw, ph;
    if (split < LVM_SPLIT_NONE || split > LVM_SPLIT_TOP_BOTTOM) { c->err = "invalid split mode"; return LVM_ERR_INVALID; }
    if (!lvm::compose_geometry(split, g.ow, g.oh, g.ow, g.oh, &pw, &ph, &P.cw, &P.chh) || P.cw <= 0 || P.chh <= 0) {
        c->err = "lvm_export_frames: empty canvas (Exporter::compose returns an empty Mat for this geometry)"; return LVM_ERR_INVALID;
    }
    // canvases as 4:2:0 surfaces (lvm_set_canvas_format; the JPEG sink encodes BGR canvases and does not take part)
    P.cfmt = sink.kind == ExportSink::Yuv ? c->canvas_format : LVM_PIX_BGR;
    if (P.cfmt != LVM_PIX_BGR) {
        if (const char* why = lvm::canvas_layout(P.cfmt, P.cw, P.chh, sink.canvas_stride, &P.host_l)) { c->err = why; return LVM_ERR_INVALID; }
        (void)lvm::canvas_layout(P.cfmt, P.cw, P.chh, (ptrdiff_t)P.cw, &P.dev_l);
    } else if (!mj && sink.canvas_stride < (ptrdiff_t)P.cw * 3) { c->err = "canvas stride too small"; return LVM_ERR_INVALID; }
    P.can_row = (size_t)P.cw * 3; P.can_bytes = P.can_row * P.chh;
    // without labels the conversion reads the panes and the BGR canvas is never written; with labels: compose, overlay, convert (the definition's order)
    P.fused = P.cfmt != LVM_PIX_BGR && c->overlay_n == 0;
    if (P.fused) lvm::env_switch("LVM_CANVAS_FUSED", P.fused);
    P.chunk = mj ? 4 : 2;        // (JPEG frames: nothing large to download, the encoder's launches want more frames each)
    lvm::env_switch(mj ? "LVM_EXPORT_MJPEG_CHUNK" : "LVM_EXPORT_CHUNK", P.chunk, [](int v) { return v >= 1; });
    P.nchunks = (n_frames + P.chunk - 1) / P.chunk;
    return LVM_OK;
}

// the staging buffers behind the front end's, the two side queues and an event pair per sub-batch
static int export_reserve(Ctx* c, const ExportPlan& P) {
    int rc = LVM_OK;
    if (!P.fused) rc = c->d_canvas.reserve(c, P.can_bytes * P.n);
    if (rc == LVM_OK && P.cfmt != LVM_PIX_BGR) rc = c->d_canvas_yuv.reserve(c, P.dev_l.bytes * P.n);
    if (rc != LVM_OK) return rc;
    if (!c->up_stream) LVM_HIP_TRY(c, hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking));
    if (!c->down_stream) LVM_HIP_TRY(c, hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking));
    for (auto* evs : {&c->ev_up, &c->ev_done})
        while ((int)evs->size() < P.nchunks) { hipEvent_t e = nullptr; LVM_HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming)); evs->push_back(e); }
    return LVM_OK;
}

// ---- the source: sub-batch q arrives on up_stream -----------------------------------------------------------------------------------------
static int source_begin(const ExportPlan& P, const ExportSource& src, int w, int h) {
    if (src.kind != ExportSource::Jpeg) return LVM_OK;
    // JPEG frames: only the compressed bytes cross PCIe, and ALL frames of the call are decoded by one set of launches -- Huffman decoding
    // is serial inside a restart interval (a lane each), its time is a latency that does not grow with the number of frames
    Ctx* c = P.st.c;
    const int rc = lvm::mjpeg_decode_begin(c, src.jpegs, src.offsets, P.n, w, h, c->up_stream);
    if (rc != LVM_OK) return rc;
    return lvm::mjpeg_decode_enqueue(c, 0, P.n, c->d_pre_in, (ptrdiff_t)P.st.src_row, (ptrdiff_t)P.st.src_fbytes, c->up_stream);
}
static int source_upload(const ExportPlan& P, const ExportSource& src, int f0, int nf) {
    if (src.kind == ExportSource::Jpeg) return LVM_OK;                  // (decoded already, or on its way: source_begin)
    for (int k = f0; k < f0 + nf; ++k) LVM_HIP_TRY(P.st.c, P.st.upload(k, src.frames[k], P.st.c->up_stream));
    return LVM_OK;
}
static int source_finish(const ExportPlan& P, const ExportSource& src) {       // a malformed input frame fails the call
    return src.kind == ExportSource::Jpeg ? lvm::mjpeg_decode_finish(P.st.c, P.st.c->up_stream) : LVM_OK;
}

// ---- the middle, on the context's stream: Preprocess + Grayscale, the magnifier as one temporal batch, the canvases -------------------------
static int export_canvases(const ExportPlan& P, int f0, int nf, const int* produced, hipStream_t s) {
    Ctx* c = P.st.c;
    for (int k = f0; k < f0 + nf; ++k) {
        const lvm::Image seen = P.st.seen(k);                                          // what the magnifier saw
        const lvm::Image proc = produced[k] ? (lvm::Image)P.st.out(k) : seen;          // MagnificationProcessor.cpp:61
        const lvm::Image orig = P.st.tap(k);                                           // ChainBuilder.cpp:25
        const int rc = P.fused ? lvm::canvas_yuv_fused(c, P.cfmt, P.split, orig, proc, P.surface(k), s) : lvm::compose_device(c, P.split, orig, proc, P.canvas(k), s);
        if (rc != LVM_OK) return rc;
    }
    if (P.fused) return LVM_OK;
    // drawLabel on every canvas of the sub-batch (Exporter.cpp:74-77, :82-85), from the tables of lvm_export_set_overlay
    const int rc = lvm::overlay_device(c, P.canvas(f0), nf, s);
    if (rc != LVM_OK || P.cfmt == LVM_PIX_BGR) return rc;
    return lvm::canvas_yuv_device(c, P.cfmt, P.canvas(f0), nf, P.surface(f0), s);       // ... and the sub-batch's canvases become surfaces in one launch
}
static int export_middle(const ExportPlan& P, const lvm_params& mp, int f0, int nf, int* produced, hipStream_t s) {
    Ctx* c = P.st.c;
    for (int k = f0; k < f0 + nf; ++k) {                         // (stateless: a frame of the batch is one more "stream" of a 1-stream context)
        const int rc = P.st.preprocess(k, s, P.st.own_tap(k));
        if (rc != LVM_OK) return rc;
    }
    const lvm::Image in = P.st.seen(f0);
    const lvm::ImageOut out = P.st.out(f0);
    const int rc = lvm::at_depth0(c, [&] {
        return lvm_process_device_frames(static_cast<lvm_ctx*>(c), &mp, nf, in.p, in.w, in.h, in.cn, in.stride, in.sstride, in.sstride, out.p, out.stride, out.sstride, out.sstride,
                                         produced + f0, s);
    });
    return rc != LVM_OK ? rc : export_canvases(P, f0, nf, produced, s);
}

// ---- the sink: takes sub-batch q on down_stream ------------------------------------------------------------------------------------------------
static int sink_begin(const ExportPlan& P, const ExportSink& sink) {
    if (sink.kind != ExportSink::Mjpeg) return LVM_OK;
    return lvm::mjpeg_begin(P.st.c, P.cw, P.chh, sink.quality, P.chunk < P.n ? P.chunk : P.n, (size_t)P.n, sink.capacity, P.st.c->down_stream);
}
// 1.5 B / pixel.  3h/2 rows of cw bytes in one copy where the chroma rows follow the Y rows at the Y stride (NV12 / NV21; the planar formats with
// packed rows: two chroma rows are one row of cw bytes); otherwise Y, then the two chroma planes
static int surface_download(const ExportPlan& P, const ExportSink& sink, int k, hipStream_t s) {
    Ctx* c = P.st.c;
    const uint8_t* d = P.surface(k).p;
    uint8_t* to = sink.canvases[k];
    const size_t cw = (size_t)P.cw, chh = (size_t)P.chh;
    const bool one = P.dev_l.plane2 == 0 || sink.canvas_stride == (ptrdiff_t)cw;
    LVM_HIP_TRY(c, hipMemcpy2DAsync(to, (size_t)sink.canvas_stride, d, cw, cw, one ? chh + chh / 2 : chh, hipMemcpyDeviceToHost, s));
    if (one) return LVM_OK;
    for (const auto& pl : {std::make_pair(P.host_l.plane1, P.dev_l.plane1), std::make_pair(P.host_l.plane2, P.dev_l.plane2)})
        LVM_HIP_TRY(c, hipMemcpy2DAsync(to + pl.first, (size_t)P.host_l.cstride, d + pl.second, cw / 2, cw / 2, chh / 2, hipMemcpyDeviceToHost, s));
    return LVM_OK;
}
static int sink_take(const ExportPlan& P, const ExportSink& sink, int f0, int nf) {
    Ctx* c = P.st.c;
    if (sink.kind == ExportSink::Mjpeg) {
        // stays on the device (down_stream, next to the magnifier of the following sub-batch): the canvases become JPEG frames behind the
        // earlier ones; the frames of sub-batch q - 2 come down meanwhile (the encoder's rule)
        const lvm::Image can = P.canvas(f0);
        return lvm::mjpeg_encode_device(c, can.p, can.stride, can.sstride, nf, sink.out, c->down_stream);
    }
    for (int k = f0; k < f0 + nf; ++k) {
        if (sink.kind == ExportSink::Yuv) { const int rc = surface_download(P, sink, k, c->down_stream); if (rc != LVM_OK) return rc; }
        else LVM_HIP_TRY(c, frame_copy(sink.canvases[k], sink.canvas_stride, P.canvas(k), hipMemcpyDeviceToHost, c->down_stream));
    }
    return LVM_OK;
}
// the end of the call: everything has been enqueued.  Motion-JPEG: waits for the encoder, then the compressed bytes come down in one copy
static int sink_finish(const ExportPlan& P, const ExportSink& sink, hipStream_t s) {
    Ctx* c = P.st.c;
    if (sink.kind == ExportSink::Mjpeg) {
        const int rc = lvm::mjpeg_finish(c, sink.out, sink.offsets, c->down_stream);
        (void)hipStreamSynchronize(s);
        (void)hipStreamSynchronize(c->up_stream);
        return rc;
    }
    LVM_HIP_TRY(c, hipStreamSynchronize(c->down_stream));     // (the last canvases: everything on `s` and `up_stream` precedes them)
    LVM_HIP_TRY(c, hipStreamSynchronize(s));
    return LVM_OK;
}

// A failed return of the loop below leaves nothing running: it waits for the three queues and for the downloads the encoder has queued.
struct ExportGuard {
    Ctx* c; bool mj; bool armed = true;
    ~ExportGuard() {
        if (!armed) return;
        (void)hipStreamSynchronize(c->up_stream); (void)hipStreamSynchronize(c->own_stream); (void)hipStreamSynchronize(c->down_stream);
        if (mj) lvm::mjpeg_abort(c);
    }
};

static int export_run(lvm_ctx* c, const lvm_preprocess_params* pp, const lvm_params* p, int split, int n_frames, int w, int h, int channels, const ExportSource& src,
                      const ExportSink& asked, int* produced) {
    if (!c || !pp || !p || !produced || n_frames < 1) return LVM_ERR_INVALID;
    // the sink is chosen here, once: the wrapper asks for host canvases, lvm_set_canvas_format says of which kind
    ExportSink chosen = asked;
    if (asked.kind == ExportSink::Bgr && c->canvas_format != LVM_PIX_BGR) chosen.kind = ExportSink::Yuv;
    const ExportSink& sink = chosen;
    if ((src.kind == ExportSource::HostFrames && !src.frames) || (sink.kind != ExportSink::Mjpeg && !sink.canvases)) return LVM_ERR_INVALID;
    ExportPlan P{};
    int rc = export_plan(c, pp, split, n_frames, w, h, channels, src, sink, produced, &P);
    if (rc != LVM_OK) return rc;
    hipStream_t s = c->own_stream;
    rc = P.st.begin(s);
    if (rc == LVM_OK) rc = export_reserve(c, P);
    if (rc == LVM_OK) rc = sink_begin(P, sink);
    if (rc != LVM_OK) return rc;
    ExportGuard guard{c, sink.kind == ExportSink::Mjpeg};
    const lvm_params mp = chain_params(*p, *pp);
    rc = source_begin(P, src, w, h);
    for (int q = 0; q < P.nchunks && rc == LVM_OK; ++q) {
        const int f0 = q * P.chunk, nf = (f0 + P.chunk <= n_frames) ? P.chunk : n_frames - f0;
        rc = source_upload(P, src, f0, nf);                                     // stage 1 (up_stream)
        if (rc != LVM_OK) break;
        LVM_HIP_TRY(c, hipEventRecord(c->ev_up[q], c->up_stream));
        LVM_HIP_TRY(c, hipStreamWaitEvent(s, c->ev_up[q], 0));
        rc = export_middle(P, mp, f0, nf, produced, s);                         // stage 2 (the context's stream)
        if (rc != LVM_OK) break;
        LVM_HIP_TRY(c, hipEventRecord(c->ev_done[q], s));
        LVM_HIP_TRY(c, hipStreamWaitEvent(c->down_stream, c->ev_done[q], 0));
        rc = sink_take(P, sink, f0, nf);                                        // stage 3 (down_stream)
    }
    if (rc != LVM_OK) return rc;
    lvm::mark_enqueued(c, s);
    const int drc = source_finish(P, src);
    rc = sink_finish(P, sink, s);
    if (drc == LVM_OK && rc == LVM_OK) guard.armed = false;
    return drc != LVM_OK ? drc : rc;
}

int lvm_export_frames(lvm_ctx* c, const lvm_preprocess_params* pp, const lvm_params* p, int split, int n_frames,
                      const uint8_t* const* frames, int w, int h, int channels, ptrdiff_t in_stride, uint8_t* const* canvases,
                      ptrdiff_t canvas_stride, int* produced) {
    return export_run(c, pp, p, split, n_frames, w, h, channels, ExportSource{ExportSource::HostFrames, frames, in_stride}, ExportSink{ExportSink::Bgr, canvases, canvas_stride}, produced);
}

int lvm_export_frames_mjpeg(lvm_ctx* c, const lvm_preprocess_params* pp, const lvm_params* p, int split, int n_frames,
                            const uint8_t* const* frames, int w, int h, int channels, ptrdiff_t in_stride, int quality,
                            uint8_t* out, size_t out_capacity, size_t* offsets, int* produced) {
    return export_run(c, pp, p, split, n_frames, w, h, channels, ExportSource{ExportSource::HostFrames, frames, in_stride}, ExportSink{ExportSink::Mjpeg, nullptr, 0, quality, out, out_capacity, offsets}, produced);
}

int lvm_mjpeg_decode_device(lvm_ctx* c, const uint8_t* jpegs, const size_t* offsets, int n_frames, int w, int h, uint8_t* d_bgr, ptrdiff_t stride,
                            ptrdiff_t frame_stride) {
    if (!c || !jpegs || !offsets || !d_bgr || n_frames < 1) return LVM_ERR_INVALID;
    if (stride < (ptrdiff_t)w * 3 || (n_frames > 1 && frame_stride < (ptrdiff_t)h * stride)) { c->err = "bad frame arguments"; return LVM_ERR_INVALID; }
    // by hand: a failed decode has waited for what it enqueued (it reads the decoder's error flags), so only a successful one is marked
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    int rc = lvm::order_after_previous(c, c->own_stream);
    if (rc != LVM_OK) return rc;
    rc = lvm::mjpeg_decode_device(c, jpegs, offsets, n_frames, w, h, d_bgr, stride, frame_stride, c->own_stream);
    if (rc == LVM_OK) lvm::mark_enqueued(c, c->own_stream);
    return rc;
}

int lvm_export_mjpeg_frames(lvm_ctx* c, const lvm_preprocess_params* pp, const lvm_params* p, int split, int n_frames, const uint8_t* jpegs,
                            const size_t* in_offsets, int w, int h, int quality, uint8_t* out, size_t out_capacity, size_t* offsets, int* produced) {
    return export_run(c, pp, p, split, n_frames, w, h, 3, ExportSource{ExportSource::Jpeg, nullptr, 0, jpegs, in_offsets}, ExportSink{ExportSink::Mjpeg, nullptr, 0, quality, out, out_capacity, offsets}, produced);
}

int lvm_mjpeg_set_restart_interval(lvm_ctx* c, int mcus) {
    if (!c || mcus < 0) return LVM_ERR_INVALID;
    lvm::mjpeg_set_restart(c, mcus);
    return LVM_OK;
}

int lvm_mjpeg_set_decoder(lvm_ctx* c, int kind) {
    if (!c) return LVM_ERR_INVALID;
    if (kind != LVM_MJPEG_DECODER_REPLICATE && kind != LVM_MJPEG_DECODER_LIBJPEG) {
        c->err = "lvm_mjpeg_set_decoder: kind must be LVM_MJPEG_DECODER_REPLICATE (0) or LVM_MJPEG_DECODER_LIBJPEG (1)";
        return LVM_ERR_INVALID;
    }
    c->mjpeg_decoder = kind;
    return LVM_OK;
}

int lvm_mjpeg_set_samplings(lvm_ctx* c, unsigned mask) {
    if (!c) return LVM_ERR_INVALID;
    if (mask == 0 || (mask & ~(unsigned)LVM_MJPEG_SAMPLING_ALL)) {
        c->err = "lvm_mjpeg_set_samplings: mask must be a non-empty combination of LVM_MJPEG_SAMPLING_420 (1), _422 (2), _444 (4), _GRAY (8)";
        return LVM_ERR_INVALID;
    }
    c->mjpeg_samplings = mask;
    return LVM_OK;
}

// Kept by lvm_reset (a property of the host's OpenCV, not of the clip); read by riesz.hip at every launch, so it holds from the next frame
// on and leaves the temporal state alone.
int lvm_set_opencv_build(lvm_ctx* c, unsigned mask) {
    if (!c) return LVM_ERR_INVALID;
    if (mask & ~(unsigned)LVM_CV_ALL) {
        c->err = "lvm_set_opencv_build: mask must be a combination of LVM_CV_FILTER_UNFUSED (1), LVM_CV_FILTER_DFT (2), LVM_CV_MUL_F32 (4)";
        return LVM_ERR_INVALID;
    }
    c->opencv_build = mask;
    return LVM_OK;
}
int lvm_get_opencv_build(lvm_ctx* c, unsigned* mask) {
    if (!c || !mask) return LVM_ERR_INVALID;
    *mask = c->opencv_build;
    return LVM_OK;
}

// Phase mode on gray frames, an extension beyond the reference (include/lvm_hip.h).  Kept by lvm_reset.  Whether a gray Phase key has a state at
// all depends on it, so a change under such a key is a structural change (process_device's rule: flush, synchronise, drop; the tracker is
// disarmed, the next frame is a first frame); under any other key the value is only stored.
int lvm_set_phase_on_gray(lvm_ctx* c, int on) {
    if (!c) return LVM_ERR_INVALID;
    if (on != 0 && on != 1) { c->err = "lvm_set_phase_on_gray: the value must be 0 or 1"; return LVM_ERR_INVALID; }
    if ((on != 0) == c->phase_on_gray) return LVM_OK;
    if (c->tracked.mode == LVM_MODE_PHASE && c->tracked.channels == 1) {
        LVM_HIP_TRY(c, hipSetDevice(c->device));
        if (c->state) (void)c->state->flush(c, c->own_stream);
        LVM_HIP_TRY(c, hipStreamSynchronize(c->own_stream));
        lvm::sync_streams(c);
        lvm::drop_state(c); lvm::tracker_disable(c);
    }
    c->phase_on_gray = on != 0;
    return LVM_OK;
}
int lvm_get_phase_on_gray(lvm_ctx* c, int* on) {
    if (!c || !on) return LVM_ERR_INVALID;
    *on = c->phase_on_gray ? 1 : 0;
    return LVM_OK;
}

// Raw camera formats in front of the chain, an extension beyond the reference (include/lvm_hip.h).  Only stored: the surfaces that take frames read
// it when they are called, and the magnifier sees the same BGR / gray frames either way.  Kept by lvm_reset.
int lvm_set_source_format(lvm_ctx* c, int fmt) {
    if (!c) return LVM_ERR_INVALID;
    if (fmt < LVM_PIX_BGR || fmt > LVM_PIX_NV21) {
        c->err = "lvm_set_source_format: the format must be LVM_PIX_BGR (0), _YUYV (1), _UYVY (2), _YVYU (3), _NV12 (4) or _NV21 (5)";
        return LVM_ERR_INVALID;
    }
    c->source_format = fmt;
    return LVM_OK;
}
int lvm_get_source_format(lvm_ctx* c, int* fmt) {
    if (!c || !fmt) return LVM_ERR_INVALID;
    *fmt = c->source_format;
    return LVM_OK;
}

// Canvases as 4:2:0 surfaces, an extension beyond the reference (include/lvm_hip.h).  Only stored: lvm_export_frames reads it when it is called;
// the magnifier, the tracked key and the overlay tables never see it.  Kept by lvm_reset.
int lvm_set_canvas_format(lvm_ctx* c, int fmt) {
    if (!c) return LVM_ERR_INVALID;
    if (fmt != LVM_PIX_BGR && fmt != LVM_PIX_NV12 && fmt != LVM_PIX_NV21 && fmt != LVM_PIX_I420 && fmt != LVM_PIX_YV12) {
        c->err = "lvm_set_canvas_format: the format must be LVM_PIX_BGR (0), _NV12 (4), _NV21 (5), _I420 (6) or _YV12 (7)";
        return LVM_ERR_INVALID;
    }
    c->canvas_format = fmt;
    return LVM_OK;
}
int lvm_get_canvas_format(lvm_ctx* c, int* fmt) {
    if (!c || !fmt) return LVM_ERR_INVALID;
    *fmt = c->canvas_format;
    return LVM_OK;
}

int lvm_canvas_layout(int fmt, int canvas_w, int canvas_h, ptrdiff_t canvas_stride, size_t* bytes, size_t* plane1_offset, size_t* plane2_offset,
                      ptrdiff_t* chroma_stride) {
    lvm::CanvasLayout L;
    if (lvm::canvas_layout(fmt, canvas_w, canvas_h, canvas_stride, &L)) return LVM_ERR_INVALID;
    if (bytes) *bytes = L.bytes;
    if (plane1_offset) *plane1_offset = L.plane1;
    if (plane2_offset) *plane2_offset = L.plane2;
    if (chroma_stride) *chroma_stride = L.cstride;
    return LVM_OK;
}

int lvm_canvas_convert_device(lvm_ctx* c, int fmt, const uint8_t* d_bgr, int w, int h, ptrdiff_t bgr_stride, ptrdiff_t bgr_frame_stride, int n_frames,
                              uint8_t* d_out, ptrdiff_t out_stride, ptrdiff_t out_frame_stride, void* hip_stream) {
    if (!c) return LVM_ERR_INVALID;
    const lvm::Image bgr{d_bgr, w, h, 3, bgr_stride, bgr_frame_stride};
    const lvm::ImageOut out{d_out, w, h, 1, out_stride, out_frame_stride};
    // validated first (no HIP call): a refused call enqueues nothing, not even the wait that orders it behind the previous one
    const int rc = lvm::canvas_yuv_device(c, fmt, bgr, n_frames, out, nullptr, true);
    if (rc != LVM_OK) return rc;
    return lvm::on_stream(c, hip_stream, [&](hipStream_t s) { return lvm::canvas_yuv_device(c, fmt, bgr, n_frames, out, s); });
}

size_t lvm_mjpeg_bound(int w, int h) { return (w < 1 || h < 1) ? 0 : lvm::mjpeg_bound(w, h); }

int lvm_mjpeg_encode_device(lvm_ctx* c, const uint8_t* d_bgr, int w, int h, ptrdiff_t stride, ptrdiff_t frame_stride, int n_frames, int quality,
                            uint8_t* out, size_t out_capacity, size_t* offsets) {
    if (!c || !d_bgr || !out || !offsets || n_frames < 1) return LVM_ERR_INVALID;
    if (stride < (ptrdiff_t)w * 3 || (n_frames > 1 && frame_stride < (ptrdiff_t)h * stride)) { c->err = "bad frame arguments"; return LVM_ERR_INVALID; }
    // by hand: the call is marked between the last encode and mjpeg_finish, which waits for it -- and only where every encode was enqueued (a failed
    // one has waited for the stream already)
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->own_stream;
    const int per = n_frames < 8 ? n_frames : 8;                 // scratch (coefficients, bit buffers) for eight frames at a time
    int rc = lvm::order_after_previous(c, s);
    if (rc != LVM_OK) return rc;
    rc = lvm::mjpeg_begin(c, w, h, quality, per, (size_t)n_frames, out_capacity, s);
    if (rc != LVM_OK) return rc;
    for (int f0 = 0; f0 < n_frames; f0 += per) {
        const int nf = f0 + per <= n_frames ? per : n_frames - f0;
        rc = lvm::mjpeg_encode_device(c, d_bgr + (size_t)f0 * frame_stride, stride, frame_stride, nf, out, s);
        if (rc != LVM_OK) { (void)hipStreamSynchronize(s); lvm::mjpeg_abort(c); return rc; }
    }
    lvm::mark_enqueued(c, s);
    return lvm::mjpeg_finish(c, out, offsets, s);
}

int lvm_chain_process(lvm_ctx* c, const lvm_preprocess_params* pp, const lvm_params* p, const uint8_t* in, int w, int h, int channels,
                      ptrdiff_t in_stride, uint8_t* out, ptrdiff_t out_stride, int* produced) {
    if (!c || !produced) return LVM_ERR_INVALID;
    *produced = 0;
    if (c->nstreams != 1) { c->err = "lvm_chain_process needs a 1-stream context"; return LVM_ERR_INVALID; }
    return lvm_chain_process_batch(c, pp, p, &in, w, h, channels, in_stride, &out, out_stride, produced);
}

// The device-visible alias of a page-locked host buffer (hipHostMalloc / hipHostRegister memory; lvm_host_alloc), or null.
static uint8_t* pinned_alias(const void* p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (a.type != hipMemoryTypeHost || !a.devicePointer) return nullptr;
    return static_cast<uint8_t*>(a.devicePointer);
}

// Round 5: frames in PAGE-LOCKED memory (lvm_host_alloc, i.e. a FramePool built on it) take no staging copy at all -- the first kernel
// reads the input straight over PCIe and the last kernel writes the output frame straight into the caller's buffer ("zero copy").
// Measured on this box (tools/ubench_pcie.hip): a kernel reads / writes a page-locked 1080p frame at 55 GB/s (112 us) while the DMA
// engine needs 120 us up and 166 us down for ONE frame in flight, and splitting a frame into row chunks to overlap copy and kernel
// costs ~20 us of queue hand-offs per chunk.  The input alias is used when exactly ONE kernel reads the u8 frame (Lab modes on BGR
// frames with the table flavour: the conversion kernel; everything downstream reads its integer planes); the colour mode and gray frames
// read their input again in the output pass and keep the upload.  The output alias is used in every mode: every mode's last kernel
// writes each output byte once.  Pageable frames take the copies as before.  LVM_ZERO_COPY=0 switches the aliases off (A/B, tests).
int lvm_process(lvm_ctx* c, const lvm_params* p, const uint8_t* in, int w, int h, int channels, ptrdiff_t in_stride,
                uint8_t* out, ptrdiff_t out_stride, int* produced) {
    if (!c || !p || !produced) return LVM_ERR_INVALID;
    *produced = 0;
    if (c->nstreams != 1) { c->err = "lvm_process needs a 1-stream context"; return LVM_ERR_INVALID; }
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    if (p->mode == LVM_MODE_NONE || !in || w <= 0 || h <= 0) {
        lvm::FrameIO io{nullptr, 0, 0, nullptr, 0, 0, w, h, channels};
        return lvm::process_device(c, p, io, c->own_stream, produced);
    }
    if (!out || lvm::source_frame_error(LVM_PIX_BGR, w, h, channels, in_stride) || out_stride < (ptrdiff_t)w * channels) { c->err = "bad frame arguments"; return LVM_ERR_INVALID; }
    const size_t row = (size_t)w * channels, bytes = row * h;
    static const bool zero_copy = [] { bool on = true; lvm::env_switch("LVM_ZERO_COPY", on); return on; }();
    const bool one_reader = channels == 3 && !c->lab_analytic && (p->mode == LVM_MODE_LAPLACE || p->mode == LVM_MODE_PHASE);
    const uint8_t* in_alias = (zero_copy && one_reader) ? pinned_alias(in) : nullptr;
    uint8_t* out_alias = zero_copy ? pinned_alias(out) : nullptr;
    if ((bytes > c->d_in.cap || bytes > c->d_out.cap) && (!in_alias || !out_alias)) {
        lvm::sync_streams(c);
        int rc = c->d_in.reserve(c, bytes);
        if (rc == LVM_OK) rc = c->d_out.reserve(c, bytes);
        if (rc != LVM_OK) return rc;
    }
    hipStream_t s = c->own_stream;
    if (!in_alias) LVM_HIP_TRY(c, hipMemcpy2DAsync(c->d_in, row, in, (size_t)in_stride, row, (size_t)h, hipMemcpyHostToDevice, s));
    lvm::FrameIO io{in_alias ? in_alias : c->d_in.p, in_alias ? in_stride : (ptrdiff_t)row, in_alias ? in_stride * h : (ptrdiff_t)bytes,
                    out_alias ? out_alias : c->d_out.p, out_alias ? out_stride : (ptrdiff_t)row, out_alias ? out_stride * h : (ptrdiff_t)bytes, w, h, channels};
    const int rc = lvm::at_depth0(c, [&] { return lvm::process_device(c, p, io, s, produced); });
    if (rc != LVM_OK) { (void)hipStreamSynchronize(s); return rc; }
    if (*produced && !out_alias)
        LVM_HIP_TRY(c, hipMemcpy2DAsync(out, (size_t)out_stride, c->d_out, row, row, (size_t)h, hipMemcpyDeviceToHost, s));
    LVM_HIP_TRY(c, hipStreamSynchronize(s));      // (polling an event instead measured the same 310 us per 1080p frame: nothing to gain)
    return LVM_OK;
}

// Page-locked host frames for the reference's FramePool (core/FramePool.cpp:29-36 allocates the pooled cv::Mat
// buffers the chain hands to process()): frames living in such memory cross PCIe by DMA at link speed in
// lvm_process / lvm_chain_process with no staging copy anywhere (hipMemcpy2DAsync sees the registration).
int lvm_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return LVM_ERR_INVALID;
    *out = nullptr;
    if (hipHostMalloc(out, bytes, 0) != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return LVM_ERR_OOM; }
    return LVM_OK;
}
void lvm_host_free(void* p) { if (p) (void)hipHostFree(p); }

int lvm_set_max_frames(lvm_ctx* c, int n_frames) {
    if (!c || n_frames < 1) return LVM_ERR_INVALID;
    c->max_frames = n_frames;
    return LVM_OK;
}

int lvm_synchronize(lvm_ctx* c) {
    if (!c) return LVM_ERR_INVALID;
    LVM_HIP_TRY(c, hipStreamSynchronize(c->own_stream));
    return LVM_OK;
}

const char* lvm_last_error(lvm_ctx* c) { return c ? c->err.c_str() : "null context"; }

int lvm_debug_keep_float(lvm_ctx* c, int on) { if (!c) return LVM_ERR_INVALID; c->keep_float = on != 0; return LVM_OK; }

int lvm_debug_exact_lab(lvm_ctx* c, int on) { if (!c) return LVM_ERR_INVALID; c->exact_lab = on != 0; return LVM_OK; }

int lvm_debug_sweep_u8_steps(lvm_ctx* c, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint32_t* first_bad_bits) {
    if (!c || !mismatches || (uint64_t)first_bits + count > (1ull << 32)) return LVM_ERR_INVALID;
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    unsigned long long bad = 0, fb = 0;
    const int rc = lvm::sweep_u8_steps(c, first_bits, count, &bad, &fb, c->own_stream);
    if (rc != LVM_OK) return rc;
    *mismatches = bad;
    if (first_bad_bits) *first_bad_bits = bad ? (uint32_t)fb : 0u;
    return LVM_OK;
}

int lvm_debug_clock_probe_start(lvm_ctx* c, double max_seconds) {
    if (!c) return LVM_ERR_INVALID;
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    return lvm::clock_probe_start(c, max_seconds);
}

int lvm_debug_clock_probe_stop(lvm_ctx* c, double* mhz, double* seconds) {
    if (!c) return LVM_ERR_INVALID;
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    return lvm::clock_probe_stop(c, mhz, seconds);
}

int lvm_debug_lab_analytic(lvm_ctx* c, int on) { if (!c) return LVM_ERR_INVALID; c->lab_analytic = on != 0; return LVM_OK; }

int lvm_debug_trig_eval(lvm_ctx* c, int fn, const float* d_x, float* d_y, size_t n, void* hip_stream) {
    if (!c || fn < 0 || fn > 2 || (n && (!d_x || !d_y))) return LVM_ERR_INVALID;
    return lvm::on_stream(c, hip_stream, [&](hipStream_t s) { return lvm::riesz_trig_eval(c, fn, d_x, d_y, n, s); });
}

int lvm_get_lab_lut(lvm_ctx* c, int16_t* dst) {
    if (!c || !dst) return LVM_ERR_INVALID;
    std::memcpy(dst, c->lab_lut_compact.data(), c->lab_lut_compact.size() * sizeof(int16_t));
    return LVM_OK;
}

int lvm_set_lab_lut(lvm_ctx* c, const int16_t* src) {
    if (!c || !src) return LVM_ERR_INVALID;
    (void)hipSetDevice(c->device);
    for (size_t i = 0; i < (size_t)LVM_LAB_LUT_ENTRIES; ++i)
        if (src[i] < 0 || src[i] > 16384) { c->err = "lvm_set_lab_lut: entry outside [0, 16384]"; return LVM_ERR_INVALID; }
    lvm::sync_streams(c);                        // kernels in flight read the old table (this context's buffers: no device-wide wait)
    c->lab_lut_compact.assign(src, src + LVM_LAB_LUT_ENTRIES);
    ++c->lab_lut_gen;                            // (the per-value table of a gray Riesz state is refilled from the new table at its next launch)
    return lvm::upload_lab_lut(c);
}

int lvm_debug_read_float(lvm_ctx* c, float* dst, size_t count) {
    if (!c || !dst) return LVM_ERR_INVALID;
    if (!c->d_float.p || count > c->float_count) { c->err = "no float frame kept"; return LVM_ERR_INVALID; }
    lvm::sync_streams(c);
    LVM_HIP_TRY(c, hipMemcpy(dst, c->d_float.p, count * sizeof(float), hipMemcpyDeviceToHost));
    return LVM_OK;
}

int lvm_profile_enable(lvm_ctx* c, int on) {
    if (!c) return LVM_ERR_INVALID;
    c->profiling = on != 0;
    return LVM_OK;
}

int lvm_profile_only(lvm_ctx* c, const char* name) {
    if (!c) return LVM_ERR_INVALID;
    (void)lvm_profile_collect(c);
    c->prof_totals.clear();
    c->prof_only = name ? name : "";
    return LVM_OK;
}

int lvm_profile_collect(lvm_ctx* c) {
    if (!c) return LVM_ERR_INVALID;
    lvm::sync_streams(c);
    for (auto& e : c->prof_events) {
        (void)hipEventSynchronize(e.e1);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.e0, e.e1) == hipSuccess) { c->prof_totals[e.name].ms += ms; c->prof_totals[e.name].n += 1; }
        (void)hipEventDestroy(e.e0); (void)hipEventDestroy(e.e1);
    }
    c->prof_events.clear();
    return (int)c->prof_totals.size();
}

int lvm_profile_entry(lvm_ctx* c, int idx, char* name, size_t cap, double* total_ms, long long* launches) {
    if (!c || idx < 0 || idx >= (int)c->prof_totals.size()) return LVM_ERR_INVALID;
    const auto& t = c->prof_totals[idx];
    if (name && cap) { std::snprintf(name, cap, "%s", t.name.c_str()); }
    if (total_ms) *total_ms = t.ms;
    if (launches) *launches = t.n;
    return LVM_OK;
}

int lvm_profile_variants(lvm_ctx* c, int idx, char* variants, size_t cap) {
    if (!c || idx < 0 || idx >= (int)c->prof_totals.size() || !variants || !cap) return LVM_ERR_INVALID;
    std::string all;
    for (const auto& v : c->prof_totals[idx].variants) { if (!all.empty()) all += ','; all += v; }
    std::snprintf(variants, cap, "%s", all.c_str());
    return LVM_OK;
}

int lvm_set_pipeline(lvm_ctx* c, int depth) {
    if (!c || depth < 0 || depth > 1) return LVM_ERR_INVALID;
    if (depth != c->pipeline_depth) {
        lvm::sync_streams(c);
        if (c->state) (void)c->state->flush(c, c->own_stream);
        lvm::sync_streams(c);
            c->pipeline_depth = depth;
    }
    return LVM_OK;
}

int lvm_flush(lvm_ctx* c, void* hip_stream) {
    if (!c) return LVM_ERR_INVALID;
    LVM_HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    if (!c->state) return LVM_OK;
    int rc = lvm::order_after_previous(c, s);           // the owed frame's pyramid was built on the stream of the call that owes it
    if (rc != LVM_OK) return rc;
    rc = c->state->flush(c, s);
    lvm::mark_enqueued(c, s);                           // (a reset or a destroy waits for the flush like for any other enqueue)
    return rc;
}

// compulsory traffic only -- every input byte read once, every output byte
// written once, every live persistent state word read once and written once.
double lvm_algorithmic_bytes(int mode, int w, int h, int channels, int levels, double framerate) {
    const int maxL = lvm::max_levels(w, h);
    if (maxL < 1) return 0.0;
    int L = levels < 1 ? 1 : (levels > maxL ? maxL : levels);
    double n[lvm::kMaxLevels + 2];
    int lw = w, lh = h;
    for (int l = 0; l <= L && l <= lvm::kMaxLevels; ++l) { n[l] = (double)lw * lh; lw = (lw + 1) / 2; lh = (lh + 1) / 2; }
    const double io = 2.0 * channels * n[0];
    if (mode == LVM_MODE_LAPLACE) {
        double s = 0; for (int l = 1; l <= L - 1; ++l) s += n[l];
        return io + 16.0 * channels * s;             // 2 low-pass states x 4 B x (R + W) per channel
    }
    if (mode == LVM_MODE_PHASE) {
        double s = 0; for (int l = 0; l <= L - 2; ++l) s += n[l];
        return io + 88.0 * s;                        // 11 live floats per band pixel, R + W
    }
    if (mode == LVM_MODE_COLOR) {
        const int T = lvm::optimal_buffer_size((int)framerate);
        return io + 4.0 * channels * n[L] * T + 4.0 * channels * n[L];
    }
    return 0.0;
}

}  // extern "C"
