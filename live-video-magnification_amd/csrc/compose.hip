// compose.hip -- the export hand-off on the device.
//
// Replaces the pane composition of Exporter::compose (reference: export/Exporter.cpp:22-34 toBgr, :53-88 compose,
// export/ExportTypes.hpp:11 SplitMode): both frames widened to BGR (gray -> b = g = r), cropped to their common EVEN
// size, and written next to each other (LeftRight), above each other (TopBottom) or alone (None) into one BGR canvas.
// Inputs are the magnifier's device output and the device copy of the original, so an export that encodes on the
// device -- or downloads ONE canvas instead of two frames -- needs no second PCIe crossing of the original.
// Byte work, bit-exact against the oracle.
//
// The text overlay (drawLabel, Exporter.cpp:36-50: addWeighted(roi, 0.35, black, 0.65) + cv::putText(LINE_AA, white)) is NOT restated
// -- OpenCV's anti-aliased Hershey strokes are not something to reproduce from memory -- and need not be: both steps read-modify-write
// single pixels, so what a label does to a canvas pixel is a FUNCTION OF THAT PIXEL'S BYTE, the same for B, G and R (white on black),
// fixed for the whole export (the label depends on the canvas size only).  Round 6: the reference-side shim renders the label once per
// export with the reference's own calls onto 256 constant canvases, which yields that function for every pixel of the label's rectangle
// exactly, whatever the OpenCV build does; pixels with the same function share a class.  k_overlay_labels applies the tables to the
// composed canvases where they lie: exact by construction, and an export with `textOverlay` stays on the device (and on the MJPEG path).
#include "lvm_internal.h"

namespace lvm {

// The panes of a canvas, on the host and as the pane part of both kernels' arguments: the two sources ([0] original, [1] processed; BGR or gray),
// the pane size (the frames' common even size) and where pane 1 starts on the canvas.  With one pane only src[1] is read.
struct Panes {
    const uint8_t* src[2]; long stride[2]; int cn[2];
    int w, h;
    int npanes, dx1, dy1;
};


struct ComposeArgs {
    Panes p; long sstride[2];
    uint8_t* dst; long dst_stride, dst_sstride;
};

// One thread per group of 4 canvas pixels of one pane row (12 output bytes as three dwords when the canvas row
// allows it, bytes otherwise); blockIdx.z = stream * npanes + pane.  (The dword packing is written out: lvm_pack_b4 costs this kernel
// 23 instructions -- the compiler builds these dwords from the byte loads better than from three v_perm_b32.)
template <bool VEC>
__global__ __launch_bounds__(256) void k_compose(ComposeArgs a) {
    const int gx = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (gx >= a.p.w || y >= a.p.h) return;
    const int pane = a.p.npanes == 2 ? (int)(blockIdx.z & 1) : 1, stream = a.p.npanes == 2 ? (int)(blockIdx.z >> 1) : (int)blockIdx.z;
    const uint8_t* p = a.p.src[pane] + (size_t)stream * a.sstride[pane] + (size_t)y * a.p.stride[pane];
    const int ox = pane ? a.p.dx1 : 0, oy = pane ? a.p.dy1 : 0;
    uint8_t* q = a.dst + (size_t)stream * a.dst_sstride + (size_t)(oy + y) * a.dst_stride + (size_t)(ox + gx) * 3;
    const int n = a.p.w - gx < 4 ? a.p.w - gx : 4;
    uint8_t v[12];
    if (a.p.cn[pane] == 3) {
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = k < 3 * n ? p[(size_t)gx * 3 + k] : 0;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) { const uint8_t g = k < n ? p[gx + k] : 0; v[3 * k] = g; v[3 * k + 1] = g; v[3 * k + 2] = g; }   // COLOR_GRAY2BGR
    }
    if (VEC && n == 4) {
        uint32_t* q4 = reinterpret_cast<uint32_t*>(q);
        q4[0] = v[0] | (v[1] << 8) | (v[2] << 16) | ((uint32_t)v[3] << 24);
        q4[1] = v[4] | (v[5] << 8) | (v[6] << 16) | ((uint32_t)v[7] << 24);
        q4[2] = v[8] | (v[9] << 8) | (v[10] << 16) | ((uint32_t)v[11] << 24);
    } else {
        for (int k = 0; k < 3 * n; ++k) q[k] = v[k];
    }
}

// ---- the text overlay as per-pixel tables (lvm_export_set_overlay) ----------------------------------------------------------------
constexpr int kMaxOverlayLabels = 4;
struct OverlayArgs {
    int n; int x[kMaxOverlayLabels], y[kMaxOverlayLabels], w[kMaxOverlayLabels], h[kMaxOverlayLabels];
    int first[kMaxOverlayLabels + 1];                   // prefix sums of w * h: thread index -> label
    const uint16_t* cls[kMaxOverlayLabels]; const uint8_t* fn[kMaxOverlayLabels];
    uint8_t* canvas; long stride, fstride;
};
// one thread per label pixel, blockIdx.y = frame: the three bytes of the pixel through the pixel's table
__global__ __launch_bounds__(256) void k_overlay_labels(OverlayArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.first[a.n]) return;
    int l = 0;
    while (l + 1 < a.n && i >= a.first[l + 1]) ++l;
    const int k = i - a.first[l], ly = k / a.w[l], lx = k - ly * a.w[l];
    const uint8_t* f = a.fn[l] + (size_t)a.cls[l][k] * 256;
    uint8_t* q = a.canvas + (size_t)blockIdx.y * a.fstride + (size_t)(a.y[l] + ly) * a.stride + (size_t)(a.x[l] + lx) * 3;
    q[0] = f[q[0]]; q[1] = f[q[1]]; q[2] = f[q[2]];
}

void overlay_release(Ctx* c) {
    if (c->d_overlay) (void)hipFree(c->d_overlay);
    c->d_overlay = nullptr; c->overlay_n = 0;
}

int overlay_set(Ctx* c, int n, const lvm_overlay_label* labels) {
    sync_streams(c);                                    // (a running export may still read the old tables)
    (void)hipStreamSynchronize(c->own_stream);
    overlay_release(c);
    if (n == 0) return LVM_OK;
    if (n < 0 || n > kMaxOverlayLabels || !labels) { c->err = "overlay: 0..4 labels"; return LVM_ERR_INVALID; }
    size_t total = 0;
    for (int l = 0; l < n; ++l) {
        const lvm_overlay_label& L = labels[l];
        if (L.w < 1 || L.h < 1 || L.x < 0 || L.y < 0 || L.n_classes < 1 || L.n_classes > 65536 || !L.cls || !L.fn || (long)L.w * L.h > (1L << 24)) { c->err = "overlay: bad label"; return LVM_ERR_INVALID; }
        for (long k = 0; k < (long)L.w * L.h; ++k) if (L.cls[k] >= L.n_classes) { c->err = "overlay: class index outside the label's tables"; return LVM_ERR_INVALID; }
        total += (((size_t)L.w * L.h * 2 + 255) & ~(size_t)255) + (size_t)L.n_classes * 256;
    }
    std::vector<uint8_t> host(total);
    LVM_HIP_TRY(c, hipMalloc((void**)&c->d_overlay, total));
    size_t off = 0;
    for (int l = 0; l < n; ++l) {
        const lvm_overlay_label& L = labels[l];
        c->ov_x[l] = L.x; c->ov_y[l] = L.y; c->ov_w[l] = L.w; c->ov_h[l] = L.h;
        c->ov_cls[l] = off; std::memcpy(host.data() + off, L.cls, (size_t)L.w * L.h * 2); off += ((size_t)L.w * L.h * 2 + 255) & ~(size_t)255;
        c->ov_fn[l] = off; std::memcpy(host.data() + off, L.fn, (size_t)L.n_classes * 256); off += (size_t)L.n_classes * 256;
    }
    if (hipMemcpy(c->d_overlay, host.data(), total, hipMemcpyHostToDevice) != hipSuccess) { overlay_release(c); c->err = "overlay: upload failed"; return LVM_ERR_HIP; }
    c->overlay_n = n;
    return LVM_OK;
}

// the labels onto n_frames canvases of cw x chh (nothing to do without labels)
int overlay_device(Ctx* c, const ImageOut& canvas, int n_frames, hipStream_t s) {
    const int cw = canvas.w, chh = canvas.h;
    if (c->overlay_n == 0 || n_frames < 1) return LVM_OK;
    if (!canvas.p || canvas.stride < (ptrdiff_t)cw * 3 || (n_frames > 1 && canvas.sstride < (ptrdiff_t)chh * canvas.stride)) { c->err = "overlay: bad canvas arguments"; return LVM_ERR_INVALID; }
    OverlayArgs a{};
    a.n = c->overlay_n; a.first[0] = 0;
    for (int l = 0; l < a.n; ++l) {
        // drawLabel clips its rectangle to the canvas BEFORE it draws (Exporter.cpp:44): the tables describe the clipped rectangle of ONE
        // canvas size -- a label that does not fit this canvas was rendered for another geometry
        if (c->ov_x[l] + c->ov_w[l] > cw || c->ov_y[l] + c->ov_h[l] > chh) { c->err = "overlay: a label lies outside the canvas (rendered for another canvas size?)"; return LVM_ERR_INVALID; }
        a.x[l] = c->ov_x[l]; a.y[l] = c->ov_y[l]; a.w[l] = c->ov_w[l]; a.h[l] = c->ov_h[l];
        a.first[l + 1] = a.first[l] + a.w[l] * a.h[l];
        a.cls[l] = reinterpret_cast<const uint16_t*>(c->d_overlay + c->ov_cls[l]); a.fn[l] = c->d_overlay + c->ov_fn[l];
    }
    a.canvas = canvas.p; a.stride = (long)canvas.stride; a.fstride = (long)canvas.sstride;
    LVM_LAUNCH(c, "overlay", k_overlay_labels, dim3((unsigned)((a.first[a.n] + 255) / 256), (unsigned)n_frames), dim3(256), s, a);
    LVM_HIP_TRY(c, hipGetLastError());
    return LVM_OK;
}

// Exporter.cpp:55-66: canvas size and pane size for the two frame sizes
int compose_geometry(int split, int ow, int oh, int pw, int ph, int* pane_w, int* pane_h, int* canvas_w, int* canvas_h) {
    int w, h;
    if (split == LVM_SPLIT_NONE) { w = pw & ~1; h = ph & ~1; }                         // :56
    else { w = (ow < pw ? ow : pw) & ~1; h = (oh < ph ? oh : ph) & ~1; }               // :63-64
    if (w <= 0 || h <= 0) { *pane_w = *pane_h = *canvas_w = *canvas_h = 0; return 0; }   // :57, :65 (empty Mat)
    *pane_w = w; *pane_h = h;
    *canvas_w = split == LVM_SPLIT_LEFT_RIGHT ? 2 * w : w;                             // :71
    *canvas_h = split == LVM_SPLIT_TOP_BOTTOM ? 2 * h : h;                             // :79
    return 1;
}

// The panes of a canvas from the two frames, for compose_device and canvas_yuv_fused alike (Exporter.cpp:53-66): the split and frame checks, the
// processed frame in place of a missing original (:62), the geometry, the row strides.  `canvas_error(canvas_w, canvas_h)` is the caller's check of
// its destination, made once the canvas size is known (null: fine).  p->w == 0 on return: an empty canvas, nothing to write.
template <class CanvasError>
static int panes_resolve(Ctx* c, int split, Image orig, const Image& proc, const void* dst, Panes* p, CanvasError&& canvas_error) {
    *p = Panes{};
    if (split < LVM_SPLIT_NONE || split > LVM_SPLIT_TOP_BOTTOM) { c->err = "invalid split mode"; return LVM_ERR_INVALID; }
    if (!proc.p || !dst || (proc.cn != 1 && proc.cn != 3)) { c->err = "bad processed frame"; return LVM_ERR_INVALID; }
    const bool two = split != LVM_SPLIT_NONE;
    if (!two || !orig.p) orig = proc;
    if (orig.cn != 1 && orig.cn != 3) { c->err = "bad original frame"; return LVM_ERR_INVALID; }
    int w, h, cw, chh;
    if (!compose_geometry(split, orig.w, orig.h, proc.w, proc.h, &w, &h, &cw, &chh)) return LVM_OK;
    if (const char* why = canvas_error(cw, chh)) { c->err = why; return LVM_ERR_INVALID; }
    // the kernels index the frames with the caller's strides: rows must hold their pixels
    if (proc.stride < (ptrdiff_t)proc.w * proc.cn || orig.stride < (ptrdiff_t)orig.w * orig.cn) { c->err = "frame stride too small"; return LVM_ERR_INVALID; }
    p->src[0] = orig.p; p->stride[0] = (long)orig.stride; p->cn[0] = orig.cn;
    p->src[1] = proc.p; p->stride[1] = (long)proc.stride; p->cn[1] = proc.cn;
    p->w = w; p->h = h;
    p->npanes = two ? 2 : 1;
    p->dx1 = split == LVM_SPLIT_LEFT_RIGHT ? w : 0;
    p->dy1 = split == LVM_SPLIT_TOP_BOTTOM ? h : 0;
    return LVM_OK;
}

int compose_device(Ctx* c, int split, const Image& orig, const Image& proc, const ImageOut& canvas, hipStream_t s) {
    ComposeArgs a{};
    int chh = 0;
    const int rc = panes_resolve(c, split, orig, proc, canvas.p, &a.p, [&](int cw, int ch) { chh = ch; return canvas.stride < (ptrdiff_t)cw * 3 ? "canvas stride too small" : nullptr; });
    if (rc != LVM_OK || a.p.w == 0) return rc;
    // ... and with several streams, the streams must not overlap (a missing original: the processed frame's)
    const Image& o = (a.p.npanes == 2 && orig.p) ? orig : proc;
    if (c->nstreams > 1 && (canvas.sstride < (ptrdiff_t)chh * canvas.stride || proc.sstride < (ptrdiff_t)proc.h * proc.stride ||
                            o.sstride < (ptrdiff_t)o.h * o.stride)) { c->err = "stream stride too small"; return LVM_ERR_INVALID; }
    a.sstride[0] = (long)o.sstride; a.sstride[1] = (long)proc.sstride;
    a.dst = canvas.p; a.dst_stride = (long)canvas.stride; a.dst_sstride = (long)canvas.sstride;
    // dword stores need every pane row segment dword-aligned: canvas base, strides and the pane-1 column offset (3 w bytes)
    const bool vec = ((uintptr_t)canvas.p % 4) == 0 && canvas.stride % 4 == 0 && canvas.sstride % 4 == 0 && (a.p.dx1 * 3) % 4 == 0;
    const dim3 grid(((a.p.w + 3) / 4 + 63) / 64, (a.p.h + 3) / 4, (unsigned)(c->nstreams * a.p.npanes)), blk(256);
    if (vec) LVM_LAUNCH(c, "compose", k_compose<true>, grid, blk, s, a);
    else LVM_LAUNCH(c, "compose", k_compose<false>, grid, blk, s, a);
    LVM_HIP_TRY(c, hipGetLastError());
    return LVM_OK;
}

// ---- canvases as 4:2:0 surfaces (lvm_set_canvas_format, include/lvm_hip.h) -------------------------------------------------------------
// cvtColor(canvas, COLOR_BGR2YUV_I420) of OpenCV 4 (color_yuv: ITU-R BT.601, limited range, 20-bit fixed point) in the layouts NV12 / NV21 /
// I420 / YV12.  Every sum is positive and below 2^31 (the extreme ones: tests/test_yuv_canvas.py), every result lies in 0..255: plain int32, a
// shift, no clamp.  Chroma is the top-left pixel's of each 2 x 2 block.  Pure streaming: 3 (or 1) bytes in, 1.5 bytes out per pixel.
__device__ __forceinline__ uint32_t yuv_y(int b, int g, int r) { return (uint32_t)((269484 * r + 528482 * g + 102760 * b + (1 << 19) + (16 << 20)) >> 20); }
__device__ __forceinline__ uint32_t yuv_u(int b, int g, int r) { return (uint32_t)((-155188 * r - 305135 * g + 460324 * b + (1 << 19) + (128 << 20)) >> 20); }
__device__ __forceinline__ uint32_t yuv_v(int b, int g, int r) { return (uint32_t)((460324 * r - 385875 * g - 74448 * b + (1 << 19) + (128 << 20)) >> 20); }

struct CanvasYuvArgs {
    // the source: a BGR canvas in memory (one BGR pane at the origin: frame f at + f * src_fstride), or the panes compose_device would write into it
    Panes p;
    long src_fstride;
    uint8_t* dst; long ystride, cstride, dst_fstride, plane1, plane2;   // plane1 / plane2: where U / V go (planar), or plane1 = the interleaved plane
    int w, h;                 // canvas size (even)
    int interleaved, v_first; // NV12 / NV21: byte pairs (U, V) / (V, U) in one plane of row stride cstride = ystride
};

// One thread per block of 2 rows x 8 pixels of the canvas: 2 x 24 BGR bytes (2 x 8 of a gray pane) in, 2 x 8 Y bytes and 4 U + 4 V bytes out;
// blockIdx.z = frame.  VEC: dword-wide loads and stores (every pointer, stride and offset dword-aligned, w % 8 == 0, the block inside ONE pane);
// otherwise bytes, a block of 2, 4 or 6 pixels at the right edge (w is even) and a pane per pixel.  (Which pane and which pixel of it is
// written out in both branches, and the fetch again in k_compose: through shared functions the byte variants grow by 43 to 130 instructions.
// The dword packing of the stores is written out too: lvm_pack_b4 reorders the whole dword variant, 34 -> 36 VGPRs.)
template <bool VEC>
__global__ __launch_bounds__(256) void k_canvas_yuv(CanvasYuvArgs a) {
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 8, y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 2;
    if (x0 >= a.w || y0 >= a.h) return;
    const size_t f = blockIdx.z;
    const int n = a.w - x0 < 8 ? a.w - x0 : 8;
    uint32_t Y[2][8], U[4], V[4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int y = y0 + r;
        // (a block of two rows lies in one pane vertically: pane heights are even)
        const int py = (a.p.npanes == 2 && y >= a.p.h && a.p.dy1) ? 1 : 0;
        uint8_t px[24];
        if (VEC) {
            const int pane = a.p.npanes == 2 ? ((a.p.dx1 && x0 >= a.p.dx1) || py ? 1 : 0) : 1;
            const int lx = x0 - (pane && a.p.npanes == 2 ? a.p.dx1 : 0), ly = y - (py ? a.p.dy1 : 0);
            const uint8_t* p = a.p.src[pane] + f * a.src_fstride + (size_t)ly * a.p.stride[pane];
            if (a.p.cn[pane] == 3) {
                const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p + (size_t)lx * 3);
#pragma unroll
                for (int k = 0; k < 6; ++k) { const uint32_t v = p4[k]; px[4 * k] = (uint8_t)v; px[4 * k + 1] = (uint8_t)(v >> 8); px[4 * k + 2] = (uint8_t)(v >> 16); px[4 * k + 3] = (uint8_t)(v >> 24); }
            } else {
                const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p + lx);
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const uint32_t v = p4[k];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const uint8_t g = (uint8_t)(v >> (8 * j)); px[12 * k + 3 * j] = g; px[12 * k + 3 * j + 1] = g; px[12 * k + 3 * j + 2] = g; }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int x = x0 + k;
                const int pane = a.p.npanes == 2 ? ((a.p.dx1 && x >= a.p.dx1) || py ? 1 : 0) : 1;
                const int lx = x - (pane && a.p.npanes == 2 ? a.p.dx1 : 0), ly = y - (py ? a.p.dy1 : 0);
                const uint8_t* p = a.p.src[pane] + f * a.src_fstride + (size_t)ly * a.p.stride[pane];
                if (k < n) {
                    if (a.p.cn[pane] == 3) { px[3 * k] = p[(size_t)lx * 3]; px[3 * k + 1] = p[(size_t)lx * 3 + 1]; px[3 * k + 2] = p[(size_t)lx * 3 + 2]; }
                    else { const uint8_t g = p[lx]; px[3 * k] = g; px[3 * k + 1] = g; px[3 * k + 2] = g; }      // COLOR_GRAY2BGR
                } else { px[3 * k] = 0; px[3 * k + 1] = 0; px[3 * k + 2] = 0; }
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) Y[r][k] = yuv_y(px[3 * k], px[3 * k + 1], px[3 * k + 2]);
        if (r == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { U[k] = yuv_u(px[6 * k], px[6 * k + 1], px[6 * k + 2]); V[k] = yuv_v(px[6 * k], px[6 * k + 1], px[6 * k + 2]); }
        }
    }
    uint8_t* q = a.dst + f * a.dst_fstride;
    uint8_t* qy = q + (size_t)y0 * a.ystride + x0;
    const size_t crow = (size_t)(y0 >> 1) * a.cstride;
    if (a.v_first && a.interleaved) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { const uint32_t t = U[k]; U[k] = V[k]; V[k] = t; }
    }
    if (VEC) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            uint32_t* q4 = reinterpret_cast<uint32_t*>(qy + (size_t)r * a.ystride);
            q4[0] = Y[r][0] | (Y[r][1] << 8) | (Y[r][2] << 16) | (Y[r][3] << 24);
            q4[1] = Y[r][4] | (Y[r][5] << 8) | (Y[r][6] << 16) | (Y[r][7] << 24);
        }
        if (a.interleaved) {
            uint32_t* c4 = reinterpret_cast<uint32_t*>(q + a.plane1 + crow + x0);
            c4[0] = U[0] | (V[0] << 8) | (U[1] << 16) | (V[1] << 24);
            c4[1] = U[2] | (V[2] << 8) | (U[3] << 16) | (V[3] << 24);
        } else {
            *reinterpret_cast<uint32_t*>(q + a.plane1 + crow + (x0 >> 1)) = U[0] | (U[1] << 8) | (U[2] << 16) | (U[3] << 24);
            *reinterpret_cast<uint32_t*>(q + a.plane2 + crow + (x0 >> 1)) = V[0] | (V[1] << 8) | (V[2] << 16) | (V[3] << 24);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 8; ++k) if (k < n) qy[(size_t)r * a.ystride + k] = (uint8_t)Y[r][k];
        if (a.interleaved) {
            uint8_t* cq = q + a.plane1 + crow + x0;
#pragma unroll
            for (int k = 0; k < 4; ++k) if (2 * k < n) { cq[2 * k] = (uint8_t)U[k]; cq[2 * k + 1] = (uint8_t)V[k]; }
        } else {
            uint8_t* uq = q + a.plane1 + crow + (x0 >> 1);
            uint8_t* vq = q + a.plane2 + crow + (x0 >> 1);
#pragma unroll
            for (int k = 0; k < 4; ++k) if (2 * k < n) { uq[k] = (uint8_t)U[k]; vq[k] = (uint8_t)V[k]; }
        }
    }
}

const char* canvas_layout(int fmt, int w, int h, ptrdiff_t stride, CanvasLayout* out) {
    CanvasLayout L{};
    if (fmt == LVM_PIX_BGR) {
        if (w < 1 || h < 1) return "canvas format: bad canvas size";
        if (stride < (ptrdiff_t)w * 3) return "canvas stride too small";
        L.bytes = (size_t)stride * h;
    } else if (fmt == LVM_PIX_NV12 || fmt == LVM_PIX_NV21 || fmt == LVM_PIX_I420 || fmt == LVM_PIX_YV12) {
        const bool nv = fmt == LVM_PIX_NV12 || fmt == LVM_PIX_NV21;
        if (w < 2 || h < 2 || w % 2 || h % 2) return "canvas format: w and h must be even and >= 2";
        if (nv && stride < (ptrdiff_t)w) return "canvas format: canvas_stride must be >= canvas_w for NV12 / NV21";
        if (!nv && (stride < (ptrdiff_t)w || stride % 2)) return "canvas format: canvas_stride must be even and >= canvas_w for I420 / YV12";
        L.plane1 = (size_t)stride * h;
        L.plane2 = nv ? 0 : L.plane1 + L.plane1 / 4;
        L.bytes = L.plane1 + L.plane1 / 2;
        L.cstride = nv ? stride : stride / 2;
    } else {
        return "canvas format: the format must be LVM_PIX_BGR (0), _NV12 (4), _NV21 (5), _I420 (6) or _YV12 (7)";
    }
    if (out) *out = L;
    return nullptr;
}

// the destination half of the arguments, and whether it allows dword stores
static bool canvas_yuv_dst(CanvasYuvArgs& a, int fmt, int w, int h, const ImageOut& out, int n_frames, const CanvasLayout& L) {
    a.w = w; a.h = h;
    a.dst = out.p; a.ystride = (long)out.stride; a.cstride = (long)L.cstride; a.dst_fstride = n_frames > 1 ? (long)out.sstride : 0;
    a.interleaved = fmt == LVM_PIX_NV12 || fmt == LVM_PIX_NV21;
    a.v_first = fmt == LVM_PIX_NV21 || fmt == LVM_PIX_YV12;
    a.plane1 = (long)L.plane1; a.plane2 = (long)L.plane2;
    if (!a.interleaved && a.v_first) { a.plane1 = (long)L.plane2; a.plane2 = (long)L.plane1; }      // YV12: the V plane comes first
    return w % 8 == 0 && (uintptr_t)out.p % 4 == 0 && out.stride % 4 == 0 && a.dst_fstride % 4 == 0 && L.cstride % 4 == 0 && L.plane1 % 4 == 0 && L.plane2 % 4 == 0;
}

static int canvas_yuv_launch(Ctx* c, const CanvasYuvArgs& a, bool vec, bool fused, int n_frames, hipStream_t s) {
    const dim3 grid(((a.w + 7) / 8 + 63) / 64, (a.h / 2 + 3) / 4, (unsigned)n_frames), blk(256);
    if (vec) LVM_LAUNCH_V(c, "canvas_yuv", "vec8", k_canvas_yuv<true>, grid, blk, s, a);
    else LVM_LAUNCH_V(c, "canvas_yuv", "bytes", k_canvas_yuv<false>, grid, blk, s, a);
    if (fused && c->profiling) prof_variant(c, "fused");
    LVM_HIP_TRY(c, hipGetLastError());
    return LVM_OK;
}

int canvas_yuv_device(Ctx* c, int fmt, const Image& bgr, int n_frames, const ImageOut& out, hipStream_t s, bool check_only) {
    const int w = bgr.w, h = bgr.h;
    if (fmt != LVM_PIX_NV12 && fmt != LVM_PIX_NV21 && fmt != LVM_PIX_I420 && fmt != LVM_PIX_YV12) {
        c->err = "lvm_canvas_convert_device: the format must be LVM_PIX_NV12 (4), _NV21 (5), _I420 (6) or _YV12 (7)"; return LVM_ERR_INVALID;
    }
    if (!bgr.p || !out.p || n_frames < 1 || n_frames > 65535) { c->err = "lvm_canvas_convert_device: null canvas pointer, or not 1..65535 frames"; return LVM_ERR_INVALID; }
    CanvasLayout L;
    if (const char* why = canvas_layout(fmt, w, h, out.stride, &L)) { c->err = why; return LVM_ERR_INVALID; }
    if (bgr.stride < (ptrdiff_t)w * 3) { c->err = "lvm_canvas_convert_device: bgr_stride must be >= 3 * w"; return LVM_ERR_INVALID; }
    if (n_frames > 1 && (out.sstride < 0 || (size_t)out.sstride < L.bytes)) { c->err = "lvm_canvas_convert_device: out_frame_stride must be >= the bytes of one canvas (the frames would overlap)"; return LVM_ERR_INVALID; }
    if (check_only) return LVM_OK;
    CanvasYuvArgs a{};
    a.p = Panes{{bgr.p, bgr.p}, {(long)bgr.stride, (long)bgr.stride}, {3, 3}, w, h, 1, 0, 0};     // one BGR pane at the origin
    a.src_fstride = n_frames > 1 ? (long)bgr.sstride : 0;
    bool vec = canvas_yuv_dst(a, fmt, w, h, out, n_frames, L);
    vec = vec && (uintptr_t)bgr.p % 4 == 0 && bgr.stride % 4 == 0 && a.src_fstride % 4 == 0;
    return canvas_yuv_launch(c, a, vec, false, n_frames, s);
}

// compose_device's panes (same geometry, same fall-back for a missing original) straight into the surface: the BGR canvas is never written
int canvas_yuv_fused(Ctx* c, int fmt, int split, const Image& orig, const Image& proc, const ImageOut& out, hipStream_t s) {
    CanvasYuvArgs a{};
    CanvasLayout L;
    int cw = 0, chh = 0;
    const int rc = panes_resolve(c, split, orig, proc, out.p, &a.p, [&](int w, int h) -> const char* {
        cw = w; chh = h;
        if (const char* why = canvas_layout(fmt, w, h, out.stride, &L)) return why;
        return fmt == LVM_PIX_BGR ? "canvas format: a YUV format is needed here" : nullptr;
    });
    if (rc != LVM_OK || a.p.w == 0) return rc;
    bool vec = canvas_yuv_dst(a, fmt, cw, chh, out, 1, L);
    // dword loads need every pane row segment dword-aligned and every 8-pixel block inside one pane: the pane-1 column (dx1 = pane width, even
    // but no multiple of 8 in general) decides, as 3 * dx1 does for compose_device's stores
    vec = vec && a.p.dx1 % 8 == 0 && (uintptr_t)a.p.src[1] % 4 == 0 && a.p.stride[1] % 4 == 0 && (a.p.npanes == 1 || ((uintptr_t)a.p.src[0] % 4 == 0 && a.p.stride[0] % 4 == 0));
    return canvas_yuv_launch(c, a, vec, true, 1, s);
}

}  // namespace lvm
