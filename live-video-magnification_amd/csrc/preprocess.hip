// preprocess.hip -- the two uint8 stages in front of the magnifier, on the device.
//
// Replaces PreprocessProcessor::process (reference: processing/PreprocessProcessor.cpp:10-51: ROI crop
// in normalised coordinates, cv::resize(INTER_AREA) by 1/2/4/8) and GrayscaleProcessor::process
// (processing/GrayscaleProcessor.cpp:7-16: cv::cvtColor(BGR2GRAY)).  One kernel does crop + decimation +
// gray per output pixel, so the full-resolution frame is read once and only the small frame is written:
//   * integer decimation (ROI size divisible by the divisor): block sum, (sum + 2) >> 2 for 2x2,
//     saturate_cast<uchar>(sum * (1.f / area)) otherwise (OpenCV resizeAreaFast_);
//   * any other size: the fractional-cell tables of OpenCV's general INTER_AREA path, float sums in table
//     order (resizeArea_), tables built on the host per geometry and cached in the context;
//   * gray: 15-bit fixed point (b*3735 + g*19235 + r*9798 + 2^14) >> 15, applied to the decimated bytes
//     exactly as the reference's stage order does.
// Byte/integer work: results are bit-exact against the oracle (tests/test_preprocess_*.py).
//
// Opt-in (lvm_set_source_format): the source frame in a raw camera format -- YUYV, UYVY, YVYU, NV12, NV21 -- converted by the same launch with the
// arithmetic of cv::cvtColor(COLOR_YUV2BGR_*), i.e. the reference chain behind a cv::VideoCapture that converted the frame itself: the fetch of a
// source pixel becomes "load the raw bytes, convert", everything behind it is the code of the BGR kernels (tests/test_yuv_source.py).
#include <cmath>
#include <cstring>
#include <vector>

#include "lvm_internal.h"

namespace lvm {

struct AreaTab { int si, di; float alpha; };

struct PreArgs {
    const uint8_t* in; long in_stride, in_sstride;     // already offset to the ROI origin
    uint8_t* out; long out_stride, out_sstride;
    int ow, oh, cn, ocn;                               // output size, input channels, output channels
    int sx, sy;                                        // integer decimation factors (fast path)
    uint8_t* tap; long tap_stride, tap_sstride;        // optional: the 3-channel frame BEFORE BGR2GRAY (runChainOnce's `original`, ChainBuilder.cpp:25)
    const AreaTab* xtab; const int* xk;                // general path: entries of output column dx are xtab[xk[dx] .. xk[dx+1])
    const AreaTab* ytab; const int* yk;
};

// (gray15: lvm_internal.h -- the gray Phase output kernels of riesz.hip apply the same weighting)

// The arithmetic of one output pixel, shared by every kernel of this file: `fetch.at(x, y)` is a cursor at source pixel (x, y) of the ROI and
// `cursor(i, v)` delivers the CN bytes of the pixel i columns to its right -- a load for BGR / gray frames, a load + conversion for the raw
// camera formats below -- and everything behind it (block sums, (sum + 2) >> 2, saturate_cast<uchar>(sum * (1.f / area)), the fractional AreaTab
// sums in table order) is the same code for all of them.  The byte cursor spells the address arithmetic the BGR kernels always had (row pointer,
// 64-bit column offset), and they form their output pointer before the loads: their instruction streams stay those of the kernels without it.
// MODE 0 = crop only, 1 = integer decimation, 2 = fractional area tables.
template <int MODE, int CN, class Fetch>
__device__ __forceinline__ void pre_pixel(const PreArgs& a, const Fetch& fetch, int dx, int dy, int (&v)[CN]) {
    if (MODE == 0) {
        fetch.at(dx, dy)(0, v);
    } else if (MODE == 1) {
        int sum[CN];
#pragma unroll
        for (int c = 0; c < CN; ++c) sum[c] = 0;
        for (int yy = 0; yy < a.sy; ++yy) {
            const auto row = fetch.at(dx * a.sx, dy * a.sy + yy);
            for (int xx = 0; xx < a.sx; ++xx) {
                int p[CN];
                row(xx, p);
#pragma unroll
                for (int c = 0; c < CN; ++c) sum[c] += p[c];
            }
        }
        const bool fast2 = a.sx == 2 && a.sy == 2;
        const float scale = 1.f / (float)(a.sx * a.sy);
#pragma unroll
        for (int c = 0; c < CN; ++c) v[c] = fast2 ? ((sum[c] + 2) >> 2) : (int)sat_u8((float)sum[c] * scale);
    } else {
        float sum[CN];
        const int x0 = a.xk[dx], x1 = a.xk[dx + 1], y0 = a.yk[dy], y1 = a.yk[dy + 1];
        for (int j = y0; j < y1; ++j) {
            const float beta = a.ytab[j].alpha;
            const auto row = fetch.at(0, a.ytab[j].si);
            float buf[CN];
#pragma unroll
            for (int c = 0; c < CN; ++c) buf[c] = 0.f;
            for (int k = x0; k < x1; ++k) {
                const float alpha = a.xtab[k].alpha;
                int p[CN];
                row(a.xtab[k].si, p);
#pragma unroll
                for (int c = 0; c < CN; ++c) buf[c] = buf[c] + (float)p[c] * alpha;
            }
#pragma unroll
            for (int c = 0; c < CN; ++c) sum[c] = (j == y0) ? beta * buf[c] : sum[c] + beta * buf[c];
        }
#pragma unroll
        for (int c = 0; c < CN; ++c) v[c] = (int)sat_u8(sum[c]);
    }
}

// ... and where it goes: the frame the magnifier sees (gray15 of the decimated bytes with grayscale on) and the optional colour tap
__device__ __forceinline__ uint8_t* pre_out(const PreArgs& a, size_t z, int dx, int dy) {
    return a.out + z * a.out_sstride + (size_t)dy * a.out_stride + (size_t)dx * a.ocn;
}
template <int CN>
__device__ __forceinline__ void pre_store(const PreArgs& a, uint8_t* q, size_t z, int dx, int dy, const int (&v)[CN]) {
    if (CN == 3 && a.ocn == 1) {
        q[0] = gray15(v[0], v[1], v[2]);
        if (a.tap) {        // PreprocessProcessor's own output: what the chain hands on as `original` before GrayscaleProcessor runs
            uint8_t* t = a.tap + z * a.tap_sstride + (size_t)dy * a.tap_stride + (size_t)dx * 3;
            t[0] = (uint8_t)v[0]; t[1] = (uint8_t)v[1]; t[2] = (uint8_t)v[2];
        }
    } else {
#pragma unroll
        for (int c = 0; c < CN; ++c) q[c] = (uint8_t)v[c];
    }
}

template <int CN>
struct FetchBytes {
    const uint8_t* src; long stride;
    struct Cursor {
        const uint8_t* p;
        __device__ __forceinline__ void operator()(int i, int (&v)[CN]) const {
            const uint8_t* q = p + (size_t)i * CN;
#pragma unroll
            for (int c = 0; c < CN; ++c) v[c] = q[c];
        }
    };
    __device__ __forceinline__ Cursor at(int x, int y) const { return Cursor{src + (size_t)y * stride + (size_t)x * CN}; }
};

// One thread per output pixel; blockIdx.z = stream.
template <int MODE, int CN>
__global__ __launch_bounds__(256) void k_preprocess(PreArgs a) {
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= a.ow || dy >= a.oh) return;
    const FetchBytes<CN> fetch{a.in + (size_t)blockIdx.z * a.in_sstride, a.in_stride};
    uint8_t* q = pre_out(a, blockIdx.z, dx, dy);
    int v[CN];
    pre_pixel<MODE, CN>(a, fetch, dx, dy, v);
    pre_store<CN>(a, q, blockIdx.z, dx, dy, v);
}

// ---- raw camera formats (lvm_set_source_format, include/lvm_hip.h) -----------------------------------------------------------------
// cv::cvtColor(COLOR_YUV2BGR_*) in front of PreprocessProcessor: OpenCV 4's color_yuv, ITU-R BT.601 limited range in 20-bit fixed point.
// All int32 (|sum| < 2^30), `>>` arithmetic: negative sums floor before the clamp.
__device__ __forceinline__ int yuv_sat(int s) { s >>= 20; return s < 0 ? 0 : (s > 255 ? 255 : s); }
__device__ __forceinline__ void yuv2bgr(int Y, int U, int V, int (&v)[3]) {
    const int y = (Y > 16 ? Y - 16 : 0) * 1220542 + (1 << 19), u = U - 128, w = V - 128;
    v[0] = yuv_sat(y + 2116026 * u);
    v[1] = yuv_sat(y - 852492 * w - 409993 * u);
    v[2] = yuv_sat(y + 1673527 * w);
}

// Where the bytes of a 4:2:2 pair sit (Y of pixel 2k at yo, of pixel 2k + 1 at yo + 2) and the order of an NV chroma pair.
template <int FMT> struct YuvLayout {
    static constexpr bool packed = FMT == LVM_PIX_YUYV || FMT == LVM_PIX_UYVY || FMT == LVM_PIX_YVYU;
    static constexpr int yo = FMT == LVM_PIX_UYVY ? 1 : 0;
    static constexpr int uo = FMT == LVM_PIX_YUYV ? 1 : (FMT == LVM_PIX_UYVY ? 0 : (FMT == LVM_PIX_YVYU ? 3 : (FMT == LVM_PIX_NV12 ? 0 : 1)));
    static constexpr int vo = FMT == LVM_PIX_YUYV ? 3 : (FMT == LVM_PIX_UYVY ? 2 : (FMT == LVM_PIX_YVYU ? 1 : (FMT == LVM_PIX_NV12 ? 1 : 0)));
};

// The source of the raw kernels.  PreArgs::in points at the 4:2:2 pair (packed) / the Y byte (NV12, NV21) that holds pixel (-x0, 0) of the
// ROI, `uv` at the chroma pair of pixel (-x0, -y0): x0, y0 in {0, 1} are the parities of the ROI's origin in the frame, so that pairs and
// 2x2 blocks are shared by ABSOLUTE frame coordinates.
struct YuvSrc { const uint8_t* uv; int x0, y0; };

template <int FMT>
struct FetchYuv {
    const uint8_t* src; const uint8_t* uv; long stride; int x0, y0;
    struct Cursor {
        const uint8_t* py; const uint8_t* pc; int X;        // the Y row (packed: the row of pairs), the chroma row, the column in them
        __device__ __forceinline__ void operator()(int i, int (&v)[3]) const {
            typedef YuvLayout<FMT> L;
            const int x = X + i;
            int Y, U, V;
            if (L::packed) {
                const uint8_t* p = py + (size_t)(x >> 1) * 4;
                Y = p[L::yo + (x & 1) * 2]; U = p[L::uo]; V = p[L::vo];
            } else {
                Y = py[x];
                const uint8_t* q = pc + (size_t)(x & ~1);
                U = q[L::uo]; V = q[L::vo];
            }
            yuv2bgr(Y, U, V, v);
        }
    };
    __device__ __forceinline__ Cursor at(int x, int y) const {
        return Cursor{src + (size_t)y * stride, YuvLayout<FMT>::packed ? nullptr : uv + (size_t)((y + y0) >> 1) * stride, x + x0};
    }
};

// Byte variant ("yuv"): any geometry, any alignment.  One thread per output pixel like k_preprocess; block sums add converted bytes.
template <int MODE, int FMT>
__global__ __launch_bounds__(256) void k_preprocess_yuv(PreArgs a, YuvSrc y) {
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= a.ow || dy >= a.oh) return;
    const size_t so = (size_t)blockIdx.z * a.in_sstride;
    const FetchYuv<FMT> fetch{a.in + so, y.uv ? y.uv + so : nullptr, a.in_stride, y.x0, y.y0};
    uint8_t* q = pre_out(a, blockIdx.z, dx, dy);
    int v[3];
    pre_pixel<MODE, 3>(a, fetch, dx, dy, v);
    pre_store<3>(a, q, blockIdx.z, dx, dy, v);
}

// Vector variant ("yuv4") of the conversion-only case, colour out: a live camera at full frame into the magnifier.  A thread takes four
// pixels -- two 4:2:2 pairs as one 8-byte load, or a dword of Y and a dword of UV -- and writes their 12 bytes as three dwords.  The
// launch code selects it where every base pointer and stride is a multiple of 4, x0 = 0 and the width a multiple of 4.  The raw rows
// are read once, by this kernel alone, and the BGR frame is written for a later launch: streaming loads and stores (lvm_gfx950.h).
template <int FMT>
__global__ __launch_bounds__(256) void k_yuv_vec4(PreArgs a, YuvSrc y) {
    typedef YuvLayout<FMT> L;
    const int g = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (g >= (a.ow >> 2) || dy >= a.oh) return;
    const size_t so = (size_t)blockIdx.z * a.in_sstride;
    uint32_t yy, uv;                   // yy: Y of the four pixels, byte k = pixel k; uv: byte 0 = U, 1 = V of pixels 0-1, bytes 2, 3 of pixels 2-3
    if (L::packed) {
        const uint2 d = ld_stream_u32x2(a.in + so + (size_t)dy * a.in_stride + (size_t)g * 8);
        const uint32_t ys = L::yo * 8, us = L::uo * 8, vs = L::vo * 8;
        yy = ((d.x >> ys) & 255u) | (((d.x >> (ys + 16)) & 255u) << 8) | (((d.y >> ys) & 255u) << 16) | (((d.y >> (ys + 16)) & 255u) << 24);
        uv = ((d.x >> us) & 255u) | (((d.x >> vs) & 255u) << 8) | (((d.y >> us) & 255u) << 16) | (((d.y >> vs) & 255u) << 24);
    } else {
        yy = __float_as_uint(ld_stream_f32(a.in + so + (size_t)dy * a.in_stride + (size_t)g * 4));
        const uint32_t q = __float_as_uint(ld_stream_f32(y.uv + so + (size_t)((dy + y.y0) >> 1) * a.in_stride + (size_t)g * 4));
        uv = L::uo == 0 ? q : (((q >> 8) & 0x00ff00ffu) | ((q & 0x00ff00ffu) << 8));
    }
    int p[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int sh = (k >> 1) * 16;
        yuv2bgr((int)((yy >> (8 * k)) & 255u), (int)((uv >> sh) & 255u), (int)((uv >> (sh + 8)) & 255u), p[k]);
    }
    uint8_t* q = a.out + (size_t)blockIdx.z * a.out_sstride + (size_t)dy * a.out_stride + (size_t)g * 12;
    st_stream_b96(q, lvm_pack_b4(p[0][0], p[0][1], p[0][2], p[1][0]), lvm_pack_b4(p[1][1], p[1][2], p[2][0], p[2][1]),
                  lvm_pack_b4(p[2][2], p[3][0], p[3][1], p[3][2]));
}

// the kernel of a run-time (MODE, CN / FMT): lvm_pick (lvm_internal.h); a format that is none of the five listed counts as the last, NV21
typedef PickInt<0, 1, 2> PickMode;
typedef PickInt<LVM_PIX_YUYV, LVM_PIX_UYVY, LVM_PIX_YVYU, LVM_PIX_NV12, LVM_PIX_NV21> PickYuv;

// ---- host ----------------------------------------------------------------------------------------
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int preprocess_divisor(const lvm_preprocess_params& pp) { return clampi(pp.downscale, 1, 8); }      // PreprocessProcessor.cpp:36
// PreprocessProcessor.cpp:13-31, :36-39; GrayscaleProcessor.cpp:8-9
void preprocess_geometry(const lvm_preprocess_params& pp, int w, int h, int channels, int* rx, int* ry, int* rw, int* rh,
                         int* ow, int* oh, int* och) {
    const int divisor = preprocess_divisor(pp);
    int x = 0, y = 0, cw = w, chh = h;
    if (pp.roi_enabled) {
        x = (int)std::lround((double)pp.roiX * w);
        y = (int)std::lround((double)pp.roiY * h);
        cw = (int)std::lround((double)pp.roiW * w);
        chh = (int)std::lround((double)pp.roiH * h);
        x = clampi(x, 0, w - 1); y = clampi(y, 0, h - 1);
        cw = clampi(cw, 1, w - x); chh = clampi(chh, 1, h - y);
    }
    *rx = x; *ry = y; *rw = cw; *rh = chh;
    *ow = divisor > 1 ? (cw / divisor > 1 ? cw / divisor : 1) : cw;
    *oh = divisor > 1 ? (chh / divisor > 1 ? chh / divisor : 1) : chh;
    *och = (pp.grayscale && channels != 1) ? 1 : channels;
}

// fractional source cells of one axis (OpenCV computeResizeAreaTab), plus the first entry of every output index
static void area_table(int ssize, int dsize, double scale, std::vector<AreaTab>& tab, std::vector<int>& first) {
    tab.clear(); first.assign((size_t)dsize + 1, 0);
    for (int dx = 0; dx < dsize; ++dx) {
        first[(size_t)dx] = (int)tab.size();
        const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        const double cell = std::min(scale, ssize - fsx1);
        int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
        sx2 = std::min(sx2, ssize - 1);
        sx1 = std::min(sx1, sx2);
        if (sx1 - fsx1 > 1e-3) tab.push_back({sx1 - 1, dx, (float)((sx1 - fsx1) / cell)});
        for (int sx = sx1; sx < sx2; ++sx) tab.push_back({sx, dx, (float)(1.0 / cell)});
        if (fsx2 - sx2 > 1e-3) tab.push_back({sx2, dx, (float)(std::min(std::min(fsx2 - sx2, 1.), cell) / cell)});
    }
    first[(size_t)dsize] = (int)tab.size();
}

struct PreTables {                       // cached per (roi size, output size)
    int rw = 0, rh = 0, ow = 0, oh = 0;
    AreaTab *xtab = nullptr, *ytab = nullptr; int *xk = nullptr, *yk = nullptr;
    void release() { for (void* p : {(void*)xtab, (void*)ytab, (void*)xk, (void*)yk}) if (p) (void)hipFree(p); xtab = ytab = nullptr; xk = yk = nullptr; rw = rh = ow = oh = 0; }
};

void preprocess_release(Ctx* c) {
    PreTables* t = static_cast<PreTables*>(c->pre_tables);
    if (t) { t->release(); delete t; c->pre_tables = nullptr; }
}

// one table of a geometry onto the device (synchronous: the launch that follows reads it)
template <class T>
static int table_upload(Ctx* c, T*& d, const std::vector<T>& host) {
    LVM_HIP_TRY(c, hipMalloc((void**)&d, host.size() * sizeof(T)));
    LVM_HIP_TRY(c, hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return LVM_OK;
}
// the fractional-cell tables of (rw x rh) -> (ow x oh), rebuilt when the geometry is another one than the cached tables'
static int area_tables(Ctx* c, int rw, int rh, int ow, int oh, hipStream_t s, PreTables** out) {
    PreTables* t = static_cast<PreTables*>(c->pre_tables);
    if (!t) { t = new PreTables(); c->pre_tables = t; }
    *out = t;
    if (t->rw == rw && t->rh == rh && t->ow == ow && t->oh == oh) return LVM_OK;
    LVM_HIP_TRY(c, hipStreamSynchronize(s));            // the old tables may still be in use
    t->release();
    std::vector<AreaTab> xt, yt; std::vector<int> xf, yf;
    area_table(rw, ow, (double)rw / ow, xt, xf);
    area_table(rh, oh, (double)rh / oh, yt, yf);
    int rc = table_upload(c, t->xtab, xt);
    if (rc == LVM_OK) rc = table_upload(c, t->ytab, yt);
    if (rc == LVM_OK) rc = table_upload(c, t->xk, xf);
    if (rc == LVM_OK) rc = table_upload(c, t->yk, yf);
    if (rc != LVM_OK) return rc;
    t->rw = rw; t->rh = rh; t->ow = ow; t->oh = oh;
    return LVM_OK;
}

int preprocess_device(Ctx* c, const lvm_preprocess_params& pp, const Image& in, const ImageOut& out, hipStream_t s, const ImageOut& tap, const RawSource* raw) {
    const int channels = in.cn;
    if (!in.p || !out.p || in.w <= 0 || in.h <= 0 || (channels != 1 && channels != 3)) { c->err = "preprocess: bad frame arguments"; return LVM_ERR_INVALID; }
    const int fmt = raw ? raw->fmt : LVM_PIX_BGR;
    if (fmt != LVM_PIX_BGR && (fmt < LVM_PIX_YUYV || fmt > LVM_PIX_NV21 || channels != 3)) { c->err = "preprocess: bad source format"; return LVM_ERR_INVALID; }
    int rx, ry, rw, rh, ow, oh, och;
    preprocess_geometry(pp, in.w, in.h, channels, &rx, &ry, &rw, &rh, &ow, &oh, &och);
    if (out.stride < (ptrdiff_t)ow * och) { c->err = "preprocess: output stride too small"; return LVM_ERR_INVALID; }
    PreArgs a{};
    a.in = in.p + (size_t)ry * in.stride + (size_t)rx * channels; a.in_stride = (long)in.stride; a.in_sstride = (long)in.sstride;
    a.out = out.p; a.out_stride = (long)out.stride; a.out_sstride = (long)out.sstride;
    a.ow = ow; a.oh = oh; a.cn = channels; a.ocn = och;
    a.tap = (channels == 3 && och == 1) ? tap.p : nullptr; a.tap_stride = (long)tap.stride; a.tap_sstride = (long)tap.sstride;
    int mode = 0;
    if (preprocess_divisor(pp) > 1) {
        // cv::resize(INTER_AREA): integer factors take resizeAreaFast_, anything else the fractional tables
        const double scx = (double)rw / ow, scy = (double)rh / oh;
        const int isx = (int)std::lrint(scx), isy = (int)std::lrint(scy);
        if (std::fabs(scx - isx) < 2.220446049250313e-16 && std::fabs(scy - isy) < 2.220446049250313e-16) {
            mode = 1; a.sx = isx; a.sy = isy;
        } else {
            mode = 2;
            PreTables* t = nullptr;
            const int rc = area_tables(c, rw, rh, ow, oh, s, &t);
            if (rc != LVM_OK) return rc;
            a.xtab = t->xtab; a.xk = t->xk; a.ytab = t->ytab; a.yk = t->yk;
        }
    }
    const dim3 grid((ow + 63) / 64, (oh + 3) / 4, c->nstreams), blk(256);
    if (fmt != LVM_PIX_BGR) {
        // the frame is raw: the ROI's origin in it, (X0, Y0), decides which pair / 2x2 block a pixel shares its chroma with
        const bool packed = fmt <= LVM_PIX_YVYU;
        const int X0 = rx + raw->px, Y0 = ry + raw->py;
        YuvSrc y{};
        y.x0 = X0 & 1; y.y0 = packed ? 0 : (Y0 & 1);
        if (packed) {
            a.in = in.p + (size_t)ry * in.stride + (size_t)(X0 >> 1) * 4;
        } else {
            a.in = in.p + (size_t)ry * in.stride + (size_t)(X0 & ~1);
            y.uv = in.p + raw->uv_offset + (size_t)(Y0 >> 1) * in.stride + (size_t)(X0 & ~1);
        }
        auto dword = [](const void* p, ptrdiff_t s0, ptrdiff_t s1) { return ((uintptr_t)p | (uintptr_t)s0 | (uintptr_t)s1) % 4 == 0; };
        const ptrdiff_t iss = c->nstreams > 1 ? in.sstride : 0, oss = c->nstreams > 1 ? out.sstride : 0;
        const bool vec = mode == 0 && och == 3 && y.x0 == 0 && ow % 4 == 0 && dword(a.in, in.stride, iss) && dword(y.uv, 0, 0) && dword(out.p, out.stride, oss);
        if (vec) {
            const dim3 grid4((ow / 4 + 63) / 64, (oh + 3) / 4, c->nstreams);
            auto k = lvm_pick([](auto f) { return k_yuv_vec4<decltype(f)::value>; }, PickYuv{fmt});
            LVM_LAUNCH_V(c, "preprocess", "yuv4", k, grid4, blk, s, a, y);
        } else {
            auto k = lvm_pick([](auto m, auto f) { return k_preprocess_yuv<decltype(m)::value, decltype(f)::value>; }, PickMode{mode}, PickYuv{fmt});
            LVM_LAUNCH_V(c, "preprocess", "yuv", k, grid, blk, s, a, y);
        }
    } else {
        auto k = lvm_pick([](auto m, auto three) { return k_preprocess<decltype(m)::value, decltype(three)::value ? 3 : 1>; }, PickMode{mode}, channels == 3);
        LVM_LAUNCH(c, "preprocess", k, grid, blk, s, a);
    }
    LVM_HIP_TRY(c, hipGetLastError());
    return LVM_OK;
}

}  // namespace lvm
