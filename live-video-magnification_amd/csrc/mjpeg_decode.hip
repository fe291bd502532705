// mjpeg_decode.hip -- Motion-JPEG decode onto the device (the decode half).
//
// Replaces what `cv::VideoCapture::read(frame)` does for an AVI / Motion-JPEG file (reference: source/FileSource.cpp:99): the compressed
// frames go up (a tenth of the pixels), the decoded BGR frames appear where the chain wants them -- in device memory.
// Accepted by default: ITU-T T.81 baseline sequential, 8 bit, three components sampled 2x2 / 1x1 / 1x1 (YCbCr 4:2:0, JFIF) in one scan, any quantiser and
// Huffman tables (frames without DHT get the Annex K tables, as AVI MJPEG implies), with or without restart intervals -- what this
// repository's encoder, libjpeg and FFmpeg's mjpeg encoder write.  Everything else is refused (LVM_ERR_INVALID), nothing is guessed.
// The entropy layer is exact by the standard; the arithmetic behind it is the decoder's choice and is restated line by line by
// oracle/mjpeg_oracle.py::decode_frame (all integer; its header has the formulas): the frames are BIT-identical to the oracle's, and within
// the bars of tests/test_mjpeg_decode.py of libjpeg's own decoder.
//
// Huffman decoding is serial inside a restart interval and nowhere else: a LANE per interval (k_mjd_huffman; 68 lanes per frame for this
// repository's streams, one for a stream without restart markers -- then the frames of the batch are the parallelism).
//   host              headers -> per-frame tables (quantisers, 9-bit look-up + canonical tables of the four Huffman codes)
//   k_mjd_intervals   RSTn markers of the entropy-coded segment -> start / end of every interval            one workgroup per frame
//   k_mjd_huffman     bits -> quantised coefficients (zigzag order, int16, zero-filled beforehand)           one lane per interval
//   k_mjd_pixels      dequantise, IDCT, chroma replication, YCbCr -> BGR                                      one wave per 16 x 16 MCU
// A context may ask for libjpeg's arithmetic behind the same entropy layer instead (lvm_mjpeg_set_decoder(ctx, LVM_MJPEG_DECODER_LIBJPEG)): the
// frames are then BYTE-identical to what libjpeg / libjpeg-turbo decode with their defaults (JDCT_ISLOW, do_fancy_upsampling) -- the decoder behind a
// libjpeg-backed cv::VideoCapture; tests/test_mjpeg_decode_libjpeg.py pins that against Pillow.  The triangle filter of the chroma planes reaches one
// sample into the neighbouring MCUs, so the pixel stage becomes two launches:
//   k_mjd_chroma_islow    dequantise + islow IDCT of the Cb and Cr blocks -> two u8 planes per frame (scratch)        one wave per four MCUs
//   k_mjd_pixels_libjpeg  dequantise + islow IDCT of the four Y blocks, h2v2 fancy upsampling, YCbCr -> BGR            one wave per 16 x 16 MCU
// The other samplings of a baseline Motion-JPEG file are accepted where the context's mask allows them (lvm_mjpeg_set_samplings; the default mask is
// 4:2:0 alone and leaves every refusal and message what it was): 4:2:2 (Y 2x1 -- UVC cameras, FFmpeg's yuvj422p), 4:4:4 and one component (b = g = r).
// The MCU is a property of the CALL (MjdSamp: all frames of a call share one sampling) -- 16 x 16 / 6 blocks, 16 x 8 / 4, 8 x 8 / 3, 8 x 8 / 1 -- and
// the entropy kernels walk its block list (nblk blocks, the first ny of them luminance); a one-component scan is not interleaved, its restart interval
// counts blocks.  These samplings have libjpeg's arithmetic only (the oracle defines none for them):
//   k_mjd_pixels_direct   4:4:4 and gray: islow IDCT of 3 x 8 (8) blocks, YCbCr -> BGR, no scratch planes                  one wave per eight 8 x 8 MCUs
//   k_mjd_chroma_islow + k_mjd_pixels_h2v1   4:2:2: the Cb / Cr planes, then islow IDCT of the Y blocks + h2v1 fancy upsampling     one wave per four 16 x 8 MCUs
// Still refused: progressive, arithmetic-coded, 12-bit, 4:4:0 / 4:1:1, four components.  tests/test_mjpeg_decode_samplings.py pins all of it against Pillow.
//
// The kernels are put together from one set of pieces:
//   lvm_internal.h     wg_inclusive_scan: the 256-thread scan inside k_mjd_intervals, k_mjp_unstuff, k_mjp_scan, k_mjp_dc (and the encoder's kernels)
//   entropy layer      mjd_stage_luts (the look-up tables into LDS), MjpExit (the exit word of a subsequence, packed and unpacked in one place),
//                      wg_chunked_scan (k_mjp_scan, k_mjp_dc: 1024 values at a time with a carry); k_mjp_sync keeps the parent's own staging and
//                      unpacking (measured: HISTORY.md, profiles/r10_mjpeg_decode_refactor_ab.txt)
//   pixel stage        MjdGeom (frame in MCUs, addresses of the chroma planes), mjd_chroma_word (the gather of the fancy upsamplers),
//                      mjl_idct_block / mjl_idct_block_inplace, mjd_store_bgr (YCbCr -> BGR, the one place with the constants)
//   host               mjd_layout ((w, h, sampling) -> MjdSamp + MjdGeom, made by begin, read by enqueue); MjdState owns every buffer as a DevBuf
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lvm_internal.h"
#include "mjpeg_tables.h"

namespace lvm {
namespace {

constexpr int MJD_LUT_BITS = 9;
struct MjdHuff {
    uint16_t lut[1 << MJD_LUT_BITS];    // (length << 8) | symbol for codes of up to 9 bits, 0 = longer
    int32_t maxcode[18];                // T.81 F.2.2.3, -1 where a length has no code; [17] = sentinel
    int32_t mincode[17];
    int32_t valptr[17];
    uint8_t vals[256];
};
struct MjdFrame {
    uint32_t data_off, data_len;        // the entropy-coded segment inside the uploaded bytes
    uint32_t restart;                   // MCUs per restart interval (0: the whole scan)
    uint32_t nintervals;                // expected
    uint32_t par;                       // 1: no restart markers -> decoded by the self-synchronising kernels (k_mjp_*), not a lane per interval
    uint32_t usub;                      // upper bound of its subsequences (from the stuffed length)
    uint32_t samp;                      // LVM_MJPEG_SAMPLING_* of the frame header
    uint32_t tq[3], td[3], ta[3];
    uint16_t q[4][64];                  // quantisers in ZIGZAG order
    uint8_t zz[64];                     // zigzag index -> natural position
    MjdHuff huff[2][2];                 // [class: 0 DC, 1 AC][id 0, 1]
};

// The MCU of a sampling: its size in pixels and its block list -- ny luminance blocks, then (three components) one Cb and one Cr block.
// A single-component scan is not interleaved (T.81 A.2.2): its "MCU" is one block, and the restart interval counts blocks.
struct MjdSamp { int mcu_w, mcu_h, nblk, ny, ncomp; const char* name; };
MjdSamp samp_of(uint32_t samp) {
    switch (samp) {
        case LVM_MJPEG_SAMPLING_422: return {16, 8, 4, 2, 3, "4:2:2"};
        case LVM_MJPEG_SAMPLING_444: return {8, 8, 3, 1, 3, "4:4:4"};
        case LVM_MJPEG_SAMPLING_GRAY: return {8, 8, 1, 1, 1, "gray"};
        default: return {16, 16, 6, 4, 3, "4:2:0"};
    }
}

// The frames of a call: size in pixels and in MCUs, the pitches of the BGR output.  The Cb / Cr planes between the two launches of 4:2:0 and 4:2:2 under
// the libjpeg kind are [frame][Cb, Cr][mh * 8][mw * 8] bytes: whole blocks, so that k_mjd_chroma_islow stores unconditionally.
struct MjdGeom {
    int w, h, mw, mh; long stride, fstride;
    __host__ __device__ int nmcu() const { return mw * mh; }
    __host__ __device__ size_t chroma_pitch() const { return (size_t)mw * 8; }
    __host__ __device__ size_t chroma_rows() const { return (size_t)mh * 8; }
    __host__ __device__ size_t chroma_row(int f, int comp, size_t y) const { return (((size_t)f * 2 + comp) * chroma_rows() + y) * chroma_pitch(); }     // byte offset; comp: 0 Cb, 1 Cr
};
// (w, h, sampling of the frame header) -> the MCU and the frames in MCUs; the pitches are the enqueue's
void mjd_layout(int w, int h, uint32_t samp, MjdSamp& sp, MjdGeom& g) {
    sp = samp_of(samp);
    g = MjdGeom{w, h, (w + sp.mcu_w - 1) / sp.mcu_w, (h + sp.mcu_h - 1) / sp.mcu_h, 0, 0};
}

// Every device buffer is an owning DevBuf: deleting the state frees them.
struct MjdState {
    uint32_t samp = 0;                   // the sampling sp and g were made for (0: none yet)
    MjdSamp sp{}; MjdGeom g{};           // of the current begin .. finish sequence
    DevBuf d_frames;                     // MjdFrame[n]
    DevBuf d_bytes;
    DevBuf d_coef;                       // int16_t[n][nmcu][nblk * 64]
    DevBuf d_err;                        // uint32_t: n error flags, then the n + 1 frame offsets
    DevBuf d_ivstart, d_ivend;           // uint32_t[n][max_iv]
    int n = 0, max_iv = 1;               // the frames of the current begin .. finish sequence, the most intervals one of them has
    // self-synchronising path (frames without restart markers)
    DevBuf d_ubytes;
    DevBuf d_ulen, d_before, d_changed;  // uint32_t[n], [n][sub_cap], [1]
    DevBuf d_exit[2];                    // unsigned long long[n][sub_cap]
    int sub_cap = 0;                     // (only grows: it is the grid of the k_mjp_* launches as well)
    // LVM_MJPEG_DECODER_LIBJPEG: the Cb / Cr planes between its two launches (MjdGeom::chroma_row)
    DevBuf d_chroma;
    int kind = 0;                        // the decoder kind of the current begin .. finish sequence
    std::vector<MjdFrame> frames;
    std::vector<uint32_t> foff;
};

int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// false: the code counts do not fit the code space (T.81 Annex C: at every length the codes assigned so far must leave room,
// code + bits[len] <= 2^len) -- an over-subscribed DHT would index past lut[]
bool build_decode_table(const uint8_t* bits, const uint8_t* vals, int nvals, MjdHuff& t) {
    std::memset(&t, 0, sizeof t);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        t.maxcode[len] = -1;
        if (code + (int)bits[len - 1] > (1 << len)) return false;
        if (bits[len - 1]) {
            t.valptr[len] = k; t.mincode[len] = code;
            for (int i = 0; i < bits[len - 1] && k < nvals; ++i, ++k, ++code) {
                if (len <= MJD_LUT_BITS)
                    for (int f = 0; f < (1 << (MJD_LUT_BITS - len)); ++f) t.lut[(code << (MJD_LUT_BITS - len)) | f] = (uint16_t)((len << 8) | vals[k]);
            }
            t.maxcode[len] = code - 1;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0x7FFFFFFF;
    for (int i = 0; i < nvals && i < 256; ++i) t.vals[i] = vals[i];
    return true;
}

// SOI .. SOS of one frame (oracle: parse_header).  Returns nullptr, or what is unsupported / malformed.
const char* parse_frame(const uint8_t* j, size_t n, int w, int h, unsigned mask, MjdFrame& f) {
    if (n < 4 || j[0] != 0xFF || j[1] != 0xD8) return "no SOI";
    bool have_q[4] = {false, false, false, false}, have_h[2][2] = {{false, false}, {false, false}}, sof = false;
    uint32_t cid[3] = {0, 0, 0};
    f.restart = 0;
    f.samp = LVM_MJPEG_SAMPLING_420;
    int nc = 3;
    for (int z = 0; z < 64; ++z) f.zz[z] = kZigzag[z];
    size_t i = 2;
    for (;;) {
        if (i + 4 > n || j[i] != 0xFF) return "marker expected";
        const int m = j[i + 1];
        if (m == 0xFF) { ++i; continue; }
        const size_t len = (size_t)be16(j + i + 2);
        if (len < 2 || i + 2 + len > n) return "segment runs past the frame";
        const uint8_t* p = j + i + 4;
        const size_t pn = len - 2;
        if (m == 0xDB) {
            for (size_t k = 0; k < pn; k += 65) {
                if (k + 65 > pn || (p[k] >> 4) || (p[k] & 15) > 3) return "quantiser table (16 bit or bad id)";
                for (int z = 0; z < 64; ++z) f.q[p[k] & 15][z] = p[k + 1 + z];
                have_q[p[k] & 15] = true;
            }
        } else if (m == 0xC4) {
            for (size_t k = 0; k < pn;) {
                if (k + 17 > pn) return "Huffman table";
                int nv = 0;
                for (int b = 0; b < 16; ++b) nv += p[k + 1 + b];
                const int cls = p[k] >> 4, id = p[k] & 15;
                if (cls > 1 || id > 1 || nv > 256 || k + 17 + (size_t)nv > pn) return "Huffman table (class / id / size)";
                if (!build_decode_table(p + k + 1, p + k + 17, nv, f.huff[cls][id])) return "Huffman table (code space)";
                have_h[cls][id] = true;
                k += 17 + (size_t)nv;
            }
        } else if (m == 0xC0) {
            // one component (its sampling factors mean nothing, T.81 A.2.2) where the mask of lvm_mjpeg_set_samplings allows it
            const bool gray = (mask & LVM_MJPEG_SAMPLING_GRAY) && pn >= 9 && p[0] == 8 && p[5] == 1;
            if (!gray && (pn < 15 || p[0] != 8 || p[5] != 3)) return "not 8-bit three-component";
            if (be16(p + 1) != h || be16(p + 3) != w) return "frame size differs from the call's";
            nc = gray ? 1 : 3;
            for (int c = 0; c < nc; ++c) { cid[c] = p[6 + 3 * c]; f.tq[c] = p[8 + 3 * c]; if (f.tq[c] > 3) return "quantiser id"; }
            if (gray) f.samp = LVM_MJPEG_SAMPLING_GRAY;
            else {
                const bool c11 = p[10] == 0x11 && p[13] == 0x11;
                f.samp = !c11 ? 0u : p[7] == 0x22 ? LVM_MJPEG_SAMPLING_420 : p[7] == 0x21 ? LVM_MJPEG_SAMPLING_422 : p[7] == 0x11 ? LVM_MJPEG_SAMPLING_444 : 0u;
                if (mask == LVM_MJPEG_SAMPLING_420) { if (f.samp != LVM_MJPEG_SAMPLING_420) return "sampling is not 4:2:0"; }
                else if (!f.samp) return "sampling is none of 4:2:0, 4:2:2, 4:4:4";
                else if (!(mask & f.samp)) return "sampling is not in the mask of lvm_mjpeg_set_samplings";
            }
            sof = true;
        } else if (m == 0xC1 || m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xCF && m != 0xC8 && m != 0xCC)) {
            return "not baseline sequential";
        } else if (m == 0xDD) {
            if (pn < 2) return "DRI";
            f.restart = (uint32_t)be16(p);
        } else if (m == 0xDA) {
            if (!sof || pn < 4 + 2 * (size_t)nc || p[0] != nc) return nc == 3 ? "scan without frame header / not three components" : "scan of a one-component frame with other components";
            for (int c = 0; c < nc; ++c) {
                if (p[1 + 2 * c] != cid[c]) return "scan component order";
                f.td[c] = p[2 + 2 * c] >> 4; f.ta[c] = p[2 + 2 * c] & 15;
                if (f.td[c] > 1 || f.ta[c] > 1) return "Huffman table id";
            }
            if (p[1 + 2 * nc] != 0 || p[2 + 2 * nc] != 63 || p[3 + 2 * nc] != 0) return "not a full baseline scan";        // Ss, Se, Ah | Al
            for (int c = 0; c < nc; ++c) if (!have_q[f.tq[c]]) return "quantiser table missing";
            // frames of an AVI may leave the Huffman tables out: the Annex K tables are implied
            if (!have_h[0][0]) build_decode_table(kDcLumaBits, kDcVals, 12, f.huff[0][0]);
            if (!have_h[1][0]) build_decode_table(kAcLumaBits, kAcLumaVals, 162, f.huff[1][0]);
            if (!have_h[0][1]) build_decode_table(kDcChromaBits, kDcVals, 12, f.huff[0][1]);
            if (!have_h[1][1]) build_decode_table(kAcChromaBits, kAcChromaVals, 162, f.huff[1][1]);
            size_t start = i + 2 + len, end = n;
            if (end >= start + 2 && j[end - 2] == 0xFF && j[end - 1] == 0xD9) end -= 2;      // EOI
            // (bit positions of a frame are 32-bit in the kernels: data_len * 8 must not wrap)
            if (end - start >= ((size_t)1 << 28)) return "entropy-coded segment of 256 MiB or more";
            f.data_off = (uint32_t)start; f.data_len = (uint32_t)(end - start);
            return nullptr;
        }
        i += 2 + len;
    }
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------------------

// One workgroup per frame: the k-th RSTn marker of the entropy-coded segment ends interval k and starts interval k + 1 (FF D0..D7 cannot
// occur inside the data: an FF byte of the data is followed by 00).
__global__ __launch_bounds__(256) void k_mjd_intervals(const uint8_t* __restrict__ bytes, const MjdFrame* __restrict__ frames, const uint32_t* __restrict__ foff,
                                                       uint32_t* __restrict__ ivstart, uint32_t* __restrict__ ivend, int iv_cap, uint32_t* __restrict__ err) {
    __shared__ uint32_t s_part[256];
    const int tid = threadIdx.x, f = blockIdx.x;
    const MjdFrame& fr = frames[f];
    const uint8_t* d = bytes + foff[f] + fr.data_off;
    const uint32_t n = fr.data_len;
    // a run of aligned 32-bit words per thread (+ the first byte of the next one: a marker may straddle two words)
    const uint32_t mis = (uint32_t)((uintptr_t)d & 3u);
    const uint32_t* wbase = reinterpret_cast<const uint32_t*>(d - mis);
    const uint32_t nwords = (n + mis + 3u) >> 2, per = (nwords + 255u) / 256u, lo = tid * per, hi = lo + per < nwords ? lo + per : nwords;
    auto scan = [&](auto&& hit) {
        if (lo >= hi) return;
        uint32_t w = wbase[lo];
        for (uint32_t i = lo; i < hi; ++i) {
            const uint32_t wn = wbase[i + 1];                                   // (the buffer is padded: always readable)
            const unsigned long long v = (unsigned long long)w | ((unsigned long long)wn << 32);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const long pos = (long)(4u * i + j) - (long)mis;                // byte position inside the segment
                const uint32_t b0 = (uint32_t)(v >> (8u * j)) & 0xFFu, b1 = (uint32_t)(v >> (8u * j + 8u)) & 0xFFu;
                if (pos >= 0 && pos + 1 < (long)n && b0 == 0xFFu && (b1 & 0xF8u) == 0xD0u) hit((uint32_t)pos);
            }
            w = wn;
        }
    };
    uint32_t cnt = 0;
    scan([&](uint32_t) { ++cnt; });
    wg_inclusive_scan(cnt, s_part, tid);
    uint32_t k = tid ? s_part[tid - 1] : 0u;
    uint32_t* st = ivstart + (size_t)f * iv_cap;
    uint32_t* en = ivend + (size_t)f * iv_cap;
    scan([&](uint32_t pos) {
        if (k + 1 < (uint32_t)iv_cap) { en[k] = pos; st[k + 1] = pos + 2; }
        ++k;
    });
    if (tid == 255) {
        const uint32_t total = s_part[255] + 1u;
        if (total != fr.nintervals) atomicOr(err + f, 1u);            // the markers do not match the restart interval of the header
        else { st[0] = 0; en[total - 1] = n; }
    }
}

// bit reader over `left` bytes from p: big-endian bits, FF 00 -> FF; behind the end the stream continues with 1-bits (a truncated interval
// decodes to something and reads nothing outside).  The bytes come in aligned 64-bit words, the next word always in flight: a lane's reads are
// a serial chain, and a byte-wise chain costs a memory latency per byte (1.85 ms per 1080p frame measured, against 0.1 with words).
struct MjdBits {
    const unsigned long long* wp;       // the word after `nxt`
    unsigned long long cur, nxt;        // bytes are consumed from the low end of cur
    int nb;                             // bytes left in cur
    long left;                          // bytes left in the interval
    uint32_t acc; int cnt;              // the next bits are the top `cnt` bits of acc
    __device__ __forceinline__ void init(const uint8_t* base, uint32_t start, uint32_t end) {
        const uint8_t* a = base + start;
        const unsigned mis = (unsigned)((uintptr_t)a & 7u);
        wp = reinterpret_cast<const unsigned long long*>(a - mis);
        cur = *wp++ >> (8u * mis); nb = 8 - (int)mis;
        nxt = *wp++;
        left = (long)end - (long)start;
        acc = 0; cnt = 0;
    }
    __device__ __forceinline__ void advance() { cur = nxt; nxt = *wp++; nb = 8; }
    __device__ __forceinline__ void fill() {
        while (cnt <= 24) {
            uint32_t b = 0xFFu;
            if (left > 0) {
                if (nb == 0) advance();
                b = (uint32_t)cur & 0xFFu; cur >>= 8; --nb; --left;
                if (b == 0xFFu && left > 0) {               // a stuffed zero behind it is dropped
                    if (nb == 0) advance();
                    if (((uint32_t)cur & 0xFFu) == 0u) { cur >>= 8; --nb; --left; }
                }
            }
            acc |= b << (24 - cnt);
            cnt += 8;
        }
    }
    __device__ __forceinline__ uint32_t peek(int n) const { return acc >> (32 - n); }
    __device__ __forceinline__ void skip(int n) { acc <<= n; cnt -= n; }
    __device__ __forceinline__ uint32_t get(int n) { if (n == 0) return 0u; fill(); const uint32_t v = peek(n); skip(n); return v; }
};

// one Huffman symbol (T.81 F.2.2.3); -1 = no such code.  (mjp_symbol below is its twin over the other bit reader; why they stay two: HISTORY.md)
__device__ __forceinline__ int mjd_symbol(MjdBits& br, const uint16_t* lut, const MjdHuff& t) {
    br.fill();
    const uint32_t e = lut[br.peek(MJD_LUT_BITS)];
    if (e) { br.skip((int)(e >> 8)); return (int)(e & 255u); }
    int code = (int)br.peek(MJD_LUT_BITS);
    for (int len = MJD_LUT_BITS + 1; len <= 16; ++len) {
        code = (int)br.peek(len);
        if (t.maxcode[len] >= 0 && code <= t.maxcode[len] && code >= t.mincode[len]) { br.skip(len); return t.vals[t.valptr[len] + code - t.mincode[len]]; }
    }
    return -1;
}
// the four 9-bit look-up tables of a frame into LDS, by the 64 lanes of a workgroup (ends with a barrier)
typedef uint16_t MjdLuts[2][2][1 << MJD_LUT_BITS];
__device__ __forceinline__ void mjd_stage_luts(MjdLuts& s_lut, const MjdFrame& fr, int tid) {
    for (int i = tid; i < 4 << MJD_LUT_BITS; i += 64) s_lut[i >> (MJD_LUT_BITS + 1)][(i >> MJD_LUT_BITS) & 1][i & ((1 << MJD_LUT_BITS) - 1)] =
        fr.huff[i >> (MJD_LUT_BITS + 1)][(i >> MJD_LUT_BITS) & 1].lut[i & ((1 << MJD_LUT_BITS) - 1)];
    __syncthreads();
}
__device__ __forceinline__ int mjd_extend(uint32_t v, int s) { return (s == 0 || v >= (1u << (s - 1))) ? (int)v : (int)v - (1 << s) + 1; }

// A lane per restart interval; the 64 lanes of a workgroup are consecutive intervals of ONE frame, whose look-up tables sit in LDS.
__global__ __launch_bounds__(64) void k_mjd_huffman(const uint8_t* __restrict__ bytes, const MjdFrame* __restrict__ frames, const uint32_t* __restrict__ foff,
                                                    const uint32_t* __restrict__ ivstart, const uint32_t* __restrict__ ivend, int iv_cap, int nmcu,
                                                    int nblk, int ny, int16_t* __restrict__ coef, uint32_t* __restrict__ err) {
    __shared__ MjdLuts s_lut;
    const int f = blockIdx.y, tid = threadIdx.x;
    const MjdFrame& fr = frames[f];
    mjd_stage_luts(s_lut, fr, tid);
    const uint32_t k = blockIdx.x * 64u + (uint32_t)tid;
    if (k >= fr.nintervals || err[f] || fr.par) return;
    const uint8_t* d = bytes + foff[f] + fr.data_off;
    MjdBits br;
    br.init(d, ivstart[(size_t)f * iv_cap + k], ivend[(size_t)f * iv_cap + k]);
    const uint32_t ri = fr.restart ? fr.restart : (uint32_t)nmcu;
    const uint32_t m0 = k * ri, m1 = m0 + ri < (uint32_t)nmcu ? m0 + ri : (uint32_t)nmcu;
    int pred[3] = {0, 0, 0};
    bool bad = false;
    for (uint32_t m = m0; m < m1 && !bad; ++m) {
        int16_t* out = coef + ((size_t)f * nmcu + m) * (size_t)(nblk * 64);
        for (int bi = 0; bi < nblk && !bad; ++bi) {
            const int comp = bi < ny ? 0 : bi - ny + 1;
            const uint32_t td = fr.td[comp], ta = fr.ta[comp];
            int s = mjd_symbol(br, s_lut[0][td], fr.huff[0][td]);
            if (s < 0 || s > 11) { bad = true; break; }
            pred[comp] += mjd_extend(br.get(s), s);
            out[bi * 64] = (int16_t)pred[comp];
            for (int kk = 1; kk < 64;) {
                const int rs = mjd_symbol(br, s_lut[1][ta], fr.huff[1][ta]);
                if (rs < 0) { bad = true; break; }
                const int r = rs >> 4;
                s = rs & 15;
                if (s == 0) { if (r != 15) break; kk += 16; continue; }
                kk += r;
                if (kk > 63) { bad = true; break; }
                out[bi * 64 + kk] = (int16_t)mjd_extend(br.get(s), s);
                ++kk;
            }
        }
    }
    if (bad) atomicOr(err + f, 2u);
}

// ---- streams WITHOUT restart markers: self-synchronising parallel decoding ------------------------------------------------------------------
// A Huffman decoder that starts inside a stream at a wrong position almost always falls into step with the true code word boundaries after a
// few symbols (the codes are not fixed-length and the run / size symbols keep re-aligning it).  So (Klein & Wiseman 2003; Weissenberger &
// Schmidt 2018 for JPEG on GPUs): cut the unstuffed entropy segment into subsequences of 1024 bits, a lane each;
//   k_mjp_unstuff   FF 00 -> FF, so that bit positions are plain arithmetic
//   k_mjp_sync      lane i decodes subsequence i from where -- and in the state (block of the MCU, coefficient index) in which -- lane i - 1
//                   last left ITS subsequence, and publishes its own exit (position, state, blocks completed).  First pass: every lane
//                   guesses (start of its subsequence, start of an MCU).  Repeated until no exit changes: lane 0's entry is exact, hence by
//                   induction every lane's.  Code word boundaries are found again within a few symbols, the position inside the MCU (the four
//                   luminance blocks of 4:2:0 share their tables; two do in 4:2:2, none in 4:4:4, gray has no position) takes longer -- hence the look-back of the first pass (8 subsequences): 6 / 16 / 29 changing passes for 102 / 581 / 1 116 subsequences
//                   without it, 0 / 2 / 7 with it.
//   k_mjp_scan      blocks completed before every lane (prefix sum)
//   k_mjp_write     the same decoding once more from the exact entries, now storing coefficients (DC as differences)
//   k_mjp_dc        DC prediction: prefix sums over the blocks of each component
// The result is what the one-lane decoder produces (same tables, same rules), the tests compare both with the oracle.
constexpr uint32_t MJP_SUB_BITS = 1024;
#ifndef MJP_LOOKBACK_N
#define MJP_LOOKBACK_N 8
#endif
constexpr uint32_t MJP_LOOKBACK = MJP_LOOKBACK_N;
struct MjpBits {
    const uint32_t* w; uint32_t nwords, next;
    unsigned long long acc; int cnt;
    uint32_t pos;
    __device__ __forceinline__ uint32_t word(uint32_t i) const { return i < nwords ? __builtin_bswap32(w[i]) : 0xFFFFFFFFu; }     // behind the end: 1-bits
    __device__ __forceinline__ void init(const uint32_t* words, uint32_t n, uint32_t p0) {
        w = words; nwords = n; pos = p0;
        const uint32_t i = p0 >> 5, sh = p0 & 31u;
        acc = (((unsigned long long)word(i) << 32) | word(i + 1)) << sh;
        cnt = 64 - (int)sh; next = i + 2;
    }
    __device__ __forceinline__ void fill() { if (cnt <= 32) { acc |= (unsigned long long)word(next++) << (32 - cnt); cnt += 32; } }
    __device__ __forceinline__ uint32_t peek(int n) const { return (uint32_t)(acc >> (64 - n)); }
    __device__ __forceinline__ void skip(int n) { acc <<= n; cnt -= n; pos += (uint32_t)n; }
    __device__ __forceinline__ uint32_t get(int n) { if (n == 0) return 0u; fill(); const uint32_t v = peek(n); skip(n); return v; }
};
__device__ __forceinline__ int mjp_symbol(MjpBits& br, const uint16_t* lut, const MjdHuff& t) {
    br.fill();
    const uint32_t e = lut[br.peek(MJD_LUT_BITS)];
    if (e) { br.skip((int)(e >> 8)); return (int)(e & 255u); }
    for (int len = MJD_LUT_BITS + 1; len <= 16; ++len) {
        const int code = (int)br.peek(len);
        if (t.maxcode[len] >= 0 && code <= t.maxcode[len] && code >= t.mincode[len]) { br.skip(len); return t.vals[t.valptr[len] + code - t.mincode[len]]; }
    }
    return -1;
}
// One symbol in state (bi = block of the MCU, kk = next coefficient index; kk == 0: a DC code comes next).  Returns the zigzag index of the
// coefficient it produced (`value`), -1 for a symbol without one, -2 for what the one-lane decoder calls an error.  `done` = the block ended.
__device__ __forceinline__ int mjp_step(MjpBits& br, int& bi, int& kk, const MjdFrame& fr, const MjdLuts& s_lut, int nblk, int ny, int& value, bool& done) {
    const int comp = bi < ny ? 0 : bi - ny + 1;
    int ci = -1;
    done = false;
    if (kk == 0) {
        const uint32_t td = fr.td[comp];
        const int s = mjp_symbol(br, s_lut[0][td], fr.huff[0][td]);
        if (s < 0 || s > 11) return -2;
        value = mjd_extend(br.get(s), s);
        ci = 0; kk = 1;
    } else {
        const uint32_t ta = fr.ta[comp];
        const int rs = mjp_symbol(br, s_lut[1][ta], fr.huff[1][ta]);
        if (rs < 0) return -2;
        const int r = rs >> 4, s = rs & 15;
        if (s == 0) {
            if (r == 15) kk += 16; else kk = 64;                 // ZRL / EOB
        } else {
            if (kk + r > 63) return -2;                          // (the state stays what it was: the caller may go on from here)
            kk += r;
            value = mjd_extend(br.get(s), s);
            ci = kk; ++kk;
        }
    }
    if (kk >= 64) { kk = 0; bi = bi == nblk - 1 ? 0 : bi + 1; done = true; }
    return ci;
}

// one workgroup per frame: the entropy-coded segment without its stuffed zeros, from a 4-byte aligned address, + its length
__global__ __launch_bounds__(256) void k_mjp_unstuff(const uint8_t* __restrict__ bytes, const MjdFrame* __restrict__ frames, const uint32_t* __restrict__ foff,
                                                     uint8_t* __restrict__ ubytes, uint32_t* __restrict__ ulen) {
    __shared__ uint32_t s_part[256];
    const int tid = threadIdx.x, f = blockIdx.x;
    const MjdFrame& fr = frames[f];
    if (!fr.par) return;
    const uint32_t o = foff[f] + fr.data_off, n = fr.data_len;
    const uint8_t* d = bytes + o;
    uint8_t* u = ubytes + ((o + 3u) & ~3u);
    const uint32_t per = (n + 255u) / 256u, lo = tid * per, hi = lo + per < n ? lo + per : n;
    uint32_t keep = 0;
    for (uint32_t i = lo; i < hi; ++i) keep += (d[i] == 0 && i > 0 && d[i - 1] == 0xFF) ? 0u : 1u;
    wg_inclusive_scan(keep, s_part, tid);
    uint32_t k = tid ? s_part[tid - 1] : 0u;
    for (uint32_t i = lo; i < hi; ++i) if (!(d[i] == 0 && i > 0 && d[i - 1] == 0xFF)) u[k++] = d[i];
    const uint32_t total = s_part[255];
    if (tid < 8) u[total + tid] = 0xFF;                          // (the word readers look a little ahead)
    if (tid == 0) ulen[f] = total;
}

// exit of a subsequence as the 64-bit word the passes exchange: the bit position in the low half; above it the state (bi * 64 + kk, 9 bits) and the
// blocks completed on the way
struct MjpExit {
    uint32_t pos; int bi, kk; uint32_t blocks;
    __device__ __forceinline__ unsigned long long pack() const { return (unsigned long long)pos | ((unsigned long long)(bi * 64 + kk) << 32) | ((unsigned long long)blocks << 41); }
    __device__ __forceinline__ static MjpExit unpack(unsigned long long e) {
        const int st = (int)((e >> 32) & 511u);
        return {(uint32_t)e, st >> 6, st & 63, (uint32_t)(e >> 41)};
    }
};

__global__ __launch_bounds__(64) void k_mjp_sync(const uint8_t* __restrict__ ubytes, const MjdFrame* __restrict__ frames, const uint32_t* __restrict__ foff,
                                                 const uint32_t* __restrict__ ulen, int sub_cap, int first, int nblk, int ny, const unsigned long long* __restrict__ ein,
                                                 unsigned long long* __restrict__ eout, uint32_t* __restrict__ changed) {
    __shared__ uint16_t s_lut[2][2][1 << MJD_LUT_BITS];
    const int f = blockIdx.y, tid = threadIdx.x;
    const MjdFrame& fr = frames[f];
    for (int i = tid; i < 4 << MJD_LUT_BITS; i += 64) s_lut[i >> (MJD_LUT_BITS + 1)][(i >> MJD_LUT_BITS) & 1][i & ((1 << MJD_LUT_BITS) - 1)] =
        fr.huff[i >> (MJD_LUT_BITS + 1)][(i >> MJD_LUT_BITS) & 1].lut[i & ((1 << MJD_LUT_BITS) - 1)];
    __syncthreads();
    if (!fr.par) return;
    const uint32_t total_bits = ulen[f] * 8u, nsub = (total_bits + MJP_SUB_BITS - 1) / MJP_SUB_BITS, i = blockIdx.x * 64u + (uint32_t)tid;
    if (i >= nsub) return;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(ubytes + ((foff[f] + fr.data_off + 3u) & ~3u));
    // first pass: the guess starts MJP_LOOKBACK subsequences EARLIER (start of an MCU assumed there) and runs up to the lane's own
    // subsequence: by then it has usually fallen into step with the code words and with the blocks of the MCU, so that most lanes are
    // exact after this pass already and the later passes only repair the chains of lanes that were not
    uint32_t p0 = first ? (i > MJP_LOOKBACK ? (i - MJP_LOOKBACK) * MJP_SUB_BITS : 0u) : i * MJP_SUB_BITS;
    int bi = 0, kk = 0;
    if (!first && i > 0) { const unsigned long long e = ein[(size_t)f * sub_cap + i - 1]; p0 = (uint32_t)e; const int st = (int)((e >> 32) & 511u); bi = st >> 6; kk = st & 63; }
    const uint32_t end = (i + 1) * MJP_SUB_BITS < total_bits ? (i + 1) * MJP_SUB_BITS : total_bits;
    MjpBits br;
    br.init(words, (ulen[f] + 3u) >> 2, p0);
    if (first) {
        const uint32_t own = i * MJP_SUB_BITS;
        while (br.pos < own) {
            int value; bool done;
            if (mjp_step(br, bi, kk, fr, s_lut, nblk, ny, value, done) == -2) br.skip(1);
        }
    }
    uint32_t blocks = 0;
    while (br.pos < end) {
        int value; bool done;
        if (mjp_step(br, bi, kk, fr, s_lut, nblk, ny, value, done) == -2) { br.skip(1); continue; }     // (a wrong guess runs into impossible codes: move on)
        blocks += done ? 1u : 0u;
    }
    const unsigned long long e = MjpExit{br.pos, bi, kk, blocks}.pack();
    if (first || e != ein[(size_t)f * sub_cap + i]) { if (!first) atomicOr(changed, 1u); }
    eout[(size_t)f * sub_cap + i] = e;
}

// n values in chunks of 1024 with a carry, by one workgroup of 256 threads: put(i, the sum of get(0 .. i), get(i)) for every i < n_all.  s_v: 1024 elements of LDS,
// s_part: 256, s_carry: one.
template <class T, class Get, class Put>
__device__ __forceinline__ void wg_chunked_scan(int n_all, T* s_v, T* s_part, T* s_carry, int tid, Get get, Put put) {
    if (tid == 0) *s_carry = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n_all; c0 += 1024) {
        const int n = n_all - c0 < 1024 ? n_all - c0 : 1024;
        for (int i = tid; i < n; i += 256) s_v[i] = get(c0 + i);
        __syncthreads();
        const int per = (n + 255) / 256, lo = tid * per, hi = lo + per < n ? lo + per : n;          // a run of the chunk per thread
        T sum = 0;
        for (int i = lo; i < hi; ++i) sum += s_v[i];
        wg_inclusive_scan(sum, s_part, tid);
        const T carry = *s_carry;
        T run = carry + (tid ? s_part[tid - 1] : T(0));
        for (int i = lo; i < hi; ++i) { put(c0 + i, run, s_v[i]); run += s_v[i]; }
        __syncthreads();
        if (tid == 0) *s_carry = carry + s_part[255];
        __syncthreads();
    }
}

// one workgroup per frame: blocks completed before every subsequence
__global__ __launch_bounds__(256) void k_mjp_scan(const MjdFrame* __restrict__ frames, const uint32_t* __restrict__ ulen, int sub_cap, const unsigned long long* __restrict__ e,
                                                  uint32_t* __restrict__ before) {
    __shared__ uint32_t s_v[1024];
    __shared__ uint32_t s_part[256];
    __shared__ uint32_t s_carry;
    const int tid = threadIdx.x, f = blockIdx.x;
    if (!frames[f].par) return;
    const int nsub = (int)((ulen[f] * 8u + MJP_SUB_BITS - 1) / MJP_SUB_BITS);
    wg_chunked_scan(nsub, s_v, s_part, &s_carry, tid, [&](int i) { return MjpExit::unpack(e[(size_t)f * sub_cap + i]).blocks; },
                    [&](int i, uint32_t sum, uint32_t) { before[(size_t)f * sub_cap + i] = sum; });
}

__global__ __launch_bounds__(64) void k_mjp_write(const uint8_t* __restrict__ ubytes, const MjdFrame* __restrict__ frames, const uint32_t* __restrict__ foff,
                                                  const uint32_t* __restrict__ ulen, int sub_cap, const unsigned long long* __restrict__ e, const uint32_t* __restrict__ before,
                                                  int nmcu, int nblk, int ny, int16_t* __restrict__ coef, uint32_t* __restrict__ err) {
    __shared__ MjdLuts s_lut;
    const int f = blockIdx.y, tid = threadIdx.x;
    const MjdFrame& fr = frames[f];
    mjd_stage_luts(s_lut, fr, tid);
    if (!fr.par) return;
    const uint32_t total_bits = ulen[f] * 8u, nsub = (total_bits + MJP_SUB_BITS - 1) / MJP_SUB_BITS, i = blockIdx.x * 64u + (uint32_t)tid;
    if (i >= nsub) return;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(ubytes + ((foff[f] + fr.data_off + 3u) & ~3u));
    uint32_t p0 = 0;
    int bi = 0, kk = 0;
    if (i > 0) { const MjpExit x = MjpExit::unpack(e[(size_t)f * sub_cap + i - 1]); p0 = x.pos; bi = x.bi; kk = x.kk; }
    const bool last = i + 1 == nsub;
    const uint32_t end = last ? total_bits + 64u : MjpExit::unpack(e[(size_t)f * sub_cap + i]).pos;
    const uint32_t nall = (uint32_t)nmcu * (uint32_t)nblk;
    uint32_t b = before[(size_t)f * sub_cap + i];
    bool bad = (uint32_t)bi != b % (uint32_t)nblk;                                   // (the state and the count must tell the same story)
    MjpBits br;
    br.init(words, (ulen[f] + 3u) >> 2, p0);
    int16_t* out = coef + (size_t)f * nmcu * (size_t)(nblk * 64);
    while (!bad && b < nall && br.pos < end) {
        int value = 0; bool done;
        const int ci = mjp_step(br, bi, kk, fr, s_lut, nblk, ny, value, done);
        if (ci == -2) { bad = true; break; }
        if (ci >= 0) out[(size_t)b * 64 + ci] = (int16_t)value;
        b += done ? 1u : 0u;
    }
    if (last && b < nall) bad = true;                                     // the stream ended before the frame did
    if (bad) atomicOr(err + f, 2u);
}

// one workgroup per (component, frame): DC coefficients = prefix sums of the differences over the blocks of the component, in scan order
__global__ __launch_bounds__(256) void k_mjp_dc(const MjdFrame* __restrict__ frames, int nmcu, int nblk, int ny, int16_t* __restrict__ coef) {
    __shared__ int s_v[1024];
    __shared__ int s_part[256];
    __shared__ int s_carry;
    const int tid = threadIdx.x, comp = blockIdx.x, f = blockIdx.y;
    if (!frames[f].par) return;
    int16_t* c = coef + (size_t)f * nmcu * (size_t)(nblk * 64);
    const int n_all = comp == 0 ? nmcu * ny : nmcu;
    // element el of the component -> its block: the ny luminance blocks lead every MCU, Cb and Cr follow
    auto block_of = [&](int el) { return comp == 0 ? (el / ny) * nblk + el % ny : el * nblk + ny + comp - 1; };
    wg_chunked_scan(n_all, s_v, s_part, &s_carry, tid, [&](int i) { return (int)c[(size_t)block_of(i) * 64]; },
                    [&](int i, int sum, int v) { c[(size_t)block_of(i) * 64] = (int16_t)(sum + v); });
}

// the (Cb | Cr << 16) word of the sample x columns and y rows from cb, a position in a frame's Cb plane; x clamped to the COMPONENT's own width cw: its
// edge samples are what libjpeg's fancy upsampling replicates, not the padding of the MCUs
__device__ __forceinline__ uint32_t mjd_chroma_word(const uint8_t* __restrict__ cb, const MjdGeom& g, int y, int x, int cw) {
    x = x < 0 ? 0 : (x > cw - 1 ? cw - 1 : x);
    const size_t o = (size_t)y * g.chroma_pitch() + (size_t)x;
    return (uint32_t)cb[o] | ((uint32_t)cb[g.chroma_row(0, 1, 0) + o] << 16);
}
// JFIF YCbCr (samples 0..255) -> the three bytes of a BGR pixel, 16-bit fixed point with rounding, clamped: both kinds' last step
__device__ __forceinline__ void mjd_store_bgr(uint8_t* o, int y, int cb, int cr) {
    cb -= 128; cr -= 128;
    int r = y + ((91881 * cr + 32768) >> 16), g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16), b = y + ((116130 * cb + 32768) >> 16);
    r = r < 0 ? 0 : (r > 255 ? 255 : r); g = g < 0 ? 0 : (g > 255 ? 255 : g); b = b < 0 ? 0 : (b > 255 ? 255 : b);
    o[0] = (uint8_t)b; o[1] = (uint8_t)g; o[2] = (uint8_t)r;
}

// One wave per MCU (four per workgroup): dequantise + un-zigzag (lane = zigzag index), IDCT (48 of the 64 lanes: a column / row of one of
// the six blocks each), then lane = one 2 x 2 pixel quad with its replicated chroma sample -> four BGR pixels.
__global__ __launch_bounds__(256) void k_mjd_pixels(const int16_t* __restrict__ coef, const MjdFrame* __restrict__ frames, MjdGeom g, uint8_t* __restrict__ dst) {
    __shared__ int s_a[4][6][64], s_b[4][6][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int mx = blockIdx.x * 4 + wave, my = blockIdx.y, f = blockIdx.z;
    const bool act = mx < g.mw;
    const MjdFrame& fr = frames[f];
    if (act) {
        const int16_t* in = coef + (((size_t)f * g.mh + my) * g.mw + mx) * 384;
        const int nat = fr.zz[lane];
#pragma unroll
        for (int blk = 0; blk < 6; ++blk) {
            const int q = fr.q[fr.tq[blk < 4 ? 0 : blk - 3]][lane];
            int v = in[blk * 64 + lane] * q;
            v = v < -4096 ? -4096 : (v > 4095 ? 4095 : v);
            s_a[wave][blk][nat] = v;
        }
    }
    __syncthreads();
    if (act && lane < 48) {               // columns: t[y][u] = (sum_v M[v][y] S[v][u] + 512) >> 10
        const int blk = lane >> 3, u = lane & 7;
        int d[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) d[v] = s_a[wave][blk][v * 8 + u];
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            int acc = 0;
#pragma unroll
            for (int v = 0; v < 8; ++v) acc += kDct[v][y] * d[v];
            s_b[wave][blk][y * 8 + u] = (acc + 512) >> 10;
        }
    }
    __syncthreads();
    if (act && lane < 48) {               // rows: s[y][x] = (sum_u M[u][x] t[y][u] + 32768) >> 16; + 128; clamp
        const int blk = lane >> 3, y = lane & 7;
        int d[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) d[u] = s_b[wave][blk][y * 8 + u];
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            int acc = 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += kDct[u][x] * d[u];
            int p = ((acc + 32768) >> 16) + 128;
            s_a[wave][blk][y * 8 + x] = p < 0 ? 0 : (p > 255 ? 255 : p);
        }
    }
    __syncthreads();
    if (act) {
        const int qx = lane & 7, qy = lane >> 3;
        const int cb = s_a[wave][4][lane], cr = s_a[wave][5][lane];
        uint8_t* fr_out = dst + (size_t)f * g.fstride;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int ly = 2 * qy + dy, py = my * 16 + ly;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int lx = 2 * qx + dx, px = mx * 16 + lx;
                if (py < g.h && px < g.w)
                    mjd_store_bgr(fr_out + (size_t)py * g.stride + (size_t)px * 3, s_a[wave][(ly >> 3) * 2 + (lx >> 3)][(ly & 7) * 8 + (lx & 7)], cb, cr);
            }
        }
    }
}


// ---- LVM_MJPEG_DECODER_LIBJPEG: jpeg_idct_islow + h2v2_fancy_upsample (libjpeg jidctint.c / jdsample.c), all integer ---------------------------
// LDS images of 8 x 8 blocks: row pitch 9, block pitch 72.  A lane of the IDCT passes is (block, column) and then (block, row): with a pitch of 8
// the row pass puts the 32 lanes of a bank group on 4 banks (8-way); with 9 both passes, the stores in between and the 2 x 2 quads' reads
// of the luminance are conflict-free or 2-way.
constexpr int MJL_ROW = 9, MJL_BLK = 72;

// One 1-D pass (CONST_BITS = 13): in[0..8) -> out[0..8), descaled by `shift` (11 behind the column pass: CONST_BITS - PASS1_BITS; 18 behind the
// row pass: CONST_BITS + PASS1_BITS + 3).  Wrap-around unsigned arithmetic, the shift arithmetic on the reinterpreted value: equal to libjpeg
// wherever libjpeg itself does not overflow (every stream an encoder makes from 8-bit samples), defined behaviour on everything else.
__device__ __forceinline__ void mjl_islow_1d(const int* in, int* out, int shift) {
    typedef uint32_t U;
    const U i0 = (U)in[0], i1 = (U)in[1], i2 = (U)in[2], i3 = (U)in[3], i4 = (U)in[4], i5 = (U)in[5], i6 = (U)in[6], i7 = (U)in[7];
    U z1 = (i2 + i6) * 4433u;
    const U tmp2 = z1 - i6 * 15137u, tmp3 = z1 + i2 * 6270u;
    const U tmp0 = (i0 + i4) << 13, tmp1 = (i0 - i4) << 13;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    U t0 = i7, t1 = i5, t2 = i3, t3 = i1;
    z1 = t0 + t3;
    U z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const U z5 = (z3 + z4) * 9633u;
    t0 *= 2446u; t1 *= 16819u; t2 *= 25172u; t3 *= 12299u;
    z1 *= (U)-7373; z2 *= (U)-20995;
    z3 = z3 * (U)-16069 + z5; z4 = z4 * (U)-3196 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    const U r = 1u << (shift - 1);
    out[0] = (int)(tmp10 + t3 + r) >> shift; out[7] = (int)(tmp10 - t3 + r) >> shift;
    out[1] = (int)(tmp11 + t2 + r) >> shift; out[6] = (int)(tmp11 - t2 + r) >> shift;
    out[2] = (int)(tmp12 + t1 + r) >> shift; out[5] = (int)(tmp12 - t1 + r) >> shift;
    out[3] = (int)(tmp13 + t0 + r) >> shift; out[4] = (int)(tmp13 - t0 + r) >> shift;
}
// dequantised coefficients of a block at a[] (natural order) -> samples 0..255 in p[8] of the lane's row k; t[] is the image between the passes.
// Called by all lanes of a workgroup (two barriers); `on` = this lane has a column / row to do.
__device__ __forceinline__ void mjl_idct_block(const int* a, int* t, bool on, int k, int* p) {
    int d[8], o[8];
    if (on) {               // columns: lane = u
#pragma unroll
        for (int v = 0; v < 8; ++v) d[v] = a[v * MJL_ROW + k];
        mjl_islow_1d(d, o, 11);
#pragma unroll
        for (int y = 0; y < 8; ++y) t[y * MJL_ROW + k] = o[y];
    }
    __syncthreads();
    if (on) {               // rows: lane = y
#pragma unroll
        for (int u = 0; u < 8; ++u) d[u] = t[k * MJL_ROW + u];
        mjl_islow_1d(d, o, 18);
#pragma unroll
        for (int x = 0; x < 8; ++x) { const int s = o[x] + 128; p[x] = s < 0 ? 0 : (s > 255 ? 255 : s); }
    }
    __syncthreads();
}

// ... in place: the lane's row of samples goes back into the block's own row of a[] (the callers put a barrier behind it)
__device__ __forceinline__ void mjl_idct_block_inplace(int* a, int* t, bool on, int k) {
    int p[8];
    mjl_idct_block(a, t, on, k, p);
    if (on) {
#pragma unroll
        for (int x = 0; x < 8; ++x) a[k * MJL_ROW + x] = p[x];
    }
}

// One wave per four MCUs of an MCU row (sixteen per workgroup): lane = zigzag index while dequantising (coef * q, no clamp -- libjpeg has none), then
// (block, column / row) of the eight Cb / Cr blocks; every row of a block leaves as one 8-byte store into its plane.
__global__ __launch_bounds__(256) void k_mjd_chroma_islow(const int16_t* __restrict__ coef, const MjdFrame* __restrict__ frames, MjdGeom g, int nblk, int ny, uint8_t* __restrict__ planes) {
    __shared__ int s_a[4][8 * MJL_BLK], s_b[4][8 * MJL_BLK];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int mx0 = blockIdx.x * 16 + wave * 4, my = blockIdx.y, f = blockIdx.z;
    const MjdFrame& fr = frames[f];
    const int nat = fr.zz[lane], at = (nat >> 3) * MJL_ROW + (nat & 7);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int mx = mx0 + (b >> 1), comp = 1 + (b & 1);
        if (mx < g.mw) s_a[wave][b * MJL_BLK + at] = coef[(((size_t)f * g.mh + my) * g.mw + mx) * (size_t)(nblk * 64) + (ny - 1 + comp) * 64 + lane] * (int)fr.q[fr.tq[comp]][lane];
    }
    __syncthreads();
    const int b = lane >> 3, k = lane & 7, mx = mx0 + (b >> 1);
    const bool on = mx < g.mw;
    int p[8];
    mjl_idct_block(&s_a[wave][b * MJL_BLK], &s_b[wave][b * MJL_BLK], on, k, p);
    if (on) {
        uint8_t* o = planes + g.chroma_row(f, b & 1, (size_t)my * 8 + k) + (size_t)mx * 8;      // (8-byte aligned: the pitch is a multiple of 8)
        uint2 v;
        v.x = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        v.y = (uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 24);
        *reinterpret_cast<uint2*>(o) = v;
    }
}

// One wave per MCU (four per workgroup), as k_mjd_pixels: islow IDCT of the four Y blocks (32 lanes), meanwhile all lanes gather the MCU's 8 x 8
// chroma samples and the ring of one sample around them from the planes -- indices clamped to the COMPONENT's size ((w + 1) / 2 x (h + 1) / 2: its
// own edge samples are what h2v2_fancy_upsample replicates, not the padding of the MCUs) -- as (Cb | Cr << 16) words; then lane = one 2 x 2 quad:
// 9 : 3 : 3 : 1 of the nearest samples, rounding 8 in even and 7 in odd columns.  libjpeg replicates instead where the chroma planes are at most 2 wide.
constexpr int MJL_CROW = 40;            // row pitch of the 10 x 10 neighbourhood: the four quad rows of a bank group on four disjoint sets of 8 banks
__global__ __launch_bounds__(256) void k_mjd_pixels_libjpeg(const int16_t* __restrict__ coef, const MjdFrame* __restrict__ frames, MjdGeom g,
                                                            const uint8_t* __restrict__ planes, uint8_t* __restrict__ dst) {
    __shared__ int s_a[4][4 * MJL_BLK], s_b[4][4 * MJL_BLK];
    __shared__ uint32_t s_c[4][10 * MJL_CROW];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int mx = blockIdx.x * 4 + wave, my = blockIdx.y, f = blockIdx.z;
    const bool act = mx < g.mw;
    const MjdFrame& fr = frames[f];
    if (act) {
        const int16_t* in = coef + (((size_t)f * g.mh + my) * g.mw + mx) * 384;
        const int nat = fr.zz[lane], at = (nat >> 3) * MJL_ROW + (nat & 7), q = fr.q[fr.tq[0]][lane];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) s_a[wave][blk * MJL_BLK + at] = in[blk * 64 + lane] * q;
        const int cw = (g.w + 1) >> 1, ch = (g.h + 1) >> 1;
        const uint8_t* cbp = planes + g.chroma_row(f, 0, 0);
        for (int i = lane; i < 100; i += 64) {
            const int r = i / 10, cc = i - r * 10;
            int y = my * 8 - 1 + r;
            y = y < 0 ? 0 : (y > ch - 1 ? ch - 1 : y);
            s_c[wave][r * MJL_CROW + cc] = mjd_chroma_word(cbp, g, y, mx * 8 - 1 + cc, cw);
        }
    }
    __syncthreads();
    {
        const int blk = (lane >> 3) & 3;
        mjl_idct_block_inplace(&s_a[wave][blk * MJL_BLK], &s_b[wave][blk * MJL_BLK], act && lane < 32, lane & 7);
    }
    __syncthreads();
    if (act) {
        const int qx = lane & 7, qy = lane >> 3;
        const int fancy = g.w > 4 ? 1 : 0;
        // the 3 x 3 samples around the quad's own, then per output row v the column sums 3 * own row + neighbouring row
        uint32_t c[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) c[r][cc] = s_c[wave][(qy + 1 + (r - 1) * fancy) * MJL_CROW + qx + 1 + (cc - 1) * fancy];
        uint8_t* fr_out = dst + (size_t)f * g.fstride;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int ly = 2 * qy + dy, py = my * 16 + ly;
            uint32_t cs[3];             // (both components at once: 16 * 255 fits the 16-bit halves)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) cs[cc] = 3u * c[1][cc] + c[dy ? 2 : 0][cc];
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int lx = 2 * qx + dx, px = mx * 16 + lx;
                if (py < g.h && px < g.w) {
                    const uint32_t both = 3u * cs[1] + cs[dx ? 2 : 0] + (dx ? 0x00070007u : 0x00080008u);
                    mjd_store_bgr(fr_out + (size_t)py * g.stride + (size_t)px * 3, s_a[wave][((ly >> 3) * 2 + (lx >> 3)) * MJL_BLK + (ly & 7) * MJL_ROW + (lx & 7)],
                                  (int)((both & 0xFFFFu) >> 4), (int)(both >> 20));
                }
            }
        }
    }
}

// ---- the other samplings of a baseline file (lvm_mjpeg_set_samplings), libjpeg's arithmetic only -------------------------------------------------
// All three kernels below give a wave the same piece of the frame: 64 pixels x 8 rows = eight 8 x 8 luminance blocks side by side (eight MCUs of
// 4:4:4 / gray, four of 4:2:2).  Why eight: the IDCT passes want (block, column) / (block, row) on all 64 lanes, and in the output stage lane = pixel
// column, so that every row of the piece leaves the wave as ONE contiguous run of 192 bytes (a wave of 2 2/3 4:4:4 MCUs would fill the IDCT as
// well, but end its rows in the middle of a block of the next wave).  With the chroma blocks of 4:4:4 that is three IDCT rounds of eight blocks
// each, all lanes busy in every one.
// LDS (ds_read_b32 / ds_write_b32: 32 banks, the two 32-lane halves apart): the IDCT passes are those of k_mjd_chroma_islow (pitch 9 / 72);
// the output stage reads block lane >> 3, row r, column lane & 7 = word 72 (lane >> 3) + 9 r + (lane & 7) = lane + 9 r (mod 32): conflict-free.

// 4:4:4 (nc = 3) and gray (nc = 1): no sample of another MCU is needed, so one launch and no scratch planes.  One wave per eight MCUs of an MCU
// row, 32 MCUs per workgroup.  NC is a template parameter: gray then holds 9.2 + 9.2 KB of LDS per workgroup where 4:4:4 holds 27.6 + 9.2 KB (the
// LDS that caps the workgroups per CU is the sampling's own), and the store loop carries no test of the sampling.
template <int NC>
__global__ __launch_bounds__(256) void k_mjd_pixels_direct(const int16_t* __restrict__ coef, const MjdFrame* __restrict__ frames, MjdGeom g, uint8_t* __restrict__ dst) {
    constexpr int nc = NC;
    __shared__ int s_a[4][NC * 8 * MJL_BLK], s_t[4][8 * MJL_BLK];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int mx0 = blockIdx.x * 32 + wave * 8, my = blockIdx.y, f = blockIdx.z;
    const MjdFrame& fr = frames[f];
    const int nat = fr.zz[lane], at = (nat >> 3) * MJL_ROW + (nat & 7);
    const int16_t* in = coef + ((size_t)f * g.mh + my) * g.mw * (size_t)(nc * 64);
    for (int c = 0; c < nc; ++c) {
        const int q = fr.q[fr.tq[c]][lane];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (mx0 + i < g.mw) s_a[wave][(c * 8 + i) * MJL_BLK + at] = in[((size_t)(mx0 + i) * nc + c) * 64 + lane] * q;
    }
    __syncthreads();
    const int b = lane >> 3, k = lane & 7;
    const bool on = mx0 + b < g.mw;
    for (int c = 0; c < nc; ++c) {      // (mjl_idct_block_inplace spelled out: HISTORY.md)
        int p[8];
        int* blk = &s_a[wave][(c * 8 + b) * MJL_BLK];
        mjl_idct_block(blk, &s_t[wave][b * MJL_BLK], on, k, p);
        if (on) {
#pragma unroll
            for (int x = 0; x < 8; ++x) blk[k * MJL_ROW + x] = p[x];
        }
    }
    __syncthreads();
    const int px = mx0 * 8 + lane;
    if (px < g.w) {
        uint8_t* o = dst + (size_t)f * g.fstride + (size_t)(my * 8) * g.stride + (size_t)px * 3;
        const int* yb = &s_a[wave][b * MJL_BLK + k];
        const int rows = g.h - my * 8 < 8 ? g.h - my * 8 : 8;
        for (int r = 0; r < rows; ++r, o += g.stride) {
            const int y = yb[r * MJL_ROW];
            if constexpr (NC == 1) { o[0] = (uint8_t)y; o[1] = (uint8_t)y; o[2] = (uint8_t)y; continue; }          // gray: b = g = r
            mjd_store_bgr(o, y, yb[8 * MJL_BLK + r * MJL_ROW], yb[16 * MJL_BLK + r * MJL_ROW]);
        }
    }
}

// 4:2:2 (Y 2 x 1, MCU 16 x 8; the Cb / Cr planes come from k_mjd_chroma_islow as for 4:2:0): libjpeg's h2v1_fancy_upsample, per chroma row c[0..n),
// n = (w + 1) / 2:  out[2i] = (3 c[i] + c[i-1] + 1) >> 2,  out[2i+1] = (3 c[i] + c[i+1] + 2) >> 2,  out[0] = c[0],  out[2n-1] = c[n-1]; nothing vertical.
// With the neighbour index clamped to the component's own width the two edge rules ARE the general ones ((3 c + c + 1 or 2) >> 2 = c).  Where
// n <= 2 libjpeg replicates: the neighbour is then the sample itself.  One wave per four MCUs of an MCU row, sixteen per workgroup: IDCT of their
// eight Y blocks, meanwhile all lanes gather the 8 rows x (32 + one either side) chroma samples as (Cb | Cr << 16) words -- both components
// filter at once, 4 * 255 + 2 fits the halves.  The gather stores word i from lane i (mod 64) into a row pitch of 34 = consecutive words; the
// output stage reads words 1 + (lane >> 1) and that +- 1 of ONE row: 17 consecutive words per half-wave, pairs of lanes on the same word
// (broadcast): both conflict-free.
constexpr int MJL_HROW = 34;
__global__ __launch_bounds__(256) void k_mjd_pixels_h2v1(const int16_t* __restrict__ coef, const MjdFrame* __restrict__ frames, MjdGeom g,
                                                         const uint8_t* __restrict__ planes, uint8_t* __restrict__ dst) {
    __shared__ int s_a[4][8 * MJL_BLK], s_t[4][8 * MJL_BLK];
    __shared__ uint32_t s_c[4][8 * MJL_HROW];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int mx0 = blockIdx.x * 16 + wave * 4, my = blockIdx.y, f = blockIdx.z;
    const MjdFrame& fr = frames[f];
    const int nat = fr.zz[lane], at = (nat >> 3) * MJL_ROW + (nat & 7), q = fr.q[fr.tq[0]][lane];
    const int16_t* in = coef + ((size_t)f * g.mh + my) * g.mw * 256;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (mx0 + (i >> 1) < g.mw) s_a[wave][i * MJL_BLK + at] = in[((size_t)(mx0 + (i >> 1)) * 4 + (i & 1)) * 64 + lane] * q;
    if (mx0 < g.mw) {
        const int cw = (g.w + 1) >> 1;
        const uint8_t* cbp = planes + g.chroma_row(f, 0, 0) + (size_t)(my * 8) * g.chroma_pitch();      // (= chroma_row(f, 0, my * 8), which costs a scalar register here)
        for (int i = lane; i < 8 * MJL_HROW; i += 64) {
            const int r = i / MJL_HROW, cc = i - r * MJL_HROW;
            s_c[wave][i] = mjd_chroma_word(cbp, g, r, mx0 * 8 - 1 + cc, cw);
        }
    }
    __syncthreads();
    const int b = lane >> 3, k = lane & 7;
    mjl_idct_block_inplace(&s_a[wave][b * MJL_BLK], &s_t[wave][b * MJL_BLK], mx0 + (b >> 1) < g.mw, k);
    __syncthreads();
    const int px = mx0 * 16 + lane;
    if (px < g.w) {
        const int odd = lane & 1, own = 1 + (lane >> 1), nb = g.w > 4 ? own + (odd ? 1 : -1) : own;
        const uint32_t rnd = odd ? 0x00020002u : 0x00010001u;
        uint8_t* o = dst + (size_t)f * g.fstride + (size_t)(my * 8) * g.stride + (size_t)px * 3;
        const int* yb = &s_a[wave][b * MJL_BLK + k];
        const int rows = g.h - my * 8 < 8 ? g.h - my * 8 : 8;
        for (int r = 0; r < rows; ++r, o += g.stride) {
            const uint32_t both = 3u * s_c[wave][r * MJL_HROW + own] + s_c[wave][r * MJL_HROW + nb] + rnd;
            mjd_store_bgr(o, yb[r * MJL_ROW], (int)((both & 0xFFFFu) >> 2), (int)(both >> 18));
        }
    }
}

}  // namespace

void mjpeg_decode_release(Ctx* c) {
    delete static_cast<MjdState*>(c->mjpeg_dec);
    c->mjpeg_dec = nullptr;
}

// Three steps, so that a caller can decode sub-batch by sub-batch between other work on the same queue (lvm_export_mjpeg_frames):
//   begin    parses every frame, uploads all bytes and tables (asynchronously on s)
//   enqueue  the three kernels for frames [f0, f0 + nf) -> BGR frames at d_bgr
//   finish   waits for s and turns the error flags into the status of the call (a malformed stream is an error, not a picture)
int mjpeg_decode_begin(Ctx* c, const uint8_t* jpegs, const size_t* offsets, int n, int w, int h, hipStream_t s) {
    if (w < 1 || h < 1 || w > 8192 || h > 16384) { c->err = "lvm_mjpeg_decode: frame size out of range (1..8192 x 1..16384)"; return LVM_ERR_INVALID; }
    MjdState* st = static_cast<MjdState*>(c->mjpeg_dec);
    if (!st) { st = new MjdState; c->mjpeg_dec = st; }
    st->frames.resize((size_t)n);
    MjdSamp sp{}; MjdGeom g{};
    std::vector<uint32_t> foff((size_t)n + 1);
    int max_iv = 1, max_sub = 1, npar = 0;
    for (int i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[0] > 0xFFFFFFF0ull) { c->err = "lvm_mjpeg_decode: bad offsets"; return LVM_ERR_INVALID; }
        MjdFrame& f = st->frames[(size_t)i];
        const char* why = parse_frame(jpegs + offsets[i], offsets[i + 1] - offsets[i], w, h, c->mjpeg_samplings, f);
        if (!why && f.samp != st->frames[0].samp) why = "sampling differs from frame 0's";
        if (why) { c->err = std::string("lvm_mjpeg_decode: frame ") + std::to_string(i) + ": " + why; return LVM_ERR_INVALID; }
        if (i == 0) {       // the frames of a call share one sampling, as the frames of a file do: the MCU is a property of the call.  The kind is
                            // checked here, before frames 1.. are parsed: a sampling the kind cannot decode is reported ahead of a later frame's damage
            mjd_layout(w, h, f.samp, sp, g);
            if (f.samp != LVM_MJPEG_SAMPLING_420 && c->mjpeg_decoder != LVM_MJPEG_DECODER_LIBJPEG) {
                c->err = std::string("lvm_mjpeg_decode: frame 0: ") + sp.name + " needs LVM_MJPEG_DECODER_LIBJPEG"; return LVM_ERR_INVALID;
            }
        }
        f.nintervals = f.restart ? (uint32_t)((g.nmcu() + (int)f.restart - 1) / (int)f.restart) : 1u;
        if ((int)f.nintervals > max_iv) max_iv = (int)f.nintervals;
        // no restart markers: one lane would decode the whole frame -- the self-synchronising kernels take it (LVM_MJD_PARALLEL=0: never, =2: also tiny frames)
        static const int par_mode = [] { int v = 1; env_switch("LVM_MJD_PARALLEL", v); return v; }();
        f.par = (f.restart == 0 && par_mode != 0 && (f.data_len >= 2048u || par_mode == 2)) ? 1u : 0u;
        f.usub = (f.data_len * 8u + MJP_SUB_BITS - 1) / MJP_SUB_BITS + 1u;
        if (f.par) { ++npar; if ((int)f.usub > max_sub) max_sub = (int)f.usub; }
        foff[(size_t)i] = (uint32_t)(offsets[i] - offsets[0]);
    }
    foff[(size_t)n] = (uint32_t)(offsets[n] - offsets[0]);
    const size_t nbytes = offsets[n] - offsets[0];
    // What this call needs of every buffer; the self-synchronising path's only with a frame for it, the chroma planes only where the pixel stage has two
    // launches.  (+ 32 / + 64: the word readers look one or two words ahead.)  A buffer grows to the exact size and keeps no contents; work queued by
    // an earlier call may still use the old allocation, hence one wait in front of the first growth.
    const int sub_cap = npar && max_sub > st->sub_cap ? max_sub : st->sub_cap;
    const size_t par = npar ? (size_t)n : 0, subs = par * (size_t)sub_cap, ivs = (size_t)n * max_iv * sizeof(uint32_t);
    const bool planes = c->mjpeg_decoder == LVM_MJPEG_DECODER_LIBJPEG && sp.ny > 1;
    const struct { DevBuf& b; size_t bytes; } need[] = {
        {st->d_frames, (size_t)n * sizeof(MjdFrame)}, {st->d_coef, (size_t)n * g.nmcu() * sp.nblk * 64 * sizeof(int16_t)}, {st->d_err, ((size_t)n * 2 + 2) * sizeof(uint32_t)},
        {st->d_ivstart, ivs}, {st->d_ivend, ivs}, {st->d_bytes, nbytes + 32},
        {st->d_ubytes, npar ? nbytes + 64 : 0}, {st->d_ulen, par * sizeof(uint32_t)}, {st->d_before, subs * sizeof(uint32_t)}, {st->d_changed, npar ? sizeof(uint32_t) : 0},
        {st->d_exit[0], subs * sizeof(unsigned long long)}, {st->d_exit[1], subs * sizeof(unsigned long long)},
        {st->d_chroma, planes ? g.chroma_row(n, 0, 0) : 0}};
    bool grow = false;
    for (const auto& x : need) grow = grow || x.b.cap < x.bytes;
    if (grow) LVM_HIP_TRY(c, hipStreamSynchronize(s));
    for (const auto& x : need) { const int rc = x.b.reserve(c, x.bytes); if (rc != LVM_OK) return rc; }
    st->samp = st->frames[0].samp; st->sp = sp; st->g = g;
    st->kind = c->mjpeg_decoder;
    st->n = n; st->max_iv = max_iv; st->sub_cap = sub_cap;
    st->foff = foff;                                             // (stays alive until the copy below has run)
    LVM_HIP_TRY(c, hipMemcpyAsync(st->d_bytes.p, jpegs + offsets[0], nbytes, hipMemcpyHostToDevice, s));
    LVM_HIP_TRY(c, hipMemcpyAsync(st->d_frames.p, st->frames.data(), (size_t)n * sizeof(MjdFrame), hipMemcpyHostToDevice, s));
    LVM_HIP_TRY(c, hipMemsetAsync(st->d_err.p, 0, (size_t)n * sizeof(uint32_t), s));
    LVM_HIP_TRY(c, hipMemcpyAsync(st->d_err.as<uint32_t>() + n, st->foff.data(), ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    return LVM_OK;
}

int mjpeg_decode_enqueue(Ctx* c, int f0, int nf, uint8_t* d_bgr, ptrdiff_t stride, ptrdiff_t fstride, hipStream_t s) {
    MjdState* st = static_cast<MjdState*>(c->mjpeg_dec);
    if (!st || f0 < 0 || nf < 1 || f0 + nf > st->n) { c->err = "lvm_mjpeg_decode: enqueue without begin"; return LVM_ERR_INVALID; }
    const MjdSamp& sp = st->sp;
    MjdGeom g = st->g;
    g.stride = (long)stride; g.fstride = (long)fstride;
    const int nmcu = g.nmcu(), mw = g.mw, mh = g.mh;
    const size_t mcu_coefs = (size_t)sp.nblk * 64;
    const MjdFrame* fr = st->d_frames.as<MjdFrame>() + f0;
    uint32_t* err = st->d_err.as<uint32_t>() + f0;
    const uint32_t* d_foff = err + st->n;
    int16_t* coef = st->d_coef.as<int16_t>() + (size_t)f0 * nmcu * mcu_coefs;
    uint32_t *ivs = st->d_ivstart.as<uint32_t>() + (size_t)f0 * st->max_iv, *ive = st->d_ivend.as<uint32_t>() + (size_t)f0 * st->max_iv;
    LVM_HIP_TRY(c, hipMemsetAsync(coef, 0, (size_t)nf * nmcu * mcu_coefs * sizeof(int16_t), s));
    LVM_LAUNCH(c, "mjd_intervals", k_mjd_intervals, dim3(nf), dim3(256), s, (const uint8_t*)st->d_bytes, fr, d_foff, ivs, ive, st->max_iv, err);
    LVM_LAUNCH(c, "mjd_huffman", k_mjd_huffman, dim3((st->max_iv + 63) / 64, nf), dim3(64), s, (const uint8_t*)st->d_bytes, fr, d_foff, (const uint32_t*)ivs,
               (const uint32_t*)ive, st->max_iv, nmcu, sp.nblk, sp.ny, coef, err);
    bool any_par = false;
    for (int i = f0; i < f0 + nf; ++i) any_par = any_par || st->frames[(size_t)i].par;
    if (any_par) {
        uint32_t *ulen = st->d_ulen.as<uint32_t>() + f0, *before = st->d_before.as<uint32_t>() + (size_t)f0 * st->sub_cap, *d_changed = st->d_changed.as<uint32_t>();
        unsigned long long* ex[2] = {st->d_exit[0].as<unsigned long long>() + (size_t)f0 * st->sub_cap, st->d_exit[1].as<unsigned long long>() + (size_t)f0 * st->sub_cap};
        const dim3 gsub((unsigned)((st->sub_cap + 63) / 64), (unsigned)nf);
        LVM_LAUNCH(c, "mjp_unstuff", k_mjp_unstuff, dim3(nf), dim3(256), s, (const uint8_t*)st->d_bytes, fr, d_foff, st->d_ubytes.p, ulen);
        LVM_LAUNCH(c, "mjp_sync", k_mjp_sync, gsub, dim3(64), s, (const uint8_t*)st->d_ubytes, fr, d_foff, (const uint32_t*)ulen, st->sub_cap, 1, sp.nblk, sp.ny, (const unsigned long long*)ex[1], ex[0], d_changed);
        int cur = 0;                                               // ex[cur] holds the latest exits
        for (int it = 0; it <= st->sub_cap; ++it) {                // (every pass makes at least one more lane exact: sub_cap passes always suffice)
            uint32_t changed = 0;
            LVM_HIP_TRY(c, hipMemsetAsync(d_changed, 0, sizeof(uint32_t), s));
            LVM_LAUNCH(c, "mjp_sync", k_mjp_sync, gsub, dim3(64), s, (const uint8_t*)st->d_ubytes, fr, d_foff, (const uint32_t*)ulen, st->sub_cap, 0, sp.nblk, sp.ny, (const unsigned long long*)ex[cur], ex[cur ^ 1],
                       d_changed);
            LVM_HIP_TRY(c, hipMemcpyAsync(&changed, d_changed, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            LVM_HIP_TRY(c, hipStreamSynchronize(s));
            cur ^= 1;
            if (!changed) break;
        }
        LVM_LAUNCH(c, "mjp_scan", k_mjp_scan, dim3(nf), dim3(256), s, fr, (const uint32_t*)ulen, st->sub_cap, (const unsigned long long*)ex[cur], before);
        LVM_LAUNCH(c, "mjp_write", k_mjp_write, gsub, dim3(64), s, (const uint8_t*)st->d_ubytes, fr, d_foff, (const uint32_t*)ulen, st->sub_cap, (const unsigned long long*)ex[cur],
                   (const uint32_t*)before, nmcu, sp.nblk, sp.ny, coef, err);
        LVM_LAUNCH(c, "mjp_dc", k_mjp_dc, dim3(sp.ncomp, nf), dim3(256), s, fr, nmcu, sp.nblk, sp.ny, coef);
    }
    // the pixel stage: under the libjpeg kind the samplings with subsampled chroma get their Cb / Cr planes first, then one launch writes the frames
    const dim3 b256(256);
    const uint8_t* planes = nullptr;
    if (st->kind == LVM_MJPEG_DECODER_LIBJPEG && sp.ny > 1) {
        uint8_t* p = st->d_chroma.p + g.chroma_row(f0, 0, 0);
        LVM_LAUNCH(c, "mjd_chroma_islow", k_mjd_chroma_islow, dim3((mw + 15) / 16, mh, nf), b256, s, (const int16_t*)coef, fr, g, sp.nblk, sp.ny, p);
        planes = p;
    }
    switch (st->samp) {
        case LVM_MJPEG_SAMPLING_GRAY: LVM_LAUNCH(c, "mjd_pixels_direct", k_mjd_pixels_direct<1>, dim3((mw + 31) / 32, mh, nf), b256, s, (const int16_t*)coef, fr, g, d_bgr); break;
        case LVM_MJPEG_SAMPLING_444: LVM_LAUNCH(c, "mjd_pixels_direct", k_mjd_pixels_direct<3>, dim3((mw + 31) / 32, mh, nf), b256, s, (const int16_t*)coef, fr, g, d_bgr); break;
        case LVM_MJPEG_SAMPLING_422: LVM_LAUNCH(c, "mjd_pixels_h2v1", k_mjd_pixels_h2v1, dim3((mw + 15) / 16, mh, nf), b256, s, (const int16_t*)coef, fr, g, planes, d_bgr); break;
        default:
            if (planes) LVM_LAUNCH(c, "mjd_pixels_libjpeg", k_mjd_pixels_libjpeg, dim3((mw + 3) / 4, mh, nf), b256, s, (const int16_t*)coef, fr, g, planes, d_bgr);
            else LVM_LAUNCH(c, "mjd_pixels", k_mjd_pixels, dim3((mw + 3) / 4, mh, nf), b256, s, (const int16_t*)coef, fr, g, d_bgr);
    }
    return LVM_OK;
}

int mjpeg_decode_finish(Ctx* c, hipStream_t s) {
    MjdState* st = static_cast<MjdState*>(c->mjpeg_dec);
    if (!st) { c->err = "lvm_mjpeg_decode: finish without begin"; return LVM_ERR_INVALID; }
    std::vector<uint32_t> err((size_t)st->n);
    LVM_HIP_TRY(c, hipMemcpyAsync(err.data(), st->d_err.p, (size_t)st->n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LVM_HIP_TRY(c, hipStreamSynchronize(s));
    for (int i = 0; i < st->n; ++i)
        if (err[(size_t)i]) {
            c->err = std::string("lvm_mjpeg_decode: frame ") + std::to_string(i) + (err[(size_t)i] & 1u ? ": restart markers do not match the restart interval" : ": invalid Huffman code / coefficient index");
            return LVM_ERR_INVALID;
        }
    return LVM_OK;
}

int mjpeg_decode_device(Ctx* c, const uint8_t* jpegs, const size_t* offsets, int n, int w, int h, uint8_t* d_bgr, ptrdiff_t stride, ptrdiff_t fstride, hipStream_t s) {
    int rc = mjpeg_decode_begin(c, jpegs, offsets, n, w, h, s);
    if (rc == LVM_OK) rc = mjpeg_decode_enqueue(c, 0, n, d_bgr, stride, fstride, s);
    if (rc != LVM_OK) { (void)hipStreamSynchronize(s); return rc; }
    return mjpeg_decode_finish(c, s);
}

}  // namespace lvm
