"""libjpeg's decode arithmetic restated in numpy (test infrastructure; the yardstick of LVM_MJPEG_DECODER_LIBJPEG).

What libjpeg / libjpeg-turbo compute with their defaults behind the entropy layer -- all integer, hence reproducible to the byte:
  dequantise   coef * q, no clamp
  IDCT         jpeg_idct_islow (jidctint.c): CONST_BITS 13, PASS1_BITS 2; columns first, descaled by 11 bits, then rows, descaled by 18, + 128, clamped
  chroma       h2v2_fancy_upsample (jdsample.c) = mjpeg_oracle.upsample_fancy on the component's OWN (w + 1) / 2 x (h + 1) / 2 samples; plain
               replication where that plane is at most 2 samples wide (libjpeg selects the fancy routine for downsampled_width > 2 only)
  colour       the YCC tables of jdcolor.c: the constants mjpeg_oracle.reconstruct uses already
The entropy layer is mjpeg_oracle.decode_coefficients, unchanged.  The stages are separate functions so that a mismatch can be localised:
  idct_planes(j) -> luma_plane / chroma_planes -> upsample -> bgr;  decode(j) chains them.
tests/test_mjpeg_decode_libjpeg.py pins decode() against Pillow (libjpeg-turbo) byte for byte, and the HIP kernels against both."""
import numpy as np

from oracle import mjpeg_oracle as mo


def islow_1d(i, shift):
    """one pass of jpeg_idct_islow over the list i[0..8) of integer arrays -> list of 8 arrays, descaled by `shift` bits"""
    i = [x.astype(np.int64) for x in i]
    z1 = (i[2] + i[6]) * 4433
    tmp2 = z1 - i[6] * 15137
    tmp3 = z1 + i[2] * 6270
    tmp0 = (i[0] + i[4]) << 13
    tmp1 = (i[0] - i[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return [(x + (1 << (shift - 1))) >> shift for x in out]


def islow(s):
    """dequantised coefficients s[..., v, u] -> samples [..., y, x] in 0..255"""
    cols = islow_1d([s[..., v, :] for v in range(8)], 11)          # over v: list over y of [..., u]
    t = np.stack(cols, -2)                                         # [..., y, u]
    rows = islow_1d([t[..., u] for u in range(8)], 18)             # over u: list over x of [..., y]
    return np.clip(np.stack(rows, -1) + 128, 0, 255)


def idct_planes(j):
    """JPEG frame -> (header, the six blocks of every MCU after the IDCT: list of [mh][mw][8][8])"""
    hd, coef = mo.decode_coefficients(j)
    mh, mw = coef.shape[:2]
    tq = [hd["comps"][0][3]] * 4 + [hd["comps"][1][3], hd["comps"][2][3]]
    planes = []
    for bi in range(6):
        q = hd["q"][tq[bi]].astype(np.int64)
        nat = np.zeros(coef.shape[:2] + (64,), np.int64)
        nat[..., mo.ZIGZAG] = coef[:, :, bi, :]
        planes.append(islow((nat * q).reshape(mh, mw, 8, 8)))
    return hd, planes


def luma_plane(planes):
    """-> Y [mh * 16][mw * 16] (MCU padding included)"""
    mh, mw = planes[0].shape[:2]
    y = np.zeros((mh * 16, mw * 16), np.int64)
    for bi in range(4):
        oy, ox = (bi >> 1) * 8, (bi & 1) * 8
        for r in range(8):
            y[oy + r::16, :].reshape(mh, mw, 16)[:, :, ox:ox + 8] = planes[bi][:, :, r, :]
    return y


def chroma_planes(hd, planes):
    """-> Cb, Cr at the component's own size, (h + 1) / 2 x (w + 1) / 2"""
    mh, mw = planes[0].shape[:2]
    ch, cw = (hd["h"] + 1) // 2, (hd["w"] + 1) // 2
    return [planes[bi].transpose(0, 2, 1, 3).reshape(mh * 8, mw * 8)[:ch, :cw] for bi in (4, 5)]


def upsample(c):
    """one chroma plane [ch][cw] -> [2 ch][2 cw]"""
    if c.shape[1] > 2:
        return mo.upsample_fancy(c)
    return np.repeat(np.repeat(c.astype(np.int64), 2, 0), 2, 1)


def bgr(hd, y, cb, cr):
    """Y (padded) and the upsampled chroma planes -> BGR u8 [h][w][3]"""
    h, w = hd["h"], hd["w"]
    y, cb, cr = y[:h, :w], cb[:h, :w] - 128, cr[:h, :w] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def decode(j):
    hd, planes = idct_planes(j)
    cb, cr = chroma_planes(hd, planes)
    return bgr(hd, luma_plane(planes), upsample(cb), upsample(cr))
