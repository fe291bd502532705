"""libjpeg's decode restated in numpy for every sampling a baseline Motion-JPEG file can have (test infrastructure; the yardstick of
lvm_mjpeg_set_samplings): 4:2:0, 4:2:2 (Y 2x1), 4:4:4 and one component.

  entropy   the loop of mjpeg_oracle.decode_coefficients over the MCU's block list -- H x V luminance blocks, then Cb and Cr; a one-component scan is
            not interleaved (T.81 A.2.2): its MCU is one block whatever the frame header's sampling factors say, and the restart interval counts blocks
  IDCT      libjpeg_ref.islow on coef * q (no clamp)
  chroma    4:2:0  libjpeg_ref.upsample (h2v2 fancy; replication where the plane is at most 2 wide)
            4:2:2  h2v1_fancy_upsample (jdsample.c) per row c[0..n): out[2i] = (3 c[i] + c[i-1] + 1) >> 2, out[2i+1] = (3 c[i] + c[i+1] + 2) >> 2,
                   out[0] = c[0], out[2n-1] = c[n-1]; replication where n <= 2; nothing vertical
            4:4:4  as it is
  colour    the YCC constants of jdcolor.c (libjpeg_ref.bgr's); gray: b = g = r = y
tests/test_mjpeg_decode_samplings.py pins decode() against Pillow (libjpeg-turbo) byte for byte, and the HIP kernels against both."""
import numpy as np

import libjpeg_ref as lj
from oracle import mjpeg_oracle as mo


def decode_coefficients(j):
    """JPEG frame -> (header, coef[mh][mw][blocks per MCU][64] in zigzag order, H, V, component of every block of the MCU)"""
    hd = mo.parse_header(j)
    comps = hd["comps"]
    nc = len(comps)
    assert nc in (1, 3) and len(hd["scan"]) == nc
    H, V = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)
    assert (H, V) in ((2, 2), (2, 1), (1, 1)) and all(c[1] == c[2] == 1 for c in comps[1:])
    tabs = {}
    for key, std in (((0, 0), mo.DC_LUMA), ((1, 0), mo.AC_LUMA), ((0, 1), mo.DC_CHROMA), ((1, 1), mo.AC_CHROMA)):
        tabs[key] = mo._decode_tables(hd["huff"].get(key, std))
    for key, spec in hd["huff"].items():
        tabs[key] = mo._decode_tables(spec)
    w, h = hd["w"], hd["h"]
    mw, mh = -(-w // (8 * H)), -(-h // (8 * V))
    blk = [0] * (H * V) + ([1, 2] if nc == 3 else [])
    coef = np.zeros((mh * mw, len(blk), 64), np.int32)
    ri = hd["restart"] or mh * mw
    for k, seg in enumerate(mo.split_intervals(j[hd["data_start"]:])):
        br, pred = mo._BitReader(seg), [0, 0, 0]
        for m in range(k * ri, min((k + 1) * ri, mh * mw)):
            for bi, comp in enumerate(blk):
                _, td, ta = hd["scan"][comp]
                s = mo._decode_symbol(br, tabs[(0, td)])
                pred[comp] += mo._extend(br.bits(s), s)
                coef[m, bi, 0] = pred[comp]
                kk = 1
                while kk < 64:
                    rs = mo._decode_symbol(br, tabs[(1, ta)])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        kk += 16
                        continue
                    kk += r
                    coef[m, bi, kk] = mo._extend(br.bits(s), s)
                    kk += 1
    return hd, coef.reshape(mh, mw, len(blk), 64), H, V, blk


def h2v1_fancy(c):
    """one chroma plane [ch][cw] -> [ch][2 cw], libjpeg's h2v1_fancy_upsample"""
    c = c.astype(np.int64)
    prev = np.hstack([c[:, :1], c[:, :-1]])
    nxt = np.hstack([c[:, 1:], c[:, -1:]])
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2] = (3 * c + prev + 1) >> 2
    out[:, 1::2] = (3 * c + nxt + 2) >> 2
    out[:, 0], out[:, -1] = c[:, 0], c[:, -1]
    return out


def upsample(c, H, V):
    if (H, V) == (2, 2):
        return lj.upsample(c)
    if (H, V) == (2, 1):
        return h2v1_fancy(c) if c.shape[1] > 2 else np.repeat(c.astype(np.int64), 2, 1)
    return c


def decode(j):
    """JPEG frame -> BGR u8 [h][w][3]"""
    hd, coef, H, V, blk = decode_coefficients(j)
    mh, mw = coef.shape[:2]
    h, w = hd["h"], hd["w"]
    planes = []
    for bi, comp in enumerate(blk):
        q = hd["q"][hd["comps"][comp][3]].astype(np.int64)
        nat = np.zeros((mh, mw, 64), np.int64)
        nat[..., mo.ZIGZAG] = coef[:, :, bi, :]
        planes.append(lj.islow((nat * q).reshape(mh, mw, 8, 8)))
    y = np.zeros((mh * 8 * V, mw * 8 * H), np.int64)
    for bi in range(H * V):
        oy, ox = (bi // H) * 8, (bi % H) * 8
        y.reshape(mh, 8 * V, mw, 8 * H)[:, oy:oy + 8, :, ox:ox + 8] = planes[bi].transpose(0, 2, 1, 3)
    if len(blk) == 1:
        y = y[:h, :w]
        return np.clip(np.stack([y, y, y], -1), 0, 255).astype(np.uint8)
    ch, cw = -(-h // V), -(-w // H)
    cb, cr = [upsample(planes[H * V + i].transpose(0, 2, 1, 3).reshape(mh * 8, mw * 8)[:ch, :cw], H, V) for i in (0, 1)]
    return lj.bgr(hd, y, cb, cr)
