"""Designed content for the Motion-JPEG tests (tests/test_mjpeg_extremes.py), and the counters that say what a frame makes the entropy coder emit.

A texture plus noise reaches neither end of the Huffman tables: the longest words of T.81 (a DC difference of category 11, an AC coefficient of category 10
behind a 16-bit code) need a block that swings over the full range in the sign pattern of one basis function, next to a block at the other end of the range;
the shortest ones need a frame without any detail.  The frames here are built for that, with numpy alone, and `coverage` counts on the ORACLE's side (its
coefficients, its interval rule, its entropy coder -- never a device) which symbols a frame reaches, so that a test can insist on them before it compares a byte."""
import math

import numpy as np

from oracle import mjpeg_oracle as mo


def sign_pattern(u, v):
    """8 x 8 booleans [y][x]: where the basis function of horizontal frequency u and vertical frequency v is not negative"""
    cy = np.array([math.cos((2 * y + 1) * v * math.pi / 16) for y in range(8)])
    cx = np.array([math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)])
    return cy[:, None] * cx[None, :] >= 0


def basis():
    """64 x 64, B = G = R (Y is the byte): the block at block row v, block column u is 255 where basis function (u, v) is not negative and 0 elsewhere --
    every AC position at full swing under its own sign pattern; block (0, 0) is black, next to white-dominated ones"""
    g = np.zeros((64, 64), np.uint8)
    for v in range(8):
        for u in range(8):
            g[v * 8:v * 8 + 8, u * 8:u * 8 + 8] = np.where(sign_pattern(u, v), 255, 0)
    g[:8, :8] = 0
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


SOLID = [(255, 0, 0), (0, 255, 255), (0, 0, 255), (255, 255, 0)]                           # BGR: blue, yellow, red, cyan
CHROMA_POSITIONS = [(1, 0), (0, 1), (4, 4), (7, 7), (4, 0), (0, 4), (7, 0), (3, 5)]       # (u, v) of MCU mx in MCU row 1


def chroma():
    """128 x 32 BGR.  MCU row 0: eight solid MCUs whose Cb and Cr jump between -1024 and 1016 (DC) from one to the next; MCU row 1: MCU mx is the sign
    pattern of chrominance position CHROMA_POSITIONS[mx] (a chroma sample = 2 x 2 pixels) in blue / yellow (mx even) or red / cyan (mx odd)"""
    f = np.zeros((32, 128, 3), np.uint8)
    for mx in range(8):
        f[0:16, mx * 16:mx * 16 + 16] = SOLID[(mx + 2 * 0) % 4]
        u, v = CHROMA_POSITIONS[mx]
        pat = np.repeat(np.repeat(sign_pattern(u, v), 2, axis=0), 2, axis=1)
        hi, lo = (SOLID[0], SOLID[1]) if mx % 2 == 0 else (SOLID[2], SOLID[3])
        f[16:32, mx * 16:mx * 16 + 16] = np.where(pat[:, :, None], np.array(hi, np.uint8), np.array(lo, np.uint8))
    return f


def flat():
    """56 x 40, every byte 7: blocks of 4 to 6 bits, several runs of blocks inside one 32-bit word of the stream"""
    return np.full((40, 56, 3), 7, np.uint8)


def tiled(frame):
    """the frame 2 x 2 times: four times the entropy data -- libjpeg's streams of basis() and chroma() (no DRI) stay below the 2 KB from which the decoder hands
    a frame without restart intervals to its self-synchronising kernels, those of the tiled frames at quality 100 are 2.6 to 6.9 KB long"""
    return np.ascontiguousarray(np.tile(frame, (2, 2, 1)))


def padded(frame, w, h):
    """the frame in the top left corner of a w x h one, its last column and row repeated"""
    fh, fw, _ = frame.shape
    return np.ascontiguousarray(np.pad(frame, ((0, h - fh), (0, w - fw), (0, 0)), mode="edge"))


def interval_length(mcus, restart):
    """MCUs per restart interval: the rule of mo.encode_frame (default 8, at most 512, at most 65535 intervals)"""
    ri = 8 if not restart else min(int(restart), 512)
    if (mcus + ri - 1) // ri > 65535:
        ri = (mcus + 65534) // 65535
    return ri


def _cat(v):
    return int(abs(int(v))).bit_length()


def coverage(frame, quality, restart):
    """What the oracle's entropy coder emits for `frame`: dict with
      ac_cat   (luminance, chrominance)  largest category of an AC coefficient
      dc_cat   (luminance, chrominance)  largest category of a DC difference (predictors reset with every interval)
      ac_max   (luminance, chrominance)  largest magnitude of an AC coefficient
      zrl      number of ZRL symbols (a zero run of 16 in front of a non-zero coefficient)
      no_eob   number of blocks whose coefficient 63 is not zero (no end-of-block symbol)
      ff00     number of stuffed FF bytes in the entropy data
      ff_at_marker   number of intervals whose last byte is a stuffed FF (FF 00 directly in front of RSTn / EOI)
      intervals      number of restart intervals"""
    c = mo.coefficients(frame, quality)
    mh, mw = c.shape[:2]
    mcus = c.reshape(mh * mw, 6, 64)
    ri = interval_length(mh * mw, restart)
    nint = (mh * mw + ri - 1) // ri
    tabs = tuple(mo.huff_codes(s) for s in (mo.DC_LUMA, mo.AC_LUMA, mo.DC_CHROMA, mo.AC_CHROMA))
    ac_cat, dc_cat, ac_max = [0, 0], [0, 0], [0, 0]
    zrl = no_eob = ff00 = ff_at_marker = 0
    for r in range(nint):
        part = mcus[r * ri:(r + 1) * ri]
        pred = [0, 0, 0]
        for mcu in part:
            for bi in range(6):
                comp = 0 if bi < 4 else bi - 3
                t = 0 if comp == 0 else 1
                blk = mcu[bi]
                dc_cat[t] = max(dc_cat[t], _cat(int(blk[0]) - pred[comp]))
                pred[comp] = int(blk[0])
                nz = np.nonzero(blk[1:])[0] + 1
                if len(nz):
                    ac_max[t] = max(ac_max[t], int(np.abs(blk[1:]).max()))
                    ac_cat[t] = max(ac_cat[t], _cat(ac_max[t]))
                    runs = np.diff(np.concatenate([[0], nz])) - 1
                    zrl += int((runs // 16).sum())
                    no_eob += int(nz[-1] == 63)
        data = mo.entropy_interval(part, tabs)
        ff00 += data.count(b"\xff")
        ff_at_marker += int(data.endswith(b"\xff\x00"))
    return dict(ac_cat=tuple(ac_cat), dc_cat=tuple(dc_cat), ac_max=tuple(ac_max), zrl=zrl, no_eob=no_eob, ff00=ff00, ff_at_marker=ff_at_marker, intervals=nint)
