"""Chromatic content for the parity tests (test infrastructure).

synth.texture is a grey grating with +-12 levels of per-channel noise: B, G and R of a pixel never differ by more than about 30
levels, so a clip built from it reads only the nodes of the 33^3 forward Lab table next to the grey diagonal and sends only
near-neutral Lab values through the inverse conversion.  The generators here supply what video has and that texture lacks:
saturated colours, channels at 0 and 255 beside channels that are not, and every u8 colour once (cube_frames).

Each kind gives a float64 texture of shape (h, w + 2 * pad, 3) in [0, 255], channel order B, G, R, a function of the seed alone;
chroma_clip puts it into a synth.Clip, whose sub-pixel motion, colour pulse and frame_torch then work unchanged."""
import numpy as np

KINDS = ("noise", "edges", "bars", "hue")
EDGE_VALUES = (0, 1, 2, 127, 128, 253, 254, 255)       # cells 0, 15 / 16 and 31 / 32 of the table, weights 0 ... 15


def _noise(w, h, rng):
    """every channel independently uniform on the integers 0 .. 255"""
    return rng.integers(0, 256, size=(h, w, 3)).astype(np.float64)


def _edges(w, h, rng):
    """every channel drawn from EDGE_VALUES: the first and last cells of the table in mixed combinations"""
    return np.asarray(EDGE_VALUES, np.float64)[rng.integers(0, len(EDGE_VALUES), size=(h, w, 3))]


def _bars(w, h, rng):
    """eight vertical bars, the corners of the colour cube, times a vertical ramp from 0.25 to 1, +- 3 levels of noise, clipped"""
    corner = (np.arange(w) * 8) // w                                                  # bar number 0 .. 7 per column
    bgr = 255.0 * np.stack([(corner >> k) & 1 for k in range(3)], axis=-1)            # (w, 3)
    ramp = np.linspace(0.25, 1.0, h)[:, None, None]
    return np.clip(bgr[None, :, :] * ramp + rng.uniform(-3.0, 3.0, size=(h, w, 3)), 0.0, 255.0)


def _hue(w, h, rng):
    """fully saturated hue along x (one turn over the width), value 0 .. 255 along y"""
    hx = 6.0 * np.arange(w, dtype=np.float64) / w                                     # [0, 6)
    r = np.clip(np.abs(hx - 3.0) - 1.0, 0.0, 1.0)
    g = np.clip(2.0 - np.abs(hx - 2.0), 0.0, 1.0)
    b = np.clip(2.0 - np.abs(hx - 4.0), 0.0, 1.0)
    value = np.linspace(0.0, 255.0, h)[:, None, None]
    return np.stack([b, g, r], axis=-1)[None, :, :] * value


_GENERATORS = {"noise": _noise, "edges": _edges, "bars": _bars, "hue": _hue}


def texture(kind, w, h, seed=1234, pad=2):
    """float64 (h, w + 2 * pad, 3) in [0, 255]"""
    tex = _GENERATORS[kind](w + 2 * pad, h, np.random.default_rng([seed, KINDS.index(kind)]))
    assert tex.shape == (h, w + 2 * pad, 3) and tex.dtype == np.float64 and tex.min() >= 0.0 and tex.max() <= 255.0
    return tex


def chroma_clip(lvm, ck, kind, seed=1234):
    """synth.Clip(**ck) with the texture of `kind`"""
    clip = lvm.synth.Clip(**ck)
    clip.tex = texture(kind, clip.w, clip.h, seed, clip.pad)
    return clip


def clip_fn(lvm, kind):
    """the clip_fn(ck, stream) of the shared bodies in helpers.py: stream s gets seed 1234 + s, as their default does"""
    return lambda ck, stream: chroma_clip(lvm, ck, kind, seed=1234 + stream)


# ---- every colour once -----------------------------------------------------------------------------------------------------------
def cube_values(n=64, seed=5):
    """n u8 values with 0, 1, 254, 255, the first value of every cell of the table ((514 u + 4) >> 12 = 0 .. 32), and 127 (weight 15);
    the rest drawn with the seed.  tests/test_chroma_cube.py asserts the coverage."""
    u = np.arange(256)
    cell = (514 * u + 4) >> 12
    must = {0, 1, 127, 254, 255} | {int(u[cell == c][0]) for c in range(33)}
    assert len(must) <= n <= 256
    rest = np.array(sorted(set(range(256)) - must))
    extra = np.random.default_rng(seed).choice(rest, size=n - len(must), replace=False)
    return np.array(sorted(must | {int(x) for x in extra}), np.uint8)


def cube_permutation(count, seed):
    return np.random.default_rng(seed).permutation(count)


def cube_frames(values, seed=9):
    """Two square u8 frames over all triples (B, G, R) in values^3: one in natural order (R fastest), one with the same pixels in
    the permutation cube_permutation(len(values)^3, seed): permuted.reshape(-1, 3) == natural.reshape(-1, 3)[perm].  256 values:
    4096 x 4096, 64 values: 512 x 512."""
    v = np.asarray(values, np.uint8)
    n = len(v)
    side = int(round((n ** 3) ** 0.5))
    assert side * side == n ** 3, "len(values)^3 must be a square"
    b, g, r = np.meshgrid(v, v, v, indexing="ij")
    flat = np.stack([b, g, r], axis=-1).reshape(-1, 3)
    perm = cube_permutation(n ** 3, seed)
    return np.ascontiguousarray(flat.reshape(side, side, 3)), np.ascontiguousarray(flat[perm].reshape(side, side, 3))
