"""The combine rules of ilm_ctx_set_light_blend_function (include/illuminant_hip.h, "Light blend functions") in numpy, for the tests of
the six light passes.  Nothing here shades a light: the rules are fed per-light SOURCE images -- one light alone on a zero clear colour,
from the oracle the pass's own tests use -- in which rgb is the pair's contribution and alpha is 1 where the (pixel, light) pair
contributes and 0 where it does not.  fp32 throughout, np.float16 round trips for the fp16-per-light model."""
import numpy as np

from illuminant_amd import abi

F = np.float32
ADD, REVERSE_SUBTRACT, MAX, MIN = 0, 1, 2, 3
FUNCTIONS = (ADD, REVERSE_SUBTRACT, MAX, MIN)
NAMES = {ADD: "ADD", REVERSE_SUBTRACT: "REVERSE_SUBTRACT", MAX: "MAX", MIN: "MIN"}


def half(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def channel_functions(color_function, alpha_function):
    return (color_function, color_function, color_function, alpha_function)


def contributes(source):
    """the pair's mask: alpha of a single-light image on a zero clear colour counts the contributing pairs of the pixel (0 or 1)"""
    a = np.asarray(source, np.float32)[..., 3]
    assert np.isin(a, (0.0, 1.0)).all(), "a source image holds one light on a zero clear colour"
    return a == 1.0


def source_value(source):
    """c = (the pair's rgb contribution, 1)"""
    c = np.array(source, np.float32, copy=True)
    c[..., 3] = 1.0
    return c


def list_order_sum(sources, shape):
    """S of the full-frame passes: the contributing pairs in list order, from zero, one rounding per addition"""
    s = np.zeros(shape, np.float32)
    for src in sources:
        m = contributes(src)
        s[m] = (s[m] + source_value(src)[m]).astype(np.float32)
    return s


def combine_fp32(base, sources, color_function, alpha_function, total=None):
    """ILM_BLEND_FP32_ACCUMULATE.  base (H, W, 4) float32 as the pass reads it; total: the sum S an ADD call forms (the device's own, where
    a test wants the bits), else the list-order sum of the sources."""
    base = np.asarray(base, np.float32)
    if total is None:
        total = list_order_sum(sources, base.shape)
    out = np.empty_like(base)
    for ch, f in enumerate(channel_functions(color_function, alpha_function)):
        b = base[..., ch]
        if f == ADD:
            out[..., ch] = (b + total[..., ch]).astype(np.float32)
        elif f == REVERSE_SUBTRACT:
            out[..., ch] = (b - total[..., ch]).astype(np.float32)
        else:
            m = np.full(b.shape, -np.inf if f == MAX else np.inf, np.float32)
            for src in sources:
                c = source_value(src)[..., ch]
                with np.errstate(invalid="ignore"):
                    take = contributes(src) & ((c > m) if f == MAX else (c < m))
                m = np.where(take, c, m)
            with np.errstate(invalid="ignore"):
                out[..., ch] = np.where((m > b) if f == MAX else (m < b), m, b)
    return out


def combine_fp16(base, sources, color_function, alpha_function):
    """ILM_BLEND_FP16_PER_LIGHT: dst = half(base), then every contributing pair in list order with s = half(c)"""
    dst = half(base)
    for src in sources:
        m = contributes(src)
        s = half(source_value(src))
        for ch, f in enumerate(channel_functions(color_function, alpha_function)):
            d, v = dst[..., ch], s[..., ch]
            with np.errstate(invalid="ignore"):
                if f == ADD:
                    new = half((d + v).astype(np.float32))
                elif f == REVERSE_SUBTRACT:
                    new = half((d - v).astype(np.float32))
                elif f == MAX:
                    new = np.where(v > d, v, d)
                else:
                    new = np.where(v < d, v, d)
            dst[..., ch] = np.where(m, new, d)
    return dst


def to_stored(image, fmt):
    """the store conversion, after the combine: HALF4 rounds once, RGBA8 saturates"""
    image = np.asarray(image, np.float32)
    if fmt == abi.LIGHTMAP_FLOAT4:
        return image.copy()
    if fmt == abi.LIGHTMAP_HALF4:
        return image.astype(np.float16)
    return np.rint((np.clip(image, F(0), F(1)) * F(255)).astype(np.float32)).astype(np.uint8)


def from_stored(texels, fmt):
    if fmt == abi.LIGHTMAP_RGBA8:
        return (np.asarray(texels, np.uint8).astype(np.float32) / F(255)).astype(np.float32)
    return np.asarray(texels).astype(np.float32)


def reverse_subtract_bound(total_want, scale, atol):
    """|got - want| of base - S: the base is exact and S is within the project's 1e-4 of S_want (the usual relative bound on the
    difference would ask for more than its terms carry)"""
    return 1e-4 * np.abs(np.asarray(total_want, np.float64)) + atol * np.asarray(scale, np.float64)
