"""The arithmetic of ilm_resolve_lighting_lut restated in numpy float32 (include/illuminant_hip.h defines it): one numpy operation per
rounded operation, in the header's order; the uniform values as the host computes them, the two divisors as reciprocals.  The fetch and
the coverage are tests/resolve_scaled_common.py's.  Nothing here asks the library anything."""
import numpy as np

from tests import resolve_scaled_common as rs
from tests.output_common import _clamp, _max0, _pow, _saturate

F = np.float32


class Blending:
    """IlmLUTBlending with the LUT textures as decoded float32 arrays of shape (N * rows, N * N, >= 3)."""

    def __init__(self, dark, bright, dark_level, bright_level, neutral_band_size=0.0, per_channel=False, lut_only=False,
                 dark_n=None, bright_n=None, dark_row=0, bright_row=0):
        self.dark, self.bright = np.asarray(dark, np.float32), np.asarray(bright, np.float32)
        self.dark_n = int(round(self.dark.shape[1] ** 0.5)) if dark_n is None else dark_n
        self.bright_n = int(round(self.bright.shape[1] ** 0.5)) if bright_n is None else bright_n
        self.dark_row, self.bright_row = dark_row, bright_row
        self.dark_level, self.neutral_band_size, self.bright_level = F(dark_level), F(neutral_band_size), F(bright_level)
        self.per_channel, self.lut_only = bool(per_channel), bool(lut_only)


def uniforms(dark_level, neutral_band_size, bright_level, per_channel):
    """The launch-uniform values, LUTResolve.fx:78-81,94,100-103, in float32 in the shader's order."""
    with np.errstate(all="ignore"):
        dark_level, neutral_band_size, bright_level = F(dark_level), F(neutral_band_size), F(bright_level)
        band_width = _saturate(bright_level - dark_level)
        neutral = np.fmin(neutral_band_size, band_width - F(0.01))
        has_band = bool(neutral > F(0.0))
        transition = (band_width - neutral) * F(0.5)
        return dict(band_width=band_width, neutral=neutral, has_band=has_band, normalize=(not per_channel) or has_band, transition=transition,
                    inv_transition=F(1.0) / transition, ramp=bool(bright_level > dark_level), inv_range=F(1.0) / (bright_level - dark_level))


def _lerp(x, y, t):
    return x + (y - x) * t


def lut_axis(c, n):
    """(i0, i1, f) of one saturated channel on a LUT of resolution n."""
    s = c * F(n - 1)
    fl = np.floor(s)
    i0 = np.minimum(fl.astype(np.int64), n - 1)
    return i0, np.minimum(i0 + 1, n - 1), s - fl


def read_lut(lut, n, row, a):
    """ReadLUT as the header defines it: a (..., 3) saturated float32; lattice point (ri, gi, bi) of row `row` is lut[row * n + gi, bi * n + ri]."""
    lut = np.asarray(lut, np.float32)[..., :3]
    r0, r1, fr = lut_axis(a[..., 0], n)
    g0, g1, fg = lut_axis(a[..., 1], n)
    b0, b1, fb = lut_axis(a[..., 2], n)
    fr, fg, fb = fr[..., None], fg[..., None], fb[..., None]

    def t(ri, gi, bi):
        return lut[row * n + gi, bi * n + ri]

    with np.errstate(all="ignore"):
        near = _lerp(_lerp(t(r0, g0, b0), t(r1, g0, b0), fr), _lerp(t(r0, g1, b0), t(r1, g1, b0), fr), fg)
        far = _lerp(_lerp(t(r0, g0, b1), t(r1, g0, b1), fr), _lerp(t(r0, g1, b1), t(r1, g1, b1), fr), fg)
        return _lerp(near, far, fb)


def lut_taps(n, row, a):
    """(rows, columns) of the eight texels read_lut reads, each (..., 8): what a test of tap selection compares against."""
    r0, r1, _ = lut_axis(a[..., 0], n)
    g0, g1, _ = lut_axis(a[..., 1], n)
    b0, b1, _ = lut_axis(a[..., 2], n)
    rows = np.stack([row * n + g for g in (g0, g0, g1, g1, g0, g0, g1, g1)], axis=-1)
    cols = np.stack([b * n + r for r, b in ((r0, b0), (r1, b0), (r0, b0), (r1, b0), (r0, b1), (r1, b1), (r0, b1), (r1, b1))], axis=-1)
    return rows, cols


def weight(light_rgb, normalize):
    """(..., 3): the luminance in every channel under `normalize` (0.144 is LUTResolve.fx:16's constant), else the light itself."""
    if not normalize:
        return light_rgb
    w = (light_rgb[..., 0] * F(0.299) + light_rgb[..., 1] * F(0.587)) + light_rgb[..., 2] * F(0.144)
    return np.repeat(w[..., None], 3, axis=-1)


def blend(tap, albedo, cfg, hdr):
    """LUTBlendedResolveWithAlbedoCommon and the plain epilogue over sampled light and albedo texels, both (..., 4) float32."""
    with np.errstate(all="ignore"):
        tap, albedo = np.asarray(tap, np.float32), np.asarray(albedo, np.float32)
        inverse_scale = F(hdr.InverseScaleFactor) if hdr.InverseScaleFactor != 0.0 else F(1.0)
        light = tap[..., :3] * (inverse_scale * F(2.0))
        a = _saturate(albedo[..., :3])
        u = uniforms(cfg.dark_level, cfg.neutral_band_size, cfg.bright_level, cfg.per_channel)
        w = weight(light, u["normalize"])
        dark = read_lut(cfg.dark, cfg.dark_n, cfg.dark_row, a)
        bright = read_lut(cfg.bright, cfg.bright_n, cfg.bright_row, a)
        if u["has_band"]:
            v = w[..., 0:1] - cfg.dark_level
            v3 = (v - u["transition"]) - u["neutral"]
            val1 = _lerp(dark, a, _saturate(v * u["inv_transition"]))
            blended = _lerp(val1, bright, _saturate(v3 * u["inv_transition"]))
        else:
            if u["ramp"]:
                w = _saturate(_max0(w - cfg.dark_level) * u["inv_range"])
            else:
                w = _saturate(w - cfg.dark_level)
            blended = _lerp(dark, bright, w)
        rgb = blended if cfg.lut_only else blended * light
        min_v, max_v = F(1.0) / F(256.0), F(99999.0)
        exposure = (_clamp(hdr.Exposure, min_v, max_v) - F(1.0)) + F(1.0)
        gamma = (_clamp(hdr.Gamma, 0.1, 4.0) - F(1.0)) + F(1.0)
        out = np.empty(rgb.shape[:-1] + (4,), np.float32)
        out[..., :3] = _pow(_max0(rgb + F(hdr.Offset)) * exposure, gamma)
        out[..., 3] = albedo[..., 3]
        return out


def resolve(light, albedo, dst_size, quad, cfg, hdr, lightmap_region=None, albedo_region=None, offset=None, lightmap_filter=rs.LINEAR,
            albedo_filter=rs.LINEAR):
    """Every pixel of a dst_size = (width, height) target, covered or not (rs.coverage says which are written); light and albedo decoded."""
    tap = rs.sample(light, dst_size, quad, lightmap_region, lightmap_filter, offset)
    texel = rs.sample(albedo, dst_size, quad, albedo_region, albedo_filter)
    return blend(tap, texel, cfg, hdr)
