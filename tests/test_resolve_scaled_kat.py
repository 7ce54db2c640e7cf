"""ilm_resolve_lighting_scaled without a GPU: the symbol in the header, the library, the ctypes table and the C# layer; the refusal that
needs no device; the numpy statement of the fetch (tests/resolve_scaled_common.py) on cases worked out by hand; the header's contract."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from illuminant_amd import abi, native
from tests import resolve_scaled_common as rs

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "ilm_resolve_lighting_scaled"


def header():
    return open(os.path.join(ROOT, "include", "illuminant_hip.h")).read()


def row(*reds):
    """a 1 x n texture whose red channel holds the given values"""
    t = np.zeros((1, len(reds), 4), np.float32)
    t[0, :, 0] = reds
    return t


def test_the_symbol_is_declared_exported_bound_and_in_the_csharp_file():
    text = header()
    stripped = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"^int32_t %s\((.*?)\);" % SYMBOL, stripped, flags=re.S | re.M).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert params == ["IlmHandle src_lightmap", "IlmHandle albedo", "IlmHandle dst", "const IlmHDRConfiguration* hdr", "const float quad[4]",
                      "const float lightmap_region[4]", "const float albedo_region[4]", "const float uv_offset[2]", "int32_t lightmap_filter",
                      "int32_t albedo_filter", "int32_t row_begin", "int32_t row_end"]
    for name, value in (("POINT", 0), ("LINEAR", 1)):
        assert re.search(r"^#define ILM_FILTER_%s\s+%d\b" % (name, value), text, flags=re.M), name
        assert getattr(abi, "FILTER_" + name) == value == getattr(rs, name)
    result, args = native.SYMBOLS[SYMBOL]
    assert result is C.c_int32 and len(args) == 12
    assert args[:3] == [abi.Handle] * 3 and args[3:8] == [C.c_void_p] * 5 and args[8:] == [C.c_int32] * 4
    assert hasattr(native.lib(), SYMBOL)
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s\b" % SYMBOL, nm)
    cs = open(os.path.join(ROOT, "integration", "IlluminantHip.cs")).read()
    assert (SYMBOL + " (ulong srcLightmap, ulong albedo, ulong dst, IlmHDRConfiguration* hdr, float* quad, float* lightmapRegion, "
            "float* albedoRegion, float* uvOffset, int lightmapFilter, int albedoFilter, int rowBegin, int rowEnd)") in cs
    assert "FILTER_POINT = 0" in cs and "FILTER_LINEAR = 1" in cs
    assert "#define ILM_ABI_VERSION 11" in text and "+ " + SYMBOL in text[:text.index("#define ILM_ABI_VERSION")]
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_csharp_binding.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr


def test_handles_are_looked_up_before_anything_else():
    lib = native.lib()
    hdr = abi.HDRConfiguration()
    quad = (C.c_float * 4)(0, 0, 4, 4)
    q = C.cast(quad, C.c_void_p)
    zero = abi.Handle(0)
    assert lib.ilm_resolve_lighting_scaled(zero, zero, zero, C.cast(C.byref(hdr), C.c_void_p), q, q, None, None, 1, 1, 0, 4) == abi.ERR_INVALID_HANDLE
    assert b"lightmap handle" in lib.ilm_last_error()
    # ... also with every other argument unusable
    assert lib.ilm_resolve_lighting_scaled(abi.Handle(123456789), zero, zero, None, None, None, None, None, 7, -3, 9, 2) == abi.ERR_INVALID_HANDLE


def test_the_contract_names_the_definitions_and_what_is_not_built():
    text = header()
    contract = text[text.index("/* The scaled, filtered resolve"):text.index("int32_t " + SYMBOL)]
    for word in ("DEFINED DEVIATION", "BitmapDrawCall", "BitmapCommon.fxh", "LightingRenderer.HDR.cs:99-151", "LightingRenderer.cs:1537-1645",
                 "u = r0 + (((float)px + 0.5f) - x) * (r1 - r0) / width", "u = fminf(fmaxf(u, r0), r1)", "Resolve.fx:34,49-50",
                 "a NaN coordinate becomes r0", "s = u - 0.5f, f = s - floorf(s)", "clamp((int)floorf(s) + 1, 0, size - 1)",
                 "lerp4(lerp4(t00, t10, fx), lerp4(t01, t11, fx), fy)", "clamps the COORDINATE, not the taps", "bleeds", "clamp((int)floorf(u), 0, size - 1)",
                 "computed in double", "keeps its bits", "writes nothing", "ILM_ERR_INVALID_HANDLE", "ILM_ERR_OUT_OF_RANGE", "Asynchronous",
                 "Not built", "world-space", "blendState", "LUT blending", "mip filtering"):
        assert word in contract, word


def test_two_texels_stretched_to_four_linear_and_point():
    src = row(0.0, 1.0)
    linear = rs.sample(src, (4, 1), (0, 0, 4, 1), filt=rs.LINEAR)[0, :, 0]
    # u = 0.25, 0.75, 1.25, 1.75; s = u - 0.5: taps (0, 0) w 0.75, (0, 1) w 0.25, (0, 1) w 0.75, (1, 1) w 0.25
    assert linear.tolist() == [0.0, 0.25, 0.75, 1.0]
    point = rs.sample(src, (4, 1), (0, 0, 4, 1), filt=rs.POINT)[0, :, 0]
    assert point.tolist() == [0.0, 0.0, 1.0, 1.0]
    (x0, x1, fx), _ = rs.axes(src.shape, (4, 1), (0, 0, 4, 1), (0, 0, 2, 1), rs.LINEAR)
    assert x0.tolist() == [0, 0, 0, 1] and x1.tolist() == [0, 1, 1, 1] and fx.tolist() == [0.75, 0.25, 0.75, 0.25]


def test_at_scale_one_the_coordinate_is_the_pixel_centre_exactly():
    for width in (37, 157):
        u = rs.coordinate(width, 0.0, width, 0.0, width)
        assert u.dtype == np.float32 and np.array_equal(u, np.arange(width, dtype=np.float32) + F(0.5))
        i0, i1, f = rs.taps(u, width, rs.LINEAR)
        assert np.array_equal(i0, np.arange(width)) and not f.any()              # weight 0 on the second tap: the texel itself
        assert np.array_equal(rs.taps(u, width, rs.POINT)[0], np.arange(width))


def test_integer_point_magnification_picks_the_texel_under_the_pixel():
    for factor in (2, 3):
        for size in (19, 13, 37):
            n = size * factor
            i0, _, _ = rs.taps(rs.coordinate(n, 0.0, n, 0.0, size), size, rs.POINT)
            assert np.array_equal(i0, np.arange(n) // factor), (factor, size)


def test_non_finite_offsets_pick_a_bound_of_the_region():
    size, r0, r1 = 24, 3.0, 19.0
    for offset, bound in ((np.nan, r0), (np.inf, r1), (-np.inf, r0), (1e9, r1), (-1e9, r0)):
        u = rs.coordinate(40, -2.5, 45.0, r0, r1, offset)
        assert np.array_equal(u, np.full(40, bound, np.float32)), offset
        i0, i1, f = rs.taps(u, size, rs.LINEAR)
        assert (i0 >= 0).all() and (i1 <= size - 1).all()
    # the far bound of a whole-texture region is `size`: POINT clamps the index to the last texel
    u = rs.coordinate(8, 0.0, 8.0, 0.0, size, np.inf)
    assert np.array_equal(rs.taps(u, size, rs.POINT)[0], np.full(8, size - 1))
    assert np.array_equal(rs.taps(u, size, rs.LINEAR)[1], np.full(8, size - 1))


def _round_to_float32(value):
    """A positive normal rational rounded to the nearest float32, ties to even, in exact arithmetic."""
    from fractions import Fraction
    if value == 0:
        return Fraction(0)
    sign, a, e = (1 if value > 0 else -1), abs(value), 0
    while a / Fraction(2) ** e >= 2 ** 24:
        e += 1
    while a / Fraction(2) ** e < 2 ** 23:
        e -= 1
    m = a / Fraction(2) ** e
    whole = m.numerator // m.denominator
    rest = m - whole
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and whole % 2 == 1):
        whole += 1
    return sign * whole * Fraction(2) ** e


def test_the_division_free_byte_decode_is_the_ieee_quotient_for_every_byte():
    """output.hip's unorm8: q = x * fl(1 / 255); fma(fma(-q, 255, x), fl(1 / 255), q) -- each fused operation rounded once -- equals
    fl(x / 255), what the 1:1 resolve's decode computes, for all 256 bytes; the plain product alone does not."""
    from fractions import Fraction
    r = _round_to_float32(Fraction(1, 255))
    assert float(r) == float(F(1.0) / F(255.0))
    plain_wrong = 0
    for x in range(256):
        want = _round_to_float32(Fraction(x, 255))
        assert float(want) == float(F(x) / F(255.0))
        q = _round_to_float32(x * r)
        plain_wrong += q != want
        assert _round_to_float32(q + _round_to_float32(x - q * 255) * r) == want, x
    assert plain_wrong > 100
    source = open(os.path.join(ROOT, "illuminant_amd", "csrc", "output.hip")).read()
    assert "return __builtin_fmaf(__builtin_fmaf(-q, 255.0f, x), r, q);" in source and "const float q = x * r;" in source


def test_coverage_is_the_pixels_whose_centre_the_quad_contains():
    c = rs.coverage((8, 6), (1.5, 0.25, 3.0, 2.5))
    # centres 1.5, 2.5, 3.5 in [1.5, 4.5); rows 0.5, 1.5, 2.5 in [0.25, 2.75)
    assert np.argwhere(c.any(axis=0)).ravel().tolist() == [1, 2, 3] and np.argwhere(c.any(axis=1)).ravel().tolist() == [0, 1, 2]
    assert not rs.coverage((8, 6), (100.0, 0.0, 5.0, 5.0)).any() and not rs.coverage((8, 6), (0.0, 0.0, 0.0, 5.0)).any()
    assert rs.coverage((8, 6), (-3.0, -3.0, 50.0, 50.0), 2, 4).sum() == 16
