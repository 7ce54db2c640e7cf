"""ilm_resolve_lighting_lut without a GPU: the numpy statement of its arithmetic (tests/resolve_lut_common.py) on cases worked out by hand;
the symbol and the struct in the header, the library, the ctypes table and the C# layer; the refusal that needs no device; the header's
contract."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from illuminant_amd import abi, native
from tests import output_common as oc
from tests import resolve_lut_common as rl

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "illuminant_hip.h")
SYMBOL = "ilm_resolve_lighting_lut"


def header():
    return open(HEADER).read()


def constant_lut(n, value, rows=1):
    return np.full((n * rows, n * n, 4), value, np.float32)


def pixel(light, albedo, cfg, hdr=None):
    """One pixel through the statement: light and albedo as rgb triples; alpha 1."""
    hdr = hdr or oc.hdr_configuration(inverse_scale=0.5)          # light = tap * (0.5 * 2): the tap itself
    tap, texel = np.array([list(light) + [1.0]], np.float32), np.array([list(albedo) + [1.0]], np.float32)
    return rl.blend(tap, texel, cfg, hdr)[0, :3].tolist()


def gray(l):
    """the luminance weight of light (l, l, l), rounded as the shader rounds it"""
    l = F(l)
    return (l * F(0.299) + l * F(0.587)) + l * F(0.144)


# ---- the statement on hand-derived values -----------------------------------------------------------------------------------------------
def test_the_three_zones_of_a_neutral_band():
    """DarkLevel 0.25, BrightLevel 0.75, NeutralBandSize 0.25: bandWidth 0.5, neutral min(0.25, 0.49) = 0.25, transition 0.125.  Dark LUT
    0.25, bright LUT 0.75, albedo 0.5, LUTOnly: below 0.25 the dark LUT, over [0.375, 0.625] the albedo, above 0.75 the bright LUT, and a
    ramp between; every value below is exact in binary."""
    u = rl.uniforms(0.25, 0.25, 0.75, False)
    assert (u["band_width"], u["neutral"], u["has_band"], u["normalize"], u["transition"], u["inv_transition"]) == (0.5, 0.25, True, True, 0.125, 8.0)
    cfg = rl.Blending(constant_lut(2, 0.25), constant_lut(2, 0.75), 0.25, 0.75, 0.25, lut_only=True)
    for l, want in ((0.0, 0.25), (0.2, 0.25), (0.4, 0.5), (0.5, 0.5), (0.6, 0.5), (0.75, 0.75), (3.0, 0.75)):
        assert pixel((l, l, l), (0.5, 0.5, 0.5), cfg) == [want] * 3, l
    # inside the two transitions, by the formula's own steps on scalars
    for l in (0.3, 0.7):
        v = gray(l) - F(0.25)
        t1 = min(max(v * F(8.0), F(0.0)), F(1.0))
        t2 = min(max(((v - F(0.125)) - F(0.25)) * F(8.0), F(0.0)), F(1.0))
        val1 = F(0.25) + (F(0.5) - F(0.25)) * t1
        want = val1 + (F(0.75) - val1) * t2
        assert 0.25 < want < 0.75 and want != 0.5
        assert pixel((l, l, l), (0.5, 0.5, 0.5), cfg) == [float(want)] * 3, l
    # without LUTOnly the blend is multiplied by the light
    cfg.lut_only = False
    assert pixel((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), cfg) == [0.25] * 3


def test_both_branches_without_a_band():
    """NeutralBandSize 0: no band.  BrightLevel > DarkLevel: w = saturate(max(0, w - 0.25) * 2); else the HACK branch saturate(w - Dark).
    PerChannel, so the weight is the light itself and every number is exact."""
    u = rl.uniforms(0.25, 0.0, 0.75, True)
    assert (u["has_band"], u["normalize"], u["ramp"], u["inv_range"]) == (False, False, True, 2.0)
    cfg = rl.Blending(constant_lut(2, 0.25), constant_lut(2, 0.75), 0.25, 0.75, 0.0, per_channel=True, lut_only=True)
    # channels 0.125 (below), 0.5 (half way), 2 (above): 0.25, 0.25 + 0.5 * 0.5, 0.75
    assert pixel((0.125, 0.5, 2.0), (0.5, 0.5, 0.5), cfg) == [0.25, 0.5, 0.75]
    for dark_level, bright_level in ((0.5, 0.5), (0.5, 0.25)):
        u = rl.uniforms(dark_level, 0.0, bright_level, True)
        assert (u["has_band"], u["ramp"]) == (False, False)
        cfg = rl.Blending(constant_lut(2, 0.25), constant_lut(2, 0.75), dark_level, bright_level, 0.0, per_channel=True, lut_only=True)
        # saturate(w - 0.5): 0, 0.25, 1
        assert pixel((0.25, 0.75, 1.75), (0.5, 0.5, 0.5), cfg) == [0.25, 0.375, 0.75]


def test_per_channel_is_overridden_by_a_band_and_differs_from_luminance_without_one():
    light = (1.0, 0.0, 0.0)                          # luminance 0.299: inside the first transition of the band below
    banded = rl.Blending(constant_lut(2, 0.25), constant_lut(2, 0.75), 0.25, 0.75, 0.25, per_channel=True, lut_only=True)
    assert rl.uniforms(0.25, 0.25, 0.75, True)["normalize"] is True
    got = pixel(light, (0.5, 0.5, 0.5), banded)
    t1 = (F(1.0) * F(0.299) - F(0.25)) * F(8.0)
    assert got == [float(F(0.25) + F(0.25) * t1)] * 3 and 0.25 < got[0] < 0.5          # one weight for the three channels
    per_channel = rl.Blending(constant_lut(2, 0.25), constant_lut(2, 0.75), 0.25, 0.75, 0.0, per_channel=True, lut_only=True)
    assert pixel(light, (0.5, 0.5, 0.5), per_channel) == [0.75, 0.25, 0.25]
    luminance = rl.Blending(constant_lut(2, 0.25), constant_lut(2, 0.75), 0.25, 0.75, 0.0, per_channel=False, lut_only=True)
    w = (F(0.299) - F(0.25)) * F(2.0)
    assert pixel(light, (0.5, 0.5, 0.5), luminance) == [float(F(0.25) + F(0.5) * w)] * 3


def test_the_band_exists_from_one_ulp_above_zero():
    """neutral = fminf(NeutralBandSize, bandWidth - 0.01f) > 0 decides: the smallest positive float is a band, 0 is none.  At the middle of
    the levels the band gives the albedo (first ramp done, second not begun), no band gives the mean of the LUTs."""
    tiny = np.nextafter(F(0.0), F(1.0))
    assert tiny > 0 and rl.uniforms(0.25, tiny, 0.75, True)["has_band"] is True and rl.uniforms(0.25, tiny, 0.75, True)["neutral"] == tiny
    assert rl.uniforms(0.25, 0.0, 0.75, True)["has_band"] is False and rl.uniforms(0.25, -tiny, 0.75, True)["has_band"] is False
    # bandWidth - 0.01 bounds it: levels 0.01 apart or closer never have a band, whatever the size asked for
    assert rl.uniforms(0.5, 1.0, 0.505, False)["has_band"] is False and rl.uniforms(0.5, 1.0, 0.25, False)["has_band"] is False
    u = rl.uniforms(0.25, 1.0, 0.75, False)
    assert u["neutral"] == F(0.5) - F(0.01) and u["transition"] == (F(0.5) - u["neutral"]) * F(0.5) 
    assert 0.00499999 < u["transition"] < 0.00500001                   # the smallest transition there is: never a zero divisor
    dark, bright = constant_lut(2, 0.25), constant_lut(2, 0.75)
    # the light whose luminance is exactly 0.5: blue alone, 0.5 / 0.144 does not round -- red and green off, per-channel off
    light = (0.0, 0.0, float(F(0.5) / F(0.144)))
    w = F(light[2]) * F(0.144)
    with_band = pixel(light, (0.375, 0.375, 0.375), rl.Blending(dark, bright, 0.25, 0.75, tiny, lut_only=True))
    without = pixel(light, (0.375, 0.375, 0.375), rl.Blending(dark, bright, 0.25, 0.75, 0.0, lut_only=True))
    v = w - F(0.25)
    t1 = min(max(v * F(4.0), F(0.0)), F(1.0))
    t2 = min(max(((v - F(0.25)) - tiny) * F(4.0), F(0.0)), F(1.0))
    val1 = F(0.25) + (F(0.375) - F(0.25)) * t1
    assert with_band == [float(val1 + (F(0.75) - val1) * t2)] * 3
    assert without == [float(F(0.25) + F(0.5) * min(max(max(v, F(0.0)) * F(2.0), F(0.0)), F(1.0)))] * 3
    assert abs(with_band[0] - 0.375) < 1e-6 and abs(without[0] - 0.5) < 1e-6


@pytest.mark.parametrize("n", (2, 5, 17))
def test_lattice_points_return_the_texel_and_midpoints_the_mean(n):
    """N - 1 a power of two: s = a * (N - 1) is exact.  Texels are multiples of 1 / 64, so every mean below is exact too."""
    rng = np.random.default_rng(n)
    rows = 2
    lut = rng.integers(0, 64, (n * rows, n * n, 4)).astype(np.float32) / F(64.0)
    idx = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 3)        # (ri, gi, bi)
    a = idx.astype(np.float32) / F(n - 1)
    for row in range(rows):
        got = rl.read_lut(lut, n, row, a)
        want = lut[row * n + idx[:, 1], idx[:, 2] * n + idx[:, 0], :3]
        assert np.array_equal(got, want)
    # midpoints of every cell: the mean of its eight corners
    cell = idx[(idx < n - 1).all(axis=1)]
    mid = (cell.astype(np.float32) + F(0.5)) / F(n - 1)
    got = rl.read_lut(lut, n, 1, mid)
    corners = [lut[n + cell[:, 1] + dg, (cell[:, 2] + db) * n + cell[:, 0] + dr, :3] for dr in (0, 1) for dg in (0, 1) for db in (0, 1)]
    assert np.array_equal(got, sum(corners) / F(8.0))
    rows_read, cols_read = rl.lut_taps(n, 1, mid)
    assert rows_read.min() >= n and rows_read.max() < 2 * n and cols_read.min() >= 0 and cols_read.max() < n * n
    # exactly 1 is the last lattice point, read twice with weight 0: never the neighbouring slice or row
    one = np.ones((1, 3), np.float32)
    r, c = rl.lut_taps(n, 0, one)
    assert (r == n - 1).all() and (c == n * n - 1).all()
    assert np.array_equal(rl.read_lut(lut, n, 0, one)[0], lut[n - 1, n * n - 1, :3])


# ---- header, library, bindings ----------------------------------------------------------------------------------------------------------
FIELDS = ["DarkLUT", "BrightLUT", "DarkResolution", "BrightResolution", "DarkRowCount", "BrightRowCount", "DarkRow", "BrightRow",
          "DarkLevel", "NeutralBandSize", "BrightLevel", "PerChannel", "LUTOnly"]


def test_the_struct_has_the_layout_of_its_ctypes_mirror(tmp_path):
    assert [name for name, _ in abi.LUTBlending._fields_] == FIELDS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(IlmLUTBlending));']
    lines += ['  printf("%s %%zu\\n", offsetof(IlmLUTBlending, %s));' % (f, f) for f in FIELDS]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == C.sizeof(abi.LUTBlending) == abi.EXPECTED_SIZES["IlmLUTBlending"][1] == 64
    assert {f: int(v) for f, v in out.items()} == {f: getattr(abi.LUTBlending, f).offset for f in FIELDS}
    assert abi.LUTBlending.LUTOnly.offset == 56


def test_the_symbol_is_declared_exported_bound_and_in_the_csharp_file():
    text = header()
    stripped = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"^int32_t %s\((.*?)\);" % SYMBOL, stripped, flags=re.S | re.M).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert params == ["IlmHandle src_lightmap", "IlmHandle albedo", "IlmHandle dst", "const IlmHDRConfiguration* hdr", "const IlmLUTBlending* lut",
                      "const float quad[4]", "const float lightmap_region[4]", "const float albedo_region[4]", "const float uv_offset[2]",
                      "int32_t lightmap_filter", "int32_t albedo_filter", "int32_t row_begin", "int32_t row_end"]
    result, args = native.SYMBOLS[SYMBOL]
    assert result is C.c_int32 and len(args) == 13
    assert args[:3] == [abi.Handle] * 3 and args[3:9] == [C.c_void_p] * 6 and args[9:] == [C.c_int32] * 4
    assert hasattr(native.lib(), SYMBOL)
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s\b" % SYMBOL, nm)
    cs = open(os.path.join(ROOT, "integration", "IlluminantHip.cs")).read()
    assert (SYMBOL + " (ulong srcLightmap, ulong albedo, ulong dst, IlmHDRConfiguration* hdr, IlmLUTBlending* lut, float* quad, "
            "float* lightmapRegion, float* albedoRegion, float* uvOffset, int lightmapFilter, int albedoFilter, int rowBegin, int rowEnd)") in cs
    struct = re.search(r"Size = 64\)\]\s+public struct IlmLUTBlending \{(.*?)\}", cs, flags=re.S).group(1)
    assert re.findall(r"public (\w+) (\w+);", struct) == [("ulong" if f.endswith("LUT") else "float" if f in FIELDS[8:11] else "int", f) for f in FIELDS]
    assert "#define ILM_ABI_VERSION 11" in text and "+ " + SYMBOL in text[:text.index("#define ILM_ABI_VERSION")]
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_csharp_binding.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr


def test_handles_are_looked_up_before_anything_else():
    lib = native.lib()
    hdr, lut = abi.HDRConfiguration(), abi.LUTBlending()
    quad = (C.c_float * 4)(0, 0, 4, 4)
    q = C.cast(quad, C.c_void_p)
    zero = abi.Handle(0)
    h, l = C.cast(C.byref(hdr), C.c_void_p), C.cast(C.byref(lut), C.c_void_p)
    assert lib.ilm_resolve_lighting_lut(zero, zero, zero, h, l, q, q, q, None, 1, 1, 0, 4) == abi.ERR_INVALID_HANDLE
    assert b"lightmap handle" in lib.ilm_last_error()
    # ... also with every other argument unusable
    assert lib.ilm_resolve_lighting_lut(abi.Handle(123456789), abi.Handle(5), zero, None, None, None, None, None, None, 7, -3, 9, 2) == abi.ERR_INVALID_HANDLE


def test_the_contract_states_the_arithmetic_the_deviation_and_the_refusals():
    text = header()
    contract = text[text.index("/* The LUT-blended resolve"):text.index("int32_t " + SYMBOL)]
    for word in ("ScreenSpaceLUTBlendedLightingResolveWithAlbedo", "LUTResolve.fx:61-115", "LightingRenderer.cs:1574-1577", "IlluminantMaterials.cs:139-147",
                 "ilm_resolve_lighting_scaled's", "light = tap * (InverseScaleFactor * 2)", "a = saturate(albedo.rgb)", "a NaN becomes 0",
                 "bandWidth = saturate(BrightLevel - DarkLevel)", "neutral = fminf(NeutralBandSize, bandWidth - 0.01f)", "hasNeutralBand = neutral > 0",
                 "normalize = !PerChannel || hasNeutralBand", "(light.r * 0.299f + light.g * 0.587f) + light.b * 0.144f", "t = (bandWidth - neutral) * 0.5f",
                 "v3 = (v - t) - neutral", "HACK", "host-side reciprocals", "LUTOnly ? blended : blended * light.rgb",
                 "pow(max(0, rgb + Offset) * Exposure, Gamma)",
                 "DEFINED DEVIATION", "LUTCommon.fxh", "ColorLUT", "width N * N and height N * R", "column bi * N + ri, texel row Row * N + gi",
                 "s = c * (float)(N - 1), i0 = min((int)floorf(s), N - 1), i1 = min(i0 + 1, N - 1), f = s - floorf(s)",
                 "lerp3(lerp3(lerp3(T000, T100, fr), lerp3(T010, T110, fr), fg), lerp3(lerp3(T001, T101, fr), lerp3(T011, T111, fr), fg), fb)",
                 "by integer arithmetic", "neighbouring slice or row", "half-texel inset",
                 "Refused", "ILM_ERR_INVALID_HANDLE", "albedo == 0", "hdr, lut,", "LUT blending is not compatible with this type of", "Resolution < 2",
                 "RowCount < 1", "not N * N x N * R", "outside [0, R)", "not finite", "different contexts", "ResolveToSRGB", "dithering", "Asynchronous"):
        assert word in contract, word
    # the scaled resolve's contract stands as it was, and the 1:1 entry point points here
    assert "Not bound: AlbedoIsSRGB.  The LUT-blended technique is ilm_resolve_lighting_lut." in text
