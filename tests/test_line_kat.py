"""Known answers of the line-light restatement (tests/line_common.py), derived by hand from LineLight.fx:7-42, LineLightCore.fxh:17-120,
FBPBR.fxh:25-101 and ConeTrace.fxh:37-139, and the defined acos against float64.  No GPU.

Measured here (printed by the tests before they assert): acos_defined differs from float64 acos by at most 4.02e-7 on the test's sample
(4.12e-7 on tools/acos_defined_error.py's 2^24 inputs; bound 2^-21 = 4.77e-7); the float32 opacity term differs from the float64
evaluation with the true acos by at most 1.02e-6 on the four KAT geometries (9.1e-7, 1.02e-6, 2.6e-7, 5.5e-7; bound 8 * 2^-21 = 3.81e-6);
the rectangle term's solid angle differs from the right pyramid's closed form by at most 2.8e-7 on the five cases.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import line_common as lc

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACOS_BOUND = 2.0 ** -21
# four acos at 2^-21 each, times the illuminance weight 0.2 * 5 (at most 1), doubled for the roundings of the sum and of the arguments
OPACITY_BOUND = 8 * 2.0 ** -21


@pytest.fixture(autouse=True)
def entry_point():
    """what the restatement restates must exist: the library exports the entry point, the binding knows it and the device header
    defines the acos.  (Most cases below exercise the Python restatement alone -- they pin it, as the GPU tests are only as good as it
    is -- and it is this fixture that ties them to the feature: without the entry point none of them passes.)"""
    assert "ilm_render_line_lights" in native.SYMBOLS
    assert hasattr(native.lib(), "ilm_render_line_lights")
    assert hasattr(native, "render_line_lights")
    assert "float acos_defined(float x)" in open(os.path.join(ROOT, "illuminant_amd", "csrc", "hlsl_math.hpp")).read()


def ground(width, height, z=0.0):
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
    n = width * height
    return [xx.ravel(), yy.ravel(), np.full(n, z, np.float32)], [np.zeros(n, np.float32), np.zeros(n, np.float32), np.ones(n, np.float32)]


def test_header_binding_and_csharp_agree_on_the_symbol():
    text = open(os.path.join(ROOT, "include", "illuminant_hip.h")).read()
    decl = re.search(r"^int32_t ilm_render_line_lights\(([^)]*)\)", text, flags=re.M).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in decl.split(",")] == [
        "IlmHandle", "const IlmLightVertex*", "int32_t", "const IlmEnvironment*", "const IlmDistanceFieldUniforms*", "IlmHandle", "IlmHandle",
        "const float", "IlmHandle", "int32_t", "int32_t", "IlmRenderStats*"]
    assert native.SYMBOLS["ilm_render_line_lights"] == native.SYMBOLS["ilm_render_directional_lights"]
    cs = open(os.path.join(ROOT, "integration", "IlluminantHip.cs")).read()
    assert "ilm_render_line_lights (ulong ctx, LightVertex* lights, int lightCount" in cs
    assert re.search(r"#define ILM_ABI_VERSION 11\b", text)


def test_handles_are_validated_without_a_device():
    lib = native.lib()
    env, dfu = scenes.environment(), lc.no_field_uniforms()
    assert lib.ilm_render_line_lights(abi.Handle(0), None, 0, C.byref(env), C.byref(dfu), abi.Handle(0), abi.Handle(0), None, abi.Handle(0), 0, 0,
                                      None) == abi.ERR_INVALID_HANDLE
    assert b"context" in lib.ilm_last_error()
    assert lib.ilm_render_line_lights(abi.Handle(123456789), None, 0, C.byref(env), C.byref(dfu), abi.Handle(0), abi.Handle(0), None,
                                      abi.Handle(0), 0, 0, None) == abi.ERR_INVALID_HANDLE


def test_the_device_header_holds_the_restatements_coefficients():
    """acos_defined of hlsl_math.hpp and of the restatement are the same polynomial: the literals, highest coefficient first"""
    text = open(os.path.join(ROOT, "illuminant_amd", "csrc", "hlsl_math.hpp")).read()
    body = text[text.index("ILM_DEV float acos_defined(float x)"):]
    body = body[:body.index("\n}\n")]
    literals = [F(float(m)) for m in re.findall(r"(-?\d+\.\d+)f;", body)][:8]
    assert literals == [lc.ACOS_COEFFICIENTS[k] for k in range(7, -1, -1)]
    assert "fma" not in body and "sqrtf(1.0f - a) * p" in body and "kPi - r" in body


def test_acos_defined_against_float64():
    n = 1 << 20
    k = np.arange(1, 150, dtype=np.float64)
    x = np.concatenate([(np.arange(n + 1, dtype=np.float64) / n * 2 - 1), [-1.0, 1.0, 0.0, -0.0], 1 - 2.0 ** -k, -1 + 2.0 ** -k, 2.0 ** -k,
                        -(2.0 ** -k)]).astype(np.float32)
    got = lc.acos_defined(x)
    assert got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - np.arccos(x.astype(np.float64)))
    print("acos_defined: largest |error| %.4g at x = %r (bound %.4g)" % (err.max(), float(x[err.argmax()]), ACOS_BOUND))
    assert err.max() <= ACOS_BOUND
    assert lc.acos_defined(F(1)) == 0 and lc.acos_defined(F(-1)) == lc.PI
    outside = lc.acos_defined(np.array([1.0000001, -1.0000001, 2.0, -3.0, np.inf, -np.inf, np.nan], np.float32))
    assert np.isnan(outside).all()


@pytest.mark.parametrize("half_length,radius,height", [(20.0, 4.0, 15.0), (22.0, 0.5, 8.0), (3.0, 1.0, 40.0), (50.0, 2.0, 60.0), (8.0, 8.0, 5.0)])
def test_the_rectangle_term_is_the_right_pyramids_solid_angle(half_length, radius, height):
    """a pixel under the midpoint of a horizontal segment (u = 0.5), normal up: the rectangle faces the pixel squarely, and its solid
    angle is rightPyramidSolidAngle (FBPBR.fxh:25-31) with a = |delta| / 2, b = radius, h = the distance"""
    light = lc.line_light((30.0 - half_length, 17.0, height), (30.0 + half_length, 17.0, height), radius)
    parts = {}
    opacity, u = lc.opacity_term(lc.v3(30.0, 17.0, 0.0), lc.v3(0.0, 0.0, 1.0), lc.prepare(light, lc.field_uniforms()), parts)
    assert u == 0.5
    a, b, h = half_length, radius, height
    want = 4 * np.arcsin(a * b / np.sqrt((a * a + h * h) * (b * b + h * h)))
    print("solid angle %.9g, closed form %.9g, difference %.3g" % (float(parts["solid_angle"]), want, float(parts["solid_angle"]) - want))
    assert abs(float(parts["solid_angle"]) - want) <= OPACITY_BOUND
    assert 0 < opacity <= 1


def test_float32_opacity_against_float64_with_the_true_acos():
    """the KAT scenes: a 64 x 48 ground plane under the four geometries, none of whose pixels lies on a segment's axis"""
    pos, normal = ground(64, 48)
    worst = []
    for start, end, radius in lc.KAT_GEOMETRIES:
        light = lc.line_light(start, end, radius)
        got, u = lc.opacity_term(pos, normal, lc.prepare(light, lc.field_uniforms()))
        want, _ = lc.opacity_term_float64(pos, normal, light)
        assert np.isfinite(want).all() and (want > 0).all()
        worst.append(float(np.abs(got.astype(np.float64) - want).max()))
        print("start %r end %r radius %g: largest |float32 - float64| %.3g (bound %.3g), opacity %.3g .. %.3g" % (
            start, end, radius, worst[-1], OPACITY_BOUND, want.min(), want.max()))
    assert max(worst) <= OPACITY_BOUND


def degenerate_lights():
    nan = float("nan")
    return {"radius 0": lc.line_light((2.0, 2.0, 6.0), (9.0, 4.0, 6.0), 0.0, casts_shadows=False),
            "start == end": lc.line_light((5.0, 3.0, 6.0), (5.0, 3.0, 6.0), 2.0, casts_shadows=False),
            "NaN start": lc.line_light((nan, 2.0, 6.0), (9.0, 4.0, 6.0), 2.0, casts_shadows=False),
            "NaN end z": lc.line_light((2.0, 2.0, 6.0), (9.0, 4.0, nan), 2.0, casts_shadows=False)}


@pytest.mark.parametrize("which", ["radius 0", "start == end", "NaN start", "NaN end z"])
def test_degenerate_lights_light_nothing(oracle, which):
    """each gives opacity 0 and a discard on every pixel: the frame keeps the ambient value, alpha included; the pairs are counted"""
    w, h = 12, 7
    ambient = (0.0625, 0.125, 0.25, 1.0)
    out = lc.render(oracle, [degenerate_lights()[which]], scenes.environment(), lc.no_field_uniforms(), None, None, ambient, w, h)
    assert np.array_equal(out.image, np.broadcast_to(np.asarray(ambient, np.float32), (h, w, 4)))
    assert out.stats == (0, w * h, 0) and out.detail == {}


def test_pixels_on_the_segments_axis_are_discarded(oracle):
    """a segment in the ground plane along x at y = 3: on row 3 the pixels beyond its ends have forward = +-left, up = cross(left,
    forward) = 0, and those between them sit on the closest point itself (forward = normalize(0)): opacity 0, discarded.  The
    other rows are lit."""
    w, h = 12, 7
    light = lc.line_light((3.0, 3.0, 0.0), (8.0, 3.0, 0.0), 2.0, casts_shadows=False)
    ambient = (0.0, 0.0, 0.0, 1.0)
    out = lc.render(oracle, [light], scenes.environment(), lc.no_field_uniforms(), None, None, ambient, w, h)
    assert (out.image[3, :, 3] == 1).all() and (out.image[3, :, :3] == 0).all()
    assert all((x, 3, 0) not in out.detail for x in range(w))
    # (a ground-plane pixel beside the axis sees the light edge-on: normal . direction = 0, so it is dark too -- raise the light to see it)
    raised = lc.line_light((3.0, 3.0, 4.0), (8.0, 3.0, 4.0), 2.0, casts_shadows=False)
    out = lc.render(oracle, [raised], scenes.environment(), lc.no_field_uniforms(), None, None, ambient, w, h)
    assert (out.image[..., 3] == 2).all() and (out.image[..., 0] > 0).all()


EMPTY = lambda p: F(1000.0)          # a hand-built field: nothing within reach


def trace_uniforms(step_limit=64):
    return lc.field_uniforms(step_limit=step_limit, min_step_size=1.5, long_step_factor=0.75, max_cone_radius=8.0)


def test_a_ray_that_has_ended_keeps_sampling():
    """a pixel beyond the start of a short, thick segment (u = 0, o = (4 + 1) / 10): the rays towards u - o and u both aim at the start,
    the one towards u + o at the middle, 3.8 further away.  With steps of 1.5 the first two end after 7 iterations and the third after
    10.  Every iteration samples all three: samples = 3 * iterations, and the iteration count is the longest ray's"""
    light = lc.line_light((20.0, 10.0, 12.0), (30.0, 10.0, 12.0), 4.0)
    dfu = trace_uniforms()
    r = lc.prepare(light, dfu)
    assert r.offset == 0.5
    calls = []

    def slow_field(p):
        calls.append([float(c) for c in p])
        return F(2.0)            # every step is the minimum step: max(2 * 0.75, 1.5) = 1.5

    opacity, u = lc.opacity_term(lc.v3(10.0, 10.0, 0.0), lc.v3(0.0, 0.0, 1.0), r)
    assert u == 0 and opacity > 0
    cone, samples, facts = lc.line_trace(slow_field, (10.0, 10.0, 0.0), (0.0, 0.0, 1.0), r, u, dfu, True)
    assert facts["along"] == [0, 0, 0.5]
    assert samples == 3 * facts["iterations"] == len(calls)
    # lengths: sqrt(100 + 10.5^2) - 4 = 10.5 and sqrt(225 + 10.5^2) - 4 = 14.31: 0.5 + 1.5 k reaches them at k = 7 and k = 10
    assert facts["ended"] == (7, 7, 10) and facts["iterations"] == 10
    # after the first ray ended its samples repeat its end point, origin + direction * length
    first = calls[0::3]
    end_point = [float(facts["start"][k]) + float(facts["rays"][0][k]) * float(facts["lengths"][0]) for k in range(3)]
    assert len(first) == 10 and all(np.allclose(c, end_point, atol=1e-4) for c in first[7:])
    assert not np.allclose(first[6], end_point, atol=1e-2)
    assert facts["positions"][0] == facts["lengths"][0] and facts["positions"][2] == facts["lengths"][2]
    # the cone radius grows by 4 / 16 per unit: the first two rays stop at 10.5, where (2 + 1.5) / (0.25 * 10.5 + 0.33) > 1; the third
    # samples last at 14, where the quotient is 3.5 / 3.83.  The mean, 0.971, is above UNSHADOWED_THRESHOLD; 10 of 64 steps were used
    assert facts["visibilities"] == [1, 1, F(F(3.5) / lc.fmaf(F(0.25), F(14), F(0.33)))]
    assert facts["steps_remaining"] == 54 and cone == 1


def test_offset_floor_and_saturation():
    dfu = trace_uniforms()
    long_segment = lc.prepare(lc.line_light((0.0, 0.0, 10.0), (1000.0, 0.0, 10.0), 2.0), dfu)
    assert long_segment.offset == F(0.03)                                    # (2 + 1) / 1000 < 0.03
    short_segment = lc.prepare(lc.line_light((20.0, 10.0, 10.0), (22.0, 10.0, 10.0), 2.0), dfu)
    assert short_segment.offset == 1                                         # (2 + 1) / 2 saturates
    middling = lc.prepare(lc.line_light((0.0, 0.0, 10.0), (30.0, 0.0, 10.0), 2.0), dfu)
    assert middling.offset == F(F(3) / F(30))
    # with o = 1 the outer rays aim at the segment's two ends whatever u is
    _, _, facts = lc.line_trace(EMPTY, (21.0, 14.0, 0.0), (0.0, 0.0, 1.0), short_segment, F(0.5), dfu, True)
    assert facts["along"] == [0, 0.5, 1]
    # createTraceConfig: maxRadius = clamp(radius, 0.33, MaxCone), growth = maxRadius / max(ramp length, 16)
    assert long_segment.max_radius == 2 and long_segment.growth == F(F(2) / F(16))
    wide = lc.prepare(lc.line_light((0.0, 0.0, 10.0), (30.0, 0.0, 10.0), 20.0, ramp_length=40.0), dfu)
    assert wide.max_radius == 8 and wide.growth == F(F(8) / F(40))
    thin = lc.prepare(lc.line_light((0.0, 0.0, 10.0), (30.0, 0.0, 10.0), 0.1), dfu)
    assert thin.max_radius == F(0.33)


def test_an_exhausted_step_budget_shadows_the_pixel():
    """three steps of 1.5 towards a light 60 away: stepsRemaining reaches 0 with every ray alive, visibility = min(1, 0 / 2) = 0"""
    dfu = trace_uniforms(step_limit=3)
    r = lc.prepare(lc.line_light((10.0, 10.0, 60.0), (50.0, 10.0, 60.0), 2.0), dfu)
    cone, samples, facts = lc.line_trace(lambda p: F(1.0), (30.0, 10.0, 0.0), (0.0, 0.0, 1.0), r, F(0.5), dfu, True)
    assert samples == 9 and facts["iterations"] == 3 and facts["steps_remaining"] == 0
    assert facts["ended"] == (None, None, None) and facts["visibilities"] == [1, 1, 1]
    assert facts["visibility"] == 0 and cone == 0
    # no field bound: no iteration, the budget untouched, cone opacity 1
    cone, samples, facts = lc.line_trace(EMPTY, (30.0, 10.0, 0.0), (0.0, 0.0, 1.0), r, F(0.5), dfu, False)
    assert samples == 0 and cone == 1 and facts["steps_remaining"] == 3


def test_an_unshadowed_pixel_has_cone_opacity_one_and_an_obstacle_lowers_one_ray():
    dfu = trace_uniforms()
    r = lc.prepare(lc.line_light((10.0, 10.0, 30.0), (50.0, 10.0, 30.0), 2.0), dfu)
    cone, samples, facts = lc.line_trace(EMPTY, (30.0, 10.0, 0.0), (0.0, 0.0, 1.0), r, F(0.5), dfu, True)
    assert cone == 1 and facts["visibilities"] == [1, 1, 1] and samples == 3       # one long step reaches every ray's end
    # an obstacle around the start-side ray only (it leans from x = 30 towards x = 27; the wall is x < 29.5 above z = 8): that ray's
    # visibility falls while the other two stay clear, and the mean of the three decides
    def wall(p):
        return F(-1.4) if (p[0] < 29.5 and p[2] > 8.0) else F(4.0)
    cone, samples, facts = lc.line_trace(wall, (30.0, 10.0, 0.0), (0.0, 0.0, 1.0), r, F(0.5), dfu, True)
    va, vb, vc = facts["visibilities"]
    assert va < 0.075 and vb == 1 and vc == 1
    want = (float(va) + 2.0) / 3.0
    assert abs(float(facts["visibility"]) - want) < 1e-6
    assert abs(float(cone) - ((want - 0.075) / 0.875) ** float(dfu.ConeAndMisc.z)) < 1e-5


def test_colour_is_interpolated_with_the_clamped_u(oracle):
    """pixels beyond the two ends take u = 0 and u = 1: exactly Color1 and Color2 (alpha included), times the opacity"""
    light = lc.line_light((20.0, 5.0, 6.0), (30.0, 5.0, 6.0), 2.0, start_color=(1.0, 0.5, 0.25, 0.5), end_color=(0.125, 0.75, 1.0, 1.0),
                          casts_shadows=False)
    w, h = 48, 8
    out = lc.render(oracle, [light], scenes.environment(), lc.no_field_uniforms(), None, None, (0.0, 0.0, 0.0, 1.0), w, h)
    left, right, mid = out.detail[(10, 5, 0)], out.detail[(40, 5, 0)], out.detail[(25, 6, 0)]
    assert left["u"] == 0 and right["u"] == 1 and mid["u"] == 0.5
    for x, facts, colour in ((10, left, (1.0, 0.5, 0.25, 0.5)), (40, right, (0.125, 0.75, 1.0, 1.0)), (25, mid, (0.5625, 0.625, 0.625, 0.75))):
        want = [F(F(F(colour[k]) * F(colour[3])) * facts["opacity"]) for k in range(3)]
        assert [out.image[5 if x != 25 else 6, x, k] for k in range(3)] == want and facts["opacity"] > 0
    assert (out.image[..., 3] == 2).all() and out.stats == (0, w * h, 0)


def test_fullbright_pixels_form_no_pair_and_invisible_ones_are_clipped():
    light = lc.prepare(lc.line_light((0.0, 0.0, 10.0), (30.0, 0.0, 10.0), 2.0), trace_uniforms())
    shaded, normal = (-10000.0, 3.0, 0.0), (0.0, 0.0, 1.0)
    assert lc.shade(EMPTY, (shaded, normal, True, False), light, F(0.25), F(0.0), trace_uniforms(), True) is None      # x <= -9999
    assert lc.shade(EMPTY, ((5.0, 3.0, 0.0), normal, True, False), light, F(0.0), F(0.2), trace_uniforms(), True) is None   # opacity 0
    lit = lc.shade(EMPTY, ((5.0, 3.0, 0.0), normal, False, False), light, F(0.25), F(0.2), trace_uniforms(), True)
    assert lit is not None and lit[1] == 0 and lit[2] is False                # shadows disabled on the pixel: casts * 0, no trace


def test_pack_line_light_matches_the_scene_packing():
    from illuminant_amd import _host as Host
    l = Host.LineLightSource()
    assert l.Radius == 0 and l.Opacity == 1 and l.CastsShadows and list(l.StartColor) == [1, 1, 1, 1]          # LightSource.cs:325,336
    l.StartPosition, l.EndPosition, l.Radius = [3.0, 4.0, 5.0], [30.0, 14.0, 9.0], 2.5
    l.StartColor, l.EndColor = [1.0, 0.5, 0.25, 0.9], [0.2, 0.4, 0.6, 0.7]
    l.Opacity, l.AmbientOcclusionRadius, l.AmbientOcclusionOpacity, l.FalloffYFactor, l.RampMode = 0.8, 5.0, 0.6, 1.5, 1
    for have_field in (True, False):
        got = Host.LightingRenderer.PackLineLightBytes(l, 1.3, have_field)
        want = scenes.line_light((3.0, 4.0, 5.0), (30.0, 14.0, 9.0), 2.5, start_color=(1.0, 0.5, 0.25, 0.9), end_color=(0.2, 0.4, 0.6, 0.7),
                                 opacity=0.8, intensity_scale=1.3, ramp_mode=1, have_distance_field=have_field, ao_radius=5.0, ao_opacity=0.6,
                                 falloff_y=1.5)
        assert got == bytes(want)
    l.ShadowDistanceFalloff = 3.0
    assert np.frombuffer(Host.LightingRenderer.PackLineLightBytes(l, 1.0, True), np.float32)[4 * 4 + 1] == 3.0
    l.Opacity = 0.0
    assert Host.LightingRenderer.PackLineLightBytes(l, 1.0, True) is None        # RenderLineLightSource's early return (:1311)
    l.SetColor([0.1, 0.2, 0.3, 0.4])
    assert list(l.StartColor) == list(l.EndColor) == [F(0.1), F(0.2), F(0.3), F(0.4)]
