"""Known answers of the directional-light restatement (tests/directional_common.py), derived by hand from DirectionalLight.fx:52-161,
LightCommon.fxh:154-165,224-231 and ConeTrace.fxh:37-191, and the host mirror's packing against LightingRenderer.cs:1256-1293.  No GPU.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import directional_common as dc

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def entry_point():
    """what the restatement restates must exist: the library exports the entry point and the binding knows it.  (Most cases below
    exercise the Python restatement alone -- they pin it, as the GPU tests are only as good as it is -- and it is this fixture that ties
    them to the feature: without the entry point none of them passes.)"""
    assert "ilm_render_directional_lights" in native.SYMBOLS
    assert hasattr(native.lib(), "ilm_render_directional_lights")
    assert hasattr(native, "render_directional_lights")


def vertex_floats(v):
    return np.frombuffer(bytes(v), np.float32).reshape(8, 4)


def one_pixel(normal=(0.0, 0.0, 1.0), shaded=(10.5, 10.5, 0.0), enable_shadows=True, fullbright=False):
    return (shaded, normal, enable_shadows, fullbright)


def test_header_binding_and_csharp_agree_on_the_symbol():
    text = open(os.path.join(ROOT, "include", "illuminant_hip.h")).read()
    decl = re.search(r"^int32_t ilm_render_directional_lights\(([^)]*)\)", text, flags=re.M).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in decl.split(",")] == [
        "IlmHandle", "const IlmLightVertex*", "int32_t", "const IlmEnvironment*", "const IlmDistanceFieldUniforms*", "IlmHandle", "IlmHandle",
        "const float", "IlmHandle", "int32_t", "int32_t", "IlmRenderStats*"]
    assert len(native.SYMBOLS["ilm_render_directional_lights"][1]) == 12
    assert native.SYMBOLS["ilm_render_directional_lights"] == native.SYMBOLS["ilm_render_sphere_lights"]
    cs = open(os.path.join(ROOT, "integration", "IlluminantHip.cs")).read()
    assert "ilm_render_directional_lights (ulong ctx, LightVertex* lights, int lightCount" in cs
    # the ramp entry point's comment names the call it now also serves
    ramp_comment = text[text.index("/* LightSource.TextureRef / Configuration.DefaultRampTexture"):text.index("int32_t ilm_ctx_set_light_ramp")]
    assert "ilm_render_directional_lights" in ramp_comment


def test_handles_are_validated_without_a_device():
    lib = native.lib()
    env, dfu = scenes.environment(), dc.no_field_uniforms()
    assert lib.ilm_render_directional_lights(abi.Handle(0), None, 0, C.byref(env), C.byref(dfu), abi.Handle(0), abi.Handle(0), None, abi.Handle(0), 0, 0,
                                             None) == abi.ERR_INVALID_HANDLE
    assert b"context" in lib.ilm_last_error()
    assert lib.ilm_render_directional_lights(abi.Handle(123456789), None, 0, C.byref(env), C.byref(dfu), abi.Handle(0), abi.Handle(0), None,
                                             abi.Handle(0), 0, 0, None) == abi.ERR_INVALID_HANDLE


def test_null_direction_without_shadows_is_ambient_plus_colour(oracle):
    """Color2 = 0: computeDirectionalLightOpacity is 1, nothing is traced; ground plane, no AO: every covered pixel is exactly
    ambient + rgb * a, alpha + 1."""
    w, h = 12, 9
    light = dc.directional_light(direction=None, bounds=(2.0, 1.0, 9.0, 6.0), color=(0.5, 0.25, 0.125, 0.5), casts_shadows=False)
    ambient = (0.0625, 0.125, 0.25, 1.0)
    out = dc.render(oracle, [light], scenes.environment(), dc.no_field_uniforms(), None, None, ambient, w, h)
    want = np.zeros((h, w, 4), np.float32)
    want[:] = ambient
    want[1:6, 2:9] = (0.0625 + 0.25, 0.125 + 0.125, 0.25 + 0.0625, 2.0)
    assert np.array_equal(out.image, want)
    assert out.stats == (0, 5 * 7, 0)


def test_normal_factor_of_a_flat_normal():
    flat = (0.0, 0.0, 1.0)
    assert dc.normal_factor((0.0, 0.0, -1.0), flat) == 1                      # light straight down: d = 1
    assert dc.normal_factor((1.0, 0.0, 0.0), flat) == 1                       # horizontal: d = 0, (0 + 0.35) / 0.35 = 1
    # dot(-direction, n) = -0.175: (0.175 / 0.35) ^ 0.85 = 0.5 ^ 0.85
    up = 0.175
    got = dc.normal_factor((float(np.sqrt(1 - up * up)), 0.0, up), flat)
    assert abs(float(got) - 0.5 ** 0.85) < 1e-6
    assert dc.normal_factor((float(np.sqrt(1 - 0.35 ** 2)), 0.0, 0.35), flat) == 0      # dot = -0.35
    assert dc.normal_factor((0.0, 0.0, 1.0), flat) == 0                       # from below: dot = -1
    assert dc.normal_factor((0.0, 0.0, 1.0), (0.0, 0.0, 0.0)) == 1            # a zero normal disables the factor


def test_a_pixel_lit_from_below_adds_alpha_but_no_colour(oracle):
    """no opacity discard in DirectionalLightPixelShader: opacity 0 still blends (0, 0, 0, 1)"""
    light = dc.directional_light(direction=(0.0, 0.0, 1.0), color=(1, 1, 1, 1), casts_shadows=False)
    out = dc.render(oracle, [light], scenes.environment(), dc.no_field_uniforms(), None, None, (0.1, 0.2, 0.3, 1.0), 3, 2)
    assert np.array_equal(out.image, np.broadcast_to(np.asarray((0.1, 0.2, 0.3, 2.0), np.float32), (2, 3, 4)))


def trace_light(length=32.5, softness=1.0, **kw):
    return dc.directional_light(direction=(0.0, 0.0, -1.0), shadow_trace_length=length, shadow_softness=softness, **kw)


def test_an_empty_field_gives_cone_opacity_one():
    """every sample far from any obstacle: visibility stays 1 and the budget is not touched (one step of 0.75 x 100 crosses the trace)"""
    dfu = dc.field_uniforms(step_limit=8)
    opacity, n, traced, facts = dc.shade(lambda p: 100.0, one_pixel(), trace_light(), dfu, True)
    assert (opacity, n, traced) == (1, 1, True)
    assert facts["steps_remaining"] == 7 and facts["visibility"] == 1
    # the trace runs from shaded + 1.5 normal towards shaded - direction * length: straight up, length 32.5 - 1.5
    assert facts["start"] == [F(10.5), F(10.5), F(1.5)] and facts["ray"] == [0, 0, 1] and facts["length"] == 31


def test_a_ray_that_enters_a_box_within_a_few_pixels_is_fully_shadowed(oracle):
    """the tests' field: a box x 10..20, y 8..16, z 0..24.  A ground pixel at x = 22.5 lit from the left (the ray towards the fake
    centre runs left and up into the box's face at x = 20): visibility falls below FULLY_SHADOWED_THRESHOLD, opacity 0."""
    dfu = dc.field_uniforms()
    tex = oracle.make_texture(dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    light = dc.directional_light(direction=(1.0, 0.0, -0.5), shadow_trace_length=24.0, shadow_softness=2.0)
    sample = lambda p: oracle.sample_distance_field(p, dfu, tex)
    opacity, n, traced, facts = dc.shade(sample, one_pixel(shaded=(22.5, 12.5, 0.0)), light, dfu, True)
    assert traced and opacity == 0 and facts["visibility"] <= dc.FULLY_SHADOWED_THRESHOLD
    assert 1 <= n <= 4 and facts["position"] < 8
    # the same light on a pixel on the far side of the box's reach sees nothing within its trace
    opacity, n, traced, facts = dc.shade(sample, one_pixel(shaded=(4.5, 28.5, 0.0)), light, dfu, True)
    assert traced and opacity == 1


@pytest.mark.parametrize("budget,remaining,visibility", [(5, 2, 1.0), (4, 1, 0.5), (3, 0, 0.0)])
def test_an_exhausted_step_budget_ramps_visibility_down(budget, remaining, visibility):
    """distance 10 everywhere, LongStepFactor 1: x = 0.5, 10.5, 20.5, 30.5 >= length - softness = 30: three steps.  What is left of the
    budget, over MAX_STEP_RAMP_WINDOW = 2, caps the visibility (ConeTrace.fxh:175-180)."""
    dfu = dc.field_uniforms(step_limit=budget, long_step_factor=1.0, power_=1.0)
    opacity, n, traced, facts = dc.shade(lambda p: 10.0, one_pixel(), trace_light(), dfu, True)
    assert n == 3 and facts["steps_remaining"] == remaining and facts["position"] == 30.5
    want = min(max((F(visibility) - dc.FULLY_SHADOWED_THRESHOLD), 0) / dc.VISIBILITY_RANGE, 1.0)
    assert abs(float(opacity) - float(want)) < 1e-6
    if remaining == 1:
        assert abs(float(opacity) - 0.425 / 0.875) < 1e-6


def test_the_trace_gates():
    dfu = dc.field_uniforms()
    near = lambda p: -5.0          # inside an obstacle everywhere: any trace gives 0
    assert dc.shade(near, one_pixel(), trace_light(), dfu, True)[0] == 0
    assert dc.shade(near, one_pixel(), trace_light(casts_shadows=False), dfu, True)[0] == 1
    assert dc.shade(near, one_pixel(enable_shadows=False), trace_light(), dfu, True)[0] == 1        # lightProperties.x *= enableShadows
    null = dc.directional_light(direction=None)
    assert dc.shade(near, one_pixel(), null, dfu, True)[:3] == (1, 0, False)                        # lightDirection.w < 0.1
    # no bound field: traceShadows holds but the loop does not run; not counted as traced
    assert dc.shade(near, one_pixel(), trace_light(), dfu, False)[:3] == (1, 0, False)
    # discards: fullbright, the shadow filter (0 = NoShadowsOnly, 1 = ShadowsOnly), a pixel that is not visible
    assert dc.shade(near, one_pixel(fullbright=True), null, dfu, True) is None
    assert dc.shade(near, one_pixel(), dc.directional_light(shadow_filter=0), dfu, True) is None
    assert dc.shade(near, one_pixel(enable_shadows=False), dc.directional_light(shadow_filter=0), dfu, True) is not None
    assert dc.shade(near, one_pixel(enable_shadows=False), dc.directional_light(shadow_filter=1), dfu, True) is None
    assert dc.shade(near, one_pixel(shaded=(-9999.0, 3.0, 0.0)), null, dfu, True) is None
    assert dc.shade(near, one_pixel(shaded=(-9998.5, 3.0, 0.0)), null, dfu, True) is not None


def test_ambient_occlusion_is_scaled_by_the_normal_and_sampled_above_the_point():
    dfu = dc.field_uniforms()
    seen = []

    def sample(p):
        seen.append([float(c) for c in p])
        return 2.0
    light = dc.directional_light(direction=None, ao_radius=8.0, ao_opacity=0.5, casts_shadows=False)
    opacity, n, traced, _ = dc.shade(sample, one_pixel(normal=(0.0, 0.6, 0.5)), light, dfu, True)
    # radius 8 * 0.5 = 4, sampled at z + 0.5 * 4; result = 1 - (1 - 2 / 4)^2 = 0.75; opacity = (1 - 0.5) + 0.75 * 0.5
    assert seen == [[10.5, 10.5, 2.0]] and (n, traced) == (1, False)
    assert opacity == F(0.875)
    assert dc.shade(sample, one_pixel(normal=(0.0, 0.0, -1.0)), light, dfu, True)[:2] == (1, 0)       # downward-facing: radius 0
    assert dc.shade(sample, one_pixel(), light, dfu, False)[:2] == (1, 0)                             # no field


def covered_mask(oracle, light, env, w=14, h=12):
    out = dc.render(oracle, [light], env, dc.no_field_uniforms(), None, None, (0, 0, 0, 0), w, h)
    return out.image[..., 3] == 1


def test_coverage_is_the_pixel_centre_in_a_half_open_rectangle(oracle):
    light = lambda b: dc.directional_light(direction=None, bounds=b, casts_shadows=False)
    # fractional edges: centres 3.5 .. 9.5 lie in [3.25, 10.5) -- 10.5 itself does not -- and 2.5 .. 7.5 in [2.5, 7.75)
    mask = covered_mask(oracle, light((3.25, 2.5, 10.5, 7.75)), scenes.environment())
    want = np.zeros_like(mask)
    want[2:8, 3:10] = True
    assert np.array_equal(mask, want)
    # edges exactly on pixel centres: the top-left rule -- the left / top centre is in, the right / bottom one is out
    mask = covered_mask(oracle, light((4.5, 3.5, 8.5, 6.5)), scenes.environment())
    want[:] = False
    want[3:6, 4:8] = True
    assert np.array_equal(mask, want)
    # a viewport: (12 - 10) * (2 * 0.75) = 3 .. (16 - 10) * 1.5 = 9 in x; (23 - 20) * (0.5 * 4) = 6 .. (25.5 - 20) * 2 = 11 in y
    env = scenes.environment(viewport_position=(10.0, 20.0), viewport_scale=(2.0, 0.5), render_scale=(0.75, 4.0))
    mask = covered_mask(oracle, light((12.0, 23.0, 16.0, 25.5)), env)
    want[:] = False
    want[6:11, 3:9] = True
    assert np.array_equal(mask, want)
    # no bounds: -99999 .. 99999 covers every pixel
    assert covered_mask(oracle, dc.directional_light(direction=None, casts_shadows=False), scenes.environment()).all()


def test_blend_models_and_stores(oracle):
    """two overlapping lights: fp32 registers in list order added to the base and rounded once at the store, against the fp16-per-light
    chain dst = half(dst + half(src)); the three formats' stores"""
    a = dc.directional_light(direction=None, color=(0.3337, 0.1113, 0.7771, 1.0), casts_shadows=False)
    b = dc.directional_light(direction=None, color=(0.0123, 0.4567, 0.0891, 0.9), casts_shadows=False)
    amb = (0.0213, 0.0377, 0.0591, 1.0)
    env, dfu = scenes.environment(), dc.no_field_uniforms()
    fp32 = dc.render(oracle, [a, b], env, dfu, None, None, amb, 2, 1).image[0, 0]
    ca = [F(F(c) * F(1.0)) for c in (0.3337, 0.1113, 0.7771)]
    cb = [F(F(c) * F(0.9)) for c in (0.0123, 0.4567, 0.0891)]
    assert [float(x) for x in fp32] == [float(F(F(amb[k]) + F(F(F(0) + ca[k]) + cb[k]))) for k in range(3)] + [3.0]
    fp16 = dc.render(oracle, [a, b], env, dfu, None, None, amb, 2, 1, blend_fp16=True).image[0, 0]
    h = dc.half
    assert [float(x) for x in fp16] == [float(h(F(h(F(h(F(amb[k])) + h(ca[k]))) + h(cb[k])))) for k in range(3)] + [3.0]
    assert np.array_equal(fp16, dc.half(fp16)) and not np.array_equal(fp16, fp32)
    image = np.asarray([[[0.5, 1.5, -0.25, 0.0019607844]]], np.float32)
    assert np.array_equal(dc.to_stored(image, abi.LIGHTMAP_RGBA8), [[[128, 255, 0, 0]]])           # rint: 127.5 -> 128 (half to even), 0.49999 -> 0
    assert dc.to_stored(image, abi.LIGHTMAP_HALF4).dtype == np.float16
    assert np.array_equal(dc.from_stored(np.asarray([[[255, 51, 0, 128]]], np.uint8), abi.LIGHTMAP_RGBA8),
                          (np.asarray([[[255, 51, 0, 128]]], np.float32) / F(255)))
    # accumulate: rows outside the strip keep what they held, rows inside add to it
    before = scenes.uniform(3, (4, 2, 4), 0.0, 1.0)
    out = dc.render(oracle, [a], env, dfu, None, None, None, 2, 4, row_begin=1, row_end=3, before=before).image
    assert np.array_equal(out[0], before[0]) and np.array_equal(out[3], before[3])
    assert np.array_equal(out[1, 0], [F(before[1, 0, k] + F(F(0) + ca[k])) for k in range(3)] + [F(before[1, 0, 3] + F(1))])


def test_with_a_ramp_the_opacity_goes_through_the_lookup(oracle):
    ramp = dc.ramp_texture()
    light = dc.directional_light(direction=(0.6, 0.0, 0.12), color=(1, 1, 1, 1), casts_shadows=False)      # from below the horizon: partial factor
    plain = dc.render(oracle, [light], scenes.environment(), dc.no_field_uniforms(), None, None, (0, 0, 0, 0), 1, 1).image[0, 0]
    assert 0.05 < plain[0] < 0.95
    ramped = dc.render(oracle, [light], scenes.environment(), dc.no_field_uniforms(), None, None, (0, 0, 0, 0), 1, 1, ramp=ramp).image[0, 0]
    assert ramped[0] == oracle.table_lookup(1, ramp, float(plain[0]), 0.0)[0] and ramped[0] != plain[0]
    # v = 0 lies between the last and the first row (V WRAP, LINEAR): the mean of the two rows' values at that u
    one_row = np.repeat(ramp[:1], 2, axis=0)
    u = float(plain[0])
    assert abs(float(oracle.table_lookup(1, ramp, u, 0.0)[0]) -
               0.5 * (float(oracle.table_lookup(1, one_row, u, 0.0)[0]) + float(oracle.table_lookup(1, np.repeat(ramp[1:], 2, axis=0), u, 0.0)[0]))) < 1e-6
    # a 1 x 1 ramp is no ramp
    tiny = np.ones((1, 1, 4), np.float32)
    assert dc.render(oracle, [light], scenes.environment(), dc.no_field_uniforms(), None, None, (0, 0, 0, 0), 1, 1, ramp=tiny).image[0, 0, 0] == plain[0]


def test_pack_directional_light_fills_the_reference_layout():
    """RenderDirectionalLightSource, LightingRenderer.cs:1256-1293, field by field; the restatement's builder packs the same bytes."""
    from illuminant_amd import _host as H
    d = H.DirectionalLightSource()
    assert (d.ShadowTraceLength, d.ShadowSoftness, d.ShadowRampRate) == (256.0, 12.0, 0.5)       # LightSource.cs:136-144
    assert d.Direction is None and d.Bounds is None and d.CastsShadows and d.Enabled and d.ShadowFilter == -1
    d.Color = [0.5, 0.25, 1.0, 0.8]
    d.Opacity = 0.5
    v = np.frombuffer(H.LightingRenderer.PackDirectionalLightBytes(d, 2.0), np.float32).reshape(8, 4)
    assert np.array_equal(v[0], [-99999, -99999, 0, 0]) and np.array_equal(v[1], [99999, 99999, 0, 0]) and not v[2].any()
    assert np.array_equal(v[3], [1, 256, 12, 0.5])                                   # castsShadows (no field test, :1279), trace length, softness, ramp rate
    assert np.array_equal(v[4], [0, -99999, 0, 1])                                   # aoRadius, shadowDistanceFalloff or -99999, 0, aoOpacity
    assert v[5, 0] == -1
    assert np.array_equal(v[6], [F(0.5), F(0.25), F(1.0), F(0.8) * (F(0.5) * F(2.0))])
    assert not v[7].any()                                                            # null direction: Color2 = 0
    # a direction is normalised when set (1 / sqrt, then three products); bounds; the optional members
    d.Direction = [3.0, 0.0, -4.0]
    factor = F(F(1) / F(np.sqrt(F(25))))
    assert d.Direction == [float(F(3) * factor), 0.0, float(F(-4) * factor)]
    d.Bounds = [1.5, 2.5, 30.0, 20.25]
    d.CastsShadows = False
    d.ShadowDistanceFalloff = 40.0
    d.AmbientOcclusionRadius, d.AmbientOcclusionOpacity, d.ShadowFilter = 6.0, 0.75, 1
    d.ShadowTraceLength, d.ShadowSoftness, d.ShadowRampRate = 64.0, 3.0, 0.25
    v = np.frombuffer(H.LightingRenderer.PackDirectionalLightBytes(d, 1.0), np.float32).reshape(8, 4)
    assert np.array_equal(v[0], [1.5, 2.5, 0, 0]) and np.array_equal(v[1], [30.0, 20.25, 0, 0])
    assert np.array_equal(v[3], [0, 64, 3, 0.25]) and np.array_equal(v[4], [6, 40, 0, 0.75]) and v[5, 0] == 1
    assert np.array_equal(v[7], [F(3) * factor, 0, F(-4) * factor, 1])
    mine = dc.directional_light(direction=(3.0, 0.0, -4.0), bounds=(1.5, 2.5, 30.0, 20.25), color=(0.5, 0.25, 1.0, 0.8), opacity=0.5,
                                casts_shadows=False, shadow_trace_length=64.0, shadow_softness=3.0, shadow_ramp_rate=0.25, ao_radius=6.0,
                                ao_opacity=0.75, shadow_distance_falloff=40.0, shadow_filter=1)
    assert np.array_equal(vertex_floats(mine), v)
    # Opacity <= 0: not drawn (:1258)
    d.Opacity = 0.0
    assert H.LightingRenderer.PackDirectionalLightBytes(d, 1.0) is None
    d.Direction = None
    assert d.Direction is None
    env = H.LightingEnvironment()
    env.DirectionalLights = [d, H.DirectionalLightSource()]
    assert len(env.DirectionalLights) == 2 and env.DirectionalLights[0].Opacity == 0.0
