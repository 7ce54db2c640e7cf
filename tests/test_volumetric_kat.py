"""Known answers of the volumetric-light restatement (tests/volumetric_common.py), derived by hand from VolumetricLightCore.fxh:25-54,85-88,
281-298,315-549 and LightingRenderer.cs:1339-1384; the packing; and the conditions of the GPU scenes (tests/volumetric_scenes.py) on the
restatement alone.  No GPU.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import volumetric_common as vc
from tests import volumetric_scenes as vs
from tests.util import assert_close

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = vc.WIDTH, vc.HEIGHT
SYMBOL = "ilm_render_volumetric_lights"


@pytest.fixture(autouse=True)
def entry_point():
    """what the restatement restates must exist: the library exports the entry point and the binding knows it.  (Most cases below
    exercise the Python restatement alone -- they pin it, as the GPU tests are only as good as it is -- and it is this fixture that ties
    them to the feature: without the entry point none of them passes.)"""
    assert SYMBOL in native.SYMBOLS
    assert hasattr(native.lib(), SYMBOL)
    assert hasattr(native, "render_volumetric_lights")


def test_header_binding_and_csharp_agree_on_the_symbol():
    text = open(os.path.join(ROOT, "include", "illuminant_hip.h")).read()
    decl = re.search(r"^int32_t %s\(([^)]*)\)" % SYMBOL, text, flags=re.M).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in decl.split(",")] == [
        "IlmHandle", "const IlmLightVertex*", "int32_t", "const IlmEnvironment*", "const IlmDistanceFieldUniforms*", "IlmHandle", "IlmHandle",
        "const float", "IlmHandle", "int32_t", "int32_t", "IlmRenderStats*"]
    assert native.SYMBOLS[SYMBOL] == native.SYMBOLS["ilm_render_directional_lights"]
    cs = open(os.path.join(ROOT, "integration", "IlluminantHip.cs")).read()
    assert SYMBOL + " (ulong ctx, LightVertex* lights, int lightCount" in cs
    assert re.search(r"#define ILM_ABI_VERSION 11\b", text)


def test_handles_are_validated_without_a_device():
    lib = native.lib()
    env, dfu = scenes.environment(), vc.no_field_uniforms()
    fn = getattr(lib, SYMBOL)
    assert fn(abi.Handle(0), None, 0, C.byref(env), C.byref(dfu), abi.Handle(0), abi.Handle(0), None, abi.Handle(0), 0, 0, None) == abi.ERR_INVALID_HANDLE
    assert b"context" in lib.ilm_last_error()
    assert fn(abi.Handle(123456789), None, 0, C.byref(env), C.byref(dfu), abi.Handle(0), abi.Handle(0), None, abi.Handle(0), 0, 0,
              None) == abi.ERR_INVALID_HANDLE


def test_the_device_code_holds_the_restatements_constants():
    text = open(os.path.join(ROOT, "illuminant_amd", "csrc", "lighting.hip")).read()
    for name, value in (("kVolumetricDitherScale", vc.DITHER_SCALE), ("kVolumetricStepScale", vc.STEP_SCALE), ("kVolumetricHit", vc.HIT),
                        ("kVolumetricProjectThreshold", vc.PROJECT_THRESHOLD), ("kVolumetricConeDot", vc.CONE_DOT),
                        ("kVolumetricBoxFloor", vc.BOX_FLOOR)):
        m = re.search(r"constexpr float %s = (-?[0-9.]+)f;" % name, text)
        assert m and F(float(m.group(1))) == value, name
    assert int(re.search(r"constexpr int kVolumetricLoopGuard = (\d+);", text).group(1)) == vc.LOOP_GUARD
    assert "((float)((2 * px + 7 * py + 11) % 17) + 0.5f) / 17.0f" in text


# ---- Dither17 -----------------------------------------------------------------------------------------------------------------------

def test_dither17_over_a_block():
    values = np.array([[vc.dither17(x, y) for x in range(17)] for y in range(17)], np.float32)
    multiples = np.array([F(F(m + 0.5) / F(17)) for m in range(17)], np.float32)
    assert set(values.ravel().tolist()) == set(multiples.tolist()), "every value is a residue + 0.5 over 17, rounded once"
    for m in multiples:
        assert (values == m).sum() == 17, "each of the 17 residues occurs 17 times"
    for row in values:
        assert len(set(row.tolist())) == 17
    assert vc.dither17(0, 0) == F(F(11.5) / F(17))
    assert vc.dither17(3, 5) == F(F((6 + 35 + 11) % 17 + 0.5) / F(17))
    # far from the origin the sum is still exact in fp32
    assert vc.dither17(100000, 70000) == F(F((200000 + 490000 + 11) % 17 + 0.5) / F(17))
    # and it is the published function at frame 0.5, up to the rounding that function leaves open
    for x, y in ((0, 0), (5, 9), (43, 26)):
        assert abs(float(vc.dither17(x, y)) - math.fmod((2 * x + 7 * y + 23 * 0.5) / 17.0, 1.0)) < 1e-6


# ---- the three distance functions ----------------------------------------------------------------------------------------------------

def test_sd_box_inside_on_a_face_and_past_a_corner():
    b = [F(2), F(2), F(2)]
    floor = float(vc.BOX_FLOOR)
    inside = vc.sd_box([F(1), F(0.5), F(0.25)], b)              # d = (-1, -1.5, -1.75): |(floor, floor, floor)| + max(d)
    assert abs(float(inside) - (math.sqrt(3) * floor - 1.0)) < 1e-6
    face = vc.sd_box([F(2), F(0), F(0)], b)                     # d = (0, -2, -2): |(floor, floor, floor)| + min(0, floor)
    assert abs(float(face) - math.sqrt(3) * floor) < 1e-9
    corner = vc.sd_box([F(5), F(-6), F(14)], b)                 # d = (3, 4, 12): 13 + floor
    assert abs(float(corner) - (13.0 + floor)) < 2e-6
    assert corner.dtype == np.float32


@pytest.mark.parametrize("point,branch,distance", [((5.0, 3.0, 4.0), 0, 5.0), ((14.0, 3.0, 0.0), 2, 5.0), ((-4.0, 0.0, 3.0), 1, 5.0)])
def test_sd_round_cone_as_a_capsule(point, branch, distance):
    """r1 == r2: the distance to the segment minus the radius, from the side and from beyond either cap"""
    taken = []
    got = vc.sd_round_cone([F(c) for c in point], [F(0)] * 3, [F(10), F(0), F(0)], F(1.5), F(1.5), taken)
    assert taken == [branch]
    assert abs(float(got) - (distance - 1.5)) < 1e-5


def test_sd_round_cone_with_two_radii():
    """on the axis beyond the caps the distance is that to the cap's sphere; at the side, that to the tangent line of the two circles"""
    a, b, r1, r2 = [F(0)] * 3, [F(10), F(0), F(0)], F(1), F(3)
    taken = []
    assert abs(float(vc.sd_round_cone([F(-5), F(0), F(0)], a, b, r1, r2, taken)) - 4.0) < 1e-5
    assert abs(float(vc.sd_round_cone([F(16), F(0), F(0)], a, b, r1, r2, taken)) - 3.0) < 1e-5
    # the side: with s = (r2 - r1) / |ba| the profile is the common tangent of the two circles, whose outward normal in the plane is
    # (-s, sqrt(1 - s^2)) and which lies r1 from the start: the distance of (x, h) is (h * sqrt(1 - s^2) - x * s) - r1
    s = 0.2
    side = vc.sd_round_cone([F(5), F(6), F(0)], a, b, r1, r2, taken)
    assert abs(float(side) - (6 * math.sqrt(1 - s * s) - 5 * s - 1.0)) < 1e-5
    assert taken == [1, 2, 0]


def test_sd_ellipsoid_of_a_sphere_and_its_degenerate_points():
    r = [F(4)] * 3
    assert abs(float(vc.sd_ellipsoid([F(0), F(0), F(7)], r)) - 3.0) < 1e-6
    assert abs(float(vc.sd_ellipsoid([F(1), F(2), F(2)], r)) + 1.0) < 1e-6
    assert np.isnan(vc.sd_ellipsoid([F(0)] * 3, r)), "0 * -1 / 0 at the centre"
    flat = vc.sd_ellipsoid([F(1), F(1), F(1)], [F(0), F(4), F(4)])
    assert np.isnan(flat) or np.isinf(flat), "a zero radius component"


def test_a_sphere_above_a_ground_plane_pixel_sums_to_the_closed_form(oracle):
    """an ellipsoid with three equal radii R centred above pixel (20, 10) of the ground plane, no field, RampPower 1: sd = |z - cz| - R,
    and the column is a finite sum written here in double"""
    R, cz, ramp_length, volumetricity = 6.0, 9.0, 2.5, 1.75
    light = vc.volumetric_light(shape=vc.ELLIPSOID, start=(20.0 - R, 10.0 - R, cz - R), end=(20.0 + R, 10.0 + R, cz + R), ramp_length=ramp_length,
                                volumetricity=volumetricity, color=(1.0, 0.5, 0.25, 0.8))
    env, dfu = scenes.environment(), vc.no_field_uniforms()
    want = vc.render(oracle, [light], env, dfu, None, None, (0, 0, 0, 0), W, H)
    facts = want.detail[(20, 10, 0)]
    steps = vc.MAX_STEP_COUNT
    z2, z1 = max(0.0, cz - R), min(128.0, cz + R)
    step = max(abs(z2 - z1), 1.0) / steps
    dither = ((2 * 20 + 7 * 10 + 11) % 17 + 0.5) / 17.0
    z, hits, n = z1 + dither * step, 0.0, 0
    while True:
        hits += min(max(-(abs(z - cz) - R) / ramp_length, 0.0), 1.0)
        n += 1
        z -= step
        if not z >= z2:
            break
    opacity = min(max(hits / steps / volumetricity, 0.0), 1.0)
    assert facts["iterations"] == n == steps + 1
    assert facts["contact"] > 0 and facts["diffuse"] == 0 and facts["returned"] == "max"
    assert 0.1 < opacity < 0.9
    assert_close(np.array([facts["hits"], facts["opacity"]], np.float32), np.array([hits, opacity]), "column sum of a sphere")
    assert_close(want.image[10, 20], np.array([0.8 * opacity, 0.4 * opacity, 0.2 * opacity, 1.0]), "the texel of a sphere")
    # footprint: centre +- R, half-open on the pixel centres
    assert want.image[10, 14, 3] == 1 or (14, 10, 0) in want.detail
    assert (13, 10, 0) not in want.detail and (14, 10, 0) in want.detail and (25, 10, 0) in want.detail and (26, 10, 0) not in want.detail


# ---- coverage ----------------------------------------------------------------------------------------------------------------------

def test_coverage_rectangles_against_hand_values():
    env = scenes.environment(viewport_position=(2.0, -1.0), viewport_scale=(2.0, 0.5), render_scale=(0.5, 2.0))
    cone = vc.prepare(vc.volumetric_light(shape=vc.CONE, start=(30.0, 4.0, 9.0), end=(10.0, 12.0, 1.0), start_radius=2.0, end_radius=5.0), env)
    assert cone.world == (5.0, -1.0, 35.0, 17.0) and (cone.z_lo, cone.z_hi) == (-4.0, 14.0)
    assert cone.footprint == (3.0, 0.0, 33.0, 18.0)                   # (world - viewport) * (scale * render scale), both products 1
    for shape in (vc.ELLIPSOID, vc.BOX):
        r = vc.prepare(vc.volumetric_light(shape=shape, start=(30.0, 4.0, 9.0), end=(10.0, 12.0, 1.0), start_radius=2.0, end_radius=5.0), env)
        assert r.start == [20.0, 8.0, 5.0] and r.end == [10.0, 4.0, 4.0]
        assert r.world == (10.0, 4.0, 30.0, 12.0) and (r.z_lo, r.z_hi) == (1.0, 9.0), "the radii are not part of these shapes' bounds"
        assert r.footprint == (8.0, 5.0, 28.0, 13.0)
        assert r.md == F(np.sqrt(F(132.0)))
    env = scenes.environment(viewport_scale=(2.0, 1.0), render_scale=(1.5, 1.0))
    r = vc.prepare(vc.volumetric_light(shape=vc.BOX, start=(1.0, 1.0, 0.0), end=(3.0, 2.0, 1.0)), env)
    assert r.footprint == (3.0, 1.0, 9.0, 2.0)
    assert vc.covers(r.footprint, 3, 1) and vc.covers(r.footprint, 8, 1) and not vc.covers(r.footprint, 2, 1) and not vc.covers(r.footprint, 9, 1)
    assert not vc.covers(r.footprint, 5, 0) and not vc.covers(r.footprint, 5, 2)
    nan = vc.prepare(vc.volumetric_light(shape=vc.BOX, start=(float("nan"), 1.0, 0.0), end=(3.0, 2.0, 1.0)), env)
    assert not any(vc.covers(nan.footprint, x, 1) for x in range(12)), "a rectangle with a NaN covers nothing"


# ---- the core's two returns ---------------------------------------------------------------------------------------------------------

def test_both_return_branches_of_the_core():
    """a sphere around the shaded point whose centre lies below it: the surface faces away, normalOpacity = 0, and blowout turns it into
    lerp(0, -1, blowout) = -blowout -- a negative diffuse term that is added to the volume's opacity; without blowout the same pixel takes
    the maximum of the two"""
    env, dfu = scenes.environment(), vc.no_field_uniforms()
    pixel = ((20.0, 10.0, 0.0), (0.0, 0.0, 1.0), True, False)
    results = {}
    for blowout in (0.0, 0.5):
        light = vc.volumetric_light(shape=vc.ELLIPSOID, start=(12.0, 2.0, -11.0), end=(28.0, 18.0, 5.0), ramp_length=4.0, blowout=blowout,
                                    volumetricity=0.5, distance_attenuation=1.0)
        r = vc.prepare(light, env)
        results[blowout] = vc.shade(None, pixel, 20, 10, r, env, dfu, False)
    opacity, samples, traced, facts = results[0.0]
    assert facts["returned"] == "max" and facts["normal_opacity"] == 0 and facts["diffuse"] == 0 and opacity == facts["pre_trace"] > 0
    assert samples == 0 and traced is False
    opacity, _samples, _traced, facts = results[0.5]
    # |p - centre| = 3 inside a sphere of radius 8: contact = -5, shapeOpacity = saturate(5 / 4) = 1; the three radii give fullLength =
    # sqrt(192), distanceOpacity = 1 - 3 / sqrt(192)
    assert facts["returned"] == "sum" and facts["normal_opacity"] == F(-0.5) and facts["shape_opacity"] == 1
    assert abs(float(facts["contact"]) + 5.0) < 1e-5
    diffuse = -0.5 * (1.0 - 3.0 / math.sqrt(192.0))
    assert abs(float(facts["diffuse"]) - diffuse) < 1e-6
    assert opacity == F(facts["pre_trace"] + facts["diffuse"]) and opacity < results[0.0][0]
    # a zero normal: the factor is 1 whatever the direction
    r = vc.prepare(vc.volumetric_light(shape=vc.ELLIPSOID, start=(12.0, 2.0, -11.0), end=(28.0, 18.0, 5.0), ramp_length=4.0), env)
    flat = vc.shade(None, ((20.0, 10.0, 0.0), (0.0, 0.0, 0.0), True, False), 20, 10, r, env, dfu, False)
    assert flat[3]["normal_opacity"] == 1 and flat[3]["returned"] == "max" and flat[3]["diffuse"] > flat[3]["pre_trace"]


def test_discards_and_the_trace_test():
    env = scenes.environment()
    r = vc.prepare(vs.box(casts_shadows=True), env)
    normal = (0.0, 0.0, 1.0)
    assert vc.shade(None, ((5.0, 20.0, 1.0), normal, True, True), 5, 20, r, env, vc.no_field_uniforms(), False) is None, "fullbright"
    assert vc.shade(None, ((-9999.0, 20.0, 1.0), normal, True, False), 5, 20, r, env, vc.no_field_uniforms(), False) is None, "not visible"
    lit = vc.shade(None, ((5.0, 20.0, 1.0), normal, True, False), 5, 20, r, env, vc.no_field_uniforms(), False)
    assert lit[0] > 0 and lit[3]["trace_shadows"] is True and lit[2] is False, "traceShadows without a bound field: no march, not counted"
    off = vc.shade(None, ((5.0, 20.0, 1.0), normal, False, False), 5, 20, r, env, vc.no_field_uniforms(), False)
    assert off[3]["trace_shadows"] is False, "w * enableShadows"
    flat = vc.no_field_uniforms()
    flat.Extent = abi.f4(48, 32, 0, 128)
    assert vc.shade(None, ((5.0, 20.0, 1.0), normal, True, False), 5, 20, r, env, flat, True)[3]["trace_shadows"] is False, "Extent.z, not .x"
    outside = vc.shade(None, ((40.0, 3.0, 1.0), normal, True, False), 40, 3, r, env, vc.no_field_uniforms(), False)
    assert outside[0] is None and outside[3]["discarded"] and outside[3]["opacity"] == 0, "opacity <= 0"


# ---- the packing --------------------------------------------------------------------------------------------------------------------

def f4(v):
    return (v.x, v.y, v.z, v.w)


@pytest.mark.parametrize("shape", [vc.ELLIPSOID, vc.CONE, vc.BOX])
def test_packing_field_by_field(shape):
    """RenderVolumetricLightSource, LightingRenderer.cs:1339-1384"""
    kw = dict(shape=shape, start=(30.0, 4.5, 9.0), end=(10.0, 12.0, 1.25), start_radius=2.0, end_radius=5.0, direction=(0.25, 0.5, -0.75),
              color=(0.5, 0.25, 0.125, 0.75), opacity=0.5, volumetricity=1.5, ramp_length=3.0, ramp_power=2.0, blowout=0.125, distance_attenuation=0.75,
              ramp_mode=1, ao_radius=6.0, ao_opacity=0.25, shadow_distance_falloff=7.0, falloff_y=1.5, intensity_scale=2)
    for casts, have_field in ((True, True), (True, False), (False, True)):
        v = scenes.volumetric_light(casts_shadows=casts, have_field=have_field, **kw)
        if shape == vc.CONE:
            assert f4(v.LightPosition1) == (30.0, 4.5, 9.0, 2.0) and f4(v.LightPosition2) == (10.0, 12.0, 1.25, 5.0)
        else:       # (end - start).Abs() * 0.5 and (start + end) * 0.5
            assert f4(v.LightPosition1) == (20.0, 8.25, 5.125, 2.0) and f4(v.LightPosition2) == (10.0, 3.75, 3.875, 5.0)
        assert f4(v.LightPosition3) == (0.25, 0.5, -0.75, 0.0)
        assert f4(v.Color1) == (0.5, 0.25, 0.125, 0.75) and f4(v.Color2) == f4(v.Color1)        # 0.75 * (0.5 * 2)
        assert f4(v.LightProperties) == (1.5, 3.0, 1.0, 1.0 if (casts and have_field) else 0.0)
        assert f4(v.MoreLightProperties) == (6.0, 7.0, 1.5, 0.25)
        assert f4(v.EvenMoreLightProperties) == (0.125, 2.0, 0.75, float(shape))
    plain = scenes.volumetric_light(shape=shape, start=(0.0, 0.0, 0.0), end=(1.0, 1.0, 1.0))
    assert f4(plain.LightPosition3) == (0.0, 0.0, 0.0, 0.0) and plain.MoreLightProperties.y == -99999.0
    assert f4(plain.LightProperties) == (1.0, 1.0, 0.0, 1.0) and f4(plain.EvenMoreLightProperties) == (0.0, 1.0, 1.0, float(shape)), "the defaults"
    assert scenes.volumetric_light(opacity=0.0, **{k: x for k, x in kw.items() if k != "opacity"}) is None
    assert scenes.volumetric_light(opacity=-1.0, **{k: x for k, x in kw.items() if k != "opacity"}) is None


def test_an_unknown_shape_is_not_packed():
    assert scenes.volumetric_light(shape=3, end=(1.0, 1.0, 1.0)) is None


def test_the_host_mirror_packs_the_same_bytes():
    from illuminant_amd import _host as Host
    l = Host.VolumetricLightSource()
    assert (l.Shape, l.Volumetricity, l.DistanceAttenuation, l.RampLength, l.RampPower, l.BlowoutFactor) == (1, 1.0, 1.0, 1.0, 1.0, 0.0)
    for shape in (0, 1, 2):
        l = Host.VolumetricLightSource()
        l.Shape, l.StartPosition, l.EndPosition, l.StartRadius, l.EndRadius = shape, [30.0, 4.5, 9.0], [10.0, 12.0, 1.25], 2.0, 5.0
        l.LightDirection, l.Color, l.Opacity, l.BlowoutFactor, l.CastsShadows = [0.25, 0.5, -0.75], [0.5, 0.25, 0.125, 0.75], 0.3, 0.125, shape != 2
        want = scenes.volumetric_light(shape=shape, start=(30.0, 4.5, 9.0), end=(10.0, 12.0, 1.25), start_radius=2.0, end_radius=5.0,
                                       direction=(0.25, 0.5, -0.75), color=(0.5, 0.25, 0.125, 0.75), opacity=0.3, blowout=0.125,
                                       casts_shadows=shape != 2, intensity_scale=1.7)
        assert Host.LightingRenderer.PackVolumetricLightBytes(l, 1.7, True) == bytes(want)
    l.Shape = 5
    assert Host.LightingRenderer.PackVolumetricLightBytes(l, 1.0, True) is None
    l.Shape, l.Opacity = 1, 0.0
    assert Host.LightingRenderer.PackVolumetricLightBytes(l, 1.0, True) is None


# ---- the conditions of the GPU scenes, on the restatement alone -----------------------------------------------------------------------

class Restated:
    """tests/test_volumetric_gpu.py's Scene without the device"""

    def __init__(self, oracle, sfmt, gfmt, viewport=(0.0, 0.0), env_kw=()):
        self.oracle = oracle
        self.dfu = vc.field_uniforms() if sfmt is not None else vc.no_field_uniforms()
        self.otex = oracle.make_texture(vc.field_atlas(sfmt), sfmt) if sfmt is not None else None
        self.ogb = None
        if gfmt is not None:
            g = vc.gbuffer_texels() if gfmt == abi.GBUFFER_FLOAT4 else vc.gbuffer_texels().astype(np.float16).view(np.uint16)
            self.ogb = oracle.make_texture(g, gfmt)
            self.env = scenes.environment(gbuffer_size=(W, H), viewport_position=viewport, **dict(env_kw))
        else:
            self.env = scenes.environment(viewport_position=viewport, **dict(env_kw))
        self.pixels = vc.decode_pixels(oracle, self.env, self.ogb, W, H)

    def want(self, lights, dfu=None, **kw):
        return vc.render(self.oracle, lights, self.env, self.dfu if dfu is None else dfu, self.ogb, self.otex, vs.AMBIENT, W, H, pixels=self.pixels, **kw)


@pytest.fixture(scope="module")
def restated(oracle):
    cache = {}

    def get(sfmt=abi.SDF_UNORM16, gfmt=abi.GBUFFER_FLOAT4, viewport=(0.0, 0.0), env_kw=()):
        key = (sfmt, gfmt, viewport, tuple(env_kw))
        if key not in cache:
            cache[key] = Restated(oracle, sfmt, gfmt, viewport, env_kw)
        return cache[key]
    return get


@pytest.mark.parametrize("sfmt,gfmt", vs.FORMAT_PAIRS)
def test_scene_three_shapes(restated, sfmt, gfmt):
    vs.assert_three_shapes(restated(sfmt, gfmt).want(vs.three_shapes()), sfmt is not None, gfmt is not None)


@pytest.mark.parametrize("which", sorted(vs.SPECIAL))
def test_scene_special(restated, which):
    vs.SPECIAL[which][1](restated().want(vs.special(which)))


@pytest.mark.parametrize("steps", vs.STEP_COUNTS)
def test_scene_step_counts(restated, steps):
    vs.assert_step_counts(restated().want(vs.step_count_lights(steps), dfu=vc.field_uniforms(step_limit=steps)), steps)


def test_scene_five_lights(restated):
    vs.assert_five_lights(restated().want(vs.five_lights()))


def test_scene_invisible_columns(restated):
    want = restated(abi.SDF_UNORM16, abi.GBUFFER_FLOAT4, vc.INVISIBLE_VIEWPORT).want(vs.invisible_lights())
    assert want.stats[1] == W * H and all(x >= 22 for (x, _y, _i) in want.detail)
    assert (want.image[:, :22, 3] == 1).all() and (want.image[:, 22:, 3] == 2).sum() > 100


def test_scene_loop_guard(restated):
    vs.assert_stuck(restated(abi.SDF_UNORM16, None, (0.0, 0.0), vs.STUCK_ENVIRONMENT).want(vs.stuck_lights()))


def test_scene_exact_lights(restated):
    vs.assert_exact_lights(restated(abi.SDF_UNORM16, None).want(vs.exact_lights()))


@pytest.mark.parametrize("gfmt", [None, abi.GBUFFER_FLOAT4])
def test_scene_degenerate_lights(restated, gfmt):
    s = restated(abi.SDF_UNORM16, gfmt)
    want = s.want(vs.degenerate_lights())
    assert np.isfinite(want.image).all() and len(vs.lit(want)) > 100
    nan_contact = {k[2] for k, f in want.detail.items() if np.isnan(f["contact"])}
    assert {1, 5} <= nan_contact
    if gfmt is None:
        assert np.isnan(want.detail[(20, 10, 4)]["contact"]), "sdEllipsoid at its centre"
    vs.assert_dark(s.want(vs.dark_degenerate_lights()))
