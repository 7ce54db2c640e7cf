"""ilm_render_directional_lights on the device against the float32 restatement of tests/directional_common.py: every pixel within the
suite's criterion (tests.util.assert_close: 1e-4 relative with the lightmap floor), the three statistics exactly.

Frames of 44 x 27 pixels (3 x 2 workgroup tiles, 6 x 4 waves, partial ones at both rims) over a field of 48 x 32 texels per slice with a
tall box and an ellipsoid, MaxStepCount 24.  Scenes keep ShadowTraceLength > 2 and no zero direction with w = 1 (no normalize(0)).
"""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import directional_common as dc
from tests.util import assert_bits_equal, assert_close

pytestmark = pytest.mark.gpu

W, H = dc.WIDTH, dc.HEIGHT
AMBIENT = (0.0213, 0.0377, 0.0591, 1.0)


class Scene:
    """the device's resources and the oracle's textures of one (field format, G-buffer format) combination, with the decoded pixels"""

    def __init__(self, ctx, oracle, sfmt, gfmt, viewport=(0.0, 0.0), viewport_scale=(1.0, 1.0), render_scale=(1.0, 1.0)):
        self.ctx, self.oracle = ctx, oracle
        self.dfu = dc.field_uniforms() if sfmt is not None else dc.no_field_uniforms()
        self.sdf = self.otex = None
        if sfmt is not None:
            self.sdf = native.DistanceFieldTexture(ctx, dc.field_atlas(sfmt), sfmt)
            self.otex = oracle.make_texture(dc.field_atlas(sfmt), sfmt)
        self.gb = self.ogb = None
        if gfmt is not None:
            g = dc.gbuffer_texels() if gfmt == abi.GBUFFER_FLOAT4 else dc.gbuffer_texels().astype(np.float16).view(np.uint16)
            self.gb = native.GBufferTexture(ctx, g, gfmt)
            self.ogb = oracle.make_texture(g, gfmt)
            self.env = scenes.environment(gbuffer_size=(W, H), viewport_position=viewport, viewport_scale=viewport_scale, render_scale=render_scale)
        else:
            self.env = scenes.environment(viewport_position=viewport, viewport_scale=viewport_scale, render_scale=render_scale)
        self.pixels = dc.decode_pixels(oracle, self.env, self.ogb, W, H)

    def want(self, lights, ambient=AMBIENT, **kw):
        return dc.render(self.oracle, lights, self.env, self.dfu, self.ogb, self.otex, ambient, W, H, pixels=self.pixels, **kw)

    def got(self, lights, ambient=AMBIENT, fmt=abi.LIGHTMAP_FLOAT4, before=None, rows=(0, None), want_stats=True):
        lm = native.Lightmap(self.ctx, W, H, fmt)
        if before is not None:
            lm.upload(before)
        stats = native.render_directional_lights(self.ctx, dc.light_array(lights) if lights else None, self.env, self.dfu, self.gb, self.sdf, ambient, lm,
                                                 rows[0], rows[1], want_stats=want_stats)
        out = lm.download()
        lm.close()
        return out, ((stats.SdfSamples, stats.PixelLightPairs, stats.TracedPairs) if want_stats else None)

    def close(self):
        for x in (self.gb, self.sdf):
            if x is not None:
                x.close()


@pytest.fixture(scope="module")
def scene_cache(ctx, oracle):
    cache = {}

    def get(sfmt=abi.SDF_UNORM16, gfmt=abi.GBUFFER_FLOAT4, viewport=(0.0, 0.0), viewport_scale=(1.0, 1.0), render_scale=(1.0, 1.0)):
        key = (sfmt, gfmt, viewport, viewport_scale, render_scale)
        if key not in cache:
            cache[key] = Scene(ctx, oracle, sfmt, gfmt, viewport, viewport_scale, render_scale)
        return cache[key]
    yield get
    for s in cache.values():
        s.close()


def oblique(**kw):
    args = dict(direction=(0.55, 0.3, -0.6), color=(1.0, 0.8, 0.6, 0.9), shadow_trace_length=20.0, shadow_softness=2.0, shadow_ramp_rate=0.5,
                ao_radius=5.0, ao_opacity=0.6)
    args.update(kw)
    return dc.directional_light(**args)


def straight_down(**kw):
    args = dict(direction=(0.0, 0.0, -1.0), color=(0.2, 0.4, 0.9, 1.0), shadow_trace_length=18.0, shadow_softness=3.0, shadow_ramp_rate=1.0)
    args.update(kw)
    return dc.directional_light(**args)


def from_below(**kw):
    args = dict(direction=(0.4, -0.2, 0.25), color=(0.7, 0.1, 0.3, 1.0), shadow_trace_length=12.0, shadow_softness=1.0)
    args.update(kw)
    return dc.directional_light(**args)


def area_ambient(bounds=(5.25, 3.5, 30.75, 20.0), **kw):
    """a null direction with bounds whose edges lie inside wave tiles: the reference's ambient light in an area"""
    args = dict(direction=None, bounds=bounds, color=(0.3337, 0.1113, 0.7771, 0.75))
    args.update(kw)
    return dc.directional_light(**args)


def check(scene, lights, what, **kw):
    """The counting instantiation (directional_lights_kernel<FMT, true>) gives the statistics and is held to the restatement; the
    instantiation every other caller runs (<FMT, false>: another code object) is rendered beside it and must give the same bits."""
    want = scene.want(lights, **kw)
    got, stats = scene.got(lights)
    assert stats == want.stats, (what, stats, want.stats)
    assert_close(got, want.image, what)
    plain, none = scene.got(lights, want_stats=False)
    assert none is None
    assert_close(plain, want.image, what + ", without statistics")
    assert_bits_equal(plain, got, what + ": the instantiation without statistics against the counting one")
    return got, want


@pytest.mark.parametrize("sfmt,gfmt", [(abi.SDF_UNORM16, None), (abi.SDF_FP16, None), (abi.SDF_UNORM16, abi.GBUFFER_FLOAT4),
                                       (abi.SDF_FP16, abi.GBUFFER_HALF4), (None, abi.GBUFFER_FLOAT4), (None, None)])
def test_one_shadowed_light_over_fields_and_gbuffers(scene_cache, sfmt, gfmt):
    """one oblique light with shadows and AO: both field formats and no field, both G-buffer formats and the ground plane"""
    s = scene_cache(sfmt, gfmt)
    got, want = check(s, [oblique()], "one oblique light, field %r, G-buffer %r" % (sfmt, gfmt))
    samples, pairs, traced = want.stats
    assert pairs == W * H
    if sfmt is None:
        assert samples == 0 and traced == 0
    else:
        assert traced > W * H // 2 and samples > traced
        lit = want.image[..., 3] == 2
        assert (want.image[..., 0][lit] < 0.03).any() and (want.image[..., 0][lit] > 0.5).any(), "the frame has shadowed and lit pixels"
    if gfmt is not None:
        assert (got[12:14, 20:30, 3] == 1).all()                 # fullbright texels: discarded


def test_three_lights_directions_bounds_filters(scene_cache):
    """straight down and unbounded, from below with AO off, a bounded null direction; then each ShadowFilter value and shadows off"""
    s = scene_cache()
    got, want = check(s, [straight_down(), from_below(ao_radius=0.0), area_ambient()], "three lights")
    assert set(np.unique(want.image[..., 3])) == {1.0, 3.0, 4.0}          # fullbright: none; outside / inside the bounded light
    # the rows with shadows disabled (5..7) take the ShadowsOnly light not at all and the NoShadowsOnly light alone
    filters = [oblique(shadow_filter=1, bounds=(2.5, 1.25, 40.0, 12.5)), straight_down(shadow_filter=0, ao_radius=4.0, ao_opacity=0.5),
               oblique(shadow_filter=-1, casts_shadows=False, ao_radius=0.0)]
    got, want = check(s, filters, "shadow filters")
    assert (got[6, :, 3] == 3).all() and (got[9, 4:38, 3] == 3).all() and (got[20, :, 3] == 2).all()


def seventy_lights():
    lights = []
    pos = scenes.uniform(41, (70, 2), 0.0, 1.0)
    for i in range(70):
        x0, y0 = float(pos[i, 0]) * (W - 6) - 2.0, float(pos[i, 1]) * (H - 5) - 2.0
        bounds = (x0, y0, x0 + 4.0 + (i % 5) * 1.75, y0 + 3.0 + (i % 4) * 1.5)
        kind = i % 4
        if kind == 0:
            lights.append(area_ambient(bounds=bounds, color=(0.01 * i, 0.02, 0.03, 0.5)))
        elif kind == 1:
            lights.append(oblique(bounds=bounds, casts_shadows=(i % 8 == 1), ao_radius=0.0, color=(0.05, 0.01 * i, 0.02, 1.0)))
        elif kind == 2:
            lights.append(straight_down(bounds=bounds, casts_shadows=False, ao_radius=3.0, ao_opacity=0.4))
        else:
            lights.append(from_below(bounds=bounds, direction=(0.3, 0.2 - 0.01 * i, 0.05)))
    lights[35] = dc.directional_light(direction=None, color=(0.002, 0.003, 0.004, 1.0), casts_shadows=False)       # one unbounded
    return lights


def test_seventy_lights_in_one_call(scene_cache):
    s = scene_cache()
    got, want = check(s, seventy_lights(), "seventy lights")
    assert want.image[..., 3].max() >= 6 and want.stats[2] > 100


def test_pixels_that_are_not_visible_are_clipped(scene_cache):
    """a viewport position that puts the shaded x of columns 0 .. 21 at or below -9999: clip(), no rgb and no + 1 on alpha, no samples"""
    s = scene_cache(abi.SDF_UNORM16, None, dc.INVISIBLE_VIEWPORT)
    got, want = check(s, [straight_down(bounds=(-10030.0, -5.0, -9900.0, 50.0), ao_radius=4.0)], "invisible columns")
    assert (got[:, :22, 3] == 1).all() and (got[:, 22:, 3] == 2).all()
    assert want.stats[1] == W * H


def test_coverage_under_a_viewport_with_scales(scene_cache):
    """prepare_directional_lights_kernel's footprint on the device with ViewportPosition, ViewportScale and RenderScale all different from
    identity and different in x and y: (12 - 10) * (2 * 0.75) = 3 .. (16 - 10) * 1.5 = 9 in x, (23 - 20) * (0.5 * 4) = 6 .. (25.5 - 20) * 2 = 11
    in y (the rectangle tests/test_directional_kat.py derives), then a shadowed bounded light with fractional edges beside it."""
    s = scene_cache(abi.SDF_UNORM16, None, (10.0, 20.0), (2.0, 0.5), (0.75, 4.0))
    area = area_ambient(bounds=(12.0, 23.0, 16.0, 25.5))
    for want_stats in (True, False):
        got, _ = s.got([area], want_stats=want_stats)
        covered = np.zeros((H, W), bool)
        covered[6:11, 3:9] = True
        assert np.array_equal(got[..., 3] == 2, covered) and np.array_equal(got[..., 3] == 1, ~covered)
    got, want = check(s, [area, oblique(bounds=(13.3, 21.1, 33.7, 25.2))], "bounded lights under a scaled viewport")
    x0, y0, x1, y1 = dc.footprint(oblique(bounds=(13.3, 21.1, 33.7, 25.2)), s.env)
    assert 0 < x0 < x1 < W and 0 < y0 < y1 < H and want.stats[2] > 50


def test_ramp_bound_and_unbound(scene_cache, ctx):
    s = scene_cache()
    lights = [oblique(bounds=(3.5, 2.0, 36.25, 22.0)), from_below(), area_ambient()]
    plain, _ = check(s, lights, "no ramp")
    ramp = dc.ramp_texture()
    ctx.set_light_ramp(ramp)
    try:
        ramped, want = check(s, lights, "DirectionalLightWithRamp", ramp=ramp)
    finally:
        ctx.set_light_ramp(None)
    assert np.abs(ramped[..., :3] - plain[..., :3]).max() > 0.05
    # the null-direction light's opacity 1 became the ramp's value at u = 1, v = 0
    again, _ = check(s, lights, "no ramp again")
    assert_bits_equal(again, plain, "unbinding the ramp restores the plain technique")


def exact_lights():
    """lights whose opacity involves no transcendental function: null directions -- bit-equality with the restatement holds"""
    return [area_ambient(), area_ambient(bounds=(0.0, 10.5, 44.0, 18.5), color=(0.0123, 0.4567, 0.0891, 0.9)),
            dc.directional_light(direction=None, color=(0.11, 0.07, 0.05, 0.37))]


@pytest.mark.parametrize("blend_fp16", [False, True])
def test_lightmap_formats_and_blend_models(scene_cache, ctx, blend_fp16):
    """the three formats' stores and both blend models; clear and accumulate.  With lights of exact opacity the device equals the
    restatement bit for bit in every format; with shaded lights the fp32 model meets the criterion and the fp16-per-light model the
    sphere tests' (one fp16 ulp where a contribution sits on a rounding boundary, under 2 % of the texels)."""
    s = scene_cache()
    ctx.set_lightmap_blend(blend_fp16)
    try:
        want = s.want(exact_lights(), blend_fp16=blend_fp16)
        before32 = scenes.uniform(77, (H, W, 4), 0.0, 1.0)
        for fmt in (abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8):
            got, stats = s.got(exact_lights(), fmt=fmt)
            assert stats == want.stats
            assert np.array_equal(got, dc.to_stored(want.image, fmt)), "clear, format %d" % fmt
            assert np.array_equal(s.got(exact_lights(), fmt=fmt, want_stats=False)[0], got), "clear without statistics, format %d" % fmt
            # accumulate onto what a lightmap of this format holds
            before = dc.to_stored(before32, fmt)
            want_acc = s.want(exact_lights(), ambient=None, before=dc.from_stored(before, fmt), blend_fp16=blend_fp16)
            got, _ = s.got(exact_lights(), ambient=None, fmt=fmt, before=before, want_stats=False)
            assert np.array_equal(got, dc.to_stored(want_acc.image, fmt)), "accumulate, format %d" % fmt
        shaded = [oblique(), from_below(), area_ambient()]
        want = s.want(shaded, blend_fp16=blend_fp16)
        got32, stats = s.got(shaded)
        assert stats == want.stats
        if blend_fp16:
            assert np.array_equal(want.image, dc.half(want.image))
            diff = np.abs(got32 - want.image)
            assert (diff <= np.abs(want.image) * 2.0 ** -10 + 1e-7).all()
            assert (diff > 0).mean() < 0.02
        else:
            assert_close(got32, want.image, "shaded lights, fp32 accumulate")
        # the other formats store the same registers through their own rounding
        for fmt in (abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8):
            got, _ = s.got(shaded, fmt=fmt, want_stats=False)           # (the instantiation without statistics)
            assert np.array_equal(got, dc.to_stored(got32, fmt))
    finally:
        ctx.set_lightmap_blend(False)


def test_clear_with_any_light_count_and_accumulate(scene_cache):
    s = scene_cache(None, None)
    got, stats = s.got([], ambient=AMBIENT)
    assert np.array_equal(got, np.broadcast_to(np.asarray(AMBIENT, np.float32), (H, W, 4))) and stats == (0, 0, 0)
    before = scenes.uniform(5, (H, W, 4), 0.0, 2.0)
    got, _ = s.got([], ambient=None, before=before)
    assert_bits_equal(got, before, "zero lights, accumulate: nothing changes")
    lights = [oblique(), area_ambient()]
    want = s.want(lights, ambient=None, before=before)
    got, stats = s.got(lights, ambient=None, before=before)
    assert stats == want.stats
    assert_close(got, want.image, "accumulate onto a prefilled lightmap")


def test_a_strip_that_cuts_wave_tiles_leaves_the_other_rows_alone(scene_cache):
    s = scene_cache()
    lights = [oblique(), area_ambient()]
    before = scenes.uniform(9, (H, W, 4), 0.0, 1.0)
    full, _ = s.got(lights)
    for ambient in (AMBIENT, None):
        want = s.want(lights, ambient=ambient, before=before, row_begin=5, row_end=19)
        got, stats = s.got(lights, ambient=ambient, before=before, rows=(5, 19))
        assert stats == want.stats and stats[1] == 14 * W + sum(1 for y in range(5, 19) for x in range(W) if dc.covers((5.25, 3.5, 30.75, 20.0), x, y))
        assert_bits_equal(got[:5], before[:5], "rows above the strip")
        assert_bits_equal(got[19:], before[19:], "rows below the strip")
        assert_close(got, want.image, "strip [5, 19)")
        assert_bits_equal(s.got(lights, ambient=ambient, before=before, rows=(5, 19), want_stats=False)[0], got, "strip [5, 19) without statistics")
        if ambient is not None:
            assert_bits_equal(got[5:19], full[5:19], "a strip computes what the whole frame computes")
    # an empty strip is no work and no error
    got, stats = s.got(lights, ambient=None, before=before, rows=(7, 7))
    assert_bits_equal(got, before, "empty strip")
    assert stats == (0, 0, 0)


def test_a_sphere_group_then_a_directional_group_on_one_lightmap(scene_cache, ctx, oracle):
    """the frame as RenderLighting draws it: the sphere lights clear and light the target, the directional lights add to it.  A float4
    target: what is stored between the two calls is what the first computed."""
    s = scene_cache()
    spheres = (abi.LightVertex * 2)(scenes.sphere_light((12.0, 20.0, 9.0), 4.0, 30.0, color=(1.0, 0.9, 0.7, 1.0)),
                                    scenes.sphere_light((38.0, 6.0, 14.0), 3.0, 25.0, color=(0.3, 0.5, 1.0, 0.8), ao_radius=6.0, ao_opacity=0.5))
    directional = [oblique(), area_ambient()]
    lm = native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4)
    st_a = native.render_sphere_lights(ctx, spheres, s.env, s.dfu, s.gb, s.sdf, AMBIENT, lm, want_stats=True)
    st_b = native.render_directional_lights(ctx, dc.light_array(directional), s.env, s.dfu, s.gb, s.sdf, None, lm, want_stats=True)
    got = lm.download()
    lm.close()
    first, ost = oracle.render_sphere_lights(spheres, s.env, s.dfu, s.ogb, s.otex, AMBIENT, W, H, want_stats=True)
    want = s.want(directional, ambient=None, before=first)
    assert (st_a.SdfSamples, st_a.PixelLightPairs, st_a.TracedPairs) == (ost.SdfSamples, ost.PixelLightPairs, ost.TracedPairs)
    assert (st_b.SdfSamples, st_b.PixelLightPairs, st_b.TracedPairs) == want.stats
    assert_close(got, want.image, "sphere group + directional group")


def test_refusals(scene_cache, ctx):
    s = scene_cache()
    lib = native.lib()
    lm = native.Lightmap(ctx, W, H)
    lights = dc.light_array([oblique()])

    def call(ctx_h=None, lights_p=C.cast(lights, C.c_void_p), count=1, gb=None, sdf=None, lm_h=None, rows=(0, H), env=s.env, dfu=s.dfu):
        return lib.ilm_render_directional_lights(ctx.handle if ctx_h is None else ctx_h, lights_p, count, C.byref(env) if env is not None else None,
                                                 C.byref(dfu) if dfu is not None else None, s.gb.handle if gb is None else gb,
                                                 s.sdf.handle if sdf is None else sdf, None, lm.handle if lm_h is None else lm_h, rows[0], rows[1], None)
    before = lm.download()
    assert call(ctx_h=abi.Handle(0)) == abi.ERR_INVALID_HANDLE
    assert call(ctx_h=lm.handle) == abi.ERR_INVALID_HANDLE and b"context" in lib.ilm_last_error()
    assert call(lm_h=s.sdf.handle) == abi.ERR_INVALID_HANDLE and b"lightmap" in lib.ilm_last_error()
    assert call(gb=s.sdf.handle) == abi.ERR_INVALID_HANDLE and b"G-buffer" in lib.ilm_last_error()
    assert call(sdf=s.gb.handle) == abi.ERR_INVALID_HANDLE and b"distance field" in lib.ilm_last_error()
    assert call(count=-1) == abi.ERR_INVALID_ARGUMENT
    assert call(lights_p=None, count=1) == abi.ERR_INVALID_ARGUMENT and b"light array" in lib.ilm_last_error()
    assert call(env=None) == abi.ERR_INVALID_ARGUMENT and call(dfu=None) == abi.ERR_INVALID_ARGUMENT
    for rows in ((-1, H), (0, H + 1), (9, 8)):
        assert call(rows=rows) == abi.ERR_OUT_OF_RANGE and b"rows" in lib.ilm_last_error()
    for what, bounds, word in (("inverted x", (30.0, 2.0, 10.0, 20.0), b"inverted"), ("inverted y", (3.0, 20.0, 10.0, 2.0), b"inverted"),
                               ("NaN", (3.0, float("nan"), 10.0, 20.0), b"NaN"), ("NaN corner", (3.0, 2.0, float("nan"), 20.0), b"NaN")):
        bad = dc.light_array([oblique(), area_ambient(bounds=bounds)])
        assert call(lights_p=C.cast(bad, C.c_void_p), count=2) == abi.ERR_INVALID_ARGUMENT, what
        assert word in lib.ilm_last_error() and b"light 1" in lib.ilm_last_error()
    # a degenerate rectangle is not inverted: it covers nothing
    empty = dc.light_array([area_ambient(bounds=(7.0, 7.0, 7.0, 7.0))])
    assert call(lights_p=C.cast(empty, C.c_void_p)) == abi.OK
    assert_bits_equal(lm.download(), before, "no refused call, and no empty rectangle, wrote a texel")
    lm.close()


# ---- the host mirror ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def Host():
    from illuminant_amd import _host
    return _host


@pytest.fixture(scope="module")
def hctx(Host):
    return Host.DeviceContext(0)


def host_directional(Host, light_kw):
    d = Host.DirectionalLightSource()
    for k, v in light_kw.items():
        setattr(d, k, v)
    return d


def host_renderer(Host, hctx, env):
    rc = Host.RendererConfiguration(W, H)
    rc.FloatLightmap = True
    q = Host.RendererQualitySettings()
    q.MinStepSize, q.LongStepFactor, q.MaxStepCount, q.MaxConeRadius, q.OcclusionToOpacityPower = 1.5, 0.75, dc.MAX_STEP_COUNT, 8.0, 0.8
    rc.DefaultQuality = q
    r = Host.LightingRenderer(hctx, rc, env)
    field = Host.DistanceField(hctx, 48, 32, 32.0, 12, 1.0)
    field.Load(dc.field_atlas(abi.SDF_UNORM16))
    r.DistanceField = field
    return r, field


def host_sphere(Host, position, sort_key=0, texture=None):
    l = Host.SphereLightSource()
    l.Position = list(position)
    l.Radius, l.RampLength, l.SortKey = 3.0, 28.0, sort_key
    l.Color = [0.9, 0.7, 0.5, 1.0]
    if texture is not None:
        l.TextureRef = texture
    return l


def test_render_lighting_over_a_mixed_environment_equals_the_direct_calls(Host, hctx, ctx, oracle):
    """sort order (SortKey, directional after spheres of equal key), groups by ramp texture in first-appearance order, sphere groups
    before directional groups, the clear on the first launch: the frame equals the same calls made through the C ABI, bit for bit"""
    ramp = dc.ramp_texture()
    tex = Host.RampTexture(ramp)
    env = Host.LightingEnvironment()
    env.Ambient = list(AMBIENT)
    env.Lights = [host_sphere(Host, (30.0, 8.0, 10.0), sort_key=2), host_sphere(Host, (10.0, 20.0, 6.0), sort_key=0, texture=tex)]
    a = host_directional(Host, dict(Direction=[0.55, 0.3, -0.6], ShadowTraceLength=20.0, ShadowSoftness=2.0, SortKey=1, Color=[1.0, 0.8, 0.6, 0.9]))
    b = host_directional(Host, dict(Bounds=[5.25, 3.5, 30.75, 20.0], Color=[0.3, 0.1, 0.7, 0.75], SortKey=0, TextureRef=tex))
    c = host_directional(Host, dict(Direction=[0.0, 0.0, -1.0], ShadowTraceLength=18.0, SortKey=0, AmbientOcclusionRadius=4.0, AmbientOcclusionOpacity=0.5))
    off = host_directional(Host, dict(Enabled=False))
    unseen = host_directional(Host, dict(Opacity=0.0))
    env.DirectionalLights = [a, b, c, off, unseen]
    r, field = host_renderer(Host, hctx, env)
    stats = r.RenderLighting(1.0, 0, -1, True)
    got = r.ReadLightmap()
    r.RenderLighting(1.0, 0, -1, False)
    assert_bits_equal(r.ReadLightmap(), got, "the frame without statistics against the counting frame")
    packed = np.frombuffer(r.GetPackedLightVertices(), np.float32).reshape(-1, 8, 4)
    pack = lambda d: np.frombuffer(Host.LightingRenderer.PackDirectionalLightBytes(d, 1.0), np.float32).reshape(8, 4)
    sphere = lambda l: np.frombuffer(Host.LightingRenderer.PackSphereLightBytes(l, 1.0, True), np.float32).reshape(8, 4)
    # key 0: the sphere, then b and c in list order; key 1: a; key 2: the other sphere
    order = [sphere(env.Lights[1]), pack(b), pack(c), pack(a), sphere(env.Lights[0])]
    assert packed.shape[0] == 5 and all(np.array_equal(packed[i], order[i]) for i in range(5))
    # the same frame through the C ABI: sphere groups (ramp, none), then directional groups (ramp: b; none: c, a)
    dfu = abi.DistanceFieldUniforms.from_buffer_copy(r.GetDistanceFieldUniformsBytes())
    envu = abi.Environment.from_buffer_copy(r.GetEnvironmentUniformsBytes())
    assert bytes(dfu) == bytes(dc.field_uniforms())
    sdf = native.DistanceFieldTexture(ctx, dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    lm = native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4)

    def vertices(rows):
        arr = (abi.LightVertex * len(rows))()
        for i, row in enumerate(rows):
            C.memmove(C.addressof(arr[i]), np.ascontiguousarray(row, np.float32).ctypes.data, 128)
        return arr
    total = np.zeros(3, np.int64)

    def add(st):
        total[:] += (st.SdfSamples, st.PixelLightPairs, st.TracedPairs)
    ctx.set_light_ramp(ramp)
    add(native.render_sphere_lights(ctx, vertices([order[0]]), envu, dfu, None, sdf, AMBIENT, lm, want_stats=True))
    ctx.set_light_ramp(None)
    add(native.render_sphere_lights(ctx, vertices([order[4]]), envu, dfu, None, sdf, None, lm, want_stats=True))
    ctx.set_light_ramp(ramp)
    add(native.render_directional_lights(ctx, vertices([order[1]]), envu, dfu, None, sdf, None, lm, want_stats=True))
    ctx.set_light_ramp(None)
    add(native.render_directional_lights(ctx, vertices([order[2], order[3]]), envu, dfu, None, sdf, None, lm, want_stats=True))
    assert_bits_equal(got, lm.download(), "RenderLighting against the direct calls")
    assert [int(x) for x in stats] == [int(x) for x in total]
    # and the directional part against the restatement, on top of what the sphere groups left
    lm2 = native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4)
    ctx.set_light_ramp(ramp)
    native.render_sphere_lights(ctx, vertices([order[0]]), envu, dfu, None, sdf, AMBIENT, lm2)
    ctx.set_light_ramp(None)
    native.render_sphere_lights(ctx, vertices([order[4]]), envu, dfu, None, sdf, None, lm2)
    spheres_only = lm2.download()
    otex = oracle.make_texture(dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    pixels = dc.decode_pixels(oracle, envu, None, W, H)
    step = dc.render(oracle, vertices([order[1]]), envu, dfu, None, otex, None, W, H, ramp=ramp, before=spheres_only, pixels=pixels)
    want = dc.render(oracle, vertices([order[2], order[3]]), envu, dfu, None, otex, None, W, H, before=step.image, pixels=pixels)
    assert_close(got, want.image, "RenderLighting against the restatement")
    # directional lights alone: their first launch carries the clear
    env.Lights = []
    env.DirectionalLights = [b]
    r.RenderLighting(1.0, 0, -1, False)
    alone = dc.render(oracle, vertices([pack(b)]), envu, dfu, None, otex, AMBIENT, W, H, ramp=ramp, pixels=pixels)
    assert_close(r.ReadLightmap(), alone.image, "a frame of directional lights alone is cleared by their first launch")
    for x in (lm, lm2, sdf):
        x.close()


def test_directional_lights_with_probes_are_refused(Host, hctx):
    env = Host.LightingEnvironment()
    env.Lights = [host_sphere(Host, (10.0, 10.0, 5.0))]
    env.DirectionalLights = [host_directional(Host, dict(Direction=[0.0, 0.0, -1.0]))]
    r, field = host_renderer(Host, hctx, env)
    probe = Host.LightProbe()
    probe.Position = [12.0, 9.0, 2.0]
    r.Probes.Add(probe)
    with pytest.raises(Host.InvalidOperationException, match="directional lights do not reach light probes yet"):
        r.RenderLighting()
    # a disabled directional light does not trip the refusal
    env.DirectionalLights = [host_directional(Host, dict(Enabled=False))]
    r.RenderLighting()
    assert r.Probes[0].Value[3] > 0


def test_an_environment_without_directional_lights_renders_what_it_rendered(Host, hctx, oracle):
    env = Host.LightingEnvironment()
    env.Ambient = list(AMBIENT)
    env.Lights = [host_sphere(Host, (30.0, 8.0, 10.0)), host_sphere(Host, (10.0, 20.0, 6.0))]
    assert len(env.DirectionalLights) == 0
    r, field = host_renderer(Host, hctx, env)
    stats = r.RenderLighting(1.0, 0, -1, True)
    dfu = abi.DistanceFieldUniforms.from_buffer_copy(r.GetDistanceFieldUniformsBytes())
    envu = abi.Environment.from_buffer_copy(r.GetEnvironmentUniformsBytes())
    packed = (abi.LightVertex * 2)(*[scenes.sphere_light(tuple(l.Position), l.Radius, l.RampLength, color=tuple(l.Color)) for l in env.Lights])
    assert r.GetPackedLightVertices() == bytes(packed)
    want, ost = oracle.render_sphere_lights(packed, envu, dfu, None, oracle.make_texture(dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16), AMBIENT, W, H,
                                            want_stats=True)
    assert_close(r.ReadLightmap(), want, "sphere lights alone")
    assert tuple(int(x) for x in stats) == (ost.SdfSamples, ost.PixelLightPairs, ost.TracedPairs)
