"""ilm_render_projector_lights on the device against the float32 restatement of tests/projector_common.py: every pixel within the
suite's criterion (tests.util.assert_close: 1e-4 relative with the lightmap floor), the three statistics exactly, the counting and the
plain instantiation bit-equal.

The directional suite's shapes: frames of 44 x 27 pixels (3 x 2 workgroup tiles, 6 x 4 waves, partial ones at both rims) over a field of
48 x 32 texels per slice with a tall box and an ellipsoid, MaxStepCount 24; textures of 5 x 3 (no power of two: the wrap arithmetic)
and 8 x 8 texels.  What a scene must contain for its comparison to mean something is asserted from the restatement inside `check`:
lit pixels, shadowed and unshadowed traces, bounding rectangles whose edges keep 1 / 64 pixel from every pixel centre (evaluated in
float64: a last-bit difference in the inverse cannot flip coverage), no shaded point at an origin.
"""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import directional_common as dc
from tests import projector_common as pc
from tests.util import assert_bits_equal, assert_close

pytestmark = pytest.mark.gpu

W, H = pc.WIDTH, pc.HEIGHT
AMBIENT = (0.0213, 0.0377, 0.0591, 1.0)


def gbuffer_texels(kind):
    """"plain": the directional suite's G-buffer (relative_y = 0).  "raised": rows 14 .. 23 carry relative_y = -9, so their shaded points
    lie 9 units up the frame, inside the volume of a light whose rectangle ends above those rows."""
    g = np.array(dc.gbuffer_texels(), np.float32, copy=True)
    if kind == "raised":
        g[14:24, :, 2] = -9.0
    return g


class Scene:
    """the oracle's textures and decoded pixels of one (field format, G-buffer format, viewport) combination, and -- with a context --
    the device's resources"""

    def __init__(self, ctx, oracle, sfmt, gfmt, viewport=(0.0, 0.0), viewport_scale=(1.0, 1.0), render_scale=(1.0, 1.0), gbuffer="plain",
                 z_to_y=0.0):
        self.ctx, self.oracle = ctx, oracle
        self.dfu = dc.field_uniforms() if sfmt is not None else dc.no_field_uniforms()
        self.sdf = self.otex = None
        if sfmt is not None:
            self.sdf = native.DistanceFieldTexture(ctx, dc.field_atlas(sfmt), sfmt) if ctx is not None else None
            self.otex = oracle.make_texture(dc.field_atlas(sfmt), sfmt)
        self.gb = self.ogb = None
        kw = dict(viewport_position=viewport, viewport_scale=viewport_scale, render_scale=render_scale, z_to_y=z_to_y, maximum_z=32.0)
        if gfmt is not None:
            g = gbuffer_texels(gbuffer) if gfmt == abi.GBUFFER_FLOAT4 else gbuffer_texels(gbuffer).astype(np.float16).view(np.uint16)
            self.gb = native.GBufferTexture(ctx, g, gfmt) if ctx is not None else None
            self.ogb = oracle.make_texture(g, gfmt)
            self.env = scenes.environment(gbuffer_size=(W, H), **kw)
        else:
            self.env = scenes.environment(**kw)
        self.pixels = pc.decode_pixels(oracle, self.env, self.ogb, W, H)

    def want(self, lights, texture, ambient=AMBIENT, **kw):
        return pc.render(self.oracle, lights, texture, self.env, self.dfu, self.ogb, self.otex, ambient, W, H, pixels=self.pixels, **kw)

    def got(self, lights, texture, ambient=AMBIENT, fmt=abi.LIGHTMAP_FLOAT4, before=None, rows=(0, None), want_stats=True):
        lm = native.Lightmap(self.ctx, W, H, fmt)
        if before is not None:
            lm.upload(before)
        native.set_projector_texture(self.ctx, texture)
        stats = native.render_projector_lights(self.ctx, pc.light_array(lights) if lights else None, self.env, self.dfu, self.gb, self.sdf, ambient, lm,
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

    def get(sfmt=abi.SDF_UNORM16, gfmt=abi.GBUFFER_FLOAT4, **kw):
        key = (sfmt, gfmt, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = Scene(ctx, oracle, sfmt, gfmt, **kw)
        return cache[key]
    yield get
    for s in cache.values():
        s.close()


# ---- the lights ----------------------------------------------------------------------------------------------------------------

def clamped(scale=(40.0, 24.0, 64.0), translation=(2.3, 1.6, 0.0), origin=(24.0, 10.0, 40.0), **kw):
    """a clamped, shadowed light with AO over most of the frame: the world rectangle 2.3 .. 42.3 x 1.6 .. 25.6, its edges 0.1 .. 0.2
    pixels from the nearest pixel centres"""
    args = dict(origin=origin, radius=2.0, ramp_length=30.0, ao_radius=5.0, ao_opacity=0.6, opacity=0.9)
    rotation = kw.pop("rotation_z", 0.0)
    args.update(kw)
    return pc.projector_light(pc.forward_matrix(scale, translation, rotation_z=rotation), **args)


def wrapping(scale=(16.0, 9.0, 64.0), translation=(1.25, 0.75, 0.0), origin=(30.0, 20.0, 35.0), **kw):
    """a wrapping light: the texture tiles the world, every pixel of any frame is covered"""
    args = dict(origin=origin, radius=1.5, ramp_length=25.0, wrap=True, opacity=0.8)
    args.update(kw)
    return pc.projector_light(pc.forward_matrix(scale, translation), **args)


def perspective(**kw):
    """m14 of the packed inverse is 0.004: w = 1 + 0.004 x grows from 1 to 1.18 across the frame (above 0.25 everywhere)"""
    l = clamped(scale=(36.0, 22.0, 64.0), translation=(1.3, 1.7, 0.0), **kw)
    l.LightPosition1.w = 0.004
    return l


def check(scene, lights, texture, what, shadowed=True, **kw):
    """The counting instantiation (projector_lights_kernel<FMT, true>) gives the statistics and is held to the restatement; the
    instantiation every other caller runs (<FMT, false>) is rendered beside it and must give the same bits.  Before that, what the
    scene must contain is asserted from the restatement."""
    want = scene.want(lights, texture, **kw)
    scene_facts(scene, lights, want, what, shadowed)
    got, stats = scene.got(lights, texture)
    assert stats == want.stats, (what, stats, want.stats)
    assert_close(got, want.image, what)
    plain, none = scene.got(lights, texture, want_stats=False)
    assert none is None
    assert_close(plain, want.image, what + ", without statistics")
    assert_bits_equal(plain, got, what + ": the instantiation without statistics against the counting one")
    return got, want


def scene_facts(scene, lights, want, what, shadowed=True):
    """a test may not hide a failure: the frame is lit, traces end both shadowed and unshadowed, no pixel centre lies within 1 / 64 pixel
    of a bounding rectangle's edge, no shaded point sits at an origin"""
    lit = {(x, y) for (x, y, i), f in want.detail.items() if f["opacity"] > 0}
    assert len(lit) >= 0.25 * W * H, (what, "lit pixels", len(lit))
    if shadowed and scene.otex is not None:
        cones = [f["cone"] for f in want.detail.values() if "cone" in f]
        assert sum(1 for c in cones if c < 0.1) >= 20 and sum(1 for c in cones if c > 0.9) >= 20, (what, "cone opacities", len(cones))
    for l in lights:
        if l.MoreLightProperties.z > 0.5:
            assert pc.edge_margin(l, scene.env) >= 1.0 / 64.0, (what, "a pixel centre within 1 / 64 pixel of the bounding rectangle")
        if l.LightPosition3.w != 0:
            o = l.LightPosition3
            assert all((p[0][0], p[0][1], p[0][2]) != (o.x, o.y, o.z) for p in scene.pixels), (what, "a shaded point at the origin")


# ---- the cases -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sfmt,gfmt", [(abi.SDF_UNORM16, None), (abi.SDF_FP16, None), (abi.SDF_UNORM16, abi.GBUFFER_FLOAT4),
                                       (abi.SDF_FP16, abi.GBUFFER_HALF4), (None, abi.GBUFFER_FLOAT4), (None, None)])
def test_one_clamped_shadowed_light_over_fields_and_gbuffers(scene_cache, sfmt, gfmt):
    """one clamped light with shadows and AO: both field formats and no field, both G-buffer formats and the ground plane"""
    s = scene_cache(sfmt, gfmt)
    got, want = check(s, [clamped()], pc.texture(5, 3), "one clamped light, field %r, G-buffer %r" % (sfmt, gfmt))
    samples, pairs, traced = want.stats
    assert pairs == 40 * 24                      # columns 2 .. 41, rows 2 .. 25: the centres inside 2.3 .. 42.3 x 1.6 .. 25.6
    if sfmt is None:
        assert samples == 0 and traced == 0
    else:
        assert traced > 400 and samples > traced
    assert (got[0, :, 3] == 1).all() and (got[:, 43, 3] == 1).all()          # outside the rectangle: alpha untouched
    if gfmt is not None:
        assert (got[12:14, 20:30, 3] == 1).all()                 # fullbright texels: discarded


def test_a_wrapping_light_covers_every_pixel(scene_cache):
    s = scene_cache()
    got, want = check(s, [wrapping()], pc.texture(5, 3), "a wrapping light")
    assert want.stats[1] == W * H
    fullbright = np.zeros((H, W), bool)
    fullbright[12:14, 20:30] = True
    assert np.array_equal(got[..., 3] == 2, ~fullbright)


def test_a_region_that_is_a_part_of_the_texture(scene_cache):
    """region (0.25, 0.2) .. (0.85, 0.8) of the 8 x 8 texture: 0.6 x 0.6 of the forward scale, 3.3 .. 39.3 x 2.7 .. 24.3 in the world"""
    s = scene_cache()
    l = clamped(scale=(60.0, 36.0, 64.0), translation=(3.3, 2.7, 0.0), region=(0.25, 0.2, 0.85, 0.8))
    got, want = check(s, [l], pc.texture(8, 8), "a sub-rectangle of the texture")
    assert want.stats[1] == 36 * 21                      # columns 3 .. 38, rows 3 .. 23
    uv = np.array([f["uv"] for f in want.detail.values()], np.float64)
    assert uv[:, 0].min() >= 0.25 and uv[:, 0].max() <= 0.85 and uv[:, 1].min() >= 0.2 and uv[:, 1].max() <= 0.8
    assert uv[:, 0].max() - uv[:, 0].min() > 0.5


def test_a_rotated_projector(scene_cache):
    """30 degrees about z: the rectangle is the box of the rotated volume's corners, and the pixels in its corners are discarded"""
    s = scene_cache()
    l = clamped(scale=(30.0, 18.0, 64.0), translation=(14.2, 1.3, 0.0), rotation_z=np.pi / 6)
    got, want = check(s, [l], pc.texture(5, 3), "a rotated projector")
    covered = want.stats[1]
    assert len(want.detail) < 0.8 * covered and len(want.detail) > 0.3 * covered          # the rectangle's corners lie outside the volume


def test_a_perspective_row(scene_cache):
    s = scene_cache()
    l = perspective()
    got, want = check(s, [l], pc.texture(8, 8), "a perspective row")
    ws = [float(f["w"]) for f in want.detail.values()]
    assert min(ws) > 0.25 and max(ws) - min(ws) > 0.1


def test_an_origin_above_the_tall_box(scene_cache):
    """the box (10 .. 20 x 8 .. 16, 24 high) shadows the pixels around its foot"""
    s = scene_cache(abi.SDF_UNORM16, None)
    l = clamped(origin=(15.0, 12.0, 60.0), ao_radius=0.0)
    got, want = check(s, [l], pc.texture(8, 8), "origin above the tall box")
    near = [f["cone"] for (x, y, i), f in want.detail.items() if 6 <= x <= 24 and 4 <= y <= 20 and "cone" in f]
    far = [f["cone"] for (x, y, i), f in want.detail.items() if x >= 30 and "cone" in f]
    assert min(near) < 0.05 and np.mean(far) > 0.5


def test_no_origin(scene_cache):
    """LightPosition3 = 0 and shadows packed off: no trace, normal opacity 1 -- no transcendental function, the device equals the
    restatement bit for bit"""
    s = scene_cache()
    l = clamped(origin=None, ao_radius=0.0)
    assert l.LightProperties.w == 0 and l.LightPosition3.w == 0
    got, want = check(s, [l], pc.texture(5, 3), "no origin", shadowed=False)
    assert want.stats[2] == 0 and want.stats[0] == 0
    assert_bits_equal(got, want.image, "no origin: exact arithmetic")


def test_the_rectangle_cuts_lit_texels_moved_by_relative_y(scene_cache):
    """rows 14 .. 23 of this G-buffer carry relative_y = -9: their shaded points lie inside the volume of a light whose world rectangle
    ends at y = 13.6, and the rectangle -- coverage is the quad's, not the volume's -- cuts them"""
    s = scene_cache(abi.SDF_UNORM16, abi.GBUFFER_FLOAT4, gbuffer="raised")
    l = clamped(scale=(40.0, 12.0, 64.0), translation=(2.3, 1.6, 0.0))
    got, want = check(s, [l], pc.texture(5, 3), "relative_y against the rectangle", probe_uncovered=True)
    assert want.uncovered_visible >= 100
    assert (got[14:24, :, 3] == 1).all()


def three_lights():
    return [clamped(), wrapping(opacity=0.4), clamped(scale=(20.0, 14.0, 64.0), translation=(18.3, 8.7, 0.0), origin=(5.0, 25.0, 30.0), ao_radius=0.0)]


@pytest.mark.parametrize("blend_fp16", [False, True])
def test_three_lights_in_one_call_in_both_blend_models(scene_cache, ctx, blend_fp16):
    """list order in fp32 registers, or the fp16-per-light chain; then the same onto an uploaded lightmap with ambient == NULL"""
    s = scene_cache()
    tex = pc.texture(8, 8)
    ctx.set_lightmap_blend(blend_fp16)
    try:
        before = scenes.uniform(77, (H, W, 4), 0.0, 1.0)
        for ambient, start in ((AMBIENT, None), (None, before)):
            want = s.want(three_lights(), tex, ambient=ambient, before=start, blend_fp16=blend_fp16)
            if ambient is not None:
                scene_facts(s, three_lights(), want, "three lights")
                assert max(a for a in np.unique(want.image[..., 3])) == 4
            got, stats = s.got(three_lights(), tex, ambient=ambient, before=start)
            assert stats == want.stats
            plain, _ = s.got(three_lights(), tex, ambient=ambient, before=start, want_stats=False)
            assert_bits_equal(plain, got, "three lights without statistics")
            if blend_fp16:
                # the sphere tests' criterion for this model: one fp16 ulp where a contribution sits on a rounding boundary, rarely
                assert np.array_equal(want.image, pc.half(want.image))
                diff = np.abs(got - want.image)
                assert (diff <= np.abs(want.image) * 2.0 ** -10 + 1e-7).all()
                assert (diff > 0).mean() < 0.02
            else:
                assert_close(got, want.image, "three lights, fp32 accumulate, ambient %r" % (ambient is not None))
    finally:
        ctx.set_lightmap_blend(False)


def test_rows_5_to_21_leave_the_other_rows_alone(scene_cache):
    s = scene_cache()
    tex = pc.texture(5, 3)
    lights = [clamped(), wrapping(opacity=0.4)]
    before = scenes.uniform(9, (H, W, 4), 0.0, 1.0)
    scene_facts(s, lights, s.want(lights, tex), "the frame the strip is cut from")
    full, _ = s.got(lights, tex)
    for ambient in (AMBIENT, None):
        want = s.want(lights, tex, ambient=ambient, before=before, row_begin=5, row_end=21)
        scene_facts(s, lights, want, "strip [5, 21)")                # the strip alone holds what a scene must hold
        got, stats = s.got(lights, tex, ambient=ambient, before=before, rows=(5, 21))
        assert stats == want.stats and stats[1] == 16 * W + 16 * 40
        assert_bits_equal(got[:5], before[:5], "rows above the strip")
        assert_bits_equal(got[21:], before[21:], "rows below the strip")
        assert_close(got, want.image, "strip [5, 21)")
        assert_bits_equal(s.got(lights, tex, ambient=ambient, before=before, rows=(5, 21), want_stats=False)[0], got, "strip [5, 21) without statistics")
        if ambient is not None:
            assert_bits_equal(got[5:21], full[5:21], "a strip computes what the whole frame computes")


def test_a_viewport_offset_and_a_render_scale(scene_cache):
    """ViewportPosition (10, 20), ViewportScale (2, 0.5), RenderScale (0.75, 4), ZToY 0.125 with MaximumZ 32: the world rectangle
    12.2 .. 36.2 x 23.1 .. 27.1 padded by 4 in y maps to 3.3 .. 39.3 x -1.8 .. 22.2 on the screen.  The frame shows the world from
    (10, 20) to (39, 33): of the field's obstacles only the ellipsoid's near side (y up to 23) lies in it, so both origins sit beyond
    the ellipsoid, above its far side, and the traces of the points in front of it run through it."""
    s = scene_cache(abi.SDF_UNORM16, None, viewport=(10.0, 20.0), viewport_scale=(2.0, 0.5), render_scale=(0.75, 4.0), z_to_y=0.125)
    l = clamped(scale=(24.0, 4.0, 64.0), translation=(12.2, 23.1, 0.0), origin=(33.0, 14.0, 14.0), ao_radius=0.0)
    assert np.allclose(pc.footprint64(l, s.env), (3.3, -1.8, 39.3, 22.2), rtol=0, atol=1e-4)
    got, want = check(s, [l, wrapping(scale=(7.0, 3.0, 64.0), translation=(10.0, 20.0, 0.0), origin=(33.0, 15.0, 16.0))], pc.texture(5, 3),
                      "a scaled viewport")
    assert want.stats[1] == W * H + 36 * 22
    shadows = [f["cone"] for (x, y, i), f in want.detail.items() if i == 0]
    assert sum(1 for c in shadows if c < 0.1) >= 20 and sum(1 for c in shadows if c > 0.9) >= 20          # the clamped light's own traces


def test_lightmap_formats(scene_cache):
    """the three formats store the same registers through their own rounding; accumulate reads what the format holds"""
    s = scene_cache()
    tex = pc.texture(8, 8)
    exact = [clamped(origin=None, ao_radius=0.0), wrapping(origin=None)]          # no transcendental function: bit-equality with the restatement
    want = s.want(exact, tex)
    scene_facts(s, exact, want, "lights of exact opacity", shadowed=False)          # (packed without an origin: nothing traces)
    assert want.stats[2] == 0
    before32 = scenes.uniform(78, (H, W, 4), 0.0, 1.0)
    for fmt in (abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8):
        got, stats = s.got(exact, tex, fmt=fmt)
        assert stats == want.stats
        assert np.array_equal(got, pc.to_stored(want.image, fmt)), "clear, format %d" % fmt
        before = pc.to_stored(before32, fmt)
        want_acc = s.want(exact, tex, ambient=None, before=pc.from_stored(before, fmt))
        got, _ = s.got(exact, tex, ambient=None, fmt=fmt, before=before, want_stats=False)
        assert np.array_equal(got, pc.to_stored(want_acc.image, fmt)), "accumulate, format %d" % fmt
    shaded = three_lights()
    scene_facts(s, shaded, s.want(shaded, tex), "three lights")
    got32, _ = s.got(shaded, tex)
    for fmt in (abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8):
        got, _ = s.got(shaded, tex, fmt=fmt, want_stats=False)
        assert np.array_equal(got, pc.to_stored(got32, fmt))


def test_zero_lights_with_and_without_ambient(scene_cache, ctx):
    s = scene_cache(None, None)
    for tex in (pc.texture(5, 3), None):                # with no lights the call needs no texture
        got, stats = s.got([], tex, ambient=AMBIENT)
        assert np.array_equal(got, np.broadcast_to(np.asarray(AMBIENT, np.float32), (H, W, 4))) and stats == (0, 0, 0)
        before = scenes.uniform(5, (H, W, 4), 0.0, 2.0)
        got, _ = s.got([], tex, ambient=None, before=before)
        assert_bits_equal(got, before, "zero lights, accumulate: nothing changes")


@pytest.mark.parametrize("translation", [1e9, 3e38])
def test_translations_far_past_the_texture(scene_cache, translation):
    """a wrapping light 1e9 and 3e38 units away: texture coordinates of -1e9 and -3e38, whose products with the texture's width are
    huge integers and an overflow to infinity.  The taps come from exact integer arithmetic (tap 0 and a NaN weight for the infinity);
    no origin, so nothing else differs: the image equals the restatement's bit for bit."""
    s = scene_cache(abi.SDF_UNORM16, None)
    l = wrapping(scale=(1.0, 1.0, 16.0), translation=(translation, -translation / 3, 0.0), origin=None)
    tex = pc.texture(5, 3)
    want = s.want([l], tex)
    scene_facts(s, [l], want, "translation %g" % translation, shadowed=False)      # (no origin: nothing traces; every pixel takes light)
    assert want.stats[2] == 0
    u = np.array([f["uv"][0] for f in want.detail.values()], np.float64)
    assert len(want.detail) == W * H and (np.abs(u) > 9e8).all()
    if translation > 1e38:
        assert np.isnan(want.image[..., :3]).all()
    else:
        assert np.isfinite(want.image).all() and len(np.unique(want.image[..., 0])) > 3
    for want_stats in (True, False):
        got, stats = s.got([l], tex, want_stats=want_stats)
        assert_bits_equal(got, want.image, "translation %g" % translation)
        assert stats is None or stats == want.stats


def test_refusals(scene_cache, ctx):
    s = scene_cache()
    lib = native.lib()
    lm = native.Lightmap(ctx, W, H)
    lights = pc.light_array([clamped()])
    native.set_projector_texture(ctx, pc.texture(5, 3))

    def call(ctx_h=None, lights_p=C.cast(lights, C.c_void_p), count=1, gb=None, sdf=None, lm_h=None, rows=(0, H), env=s.env, dfu=s.dfu):
        return lib.ilm_render_projector_lights(ctx.handle if ctx_h is None else ctx_h, lights_p, count, C.byref(env) if env is not None else None,
                                               C.byref(dfu) if dfu is not None else None, s.gb.handle if gb is None else gb,
                                               s.sdf.handle if sdf is None else sdf, None, lm.handle if lm_h is None else lm_h, rows[0], rows[1], None)
    before = lm.download()
    assert call(ctx_h=abi.Handle(0)) == abi.ERR_INVALID_HANDLE
    assert call(ctx_h=lm.handle) == abi.ERR_INVALID_HANDLE and b"context" in lib.ilm_last_error()
    assert call(lm_h=s.sdf.handle) == abi.ERR_INVALID_HANDLE and b"lightmap" in lib.ilm_last_error()
    assert call(gb=s.sdf.handle) == abi.ERR_INVALID_HANDLE and b"G-buffer" in lib.ilm_last_error()
    assert call(sdf=s.gb.handle) == abi.ERR_INVALID_HANDLE and b"distance field" in lib.ilm_last_error()
    assert call(count=-1) == abi.ERR_INVALID_ARGUMENT
    assert call(count=(1 << 24) + 1) == abi.ERR_INVALID_ARGUMENT and b"at most" in lib.ilm_last_error()          # refused before anything is read
    assert call(count=2 ** 31 - 1) == abi.ERR_INVALID_ARGUMENT
    assert call(lights_p=None, count=1) == abi.ERR_INVALID_ARGUMENT and b"light array" in lib.ilm_last_error()
    assert call(env=None) == abi.ERR_INVALID_ARGUMENT and call(dfu=None) == abi.ERR_INVALID_ARGUMENT
    for rows in ((-1, H), (0, H + 1), (9, 8)):
        assert call(rows=rows) == abi.ERR_OUT_OF_RANGE and b"rows" in lib.ilm_last_error()
    # no texture bound: lights are refused with a reason, zero lights are not
    native.set_projector_texture(ctx, None)
    assert call() == abi.ERR_INVALID_ARGUMENT and b"texture" in lib.ilm_last_error()
    assert call(lights_p=None, count=0) == abi.OK
    # the texture's own refusals
    t = np.ascontiguousarray(pc.texture(5, 3))
    p = t.ctypes.data_as(C.c_void_p)
    assert lib.ilm_ctx_set_projector_texture(lm.handle, p, 5, 3) == abi.ERR_INVALID_HANDLE
    assert lib.ilm_ctx_set_projector_texture(ctx.handle, p, -1, 3) == abi.ERR_INVALID_ARGUMENT
    assert lib.ilm_ctx_set_projector_texture(ctx.handle, p, 5, 0) == abi.ERR_INVALID_ARGUMENT
    assert lib.ilm_ctx_set_projector_texture(ctx.handle, None, 5, 3) == abi.ERR_INVALID_ARGUMENT
    assert call() == abi.ERR_INVALID_ARGUMENT                    # and none of them bound anything
    assert_bits_equal(lm.download(), before, "no refused call wrote a texel")
    # a 1 x 1 texture is a texture
    assert lib.ilm_ctx_set_projector_texture(ctx.handle, p, 1, 1) == abi.OK and call() == abi.OK
    assert (lm.download()[..., 3] > before[..., 3]).any()
    native.set_projector_texture(ctx, None)
    lm.close()


def test_the_ramp_binding_is_untouched_by_a_projector_call(scene_cache, ctx):
    """the same sphere-light frame with a ramp bound, before and after binding a projector texture and rendering a projector group:
    the same bits -- and the projector group is the same with and without the ramp"""
    s = scene_cache()
    spheres = (abi.LightVertex * 2)(scenes.sphere_light((12.0, 20.0, 9.0), 4.0, 30.0, color=(1.0, 0.9, 0.7, 1.0)),
                                    scenes.sphere_light((38.0, 6.0, 14.0), 3.0, 25.0, color=(0.3, 0.5, 1.0, 0.8)))

    def sphere_frame():
        lm = native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4)
        native.render_sphere_lights(ctx, spheres, s.env, s.dfu, s.gb, s.sdf, AMBIENT, lm)
        out = lm.download()
        lm.close()
        return out
    plain = sphere_frame()
    no_ramp, _ = s.got([clamped()], pc.texture(5, 3))
    ctx.set_light_ramp(dc.ramp_texture())
    try:
        ramped = sphere_frame()
        assert np.abs(ramped - plain).max() > 0.01
        with_ramp, _ = s.got([clamped()], pc.texture(5, 3))
        assert_bits_equal(with_ramp, no_ramp, "a projector group does not read the ramp")
        native.set_projector_texture(ctx, pc.texture(8, 8))
        native.set_projector_texture(ctx, None)
        assert_bits_equal(sphere_frame(), ramped, "the ramp binding after a projector call")
    finally:
        ctx.set_light_ramp(None)
    assert_bits_equal(sphere_frame(), plain, "the ramp unbound again")
