"""ilm_render_volumetric_lights on the device against the float32 restatement of tests/volumetric_common.py: every pixel within the
suite's criterion (tests.util.assert_close: 1e-4 relative with the lightmap floor), the three statistics exactly.

Frames of 44 x 27 pixels (3 x 2 workgroup tiles, 6 x 4 waves, partial ones at both rims) over directional_common's field of 48 x 32
texels per slice with a tall box and an ellipsoid, MaxStepCount 8 (a pair walks nine column points of up to eight samples each).  Every
shaded scene asserts what it must contain; tests/test_volumetric_kat.py asserts the same conditions on the restatement alone.
"""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import volumetric_common as vc
from tests import volumetric_scenes as vs
from tests.util import assert_bits_equal, assert_close

pytestmark = pytest.mark.gpu

W, H = vc.WIDTH, vc.HEIGHT
AMBIENT = vs.AMBIENT


class Scene:
    """the device's resources and the oracle's textures of one (field format, G-buffer format) combination, with the decoded pixels"""

    def __init__(self, ctx, oracle, sfmt, gfmt, viewport=(0.0, 0.0), env_kw=None):
        self.ctx, self.oracle = ctx, oracle
        self.dfu = vc.field_uniforms() if sfmt is not None else vc.no_field_uniforms()
        self.sdf = self.otex = None
        if sfmt is not None:
            self.sdf = native.DistanceFieldTexture(ctx, vc.field_atlas(sfmt), sfmt)
            self.otex = oracle.make_texture(vc.field_atlas(sfmt), sfmt)
        self.gb = self.ogb = None
        env_kw = dict(env_kw or {})
        if gfmt is not None:
            g = vc.gbuffer_texels() if gfmt == abi.GBUFFER_FLOAT4 else vc.gbuffer_texels().astype(np.float16).view(np.uint16)
            self.gb = native.GBufferTexture(ctx, g, gfmt)
            self.ogb = oracle.make_texture(g, gfmt)
            self.env = scenes.environment(gbuffer_size=(W, H), viewport_position=viewport, **env_kw)
        else:
            self.env = scenes.environment(viewport_position=viewport, **env_kw)
        self.pixels = vc.decode_pixels(oracle, self.env, self.ogb, W, H)
        self.fullbright = sum(1 for p in self.pixels if p[3])

    def want(self, lights, ambient=AMBIENT, dfu=None, **kw):
        return vc.render(self.oracle, lights, self.env, self.dfu if dfu is None else dfu, self.ogb, self.otex, ambient, W, H, pixels=self.pixels, **kw)

    def got(self, lights, ambient=AMBIENT, fmt=abi.LIGHTMAP_FLOAT4, before=None, rows=(0, None), want_stats=True, dfu=None):
        lm = native.Lightmap(self.ctx, W, H, fmt)
        if before is not None:
            lm.upload(before)
        stats = native.render_volumetric_lights(self.ctx, vc.light_array(lights) if lights else None, self.env, self.dfu if dfu is None else dfu,
                                                self.gb, self.sdf, ambient, lm, rows[0], rows[1], want_stats=want_stats)
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

    def get(sfmt=abi.SDF_UNORM16, gfmt=abi.GBUFFER_FLOAT4, viewport=(0.0, 0.0), env_kw=()):
        key = (sfmt, gfmt, viewport, tuple(env_kw))
        if key not in cache:
            cache[key] = Scene(ctx, oracle, sfmt, gfmt, viewport, dict(env_kw))
        return cache[key]
    yield get
    for s in cache.values():
        s.close()


def check(scene, lights, what, **kw):
    """The counting instantiation (volumetric_lights_kernel<FMT, true>) gives the statistics and is held to the restatement; the
    instantiation every other caller runs (<FMT, false>: another code object) is rendered beside it and must give the same bits."""
    want = scene.want(lights, **kw)
    got, stats = scene.got(lights, dfu=kw.get("dfu"))
    assert stats == want.stats, (what, stats, want.stats)
    assert_close(got, want.image, what)
    plain, none = scene.got(lights, want_stats=False, dfu=kw.get("dfu"))
    assert none is None
    assert_bits_equal(plain, got, what + ": the instantiation without statistics against the counting one")
    return got, want


@pytest.mark.parametrize("sfmt,gfmt", vs.FORMAT_PAIRS)
def test_three_shapes_over_fields_and_gbuffers(scene_cache, sfmt, gfmt):
    """both field formats and no field, both G-buffer formats and the ground plane: a cone that projects from its origin, an ellipsoid
    with a light direction and a box that casts no shadow"""
    s = scene_cache(sfmt, gfmt)
    got, want = check(s, vs.three_shapes(), "three shapes, field %r, G-buffer %r" % (sfmt, gfmt))
    vs.assert_three_shapes(want, sfmt is not None, gfmt is not None)
    if gfmt is not None:
        assert s.fullbright == 20 and (got[12:14, 20:30, 3] == 1).all()                 # fullbright texels: discarded


@pytest.mark.parametrize("which", sorted(vs.SPECIAL))
def test_special_lights(scene_cache, which):
    s = scene_cache()
    lights = vs.special(which)
    got, want = check(s, lights, which)
    vs.SPECIAL[which][1](want)


@pytest.mark.parametrize("steps", vs.STEP_COUNTS)
def test_step_counts(scene_cache, steps):
    """MaxStepCount 1, a fractional one (the march counts (int)steps, the column divides by steps) and 4096 under a light of four pixels"""
    s = scene_cache()
    dfu = vc.field_uniforms(step_limit=steps)
    lights = vs.step_count_lights(steps)
    got, want = check(s, lights, "MaxStepCount %r" % steps, dfu=dfu)
    vs.assert_step_counts(want, steps)


def test_five_lights_in_list_order(scene_cache):
    s = scene_cache()
    lights = vs.five_lights()
    got, want = check(s, lights, "five lights")
    vs.assert_five_lights(want)
    backwards, _ = s.got(lights[::-1], want_stats=False)
    assert_close(backwards, want.image, "five lights, reversed")
    assert (backwards != got).any(), "the fp32 sum runs in list order: the reversed list rounds differently somewhere"


def test_pixels_that_are_not_visible_are_discarded(scene_cache):
    """a viewport position that puts the shaded x of columns 0 .. 21 at or below -9999: the core returns 0 -- no rgb, no + 1 on alpha, no
    samples, but a pair, since the pixel lies in the footprint"""
    s = scene_cache(abi.SDF_UNORM16, abi.GBUFFER_FLOAT4, vc.INVISIBLE_VIEWPORT)
    got, want = check(s, vs.invisible_lights(), "invisible columns")
    assert (got[:, :22, 3] == 1).all() and (got[:, 22:, 3] == 2).sum() > 100
    assert want.stats[1] == W * H and all(x >= 22 for (x, _y, _i) in want.detail)


def test_the_loop_guard_ends_a_column_that_makes_no_progress(scene_cache):
    """GroundZ = MaximumZ = 2^40 under a box that reaches above it: step = 1 / 8 is below an ulp of z, z -= step changes nothing, and the
    integer guard ends the column after (int)MaxStepCount + 4 bodies"""
    s = scene_cache(abi.SDF_UNORM16, None, (0.0, 0.0), vs.STUCK_ENVIRONMENT)
    got, want = check(s, vs.stuck_lights(), "a column that makes no progress")
    vs.assert_stuck(want)


@pytest.mark.parametrize("blend_fp16", [False, True])
def test_lightmap_formats_and_blend_models(scene_cache, ctx, blend_fp16):
    """the three formats' stores and both blend models; clear and accumulate onto uploaded contents.  Lights whose RampPower is 0 (pow(x,
    0) = 1 exactly) above the shaded points (no contact term) involve no pow: over the ground plane they equal the restatement bit for bit
    in every format, marches included (the sampler is the oracle's)."""
    s = scene_cache(abi.SDF_UNORM16, None)
    ctx.set_lightmap_blend(blend_fp16)
    try:
        lights = vs.exact_lights()
        want = s.want(lights, blend_fp16=blend_fp16)
        vs.assert_exact_lights(want)
        before32 = scenes.uniform(77, (H, W, 4), 0.0, 1.0)
        for fmt in (abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8):
            got, stats = s.got(lights, fmt=fmt)
            assert stats == want.stats
            assert np.array_equal(got, vc.to_stored(want.image, fmt)), "clear, format %d" % fmt
            assert np.array_equal(s.got(lights, fmt=fmt, want_stats=False)[0], got), "clear without statistics, format %d" % fmt
            before = vc.to_stored(before32, fmt)
            want_acc = s.want(lights, ambient=None, before=vc.from_stored(before, fmt), blend_fp16=blend_fp16)
            got, _ = s.got(lights, ambient=None, fmt=fmt, before=before, want_stats=False)
            assert np.array_equal(got, vc.to_stored(want_acc.image, fmt)), "accumulate, format %d" % fmt
        shaded = vs.three_shapes()
        want = s.want(shaded, blend_fp16=blend_fp16)
        got32, stats = s.got(shaded)
        assert stats == want.stats
        if blend_fp16:
            assert np.array_equal(want.image, vc.half(want.image))
            diff = np.abs(got32 - want.image)
            assert (diff <= np.abs(want.image) * 2.0 ** -10 + 1e-7).all()
            assert (diff > 0).mean() < 0.02
        else:
            assert_close(got32, want.image, "three shapes, fp32 accumulate")
        for fmt in (abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8):
            got, _ = s.got(shaded, fmt=fmt, want_stats=False)
            assert np.array_equal(got, vc.to_stored(got32, fmt))
    finally:
        ctx.set_lightmap_blend(False)


def test_clear_with_any_light_count_and_accumulate(scene_cache):
    s = scene_cache(None, None)
    got, stats = s.got([], ambient=AMBIENT)
    assert np.array_equal(got, np.broadcast_to(np.asarray(AMBIENT, np.float32), (H, W, 4))) and stats == (0, 0, 0)
    before = scenes.uniform(5, (H, W, 4), 0.0, 2.0)
    got, _ = s.got([], ambient=None, before=before)
    assert_bits_equal(got, before, "zero lights, accumulate: nothing changes")
    lights = vs.three_shapes()
    want = s.want(lights, ambient=None, before=before)
    got, stats = s.got(lights, ambient=None, before=before)
    assert stats == want.stats
    assert_close(got, want.image, "accumulate onto a prefilled lightmap")


def test_a_strip_that_cuts_wave_tiles_leaves_the_other_rows_alone(scene_cache):
    s = scene_cache()
    lights = vs.three_shapes()
    before = scenes.uniform(9, (H, W, 4), 0.0, 1.0)
    full, _ = s.got(lights)
    for ambient in (AMBIENT, None):
        want = s.want(lights, ambient=ambient, before=before, row_begin=5, row_end=19)
        got, stats = s.got(lights, ambient=ambient, before=before, rows=(5, 19))
        assert stats == want.stats and stats[2] > 50
        assert all(5 <= y < 19 for (_x, y, _i) in want.detail)
        assert_bits_equal(got[:5], before[:5], "rows above the strip")
        assert_bits_equal(got[19:], before[19:], "rows below the strip")
        assert_close(got, want.image, "strip [5, 19)")
        assert_bits_equal(s.got(lights, ambient=ambient, before=before, rows=(5, 19), want_stats=False)[0], got, "strip [5, 19) without statistics")
        if ambient is not None:
            assert_bits_equal(got[5:19], full[5:19], "a strip computes what the whole frame computes")
    got, stats = s.got(lights, ambient=None, before=before, rows=(7, 7))
    assert_bits_equal(got, before, "empty strip")
    assert stats == (0, 0, 0)


@pytest.mark.parametrize("gfmt", [None, abi.GBUFFER_FLOAT4])
def test_degenerate_lights_beside_a_good_one(scene_cache, gfmt):
    """zero radii, a zero-length cone, RampLength 0, Volumetricity 0 and NaN positions in one list with a good light between them: held
    to the restatement like any other list, and a list of those that light nothing leaves the clear colour"""
    s = scene_cache(abi.SDF_UNORM16, gfmt)
    lights = vs.degenerate_lights()
    got, want = check(s, lights[:4] + [vs.three_shapes()[0]] + lights[4:], "degenerate lights around a good one")
    dark = vs.dark_degenerate_lights()
    got, want = check(s, dark, "degenerate lights that light nothing")
    assert np.array_equal(got, np.broadcast_to(np.asarray(AMBIENT, np.float32), (H, W, 4)))
    vs.assert_dark(want)


def test_bound_ramp_and_projector_texture_change_nothing(scene_cache, ctx):
    s = scene_cache()
    lights = vs.three_shapes()
    plain, plain_stats = s.got(lights)
    ctx.set_light_ramp(vc.ramp_texture())
    native.set_projector_texture(ctx, vc.ramp_texture())
    try:
        bound, bound_stats = s.got(lights)
    finally:
        ctx.set_light_ramp(None)
        native.set_projector_texture(ctx, None)
    assert_bits_equal(bound, plain, "neither binding is read")
    assert bound_stats == plain_stats and plain_stats[2] > 50


def test_refusals(scene_cache, ctx):
    s = scene_cache()
    lib = native.lib()
    lm = native.Lightmap(ctx, W, H)
    good = vs.three_shapes()

    def call(ctx_h=None, lights=good, lights_p=0, count=None, gb=None, sdf=None, lm_h=None, rows=(0, H), env=s.env, dfu=s.dfu):
        arr = vc.light_array(lights)
        return lib.ilm_render_volumetric_lights(ctx.handle if ctx_h is None else ctx_h, C.cast(arr, C.c_void_p) if lights_p == 0 else lights_p,
                                                len(lights) if count is None else count, C.byref(env) if env is not None else None,
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
    for shape in (3.0, -1.0, 0.5, 1.0000001, float("nan"), float("inf")):
        bad = vs.three_shapes()
        bad[1].EvenMoreLightProperties.w = shape
        assert call(lights=bad) == abi.ERR_INVALID_ARGUMENT and b"shape" in lib.ilm_last_error(), shape
    for steps in (0.0, 0.99, -3.0, 4096.5, float("nan"), float("inf")):
        assert call(dfu=vc.field_uniforms(step_limit=steps)) == abi.ERR_INVALID_ARGUMENT and b"MaxStepCount" in lib.ilm_last_error(), steps
    assert_bits_equal(lm.download(), before, "no refused call wrote a texel")
    lm.close()
