"""ilm_render_line_lights on the device against the float32 restatement of tests/line_common.py: every pixel within the suite's
criterion (tests.util.assert_close: 1e-4 relative with the lightmap floor), the three statistics exactly.

Frames of 44 x 27 pixels (3 x 2 workgroup tiles, 6 x 4 waves, partial ones at both rims) over directional_common's field of 48 x 32
texels per slice with a tall box and an ellipsoid, MaxStepCount 24.  Every shaded scene asserts what it must contain: pairs that trace,
pairs the opacity term discards, and pairs whose three rays end at different iterations.
"""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import line_common as lc
from tests.util import assert_bits_equal, assert_close

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = lc.WIDTH, lc.HEIGHT
AMBIENT = (0.0213, 0.0377, 0.0591, 1.0)


class Scene:
    """the device's resources and the oracle's textures of one (field format, G-buffer format) combination, with the decoded pixels"""

    def __init__(self, ctx, oracle, sfmt, gfmt, viewport=(0.0, 0.0)):
        self.ctx, self.oracle = ctx, oracle
        self.dfu = lc.field_uniforms() if sfmt is not None else lc.no_field_uniforms()
        self.sdf = self.otex = None
        if sfmt is not None:
            self.sdf = native.DistanceFieldTexture(ctx, lc.field_atlas(sfmt), sfmt)
            self.otex = oracle.make_texture(lc.field_atlas(sfmt), sfmt)
        self.gb = self.ogb = None
        if gfmt is not None:
            g = lc.gbuffer_texels() if gfmt == abi.GBUFFER_FLOAT4 else lc.gbuffer_texels().astype(np.float16).view(np.uint16)
            self.gb = native.GBufferTexture(ctx, g, gfmt)
            self.ogb = oracle.make_texture(g, gfmt)
            self.env = scenes.environment(gbuffer_size=(W, H), viewport_position=viewport)
        else:
            self.env = scenes.environment(viewport_position=viewport)
        self.pixels = lc.decode_pixels(oracle, self.env, self.ogb, W, H)
        self.fullbright = sum(1 for p in self.pixels if p[3])

    def want(self, lights, ambient=AMBIENT, dfu=None, **kw):
        return lc.render(self.oracle, lights, self.env, self.dfu if dfu is None else dfu, self.ogb, self.otex, ambient, W, H, pixels=self.pixels, **kw)

    def got(self, lights, ambient=AMBIENT, fmt=abi.LIGHTMAP_FLOAT4, before=None, rows=(0, None), want_stats=True, dfu=None):
        lm = native.Lightmap(self.ctx, W, H, fmt)
        if before is not None:
            lm.upload(before)
        stats = native.render_line_lights(self.ctx, lc.light_array(lights) if lights else None, self.env, self.dfu if dfu is None else dfu, self.gb,
                                          self.sdf, ambient, lm, rows[0], rows[1], want_stats=want_stats)
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

    def get(sfmt=abi.SDF_UNORM16, gfmt=abi.GBUFFER_FLOAT4, viewport=(0.0, 0.0)):
        key = (sfmt, gfmt, viewport)
        if key not in cache:
            cache[key] = Scene(ctx, oracle, sfmt, gfmt, viewport)
        return cache[key]
    yield get
    for s in cache.values():
        s.close()


def overhead(**kw):
    """a diagonal segment above the frame, past the box and the ellipsoid: shadows, AO, two colours"""
    args = dict(start=(6.0, 4.5, 20.0), end=(40.0, 22.0, 14.0), radius=2.0, start_color=(1.0, 0.8, 0.6, 0.9), end_color=(0.3, 0.5, 1.0, 0.7),
                ao_radius=5.0, ao_opacity=0.6)
    args.update(kw)
    return lc.line_light(**args)


def low(**kw):
    """a segment at z = 3, inside the G-buffer's relief (z = 0.5 .. 5.5): the pixels above it see it from behind -- opacity 0, discarded"""
    args = dict(start=(4.0, 20.0, 3.0), end=(26.0, 25.0, 3.0), radius=1.0, start_color=(0.2, 0.9, 0.4, 1.0), end_color=(0.9, 0.2, 0.4, 1.0))
    args.update(kw)
    return lc.line_light(**args)


def buried(**kw):
    """a segment below every shaded point: every pair is discarded by the opacity term"""
    args = dict(start=(5.0, 5.0, -6.0), end=(30.0, 20.0, -4.0), radius=2.0)
    args.update(kw)
    return lc.line_light(**args)


def scene_lights(s, **kw):
    return [overhead(**kw), low(**kw) if s.gb is not None else buried(**kw)]


def contents(want, lights):
    """(pairs that trace, pairs the shader discarded, traced pairs whose three rays ended at different iterations)"""
    pairs = want.stats[1]
    discarded = pairs - len(want.detail)
    apart = sum(1 for f in want.detail.values() if "ended" in f and len(set(f["ended"])) > 1)
    return want.stats[2], discarded, apart


def check(scene, lights, what, traces=True, discards=True, **kw):
    """The counting instantiation (line_lights_kernel<FMT, true>) gives the statistics and is held to the restatement; the
    instantiation every other caller runs (<FMT, false>: another code object) is rendered beside it and must give the same bits."""
    want = scene.want(lights, **kw)
    got, stats = scene.got(lights, dfu=kw.get("dfu"))
    traced, discarded, apart = contents(want, lights)
    if traces:
        assert traced > 50 and apart > 20, (what, traced, apart)
    if discards:
        assert discarded > 20, (what, discarded)
    assert stats == want.stats, (what, stats, want.stats)
    assert_close(got, want.image, what)
    plain, none = scene.got(lights, want_stats=False, dfu=kw.get("dfu"))
    assert none is None
    assert_close(plain, want.image, what + ", without statistics")
    assert_bits_equal(plain, got, what + ": the instantiation without statistics against the counting one")
    return got, want


@pytest.mark.parametrize("sfmt,gfmt", [(abi.SDF_UNORM16, None), (abi.SDF_FP16, None), (abi.SDF_UNORM16, abi.GBUFFER_FLOAT4),
                                       (abi.SDF_FP16, abi.GBUFFER_HALF4), (None, abi.GBUFFER_FLOAT4), (None, None)])
def test_shadowed_lights_over_fields_and_gbuffers(scene_cache, sfmt, gfmt):
    """both field formats and no field, both G-buffer formats and the ground plane"""
    s = scene_cache(sfmt, gfmt)
    got, want = check(s, scene_lights(s), "two lights, field %r, G-buffer %r" % (sfmt, gfmt), traces=sfmt is not None)
    samples, pairs, traced = want.stats
    assert pairs == 2 * (W * H - s.fullbright)
    if sfmt is None:
        assert samples == 0 and traced == 0
    else:
        assert samples > 3 * traced
        lit = [f["cone"] for f in want.detail.values() if "cone" in f]
        assert min(lit) < 0.05 and max(lit) == 1, "the frame has shadowed and unshadowed pixels"
    if gfmt is not None:
        assert s.fullbright == 20 and (got[12:14, 20:30, 3] == 1).all()                 # fullbright texels: discarded, no pair
        assert {1.0, 2.0, 3.0} == set(np.unique(got[..., 3]))                           # `low` lights only the pixels below it
        # rows 5 .. 7 have shadows disabled: lit, never traced
        assert all("cone" not in want.detail[(x, 6, 0)] for x in range(W))
    else:
        assert (got[..., 3] == 2).all()                                                 # `buried` lights nothing


SPECIAL = {
    "partly outside the frame": dict(start=(-20.0, 5.0, 15.0), end=(25.0, 15.0, 15.0), radius=2.0),
    "wholly outside the frame": dict(start=(60.0, -30.0, 25.0), end=(90.0, -10.0, 25.0), radius=3.0, start_color=(4.0, 3.0, 2.0, 1.0)),
    "vertical": dict(start=(30.0, 14.0, 4.0), end=(30.0, 14.0, 28.0), radius=1.5),
    "short": dict(start=(22.0, 20.0, 12.0), end=(23.0, 20.5, 12.0), radius=2.0),
    "radius above MaxCone": dict(start=(8.0, 24.0, 18.0), end=(36.0, 3.0, 18.0), radius=10.0),
    "ramp length in LightProperties.y": dict(start=(8.0, 24.0, 18.0), end=(36.0, 3.0, 18.0), radius=4.0, ramp_length=40.0),
}


@pytest.mark.parametrize("which", sorted(SPECIAL))
def test_special_segments(scene_cache, which):
    s = scene_cache()
    light = overhead(**SPECIAL[which])
    got, want = check(s, [light, low()], which)
    r = lc.prepare(light, s.dfu)
    if which == "short":
        assert r.offset == 1
    if which == "radius above MaxCone":
        assert r.max_radius == F32(8) and r.radius == 10
    if which == "ramp length in LightProperties.y":
        assert r.growth == F32(F32(4) / F32(40))
        other, _ = s.got([overhead(**dict(SPECIAL[which], ramp_length=0.0)), low()], want_stats=False)
        assert np.abs(other - got).max() > 1e-3, "the ramp length given is honoured"
    if which == "vertical":
        assert r.delta[0] == 0 and r.delta[1] == 0 and r.delta[2] == 24


def five_lights():
    return [overhead(**SPECIAL["partly outside the frame"]), overhead(**SPECIAL["wholly outside the frame"]), overhead(**SPECIAL["vertical"]),
            low(), overhead(**SPECIAL["radius above MaxCone"])]


def test_five_lights_in_list_order(scene_cache):
    s = scene_cache()
    got, want = check(s, five_lights(), "five lights")
    assert want.image[..., 3].max() == 6 and want.stats[1] == 5 * (W * H - s.fullbright)
    backwards, _ = s.got(five_lights()[::-1], want_stats=False)
    assert_close(backwards, want.image, "five lights, reversed")
    assert (backwards != got).any(), "the fp32 sum runs in list order: the reversed list rounds differently somewhere"


def test_pixels_that_are_not_visible_are_clipped(scene_cache):
    """a viewport position that puts the shaded x of columns 0 .. 21 at or below -9999, under a G-buffer with fullbright texels and
    texels without shadows: clip(), no rgb and no + 1 on alpha, no samples -- but a pair, since the opacity term was reached"""
    s = scene_cache(abi.SDF_UNORM16, abi.GBUFFER_FLOAT4, lc.INVISIBLE_VIEWPORT)
    light = overhead(start=(-10012.0, 4.5, 20.0), end=(-9985.0, 22.0, 14.0))
    got, want = check(s, [light], "invisible columns", traces=False)
    assert (got[:, :22, 3] == 1).all()
    visible = got[:, 22:, 3]
    assert (visible[12:14, :8] == 1).all() and (np.delete(visible, (12, 13), axis=0) == 2).all()
    assert want.stats[1] == W * H - s.fullbright and contents(want, [light])[1] >= 22 * H - s.fullbright


def exact_lights():
    """lights that do not trace, for the ground plane (whose normal involves no sin / cos of the G-buffer decode): every operation of
    their contribution is the defined arithmetic -- bit-equality with the restatement"""
    return [overhead(casts_shadows=False), buried(casts_shadows=False), overhead(casts_shadows=False, **SPECIAL["vertical"])]


@pytest.mark.parametrize("blend_fp16", [False, True])
def test_lightmap_formats_and_blend_models(scene_cache, ctx, blend_fp16):
    """the three formats' stores and both blend models; clear and accumulate onto uploaded contents.  Over the ground plane, lights that
    do not trace equal the restatement bit for bit in every format (AO included: the sampler is the oracle's); with traced lights the
    fp32 model meets the criterion and the fp16-per-light model the sphere tests' (one fp16 ulp where a contribution sits on a rounding
    boundary)."""
    s = scene_cache(abi.SDF_UNORM16, None)
    ctx.set_lightmap_blend(blend_fp16)
    try:
        want = s.want(exact_lights(), blend_fp16=blend_fp16)
        assert contents(want, None)[1] > 20
        before32 = scenes.uniform(77, (H, W, 4), 0.0, 1.0)
        for fmt in (abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8):
            got, stats = s.got(exact_lights(), fmt=fmt)
            assert stats == want.stats
            assert np.array_equal(got, lc.to_stored(want.image, fmt)), "clear, format %d" % fmt
            assert np.array_equal(s.got(exact_lights(), fmt=fmt, want_stats=False)[0], got), "clear without statistics, format %d" % fmt
            before = lc.to_stored(before32, fmt)
            want_acc = s.want(exact_lights(), ambient=None, before=lc.from_stored(before, fmt), blend_fp16=blend_fp16)
            got, _ = s.got(exact_lights(), ambient=None, fmt=fmt, before=before, want_stats=False)
            assert np.array_equal(got, lc.to_stored(want_acc.image, fmt)), "accumulate, format %d" % fmt
        shaded = scene_lights(s)
        want = s.want(shaded, blend_fp16=blend_fp16)
        assert contents(want, shaded)[0] > 50
        got32, stats = s.got(shaded)
        assert stats == want.stats
        if blend_fp16:
            assert np.array_equal(want.image, lc.half(want.image))
            diff = np.abs(got32 - want.image)
            assert (diff <= np.abs(want.image) * 2.0 ** -10 + 1e-7).all()
            assert (diff > 0).mean() < 0.02
        else:
            assert_close(got32, want.image, "shaded lights, fp32 accumulate")
        for fmt in (abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8):
            got, _ = s.got(shaded, fmt=fmt, want_stats=False)           # (the instantiation without statistics)
            assert np.array_equal(got, lc.to_stored(got32, fmt))
    finally:
        ctx.set_lightmap_blend(False)


def test_clear_with_any_light_count_and_accumulate(scene_cache):
    s = scene_cache(None, None)
    got, stats = s.got([], ambient=AMBIENT)
    assert np.array_equal(got, np.broadcast_to(np.asarray(AMBIENT, np.float32), (H, W, 4))) and stats == (0, 0, 0)
    before = scenes.uniform(5, (H, W, 4), 0.0, 2.0)
    got, _ = s.got([], ambient=None, before=before)
    assert_bits_equal(got, before, "zero lights, accumulate: nothing changes")
    lights = scene_lights(s)
    want = s.want(lights, ambient=None, before=before)
    got, stats = s.got(lights, ambient=None, before=before)
    assert stats == want.stats
    assert_close(got, want.image, "accumulate onto a prefilled lightmap")


def test_a_strip_that_cuts_wave_tiles_leaves_the_other_rows_alone(scene_cache):
    s = scene_cache()
    lights = scene_lights(s)
    before = scenes.uniform(9, (H, W, 4), 0.0, 1.0)
    full, _ = s.got(lights)
    for ambient in (AMBIENT, None):
        want = s.want(lights, ambient=ambient, before=before, row_begin=5, row_end=19)
        got, stats = s.got(lights, ambient=ambient, before=before, rows=(5, 19))
        assert stats == want.stats and stats[1] == 2 * (14 * W - s.fullbright) and stats[2] > 50
        assert_bits_equal(got[:5], before[:5], "rows above the strip")
        assert_bits_equal(got[19:], before[19:], "rows below the strip")
        assert_close(got, want.image, "strip [5, 19)")
        assert_bits_equal(s.got(lights, ambient=ambient, before=before, rows=(5, 19), want_stats=False)[0], got, "strip [5, 19) without statistics")
        if ambient is not None:
            assert_bits_equal(got[5:19], full[5:19], "a strip computes what the whole frame computes")
    got, stats = s.got(lights, ambient=None, before=before, rows=(7, 7))
    assert_bits_equal(got, before, "empty strip")
    assert stats == (0, 0, 0)


def degenerate():
    nan = float("nan")
    return [overhead(radius=0.0), overhead(start=(20.0, 10.0, 9.0), end=(20.0, 10.0, 9.0)), overhead(start=(nan, 4.5, 20.0)),
            overhead(end=(40.0, 22.0, nan)), overhead(start=(nan, nan, nan), end=(nan, nan, nan), radius=nan)]


@pytest.mark.parametrize("gfmt", [None, abi.GBUFFER_FLOAT4])
def test_degenerate_lights_beside_a_good_one_change_nothing(scene_cache, gfmt):
    """Radius 0, start == end and NaN positions in one list with a good light between them: the frame is the good light's alone, bit
    for bit; the samples and traced pairs are the good light's, the pairs count every light."""
    s = scene_cache(abi.SDF_UNORM16, gfmt)
    bad = degenerate()
    good = overhead()
    alone, alone_stats = s.got([good])
    mixed, stats = s.got(bad[:3] + [good] + bad[3:])
    assert_bits_equal(mixed, alone, "degenerate lights around a good one")
    assert stats[0] == alone_stats[0] and stats[2] == alone_stats[2] and stats[1] == (len(bad) + 1) * alone_stats[1]
    plain, _ = s.got(bad[:3] + [good] + bad[3:], want_stats=False)
    assert_bits_equal(plain, alone, "degenerate lights around a good one, without statistics")
    only_bad, stats = s.got(bad)
    assert np.array_equal(only_bad, np.broadcast_to(np.asarray(AMBIENT, np.float32), (H, W, 4))) and stats == (0, len(bad) * alone_stats[1], 0)
    # and the restatement agrees on what they are
    want = s.want(bad)
    assert want.detail == {} and want.stats == stats


def test_pixels_on_the_segments_axis_are_discarded(scene_cache):
    """a segment in the ground plane along x at y = 13: the pixels of row 13 lie on its axis -- beyond its ends forward = +-left, between
    them the closest point is (nearly) the pixel itself, up = cross(left, forward) = 0 either way -- and are discarded; the other rows
    see the rectangle standing on the ground and are lit and traced"""
    s = scene_cache(abi.SDF_UNORM16, None)
    in_plane = overhead(start=(10.0, 13.0, 0.0), end=(30.0, 13.0, 0.0))
    got, want = check(s, [in_plane, overhead()], "a segment in the ground plane")
    assert all((x, 13, 0) not in want.detail and (x, 13, 1) in want.detail for x in range(W))
    assert (got[13, :, 3] == 2).all() and (got[12, :, 3] == 3).all() and (got[14, :, 3] == 3).all()


def test_a_bound_light_ramp_changes_nothing(scene_cache, ctx):
    s = scene_cache()
    lights = scene_lights(s)
    plain, plain_stats = s.got(lights)
    ctx.set_light_ramp(lc.ramp_texture())
    try:
        ramped, ramped_stats = s.got(lights)
    finally:
        ctx.set_light_ramp(None)
    assert_bits_equal(ramped, plain, "the reference has no LineLightWithRamp")
    assert ramped_stats == plain_stats and plain_stats[2] > 50


def test_refusals(scene_cache, ctx):
    s = scene_cache()
    lib = native.lib()
    lm = native.Lightmap(ctx, W, H)
    lights = lc.light_array([overhead()])

    def call(ctx_h=None, lights_p=C.cast(lights, C.c_void_p), count=1, gb=None, sdf=None, lm_h=None, rows=(0, H), env=s.env, dfu=s.dfu):
        return lib.ilm_render_line_lights(ctx.handle if ctx_h is None else ctx_h, lights_p, count, C.byref(env) if env is not None else None,
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
    assert_bits_equal(lm.download(), before, "no refused call wrote a texel")
    lm.close()
