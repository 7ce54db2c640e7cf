"""ilm_resolve_lighting_scaled on the device.  The fetch is checked against its numpy statement (tests/resolve_scaled_common.py), bit for
bit where the definition allows it (scale 1 against the 1:1 entry points, integer POINT magnification, tap selection); the filtered frame
against oracle.resolve_lighting over the arrays that statement samples, at the criteria of tests/test_output_gpu.py (assert_close's
default, +-1 byte and the exact band for RGBA8).  Shapes: 37 x 29, 19 x 13, 23 x 17 and 1 x 1 -- odd, no multiple of the wave, rows of
both parities, a magnification, a minification and a single texel."""
import numpy as np
import pytest

from illuminant_amd import abi, native
from tests import output_common as oc
from tests import resolve_scaled_common as rs
from tests.util import assert_close

pytestmark = pytest.mark.gpu

F4, H4, C8 = abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8
_DTYPE = {F4: np.float32, H4: np.float16, C8: np.uint8}
FILTER_NAME = {rs.POINT: "point", rs.LINEAR: "linear"}
SHAPES = (((19, 13), (37, 29)), ((37, 29), (19, 13)), ((1, 1), (5, 3)))          # (source, destination) as (width, height)
SHAPE_IDS = ["19x13_to_37x29", "37x29_to_19x13", "1x1_to_5x3"]


def _random(fmt, size, seed, hi=3.0):
    """Independent finite texels of a (width, height) texture in the format's element type: [0, hi) or bytes."""
    w, h = size
    rng = np.random.default_rng(seed)
    if fmt == C8:
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return rng.uniform(0.0, hi, (h, w, 4)).astype(_DTYPE[fmt])


def _texture(ctx, texels, fmt):
    t = native.Lightmap(ctx, texels.shape[1], texels.shape[0], fmt)
    t.upload(texels)
    return t


def _sentinel(fmt, size):
    return np.full((size[1], size[0], 4), oc.SENTINEL[fmt])


def _filled(ctx, fmt, size):
    dst = native.Lightmap(ctx, size[0], size[1], fmt)
    dst.upload(_sentinel(fmt, size))
    return dst


def _close(*textures):
    for t in textures:
        if t is not None:
            t.close()


def _written(out, fmt):
    """(height, width) bool: the texels that no longer hold the sentinel (alpha is 1 or an albedo's, never the sentinel's)."""
    return (out != oc.SENTINEL[fmt]).any(axis=-1)


# ---- scale 1: the bits of the 1:1 entry points ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", (rs.POINT, rs.LINEAR), ids=lambda f: FILTER_NAME[f])
@pytest.mark.parametrize("with_albedo", (False, True), ids=("plain", "albedo"))
@pytest.mark.parametrize("dst_fmt", (F4, C8), ids=lambda f: "to_" + oc.FORMAT_NAME[f])
@pytest.mark.parametrize("src_fmt", oc.FORMATS, ids=lambda f: oc.FORMAT_NAME[f])
def test_scale_one_is_bit_equal_to_the_one_to_one_resolve(ctx, src_fmt, dst_fmt, with_albedo, filt):
    """The whole-target quad on a 37 x 29 frame: the coordinate is px + 0.5 exactly, LINEAR's second taps weigh 0, and every mode gives
    the bytes of ilm_resolve_lighting[_with_albedo]; on rows [5, 18) the rows outside keep theirs."""
    size = (oc.W, oc.H)
    albedo_fmt = oc.edge_albedo_format(src_fmt)
    src = _texture(ctx, oc.random_source(src_fmt), src_fmt)
    tex = _texture(ctx, oc.random_albedo(albedo_fmt), albedo_fmt) if with_albedo else None
    one, dst = native.Lightmap(ctx, oc.W, oc.H, dst_fmt), _filled(ctx, dst_fmt, size)
    for mode in oc.MODES:
        hdr = oc.matrix_hdr(mode)
        native.resolve_lighting(src, one, hdr, albedo=tex)
        want = one.download()
        dst.upload(_sentinel(dst_fmt, size))
        native.resolve_lighting_scaled(src, dst, hdr, (0, 0, oc.W, oc.H), albedo=tex, lightmap_filter=filt, albedo_filter=filt)
        assert dst.download().tobytes() == want.tobytes(), "whole frame, %s" % oc.MODE_NAME[mode]
        dst.upload(_sentinel(dst_fmt, size))
        native.resolve_lighting_scaled(src, dst, hdr, (0, 0, oc.W, oc.H), albedo=tex, lightmap_filter=filt, albedo_filter=filt, row_begin=5, row_end=18)
        part = dst.download()
        assert part[5:18].tobytes() == want[5:18].tobytes(), "rows [5, 18), %s" % oc.MODE_NAME[mode]
        fill = _sentinel(dst_fmt, size)
        assert np.array_equal(part[:5], fill[:5]) and np.array_equal(part[18:], fill[18:]), "rows outside [5, 18) were written"
    _close(src, tex, one, dst)


@pytest.mark.parametrize("with_albedo", (False, True), ids=("plain", "albedo"))
@pytest.mark.parametrize("src_fmt,dst_fmt,albedo_fmt", [(H4, C8, C8), (F4, F4, F4)], ids=["half4_to_rgba8", "float4_to_float4"])
def test_point_magnification_by_two_repeats_the_resolved_texel(ctx, src_fmt, dst_fmt, albedo_fmt, with_albedo):
    """19 x 13 -> 38 x 26, POINT: destination texel (x, y) holds the bits of the 1:1 resolve of source texel (x // 2, y // 2)."""
    small, big = (19, 13), (38, 26)
    src = _texture(ctx, _random(src_fmt, small, 31), src_fmt)
    tex = _texture(ctx, _random(albedo_fmt, small, 32, 1.5), albedo_fmt) if with_albedo else None
    one, dst = native.Lightmap(ctx, small[0], small[1], dst_fmt), _filled(ctx, dst_fmt, big)
    for mode in oc.MODES:
        hdr = oc.matrix_hdr(mode)
        native.resolve_lighting(src, one, hdr, albedo=tex)
        native.resolve_lighting_scaled(src, dst, hdr, (0, 0, big[0], big[1]), albedo=tex, lightmap_filter=rs.POINT, albedo_filter=rs.POINT)
        want = one.download()[(np.arange(big[1]) // 2)[:, None], (np.arange(big[0]) // 2)[None, :]]
        assert dst.download().tobytes() == np.ascontiguousarray(want).tobytes(), oc.MODE_NAME[mode]
    _close(src, tex, one, dst)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_point_fetch_picks_the_texel_the_definition_names(ctx, shape):
    """A float source whose red channel is the texel's linear index, plain mode at exposure and gamma 1: rint(red) of every destination
    pixel is the index the numpy statement picks."""
    (sw, sh), dsize = shape
    texels = np.zeros((sh, sw, 4), np.float32)
    texels[..., 0] = np.arange(sw * sh, dtype=np.float32).reshape(sh, sw)
    assert sw * sh < 4096
    src, dst = _texture(ctx, texels, F4), _filled(ctx, F4, dsize)
    native.resolve_lighting_scaled(src, dst, oc.hdr_configuration(), (0, 0, dsize[0], dsize[1]), lightmap_filter=rs.POINT)
    got = np.rint(dst.download()[..., 0]).astype(np.int64)
    want = rs.point_index(texels.shape, dsize, (0, 0, dsize[0], dsize[1]))
    assert np.array_equal(got, want), np.argwhere(got != want)[:6].tolist()
    _close(src, dst)


# ---- the filtered frame against the oracle ---------------------------------------------------------------------------------------------
def _expected(oracle, light, albedo, dsize, quad, hdr, lightmap_region=None, albedo_region=None, offset=None, filt=rs.LINEAR):
    sampled_light = rs.sample(light, dsize, quad, lightmap_region, filt, offset)
    sampled_albedo = rs.sample(albedo, dsize, quad, albedo_region, filt) if albedo is not None else None
    return oracle.resolve_lighting(np.ascontiguousarray(sampled_light), hdr, albedo=sampled_albedo)


@pytest.mark.parametrize("mode", oc.MODES, ids=lambda m: oc.MODE_NAME[m])
@pytest.mark.parametrize("with_albedo", (False, True), ids=("plain", "albedo"))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_linear_resolve_matches_the_oracle_over_the_sampled_arrays(ctx, oracle, shape, with_albedo, mode):
    """A HALF4 lightmap and an RGBA8 albedo of a third size (23 x 17), both LINEAR, into a float and a Color destination."""
    ssize, dsize = shape
    quad = (0, 0, dsize[0], dsize[1])
    light_t, albedo_t = _random(H4, ssize, 41), _random(C8, (23, 17), 42)
    src = _texture(ctx, light_t, H4)
    tex = _texture(ctx, albedo_t, C8) if with_albedo else None
    hdr = oc.matrix_hdr(mode)
    want = _expected(oracle, oc.decode(light_t, H4), oc.decode(albedo_t, C8) if with_albedo else None, dsize, quad, hdr)
    what = "%s %s %s" % (SHAPE_IDS[SHAPES.index(shape)], "albedo" if with_albedo else "plain", oc.MODE_NAME[mode])
    for dst_fmt in (F4, C8):
        dst = _filled(ctx, dst_fmt, dsize)
        native.resolve_lighting_scaled(src, dst, hdr, quad, albedo=tex)
        oc.check_destination(dst.download(), want, dst_fmt, what + " -> " + oc.FORMAT_NAME[dst_fmt])
        dst.close()
    _close(src, tex)


@pytest.mark.parametrize("region", [(0, 0, 19, 13), (3, 2, 19, 13)], ids=["from_the_origin", "from_3_2"])
def test_a_region_smaller_than_the_texture_bleeds_its_far_neighbours(ctx, oracle, region):
    """A 24 x 16 source read over a 19 x 13 (or 16 x 11) region, magnified to 37 x 29: the coordinate is clamped to the region, the taps
    to the texture, so the last pixels blend column 19 and row 13 in -- the statement says so, and the device agrees with it."""
    ssize, dsize = (24, 16), (37, 29)
    quad = (0, 0, dsize[0], dsize[1])
    light = _random(F4, ssize, 51)
    (x0, x1, fx), (y0, y1, fy) = rs.axes(light.shape, dsize, quad, region, rs.LINEAR)
    assert ((x1 == 19) & (fx > 0)).any() and ((y1 == 13) & (fy > 0)).any() and x1.max() == 19 and y1.max() == 13       # the bleed is in the test
    assert x0.min() == max(region[0] - 1, 0) and y0.min() == max(region[1] - 1, 0)
    src, dst = _texture(ctx, light, F4), _filled(ctx, F4, dsize)
    for mode in (abi.HDR_NONE, abi.HDR_TONE_MAP):
        hdr = oc.matrix_hdr(mode)
        native.resolve_lighting_scaled(src, dst, hdr, quad, lightmap_region=region)
        oc.check_destination(dst.download(), _expected(oracle, light, None, dsize, quad, hdr, lightmap_region=region), F4,
                             "region %s, %s" % (region, oc.MODE_NAME[mode]))
    _close(src, dst)


QUADS = [(-7.5, 4.25, 30.0, 20.0), (21.25, 17.5, 40.0, 33.0), (37.5, -12.0, 10.0, 60.0)]


@pytest.mark.parametrize("dst_fmt", (F4, C8), ids=lambda f: "to_" + oc.FORMAT_NAME[f])
@pytest.mark.parametrize("quad", QUADS, ids=["off_the_left", "off_the_bottom_right", "outside"])
def test_a_quad_writes_the_pixels_whose_centre_it_contains_and_no_other(ctx, oracle, quad, dst_fmt):
    """A 37 x 29 target filled with a sentinel under a quad that covers part of it, hangs off it, or misses it: the covered set is the
    statement's, covered pixels match the oracle, every other texel keeps its bits.  Again on rows [6, 23)."""
    ssize, dsize = (19, 13), (37, 29)
    light_t, albedo_t = _random(H4, ssize, 61), _random(C8, (23, 17), 62)
    src, tex = _texture(ctx, light_t, H4), _texture(ctx, albedo_t, C8)
    hdr = oc.matrix_hdr(abi.HDR_TONE_MAP)
    want = _expected(oracle, oc.decode(light_t, H4), oc.decode(albedo_t, C8), dsize, quad, hdr)
    dst = _filled(ctx, dst_fmt, dsize)
    fill = _sentinel(dst_fmt, dsize)
    for rows in ((0, None), (6, 23)):
        covered = rs.coverage(dsize, quad, *rows)
        assert covered.any() == (quad is not QUADS[2])
        dst.upload(fill)
        native.resolve_lighting_scaled(src, dst, hdr, quad, albedo=tex, row_begin=rows[0], row_end=rows[1])
        out = dst.download()
        assert np.array_equal(out[~covered], fill[~covered]), "a texel outside the quad was written"
        assert np.array_equal(_written(out, dst_fmt), covered), "the covered set differs from the definition's"
        if covered.any():
            oc.check_destination(out[covered], want[covered], dst_fmt, "quad %s rows %s" % (quad, rows))
    _close(src, tex, dst)


@pytest.mark.parametrize("offset", [(0.5, -0.25), (1e9, -1e9), (float("nan"), float("inf"))], ids=["half_a_texel", "huge", "nan_inf"])
@pytest.mark.parametrize("filt", (rs.POINT, rs.LINEAR), ids=lambda f: FILTER_NAME[f])
def test_uv_offsets_move_the_lightmap_fetch_and_are_clamped_to_the_region(ctx, oracle, offset, filt):
    """LightmapUVOffset of any value is valid input: the coordinate is clamped to the region (a NaN becomes its near bound) and every
    index is clamped by integer arithmetic.  The albedo's fetch does not move."""
    ssize, dsize = (19, 13), (37, 29)
    quad = (0, 0, dsize[0], dsize[1])
    light, albedo_t = _random(F4, ssize, 71), _random(C8, (23, 17), 72)
    src, tex, dst = _texture(ctx, light, F4), _texture(ctx, albedo_t, C8), _filled(ctx, F4, dsize)
    hdr = oc.matrix_hdr(abi.HDR_NONE)
    native.resolve_lighting_scaled(src, dst, hdr, quad, albedo=tex, uv_offset=offset, lightmap_filter=filt, albedo_filter=filt)
    want = _expected(oracle, light, oc.decode(albedo_t, C8), dsize, quad, hdr, offset=offset, filt=filt)
    oc.check_destination(dst.download(), want, F4, "uv_offset %s %s" % (offset, FILTER_NAME[filt]))
    _close(src, tex, dst)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_destination_untouched(ctx):
    size = (12, 9)
    src, tex, dst = native.Lightmap(ctx, 8, 6, H4), native.Lightmap(ctx, 10, 7, C8), _filled(ctx, F4, size)
    fill = _sentinel(F4, size)
    ok = dict(quad=(0, 0, 12, 9))

    def refused(code, words=None, **changes):
        a = dict(ok, hdr=oc.hdr_configuration())
        a.update(changes)
        with pytest.raises(native.IlluminantError) as e:
            native.resolve_lighting_scaled(a.pop("src", src), a.pop("dst", dst), a.pop("hdr"), a.pop("quad"), **a)
        assert e.value.code == code, (changes, str(e.value))
        assert words is None or words in str(e.value), str(e.value)
        assert np.array_equal(dst.download(), fill), changes

    bad = abi.ERR_INVALID_ARGUMENT
    nan, inf = float("nan"), float("inf")
    for quad in ((0, 0, -1, 9), (0, 0, 12, -0.5), (0, 0, nan, 9), (0, 0, 12, nan), (nan, 0, 12, 9), (0, inf, 12, 9), (0, 0, inf, 9)):
        refused(bad, quad=quad)
    for region in ((0, 0, 9, 6), (0, 0, 8, 6.5), (-1, 0, 8, 6), (5, 0, 4, 6), (0, 4, 8, 3), (0, 0, nan, 6), (0, 0, 8, inf)):
        refused(bad, lightmap_region=region)
    for region in ((0, 0, 11, 7), (0, -0.5, 10, 7), (0, 0, 10, nan)):
        refused(bad, albedo=tex, albedo_region=region)
    refused(bad, lightmap_filter=2)
    refused(bad, albedo_filter=2)
    refused(bad, lightmap_filter=-1)
    refused(abi.ERR_OUT_OF_RANGE, row_end=10)
    refused(abi.ERR_OUT_OF_RANGE, row_begin=-1)
    refused(abi.ERR_OUT_OF_RANGE, row_begin=5, row_end=4)
    hdr = oc.hdr_configuration(); hdr.ResolveToSRGB = 1
    refused(bad, "pLinearToPSRGB", hdr=hdr)
    hdr = oc.hdr_configuration(); hdr.DitheringStrength = 1
    refused(bad, "ApplyDither", hdr=hdr)
    hdr = oc.hdr_configuration(); hdr.AlbedoIsSRGB = 1
    refused(bad, "pSRGBToPLinear", hdr=hdr, albedo=tex)
    hdr = oc.hdr_configuration(); hdr.Mode = 3
    refused(bad, hdr=hdr)
    # only the with-albedo techniques read AlbedoIsSRGB; a zero-sized quad and a zero-sized region are valid and the first writes nothing
    hdr = oc.hdr_configuration(); hdr.AlbedoIsSRGB = 1
    native.resolve_lighting_scaled(src, dst, hdr, (3, 3, 0, 5))
    native.resolve_lighting_scaled(src, dst, oc.hdr_configuration(), (3, 3, 5, 0), lightmap_region=(4, 4, 4, 4))
    assert np.array_equal(dst.download(), fill)
    # textures of another context
    other = native.Context(0)
    foreign_src, foreign_tex, foreign_dst = native.Lightmap(other, 8, 6, H4), native.Lightmap(other, 10, 7, C8), native.Lightmap(other, 12, 9, F4)
    foreign_dst.upload(fill)
    refused(bad, "context", src=foreign_src)
    refused(bad, "context", albedo=foreign_tex)
    with pytest.raises(native.IlluminantError) as e:
        native.resolve_lighting_scaled(src, foreign_dst, oc.hdr_configuration(), (0, 0, 12, 9))
    assert e.value.code == bad and np.array_equal(foreign_dst.download(), fill)
    _close(foreign_src, foreign_tex, foreign_dst)
    other.close()
    _close(src, tex, dst)
