"""Parity of the output-side kernels (ordered read-back compaction, lightmap resolve -- SURVEY 8f-4) against the CPU oracle.

The resolve: two lit-frame tests, then (contents and criteria in tests/output_common.py) every source / destination / albedo format and
mode on a frame of independent random texels, a frame of black, dim, negative and non-finite texels at six gammas, and strips whose
first texel or texel count is odd -- all on 37 x 29 texels uploaded as they are."""
import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import output_common as oc
from tests.util import assert_close

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("index", range(len(oc.load_cases())))
def test_closed_form_case(ctx, index):
    oc.check_case(oc.load_cases()[index], oc.GpuBackend(ctx))


def test_readback_matches_oracle_record_for_record(ctx, oracle):
    """3 chunks of 64^2 slots with dead slots, a 4 x 4 frame sheet, velocity-driven frames, sorted: integer fields (colour bytes),
    record count and order are exact; float fields within 1e-6."""
    cs, n_chunks = 64, 3
    n = cs * cs
    eng = native.Engine(ctx, cs, scenes.randomness_table(7))
    sysm = native.System(eng)
    chunks = []
    for c in range(n_chunks):
        sysm.add_chunk()
        pos, vel, attr = scenes.make_particles(60 + c, n, pos_lo=(0, 0, 0), pos_hi=(1920, 1080, 32), dead_fraction=0.4)
        rc = scenes.uniform(70 + c, (n, 4), 0.0, 1.2).astype(np.float32)
        rd = np.stack([scenes.uniform(80 + c, (n,), 0.2, 3.0), scenes.uniform(81 + c, (n,), -10.0, 20.0),
                       scenes.uniform(82 + c, (n,), 0.0, 90.0), np.floor(scenes.uniform(83 + c, (n,), 0.0, 6.0))], axis=1).astype(np.float32)
        sysm.upload(c, abi.PLANE_POSITION, pos); sysm.upload(c, abi.PLANE_RENDER_COLOR, rc); sysm.upload(c, abi.PLANE_RENDER_DATA, rd)
        chunks.append([pos, vel, attr, rc, rd])
    params = oc.readback_params((2.0, 3.0), (0.0, 0.0, 0.25, 0.25), (1.7, -0.6), 0.35, True, True, True, True)
    elems = [n, 40 * cs, 17 * cs]        # ceil(TotalSpawned / ChunkSize) * ChunkSize per chunk
    got, gn = sysm.readback(params, element_counts=elems)
    want, wn = oracle.fill_readback_result(chunks, params, element_counts=elems)
    assert gn == wn and 0.3 * sum(elems) < gn < 0.9 * sum(elems)
    g, w = np.frombuffer(got, dtype=np.uint8).reshape(-1, 48)[:gn], np.frombuffer(want, dtype=np.uint8).reshape(-1, 48)[:wn]
    assert np.array_equal(g[:, 40:44], w[:, 40:44])                    # MultiplyColor bytes
    gf, wf = g[:, :40].copy().view(np.float32), w[:, :40].copy().view(np.float32)
    assert np.array_equal(gf[:, :2], wf[:, :2])                        # positions are copies: bit-equal, which also pins the order
    assert_close(gf, wf, "draw call floats", rtol=1e-6, atol=1e-6)
    # a capacity smaller than the live count: the total is still reported, the prefix is returned
    got2, gn2 = sysm.readback(params, element_counts=elems, capacity=100)
    assert gn2 == gn
    assert np.array_equal(np.frombuffer(got2, dtype=np.uint8).reshape(-1, 48)[:100], g[:100])
    # the zero-copy form: the same records, viewed in the context's pinned buffer
    view = sysm.readback_view(params, element_counts=elems)
    assert view.shape == (gn, 12) and np.array_equal(view.view(np.uint8).reshape(-1, 48), g)
    # nothing examined -> nothing returned
    assert sysm.readback_view(params, element_counts=[0, 0, 0]).shape[0] == 0
    sysm.close(); eng.close()


@pytest.mark.parametrize("mode", [abi.HDR_NONE, abi.HDR_GAMMA_COMPRESS, abi.HDR_TONE_MAP])
@pytest.mark.parametrize("fmt", [abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_HALF4])
def test_resolve_matches_oracle_on_a_lit_frame(ctx, oracle, mode, fmt):
    w, h = 160, 112
    layout = scenes.DistanceFieldLayout(256, 192, 96.0, 12, 0.5, 128)
    atlas = scenes.build_sdf_atlas(layout, scenes.random_obstacles(5, 14, (256, 192), size_lo=8.0, size_hi=30.0, z_hi=40.0))
    dfu = layout.uniforms(max_cone_radius=24.0, power=0.7, step_limit=64, min_step_size=1.0, long_step_factor=0.5)
    lights = scenes.random_lights(6, 12, w, h, z=(8.0, 48.0), radius=10.0, ramp=(40.0, 120.0))
    env = scenes.environment()
    sdf = native.DistanceFieldTexture(ctx, atlas)
    src = native.Lightmap(ctx, w, h, fmt)
    native.render_sphere_lights(ctx, lights, env, dfu, None, sdf, (0.05, 0.06, 0.07, 1.0), src)
    lit = src.download().astype(np.float32)            # what the resolve reads (fp16-rounded for the HalfVector4 lightmap)
    hdr = oc.hdr_configuration(mode, 0.5, 0.02, 1.3, 0.9, 0.5, 0.8, 3.0, 2.5)
    dst = native.Lightmap(ctx, w, h, abi.LIGHTMAP_FLOAT4)
    native.resolve_lighting(src, dst, hdr, 8, h - 8)
    got = dst.download()
    want = oracle.resolve_lighting(np.ascontiguousarray(lit), hdr, 8, h - 8)
    assert_close(got[8:h - 8], want[8:h - 8], "resolved frame")
    assert not got[:8].any() and not got[h - 8:].any()             # rows outside the strip untouched
    # the back-buffer case: RGBA8 destination = round(saturate(x) * 255)
    dst8 = native.Lightmap(ctx, w, h, abi.LIGHTMAP_RGBA8)
    native.resolve_lighting(src, dst8, hdr)
    full = oracle.resolve_lighting(np.ascontiguousarray(lit), hdr)
    want8 = np.rint(np.clip(full, 0.0, 1.0) * 255.0).astype(np.int32)
    assert np.abs(dst8.download().astype(np.int32) - want8).max() <= 1
    for x in (dst8, dst, src, sdf):
        x.close()


@pytest.mark.parametrize("mode", [abi.HDR_NONE, abi.HDR_GAMMA_COMPRESS, abi.HDR_TONE_MAP])
@pytest.mark.parametrize("albedo_fmt", [abi.LIGHTMAP_RGBA8, abi.LIGHTMAP_FLOAT4])
def test_resolve_with_albedo_matches_oracle_on_a_lit_frame(ctx, oracle, mode, albedo_fmt):
    """The ...WithAlbedo techniques (Resolve.fx:43-60,141-233): a lit half4 frame over a Color (or float) albedo texture, ragged width so the
    two-texel fast path and the single-texel tail both run."""
    w, h = 157, 96
    layout = scenes.DistanceFieldLayout(256, 192, 96.0, 12, 0.5, 128)
    atlas = scenes.build_sdf_atlas(layout, scenes.random_obstacles(5, 14, (256, 192), size_lo=8.0, size_hi=30.0, z_hi=40.0))
    dfu = layout.uniforms(max_cone_radius=24.0, power=0.7, step_limit=64, min_step_size=1.0, long_step_factor=0.5)
    lights = scenes.random_lights(6, 12, w, h, z=(8.0, 48.0), radius=10.0, ramp=(40.0, 120.0))
    sdf = native.DistanceFieldTexture(ctx, atlas)
    src = native.Lightmap(ctx, w, h, abi.LIGHTMAP_HALF4)
    native.render_sphere_lights(ctx, lights, scenes.environment(), dfu, None, sdf, (0.05, 0.06, 0.07, 0.35), src)
    lit = src.download().astype(np.float32)
    texels = (scenes.uniform(91, (h, w, 4), 0.0, 1.0) * 255.0).astype(np.uint8)
    tex = native.Lightmap(ctx, w, h, albedo_fmt)
    if albedo_fmt == abi.LIGHTMAP_RGBA8:
        tex.upload(texels)
        albedo = texels.astype(np.float32) / np.float32(255.0)
    else:
        albedo = scenes.uniform(92, (h, w, 4), 0.0, 1.5).astype(np.float32)
        tex.upload(albedo)
    hdr = oc.hdr_configuration(mode, 0.75, 0.02, 1.3, 0.9, 0.5, 0.8, 3.0, 2.5)
    dst = native.Lightmap(ctx, w, h, abi.LIGHTMAP_FLOAT4)
    native.resolve_lighting(src, dst, hdr, albedo=tex)
    want = oracle.resolve_lighting(np.ascontiguousarray(lit), hdr, albedo=albedo)
    assert_close(dst.download(), want, "resolved frame with albedo")
    dst8 = native.Lightmap(ctx, w, h, abi.LIGHTMAP_RGBA8)
    native.resolve_lighting(src, dst8, hdr, albedo=tex)
    want8 = np.rint(np.clip(want, 0.0, 1.0) * 255.0).astype(np.int32)
    got8 = dst8.download().astype(np.int32)
    assert np.abs(got8 - want8).max() <= 1
    assert np.array_equal(got8[..., 3], want8[..., 3])          # the albedo's alpha goes straight through
    # strips: rows outside stay untouched
    dst.clear((0.0, 0.0, 0.0, 0.0))
    native.resolve_lighting(src, dst, hdr, 16, 48, albedo=tex)
    part = dst.download()
    assert not part[:16].any() and not part[48:].any()
    assert_close(part[16:48], want[16:48], "strip of the resolved frame with albedo")
    for x in (dst8, dst, tex, src, sdf):
        x.close()


def test_fracture_only_options_are_refused(ctx):
    a = native.Lightmap(ctx, 8, 8, abi.LIGHTMAP_FLOAT4)
    b = native.Lightmap(ctx, 8, 8, abi.LIGHTMAP_FLOAT4)
    hdr = oc.hdr_configuration()
    hdr.ResolveToSRGB = 1
    with pytest.raises(native.IlluminantError) as e:
        native.resolve_lighting(a, b, hdr)
    assert e.value.code == abi.ERR_INVALID_ARGUMENT and "pLinearToPSRGB" in str(e.value)
    hdr = oc.hdr_configuration()
    hdr.AlbedoIsSRGB = 1
    native.resolve_lighting(a, b, hdr)                      # only the with-albedo techniques read it
    t = native.Lightmap(ctx, 8, 8, abi.LIGHTMAP_RGBA8)
    with pytest.raises(native.IlluminantError) as e:
        native.resolve_lighting(a, b, hdr, albedo=t)
    assert e.value.code == abi.ERR_INVALID_ARGUMENT and "pSRGBToPLinear" in str(e.value)
    small = native.Lightmap(ctx, 4, 8, abi.LIGHTMAP_RGBA8)
    with pytest.raises(native.IlluminantError):
        native.resolve_lighting(a, b, oc.hdr_configuration(), albedo=small)
    a.close(); b.close(); t.close(); small.close()


# ---- the resolve on uploaded 37 x 29 frames: formats, edge texels, ragged strips ------------------------------------------------------
_ids = lambda names: (lambda v: names[v])
_WANT = {}


def _want(oracle, key, light, hdr, albedo):
    """The oracle's frame, computed once per content and configuration and shared by the destinations."""
    if key not in _WANT:
        _WANT[key] = oracle.resolve_lighting(np.ascontiguousarray(light), hdr, albedo=albedo)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _texture(ctx, texels, fmt):
    t = native.Lightmap(ctx, texels.shape[1], texels.shape[0], fmt)
    t.upload(texels)
    return t


def _sentinel(fmt, height=oc.H):
    return np.full((height, oc.W, 4), oc.SENTINEL[fmt])


def _resolve_into(dst, src, hdr, tex, row_begin=0, row_end=None):
    """Resolve rows [row_begin, row_end) into a destination filled with the sentinel; the rows outside must still hold it."""
    fill = _sentinel(dst.format, dst.height)
    dst.upload(fill)
    native.resolve_lighting(src, dst, hdr, row_begin, row_end, albedo=tex)
    out = dst.download()
    end = dst.height if row_end is None else row_end
    assert np.array_equal(out[:row_begin], fill[:row_begin]) and np.array_equal(out[end:], fill[end:]), "rows outside the strip were written"
    return out


@pytest.mark.parametrize("index", range(len(oc.EDGE_CASES)), ids=[c["name"] for c in oc.EDGE_CASES])
def test_edge_closed_form_case(ctx, index):
    oc.check_edge_case(oc.EDGE_CASES[index], oc.GpuBackend(ctx))


@pytest.mark.parametrize("mode", oc.MODES, ids=_ids(oc.MODE_NAME))
@pytest.mark.parametrize("albedo_fmt", (None,) + oc.FORMATS, ids=lambda f: "albedo_" + oc.FORMAT_NAME[f])
@pytest.mark.parametrize("dst_fmt", oc.FORMATS, ids=lambda f: "to_" + oc.FORMAT_NAME[f])
@pytest.mark.parametrize("src_fmt", oc.FORMATS, ids=_ids(oc.FORMAT_NAME))
def test_resolve_format_matrix(ctx, oracle, src_fmt, dst_fmt, albedo_fmt, mode):
    """Every source x destination x albedo format x mode on independent random texels (light in [0, 3), albedo in [0, 1.5) or bytes):
    the whole frame and the two ragged strips against the oracle on the decoded textures.  Every texel is identifiable, and an RGBA8
    destination must hold the exact byte on at least 90 % of the colour bytes: swapped pairs or an albedo word off by one cannot pass."""
    src_t, alb_t = oc.random_source(src_fmt), oc.random_albedo(albedo_fmt)
    hdr = oc.matrix_hdr(mode)
    want = _want(oracle, ("matrix", src_fmt, albedo_fmt, mode), oc.decode(src_t, src_fmt), hdr,
                 oc.decode(alb_t, albedo_fmt) if alb_t is not None else None)
    what = "%s -> %s, albedo %s, %s" % (oc.FORMAT_NAME[src_fmt], oc.FORMAT_NAME[dst_fmt], oc.FORMAT_NAME[albedo_fmt], oc.MODE_NAME[mode])
    src, dst = _texture(ctx, src_t, src_fmt), native.Lightmap(ctx, oc.W, oc.H, dst_fmt)
    tex = _texture(ctx, alb_t, albedo_fmt) if alb_t is not None else None
    whole = _resolve_into(dst, src, hdr, tex)
    oc.check_destination(whole, want, dst_fmt, what, exact_share=0.9)
    oc.check_alpha(whole, dst_fmt, alb_t, albedo_fmt, what)
    for b, e in oc.STRIPS:
        part = _resolve_into(dst, src, hdr, tex, b, e)
        oc.check_destination(part[b:e], want[b:e], dst_fmt, what + " rows [%d, %d)" % (b, e))
        oc.check_alpha(part[b:e], dst_fmt, alb_t[b:e] if alb_t is not None else None, albedo_fmt, what)
    for x in (src, dst, tex):
        if x is not None:
            x.close()


_EDGE_PARAMS = [(m, g) for m in oc.MODES for g in (oc.EDGE_GAMMAS if m != abi.HDR_GAMMA_COMPRESS else (1.0,))]


@pytest.mark.parametrize("mode,gamma", _EDGE_PARAMS, ids=["%s-gamma_%g" % (oc.MODE_NAME[m], g) for m, g in _EDGE_PARAMS])
@pytest.mark.parametrize("src_fmt", oc.FORMATS, ids=_ids(oc.FORMAT_NAME))
def test_resolve_black_dim_and_non_finite_texels(ctx, oracle, src_fmt, mode, gamma):
    """Texels cycling through 0, -0, 25 dim values (1e-7 .. 1e-2), the neighbours of -Offset, negatives, 1, 65504, inf and NaN, at Offset 0
    and -0.01, with and without albedo, into every destination format (GammaCompress does not read Gamma: one case).
    A tone-mapped black pixel is ((q - kE / kF) / white) ^ gamma with q = num / den one ulp (2^-27) above kE / kF: a quotient one ulp low
    makes it 0 -- at gamma 0.1 the oracle's 0.164 against 0, and outside the criterion for every v below about 1e-4 at gamma < 1 --, two
    ulps low NaN.  So the quotient has to be the correctly rounded one; the criterion is the default one and not wider.
    The float destination is held to it twice: over the frame, whose component scale the 65504 texels set, and over the texels the
    oracle resolves to at most 2, where the floor is 1e-7 of a scale near 1."""
    src_t = oc.edge_source(src_fmt)
    light = oc.decode(src_t, src_fmt)
    albedo_fmt = oc.edge_albedo_format(src_fmt)
    alb_t = oc.edge_albedo(albedo_fmt)
    albedo = oc.decode(alb_t, albedo_fmt)
    src, tex = _texture(ctx, src_t, src_fmt), _texture(ctx, alb_t, albedo_fmt)
    dsts = [native.Lightmap(ctx, oc.W, oc.H, f) for f in oc.FORMATS]
    for offset in oc.EDGE_OFFSETS:
        hdr = oc.edge_hdr(mode, gamma, offset)
        for with_albedo in (False, True):
            want = _want(oracle, ("edge", src_fmt, mode, gamma, offset, with_albedo), light, hdr, albedo if with_albedo else None)
            finite = np.isfinite(light).all(axis=-1) & (np.isfinite(albedo).all(axis=-1) | (not with_albedo))
            for dst in dsts:
                what = "edge texels %s -> %s, %s, gamma %g, offset %g, %s" % (oc.FORMAT_NAME[src_fmt], oc.FORMAT_NAME[dst.format], oc.MODE_NAME[mode],
                                                                         gamma, offset, "albedo" if with_albedo else "plain")
                got = _resolve_into(dst, src, hdr, tex if with_albedo else None)
                if dst.format != abi.LIGHTMAP_RGBA8 and mode != abi.HDR_GAMMA_COMPRESS:
                    assert not np.isnan(got[finite].astype(np.float32)).any(), what + ": a finite texel resolved to NaN"
                oc.check_destination(got, want, dst.format, what)
                if dst.format == abi.LIGHTMAP_FLOAT4:
                    low = (np.isfinite(want) & (np.abs(want) <= 2.0)).all(axis=-1)
                    assert low.sum() > 100
                    assert_close(got[low], want[low], what + " (texels resolving to at most 2)")
                oc.check_alpha(got, dst.format, alb_t if with_albedo else None, albedo_fmt, what)
    for x in dsts + [src, tex]:
        x.close()


_STRIP_PARAMS = [(abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8, abi.LIGHTMAP_RGBA8), (abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_FLOAT4)]
_STRIP_IDS = ["packed_half4_to_rgba8", "float4_to_float4"]


@pytest.mark.parametrize("mode", oc.MODES, ids=_ids(oc.MODE_NAME))
@pytest.mark.parametrize("src_fmt,dst_fmt,albedo_fmt", _STRIP_PARAMS, ids=_STRIP_IDS)
def test_resolve_ragged_strips_equal_the_whole_frame_bit_for_bit(ctx, src_fmt, dst_fmt, albedo_fmt, mode):
    """Rows [1, 8): 1 * 37 is odd, so no pair of the strip is aligned and the two-texel path falls back throughout (259 texels, odd).
    Rows [2, 29): aligned, 999 texels, so the strip ends in a pair with one texel.  Both do the arithmetic of the whole-frame resolve."""
    src_t, alb_t = oc.random_source(src_fmt), oc.random_albedo(albedo_fmt)
    src, tex, dst = _texture(ctx, src_t, src_fmt), _texture(ctx, alb_t, albedo_fmt), native.Lightmap(ctx, oc.W, oc.H, dst_fmt)
    hdr = oc.matrix_hdr(mode)
    whole = _resolve_into(dst, src, hdr, tex)
    assert not np.array_equal(whole, _sentinel(dst_fmt))
    for b, e in oc.STRIPS:
        part = _resolve_into(dst, src, hdr, tex, b, e)
        assert part[b:e].tobytes() == whole[b:e].tobytes(), "rows [%d, %d) differ from the whole-frame resolve" % (b, e)
    for x in (src, tex, dst):
        x.close()


@pytest.mark.parametrize("src_fmt,dst_fmt,albedo_fmt", _STRIP_PARAMS, ids=_STRIP_IDS)
def test_resolve_textures_of_different_heights(ctx, oracle, src_fmt, dst_fmt, albedo_fmt):
    """Source 37 x 12, destination 37 x 9, albedo 37 x 10: rows [0, 9) exist in all three and resolve; row_end = 10 is refused and
    writes nothing."""
    src_t, alb_t = oc.random_source(src_fmt)[:12], oc.random_albedo(albedo_fmt)[:10]
    src, tex, dst = _texture(ctx, src_t, src_fmt), _texture(ctx, alb_t, albedo_fmt), native.Lightmap(ctx, oc.W, 9, dst_fmt)
    hdr = oc.matrix_hdr(abi.HDR_TONE_MAP)
    got = _resolve_into(dst, src, hdr, tex)
    want = oracle.resolve_lighting(oc.decode(src_t[:9], src_fmt), hdr, albedo=oc.decode(alb_t[:9], albedo_fmt))
    oc.check_destination(got, want, dst_fmt, "rows [0, 9) of textures 12 / 9 / 10 rows high", exact_share=0.9)
    oc.check_alpha(got, dst_fmt, alb_t[:9], albedo_fmt, "rows [0, 9)")
    dst.upload(_sentinel(dst_fmt, 9))
    with pytest.raises(native.IlluminantError) as e:
        native.resolve_lighting(src, dst, hdr, 0, 10, albedo=tex)
    assert e.value.code == abi.ERR_OUT_OF_RANGE
    assert np.array_equal(dst.download(), _sentinel(dst_fmt, 9))
    for x in (src, tex, dst):
        x.close()
