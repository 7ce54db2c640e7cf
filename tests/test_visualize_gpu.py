"""ilm_visualize_distance_field on the device against the float32 restatement (tests/visualize_common.py): the drawn mask and the three
statistics EXACTLY, drawn texels by the suite's float criterion, everything else bit for bit.

The field is the small one of visualize_common (64 x 48 x 32, a 2 x 2 atlas, three obstructions) in both atlas formats; the target is
40 x 27 (partial 16 x 16 tiles on both axes, six workgroups) pre-filled with non-constant texels; the view is 32 x 24 pixels at a
fractional offset.  Every view has rays that hit, rays that miss and pixels that are discarded.  Restated images are computed once per
(format, view, mode, ...) and shared.
"""
import types

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import visualize_common as vc
from tests.util import assert_close

pytestmark = pytest.mark.gpu

W, H = 40, 27
OFFSET = (4.25, 1.5)        # px0 = 4.25, py0 = 1.5: pixel row 1 has its centre exactly on the top edge (covered), column 36 is not covered
VIEWS = {"top-down": vc.TOP_DOWN, "oblique": vc.OBLIQUE}
MODES = {"surfaces": vc.SURFACES, "outlines": vc.OUTLINES, "silhouettes": vc.SILHOUETTES}
FORMATS = {"unorm16": abi.SDF_UNORM16, "fp16": abi.SDF_FP16}
PREFILL = vc.prefill(W, H)
_restated = {}


@pytest.fixture(scope="module")
def fields(ctx, oracle):
    """{atlas format: (uniforms, device field, oracle texture)}"""
    dfu = vc.field_layout().uniforms()
    out = {}
    for fmt in FORMATS.values():
        atlas = np.ascontiguousarray(vc.field_atlas(fmt))
        out[fmt] = (dfu, native.DistanceFieldTexture(ctx, atlas, fmt), oracle.make_texture(atlas, fmt))
    yield out
    for _, sdf, _ in out.values():
        sdf.close()


@pytest.fixture(scope="module")
def target(ctx):
    lm = native.Lightmap(ctx, W, H)
    yield lm
    lm.close()


def restated(oracle, fields, fmt, view, mode, offset=OFFSET, size=vc.VIEW_SIZE, color=(1.0, 1.0, 1.0, 1.0), blend=abi.BLEND_ALPHA):
    key = (fmt, view, mode, offset, size, color, blend)
    if key not in _restated:
        dfu, _, texture = fields[fmt]
        quad = vc.camera_quad(VIEWS[view], offset=offset, size=size, color=color)
        _restated[key] = (quad, vc.render(oracle, dfu, texture, quad, vc.make_params(mode, blend), PREFILL))
    return _restated[key]


def bits_differ(a, b):
    """(H, W): texels of two float4 images whose bits differ in any channel."""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) != np.ascontiguousarray(b, np.float32).view(np.uint32)).any(axis=-1)


def check_against(got, want, before, what):
    """Every texel is compared: drawn ones by the float criterion, the others bit for bit with what the target held; and the device
    changed exactly the texels the restatement changed."""
    assert np.array_equal(bits_differ(got, before), bits_differ(want.image, before)), what + ": the device drew other pixels than the restatement"
    assert np.array_equal(np.ascontiguousarray(got[~want.drawn]).view(np.uint32), np.ascontiguousarray(before[~want.drawn]).view(np.uint32)), what
    assert_close(got[want.drawn], want.image[want.drawn], what)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("mode", MODES)
def test_exactness(ctx, oracle, fields, target, mode, view, fmt):
    quad, want = restated(oracle, fields, FORMATS[fmt], view, MODES[mode])
    assert want.stats[0] == 32 * 24 and 0 < want.stats[1] < want.stats[0], "the case must hit, miss and discard"
    dfu, sdf, _ = fields[FORMATS[fmt]]
    target.upload(PREFILL)
    stats = native.visualize_distance_field(ctx, sdf, dfu, vc.quad_array(quad), vc.make_params(MODES[mode]), target, want_stats=True)
    got = target.download()
    print("%s %s %s: device stats %s, restatement %s, most samples on a ray %d" % (mode, view, fmt, stats, want.stats, int(want.samples.max())))
    assert stats == want.stats
    check_against(got, want, PREFILL, "%s %s %s" % (mode, view, fmt))
    # without the counters the image is the same bits (another instantiation of the kernel)
    target.upload(PREFILL)
    assert native.visualize_distance_field(ctx, sdf, dfu, vc.quad_array(quad), vc.make_params(MODES[mode]), target) is None
    assert np.array_equal(target.download().view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("blend", [abi.BLEND_ALPHA, abi.BLEND_ADDITIVE])
def test_outlines_with_a_half_transparent_colour(ctx, oracle, fields, target, blend):
    color = (0.4, 0.2, 0.5, 0.5)        # premultiplied
    quad, want = restated(oracle, fields, abi.SDF_UNORM16, "oblique", vc.OUTLINES, color=color, blend=blend)
    dfu, sdf, _ = fields[abi.SDF_UNORM16]
    target.upload(PREFILL)
    stats = native.visualize_distance_field(ctx, sdf, dfu, vc.quad_array(quad), vc.make_params(vc.OUTLINES, blend), target, want_stats=True)
    got = target.download()
    assert stats == want.stats and want.stats[1] > 0
    check_against(got, want, PREFILL, "outlines, blend %d" % blend)
    # the two blends differ wherever something was drawn, and by the blend's own arithmetic
    _, other = restated(oracle, fields, abi.SDF_UNORM16, "oblique", vc.OUTLINES, color=color, blend=1 - blend)
    assert bits_differ(want.image, other.image)[want.drawn].any()


def test_a_second_pass_composites_over_the_first(ctx, oracle, fields, target):
    dfu, sdf, texture = fields[abi.SDF_UNORM16]
    quad1, first = restated(oracle, fields, abi.SDF_UNORM16, "top-down", vc.SURFACES)
    quad2 = vc.camera_quad(vc.OBLIQUE, offset=OFFSET, color=(0.5, 0.25, 0.125, 1.0))
    p_alpha, p_add = vc.make_params(vc.SURFACES), vc.make_params(vc.SURFACES, abi.BLEND_ADDITIVE)
    again = vc.render(oracle, dfu, texture, quad1, p_alpha, first.image)           # alpha 1 over itself: the same texels
    second = vc.render(oracle, dfu, texture, quad2, p_add, again.image)            # added to what the first two left
    target.upload(PREFILL)
    native.visualize_distance_field(ctx, sdf, dfu, vc.quad_array(quad1), p_alpha, target)
    native.visualize_distance_field(ctx, sdf, dfu, vc.quad_array(quad1), p_alpha, target)
    mid = target.download()
    check_against(mid, again, PREFILL, "surfaces twice")
    assert np.array_equal(again.image.view(np.uint32), first.image.view(np.uint32))
    native.visualize_distance_field(ctx, sdf, dfu, vc.quad_array(quad2), p_add, target)
    got = target.download()
    both = first.drawn & second.drawn
    assert both.any() and (second.drawn & ~first.drawn).any()
    assert np.array_equal(bits_differ(got, mid), bits_differ(second.image, again.image))
    assert np.array_equal(got[~second.drawn].view(np.uint32), mid[~second.drawn].view(np.uint32))
    assert_close(got[second.drawn], second.image[second.drawn], "additive surfaces over alpha surfaces")
    assert np.all(got[both][:, 3] == 2.0)                                            # alpha 1 + alpha 1


def test_clipping(ctx, oracle, fields, target):
    dfu, sdf, _ = fields[abi.SDF_FP16]
    # the rectangle overhangs all four edges of the target: px0 = -6.5, py0 = -5.25, 52 x 36 pixels
    quad, want = restated(oracle, fields, abi.SDF_FP16, "oblique", vc.SURFACES, offset=(-6.5, -5.25), size=(52, 36))
    assert want.covered.all() and want.stats[0] == W * H and 0 < want.stats[1] < W * H
    target.upload(PREFILL)
    stats = native.visualize_distance_field(ctx, sdf, dfu, vc.quad_array(quad), vc.make_params(vc.SURFACES), target, want_stats=True)
    assert stats == want.stats
    check_against(target.download(), want, PREFILL, "overhanging rectangle")
    # entirely outside the target (each side), and empty rectangles: nothing drawn, zero stats
    target.upload(PREFILL)
    for offset, size in (((50.0, 3.0), (32, 24)), ((-40.5, 2.0), (32, 24)), ((3.0, 27.5), (32, 24)), ((3.0, -30.0), (32, 24)),
                         ((5.0, 5.0), (0, 10)), ((5.0, 5.0), (10, 0)), ((5.25, 5.0), (0.125, 10))):
        q = vc.camera_quad(vc.TOP_DOWN, offset=offset, size=size)
        for mode in MODES.values():
            assert native.visualize_distance_field(ctx, sdf, dfu, vc.quad_array(q), vc.make_params(mode), target, want_stats=True) == (0, 0, 0), (offset, size)
    assert np.array_equal(target.download().view(np.uint32), PREFILL.view(np.uint32))
    # a negative viewport scale turns the rectangle inside out: empty
    p = vc.make_params(vc.SURFACES, viewport_scale=(-1.0, 1.0))
    assert native.visualize_distance_field(ctx, sdf, dfu, vc.quad_array(quad), p, target, want_stats=True) == (0, 0, 0)


def test_viewport_transform(ctx, oracle, fields, target):
    """pixel = (Position - ViewportPosition) * ViewportScale: a quad given in display units twice as fine, moved by (10, 6)."""
    dfu, sdf, texture = fields[abi.SDF_UNORM16]
    quad = vc.camera_quad(vc.TOP_DOWN, offset=(10.0 + 2 * 4.25, 6.0 + 2 * 1.5), size=(64, 48))
    p = vc.make_params(vc.SILHOUETTES, viewport_scale=(0.5, 0.5), viewport_position=(10.0, 6.0))
    want = vc.render(oracle, dfu, texture, quad, p, PREFILL)
    _, same = restated(oracle, fields, abi.SDF_UNORM16, "top-down", vc.SILHOUETTES)
    assert np.array_equal(want.image.view(np.uint32), same.image.view(np.uint32))      # (all of these are exact in binary)
    target.upload(PREFILL)
    assert native.visualize_distance_field(ctx, sdf, dfu, vc.quad_array(quad), p, target, want_stats=True) == want.stats
    check_against(target.download(), want, PREFILL, "viewport transform")


def half_units_apart(a, b):
    """Distance in representable half values (both finite, same sign or zero)."""
    ai, bi = a.view(np.int16).astype(np.int32), b.view(np.int16).astype(np.int32)
    ai, bi = np.where(ai < 0, -(ai & 0x7FFF), ai), np.where(bi < 0, -(bi & 0x7FFF), bi)
    return np.abs(ai - bi)


@pytest.mark.parametrize("mode", ["surfaces", "outlines"])
def test_target_formats(ctx, oracle, fields, mode):
    """HALF4 and RGBA8 targets: the pre-fill in the target's format, the restatement over its decoded texels, its image passed through the
    format's conversion; one unit of the format where drawn, the pre-fill's bits elsewhere."""
    dfu, sdf, texture = fields[abi.SDF_UNORM16]
    color = (0.4, 0.2, 0.5, 0.5) if mode == "outlines" else (1.0, 1.0, 1.0, 1.0)
    quad = vc.camera_quad(vc.OBLIQUE, offset=OFFSET, color=color)
    params = vc.make_params(MODES[mode])
    for fmt, encode, decode in ((abi.LIGHTMAP_HALF4, vc.to_half4, lambda t: t.astype(np.float32)), (abi.LIGHTMAP_RGBA8, vc.to_rgba8, vc.from_rgba8)):
        before = encode(PREFILL)
        want = vc.render(oracle, dfu, texture, quad, params, decode(before))
        lm = native.Lightmap(ctx, W, H, fmt)
        lm.upload(before)
        stats = native.visualize_distance_field(ctx, sdf, dfu, vc.quad_array(quad), params, lm, want_stats=True)
        got = lm.download()
        lm.close()
        assert stats == want.stats and want.stats[1] > 0
        assert np.array_equal(got[~want.drawn], before[~want.drawn]), fmt
        expect = encode(want.image)
        if fmt == abi.LIGHTMAP_HALF4:
            assert half_units_apart(got[want.drawn], expect[want.drawn]).max() <= 1
        else:
            assert np.abs(got[want.drawn].astype(np.int32) - expect[want.drawn].astype(np.int32)).max() <= 1
        assert (got[want.drawn] != before[want.drawn]).any()


def test_refusals_on_a_live_context(ctx, fields, target):
    dfu, sdf, _ = fields[abi.SDF_UNORM16]
    target.upload(PREFILL)
    for name, quad, params, word in vc.refusal_cases():
        with pytest.raises(native.IlluminantError) as e:
            native.visualize_distance_field(ctx, sdf, dfu, vc.quad_array(quad), params, target, want_stats=True)
        assert e.value.code == abi.ERR_INVALID_ARGUMENT and word.lower() in str(e.value).lower(), (name, str(e.value))
        assert np.array_equal(target.download().view(np.uint32), PREFILL.view(np.uint32)), name
    good, params = vc.quad_array(vc.camera_quad(vc.TOP_DOWN, offset=OFFSET)), vc.make_params(vc.SURFACES)
    # no field: the reference returns Failed (LightingRenderer.cs:1713)
    with pytest.raises(native.IlluminantError) as e:
        native.visualize_distance_field(ctx, None, dfu, good, params, target)
    assert e.value.code == abi.ERR_STATE
    # a target of another context may not be written from this one: the code ilm_render_particles uses
    other = native.Context(0)
    foreign = native.Lightmap(other, W, H)
    foreign.upload(PREFILL)
    with pytest.raises(native.IlluminantError) as e:
        native.visualize_distance_field(ctx, sdf, dfu, good, params, foreign)
    assert e.value.code == abi.ERR_INVALID_ARGUMENT and "context" in str(e.value)
    assert np.array_equal(foreign.download().view(np.uint32), PREFILL.view(np.uint32))
    # ... nor may an unrelated context read this one's field
    with pytest.raises(native.IlluminantError) as e:
        native.visualize_distance_field(other, sdf, dfu, good, params, foreign)
    assert e.value.code == abi.ERR_INVALID_ARGUMENT
    foreign.close(); other.close()
    # handles that are not what they should be
    for args in ((target, sdf, target), (ctx, target, target), (ctx, sdf, sdf)):
        with pytest.raises(native.IlluminantError) as e:
            native.visualize_distance_field(args[0], args[1], dfu, good, params, args[2])
        assert e.value.code == abi.ERR_INVALID_HANDLE
    # uniforms that describe another atlas, as the light pass refuses them
    bad = scenes.DistanceFieldLayout(64, 48, 32.0, 3).uniforms()
    with pytest.raises(native.IlluminantError) as e:
        native.visualize_distance_field(ctx, sdf, bad, good, params, target)
    assert e.value.code == abi.ERR_INVALID_ARGUMENT and "atlas" in str(e.value)
    assert np.array_equal(target.download().view(np.uint32), PREFILL.view(np.uint32))


def test_a_sibling_context_views_the_field(ctx, oracle, fields):
    """The field may belong to a sibling context (ilm_ctx_create_sibling), as in ilm_render_sphere_lights: same texels."""
    dfu, sdf, _ = fields[abi.SDF_UNORM16]
    quad, want = restated(oracle, fields, abi.SDF_UNORM16, "oblique", vc.SURFACES)
    sibling = ctx.sibling()
    lm = native.Lightmap(sibling, W, H)
    lm.upload(PREFILL)
    stats = native.visualize_distance_field(sibling, sdf, dfu, vc.quad_array(quad), vc.make_params(vc.SURFACES), lm, want_stats=True)
    got = lm.download()
    lm.close(); sibling.close()
    assert stats == want.stats
    check_against(got, want, PREFILL, "from a sibling context")


def test_a_generated_field_is_viewed_in_place(ctx, oracle, target):
    """ilm_sdf_render_slices output viewed without a download; the restatement then runs over the downloaded atlas."""
    layout = vc.field_layout()
    obstructions = scenes.random_obstructions(17, 3, (64, 48), 4.0, 11.0, 20.0)
    desc = scenes.render_desc(layout)
    field = native.DistanceFieldTexture(ctx, None, abi.SDF_UNORM16, size=(layout.atlas_width, layout.atlas_height))
    field.render_slices(desc, list(range(0, layout.slice_count, 3)), scenes.obstruction_array(obstructions))
    dfu = layout.uniforms()
    quad = vc.camera_quad(vc.OBLIQUE, offset=OFFSET)
    results = {}
    for mode in (vc.SURFACES, vc.SILHOUETTES):
        target.upload(PREFILL)
        stats = native.visualize_distance_field(ctx, field, dfu, vc.quad_array(quad), vc.make_params(mode), target, want_stats=True)
        results[mode] = (stats, target.download())
    atlas = field.download()
    field.close()
    texture = oracle.make_texture(atlas, abi.SDF_UNORM16)
    for mode, (stats, got) in results.items():
        want = vc.render(oracle, dfu, texture, quad, vc.make_params(mode), PREFILL)
        assert 0 < want.stats[1] < want.stats[0]
        assert stats == want.stats
        check_against(got, want, PREFILL, "generated field, mode %d" % mode)


def test_host_mirror(oracle):
    """LightingRenderer.VisualizeDistanceField of the host mirror: the same image as the C ABI with the mirror's own vertices, which are
    the reference's quad (a view plane one unit above the field's floor, looking down: LightingRenderer.cs:1782-1789)."""
    from illuminant_amd import _host as Host
    hctx = Host.DeviceContext(0)
    layout = vc.field_layout()
    atlas = np.ascontiguousarray(vc.field_atlas(abi.SDF_UNORM16))
    env = Host.LightingEnvironment()
    r = Host.LightingRenderer(hctx, Host.RendererConfiguration(W, H), env)
    view = (0.0, 0.0, -1.0)
    rectangle = (OFFSET[0], OFFSET[1], OFFSET[0] + 32, OFFSET[1] + 24)
    rt = Host.RenderTarget(hctx, W, H)
    info, stats = r.VisualizeDistanceField(rt.Handle, list(rectangle), list(view), wantStats=True)
    assert info.Failed and stats is None                                  # no field (:1713)
    field = Host.DistanceField(hctx, 64, 48, 32.0, 12, 1.0)
    field.Load(atlas)
    r.DistanceField = field
    direct = native.Lightmap(None, W, H, abi.LIGHTMAP_FLOAT4, borrowed_handle=rt.Handle)
    direct.upload(PREFILL)
    color = (0.9, 0.8, 0.7, 1.0)
    info, stats = r.VisualizeDistanceField(rt.Handle, list(rectangle), list(view), mode=vc.SURFACES, color=list(color), wantStats=True)
    got = rt.Download()
    dfu = abi.DistanceFieldUniforms.from_buffer_copy(r.GetDistanceFieldUniformsBytes())
    want_info, quad = vc.reference_quad(rectangle, view, (0, 0, 0), (64, 48, 32), color)
    assert not info.Failed and np.array(info.ViewCenter, np.float32).tobytes() == want_info["ViewCenter"].tobytes()
    want = vc.render(oracle, dfu, oracle.make_texture(atlas, abi.SDF_UNORM16), quad, vc.make_params(vc.SURFACES), PREFILL)
    assert tuple(stats) == want.stats and 0 < want.stats[1] < want.stats[0]
    check_against(got, want, PREFILL, "host mirror")
    # the C ABI with the mirror's vertices, on the mirror's context and field
    nctx = native.Context(borrowed_handle=hctx.Handle)
    direct.upload(PREFILL)
    sdf = types.SimpleNamespace(handle=abi.Handle(int(field.TextureHandle)))
    assert native.visualize_distance_field(nctx, sdf, dfu, vc.quad_array(quad), vc.make_params(vc.SURFACES), direct, want_stats=True) == want.stats
    assert np.array_equal(direct.download().view(np.uint32), np.ascontiguousarray(got).view(np.uint32))
    # outlines through the mirror: the default OutlineSize 1.8 and a request below 1, which the reference raises to 1 (:1877)
    for outline, bound in ((1.8, 1.8), (0.25, 1.0)):
        direct.upload(PREFILL)
        info, stats = r.VisualizeDistanceField(rt.Handle, list(rectangle), list(view), mode=vc.OUTLINES, outlineSize=outline, wantStats=True)
        o = vc.render(oracle, dfu, oracle.make_texture(atlas, abi.SDF_UNORM16), vc.reference_quad(rectangle, view, (0, 0, 0), (64, 48, 32))[1],
                      vc.make_params(vc.OUTLINES, outline_size=bound), PREFILL)
        assert tuple(stats) == o.stats
        check_against(rt.Download(), o, PREFILL, "host mirror outlines %g" % outline)
