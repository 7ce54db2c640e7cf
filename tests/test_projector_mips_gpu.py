"""ilm_render_projector_lights over a mip chain (ilm_ctx_set_projector_texture_mips) on the device against the float32 restatement of
tests/projector_mip_common.py.  The frame and scenes are tests/test_projector_gpu.py's (44 x 27 pixels: 3 x 2 workgroup tiles, partial
ones at both rims).  The lights have no origin and no ambient occlusion -- no trace, no pow: every operation of theirs is one float32
rounding on both sides, as in that file's test_lightmap_formats -- so the device must give the restatement's BITS and its statistics;
one shadowed light over the field is held to the suite's criterion.

The chains' levels are unrelated textures (projector_mip_common.chain), not a box filter: a wrong level, a wrong weight or a level read
with another level's size changes the image.  That the cases can tell is asserted: LOD 1 differs from LOD 0 wherever there are two levels.
"""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import projector_common as pc
from tests import projector_mip_common as pmc
from tests import test_projector_gpu as tp
from tests.util import assert_bits_equal, assert_close

pytestmark = pytest.mark.gpu

W, H = pc.WIDTH, pc.HEIGHT
AMBIENT = tp.AMBIENT
NAN, INF = float("nan"), float("inf")

# (width, height, levels): one texel; two levels; no power of two, its last two levels 1 x 1; a square power of two not down to 1 x 1; the
# full chain of a tall odd texture (7 x 16, 3 x 8, 1 x 4, 1 x 2, 1 x 1)
CHAINS = [(1, 1, 1), (2, 1, 2), (5, 3, 4), (8, 8, 4), (7, 16, 5)]


def lods(levels):
    """below, at, between and past the levels; the half-size light's 0.67; what does not compare"""
    return [0.0, 0.25, 0.67, 1.0, 1.5, float(levels - 1), float(levels + 2), -0.5, NAN, INF]


def clamped(lod, **kw):
    return tp.clamped(origin=None, ao_radius=0.0, mip_bias=lod, **kw)


def wrapping(lod, **kw):
    return tp.wrapping(origin=None, mip_bias=lod, **kw)


@pytest.fixture(scope="module")
def scene(ctx, oracle):
    """one scene for the module (unorm16 field, float4 G-buffer) and the restatement's cache of what no LOD changes"""
    s = tp.Scene(ctx, oracle, abi.SDF_UNORM16, abi.GBUFFER_FLOAT4)
    s.cache = {}
    yield s
    s.close()


def want(s, lights, chain, ambient=AMBIENT, **kw):
    return pmc.render(s.oracle, lights, chain, s.env, s.dfu, s.ogb, s.otex, ambient, W, H, pixels=s.pixels, cache=s.cache, **kw)


def check_exact(s, lights, chain, what, **kw):
    """the counting instantiation: the restatement's bits and statistics; the plain one: the counting one's bits"""
    w = want(s, lights, chain, **kw)
    assert w.stats[0] == 0 and w.stats[2] == 0, (what, "a light of exact arithmetic traces nothing")
    got, stats = s.got(lights, chain)
    assert stats == w.stats, (what, stats, w.stats)
    assert_bits_equal(got, w.image, what)
    plain, _ = s.got(lights, chain, want_stats=False)
    assert_bits_equal(plain, got, what + ": the instantiation without statistics against the counting one")
    return got, w


@pytest.mark.parametrize("width,height,levels", CHAINS)
def test_every_lod_on_a_wrapping_and_a_clamped_light(scene, width, height, levels):
    chain = pmc.chain(width, height, levels)
    images = {}
    for lod in lods(levels):
        lights = [wrapping(lod), clamped(lod, opacity=0.7)]
        got, w = check_exact(scene, lights, chain, "%d x %d, %d levels, LOD %r" % (width, height, levels, lod))
        images[repr(lod)] = got
        if lod == 0.0:
            tp.scene_facts(scene, lights, w, "the frame of every LOD", shadowed=False)
            assert w.stats[1] == W * H + 40 * 24
    # what the clamp says: below 0, NaN and 0 are level 0; L - 1, L + 2 and +inf the last level
    for same, as_ in ((-0.5, 0.0), (NAN, 0.0), (float(levels + 2), float(levels - 1)), (INF, float(levels - 1))):
        assert_bits_equal(images[repr(same)], images[repr(as_)], "LOD %r reads what LOD %r reads" % (same, as_))
    if levels > 1:
        # unrelated levels: the cases can tell level 1 from level 0, and a blend from either
        assert (images["1.0"] != images["0.0"]).mean() > 0.5 and (images["0.25"] != images["0.0"]).mean() > 0.5
        assert (images["0.25"] != images["0.67"]).mean() > 0.5
    else:
        assert all(np.array_equal(i, images["0.0"], equal_nan=True) for i in images.values())


@pytest.mark.parametrize("blend_fp16", [False, True])
def test_three_lights_with_different_lods_in_one_call(scene, ctx, blend_fp16):
    """LOD 0.67 (two levels), 1 (weight 0: one level) and NaN (level 0 alone) in one launch: the scalar branch taken and not taken inside
    one light loop; in both blend models, cleared and added onto an uploaded lightmap"""
    chain = pmc.chain(8, 8, 4)
    lights = [clamped(0.67), wrapping(1.0, opacity=0.4), clamped(NAN, scale=(20.0, 14.0, 64.0), translation=(18.3, 8.7, 0.0))]
    ctx.set_lightmap_blend(blend_fp16)
    try:
        before = scenes.uniform(77, (H, W, 4), 0.0, 1.0)
        for ambient, start in ((AMBIENT, None), (None, before)):
            w = want(scene, lights, chain, ambient=ambient, before=start, blend_fp16=blend_fp16)
            assert max(np.unique(w.image[..., 3])) >= 3 and w.stats[1] == W * H + 40 * 24 + 20 * 14
            got, stats = scene.got(lights, chain, ambient=ambient, before=start)
            assert stats == w.stats
            assert_bits_equal(got, w.image, "three LODs in one call, fp16 per light %r, cleared %r" % (blend_fp16, ambient is not None))
            plain, _ = scene.got(lights, chain, ambient=ambient, before=start, want_stats=False)
            assert_bits_equal(plain, got, "three LODs in one call without statistics")
    finally:
        ctx.set_lightmap_blend(False)


def test_one_shadowed_light_over_the_field(scene):
    """a clamped light with an origin, shadows and AO at the half-size light's LOD: the trace and the pows are the one-level pass's, held
    to its criterion; the statistics do not count texture taps"""
    chain = pmc.chain(8, 8, 4)
    lights = [tp.clamped(mip_bias=0.67)]
    w = want(scene, lights, chain)
    tp.scene_facts(scene, lights, w, "a shadowed light over a chain")
    level_0 = want(scene, [tp.clamped(mip_bias=0.0)], chain)
    assert w.stats == level_0.stats and w.stats[2] > 400
    assert np.abs(w.image - level_0.image).max() > 0.01
    got, stats = scene.got(lights, chain)
    assert stats == w.stats
    assert_close(got, w.image, "a shadowed light over a chain")
    plain, _ = scene.got(lights, chain, want_stats=False)
    assert_bits_equal(plain, got, "a shadowed light over a chain without statistics")


def test_rows_5_to_21_leave_the_other_rows_alone(scene):
    chain = pmc.chain(5, 3, 4)
    lights = [clamped(1.5), wrapping(0.25, opacity=0.4)]
    before = scenes.uniform(9, (H, W, 4), 0.0, 1.0)
    full, _ = scene.got(lights, chain)
    for ambient in (AMBIENT, None):
        w = want(scene, lights, chain, ambient=ambient, before=before, row_begin=5, row_end=21)
        got, stats = scene.got(lights, chain, ambient=ambient, before=before, rows=(5, 21))
        assert stats == w.stats and stats[1] == 16 * W + 16 * 40
        assert_bits_equal(got[:5], before[:5], "rows above the strip")
        assert_bits_equal(got[21:], before[21:], "rows below the strip")
        assert_bits_equal(got, w.image, "strip [5, 21)")
        assert_bits_equal(scene.got(lights, chain, ambient=ambient, before=before, rows=(5, 21), want_stats=False)[0], got, "the strip without statistics")
        if ambient is not None:
            assert_bits_equal(got[5:21], full[5:21], "a strip computes what the whole frame computes")


def flat(chain):
    return np.ascontiguousarray(np.concatenate([np.asarray(t, np.float32).reshape(-1, 4) for t in chain]))


def render(s, lights, want_stats=False):
    """the texture is whatever is bound"""
    lm = native.Lightmap(s.ctx, W, H, abi.LIGHTMAP_FLOAT4)
    native.render_projector_lights(s.ctx, pc.light_array(lights), s.env, s.dfu, s.gb, s.sdf, AMBIENT, lm, want_stats=want_stats)
    out = lm.download()
    lm.close()
    return out


def test_one_level_through_the_new_setter_is_the_old_setter(scene, ctx):
    lib = native.lib()
    t = np.ascontiguousarray(pc.texture(5, 3))
    lights = [wrapping(0.67), clamped(2.0, opacity=0.7)]
    try:
        assert lib.ilm_ctx_set_projector_texture(ctx.handle, t.ctypes.data_as(C.c_void_p), 5, 3) == abi.OK
        old = render(scene, lights)
        native.set_projector_texture(ctx, None)
        assert lib.ilm_ctx_set_projector_texture_mips(ctx.handle, t.ctypes.data_as(C.c_void_p), 5, 3, 1) == abi.OK
        assert_bits_equal(render(scene, lights), old, "levels == 1 through the new setter")
        assert_bits_equal(old, scene.want(lights, pc.texture(5, 3)).image, "one level: the LOD changes nothing")
    finally:
        native.set_projector_texture(ctx, None)


def test_either_setter_replaces_what_the_other_bound(scene, ctx):
    chain = pmc.chain(8, 8, 4)
    single = pc.texture(5, 3)
    lights = [wrapping(1.0), clamped(0.67, opacity=0.7)]
    try:
        native.set_projector_texture(ctx, chain)
        over_chain = render(scene, lights)
        assert_bits_equal(over_chain, want(scene, lights, chain).image, "the chain")
        native.set_projector_texture(ctx, single)                     # the old call: one level, the chain's table is gone with it
        over_single = render(scene, lights)
        assert_bits_equal(over_single, scene.want(lights, single).image, "the one-level texture after the chain")
        native.set_projector_texture(ctx, chain)
        assert_bits_equal(render(scene, lights), over_chain, "the chain after the one-level texture")
        native.set_projector_texture(ctx, pmc.chain(5, 3, 4))          # a chain replaces a chain
        assert_bits_equal(render(scene, lights), want(scene, lights, pmc.chain(5, 3, 4)).image, "another chain")
        # levels == 0 and width == 0 unbind, through the new setter too
        lib = native.lib()
        p = flat(chain).ctypes.data_as(C.c_void_p)
        for width, height, levels in ((8, 8, 0), (0, 0, 4)):
            native.set_projector_texture(ctx, chain)
            assert lib.ilm_ctx_set_projector_texture_mips(ctx.handle, p, width, height, levels) == abi.OK
            with pytest.raises(native.IlluminantError, match="texture"):
                render(scene, lights)
    finally:
        native.set_projector_texture(ctx, None)


def test_refusals_bind_nothing_and_write_nothing(scene, ctx):
    lib = native.lib()
    chain = pmc.chain(8, 8, 4)
    lights = [wrapping(1.0), clamped(0.67, opacity=0.7)]
    data = flat(chain)
    p = data.ctypes.data_as(C.c_void_p)
    lm = native.Lightmap(ctx, W, H)
    try:
        native.set_projector_texture(ctx, chain)
        bound = render(scene, lights)
        before = lm.download()
        mips = lib.ilm_ctx_set_projector_texture_mips
        assert mips(lm.handle, p, 8, 8, 4) == abi.ERR_INVALID_HANDLE and b"context" in lib.ilm_last_error()
        assert mips(abi.Handle(0), p, 8, 8, 4) == abi.ERR_INVALID_HANDLE
        assert mips(ctx.handle, p, 8, 8, 17) == abi.ERR_OUT_OF_RANGE and b"mip levels" in lib.ilm_last_error()
        assert mips(ctx.handle, p, 8, 8, -1) == abi.ERR_OUT_OF_RANGE
        assert mips(ctx.handle, None, 8, 8, 4) == abi.ERR_INVALID_ARGUMENT
        assert mips(ctx.handle, None, 8, 8, 1) == abi.ERR_INVALID_ARGUMENT
        for width, height in ((8, 0), (0, 8), (-1, 8), (8, -1), (16385, 8), (8, 16385)):
            assert mips(ctx.handle, p, width, height, 4) == abi.ERR_INVALID_ARGUMENT, (width, height)
            assert b"bad projector texture" in lib.ilm_last_error()
        assert_bits_equal(lm.download(), before, "no refused call wrote a texel")
        assert_bits_equal(render(scene, lights), bound, "the binding a refused call leaves is the one it found")
    finally:
        native.set_projector_texture(ctx, None)
        lm.close()


@pytest.mark.parametrize("translation", [1e9, 3e38])
@pytest.mark.parametrize("lod", [3.0, 2.5, 1.5])
def test_taps_far_past_the_texture(scene, translation, lod):
    """texture coordinates of -1e9 and -3e38 (times the level's width: huge integers, an overflow to infinity) on the 5 x 3 chain, whose
    levels 2 and 3 are 1 x 1: LOD 3 reads the last level, 2.5 two 1 x 1 levels, 1.5 the 2 x 1 level and a 1 x 1 one.  Every tap comes
    from exact integer arithmetic (tap 0 and a NaN weight where the product is infinite): the restatement's bits."""
    chain = pmc.chain(5, 3, 4)
    l = tp.wrapping(scale=(1.0, 1.0, 16.0), translation=(translation, -translation / 3, 0.0), origin=None, mip_bias=lod)
    w = want(scene, [l], chain)
    u = np.array([f["uv"][0] for f in w.detail.values()], np.float64)
    assert len(w.detail) == W * H - 20 and (np.abs(u) > 9e8).all()          # (20 fullbright texels)
    lit = w.image[..., :3][w.image[..., 3] == 2]
    # -3e38 times the 2 texels of level 1 overflows (tap 0, a NaN weight); times the one texel of levels 2 and 3 it stays a huge integer
    assert np.isnan(lit).all() if (translation > 1e38 and lod < 2.0) else np.isfinite(lit).all()
    for want_stats in (True, False):
        got, stats = scene.got([l], chain, want_stats=want_stats)
        assert_bits_equal(got, w.image, "translation %g, LOD %g" % (translation, lod))
        assert stats is None or stats == w.stats
