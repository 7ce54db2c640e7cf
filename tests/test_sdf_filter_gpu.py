"""The distance field's bilinear filter (ilm_sdf_set_filter) on the device, against the restatements of tests/sdf_filter_common.py at
8 fraction bits: both sampler forms bit for bit, the sphere pass with exact statistics and alpha and rgb within the suite's criterion
(tests.util.assert_close), the default path bit for bit what it was, and every consumer that does not honour the filter refusing a
filtered field with its target untouched.

Frames of 44 x 27 pixels (partial 16 x 16 tiles on both rims) over directional_common's field, MaxStepCount 24; the scene is
sdf_filter_common.scene_lights (tests/test_sdf_filter_kat.py holds it to the conditions that make these tests mean something: port(8)
and port(0) differ beyond the criterion on at least 20 pixels of every frame, so a kernel that ignores the filter fails here)."""
import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import directional_common as dc
from tests import lights_common as lc
from tests import sdf_filter_common as sf
from tests import visualize_common as vc
from tests.sdf_filter_common import Z_VALUES, kat_field, position
from tests.util import assert_bits_equal, assert_close

pytestmark = pytest.mark.gpu

W, H = sf.WIDTH, sf.HEIGHT
F = np.float32
FIXED8, FP32 = abi.SDF_FILTER_FIXED8, abi.SDF_FILTER_FP32


def refused(call, word="filter"):
    with pytest.raises(native.IlluminantError) as e:
        call()
    assert e.value.code == abi.ERR_INVALID_ARGUMENT and word in str(e.value), str(e.value)


# ---- 1. the sample entry points ----------------------------------------------------------------------------------------------------

def kat_positions():
    """the known-answer positions of tests/test_sdf_filter_kat.py on its 16 x 16 field: fractions k / 256, ties, their neighbours one ulp
    of the coordinate away, fractions of 255.5 / 256 and more, and 0 -- on x and on y"""
    base = F(5.5)
    ulp = np.spacing(base)
    fractions = [F(k) / F(256) for k in (0, 1, 2, 3, 127, 128, 129, 254, 255)]
    for tie in (F(0.5), F(1.5), F(2.5), F(254.5), F(255.5)):
        fractions += [tie / F(256) - ulp, tie / F(256), tie / F(256) + ulp]
    fractions += [ulp, F(255.75) / F(256), F(1) - ulp, F(100.25) / F(256), F(100.75) / F(256)]
    pts = []
    for axis in (0, 1):
        for f in fractions:
            for z in Z_VALUES:
                pts.append(position(axis, F(base + f), F(9.5) + F(77) / F(256), z))
    # (outside the table form's box: next to a face of the volume, and beyond it)
    pts += [(0.2, 9.7, 1.0), (8.3, 15.9, 2.0), (-1.25, 4.4, 3.0), (7.7, 17.5, 1.0), (3.3, 4.4, 9.5)]
    return np.array(pts, np.float32)


@pytest.mark.parametrize("fmt", sf.FORMATS)
def test_both_sampler_forms_equal_the_port_at_8_bits_bit_for_bit(ctx, fmt):
    cases = []
    dfu = sf.field_uniforms()
    visited = np.unique(np.concatenate([sf.reference(fmt, g, 8).visited for g in (False, True)]), axis=0)
    cases.append((dc.field_atlas(fmt), dfu, np.concatenate([sf.probe_positions(dfu), visited])))
    atlas, kdfu = kat_field(fmt)
    cases.append((atlas, kdfu, kat_positions()))
    for atlas, dfu, pts in cases:
        sdf = native.DistanceFieldTexture(ctx, atlas, fmt)
        try:
            assert sdf.filter == FP32
            before, (before_inside, used0) = sdf.sample(dfu, pts), sdf.sample_inside(dfu, pts)
            want0 = sf.Sampler(atlas, fmt, dfu, 0).many(pts)
            assert_bits_equal(before, want0, "general form, fp32 weights")
            assert_bits_equal(before_inside, want0, "table form, fp32 weights")
            sdf.set_filter(FIXED8)
            assert sdf.filter == FIXED8
            want8 = sf.Sampler(atlas, fmt, dfu, 8).many(pts)
            assert (want8.view(np.uint32) != want0.view(np.uint32)).sum() > len(pts) // 4, "the positions must see the filter"
            assert_bits_equal(sdf.sample(dfu, pts), want8, "general form, FIXED8")
            got, used = sdf.sample_inside(dfu, pts)
            assert_bits_equal(got, want8, "table form, FIXED8")
            assert used.any() and not used.all() and np.array_equal(used, used0)
            sdf.set_filter(FP32)
            assert_bits_equal(sdf.sample(dfu, pts), before, "general form, back at fp32 weights")
            assert_bits_equal(sdf.sample_inside(dfu, pts)[0], before_inside, "table form, back at fp32 weights")
        finally:
            sdf.close()


# ---- 2. the sphere pass ------------------------------------------------------------------------------------------------------------

class Scene:
    def __init__(self, ctx, fmt, with_gbuffer):
        self.ctx = ctx
        self.ref = sf.reference(fmt, with_gbuffer, 8)
        self.sdf = native.DistanceFieldTexture(ctx, self.ref.atlas, fmt)
        self.gb = native.GBufferTexture(ctx, self.ref.gbuffer, abi.GBUFFER_FLOAT4) if with_gbuffer else None

    def render(self, light_set, lm_fmt=abi.LIGHTMAP_FLOAT4, want_stats=True, sdf=None):
        lm = native.Lightmap(self.ctx, W, H, lm_fmt)
        lights = dc.light_array([self.ref.lights[i] for i in light_set])
        stats = native.render_sphere_lights(self.ctx, lights, self.ref.env, self.ref.dfu, self.gb, sdf or self.sdf, sf.AMBIENT, lm, want_stats=want_stats)
        out = lm.download()
        lm.close()
        return out, ((stats.SdfSamples, stats.PixelLightPairs, stats.TracedPairs) if want_stats else None)

    def close(self):
        for x in (self.sdf, self.gb):
            if x is not None:
                x.close()


@pytest.fixture(scope="module")
def scene_cache(ctx):
    cache = {}

    def get(fmt, with_gbuffer):
        if (fmt, with_gbuffer) not in cache:
            cache[(fmt, with_gbuffer)] = Scene(ctx, fmt, with_gbuffer)
        return cache[(fmt, with_gbuffer)]
    yield get
    for s in cache.values():
        s.close()


@pytest.mark.parametrize("fmt", sf.FORMATS)
@pytest.mark.parametrize("with_gbuffer", [False, True])
def test_the_sphere_pass_in_the_mode_is_the_port_at_8_bits(scene_cache, fmt, with_gbuffer):
    s = scene_cache(fmt, with_gbuffer)
    s.sdf.set_filter(FIXED8)
    try:
        for light_set in sf.LIGHT_SETS:
            what = "FIXED8, field format %d, G-buffer %s, lights %s" % (fmt, with_gbuffer, light_set)
            want, want_stats = s.ref.frame(light_set)
            got, stats = s.render(light_set)
            assert stats == want_stats, what
            assert np.array_equal(got[..., 3], want[..., 3]), what
            assert_close(got[..., :3], want[..., :3], "lightmap rgb, " + what)
            # the plain launch's lightmap is the counting launch's, bit for bit
            plain, _ = s.render(light_set, want_stats=False)
            assert_bits_equal(plain, got, "plain against counting, " + what)
            # the mode was on: the same frame with fp32 weights lies beyond the criterion
            assert sf.beyond_criterion(got, sf.reference(fmt, with_gbuffer, 0).frame(light_set)[0]).sum() >= 20, what
    finally:
        s.sdf.set_filter(FP32)


@pytest.mark.parametrize("fmt", sf.FORMATS)
def test_a_half4_lightmap_stores_the_same_registers(scene_cache, fmt):
    s = scene_cache(fmt, True)
    s.sdf.set_filter(FIXED8)
    try:
        got32, stats = s.render(sf.LIGHT_SETS[-1])
        want, want_stats = s.ref.frame(sf.LIGHT_SETS[-1])
        assert stats == want_stats
        assert_close(got32[..., :3], want[..., :3], "lightmap rgb")
        for want_stats_ in (True, False):
            got16, _ = s.render(sf.LIGHT_SETS[-1], lm_fmt=abi.LIGHTMAP_HALF4, want_stats=want_stats_)
            assert np.array_equal(np.asarray(got16).view(np.uint16), dc.to_stored(got32, abi.LIGHTMAP_HALF4).view(np.uint16))
    finally:
        s.sdf.set_filter(FP32)


# ---- 3. the cells, 4. the default path ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", sf.FORMATS)
def test_toggling_the_filter_rebuilds_nothing_and_the_default_path_is_what_it_was(scene_cache, ctx, fmt):
    s = scene_cache(fmt, False)
    light_set = sf.LIGHT_SETS[-1]
    never_set = native.DistanceFieldTexture(ctx, s.ref.atlas, fmt)          # a texture whose filter was never set
    try:
        want, want_stats = s.render(light_set, sdf=never_set)
        first, _ = s.render(light_set)
        info = s.sdf.trace_info()
        assert info.CellBytes > 0 and info.TableSlices == 12
        rebuilds, cell_bytes, slices = info.CellRebuilds, info.CellBytes, info.CellSlicesRebuilt
        for bits in (FIXED8, FP32, FIXED8, FP32):
            s.sdf.set_filter(bits)
            frame, stats = s.render(light_set)
            info = s.sdf.trace_info()
            assert (info.CellRebuilds, info.CellBytes, info.CellSlicesRebuilt) == (rebuilds, cell_bytes, slices), bits
            if bits == FP32:
                assert_bits_equal(frame, want, "a frame after set_filter(0) against a texture whose filter was never set")
                assert stats == want_stats
            else:
                assert not np.array_equal(frame, want)
        assert_bits_equal(first, want, "two textures of the same atlas")
    finally:
        s.sdf.set_filter(FP32)
        never_set.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------

def test_the_setter_refuses_other_widths_and_reports_a_bad_handle_first(ctx):
    sdf = native.DistanceFieldTexture(ctx, dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    try:
        sdf.set_filter(FIXED8)
        for bits in (5, 1, 7, 9, 16, -8, 256):
            refused(lambda: sdf.set_filter(bits), "fraction bits")
            assert sdf.filter == FIXED8                          # the state is kept
        sdf.set_filter(FP32)
        refused(lambda: sdf.set_filter(5), "fraction bits")
        assert sdf.filter == FP32
        lib = native.lib()
        assert lib.ilm_sdf_set_filter(abi.Handle(0), 5) == abi.ERR_INVALID_HANDLE              # the handle is looked up first
        assert lib.ilm_sdf_set_filter(ctx.handle, FIXED8) == abi.ERR_INVALID_HANDLE           # (a context is no distance field)
        assert lib.ilm_sdf_get_filter(abi.Handle(0), None) == abi.ERR_INVALID_HANDLE
        assert lib.ilm_sdf_get_filter(sdf.handle, None) == abi.ERR_INVALID_ARGUMENT
    finally:
        sdf.close()


def test_the_sphere_pass_refuses_the_models_it_does_not_compose_with(scene_cache, ctx):
    s = scene_cache(abi.SDF_UNORM16, False)
    lights = dc.light_array(s.ref.lights)
    before = scenes.uniform(91, (H, W, 4), 0.0, 1.0)
    lm = native.Lightmap(ctx, W, H)
    lm.upload(before)
    s.sdf.set_filter(FIXED8)
    try:
        ctx.set_lightmap_blend(True)
        refused(lambda: native.render_sphere_lights(ctx, lights, s.ref.env, s.ref.dfu, None, s.sdf, sf.AMBIENT, lm, want_stats=True))
        ctx.set_lightmap_blend(False)
        ctx.set_light_blend_function(abi.LIGHT_BLEND_MAX, abi.LIGHT_BLEND_MAX)
        refused(lambda: native.render_sphere_lights(ctx, lights, s.ref.env, s.ref.dfu, None, s.sdf, sf.AMBIENT, lm))
        ctx.set_light_blend_function(abi.LIGHT_BLEND_ADD, abi.LIGHT_BLEND_MAX)
        refused(lambda: native.render_sphere_lights(ctx, lights, s.ref.env, s.ref.dfu, None, s.sdf, None, lm))
        assert_bits_equal(lm.download(), before, "the refused sphere passes left the lightmap alone")
        # with the filter back at 0 both models run as before
        s.sdf.set_filter(FP32)
        native.render_sphere_lights(ctx, lights, s.ref.env, s.ref.dfu, None, s.sdf, sf.AMBIENT, lm)
        assert not np.array_equal(lm.download(), before)
    finally:
        ctx.set_lightmap_blend(False)
        ctx.set_light_blend_function(abi.LIGHT_BLEND_ADD, abi.LIGHT_BLEND_ADD)
        s.sdf.set_filter(FP32)
        lm.close()


def test_every_light_pass_that_does_not_honour_the_filter_refuses_it(scene_cache, ctx):
    s = scene_cache(abi.SDF_UNORM16, False)
    env, dfu = s.ref.env, s.ref.dfu
    before = scenes.uniform(92, (H, W, 4), 0.0, 1.0)
    lm = native.Lightmap(ctx, W, H)
    lm.upload(before)
    cs = 16
    eng = native.Engine(ctx, cs, scenes.randomness_table(7))
    sysm = native.System(eng)
    sysm.add_chunk()
    s.sdf.set_filter(FIXED8)
    try:
        # the full-frame passes: a call without lights would clear the rows to the ambient colour
        for render in (native.render_directional_lights, native.render_line_lights, native.render_projector_lights, native.render_volumetric_lights):
            refused(lambda: render(ctx, None, env, dfu, None, s.sdf, sf.AMBIENT, lm, want_stats=True))
        one = dc.light_array([dc.directional_light(direction=(0.3, 0.2, -0.9), bounds=(0.0, 0.0, 44.0, 27.0))])
        refused(lambda: native.render_directional_lights(ctx, one, env, dfu, None, s.sdf, None, lm))
        params = lc.particle_light_params(3.0, 30.0, (0.9, 0.8, 0.7, 0.6), casts_shadows=True)
        refused(lambda: native.render_particle_lights(ctx, sysm, params, env, dfu, None, s.sdf, lm, want_stats=True))
        positions = np.array([[10.0, 10.0, 2.0, 0.0], [30.0, 20.0, 4.0, 0.0]], np.float32)
        normals = np.array([[0.0, 0.0, 1.0, 0.0]] * 2, np.float32)
        refused(lambda: native.render_light_probes(ctx, dc.light_array(s.ref.lights), positions, normals, env, dfu, s.sdf))
        quad = vc.quad_array(vc.camera_quad(vc.TOP_DOWN, size=(32, 24)))
        refused(lambda: native.visualize_distance_field(ctx, s.sdf, dfu, quad, vc.make_params(vc.SURFACES), lm, want_stats=True))
        assert_bits_equal(lm.download(), before, "the refused passes left the lightmap alone")
        # the same calls run once the filter is back at 0
        s.sdf.set_filter(FP32)
        native.render_directional_lights(ctx, None, env, dfu, None, s.sdf, sf.AMBIENT, lm)
        assert np.array_equal(lm.download(), np.broadcast_to(np.asarray(sf.AMBIENT, np.float32), (H, W, 4)))
    finally:
        s.sdf.set_filter(FP32)
        for x in (sysm, eng, lm):
            x.close()


def test_the_group_entry_refuses_a_filtered_field(ctx):
    ref = sf.reference(abi.SDF_UNORM16, False, 8)
    g = native.Group([0, 0])
    glm = native.GroupLightmap(g, W, H)
    sdfs = [native.DistanceFieldTexture(c, ref.atlas, abi.SDF_UNORM16) for c in g.contexts]
    lights = dc.light_array(ref.lights)
    try:
        g.render_sphere_lights(lights, ref.env, ref.dfu, None, sdfs, sf.AMBIENT, glm, native.GATHER_NONE)
        g.sync()
        before = [glm.download(i) for i in range(g.n_local)]
        sdfs[1].set_filter(FIXED8)
        refused(lambda: g.render_sphere_lights(lights, ref.env, ref.dfu, None, sdfs, (0.5, 0.5, 0.5, 1.0), glm, native.GATHER_NONE, want_stats=True))
        g.sync()
        for i in range(g.n_local):
            assert_bits_equal(glm.download(i), before[i], "member %d's frame after the refused group call" % i)
        sdfs[1].set_filter(FP32)
        g.render_sphere_lights(lights, ref.env, ref.dfu, None, sdfs, sf.AMBIENT, glm, native.GATHER_NONE)
        g.sync()
        assert_bits_equal(glm.download(0), before[0], "the group call with the filter back at 0")
    finally:
        for x in sdfs:
            x.close()
        glm.close(); g.close()


def collision_step(cs, dfu):
    d = abi.StepDesc()
    d.FirstChunk, d.ChunkCount = 0, -1
    d.System = scenes.system_uniforms(cs, friction=0.1, max_velocity=2048.0, life_decay=1.2)
    d.Update = abi.UpdateParams.default()
    d.OpCount = 1
    d.Ops[0].Type = abi.OP_GRAVITY
    d.Ops[0].u.Gravity = scenes.gravity_params([((24.0, 16.0, 8.0), 150.0, 60.0, 1)])
    d.UpdateMode = abi.UPDATE_WITH_DISTANCE_FIELD
    d.DistanceField = dfu
    return d


def test_the_particle_entry_points_refuse_a_filtered_field(ctx):
    cs = 64
    n = cs * cs
    layout = dc.field_layout()
    dfu = layout.uniforms(packed1=False)          # as the reference's particle path binds the uniforms
    sdf = native.DistanceFieldTexture(ctx, dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    eng = native.Engine(ctx, cs, scenes.randomness_table(7))
    sysm = native.System(eng)
    sysm.add_chunk()
    pos, vel, attr = scenes.make_particles(3, n, dead_fraction=0.25)
    pos[:, :3] = np.abs(pos[:, :3]) % np.array([48.0, 32.0, 32.0], np.float32)
    for plane, data in ((abi.PLANE_POSITION, pos), (abi.PLANE_VELOCITY, vel), (abi.PLANE_ATTRIBUTES, attr)):
        sysm.upload(0, plane, data)
    planes = (abi.PLANE_POSITION, abi.PLANE_VELOCITY, abi.PLANE_ATTRIBUTES)
    try:
        sdf.set_filter(FIXED8)
        refused(lambda: sysm.set_distance_field(sdf))                    # attaching it
        sdf.set_filter(FP32)
        sysm.set_distance_field(sdf)
        sdf.set_filter(FIXED8)                                           # ... or filtering an attached field
        before = [sysm.download(0, p) for p in planes]
        d = collision_step(cs, dfu)
        refused(lambda: sysm.step(d))
        refused(lambda: eng.step_batch([sysm], [d]))
        for p, b in zip(planes, before):
            assert_bits_equal(sysm.download(0, p), b, "plane %d after the refused steps" % p)
        # a step that does not sample the field is not concerned
        free = collision_step(cs, dfu)
        free.UpdateMode = abi.UPDATE_POSITIONS
        sysm.step(free)
        assert not np.array_equal(sysm.download(0, abi.PLANE_POSITION), before[0])
        # and with the filter back at 0 the collision update runs
        sdf.set_filter(FP32)
        sysm.step(d)
        eng.step_batch([sysm], [d])
    finally:
        for x in (sysm, eng, sdf):
            x.close()
