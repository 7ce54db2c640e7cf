"""ilm_render_directional_light_probes and ilm_render_line_light_probes on the device against tests/probe_kinds_common.py.

Criterion: tests.util.assert_close with its defaults on the whole value (the call tests/test_directional_gpu.py makes), and alpha -- the
number of contributing lights -- exactly equal; no element is exempted.  The probes are the committed list pk.probes(), which
tests/test_probe_kinds_kat.py holds off the trace's knife edges on the CPU.  Counts sit at the kernels' edges: 1, 64, 65 and 129 probes
(one lane per probe, 64 per block) under 0, 1, 8, 9 and 17 lights (the sum kernel reads eight contributions at a time), and 3 probes
under 65 536 lights of the sphere and the directional kind: the one-kernel form's loop, past the pair form's grid.
"""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import directional_common as dc
from tests import probe_kinds_common as pk
from tests.util import assert_bits_equal, assert_close

pytestmark = pytest.mark.gpu

PROBE_COUNTS = (1, 64, 65, 129)
LIGHT_COUNTS = (0, 1, 8, 9, 17)
ENV = scenes.environment()


class World:
    def __init__(self, ctx, oracle, fmt):
        self.ctx, self.oracle = ctx, oracle
        self.dfu = dc.field_uniforms()
        self.sdf = native.DistanceFieldTexture(ctx, dc.field_atlas(fmt), fmt)
        self.otex = oracle.make_texture(dc.field_atlas(fmt), fmt)

    def directional(self, lights, pp, pn, dfu=None, sdf=True):
        return native.render_directional_light_probes(self.ctx, dc.light_array(lights) if lights else None, pp, pn, ENV, dfu or self.dfu,
                                                      self.sdf if sdf else None)

    def line(self, lights, pp, pn):
        return native.render_line_light_probes(self.ctx, dc.light_array(lights) if lights else None, pp, pn, ENV, self.dfu, self.sdf)

    def want_pairs(self, lights, pp, pn, dfu=None, sdf=True, ramp=None):
        return pk.directional_pairs(self.oracle, lights, pp, pn, dfu or self.dfu, self.otex if sdf else None, ramp)[0]


@pytest.fixture(scope="module")
def worlds(ctx, oracle):
    made = {}

    def get(fmt=abi.SDF_UNORM16):
        if fmt not in made:
            made[fmt] = World(ctx, oracle, fmt)
        return made[fmt]
    yield get
    for w in made.values():
        w.sdf.close()


def hold(got, want, what):
    print("%s: largest |got - want| %.3g, largest |want| %.3g" % (what, float(np.abs(got - want).max(initial=0)), float(np.abs(want).max(initial=0))))
    assert_close(got, want, what)
    assert np.array_equal(got[:, 3], want[:, 3]), what + ": alpha is the number of contributing lights, exactly"


# ---- directional probes: counts -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def unshadowed(worlds):
    """the reference of the largest case, once: every smaller case is a prefix of it in probes and in lights"""
    pp, pn = pk.probes()
    lights = pk.unshadowed_lights(max(LIGHT_COUNTS))
    pairs = worlds().want_pairs(lights, pp, pn)
    pairs.setflags(write=False)
    return pp, pn, lights, pairs


@pytest.mark.parametrize("probe_count", PROBE_COUNTS)
def test_unshadowed_lights_at_every_count(worlds, unshadowed, probe_count):
    pp, pn, lights, pairs = unshadowed
    for light_count in LIGHT_COUNTS:
        got = worlds().directional(lights[:light_count], pp[:probe_count], pn[:probe_count])
        want = pk.sum_pairs(pairs, probe_count, light_count)
        hold(got, want, "%d probes under %d unshadowed lights" % (probe_count, light_count))
        if light_count == 0:
            assert not got.any()
    if probe_count == 129:
        # the branches of the list: opacity 0 and invisible probes get nothing, every other probe every light (no opacity discard)
        full = pk.sum_pairs(pairs, 129, 17)
        idx = np.arange(129)
        nothing = (idx % 11 == 5) | (idx % 13 == 6)
        assert not full[nothing].any() and (full[~nothing, 3] == 17).all()
        assert (full[~nothing, :3].min(axis=1) > 0).all()
        halved = idx % 7 == 2
        assert halved[~nothing].any() and (pp[halved & ~nothing, 3] == 0.5).all()


@pytest.mark.parametrize("fmt", [abi.SDF_UNORM16, abi.SDF_FP16])
@pytest.mark.parametrize("probe_count,light_count,shadowed", [(65, 9, 9), (129, 17, 4)])
def test_shadowed_lights(worlds, fmt, probe_count, light_count, shadowed):
    """every light shadowed at 65 x 9; four of seventeen at 129 x 17, among directed and undirected lights without shadows"""
    w = worlds(fmt)
    pp, pn = pk.probes(probe_count)
    lights = [pk.shadowed_light(k) for k in range(9)] if shadowed == light_count else pk.mixed_lights(light_count, shadowed)
    pairs = w.want_pairs(lights, pp, pn)
    want = pk.sum_pairs(pairs)
    got = w.directional(lights, pp, pn)
    hold(got, want, "%d probes under %d lights, %d shadowed, format %d" % (probe_count, light_count, shadowed, fmt))
    # the shadows show: with enableShadows a traced pair is darker than without it somewhere, and equal elsewhere
    flat = pn.copy()
    flat[:, 3] = 0.0
    unshadowed_want = pk.sum_pairs(w.want_pairs(lights, pp, flat))
    assert (want[:, 0] < unshadowed_want[:, 0] - 0.01).any() and (want[:, 0] == unshadowed_want[:, 0]).any()
    hold(w.directional(lights, pp, flat), unshadowed_want, "the same with normals.w = 0")
    # the same call again: the same bits
    assert_bits_equal(w.directional(lights, pp, pn), got, "the same call twice")


def test_scratch_is_reused_after_a_larger_call(worlds):
    w = worlds()
    pp, pn = pk.probes()
    small_lights, large_lights = pk.mixed_lights(9, 2), pk.mixed_lights(17, 4)
    first = w.directional(small_lights, pp[:65], pn[:65])
    large = w.directional(large_lights, pp, pn)
    assert_bits_equal(w.directional(small_lights, pp[:65], pn[:65]), first, "65 x 9 after 129 x 17")
    assert_bits_equal(w.directional(large_lights, pp, pn), large, "129 x 17 again")
    # one light takes the one-kernel form (no scratch): the pair-and-sum form of two lights whose second adds nothing agrees with it
    one = w.directional(small_lights[1:2], pp, pn)
    black = dc.directional_light(direction=None, color=(0, 0, 0, 1), casts_shadows=False)
    two = w.directional([small_lights[1], black], pp, pn)
    assert_bits_equal(two[:, :3], one[:, :3], "one light alone and beside a black light")
    assert np.array_equal(two[:, 3], one[:, 3] * 2)


# ---- directional probes: what is read and what is not ---------------------------------------------------------------------------------

def test_bounds_filter_and_ao_members_are_not_read(worlds):
    w = worlds()
    pp, pn = pk.probes(65)
    plain = [pk.shadowed_light(0), pk.unshadowed_lights(3)[2], pk.shadowed_light(1, casts_shadows=False)]
    want = pk.sum_pairs(w.want_pairs(plain, pp, pn))
    got = w.directional(plain, pp, pn)
    hold(got, want, "the plain lights")
    # Bounds that exclude every probe (and would be refused by the frame pass when inverted): all probes are lit, the same bits
    for bounds in ((100.0, 100.0, 101.0, 101.0), (101.0, 101.0, 100.0, 100.0)):
        bounded = [abi.LightVertex.from_buffer_copy(bytes(l)) for l in plain]
        for l in bounded:
            l.LightPosition1 = abi.f4(bounds[0], bounds[1], 0, 0)
            l.LightPosition2 = abi.f4(bounds[2], bounds[3], 0, 0)
        assert_bits_equal(w.directional(bounded, pp, pn), got, "bounds %r" % (bounds,))
    visible = (pp[:, 3] > 0) & (pp[:, 0] > -9999)
    assert (got[visible, 3] == 3).all() and not got[~visible].any()
    # a shadow filter the frame pass would reject pairs by: ShadowsOnly on probes with shadows off, NoShadowsOnly on the others
    for value in (0.0, 1.0):
        filtered = [abi.LightVertex.from_buffer_copy(bytes(l)) for l in plain]
        for l in filtered:
            l.EvenMoreLightProperties.x = value
        assert_bits_equal(w.directional(filtered, pp, pn), got, "shadow filter %g" % value)
    # AO members
    ao = [abi.LightVertex.from_buffer_copy(bytes(l)) for l in plain]
    for l in ao:
        l.MoreLightProperties.x, l.MoreLightProperties.w = 5.0, 0.6
    assert_bits_equal(w.directional(ao, pp, pn), got, "AO radius 5, opacity 0.6")


def test_without_a_field(worlds):
    w = worlds()
    pp, pn = pk.probes(65)
    lights = pk.mixed_lights(5, 1)
    none = pk.sum_pairs(w.want_pairs(lights, pp, pn, dfu=dc.no_field_uniforms(), sdf=False))
    hold(w.directional(lights, pp, pn, dfu=dc.no_field_uniforms(), sdf=False), none, "sdf == 0")
    flat = abi.DistanceFieldUniforms.from_buffer_copy(bytes(w.dfu))
    flat.Extent.x = 0.0
    want = pk.sum_pairs(w.want_pairs(lights, pp, pn, dfu=flat))
    hold(w.directional(lights, pp, pn, dfu=flat), want, "Extent.x == 0")
    # neither traces: the shadowed light is as bright as if it cast none
    shadows_off = pn.copy()
    shadows_off[:, 3] = 0.0
    assert np.array_equal(want, pk.sum_pairs(w.want_pairs(lights, pp, shadows_off))) and np.array_equal(want, none)


def test_ramp_binding_and_context_settings(worlds, ctx):
    w = worlds()
    pp, pn = pk.probes(65)
    lights = pk.mixed_lights(9, 2)
    plain = w.directional(lights, pp, pn)
    hold(plain, pk.sum_pairs(w.want_pairs(lights, pp, pn)), "no ramp")
    ramp = dc.ramp_texture()
    try:
        ctx.set_light_ramp(ramp)
        ramped = w.directional(lights, pp, pn)
        hold(ramped, pk.sum_pairs(w.want_pairs(lights, pp, pn, ramp=ramp)), "DirectionalLightProbeWithRamp")
        assert (ramped[:, :3] != plain[:, :3]).any() and np.array_equal(ramped[:, 3], plain[:, 3])
        ctx.set_light_ramp(np.full((1, 1, 4), 0.25, np.float32))
        assert_bits_equal(w.directional(lights, pp, pn), plain, "a 1 x 1 ramp is no ramp")
        ctx.set_light_ramp(ramp)
        ctx.set_light_ramp(None)
        assert_bits_equal(w.directional(lights, pp, pn), plain, "unbinding restores the plain values")
        # the blend function and the lightmap blend model of the context are not the probe target's
        ctx.set_light_blend_function(abi.LIGHT_BLEND_MAX, abi.LIGHT_BLEND_MAX)
        ctx.set_lightmap_blend(True)
        assert_bits_equal(w.directional(lights, pp, pn), plain, "blend function MAX, fp16-per-light model")
    finally:
        ctx.set_light_ramp(None)
        ctx.set_light_blend_function()
        ctx.set_lightmap_blend(False)


# ---- line probes --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [abi.SDF_UNORM16, abi.SDF_FP16])
def test_line_probes_against_the_oracle_and_the_sphere_entry(worlds, ctx, oracle, fmt):
    w = worlds(fmt)
    pp, pn = pk.probes()
    for ramp_length in (0.0, 12.0):          # 0: what PackLineLight writes
        for probe_count, light_count in ((129, 17), (65, 9), (64, 8), (1, 1), (65, 0)):
            lines = pk.line_lights(light_count, ramp_length=ramp_length)
            p, n = pp[:probe_count], pn[:probe_count]
            got = w.line(lines, p, n)
            want = pk.line_probes(oracle, dc.light_array(lines) if lines else None, p, n, ENV, w.dfu, w.otex)
            hold(got, want, "%d probes under %d line lights, ramp length %g, format %d" % (probe_count, light_count, ramp_length, fmt))
            spheres = [pk.sphere_vertex_of(l) for l in lines]
            same = native.render_light_probes(ctx, dc.light_array(spheres) if spheres else None, p, n, ENV, w.dfu, w.sdf)
            assert_bits_equal(got, same, "ilm_render_light_probes fed the equivalent sphere vertices")
            if light_count == 17:
                assert (got[:, 3] > 0).any() and (got[:, 3] < 17).any() and (got[:, :3] > 0).any()


def test_line_probes_read_four_members_and_no_ramp(worlds, ctx):
    w = worlds()
    pp, pn = pk.probes(65)
    lines = pk.line_lights(9)
    got = w.line(lines, pp, pn)
    moved = pk.line_lights(9)
    for l in moved:
        l.LightPosition2 = abi.f4(1.0, 2.0, 3.0, 4.0)
        l.Color2 = abi.f4(9.0, 8.0, 7.0, 6.0)
        l.EvenMoreLightProperties = abi.f4(1.0, 2.0, 3.0, 4.0)
    assert_bits_equal(w.line(moved, pp, pn), got, "LightPosition2, Color2 and EvenMoreLightProperties")
    try:
        ctx.set_light_ramp(dc.ramp_texture())
        assert_bits_equal(w.line(lines, pp, pn), got, "a bound ramp")
        # (the sphere entry does read it: the binding is live)
        spheres = dc.light_array([pk.sphere_vertex_of(l) for l in lines])
        assert (native.render_light_probes(ctx, spheres, pp, pn, ENV, w.dfu, w.sdf) != got).any()
    finally:
        ctx.set_light_ramp(None)
    assert_bits_equal(w.line(lines, pp, pn), got, "the same call again")


# ---- the one-kernel form under more than one light ---------------------------------------------------------------------------------------

MANY = 65536                 # the pair form's grid ends at 65 535 lights: from here on one lane per probe walks every record
AT = (0, 1, 31999, 32768, 65533, 65534)      # where the lights that reach the probes lie; every other record adds nothing, the last included


def many_lights(dark, bright):
    lights = (abi.LightVertex * MANY).from_buffer_copy(bytes(dark) * MANY)
    for at, light in zip(AT, bright):
        lights[at] = light
    return lights


def test_sphere_probes_in_one_kernel_under_65536_lights(worlds, ctx, oracle):
    """65 536 sphere lights on 3 probes (one ragged wave): the loop of the one-kernel form against the pair-and-sum form of the first
    65 535, bit for bit -- both add the same contributions in the same order, the last light is out of range.  Six lights reach the
    probes (one is shadowed on one of them), the others lie 5 000 px away.  Measured once on an MI355X: 0.08 s for the test's call."""
    w = worlds()
    pp, pn = (a[[2, 4, 10]] for a in pk.probes(11))
    lights = many_lights(scenes.sphere_light((5000.0, 5000.0, 10.0), 4.0, 2.0), [pk.sphere_vertex_of(l) for l in pk.line_lights(8)[1:4] + pk.line_lights(8)[5:8]])
    got = native.render_light_probes(ctx, lights, pp, pn, ENV, w.dfu, w.sdf)
    fewer = native.render_light_probes(ctx, (abi.LightVertex * (MANY - 1)).from_buffer(lights), pp, pn, ENV, w.dfu, w.sdf)
    assert np.array_equal(got, fewer), "65 536 lights in one kernel against 65 535 as pairs"
    want = oracle.render_light_probes(lights, pp, pn, ENV, w.dfu, w.otex)
    hold(got, want, "3 probes under 65 536 sphere lights")
    assert tuple(want[:, 3]) == (1.0, 3.0, 3.0) and (want[1:, :3] > 0).all()
    flat = pn.copy()
    flat[:, 3] = 0.0
    assert (want[:, 0] < oracle.render_light_probes(lights, pp, flat, ENV, w.dfu, w.otex)[:, 0] - 0.01).any(), "a shadow shows"


def test_directional_probes_in_one_kernel_under_65536_lights(worlds):
    """The same under directional lights.  No directional light misses a visible probe, so the 65 530 others are the black, undirected
    light of test_scratch_is_reused_after_a_larger_call: they add 0 to the colours and 1 to alpha.  The colours are compared bit for
    bit with the pair-and-sum form of the first 65 535 lights, and each call's alpha is its number of lights.  Measured once on an
    MI355X: 0.05 s for the test's call."""
    w = worlds()
    pp, pn = (a[[1, 2, 4]] for a in pk.probes(5))
    black = dc.directional_light(direction=None, color=(0, 0, 0, 1), casts_shadows=False)
    mixed = pk.mixed_lights(9, 2)
    bright = [mixed[k] for k in (0, 1, 2, 5, 4, 3)]      # (1 and 5 cast shadows)
    lights = many_lights(black, bright)
    got = native.render_directional_light_probes(w.ctx, lights, pp, pn, ENV, w.dfu, w.sdf)
    fewer = native.render_directional_light_probes(w.ctx, (abi.LightVertex * (MANY - 1)).from_buffer(lights), pp, pn, ENV, w.dfu, w.sdf)
    assert np.array_equal(got[:, :3], fewer[:, :3]), "65 536 lights in one kernel against 65 535 as pairs"
    pairs = w.want_pairs(bright + [black], pp, pn)
    assert (pairs[:, :, 3] == 1).all(), "every light reaches every probe"
    want = pk.sum_pairs(pairs)              # (the black lights between the six add +0 to a sum that is not -0: no bit moves)
    want[:, 3] = MANY
    hold(got, want, "3 probes under 65 536 directional lights")
    assert np.array_equal(fewer[:, 3], want[:, 3] - 1)
    flat = pn.copy()
    flat[:, 3] = 0.0
    assert (want[:, 0] > 0).all() and (want[:, 0] < pk.sum_pairs(w.want_pairs(bright, pp, flat))[:, 0] - 0.01).any(), "a shadow shows"


# ---- the frame pass and the probes agree -----------------------------------------------------------------------------------------------

def test_a_probe_at_a_gbuffer_texel_sees_what_the_frame_pass_sees(worlds, ctx, oracle):
    """probes at the decoded position and normal of G-buffer texels of directional_common's scene, enableShadows = 1, against a
    directional frame without AO or filter, fp32 lightmap, ambient 0"""
    w = worlds()
    W, H = dc.WIDTH, dc.HEIGHT
    g = dc.gbuffer_texels()
    env = scenes.environment(gbuffer_size=(W, H))
    ogb = oracle.make_texture(g, abi.GBUFFER_FLOAT4)
    lights = [pk.shadowed_light(0), pk.shadowed_light(1), pk.unshadowed_lights(3)[2]]
    texels = [(3, 2), (24, 10), (30, 15), (40, 22), (9, 20), (17, 25)]           # ordinary texels: shadows on, not fullbright, a normal
    pp, pn = [], []
    for x, y in texels:
        shaded, normal, enable_shadows, fullbright, _camera = oracle.sample_gbuffer(float(x), float(y), env, ogb)
        assert enable_shadows and not fullbright and any(c != 0 for c in normal)
        pp.append(list(shaded) + [1.0])
        pn.append(list(normal) + [1.0])
    pp, pn = np.array(pp, np.float32), np.array(pn, np.float32)
    gb = native.GBufferTexture(ctx, g, abi.GBUFFER_FLOAT4)
    lm = native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4)
    try:
        native.render_directional_lights(ctx, dc.light_array(lights), env, w.dfu, gb, w.sdf, (0.0, 0.0, 0.0, 0.0), lm)
        frame = lm.download()
    finally:
        lm.close()
        gb.close()
    want = np.array([frame[y, x] for x, y in texels], np.float32)
    got = native.render_directional_light_probes(ctx, dc.light_array(lights), pp, pn, env, w.dfu, w.sdf)
    same = got.view(np.uint32) == want.view(np.uint32)
    print("probe against frame texel: %d of %d components bit-equal" % (int(same.sum()), same.size))
    hold(got, want, "probes at G-buffer texels against the frame")
    assert (want[:, 3] == 3).all() and (want[:, 0] > 0).any()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ilm_render_directional_light_probes", "ilm_render_line_light_probes"])
def test_refusals(ctx, name):
    lib = native.lib()
    entry = getattr(lib, name)
    pp, pn = pk.probes(3)
    out = np.full((3, 4), 7.0, np.float32)
    lights = dc.light_array([pk.shadowed_light(0)] if "directional" in name else pk.line_lights(1))
    dfu = dc.field_uniforms()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda light_count, positions, normals, probe_count, values, sdf=abi.Handle(0), lights=lights: entry(
        ctx.handle, lights, light_count, positions, normals, probe_count, C.byref(ENV), C.byref(dfu), sdf, values)
    # a field with the fixed-point filter: refused by name, nothing written
    sdf = native.DistanceFieldTexture(ctx, dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    try:
        sdf.set_filter(abi.SDF_FILTER_FIXED8)
        assert call(1, ptr(pp), ptr(pn), 3, ptr(out), sdf.handle) == abi.ERR_INVALID_ARGUMENT
        message = lib.ilm_last_error().decode()
        assert name in message and "filter" in message and "8 fraction bits" in message
        assert (out == 7.0).all()
        sdf.set_filter(abi.SDF_FILTER_FP32)
        assert call(1, ptr(pp), ptr(pn), 3, ptr(out), sdf.handle) == 0 and (out != 7.0).all()
    finally:
        sdf.close()
    out[:] = 7.0
    # bad arrays, negative counts
    for args in ((1, None, ptr(pn), 3, ptr(out)), (1, ptr(pp), None, 3, ptr(out)), (1, ptr(pp), ptr(pn), 3, None), (1, ptr(pp), ptr(pn), -1, ptr(out)),
                 (-1, ptr(pp), ptr(pn), 3, ptr(out))):
        assert call(*args) == abi.ERR_INVALID_ARGUMENT, args
    assert call(1, ptr(pp), ptr(pn), 3, ptr(out), lights=None) == abi.ERR_INVALID_ARGUMENT
    assert entry(ctx.handle, lights, 1, ptr(pp), ptr(pn), 3, None, C.byref(dfu), abi.Handle(0), ptr(out)) == abi.ERR_INVALID_ARGUMENT
    assert call(1, ptr(pp), ptr(pn), 3, ptr(out), abi.Handle(987654321)) == abi.ERR_INVALID_HANDLE
    assert (out == 7.0).all()
    # no probes: ILM_OK, nothing touched (not even looked at); no lights: zeros
    assert call(1, None, None, 0, None) == 0
    assert call(0, ptr(pp), ptr(pn), 3, ptr(out), lights=None) == 0 and not out.any()
