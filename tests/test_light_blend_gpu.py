"""ilm_ctx_set_light_blend_function on the device, for the six light passes: REVERSE_SUBTRACT, MAX and MIN light groups against the
unchanged additive path (exactly) and against per-light oracle images combined by tests/light_blend_common.py (the suite's criterion).

Frames of 40 x 24 pixels (3 x 2 workgroup tiles, ragged on both axes) over directional_common's field and G-buffer, with the light sets
of each pass's own tests.  A pass's SOURCE images -- one light alone on zeros: rgb = the pair's contribution, alpha = 1 where the pair
contributes -- are made once per module, by the device's additive path (for the exact checks) and by the pass's oracle, unchanged.
No pixel is left out of any comparison."""
import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import directional_common as dc
from tests import light_blend_common as lb
from tests import lights_common as plc
from tests import line_common as lc
from tests import projector_common as pc
from tests import volumetric_common as vc
from tests import volumetric_scenes as vs
from tests.util import ATOL_TIGHT, assert_bits_equal, assert_close

pytestmark = pytest.mark.gpu

W, H = 40, 24
ADD, RSUB, MAX, MIN = lb.ADD, lb.REVERSE_SUBTRACT, lb.MAX, lb.MIN
NON_ADDITIVE = (RSUB, MAX, MIN)
PASSES = ("sphere", "particle", "directional", "line", "projector", "volumetric")
AMBIENT = (0.2713, 0.1377, 0.3591, 1.0)
ZEROS = np.zeros((H, W, 4), np.float32)


class LightPass:
    """One pass over the shared scene: `render` is the native call over a subset of its lights (always in list order), `oracle_source`
    the oracle's image of one light alone on a zero clear colour."""
    has_clear = True

    def __init__(self, ctx, oracle):
        self.ctx, self.oracle = ctx, oracle
        self.dfu = self.field_uniforms()
        self.sdf = native.DistanceFieldTexture(ctx, dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
        self.otex = oracle.make_texture(dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
        g = np.ascontiguousarray(dc.gbuffer_texels()[:H, :W])
        self.gb = native.GBufferTexture(ctx, g, abi.GBUFFER_FLOAT4)
        self.ogb = oracle.make_texture(g, abi.GBUFFER_FLOAT4)
        self.env = scenes.environment(gbuffer_size=(W, H), **self.env_kw())
        self.lights = self.make_lights()
        self.n = len(self.lights)
        self._pixels = None
        self._device_sources = self._oracle_sources = None

    def env_kw(self):
        return {}

    def field_uniforms(self):
        return dc.field_uniforms()

    def pixels(self):
        if self._pixels is None:
            self._pixels = dc.decode_pixels(self.oracle, self.env, self.ogb, W, H)
        return self._pixels

    def call(self, lights, ambient, lm, rows, want_stats):
        return self.native_call(self.ctx, dc.light_array(lights) if lights else None, self.env, self.dfu, self.gb, self.sdf, ambient, lm, rows[0], rows[1],
                                want_stats=want_stats)

    def render(self, which=None, ambient=None, base=None, fmt=abi.LIGHTMAP_FLOAT4, rows=(0, None), want_stats=False):
        """the lightmap after one call over the lights `which` (indices; None: all): onto `base` (uploaded, in the format's own type)
        when ambient is None, else cleared to ambient by the call.  -> (texels as downloaded, statistics triple or None)"""
        lm = native.Lightmap(self.ctx, W, H, fmt)
        try:
            if base is not None:
                lm.upload(base)
            else:
                lm.upload(lb.to_stored(ZEROS, fmt))
            st = self.call([self.lights[i] for i in (range(self.n) if which is None else which)], ambient, lm, rows, want_stats)
            return lm.download(), ((st.SdfSamples, st.PixelLightPairs, st.TracedPairs) if want_stats else None)
        finally:
            lm.close()

    def device_sources(self):
        """each light alone, added onto zeros by the additive path: 0 + c = c"""
        if self._device_sources is None:
            self._device_sources = [self.render([i])[0] for i in range(self.n)]
        return self._device_sources

    def oracle_sources(self):
        if self._oracle_sources is None:
            self._oracle_sources = [np.asarray(self.oracle_source(i), np.float32) for i in range(self.n)]
        return self._oracle_sources

    def close(self):
        for x in (self.gb, self.sdf):
            x.close()


class Sphere(LightPass):
    native_call = staticmethod(native.render_sphere_lights)

    def make_lights(self):
        return [scenes.sphere_light((9.0, 7.0, 6.0), 2.0, 9.0, color=(1.0, 0.8, 0.6, 0.9), ao_radius=4.0, ao_opacity=0.5),
                scenes.sphere_light((27.0, 13.0, 9.0), 3.0, 11.0, color=(0.3, 0.5, 1.0, 0.8)),
                scenes.sphere_light((19.0, 19.0, 5.0), 1.5, 8.0, color=(0.2, 0.9, 0.4, 1.0), specular=(0.3, 0.2, 0.1), specular_power=4.0)]

    def oracle_source(self, i):
        return self.oracle.render_sphere_lights(dc.light_array([self.lights[i]]), self.env, self.dfu, self.ogb, self.otex, (0, 0, 0, 0), W, H)[0]


class SeventeenSpheres(Sphere):
    """17 lights: the smallest count at which the light split engages (a launch of 16 or more lights)"""

    def make_lights(self):
        arr = scenes.random_lights(61, 17, W, H, z=(3.0, 10.0), radius=2.0, ramp=(5.0, 12.0))
        return [arr[i] for i in range(17)]


class Directional(LightPass):
    native_call = staticmethod(native.render_directional_lights)

    def make_lights(self):
        return [dc.directional_light(direction=(0.55, 0.3, -0.6), color=(1.0, 0.8, 0.6, 0.9), shadow_trace_length=20.0, shadow_softness=2.0,
                                     shadow_ramp_rate=0.5, ao_radius=5.0, ao_opacity=0.6),
                dc.directional_light(direction=None, bounds=(5.25, 3.5, 30.75, 20.0), color=(0.3337, 0.1113, 0.7771, 0.75)),
                dc.directional_light(direction=(0.4, -0.2, 0.25), color=(0.7, 0.1, 0.3, 1.0), shadow_trace_length=12.0, shadow_softness=1.0,
                                     bounds=(12.25, 0.0, 44.0, 15.25))]

    def oracle_source(self, i):
        return dc.render(self.oracle, [self.lights[i]], self.env, self.dfu, self.ogb, self.otex, (0, 0, 0, 0), W, H, pixels=self.pixels()).image


class Line(LightPass):
    native_call = staticmethod(native.render_line_lights)

    def make_lights(self):
        return [lc.line_light(start=(6.0, 4.5, 20.0), end=(40.0, 22.0, 14.0), radius=2.0, start_color=(1.0, 0.8, 0.6, 0.9), end_color=(0.3, 0.5, 1.0, 0.7),
                              ao_radius=5.0, ao_opacity=0.6),
                lc.line_light(start=(4.0, 20.0, 3.0), end=(26.0, 25.0, 3.0), radius=1.0, start_color=(0.2, 0.9, 0.4, 1.0), end_color=(0.9, 0.2, 0.4, 1.0))]

    def oracle_source(self, i):
        return lc.render(self.oracle, [self.lights[i]], self.env, self.dfu, self.ogb, self.otex, (0, 0, 0, 0), W, H, pixels=self.pixels()).image


class Projector(LightPass):
    native_call = staticmethod(native.render_projector_lights)
    texture = pc.texture(5, 3)

    def env_kw(self):
        return dict(maximum_z=32.0)

    def make_lights(self):
        return [pc.projector_light(pc.forward_matrix((40.0, 24.0, 64.0), (2.3, 1.6, 0.0)), origin=(24.0, 10.0, 40.0), radius=2.0, ramp_length=30.0,
                                   ao_radius=5.0, ao_opacity=0.6, opacity=0.9),
                pc.projector_light(pc.forward_matrix((16.0, 9.0, 64.0), (1.25, 0.75, 0.0)), origin=(30.0, 20.0, 35.0), radius=1.5, ramp_length=25.0,
                                   wrap=True, opacity=0.8)]

    def call(self, lights, ambient, lm, rows, want_stats):
        native.set_projector_texture(self.ctx, self.texture)
        try:
            return LightPass.call(self, lights, ambient, lm, rows, want_stats)
        finally:
            native.set_projector_texture(self.ctx, None)

    def oracle_source(self, i):
        return pc.render(self.oracle, [self.lights[i]], self.texture, self.env, self.dfu, self.ogb, self.otex, (0, 0, 0, 0), W, H, pixels=self.pixels()).image


class Volumetric(LightPass):
    native_call = staticmethod(native.render_volumetric_lights)

    def field_uniforms(self):
        return vc.field_uniforms()

    def make_lights(self):
        return list(vs.three_shapes())

    def oracle_source(self, i):
        return vc.render(self.oracle, [self.lights[i]], self.env, self.dfu, self.ogb, self.otex, (0, 0, 0, 0), W, H, pixels=self.pixels()).image


class Particle(LightPass):
    """one chunk of 64 slots with six live particles; a `light` is a live slot, a subset a copy of the state in which the others' life is 0.
    The call has no clear form: it always adds to what the lightmap holds."""
    has_clear = False
    CS = 8

    def make_lights(self):
        n = self.CS * self.CS
        self.planes = [np.zeros((n, 4), np.float32) for _ in range(5)]
        live = {3: (8.0, 6.0, 5.0), 10: (30.0, 17.0, 8.0), 11: (17.5, 12.5, 4.0), 29: (22.0, 4.0, 12.0), 40: (5.0, 20.0, 3.0), 63: (34.0, 8.0, 6.0)}
        for k, (slot, p) in enumerate(sorted(live.items())):
            self.planes[0][slot] = (p[0], p[1], p[2], 1.0 + k)
            a = 0.5 + 0.08 * k
            self.planes[3][slot] = (a * (0.9 - 0.1 * k), a * (0.3 + 0.1 * k), a * 0.5, a)      # premultiplied
        self.params = plc.particle_light_params(2.0, 9.0, (0.9, 0.8, 0.7, 0.8), casts_shadows=True, ao_radius=4.0, ao_opacity=0.5)
        self.engine = native.Engine(self.ctx, self.CS, scenes.randomness_table(7))
        self.systems = {}
        return sorted(live)

    def subset_planes(self, slots):
        planes = [p.copy() for p in self.planes]
        for s in self.lights:
            if s not in slots:
                planes[0][s, 3] = 0.0
        return planes

    def call(self, slots, ambient, lm, rows, want_stats):
        assert ambient is None
        key = tuple(slots)
        if key not in self.systems:
            sysm = native.System(self.engine)
            sysm.add_chunk()
            planes = self.subset_planes(key)
            sysm.upload(0, abi.PLANE_POSITION, planes[0])
            sysm.upload(0, abi.PLANE_RENDER_COLOR, planes[3])
            self.systems[key] = sysm
        return native.render_particle_lights(self.ctx, self.systems[key], self.params, self.env, self.dfu, self.gb, self.sdf, lm, row_begin=rows[0],
                                             row_end=rows[1], want_stats=want_stats)

    def oracle_source(self, i):
        out = np.zeros((H, W, 4), np.float32)
        self.oracle.render_particle_lights([self.subset_planes((self.lights[i],))], [self.CS * self.CS], self.params, self.env, self.dfu, self.ogb, self.otex, out)
        return out

    def close(self):
        for s in self.systems.values():
            s.close()
        self.engine.close()
        LightPass.close(self)


CLASSES = dict(sphere=Sphere, particle=Particle, directional=Directional, line=Line, projector=Projector, volumetric=Volumetric, seventeen=SeventeenSpheres)


@pytest.fixture(scope="module")
def passes(ctx, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = CLASSES[name](ctx, oracle)
        return cache[name]
    yield get
    ctx.set_light_blend_function()
    for p in cache.values():
        p.close()


class functions:
    """the context's blend functions for the duration of a block; ADD / ADD afterwards"""

    def __init__(self, ctx, color, alpha):
        self.ctx, self.pair = ctx, (color, alpha)

    def __enter__(self):
        self.ctx.set_light_blend_function(*self.pair)

    def __exit__(self, *exc):
        self.ctx.set_light_blend_function()


def base_around(total):
    """base texels above, below and equal to the contributions, by (x + y) % 3"""
    yy, xx = np.mgrid[0:H, 0:W]
    k = ((xx + yy) % 3)[..., None]
    return np.where(k == 0, total, np.where(k == 1, total * np.float32(0.5), total * np.float32(2.0) + np.float32(0.25))).astype(np.float32)


def assert_values_equal(got, want, what):
    """value equality: +0 and -0 compare equal"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %d of %d elements differ, first at %s" % (what, int((~same).sum()), same.size, tuple(np.argwhere(~same)[0]))


def additive_total(p, which=None, rows=(0, None)):
    """S: what the ADD call leaves in a lightmap of zeros"""
    return p.render(which, rows=rows)[0]


# ---- (a) the default -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PASSES)
def test_add_set_explicitly_is_the_call_without_the_setter(passes, ctx, name):
    p = passes(name)
    base = scenes.uniform(3, (H, W, 4), 0.0, 1.0)
    plain, stats = p.render(base=base, want_stats=True)
    with functions(ctx, ADD, ADD):
        again, stats2 = p.render(base=base, want_stats=True)
        no_stats, _ = p.render(base=base)
    assert_bits_equal(again, plain, "%s: ADD / ADD set explicitly" % name)
    assert_bits_equal(no_stats, plain, "%s: ADD / ADD, without statistics" % name)
    assert stats == stats2 and stats[1] > 0


# ---- (b) exactly, against the additive path --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PASSES)
def test_reverse_subtract_is_base_minus_the_additive_sum_bit_for_bit(passes, ctx, name):
    p = passes(name)
    total = additive_total(p)
    assert (total[..., 3] == 0).any() and (total[..., 3] >= 2).any(), "the frame has pixels no light reaches and pixels several do"
    base = base_around(total)
    with functions(ctx, RSUB, RSUB):
        got, _ = p.render(base=base)
        counted, _ = p.render(base=base, want_stats=True)
    assert_bits_equal(got, (base - total).astype(np.float32), "%s: base - S" % name)
    assert_bits_equal(counted, got, "%s: the counting instantiation" % name)
    assert (got[..., :3] < 0).any() and (got[..., :3] == 0).any() and (got[..., :3] > 0).any()


@pytest.mark.parametrize("function", [MAX, MIN])
@pytest.mark.parametrize("name", PASSES)
def test_max_and_min_select_over_the_single_light_renders(passes, ctx, name, function):
    p = passes(name)
    sources = p.device_sources()
    total = additive_total(p)
    base = base_around(lb.combine_fp32(ZEROS, sources, MAX, MAX))          # around the largest contribution of each pixel
    base[..., 3] = ((np.mgrid[0:H, 0:W][0] % 3) * 0.75).astype(np.float32)  # alpha 0, 0.75, 1.5 around the source alpha 1
    want = lb.combine_fp32(base, sources, function, function, total=total)
    with functions(ctx, function, function):
        got, _ = p.render(base=base)
        counted, _ = p.render(base=base, want_stats=True)
    assert_values_equal(got, want, "%s: %s / %s" % (name, lb.NAMES[function], lb.NAMES[function]))
    assert_bits_equal(counted, got, "%s: the counting instantiation" % name)
    untouched = total[..., 3] == 0
    assert_bits_equal(got[untouched], base[untouched], "%s: pixels without a contributing pair keep their base bit for bit" % name)
    assert (got != base).any() and (got == base)[~untouched].any(), "the function selects sources at some texels and the base at others"
    # colour and alpha take their own functions
    with functions(ctx, function, ADD):
        mixed, _ = p.render(base=base)
    assert_values_equal(mixed, lb.combine_fp32(base, sources, function, ADD, total=total), "%s: %s / ADD" % (name, lb.NAMES[function]))
    with functions(ctx, ADD, function):
        mixed, _ = p.render(base=base)
    assert_values_equal(mixed, lb.combine_fp32(base, sources, ADD, function, total=total), "%s: ADD / %s" % (name, lb.NAMES[function]))


# ---- (c) against the oracle ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("color,alpha", [(ADD, ADD), (RSUB, ADD), (MAX, ADD), (MIN, ADD), (RSUB, RSUB), (MAX, MAX), (MIN, MIN)])
@pytest.mark.parametrize("name", PASSES)
def test_against_the_oracles_per_light_images(passes, ctx, name, color, alpha):
    p = passes(name)
    sources = p.oracle_sources()
    base = scenes.uniform(11, (H, W, 4), 0.0, 1.25)
    total_want = lb.list_order_sum(sources, base.shape)
    want = lb.combine_fp32(base, sources, color, alpha)
    with functions(ctx, color, alpha):
        got, _ = p.render(base=base)
    what = "%s: %s / %s against the oracle" % (name, lb.NAMES[color], lb.NAMES[alpha])
    scale = np.abs(want).reshape(-1, 4).max(axis=0)
    for ch, f in enumerate(lb.channel_functions(color, alpha)):
        if f == RSUB:
            err = np.abs(got[..., ch].astype(np.float64) - want[..., ch].astype(np.float64))
            bound = lb.reverse_subtract_bound(total_want[..., ch], scale[ch], ATOL_TIGHT)
            assert (err <= bound).all(), "%s, channel %d: %d texels outside 1e-4 |S| + floor, worst %.3g over %.3g" % (
                what, ch, int((err > bound).sum()), float(err.max()), float(bound[np.unravel_index(err.argmax(), err.shape)]))
        else:
            assert_close(got[..., ch], want[..., ch], what + ", channel %d" % ch, scale=float(scale[ch]))


# ---- (d) the fp16-per-light model ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("function", NON_ADDITIVE)
@pytest.mark.parametrize("name", PASSES)
def test_the_fp16_model_is_the_chain_in_list_order(passes, ctx, name, function):
    p = passes(name)
    sources = p.device_sources()
    base = base_around(lb.combine_fp32(ZEROS, sources, MAX, MAX))
    base[..., 3] = 1.0
    ctx.set_lightmap_blend(True)
    try:
        with functions(ctx, function, function):
            got, _ = p.render(base=base)
            half4, _ = p.render(base=base.astype(np.float16), fmt=abi.LIGHTMAP_HALF4)
        with functions(ctx, function, ADD):
            mixed, _ = p.render(base=base)
    finally:
        ctx.set_lightmap_blend(False)
    assert_values_equal(got, lb.combine_fp16(base, sources, function, function), "%s: fp16 chain, %s" % (name, lb.NAMES[function]))
    assert_values_equal(mixed, lb.combine_fp16(base, sources, function, ADD), "%s: fp16 chain, %s / ADD" % (name, lb.NAMES[function]))
    assert_values_equal(half4.astype(np.float32), lb.combine_fp16(lb.half(base), sources, function, function), "%s: fp16 chain into HALF4" % name)


# ---- (e) the clear form and a strip ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("function", NON_ADDITIVE)
@pytest.mark.parametrize("name", PASSES)
def test_clear_form_and_a_strip(passes, ctx, name, function):
    p = passes(name)
    sources = p.device_sources()
    before = scenes.uniform(17, (H, W, 4), 0.0, 1.0)
    strip_total = additive_total(p, rows=(5, 21))
    assert_bits_equal(strip_total[:5], ZEROS[:5], "rows above the additive strip")
    assert_bits_equal(strip_total[21:], ZEROS[21:], "rows below the additive strip")
    with functions(ctx, function, function):
        if p.has_clear:
            cleared, _ = p.render(ambient=AMBIENT, base=before)
            nothing, _ = p.render(which=[], ambient=AMBIENT, base=before)
        strip, _ = p.render(base=before, rows=(5, 21))
        empty, _ = p.render(which=[], base=before)
    if p.has_clear:
        clear = np.broadcast_to(np.asarray(AMBIENT, np.float32), (H, W, 4))
        want = lb.combine_fp32(clear, sources, function, function, total=additive_total(p))
        (assert_bits_equal if function == RSUB else assert_values_equal)(cleared, want, "%s: clear form, %s" % (name, lb.NAMES[function]))
        assert_bits_equal(nothing, clear, "%s: ambient with no lights still clears" % name)
    assert_bits_equal(empty, before, "%s: no lights onto the lightmap: nothing changes" % name)
    want = lb.combine_fp32(before, sources, function, function, total=strip_total)
    assert_bits_equal(strip[:5], before[:5], "%s: rows above the strip" % name)
    assert_bits_equal(strip[21:], before[21:], "%s: rows below the strip" % name)
    (assert_bits_equal if function == RSUB else assert_values_equal)(strip[5:21], want[5:21], "%s: strip rows 5 .. 21, %s" % (name, lb.NAMES[function]))


# ---- (f) the other lightmap formats, (g) the statistics --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PASSES)
def test_half4_and_rgba8_store_after_the_combine(passes, ctx, name):
    p = passes(name)
    sources = p.device_sources()
    total = additive_total(p)
    before = base_around(np.minimum(total, np.float32(0.9)))
    before[..., 3] = 1.0
    for fmt, function in ((abi.LIGHTMAP_HALF4, RSUB), (abi.LIGHTMAP_RGBA8, RSUB), (abi.LIGHTMAP_HALF4, MIN), (abi.LIGHTMAP_RGBA8, MAX)):
        stored = lb.to_stored(before, fmt)
        with functions(ctx, function, function):
            got, _ = p.render(base=stored, fmt=fmt)
        want = lb.to_stored(lb.combine_fp32(lb.from_stored(stored, fmt), sources, function, function, total=total), fmt)
        assert np.array_equal(got, want), "%s: format %d, %s" % (name, fmt, lb.NAMES[function])
        if fmt == abi.LIGHTMAP_RGBA8 and function == RSUB:
            assert (got[..., :3] == 0).any() and (got[..., :3] > 0).any(), "a subtraction below zero ends at byte 0"


@pytest.mark.parametrize("name", PASSES)
def test_the_statistics_do_not_depend_on_the_functions(passes, ctx, name):
    p = passes(name)
    base = scenes.uniform(23, (H, W, 4), 0.0, 1.0)
    _, want = p.render(base=base, want_stats=True)
    assert want[1] > 0
    for color, alpha in ((RSUB, RSUB), (MAX, ADD), (MIN, MIN)):
        with functions(ctx, color, alpha):
            assert p.render(base=base, want_stats=True)[1] == want
    ctx.set_lightmap_blend(True)
    try:
        with functions(ctx, MAX, RSUB):
            assert p.render(base=base, want_stats=True)[1] == want
    finally:
        ctx.set_lightmap_blend(False)


# ---- sphere lights: the light split ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("color,alpha", [(ADD, ADD), (RSUB, RSUB), (MAX, MAX), (MIN, ADD)])
def test_seventeen_sphere_lights_give_the_same_bits_at_split_one_and_eight(passes, ctx, color, alpha):
    p = passes("seventeen")
    total = additive_total(p)
    assert total[..., 3].max() >= 3
    base = base_around(total)
    frames = {}
    try:
        for split in (1, 8):
            ctx.set_light_split(split)
            with functions(ctx, color, alpha):
                frames[split] = p.render(base=base)[0]
            if (color, alpha) == (ADD, ADD):
                assert ctx.last_light_launch()[1] == split, "17 lights engage the split"
    finally:
        ctx.set_light_split(0)
    assert_bits_equal(frames[8], frames[1], "17 sphere lights, %s / %s: split 8 against split 1" % (lb.NAMES[color], lb.NAMES[alpha]))
    want = lb.combine_fp32(base, p.device_sources(), color, alpha, total=total)
    if RSUB in (color, alpha) or (color, alpha) == (ADD, ADD):
        assert_bits_equal(frames[1][..., :3], want[..., :3], "17 sphere lights: the sum is the one ADD forms")
    assert_values_equal(frames[1], want, "17 sphere lights against the numpy rules")


# ---- a group, and the refusals -----------------------------------------------------------------------------------------------------------

def test_a_group_of_two_members_subtracts_like_one_context(passes, ctx):
    p = passes("sphere")
    lights = dc.light_array(p.lights)
    atlas = dc.field_atlas(abi.SDF_UNORM16)
    env = scenes.environment()
    with functions(ctx, RSUB, RSUB):
        lm = native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4)
        native.render_sphere_lights(ctx, lights, env, p.dfu, None, p.sdf, AMBIENT, lm)
        want = lm.download()
        lm.close()
    g = native.Group([0, 0])
    sdfs = [native.DistanceFieldTexture(c, atlas, abi.SDF_UNORM16) for c in g.contexts]
    glm = native.GroupLightmap(g, W, H, abi.LIGHTMAP_FLOAT4)
    try:
        for c in g.contexts:
            c.set_light_blend_function(RSUB, RSUB)
        g.render_sphere_lights(lights, env, p.dfu, None, sdfs, AMBIENT, glm, native.GATHER_PEER)
        g.sync()
        assert len(glm.strips) == 2
        for i in range(2):
            assert_bits_equal(glm.download(i), want, "member %d's frame" % i)
    finally:
        glm.close()
        for s in sdfs:
            s.close()
        g.close()
    assert (want[..., :3] < np.asarray(AMBIENT, np.float32)[:3]).any(), "the group darkened the clear colour"


def test_unknown_functions_are_refused_and_leave_the_state(passes, ctx):
    p = passes("directional")
    lib = native.lib()
    base = scenes.uniform(29, (H, W, 4), 0.0, 1.0)
    with functions(ctx, MAX, RSUB):
        want, _ = p.render(base=base)
        for color, alpha in ((4, ADD), (-1, ADD), (ADD, 4), (MIN, -1), (1 << 16, ADD)):
            assert lib.ilm_ctx_set_light_blend_function(ctx.handle, color, alpha) == abi.ERR_INVALID_ARGUMENT
            assert b"blend function" in lib.ilm_last_error()
        assert lib.ilm_ctx_set_light_blend_function(abi.Handle(0), MAX, MAX) == abi.ERR_INVALID_HANDLE
        got, _ = p.render(base=base)
    assert_bits_equal(got, want, "the call after the refusals renders with the state before them")
    assert_values_equal(want, lb.combine_fp32(base, p.device_sources(), MAX, RSUB, total=additive_total(p)), "MAX / REVERSE_SUBTRACT")
