"""Scenes of ilm_engine_render_particle_lights_batch and their expected frames.

The expected frame is the existing oracle, chained: oracle.render_particle_lights accumulates into the lightmap it is given, so it is
called item after item on one array and its statistics are summed.  A chain is computed once per (scene, field format, G-buffer) and
handed out as copies."""
import numpy as np

from illuminant_amd import abi, native, scenes
from tests import light_blend_common as lb
from tests import lights_common as lc
from tests.test_lights_ext_gpu import particle_scene, small_field

AMBIENT = (0.05, 0.06, 0.07, 1.0)        # a clear colour; 0.05 / 0.06 / 0.07 are no halves ...
HALF_AMBIENT = tuple(float(np.float16(x)) for x in AMBIENT)      # ... these are: the starting contents of the half tests
_RND = scenes.randomness_table(7)


class Item:
    """One entry of a batch: `system` indexes the scene's systems, whose first `chunk_count` chunks take part with `quads` (None: every slot)"""

    def __init__(self, system, chunk_count, quads, params):
        self.system, self.chunk_count, self.quads, self.params = system, chunk_count, quads, params


class Scene:
    def __init__(self, name, width, height, cs, systems, items):
        self.name, self.width, self.height, self.cs, self.systems, self.items = name, width, height, cs, systems, items
        self.slots = cs * cs

    def quads_of(self, item):
        return list(item.quads) if item.quads is not None else [self.slots] * item.chunk_count

    def emitting(self, item):
        """records the item emits, from the planes: life > 0 and a render colour whose alpha x LightColor.a is above 0, below the quad count"""
        n = 0
        for planes, q in zip(self.systems[item.system][:item.chunk_count], self.quads_of(item)):
            n += int(((planes[0][:q, 3] > 0) & (planes[3][:q, 3] * np.float32(item.params.LightColor.w) > 0)).sum())
        return n


_SCENES = {}


def mixed_scene():
    """70 x 45 (partial tiles on both rims), chunks of 144 slots (no power of two, less than one workgroup); six items of 0, 1, 3, 2, 6
    and 1 chunks, each with its own template; item 3 is all dead, item 4 passes six of its system's seven chunks, items 1 and 5 are the
    same system under different templates; every item's last chunk is cut to 100 quads."""
    if "mixed" not in _SCENES:
        w, h, cs = 70, 45, 12
        systems = [[],
                   particle_scene(cs, 1, w, h, seed=211, dead_fraction=0.3),
                   particle_scene(cs, 3, w, h, seed=223, dead_fraction=0.4),
                   particle_scene(cs, 2, w, h, seed=239, dead_fraction=0.3),
                   particle_scene(cs, 7, w, h, seed=251, dead_fraction=0.5)]
        for planes in systems[3]:
            planes[0][:, 3] = np.where(np.arange(cs * cs) % 2 == 0, 0.0, -1.5).astype(np.float32)      # all dead: life 0 or below
        colors = [(1.0, 1.0, 1.0, 1.0), (0.9, 0.8, 0.7, 0.6), (0.5, 0.9, 1.0, 0.8), (1.0, 0.4, 0.3, 1.0), (0.7, 0.7, 1.0, 0.5), (0.3, 1.0, 0.6, 0.9)]
        items = []
        for i, (system, chunk_count) in enumerate(((0, 0), (1, 1), (2, 3), (3, 2), (4, 6), (1, 1))):
            params = lc.particle_light_params(1.0 + 0.5 * i, 4.0 + i, colors[i], casts_shadows=(i % 2 == 0),
                                              ao_radius=5.0 if i == 2 else 0.0, ao_opacity=0.6 if i == 2 else 0.0,
                                              spec=(0.3, 0.2, 0.1) if i == 4 else (0, 0, 0), spec_power=3.0 if i == 4 else 1.0)
            quads = [cs * cs] * (chunk_count - 1) + [100] if chunk_count else []
            items.append(Item(system, chunk_count, quads, params))
        _SCENES["mixed"] = Scene("mixed", w, h, cs, systems, items)
    return _SCENES["mixed"]


CROWDED_PARAMS = dict(radius=1.0, ramp=3.0, casts_shadows=True)


def crowded_scene():
    """64 x 48, chunks of 1 600 slots; four chunks split over three items as 1 + 2 + 1 under ONE template, and system 3 holds all four
    (the single call the split batch must equal); more records than one wide list batch of the tile kernel (4 096)"""
    if "crowded" not in _SCENES:
        w, h, cs = 64, 48, 40
        chunks = particle_scene(cs, 4, w, h, seed=5, dead_fraction=0.05)
        params = lc.particle_light_params(CROWDED_PARAMS["radius"], CROWDED_PARAMS["ramp"], casts_shadows=CROWDED_PARAMS["casts_shadows"])
        systems = [chunks[0:1], chunks[1:3], chunks[3:4], chunks]
        items = [Item(0, 1, None, params), Item(1, 2, None, params), Item(2, 1, None, params)]
        _SCENES["crowded"] = Scene("crowded", w, h, cs, systems, items)
    return _SCENES["crowded"]


def scene(name):
    return mixed_scene() if name == "mixed" else crowded_scene()


_FIELDS = {}


def field(sfmt=abi.SDF_UNORM16):
    if sfmt not in _FIELDS:
        _FIELDS[sfmt] = small_field(sfmt)
    return _FIELDS[sfmt]


def gbuffer_texels(width, height):
    """smooth normals and heights with a fullbright band (discarded pixels) across rows 10 .. 13"""
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
    nx = 0.3 * np.sin(xx / 9.0); ny = 0.3 * np.cos(yy / 7.0)
    nz = np.sqrt(np.maximum(1.0 - nx * nx - ny * ny, 0.0))
    z = 6.0 + 5.0 * np.sin(xx / 17.0) * np.cos(yy / 13.0)
    g = scenes.encode_gbuffer(np.stack([nx, ny, nz], axis=-1), 0.0, z)
    g[10:14, :, 3] = 99999.0
    return np.ascontiguousarray(g)


def environment(sc, with_gbuffer=False):
    return scenes.environment(gbuffer_size=(sc.width, sc.height)) if with_gbuffer else scenes.environment()


def ambient_frame(sc, rgba=AMBIENT):
    base = np.zeros((sc.height, sc.width, 4), np.float32)
    base[:] = np.asarray(rgba, np.float32)
    return base


_CHAINS = {}


def chained_oracle(oracle, sc, sfmt=abi.SDF_UNORM16, with_gbuffer=False, items=None, ambient=AMBIENT):
    """-> (frame, (SdfSamples, PixelLightPairs, TracedPairs)): the oracle's particle-light pass item after item onto the ambient frame.
    `items`: indices into the scene's items (None: all)"""
    key = (sc.name, sfmt, with_gbuffer, None if items is None else tuple(items), tuple(float(x) for x in ambient))
    if key not in _CHAINS:
        atlas, dfu = field(sfmt)
        otex = oracle.make_texture(atlas, sfmt)
        ogb = oracle.make_texture(gbuffer_texels(sc.width, sc.height), abi.GBUFFER_FLOAT4) if with_gbuffer else None
        env = environment(sc, with_gbuffer)
        want = ambient_frame(sc, ambient)
        total = [0, 0, 0]
        for i in (range(len(sc.items)) if items is None else items):
            item = sc.items[i]
            if item.chunk_count == 0:
                continue
            st = oracle.render_particle_lights(sc.systems[item.system][:item.chunk_count], sc.quads_of(item), item.params, env, dfu, ogb, otex, want,
                                               want_stats=True)
            total = [a + b for a, b in zip(total, (st.SdfSamples, st.PixelLightPairs, st.TracedPairs))]
        _CHAINS[key] = (want, tuple(int(x) for x in total))
    want, total = _CHAINS[key]
    return want.copy(), total


class Device:
    """A scene's engine and systems on the device, with the frame's field (and G-buffer)"""

    def __init__(self, ctx, sc, sfmt=abi.SDF_UNORM16, with_gbuffer=False):
        self.ctx, self.scene = ctx, sc
        self.engine = native.Engine(ctx, sc.cs, _RND)
        self.systems = []
        for chunks in sc.systems:
            s = native.System(self.engine)
            for c, planes in enumerate(chunks):
                s.add_chunk()
                s.upload(c, abi.PLANE_POSITION, planes[0])
                s.upload(c, abi.PLANE_RENDER_COLOR, planes[3])
            self.systems.append(s)
        atlas, self.dfu = field(sfmt)
        self.sdf = native.DistanceFieldTexture(ctx, atlas, sfmt)
        self.gb = native.GBufferTexture(ctx, gbuffer_texels(sc.width, sc.height), abi.GBUFFER_FLOAT4) if with_gbuffer else None
        self.env = environment(sc, with_gbuffer)

    def items(self, which=None):
        """the (system, params, quad_counts, chunk_count) tuples Engine.render_particle_lights_batch takes"""
        sc = self.scene
        return [(self.systems[it.system], it.params, it.quads, it.chunk_count) for it in (sc.items if which is None else [sc.items[i] for i in which])]

    def lightmap(self, fmt=abi.LIGHTMAP_FLOAT4, base=None):
        """a lightmap holding `base` (a float32 frame; None: the ambient frame) after the format's store conversion"""
        lm = native.Lightmap(self.ctx, self.scene.width, self.scene.height, fmt)
        lm.upload(lb.to_stored(ambient_frame(self.scene) if base is None else base, fmt))
        return lm

    def batch(self, lm, which=None, rows=(0, None), want_stats=False):
        return self.engine.render_particle_lights_batch(self.items(which), self.env, self.dfu, self.gb, self.sdf, lm, rows[0], rows[1], want_stats)

    def loop(self, lm, which=None, rows=(0, None), want_stats=False):
        """the K single calls in item order -> the summed statistics"""
        total = [0, 0, 0]
        for system, params, quads, chunk_count in self.items(which):
            st = native.render_particle_lights(self.ctx, system, params, self.env, self.dfu, self.gb, self.sdf, lm, quad_counts=quads,
                                               chunk_count=chunk_count, row_begin=rows[0], row_end=rows[1], want_stats=want_stats)
            if want_stats:
                total = [a + b for a, b in zip(total, (st.SdfSamples, st.PixelLightPairs, st.TracedPairs))]
        return tuple(total)

    def close(self):
        for x in [self.sdf] + ([self.gb] if self.gb is not None else []) + self.systems + [self.engine]:
            x.close()


def stats_triple(st):
    return (int(st.SdfSamples), int(st.PixelLightPairs), int(st.TracedPairs))
