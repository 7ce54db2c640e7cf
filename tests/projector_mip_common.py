"""The projector pass's fetch over a mip chain restated in numpy float32, on top of tests/projector_common.py: the explicit LOD of
tex2Dlod(ProjectorTextureSampler, (u, v, 0, lod)) with MipFilter LINEAR, as the header states it under ilm_render_projector_lights --

    c = fminf(fmaxf(lod, 0), L - 1);  l0 = (int)floorf(c);  f = c - floorf(c);  l1 = min(l0 + 1, L - 1)
    c0 = the bilinear WRAP fetch on level l0;  f == 0: the texel is c0 and level l1 is not read
    otherwise c1 = the same fetch on level l1 and the texel is c0 + (c1 - c0) * f per component

with one float32 rounding per operation.  A chain is a list of (h, w, 4) float32 levels, level l being max(1, h >> l) x max(1, w >> l).

Shared by tests/test_projector_mips_kat.py (no GPU), tests/test_projector_mips_gpu.py and tests/test_host_projector_mips_gpu.py.
"""
import functools

import numpy as np

from illuminant_amd import scenes
from tests import projector_common as pc

F = np.float32

ONES = np.ones((1, 1, 4), np.float32)
ONES.setflags(write=False)


def level_sizes(width, height, levels):
    """[(w, h)] of the levels of a width x height texture"""
    return [(max(1, width >> l), max(1, height >> l)) for l in range(levels)]


def resolve_lod(lod, levels):
    """(l0, l1, f) of an LOD over a chain of `levels` levels.  np.fmax / np.fmin are fmaxf / fminf: a NaN operand loses."""
    with np.errstate(all="ignore"):
        c = np.fmin(np.fmax(F(lod), F(0)), F(levels - 1))
        whole = F(np.floor(c))
        f = F(c - whole)
    l0 = int(whole)
    return l0, min(l0 + 1, levels - 1), f


def fetch_lod(chain, u, v, lod, fetch=pc.fetch):
    """the four components of the texel at (u, v) and `lod`"""
    l0, l1, f = resolve_lod(lod, len(chain))
    c0 = fetch(chain[l0], u, v)
    if f == 0:
        return c0
    c1 = fetch(chain[l1], u, v)
    with np.errstate(all="ignore"):
        return [pc.lerp(c0[k], c1[k], f) for k in range(4)]


def geometry_key(light):
    """a light without its LOD: Color2.w is the vertex's last float, and nothing but the fetch reads it (pc.matrix_rows puts m44 = 1 there)"""
    return bytes(light)[:-4]


def render(oracle, lights, chain, env, dfu, gbuffer, sdf, ambient, width, height, row_begin=0, row_end=None, blend_fp16=False, before=None,
           pixels=None, cache=None):
    """tests/projector_common.render over a chain.  Each light's opacity comes from pc.shade with a 1 x 1 texture of ones -- there the
    rgb it returns is the opacity exactly, (1 * 1) * o == o -- and multiplies the texel fetched at the pair's (u, v) and the light's LOD
    (Color2.w) in the kernel's order, (t.k * t.a) * opacity.  Statistics as pc.render: texture taps are not counted.  `cache`: a dict a
    test hands to the renders of ONE scene (env, dfu, field, pixels) to share what does not depend on the LOD -- a pair's opacity and
    (u, v), and a level's bilinear fetch at them -- between its LODs; values are computed once and never changed."""
    row_end = height if row_end is None else row_end
    image = np.zeros((height, width, 4), np.float32) if before is None else np.array(before, np.float32, copy=True)
    have_field = sdf is not None and F(dfu.Extent.x) > 0
    if pixels is None:
        pixels = pc.decode_pixels(oracle, env, gbuffer, width, height)

    def sample(p):
        return oracle.sample_distance_field(p, dfu, sdf)

    prepared = [(pc.footprint(l, env), pc.matrix_rows(l)) for l in lights]
    cache = {} if cache is None else cache
    shades, fetches = cache.setdefault("shade", {}), cache.setdefault("fetch", {})

    def fetch(level, u, v):
        key = (id(level), level.shape, F(u).tobytes(), F(v).tobytes())
        if key not in fetches:
            fetches[key] = (level, pc.fetch(level, u, v))        # (the level is held: its id stays its own)
        return fetches[key][1]

    out = pc.Result()
    out.detail = {}
    n_samples = n_pairs = n_traced = 0
    for y in range(row_begin, row_end):
        for x in range(width):
            base = np.asarray(ambient, np.float32) if ambient is not None else image[y, x].copy()
            if blend_fp16:
                base = pc.half(base)
            acc = [base[k] for k in range(4)] if blend_fp16 else [F(0)] * 4
            for i, l in enumerate(lights):
                fp, rows = prepared[i]
                if not pc.covers(fp, x, y):
                    continue
                n_pairs += 1
                key = (geometry_key(l), x, y, have_field)
                if key not in shades:
                    shades[key] = pc.shade(sample, pixels[y * width + x], l, rows, dfu, have_field, ONES)
                if shades[key] is None:
                    continue
                (opacity, _, _), n, traced, facts = shades[key]
                facts = dict(facts)
                assert opacity == facts["opacity"] or (np.isnan(opacity) and np.isnan(facts["opacity"]))
                n_samples += n
                n_traced += 1 if traced else 0
                t = fetch_lod(chain, facts["uv"][0], facts["uv"][1], l.Color2.w, fetch)
                facts["texel"] = t
                out.detail[(x, y, i)] = facts
                with np.errstate(all="ignore"):
                    c = [F(F(t[k] * t[3]) * opacity) for k in range(3)] + [F(1)]
                    if blend_fp16:
                        acc = [pc.half(F(acc[k] + pc.half(c[k]))) for k in range(4)]
                    else:
                        acc = [F(acc[k] + c[k]) for k in range(4)]
            with np.errstate(all="ignore"):
                image[y, x] = acc if blend_fp16 else [F(base[k] + acc[k]) for k in range(4)]
    out.image = image
    out.stats = (n_samples, n_pairs, n_traced)
    return out


@functools.lru_cache(maxsize=None)
def chain(width, height, levels):
    """a chain of UNRELATED levels (no box filter: level l is a texture of its own, every texel different, alpha 0.5 .. 1), so that a
    wrong level, a wrong weight or a wrong level size shows.  Level 0 is pc.texture(width, height)."""
    out = [pc.texture(width, height)]
    for l, (w, h) in enumerate(level_sizes(width, height, levels)[1:], start=1):
        t = scenes.uniform(5000 + 97 * l + width * 31 + height, (h, w, 4), 0.1, 1.0)
        t[..., 3] = 0.5 + 0.5 * t[..., 3]
        t.setflags(write=False)
        out.append(t)
    return tuple(out)
