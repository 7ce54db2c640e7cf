"""ilm_render_volumetric_lights restated in numpy float32: the two pixel shaders (VolumetricLight.fx:7-51, ShadowedVolumetricLight.fx:7-52)
over VolumetricLightPixelCore, volumetricTrace, eval, sdEllipsoid, sdRoundCone, sdBox and VolumetricLightVertexShader
(VolumetricLightCore.fxh:25-54,85-88,281-298,315-549), computeNormalFactorEx (LightCommon.fxh:154-165), computeAO (AOCommon.fxh:1-19) and the
entry point's contract (coverage, discards, blend models, stores, statistics, the loop guard) as the header states it.

The G-buffer decode and every distance come from the oracle library (oracle.sample_gbuffer, oracle.sample_distance_field).  Everything
else is the header's defined arithmetic, operation for operation: one float32 rounding per +, -, *, /, sqrt in the order the HLSL writes
it, Dither17 as the header defines it, and libm's fmaf where the device code fuses on purpose: the march's sample position from + along *
d.  Only power() (directional_common: pow in double, rounded once) may differ from the kernel, within the suite's criterion.

Per pair the restatement keeps a `detail` record: shape, the column's iterations, the march's samples per column point and how each march
ended ("hit", "end": d >= md, "count": the counter), hits, diffuse, the return branch and the opacity.

Shared by tests/test_volumetric_kat.py (no GPU), tests/test_volumetric_gpu.py and tests/test_host_volumetric_gpu.py.
"""
import numpy as np

from illuminant_amd import scenes
from tests import directional_common as dc
from tests.directional_common import (F, fmaf, sat, power, light_array, half, to_stored, from_stored, decode_pixels, Result,  # noqa: F401
                                      covers, DOT_EXPONENT)

# VolumetricLightCore.fxh:15-17,87,327,361,388,469; LightCommon.fxh:5-6
ELLIPSOID, CONE, BOX = scenes.VOLUMETRIC_ELLIPSOID, scenes.VOLUMETRIC_CONE, scenes.VOLUMETRIC_BOX
DOT_OFFSET = F(0.15)
DOT_RAMP_RANGE = F(0.15)
CONE_DOT = F(0.33)
BOX_FLOOR = F(0.0001)
PROJECT_THRESHOLD = F(0.01)
DITHER_SCALE = F(0.66)
STEP_SCALE = F(0.99)
HIT = F(-0.1)
LOOP_GUARD = 4
MAX_STEP_COUNT_LIMIT = 4096

volumetric_light = scenes.volumetric_light      # RenderVolumetricLightSource's packing


def dither17(x, y):
    """the header's Dither17 at f = 0.5: k = 2 x + 7 y + 11.5 (exact), k mod 17 (exact), one division"""
    k = F(F(F(2) * F(x)) + F(F(7) * F(y))) + F(11.5)
    return F(F(np.fmod(F(k), F(17))) / F(17))


def sgn(x):
    return F(1) if x > 0 else (F(-1) if x < 0 else F(0))


def lerp(a, b, t):
    return F(a + F(F(b - a) * t))


def dot3(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def len3(a):
    return F(np.sqrt(dot3(a, a)))


def sd_ellipsoid(p, r):
    """sdEllipsoid, :25-29"""
    with np.errstate(all="ignore"):
        rr = [F(c * c) for c in r]
        k0 = len3([F(p[k] / r[k]) for k in range(3)])
        k1 = len3([F(p[k] / rr[k]) for k in range(3)])
        return F(F(k0 * F(k0 - F(1))) / k1)


def sd_round_cone(p, a, b, r1, r2, branch=None):
    """sdRoundCone, :31-54; branch: a list that receives which return was taken (2: the far cap, 1: the near cap, 0: the side)"""
    with np.errstate(all="ignore"):
        ba = [F(b[k] - a[k]) for k in range(3)]
        l2 = dot3(ba, ba)
        rr = F(r1 - r2)
        a2 = F(l2 - F(rr * rr))
        il2 = F(F(1) / l2)
        pa = [F(p[k] - a[k]) for k in range(3)]
        y = dot3(pa, ba)
        z = F(y - l2)
        v = [F(F(pa[k] * l2) - F(ba[k] * y)) for k in range(3)]
        x2 = dot3(v, v)
        y2 = F(F(y * y) * l2)
        z2 = F(F(z * z) * l2)
        k = F(F(F(sgn(rr) * rr) * rr) * x2)
        if F(F(sgn(z) * a2) * z2) > k:
            which, out = 2, F(F(F(np.sqrt(F(x2 + z2))) * il2) - r2)
        elif F(F(sgn(y) * a2) * y2) < k:
            which, out = 1, F(F(F(np.sqrt(F(x2 + y2))) * il2) - r1)
        else:
            which, out = 0, F(F(F(F(np.sqrt(F(F(x2 * a2) * il2))) + F(y * rr)) * il2) - r1)
    if branch is not None:
        branch.append(which)
    return out


def sd_box(p, b):
    """sdBox, :85-88"""
    with np.errstate(all="ignore"):
        d = [F(np.abs(p[k]) - b[k]) for k in range(3)]
        m = [np.fmax(c, BOX_FLOOR) for c in d]
        return F(len3(m) + np.fmin(np.fmax(np.fmax(d[0], d[1]), d[2]), BOX_FLOOR))


class Record:
    """what prepare_volumetric_lights_kernel computes once per light, with the same roundings"""


def shape_of(light):
    return int(light.EvenMoreLightProperties.w)


def prepare(light, env):
    r = Record()
    with np.errstate(all="ignore"):
        r.shape = shape_of(light)
        assert F(light.EvenMoreLightProperties.w) in (F(0), F(1), F(2)), "the entry point refuses every other shape"
        r.start = [F(light.LightPosition1.x), F(light.LightPosition1.y), F(light.LightPosition1.z)]
        r.end = [F(light.LightPosition2.x), F(light.LightPosition2.y), F(light.LightPosition2.z)]
        r.r1, r.r2 = F(light.LightPosition1.w), F(light.LightPosition2.w)
        s, e = r.start, r.end
        if r.shape == CONE:
            m = np.fmax(r.r1, r.r2)
            p1 = [F(np.fmin(s[k], e[k]) - m) for k in range(3)]
            p2 = [F(np.fmax(s[k], e[k]) + m) for k in range(3)]
            r.z_hi, r.z_lo = p2[2], p1[2]
            r.md = len3([F(e[k] - s[k]) for k in range(3)])
        else:
            p1 = [F(s[k] - e[k]) for k in range(3)]
            p2 = [F(s[k] + e[k]) for k in range(3)]
            r.z_hi, r.z_lo = p2[2], p1[2]
            r.md = len3(e)
        r.world = (np.fmin(p1[0], p2[0]), np.fmin(p1[1], p2[1]), np.fmax(p1[0], p2[0]), np.fmax(p1[1], p2[1]))
        sx = F(F(env.GBufferTexelSizeAndMisc.z) * F(env.ZAndScale.z))
        sy = F(F(env.GBufferTexelSizeAndMisc.w) * F(env.ZAndScale.w))
        vx, vy = F(env.ViewportPosition[0]), F(env.ViewportPosition[1])
        r.footprint = (F(F(r.world[0] - vx) * sx), F(F(r.world[1] - vy) * sy), F(F(r.world[2] - vx) * sx), F(F(r.world[3] - vy) * sy))
        ray = [F(light.LightPosition3.x), F(light.LightPosition3.y), F(light.LightPosition3.z)]
        r.project = bool(len3(ray) < PROJECT_THRESHOLD)
        r.trace = [F(c * r.md) for c in ray]
        r.full_att = F(r.md * F(light.EvenMoreLightProperties.z))
        r.w = F(light.LightProperties.w)
        r.volumetricity, r.ramp_length = F(light.LightProperties.x), F(light.LightProperties.y)
        r.blowout, r.ramp_power = F(light.EvenMoreLightProperties.x), F(light.EvenMoreLightProperties.y)
        r.ao_radius, r.ao_opacity = F(light.MoreLightProperties.x), F(light.MoreLightProperties.w)
        a = F(light.Color1.w)
        r.color = (F(F(light.Color1.x) * a), F(F(light.Color1.y) * a), F(F(light.Color1.z) * a))
    return r


def evaluate(r, pos, branch=None):
    """eval, :281-298"""
    if r.shape == ELLIPSOID:
        return sd_ellipsoid([F(pos[k] - r.start[k]) for k in range(3)], r.end)
    if r.shape == CONE:
        return sd_round_cone(pos, r.start, r.end, r.r1, r.r2, branch)
    return sd_box([F(pos[k] - r.start[k]) for k in range(3)], r.end)


def march(sample, r, pos, dither, dfu):
    """the inner march of volumetricTrace (:359-399) from one column point with a bound field.  Returns (occlusion, samples, how it
    ended: "hit", "end" or "count")."""
    with np.errstate(all="ignore"):
        if r.project:
            along = [F(pos[k] - r.start[k]) for k in range(3)]
            start = list(r.start)
            md = len3(along)
        else:
            along = list(r.trace)
            start = [F(pos[k] - along[k]) for k in range(3)]
            md = r.md
        along = [F(c / md) for c in along]
    for k in range(3):          # (the sampler reads a NaN coordinate as 0: such an axis is from = along = 0, as the kernel hoists it)
        if np.isnan(start[k]) or np.isnan(along[k]):
            start[k], along[k] = F(0), F(0)
    d = F(dither * DITHER_SCALE)
    remaining = int(F(dfu.StepAndMisc2.x))
    min_step = F(dfu.Packed1.w)
    occlusion, samples, ended = F(1), 0, "count"
    while remaining > 0:
        s = F(sample([fmaf(along[k], d, start[k]) for k in range(3)]))
        samples += 1
        occlusion = sat(F(s * F(0.5)))
        hit = s <= HIT
        if hit:
            remaining, occlusion, ended = 0, F(0), "hit"
        d = F(d + np.fmax(F(np.abs(s) * STEP_SCALE), min_step))
        if d >= md:
            remaining = 0
            ended = "hit" if hit else "end"
        else:
            remaining -= 1
    return occlusion, samples, ended


def trace(sample, r, shaded, x, y, env, dfu, marches, facts):
    """volumetricTrace, :315-409.  marches: traceShadows with a bound field."""
    steps = F(dfu.StepAndMisc2.x)
    assert 1 <= steps <= MAX_STEP_COUNT_LIMIT, "the entry point refuses every other MaxStepCount"
    with np.errstate(all="ignore"):
        z2 = np.fmax(F(shaded[2]), F(env.ZAndScale.x))
        z1 = np.fmax(F(env.ZAndScale.y), z2)
        z1 = np.fmin(z1, r.z_hi)
        z2 = np.fmax(z2, r.z_lo)
        step = F(np.fmax(np.abs(F(z2 - z1)), F(1)) / steps)
        dither = dither17(x, y)
        z = F(z1 + F(dither * step))
    hits = F(0)
    guard = int(steps) + LOOP_GUARD
    iterations, samples, per_point, ends, branches = 0, 0, [], [], []
    while True:
        iterations += 1
        pos = [F(shaded[0]), F(shaded[1]), z]
        sd = evaluate(r, pos, branches)
        occlusion = F(1)
        if marches:
            occlusion, n, ended = march(sample, r, pos, dither, dfu)
            samples += n
            per_point.append(n)
            ends.append(ended)
        with np.errstate(all="ignore"):
            ramp = power(sat(F(F(-sd) / r.ramp_length)), r.ramp_power)
            hits = F(hits + F(ramp * occlusion))
            z = F(z - step)
        guard -= 1
        if not ((z >= z2) and (guard > 0)):
            break
    with np.errstate(all="ignore"):
        opacity = sat(F(F(hits / steps) / r.volumetricity))
    facts.update(iterations=iterations, march_samples=tuple(per_point), march_ends=tuple(ends), hits=hits, volumetric=opacity, z1=z1, z2=z2,
                 step=step, dither=dither, guard_left=guard, column_branches=tuple(branches))
    return opacity, samples


def shade(sample, pixel, x, y, r, env, dfu, have_field):
    """One light on one decoded G-buffer texel inside its footprint.  Returns None when the shader discards, else (opacity, samples,
    traced, facts)."""
    shaded, normal, enable_shadows, fullbright = pixel
    if fullbright:
        return None
    shaded = [F(c) for c in shaded]
    normal = [F(c) for c in normal]
    if not (shaded[0] > F(-9999)):
        return None
    samples = 0
    ao = F(1)
    ao_radius = F(r.ao_radius * np.fmax(F(0), normal[2]))
    if ao_radius >= F(0.5) and have_field:
        distance = F(sample((shaded[0], shaded[1], F(shaded[2] + F(normal[2] * ao_radius)))))
        samples += 1
        t = F(F(1) - sat(F(np.fmin(np.fmax(distance, F(0)), ao_radius) / ao_radius)))
        t = F(t * t)
        t = F(F(1) - t)
        ao = F(F(F(1) - r.ao_opacity) + F(t * r.ao_opacity))
    with np.errstate(all="ignore"):
        casts = F(r.w * (F(1) if enable_shadows else F(0))) != 0
    trace_shadows = bool(casts and F(dfu.Extent.z) > 0)
    marches = trace_shadows and have_field
    facts = {"shape": r.shape, "ao": ao, "trace_shadows": trace_shadows}
    volumetric, n = trace(sample, r, shaded, x, y, env, dfu, marches, facts)
    samples += n
    with np.errstate(all="ignore"):
        pre_trace = F(ao * volumetric)
        cone_dot = F(np.fmax(r.r1, r.r2) / F(64)) if r.shape == CONE else F(0)
        dot_range, dot_offset = lerp(DOT_RAMP_RANGE, CONE_DOT, cone_dot), lerp(DOT_OFFSET, CONE_DOT, cone_dot)
        to_point = [F(shaded[k] - r.start[k]) for k in range(3)]
        distance = len3(to_point)
        normal_opacity = F(1)
        if any(c != 0 for c in normal):
            light_normal = [F(c / distance) for c in to_point]
            d = dot3([F(c * F(-1)) for c in light_normal], normal)
            normal_opacity = power(sat(F(F(d + dot_offset) / dot_range)), DOT_EXPONENT)
        normal_opacity = lerp(normal_opacity, F(F(normal_opacity * F(2)) - F(1)), r.blowout)
        branch = []
        contact = evaluate(r, shaded, branch)
        shape_opacity = power(sat(F(F(-contact) / r.ramp_length)), r.ramp_power) if contact < 0 else F(0)
        distance_opacity = F(F(1) - sat(F(distance / r.full_att)))
        diffuse = F(F(normal_opacity * shape_opacity) * distance_opacity)
        if diffuse < 0:
            opacity, which = F(pre_trace + diffuse), "sum"
        else:
            opacity, which = np.fmax(pre_trace, diffuse), "max"
    facts.update(pre_trace=pre_trace, normal_opacity=normal_opacity, contact=contact, shape_opacity=shape_opacity,
                 distance_opacity=distance_opacity, diffuse=diffuse, returned=which, opacity=opacity, contact_branch=tuple(branch))
    if opacity <= 0:
        facts["discarded"] = True
        return None, samples, marches, facts
    return opacity, samples, marches, facts


def render(oracle, lights, env, dfu, gbuffer, sdf, ambient, width, height, row_begin=0, row_end=None, blend_fp16=False, before=None, pixels=None):
    """The whole call.  ambient None: the lights are added to `before` ((H, W, 4) float32: the lightmap's texels as the pass reads them
    back); else rows [row_begin, row_end) start from ambient and the other rows keep `before` (zeros when None).  pixels:
    decode_pixels(...) of the scene, to share among calls.  detail holds every pair that reached the core, discarded ones included
    (facts["discarded"])."""
    row_end = height if row_end is None else row_end
    image = np.zeros((height, width, 4), np.float32) if before is None else np.array(before, np.float32, copy=True)
    have_field = sdf is not None and F(dfu.Extent.x) > 0
    if pixels is None:
        pixels = decode_pixels(oracle, env, gbuffer, width, height)

    def sample(p):
        return oracle.sample_distance_field(p, dfu, sdf)

    prepared = [prepare(l, env) for l in lights]
    out = Result()
    out.detail = {}
    n_samples = n_pairs = n_traced = 0
    for y in range(row_begin, row_end):
        for x in range(width):
            base = np.asarray(ambient, np.float32) if ambient is not None else image[y, x].copy()
            if blend_fp16:
                base = half(base)
            acc = [base[k] for k in range(4)] if blend_fp16 else [F(0)] * 4
            for i, r in enumerate(prepared):
                if not covers(r.footprint, x, y):
                    continue
                n_pairs += 1
                shaded = shade(sample, pixels[y * width + x], x, y, r, env, dfu, have_field)
                if shaded is None:
                    continue
                opacity, n, traced, facts = shaded
                n_samples += n
                n_traced += 1 if traced else 0
                out.detail[(x, y, i)] = facts
                if opacity is None:
                    continue
                c = [F(r.color[0] * opacity), F(r.color[1] * opacity), F(r.color[2] * opacity), F(1)]
                if blend_fp16:
                    acc = [half(F(acc[k] + half(c[k]))) for k in range(4)]
                else:
                    acc = [F(acc[k] + c[k]) for k in range(4)]
            image[y, x] = acc if blend_fp16 else [F(base[k] + acc[k]) for k in range(4)]
    out.image = image
    out.stats = (n_samples, n_pairs, n_traced)
    return out


# ---- the scene of the tests: directional_common's frame, field and G-buffer, with a short step budget --------------------------------
# (a pair costs up to (MaxStepCount + 1) * MaxStepCount samples: 72 at 8)

WIDTH, HEIGHT = dc.WIDTH, dc.HEIGHT
MAX_STEP_COUNT = 8
field_layout, field_atlas, gbuffer_texels = dc.field_layout, dc.field_atlas, dc.gbuffer_texels
ramp_texture = dc.ramp_texture
INVISIBLE_VIEWPORT = dc.INVISIBLE_VIEWPORT


def field_uniforms(step_limit=MAX_STEP_COUNT, **kw):
    return dc.field_uniforms(step_limit=step_limit, **kw)


def no_field_uniforms(step_limit=MAX_STEP_COUNT):
    return dc.no_field_uniforms(step_limit=step_limit)
