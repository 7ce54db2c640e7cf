"""ilm_render_line_lights restated in numpy float32: LineLightPixelShader (LineLight.fx:7-42) over LineLightPixelCore and lineConeTrace
(LineLightCore.fxh:17-120), computeLineLightOpacity / rectangleSolidAngle (FBPBR.fxh:33-101), closestPointOnLineSegment3
(DistanceFieldCommon.fxh:151-155), computeAO (AOCommon.fxh:1-19), coneTraceInitialize / coneTraceStep / coneTraceAdvanceEx / createTraceConfig
(ConeTrace.fxh:37-139) and the entry point's contract (coverage, discards, blend models, stores, statistics) as the header states it.

The G-buffer decode and every distance come from the oracle library (oracle.sample_gbuffer, oracle.sample_distance_field).  Everything
else is the header's defined arithmetic, operation for operation: one float32 rounding per +, -, *, /, sqrt in the order the HLSL writes
it, acos as acos_defined (a fixed polynomial form, no library call), and libm's fmaf where the device code fuses on purpose: the sample
position origin + direction * x and the cone radius growth * x + MIN_CONE_RADIUS.  The loop's liveness is computed as the reference writes
it -- stepsRemaining * (the sum of three products of saturates) -- not as the compares the kernel decomposes it into.  Only pow in the final
cone opacity may differ from the kernel, within the suite's criterion.

The opacity term is written over arrays (one element per pixel; scalars work too): numpy rounds every float32 operation once.

Shared by tests/test_line_kat.py (no GPU), tests/test_line_gpu.py and tests/test_host_line_gpu.py.
"""
import numpy as np

from illuminant_amd import abi, scenes
from tests import directional_common as dc
from tests.directional_common import (F, fmaf, sat, power, light_array, half, to_stored, from_stored, decode_pixels, Result,  # noqa: F401
                                      MIN_CONE_RADIUS, MAX_STEP_RAMP_WINDOW, TRACE_INITIAL_OFFSET_PX, FULLY_SHADOWED_THRESHOLD,
                                      HACK_DISTANCE_OFFSET, VISIBILITY_RANGE)

# LineLightCore.fxh:10-11,30, ConeTrace.fxh:29, FBPBR.fxh:76
SELF_OCCLUSION_HACK = F(1.5)
TRACE_THRESHOLD = F(F(0.75) / F(255))
MINIMUM_OFFSET = F(0.03)
TRACE_END_MULTIPLIER = F(100)
ILLUMINANCE_WEIGHT = F(0.2)
PI = F(np.pi)
TWO_PI = F(F(2) * PI)

line_light = scenes.line_light      # RenderLineLightSource's packing

# Abramowitz & Stegun 4.4.46, rounded to float32
ACOS_COEFFICIENTS = tuple(F(c) for c in (1.5707963050, -0.2145988016, 0.0889789874, -0.0501743046, 0.0308918810, -0.0170881256, 0.0066700901,
                                         -0.0012624911))


def acos_defined(x):
    """hlsl_math.hpp acos_defined: sqrt(1 - |x|) * P7(|x|), Horner from the highest coefficient down without fma, pi - r for x < 0."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        a = np.abs(x)
        p = np.full_like(a, ACOS_COEFFICIENTS[7])
        for k in range(6, -1, -1):
            p = (p * a).astype(np.float32) + ACOS_COEFFICIENTS[k]
        r = np.sqrt(F(1) - a) * p
        out = np.where(x < 0, PI - r, r).astype(np.float32)
    return out if out.ndim else F(out)


def v3(x, y, z):
    return [np.asarray(x, np.float32), np.asarray(y, np.float32), np.asarray(z, np.float32)]


def sub3(a, b):
    return [a[k] - b[k] for k in range(3)]


def add3(a, b):
    return [a[k] + b[k] for k in range(3)]


def scale3(a, s):
    return [a[k] * s for k in range(3)]


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def len3(a):
    return np.sqrt(dot3(a, a))


def norm3(a):
    l = len3(a)
    return [a[0] / l, a[1] / l, a[2] / l]


def cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


class Record:
    """what prepare_line_lights_kernel computes once per light, with the same roundings"""


def prepare(light, dfu):
    r = Record()
    with np.errstate(all="ignore"):
        r.a = v3(light.LightPosition1.x, light.LightPosition1.y, light.LightPosition1.z)
        r.b = v3(light.LightPosition2.x, light.LightPosition2.y, light.LightPosition2.z)
        r.delta = sub3(r.b, r.a)
        r.left = norm3(r.delta)
        r.centre = add3(r.a, scale3(sub3(r.b, r.a), F(0.5)))
        r.ab_dot = dot3(r.delta, r.delta)
        r.radius = F(light.LightProperties.x)
        r.radius_sq = F(r.radius * r.radius)
        r.offset = np.fmax(sat(F(F(r.radius + F(1)) / len3(r.delta))), MINIMUM_OFFSET)
        r.casts = F(light.LightProperties.w)
        # createTraceConfig((Radius, ramp length), (1, falloff))
        r.max_radius = np.fmin(np.fmax(r.radius, MIN_CONE_RADIUS), F(dfu.ConeAndMisc.x))
        r.growth = F(F(r.max_radius / np.fmax(F(light.LightProperties.y), F(16))) * F(1))
        r.ao_radius, r.ao_opacity = F(light.MoreLightProperties.x), F(light.MoreLightProperties.w)
        r.c1 = [F(light.Color1.x), F(light.Color1.y), F(light.Color1.z), F(light.Color1.w)]
        r.c2 = [F(light.Color2.x), F(light.Color2.y), F(light.Color2.z), F(light.Color2.w)]
    return r


def opacity_term(pos, normal, r, parts=None):
    """computeLineLightOpacity over pixels: pos, normal = [x, y, z] float32 arrays (or scalars).  Returns (opacity, u).  parts: a dict
    that receives the solid angle and the two illuminances."""
    with np.errstate(all="ignore"):
        u = sat(dot3(sub3(pos, r.a), r.delta) / r.ab_dot)
        sphere = add3(r.a, scale3(r.delta, u))
        to_sphere = sub3(sphere, pos)
        forward = norm3(to_sphere)
        up = cross3(r.left, forward)
        ru = scale3(up, r.radius)
        v = [sub3(add3(r.a, ru), pos), sub3(sub3(r.a, ru), pos), sub3(sub3(r.b, ru), pos), sub3(add3(r.b, ru), pos)]
        n = [norm3(cross3(v[i], v[(i + 1) % 4])) for i in range(4)]
        g = [acos_defined(dot3(scale3(n[i], F(-1)), n[(i + 1) % 4])) for i in range(4)]
        solid_angle = (((g[0] + g[1]) + g[2]) + g[3]) - TWO_PI
        facing = (((sat(dot3(norm3(v[0]), normal)) + sat(dot3(norm3(v[1]), normal))) + sat(dot3(norm3(v[2]), normal))) +
                  sat(dot3(norm3(v[3]), normal))) + sat(dot3(norm3(sub3(r.centre, pos)), normal))
        illuminance = (solid_angle * ILLUMINANCE_WEIGHT) * facing
        illuminance_sphere = (PI * sat(dot3(forward, normal))) * (r.radius_sq / dot3(to_sphere, to_sphere))
        opacity = sat(illuminance + illuminance_sphere)
    if parts is not None:
        parts.update(solid_angle=solid_angle, illuminance=illuminance, illuminance_sphere=illuminance_sphere)
    assert np.asarray(opacity).dtype == np.float32 and np.asarray(u).dtype == np.float32
    return opacity, u


def opacity_term_float64(pos, normal, light):
    """the same formula in float64 with the true acos, from the light's float32 members: the yardstick of the fidelity test"""
    D = np.float64
    a = [D(light.LightPosition1.x), D(light.LightPosition1.y), D(light.LightPosition1.z)]
    b = [D(light.LightPosition2.x), D(light.LightPosition2.y), D(light.LightPosition2.z)]
    radius = D(light.LightProperties.x)
    pos = [np.asarray(c, D) for c in pos]
    normal = [np.asarray(c, D) for c in normal]
    clip = lambda x: np.clip(x, 0.0, 1.0)
    with np.errstate(all="ignore"):
        delta = sub3(b, a)
        u = clip(dot3(sub3(pos, a), delta) / dot3(delta, delta))
        to_sphere = sub3(add3(a, scale3(delta, u)), pos)
        forward = norm3(to_sphere)
        ru = scale3(cross3(norm3(delta), forward), radius)
        v = [sub3(add3(a, ru), pos), sub3(sub3(a, ru), pos), sub3(sub3(b, ru), pos), sub3(add3(b, ru), pos)]
        n = [norm3(cross3(v[i], v[(i + 1) % 4])) for i in range(4)]
        g = [np.arccos(np.clip(dot3(scale3(n[i], -1.0), n[(i + 1) % 4]), -1.0, 1.0)) for i in range(4)]
        solid_angle = g[0] + g[1] + g[2] + g[3] - 2 * np.pi
        centre = add3(a, scale3(delta, 0.5))
        facing = sum(clip(dot3(norm3(v[i]), normal)) for i in range(4)) + clip(dot3(norm3(sub3(centre, pos)), normal))
        sphere = np.pi * clip(dot3(forward, normal)) * (radius * radius / dot3(to_sphere, to_sphere))
        return clip(solid_angle * 0.2 * facing + sphere), solid_angle


def line_trace(sample, shaded, normal, r, u, dfu, have_field):
    """lineConeTrace from shaded + 1.5 normal towards the three points of the segment.  Returns (cone opacity, samples taken, facts)."""
    shaded = [F(c) for c in shaded]
    normal = [F(c) for c in normal]
    u = F(u)
    start = [F(shaded[k] + F(normal[k] * SELF_OCCLUSION_HACK)) for k in range(3)]
    along = [sat(F(u - r.offset)), u, sat(F(u + r.offset))]
    rays, lengths = [], []
    with np.errstate(all="ignore"):
        for t in along:
            target = [F(F(r.a[k]) + F(F(r.delta[k]) * t)) for k in range(3)]
            tv = [F(target[k] - start[k]) for k in range(3)]
            trace_length = F(np.sqrt(F(F(F(tv[0] * tv[0]) + F(tv[1] * tv[1])) + F(tv[2] * tv[2]))))
            rays.append([F(tv[k] / trace_length) for k in range(3)])
            lengths.append(np.fmax(F(trace_length - r.radius), F(1)))
    x, z = [TRACE_INITIAL_OFFSET_PX] * 3, [F(1)] * 3
    min_step = np.fmax(F(1), F(dfu.Packed1.w))
    long_step = F(dfu.StepAndMisc2.z)
    steps = F(dfu.StepAndMisc2.x)
    samples = iterations = 0
    ended = [None, None, None]          # the iteration after which a ray's own liveness factor was first 0
    liveness = F(1) if have_field else F(0)
    while liveness > 0:
        iterations += 1
        live = []
        for i in range(3):
            position = [fmaf(rays[i][k], x[i], start[k]) for k in range(3)]
            position = [F(0) if np.isnan(c) else c for c in position]          # (the sampler reads a NaN coordinate as 0)
            s = F(sample(position))
            samples += 1
            radius = np.fmin(fmaf(r.growth, x[i], MIN_CONE_RADIUS), r.max_radius)
            with np.errstate(all="ignore"):
                z[i] = np.fmin(z[i], F(F(s + HACK_DISTANCE_OFFSET) / radius))
                x[i] = np.fmin(F(x[i] + np.fmax(F(np.abs(s) * long_step), min_step)), lengths[i])
                live.append(F(sat(F(z[i] - FULLY_SHADOWED_THRESHOLD)) * sat(F(F(lengths[i] - x[i]) * TRACE_END_MULTIPLIER))))
            if ended[i] is None and not (live[i] > 0):
                ended[i] = iterations
        steps = F(steps - F(1))
        with np.errstate(all="ignore"):
            liveness = F(steps * F(F(live[0] + live[1]) + live[2]))
    with np.errstate(all="ignore"):
        visibility = np.fmin(F(F(F(z[0] + z[1]) + z[2]) / F(3)), F(steps / MAX_STEP_RAMP_WINDOW))
    opacity = power(sat(F(sat(F(visibility - FULLY_SHADOWED_THRESHOLD)) / VISIBILITY_RANGE)), F(dfu.ConeAndMisc.z))
    return opacity, samples, {"start": start, "rays": rays, "lengths": lengths, "along": along, "visibilities": list(z), "positions": list(x),
                              "steps_remaining": steps, "iterations": iterations, "ended": tuple(ended), "visibility": visibility}


def shade(sample, pixel, r, distance_opacity, u, dfu, have_field):
    """One light on one decoded G-buffer texel that is not fullbright, given the pair's opacity term.  Returns None when the shader
    discards, else (rgb, samples, traced, facts)."""
    shaded, normal, enable_shadows, _fullbright = pixel
    if not ((distance_opacity > 0) and (F(shaded[0]) > F(-9999))):
        return None
    samples = 0
    ao = F(1)
    ao_radius = F(r.ao_radius * np.fmax(F(0), F(normal[2])))
    if ao_radius >= F(0.5) and have_field:
        distance = F(sample((F(shaded[0]), F(shaded[1]), F(F(shaded[2]) + F(F(normal[2]) * ao_radius)))))
        samples += 1
        t = F(F(1) - sat(F(np.fmin(np.fmax(distance, F(0)), ao_radius) / ao_radius)))
        t = F(t * t)
        t = F(F(1) - t)
        ao = F(F(F(1) - r.ao_opacity) + F(t * r.ao_opacity))
    pre_trace = F(distance_opacity * ao)
    facts = {"distance_opacity": distance_opacity, "u": u, "pre_trace": pre_trace}
    casts = F(r.casts * (F(1) if enable_shadows else F(0)))
    cone = F(1)
    traced = False
    if casts != 0 and pre_trace >= TRACE_THRESHOLD:
        cone, n, trace_facts = line_trace(sample, shaded, normal, r, u, dfu, have_field)
        samples += n
        traced = have_field
        facts.update(trace_facts, cone=cone)
    opacity = F(pre_trace * cone)
    color = [F(r.c1[k] + F(F(r.c2[k] - r.c1[k]) * u)) for k in range(4)]
    rgb = [F(F(color[k] * color[3]) * opacity) for k in range(3)]
    facts["opacity"] = opacity
    return rgb, samples, traced, facts


def pixel_arrays(pixels):
    pos = [np.array([p[0][k] for p in pixels], np.float32) for k in range(3)]
    normal = [np.array([p[1][k] for p in pixels], np.float32) for k in range(3)]
    return pos, normal


def render(oracle, lights, env, dfu, gbuffer, sdf, ambient, width, height, row_begin=0, row_end=None, blend_fp16=False, before=None, pixels=None):
    """The whole call.  ambient None: the lights are added to `before` ((H, W, 4) float32: the lightmap's texels as the pass reads them
    back); else rows [row_begin, row_end) start from ambient and the other rows keep `before` (zeros when None).  pixels:
    decode_pixels(...) of the scene, to share among calls."""
    row_end = height if row_end is None else row_end
    image = np.zeros((height, width, 4), np.float32) if before is None else np.array(before, np.float32, copy=True)
    have_field = sdf is not None and F(dfu.Extent.x) > 0
    if pixels is None:
        pixels = decode_pixels(oracle, env, gbuffer, width, height)

    def sample(p):
        return oracle.sample_distance_field(p, dfu, sdf)

    pos, normal = pixel_arrays(pixels)
    prepared = [prepare(l, dfu) for l in lights]
    terms = [opacity_term(pos, normal, r) for r in prepared]
    out = Result()
    out.detail = {}
    n_samples = n_pairs = n_traced = 0
    for y in range(row_begin, row_end):
        for x in range(width):
            base = np.asarray(ambient, np.float32) if ambient is not None else image[y, x].copy()
            if blend_fp16:
                base = half(base)
            acc = [base[k] for k in range(4)] if blend_fp16 else [F(0)] * 4
            pixel = pixels[y * width + x]
            for i, r in enumerate(prepared):
                if pixel[3]:                    # fullbright: discarded before the opacity term, no pair
                    continue
                n_pairs += 1
                shaded = shade(sample, pixel, r, F(terms[i][0][y * width + x]), F(terms[i][1][y * width + x]), dfu, have_field)
                if shaded is None:
                    continue
                rgb, n, traced, facts = shaded
                n_samples += n
                n_traced += 1 if traced else 0
                out.detail[(x, y, i)] = facts
                c = [rgb[0], rgb[1], rgb[2], F(1)]
                if blend_fp16:
                    acc = [half(F(acc[k] + half(c[k]))) for k in range(4)]
                else:
                    acc = [F(acc[k] + c[k]) for k in range(4)]
            image[y, x] = acc if blend_fp16 else [F(base[k] + acc[k]) for k in range(4)]
    out.image = image
    out.stats = (n_samples, n_pairs, n_traced)
    return out


# ---- the scene of the tests: directional_common's frame, field and G-buffer --------------------------------------------------------

WIDTH, HEIGHT = dc.WIDTH, dc.HEIGHT
MAX_STEP_COUNT = dc.MAX_STEP_COUNT
field_layout, field_atlas, field_uniforms, no_field_uniforms, gbuffer_texels = (dc.field_layout, dc.field_atlas, dc.field_uniforms,
                                                                                dc.no_field_uniforms, dc.gbuffer_texels)
ramp_texture = dc.ramp_texture
INVISIBLE_VIEWPORT = dc.INVISIBLE_VIEWPORT

# the four light geometries of the fidelity measurement (start, end, radius) over a 64 x 48 ground plane
KAT_GEOMETRIES = (((10.0, 10.0, 20.0), (50.0, 30.0, 20.0), 4.0), ((10.0, 10.0, 20.0), (50.0, 30.0, 40.0), 1.0),
                  ((-200.0, 10.0, 60.0), (-100.0, 30.0, 60.0), 2.0), ((10.0, 24.0, 8.0), (54.0, 24.0, 8.0), 0.5))
