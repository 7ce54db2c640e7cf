"""ilm_render_directional_lights restated in numpy float32: DirectionalLightPixelShader / ...WithRamp (DirectionalLight.fx:52-161),
computeNormalFactorEx / computeDirectionalLightOpacity (LightCommon.fxh:154-165,224-231), computeAO (AOCommon.fxh:1-19), coneTrace
(ConeTrace.fxh:37-191) and the entry point's contract (coverage, discards, blend models, stores, statistics) as the header states it.

The G-buffer decode, every distance and the ramp lookup come from the oracle library (oracle.sample_gbuffer,
oracle.sample_distance_field, oracle.table_lookup(1, ...)).  The trace state -- position along the ray, visibility, step budget, sample
coordinates -- is computed in the kernel's arithmetic, operation for operation: one float32 rounding per +, -, *, /, sqrt (the
library is built without contraction), and libm's fmaf (exact by definition) where the device code fuses on purpose: the sample
position start + direction * x and the cone radius growth * x + MIN_CONE_RADIUS.  Only pow (normal factor, final opacity) and the ramp's
filter may differ from the kernel, within the suite's criterion.

Shared by tests/test_directional_kat.py (no GPU) and tests/test_directional_gpu.py.
"""
import ctypes as C
import ctypes.util
import functools

import numpy as np

from illuminant_amd import abi, scenes

F = np.float32

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = C.c_float
_libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]


def fmaf(a, b, c):
    return F(_libm.fmaf(float(a), float(b), float(c)))


# the shader's constants (LightCommon.fxh:7-10, DirectionalLight.fx:13,73, ConeTrace.fxh:5-23)
DIRECTIONAL_DOT_OFFSET = F(0.35)
DIRECTIONAL_DOT_RAMP_RANGE = F(0.35)
DOT_EXPONENT = F(0.85)
SELF_OCCLUSION_HACK = F(1.5)
TRACE_THRESHOLD = F(F(1) / F(256))
MINIMUM_W = F(0.1)
MIN_CONE_RADIUS = F(0.33)
MAX_STEP_RAMP_WINDOW = F(2)
TRACE_INITIAL_OFFSET_PX = F(0.5)
FULLY_SHADOWED_THRESHOLD = F(0.075)
UNSHADOWED_THRESHOLD = F(0.95)
HACK_DISTANCE_OFFSET = F(1.5)
VISIBILITY_RANGE = F(UNSHADOWED_THRESHOLD - FULLY_SHADOWED_THRESHOLD)


def sat(x):
    return np.fmin(np.fmax(F(x), F(0)), F(1))


def power(x, y):
    """pow(x, y) for x >= 0, in double, rounded once (the kernel's exp2(y log2 x) may differ by a few ulp)."""
    if y == 0:
        return F(1)
    return F(float(x) ** float(y)) if x > 0 else F(0)


directional_light = scenes.directional_light      # RenderDirectionalLightSource's packing, beside scenes.sphere_light


def light_array(lights):
    arr = (abi.LightVertex * len(lights))()
    for i, l in enumerate(lights):
        arr[i] = l
    return arr


def footprint(light, env):
    """(x0, y0, x1, y1) in screen pixels, the header's arithmetic: (LightPosition - ViewportPosition) * (ViewportScale * RenderScale)."""
    sx = F(F(env.GBufferTexelSizeAndMisc.z) * F(env.ZAndScale.z))
    sy = F(F(env.GBufferTexelSizeAndMisc.w) * F(env.ZAndScale.w))
    vx, vy = F(env.ViewportPosition[0]), F(env.ViewportPosition[1])
    return (F(F(F(light.LightPosition1.x) - vx) * sx), F(F(F(light.LightPosition1.y) - vy) * sy),
            F(F(F(light.LightPosition2.x) - vx) * sx), F(F(F(light.LightPosition2.y) - vy) * sy))


def covers(fp, x, y):
    """the pixel's centre (x + 0.5, y + 0.5) in [x0, x1) x [y0, y1)"""
    cx, cy = F(F(x) + F(0.5)), F(F(y) + F(0.5))
    return bool((cx >= fp[0]) and (cx < fp[2]) and (cy >= fp[1]) and (cy < fp[3]))


def normal_factor(direction, normal):
    """computeNormalFactorEx with DIRECTIONAL_DOT_OFFSET / DIRECTIONAL_DOT_RAMP_RANGE; 1 for a zero normal."""
    n = [F(c) for c in normal]
    if not any(c != 0 for c in n):
        return F(1)
    m = [F(F(c) * F(-1)) for c in direction]
    d = F(F(F(m[0] * n[0]) + F(m[1] * n[1])) + F(m[2] * n[2]))
    return power(sat(F(F(d + DIRECTIONAL_DOT_OFFSET) / DIRECTIONAL_DOT_RAMP_RANGE)), DOT_EXPONENT)


def trace_config(light, dfu):
    """createTraceConfig with lightRamp = (ShadowSoftness, shadowDistanceFalloff) and cone growth ShadowRampRate: maxRadius, growth."""
    max_radius = np.fmin(np.fmax(F(light.LightProperties.z), MIN_CONE_RADIUS), F(dfu.ConeAndMisc.x))
    growth = F(F(max_radius / np.fmax(F(light.MoreLightProperties.y), F(16))) * F(light.LightProperties.w))
    return max_radius, growth


def cone_trace(sample, shaded, normal, light, dfu, have_field):
    """coneTrace towards shaded - direction * ShadowTraceLength from shaded + 1.5 normal.  Returns (cone opacity, samples taken,
    facts of the trace for the known-answer tests)."""
    shaded = [F(c) for c in shaded]
    normal = [F(c) for c in normal]
    direction = [F(light.Color2.x), F(light.Color2.y), F(light.Color2.z)]
    length, softness = F(light.LightProperties.y), F(light.LightProperties.z)
    start = [F(shaded[k] + F(normal[k] * SELF_OCCLUSION_HACK)) for k in range(3)]
    centre = [F(shaded[k] - F(direction[k] * length)) for k in range(3)]
    tv = [F(centre[k] - start[k]) for k in range(3)]
    with np.errstate(all="ignore"):
        trace_length = F(np.sqrt(F(F(F(tv[0] * tv[0]) + F(tv[1] * tv[1])) + F(tv[2] * tv[2]))))
        ray = [F(tv[k] / trace_length) for k in range(3)]
    data_y = np.fmax(F(trace_length - softness), F(1))
    x, z = TRACE_INITIAL_OFFSET_PX, F(1)
    min_step = np.fmax(F(1), F(dfu.Packed1.w))
    long_step = F(dfu.StepAndMisc2.z)
    steps = F(dfu.StepAndMisc2.x)
    max_radius, growth = trace_config(light, dfu)
    # (the sampler reads a NaN coordinate as 0: such an axis is start = direction = 0, as the kernel hoists it)
    for k in range(3):
        if np.isnan(start[k]) or np.isnan(ray[k]):
            start[k], ray[k] = F(0), F(0)
    samples = 0
    alive = have_field
    while alive:
        steps = F(steps - F(1))
        position = [fmaf(ray[k], x, start[k]) for k in range(3)]
        s = F(sample(position))
        samples += 1
        radius = np.fmin(fmaf(growth, x, MIN_CONE_RADIUS), max_radius)
        with np.errstate(all="ignore"):
            z = np.fmin(z, F(F(s + HACK_DISTANCE_OFFSET) / radius))
        x = F(x + np.fmax(F(np.abs(s) * long_step), min_step))
        alive = bool((steps > 0) and (z > FULLY_SHADOWED_THRESHOLD) and (data_y > x))
    visibility = np.fmin(z, F(steps / MAX_STEP_RAMP_WINDOW))
    opacity = power(sat(F(sat(F(visibility - FULLY_SHADOWED_THRESHOLD)) / VISIBILITY_RANGE)), F(dfu.ConeAndMisc.z))
    return opacity, samples, {"start": start, "ray": ray, "length": trace_length, "visibility": z, "steps_remaining": steps, "position": x}


def shade(sample, pixel, light, dfu, have_field, ramp_lookup=None):
    """One light on one decoded G-buffer texel (shaded, normal, enable_shadows, fullbright).  Returns None when the shader discards,
    else (opacity, AO + trace samples, traced: the pair ran traceShadows with a bound field, facts)."""
    shaded, normal, enable_shadows, fullbright = pixel
    shadow_filter = F(light.EvenMoreLightProperties.x)
    filtered = False if shadow_filter < 0 else ((shadow_filter > F(0.5)) != enable_shadows)
    if fullbright or filtered:
        return None
    if not (F(shaded[0]) > F(-9999)):
        return None
    casts = F(F(light.LightProperties.x) * (F(1) if enable_shadows else F(0)))
    direction = (light.Color2.x, light.Color2.y, light.Color2.z)
    directed = F(light.Color2.w) >= MINIMUM_W
    opacity = normal_factor(direction, normal) if directed else F(1)
    samples = 0
    ao_radius = F(F(light.MoreLightProperties.x) * np.fmax(F(0), F(normal[2])))
    if ao_radius >= F(0.5) and have_field:
        distance = F(sample((F(shaded[0]), F(shaded[1]), F(F(shaded[2]) + F(F(normal[2]) * ao_radius)))))
        samples += 1
        r = F(F(1) - sat(F(np.fmin(np.fmax(distance, F(0)), ao_radius) / ao_radius)))
        r = F(r * r)
        r = F(F(1) - r)
        ao_opacity = F(light.MoreLightProperties.w)
        opacity = F(opacity * F(F(F(1) - ao_opacity) + F(r * ao_opacity)))
    facts = {"pre_trace": opacity}
    traced = False
    if casts != 0 and opacity >= TRACE_THRESHOLD and directed:
        cone, n, trace_facts = cone_trace(sample, shaded, normal, light, dfu, have_field)
        samples += n
        traced = have_field
        facts.update(trace_facts, cone=cone)
        opacity = F(opacity * cone)
    if ramp_lookup is not None:
        opacity = F(ramp_lookup(opacity))
    return opacity, samples, traced, facts


def half(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def to_stored(image, fmt):
    """What ilm_lightmap_download returns for a lightmap of format fmt holding `image`: the store's rounding."""
    image = np.asarray(image, np.float32)
    if fmt == abi.LIGHTMAP_FLOAT4:
        return image.copy()
    if fmt == abi.LIGHTMAP_HALF4:
        return image.astype(np.float16)
    return np.rint((np.clip(image, F(0), F(1)) * F(255)).astype(np.float32)).astype(np.uint8)


def from_stored(texels, fmt):
    """What the pass reads back from a lightmap of format fmt (accumulate mode)."""
    if fmt == abi.LIGHTMAP_RGBA8:
        return (np.asarray(texels, np.uint8).astype(np.float32) / F(255)).astype(np.float32)
    return np.asarray(texels).astype(np.float32)


class Result:
    """image (H, W, 4) float32 before the store's rounding, stats (SdfSamples, PixelLightPairs, TracedPairs), detail {(x, y, light
    index): facts of that pair}."""


def decode_pixels(oracle, env, gbuffer, width, height):
    """oracle.sample_gbuffer for every pixel: [(shaded, normal, enable_shadows, fullbright)] row-major.  Compute once per scene."""
    out = []
    for y in range(height):
        for x in range(width):
            shaded, normal, enable_shadows, fullbright, _camera = oracle.sample_gbuffer(float(x), float(y), env, gbuffer)
            out.append((shaded, normal, enable_shadows, fullbright))
    return out


def render(oracle, lights, env, dfu, gbuffer, sdf, ambient, width, height, row_begin=0, row_end=None, ramp=None, blend_fp16=False,
           before=None, pixels=None):
    """The whole call.  ambient None: the lights are added to `before` ((H, W, 4) float32: the lightmap's texels as the pass reads them
    back); else rows [row_begin, row_end) start from ambient and the other rows keep `before` (zeros when None).  ramp: (h, w, 4)
    float32 or None; a 1 x 1 ramp is none.  pixels: decode_pixels(...) of the scene, to share among calls."""
    row_end = height if row_end is None else row_end
    image = np.zeros((height, width, 4), np.float32) if before is None else np.array(before, np.float32, copy=True)
    have_field = sdf is not None and F(dfu.Extent.x) > 0
    if pixels is None:
        pixels = decode_pixels(oracle, env, gbuffer, width, height)
    if ramp is not None and (np.asarray(ramp).shape[0] == 1 and np.asarray(ramp).shape[1] == 1):
        ramp = None
    ramp_lookup = (lambda u: oracle.table_lookup(1, ramp, float(u), 0.0)[0]) if ramp is not None else None

    def sample(p):
        return oracle.sample_distance_field(p, dfu, sdf)

    prepared = []
    for l in lights:
        a = F(l.Color1.w)
        prepared.append((footprint(l, env), (F(F(l.Color1.x) * a), F(F(l.Color1.y) * a), F(F(l.Color1.z) * a))))
    out = Result()
    out.detail = {}
    n_samples = n_pairs = n_traced = 0
    for y in range(row_begin, row_end):
        for x in range(width):
            base = np.asarray(ambient, np.float32) if ambient is not None else image[y, x].copy()
            if blend_fp16:
                base = half(base)
            acc = [base[k] for k in range(4)] if blend_fp16 else [F(0)] * 4
            for i, l in enumerate(lights):
                fp, col = prepared[i]
                if not covers(fp, x, y):
                    continue
                n_pairs += 1
                shaded = shade(sample, pixels[y * width + x], l, dfu, have_field, ramp_lookup)
                if shaded is None:
                    continue
                opacity, n, traced, facts = shaded
                n_samples += n
                n_traced += 1 if traced else 0
                facts["opacity"] = opacity
                out.detail[(x, y, i)] = facts
                c = [F(col[0] * opacity), F(col[1] * opacity), F(col[2] * opacity), F(1)]
                if blend_fp16:
                    acc = [half(F(acc[k] + half(c[k]))) for k in range(4)]
                else:
                    acc = [F(acc[k] + c[k]) for k in range(4)]
            image[y, x] = acc if blend_fp16 else [F(base[k] + acc[k]) for k in range(4)]
    out.image = image
    out.stats = (n_samples, n_pairs, n_traced)
    return out


# ---- the scene of the tests -----------------------------------------------------------------------------------------------------

WIDTH, HEIGHT = 44, 27          # 1 188 pixels; neither side a multiple of 8: 3 x 2 workgroup tiles, 6 x 4 waves, partial ones at both rims
# a field of 48 x 32 x 32 units, 12 slices of 48 x 32 texels (2 x 2 atlas of 96 x 64): a tall box and an ellipsoid
FIELD_OBSTACLES = ((2, (15.0, 12.0, 12.0), (5.0, 4.0, 12.0)), (1, (33.0, 18.0, 6.0), (6.0, 5.0, 6.0)))
MAX_STEP_COUNT = 24


def field_layout():
    return scenes.DistanceFieldLayout(48, 32, 32.0, 12, maximum_encoded_distance=128)


@functools.lru_cache(maxsize=None)
def field_atlas(fmt):
    atlas = scenes.build_sdf_atlas(field_layout(), list(FIELD_OBSTACLES), fmt=fmt)
    atlas.setflags(write=False)
    return atlas


def field_uniforms(step_limit=MAX_STEP_COUNT, power_=0.8, min_step_size=1.5, long_step_factor=0.75, max_cone_radius=8.0):
    return field_layout().uniforms(max_cone_radius=max_cone_radius, power=power_, step_limit=step_limit, min_step_size=min_step_size,
                                   long_step_factor=long_step_factor)


def no_field_uniforms(step_limit=MAX_STEP_COUNT):
    u = abi.DistanceFieldUniforms()
    u.ConeAndMisc = abi.f4(0, 0, 0, 1)
    u.StepAndMisc2 = abi.f4(step_limit, 3, 0, 1)
    u.Extent = abi.f4(0, 0, 128, 0)
    return u


@functools.lru_cache(maxsize=None)
def gbuffer_texels():
    """(HEIGHT, WIDTH, 4) float32 G-buffer: tilted normals over raised ground, and bands of texels with shadows disabled, fullbright
    texels and zero normals.  (Pixels that are not `visible` -- shaded x <= -9999 -- cannot come from a texel: sampleGBuffer takes x from
    the pixel's own coordinates and the viewport, LightCommon.fxh:118-121.  INVISIBLE_VIEWPORT below makes some.)"""
    h, w = HEIGHT, WIDTH
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    nx = 0.35 * np.sin(xx / 5.0)
    ny = 0.3 * np.cos(yy / 4.0)
    nz = np.sqrt(np.maximum(1.0 - nx * nx - ny * ny, 0.0))
    normal = np.stack([nx, ny, nz], axis=-1)
    z = 3.0 + 2.5 * np.sin(xx / 7.0) * np.cos(yy / 6.0)
    g = scenes.encode_gbuffer(normal, 0.0, z)
    g[5:8] = scenes.encode_gbuffer(normal[5:8], 0.0, z[5:8], enable_shadows=False)
    g[12:14, 20:30] = scenes.encode_gbuffer(normal[12:14, 20:30], 0.0, z[12:14, 20:30], fullbright=True)
    g[17:19, 3:12, :2] = 0.0                     # zero normal
    g.setflags(write=False)
    return g


def ramp_texture(width=16):
    """a 16 x 2 ramp whose r channel is a bent curve (not the identity), so that the with-ramp technique shows"""
    u = (np.arange(width, dtype=np.float32) + 0.5) / width
    t = np.zeros((2, width, 4), np.float32)
    t[0, :, 0] = u * u * 0.9 + 0.05
    t[1, :, 0] = np.sqrt(u) * 0.8
    t[..., 1] = 0.25
    t[..., 2] = 0.5
    t[..., 3] = 1.0
    return t


# a viewport position that puts the shaded x of pixel columns 0 .. 21 at or below -9999 (x - 10020 <= -9999: not `visible`, clip())
INVISIBLE_VIEWPORT = (-10020.0, 0.0)
