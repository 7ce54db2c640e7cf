"""The references of ilm_render_directional_light_probes and ilm_render_line_light_probes, from existing code alone.

Directional: DirectionalLightProbePixelShader / ...WithRampPixelShader (DirectionalLight.fx:163-219) is the frame pass's core on the probe,
so every (probe, light) pair is tests.directional_common.shade on pixel = (position, normal, enableShadows != 0, not fullbright) with a copy
of the light whose shadow filter is off (EvenMoreLightProperties.x = -1: the probe shaders do not take the member) and whose AO members are
0 (:183).  A probe with w <= 0 gets nothing (sampleLightProbeBuffer discards); the pair's rgb is F(F(colour * opacity) * w) with colour =
F(Color1.rgb * Color1.a), and the pairs are added in fp32 in light order, alpha + 1 per contributing pair.

Line: LineLightProbe.fx is SphereLightProbe's shader at LightPosition1, and oracle.render_light_probes is already the restatement of
that shader: it is called on the line vertices as they are.

The scene is directional_common's field (48 x 32 x 32, a tall box and an ellipsoid, both atlas formats) under dc.field_uniforms().

Shared by tests/test_probe_kinds_kat.py (no GPU) and tests/test_probe_kinds_gpu.py.
"""
import numpy as np

from illuminant_amd import abi, scenes
from tests import directional_common as dc

F = np.float32
KNIFE = 1e-3


def probe_light(light):
    """the light as the probe shader's core sees it: no shadow filter, no ambient occlusion"""
    l = abi.LightVertex.from_buffer_copy(bytes(light))
    l.EvenMoreLightProperties.x = -1.0
    l.MoreLightProperties.x = 0.0
    l.MoreLightProperties.w = 0.0
    return l


def directional_pairs(oracle, lights, positions, normals, dfu, sdf, ramp=None):
    """(pairs (probes, lights, 4) float32: each pair's rgb and 1, or zeros where the pair contributes nothing; facts {(probe, light): facts
    of dc.shade})"""
    pp = np.ascontiguousarray(positions, np.float32).reshape(-1, 4)
    pn = np.ascontiguousarray(normals, np.float32).reshape(-1, 4)
    lights = list(lights) if lights is not None else []
    have_field = sdf is not None and F(dfu.Extent.x) > 0
    if ramp is not None and (np.asarray(ramp).shape[0] == 1 and np.asarray(ramp).shape[1] == 1):
        ramp = None
    ramp_lookup = (lambda u: oracle.table_lookup(1, ramp, float(u), 0.0)[0]) if ramp is not None else None

    def sample(p):
        return oracle.sample_distance_field(p, dfu, sdf)

    prepared = []
    for l in lights:
        a = F(l.Color1.w)
        prepared.append((probe_light(l), (F(F(l.Color1.x) * a), F(F(l.Color1.y) * a), F(F(l.Color1.z) * a))))
    pairs = np.zeros((pp.shape[0], len(lights), 4), np.float32)
    facts = {}
    for i in range(pp.shape[0]):
        w = F(pp[i, 3])
        if not (w > 0):
            continue
        pixel = ([F(c) for c in pp[i, :3]], [F(c) for c in pn[i, :3]], bool(pn[i, 3] != 0), False)
        for k, (l, col) in enumerate(prepared):
            shaded = dc.shade(sample, pixel, l, dfu, have_field, ramp_lookup)
            if shaded is None:
                continue
            opacity, _n, _traced, f = shaded
            f["opacity"] = opacity
            facts[(i, k)] = f
            pairs[i, k] = [F(F(col[0] * opacity) * w), F(F(col[1] * opacity) * w), F(F(col[2] * opacity) * w), F(1)]
    return pairs, facts


def sum_pairs(pairs, probe_count=None, light_count=None):
    """the first light_count lights on the first probe_count probes, added in fp32 in light order"""
    pairs = pairs[:probe_count, :light_count]
    out = np.zeros((pairs.shape[0], 4), np.float32)
    for k in range(pairs.shape[1]):
        lit = pairs[:, k, 3] != 0
        out[lit] = (out[lit] + pairs[lit, k]).astype(np.float32)
    return out


def directional_probes(oracle, lights, positions, normals, dfu, sdf, ramp=None):
    return sum_pairs(directional_pairs(oracle, lights, positions, normals, dfu, sdf, ramp)[0])


def knife_edges(facts, lights):
    """the pairs whose trace left its loop within KNIFE of a decision: visibility at the fully-shadowed threshold, or the position at the
    trace's end (data_y - x = 0).  A probe of such a pair is moved before the list below is committed."""
    out = []
    for (i, k), f in facts.items():
        if "visibility" not in f or f["position"] == dc.TRACE_INITIAL_OFFSET_PX:      # no trace, or a trace without a field: no loop
            continue
        data_y = np.fmax(F(f["length"] - F(lights[k].LightProperties.z)), F(1))
        if abs(float(f["visibility"]) - float(dc.FULLY_SHADOWED_THRESHOLD)) < KNIFE or abs(float(data_y) - float(f["position"])) < KNIFE:
            out.append((i, k, float(f["visibility"]), float(data_y) - float(f["position"])))
    return out


def line_probes(oracle, lights, positions, normals, env, dfu, sdf):
    return oracle.render_light_probes(lights, positions, normals, env, dfu, sdf)


def sphere_vertex_of(line):
    """the sphere vertex of a line vertex's four members LineLightProbe reads: centre, Color1, LightProperties, MoreLightProperties"""
    v = abi.LightVertex()
    v.LightPosition1 = v.LightPosition2 = v.LightPosition3 = abi.f4(line.LightPosition1.x, line.LightPosition1.y, line.LightPosition1.z, 0)
    v.Color1 = abi.f4(line.Color1.x, line.Color1.y, line.Color1.z, line.Color1.w)
    v.Color2 = abi.f4(0, 0, 0, 1)
    p, m = line.LightProperties, line.MoreLightProperties
    v.LightProperties = abi.f4(p.x, p.y, p.z, p.w)
    v.MoreLightProperties = abi.f4(m.x, m.y, m.z, m.w)
    v.EvenMoreLightProperties = abi.f4(-1, 0, F(-np.pi), F(1.0 / (np.pi * 2)))
    return v


# ---- the probes and lights of the tests ---------------------------------------------------------------------------------------------

PROBE_COUNT = 129           # 64 lanes per block: two full blocks and one lane of a third
NORMALS = ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.36, 0.48, 0.8), (-0.6, 0.0, 0.8))
# probes moved off a knife edge (tests/test_probe_kinds_kat.py finds them): index -> position
MOVED = {}


def probes(count=PROBE_COUNT):
    """(positions (count, 4), normals (count, 4)): a fixed list over the field -- every fourth probe without a normal, every fifth with
    shadows off, opacities 0.5 (i % 7 == 2) and 0 (i % 11 == 5), invisible probes (x = -10000, i % 13 == 6)"""
    pp = np.zeros((count, 4), np.float32)
    pn = np.zeros((count, 4), np.float32)
    for i in range(count):
        pos = (round(2.0 + (i * 7.13) % 44.0, 2), round(2.0 + (i * 3.71) % 28.0, 2), round(0.5 + (i * 1.37) % 9.0, 2))
        pos = MOVED.get(i, pos)
        w = 0.0 if i % 11 == 5 else 0.5 if i % 7 == 2 else 1.0
        if i % 13 == 6:
            pos = (-10000.0, pos[1], pos[2])
        pp[i] = (pos[0], pos[1], pos[2], w)
        pn[i, :3] = NORMALS[i % 4]
        pn[i, 3] = 0.0 if i % 5 == 3 else 1.0
    return pp, pn


DIRECTIONS = ((0.55, 0.3, -0.6), (0.0, 0.0, -1.0), (-0.4, 0.5, -0.7), (0.4, -0.2, 0.25))


def unshadowed_lights(count):
    """directed lights without shadows and, every third, an undirected one (Color2 = 0: an ambient light)"""
    out = []
    for k in range(count):
        color = (0.2 + 0.047 * k, 0.9 - 0.041 * k, 0.3 + 0.023 * (k % 7), 1.0 - 0.03 * (k % 5))
        direction = None if k % 3 == 2 else DIRECTIONS[k % 4]
        out.append(dc.directional_light(direction=direction, color=color, casts_shadows=False, opacity=1.0 - 0.02 * k))
    return out


def shadowed_light(k, **kw):
    """(no trace length minus softness is 0.5 + a multiple of the minimum step 1.5: a probe without a normal in open space would end its
    trace exactly there, on the knife edge of `length > position`)"""
    args = dict(direction=DIRECTIONS[k % 4], color=(0.9 - 0.1 * k, 0.4 + 0.1 * k, 0.6, 0.9), shadow_trace_length=(20.0, 18.0, 24.0, 12.4)[k % 4],
                shadow_softness=(2.0, 3.0, 1.5, 1.0)[k % 4], shadow_ramp_rate=(0.5, 1.0, 0.75, 0.5)[k % 4])
    args.update(kw)
    return dc.directional_light(**args)


def mixed_lights(count, shadowed):
    """`count` lights of which the ones at indices 1, 5, 9, ... (`shadowed` of them) cast shadows"""
    out = unshadowed_lights(count)
    at = [1 + 4 * j for j in range(shadowed)]
    for j, k in enumerate(at):
        out[k] = shadowed_light(j)
    return out


def line_lights(count, ramp_length=0.0):
    out = []
    for k in range(count):
        start = (4.0 + (k * 9.7) % 40.0, 3.0 + (k * 5.3) % 26.0, 6.0 + (k * 2.9) % 14.0)
        end = (44.0 - (k * 6.1) % 40.0, 29.0 - (k * 4.7) % 26.0, 4.0 + (k * 1.3) % 10.0)
        out.append(scenes.line_light(start, end, 6.0 + (k % 5) * 2.5, start_color=(0.9 - 0.04 * k, 0.3 + 0.03 * k, 0.5, 0.9),
                                     end_color=(0.1, 0.8, 0.2 + 0.04 * k, 0.6), casts_shadows=(k % 4 != 3), ramp_length=ramp_length,
                                     falloff_y=1.0 + 0.25 * (k % 3), ramp_mode=k % 3))
    return out
