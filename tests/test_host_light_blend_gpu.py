"""The host mirror's light sources carry LightSource.BlendMode as two blend functions: lights of a type with different functions form
different render states, RenderLighting sets a state's functions before its call and leaves the context additive.  The frame must equal
the same groups issued through the C ABI in the mirror's order, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native
from tests import directional_common as dc
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

W, H = 40, 24
AMBIENT = (0.4213, 0.3377, 0.5591, 1.0)
ADD, RSUB, MAX, MIN = abi.LIGHT_BLEND_ADD, abi.LIGHT_BLEND_REVERSE_SUBTRACT, abi.LIGHT_BLEND_MAX, abi.LIGHT_BLEND_MIN


@pytest.fixture(scope="module")
def Host():
    from illuminant_amd import _host
    return _host


@pytest.fixture(scope="module")
def hctx(Host):
    return Host.DeviceContext(0)


def renderer(Host, hctx, env):
    rc = Host.RendererConfiguration(W, H)
    rc.FloatLightmap = True
    q = Host.RendererQualitySettings()
    q.MinStepSize, q.LongStepFactor, q.MaxStepCount, q.MaxConeRadius, q.OcclusionToOpacityPower = 1.5, 0.75, dc.MAX_STEP_COUNT, 8.0, 0.8
    rc.DefaultQuality = q
    r = Host.LightingRenderer(hctx, rc, env)
    field = Host.DistanceField(hctx, 48, 32, 32.0, 12, 1.0)
    field.Load(dc.field_atlas(abi.SDF_UNORM16))
    r.DistanceField = field
    return r, field


def sphere(Host, position, color, sort_key=0, functions=(ADD, ADD)):
    l = Host.SphereLightSource()
    l.Position = list(position)
    l.Radius, l.RampLength, l.SortKey = 2.0, 12.0, sort_key
    l.Color = list(color)
    l.BlendColorFunction, l.BlendAlphaFunction = functions
    return l


def environment(Host, blended):
    """two additive spheres around a subtractive one, a MAX directional light over part of the frame and a MIN line light; blended =
    False: the same lights, every one at the default"""
    env = Host.LightingEnvironment()
    env.Ambient = list(AMBIENT)
    env.Lights = [sphere(Host, (9.0, 8.0, 6.0), (1.0, 0.8, 0.6, 0.9), sort_key=0),
                  sphere(Host, (22.0, 12.0, 7.0), (0.5, 0.6, 0.7, 1.0), sort_key=1, functions=(RSUB, ADD) if blended else (ADD, ADD)),
                  sphere(Host, (30.0, 15.0, 8.0), (0.3, 0.5, 1.0, 0.8), sort_key=2)]
    d = Host.DirectionalLightSource()
    d.Bounds = [5.25, 3.5, 30.75, 20.0]
    d.Color = [0.9, 0.2, 0.7, 0.75]
    line = Host.LineLightSource()
    line.StartPosition, line.EndPosition, line.Radius = [6.0, 4.5, 20.0], [40.0, 22.0, 14.0], 2.0
    line.StartColor, line.EndColor = [0.4, 0.3, 0.2, 0.9], [0.1, 0.2, 0.4, 0.7]
    if blended:
        d.BlendColorFunction, d.BlendAlphaFunction = MAX, MAX
        line.BlendColorFunction, line.BlendAlphaFunction = MIN, ADD
    env.DirectionalLights = [d]
    env.LineLights = [line]
    return env


def vertices(rows):
    arr = (abi.LightVertex * len(rows))()
    for i, row in enumerate(rows):
        C.memmove(C.addressof(arr[i]), np.ascontiguousarray(row, np.float32).ctypes.data, 128)
    return arr


def native_frame(ctx, Host, r, env, groups):
    """the frame through the C ABI: groups = [(render function, [packed vertices], (colour function, alpha function) or None)] in the
    mirror's order; None makes no setter call at all (the parent's sequence of calls)"""
    dfu = abi.DistanceFieldUniforms.from_buffer_copy(r.GetDistanceFieldUniformsBytes())
    envu = abi.Environment.from_buffer_copy(r.GetEnvironmentUniformsBytes())
    sdf = native.DistanceFieldTexture(ctx, dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    lm = native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4)
    total = np.zeros(3, np.int64)
    try:
        for k, (render, rows, functions) in enumerate(groups):
            if functions is not None:
                ctx.set_light_blend_function(*functions)
            st = render(ctx, vertices(rows), envu, dfu, None, sdf, AMBIENT if k == 0 else None, lm, want_stats=True)
            total += (st.SdfSamples, st.PixelLightPairs, st.TracedPairs)
        return lm.download(), [int(x) for x in total]
    finally:
        ctx.set_light_blend_function()
        lm.close(); sdf.close()


def assert_an_additive_call_adds(hctx, r, directional):
    """ilm_render_directional_lights of the bounded, unshadowed light `directional` on the renderer's OWN context, onto a lightmap of 0.25"""
    own = native.Context(0, borrowed_handle=hctx.Handle)
    dfu = dc.no_field_uniforms()
    envu = abi.Environment.from_buffer_copy(r.GetEnvironmentUniformsBytes())
    lm = native.Lightmap(own, W, H, abi.LIGHTMAP_FLOAT4)
    base = np.full((H, W, 4), 0.25, np.float32)
    lm.upload(base)
    native.render_directional_lights(own, vertices([directional]), envu, dfu, None, None, None, lm)
    after = lm.download()
    lm.close()
    assert after[10, 10, 3] == 1.25 and (after[10, 10, :3] > 0.25).all(), "an additive call after RenderLighting adds"
    assert_bits_equal(after[0, 0], base[0, 0], "outside the light's bounds nothing changed")


def packed(Host, env):
    s = [np.frombuffer(Host.LightingRenderer.PackSphereLightBytes(l, 1.0, True), np.float32).reshape(8, 4) for l in env.Lights]
    d = np.frombuffer(Host.LightingRenderer.PackDirectionalLightBytes(env.DirectionalLights[0], 1.0), np.float32).reshape(8, 4)
    ln = np.frombuffer(Host.LightingRenderer.PackLineLightBytes(env.LineLights[0], 1.0, True), np.float32).reshape(8, 4)
    return s, d, ln


def test_render_lighting_issues_each_blend_group_with_its_functions(Host, hctx, ctx):
    env = environment(Host, True)
    r, field = renderer(Host, hctx, env)
    stats = r.RenderLighting(1.0, 0, -1, True)
    got = r.ReadLightmap()
    s, d, ln = packed(Host, env)
    # sphere states in first-appearance order (the additive one holds both additive spheres, the subtractive one its own), then the
    # directional state, then the line state
    groups = [(native.render_sphere_lights, [s[0], s[2]], (ADD, ADD)), (native.render_sphere_lights, [s[1]], (RSUB, ADD)),
              (native.render_directional_lights, [d], (MAX, MAX)), (native.render_line_lights, [ln], (MIN, ADD))]
    want, total = native_frame(ctx, Host, r, env, groups)
    assert_bits_equal(got, want, "RenderLighting against the native calls in the mirror's order")
    assert [int(x) for x in stats] == total
    # the blend functions did something: the all-additive frame of the same lights differs, and is brighter where the subtractive sphere lies
    additive, _ = native_frame(ctx, Host, r, env, [(native.render_sphere_lights, [s[0], s[2]], None), (native.render_sphere_lights, [s[1]], None),
                                                   (native.render_directional_lights, [d], None), (native.render_line_lights, [ln], None)])
    assert (additive[12, 22, :3] > got[12, 22, :3]).all() and (got != additive).mean() > 0.5
    # the context was left additive: a native additive call made on the renderer's own context adds
    assert_an_additive_call_adds(hctx, r, d)
    # and a second frame equals the first: no state leaks from one RenderLighting into the next
    r.RenderLighting(1.0, 0, -1, False)
    assert_bits_equal(r.ReadLightmap(), got, "the second frame")


def test_a_frame_that_fails_half_way_leaves_the_context_additive(Host, hctx):
    """the subtractive sphere state has been drawn when the directional state is refused (inverted bounds): the exception passes through
    RenderLighting, and the functions it had set are undone"""
    env = environment(Host, True)
    env.Lights = [env.Lights[1]]
    bad = env.DirectionalLights[0]
    bad.Bounds = [30.0, 2.0, 10.0, 20.0]
    env.DirectionalLights = [bad]
    r, field = renderer(Host, hctx, env)
    with pytest.raises(Exception, match="inverted"):
        r.RenderLighting(1.0, 0, -1, False)
    good = environment(Host, False).DirectionalLights[0]
    assert_an_additive_call_adds(hctx, r, np.frombuffer(Host.LightingRenderer.PackDirectionalLightBytes(good, 1.0), np.float32).reshape(8, 4))


def test_with_every_light_at_the_default_the_frame_is_the_one_rendered_without_the_setter(Host, hctx, ctx):
    env = environment(Host, False)
    r, field = renderer(Host, hctx, env)
    stats = r.RenderLighting(1.0, 0, -1, True)
    got = r.ReadLightmap()
    s, d, ln = packed(Host, env)
    # one sphere state (all three, by SortKey), the directional state, the line state -- and no call of the setter
    want, total = native_frame(ctx, Host, r, env, [(native.render_sphere_lights, s, None), (native.render_directional_lights, [d], None),
                                                  (native.render_line_lights, [ln], None)])
    assert_bits_equal(got, want, "default lights: the frame of the native calls made without the setter")
    assert [int(x) for x in stats] == total
