"""The host mirror's line lights on the device: RenderLighting over an environment with sphere, directional and line lights equals the
three C ABI calls in the mirror's order, bit for bit; PackLineLight is scenes.line_light; line lights and probes are refused.
"""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import line_common as lc
from tests.util import assert_bits_equal, assert_close

pytestmark = pytest.mark.gpu

W, H = lc.WIDTH, lc.HEIGHT
AMBIENT = (0.0213, 0.0377, 0.0591, 1.0)


@pytest.fixture(scope="module")
def Host():
    from illuminant_amd import _host
    return _host


@pytest.fixture(scope="module")
def hctx(Host):
    return Host.DeviceContext(0)


def host_renderer(Host, hctx, env):
    rc = Host.RendererConfiguration(W, H)
    rc.FloatLightmap = True
    q = Host.RendererQualitySettings()
    q.MinStepSize, q.LongStepFactor, q.MaxStepCount, q.MaxConeRadius, q.OcclusionToOpacityPower = 1.5, 0.75, lc.MAX_STEP_COUNT, 8.0, 0.8
    rc.DefaultQuality = q
    r = Host.LightingRenderer(hctx, rc, env)
    field = Host.DistanceField(hctx, 48, 32, 32.0, 12, 1.0)
    field.Load(lc.field_atlas(abi.SDF_UNORM16))
    r.DistanceField = field
    return r, field


def host_sphere(Host, position, sort_key=0):
    l = Host.SphereLightSource()
    l.Position = list(position)
    l.Radius, l.RampLength, l.SortKey = 3.0, 28.0, sort_key
    l.Color = [0.9, 0.7, 0.5, 1.0]
    return l


def host_line(Host, **kw):
    l = Host.LineLightSource()
    for k, v in kw.items():
        setattr(l, k, v)
    return l


LINE_A = dict(StartPosition=[6.0, 4.5, 20.0], EndPosition=[40.0, 22.0, 14.0], Radius=2.0, StartColor=[1.0, 0.8, 0.6, 0.9], EndColor=[0.3, 0.5, 1.0, 0.7],
              AmbientOcclusionRadius=5.0, AmbientOcclusionOpacity=0.6, Opacity=0.8)
LINE_B = dict(StartPosition=[30.0, 14.0, 4.0], EndPosition=[30.0, 14.0, 28.0], Radius=1.5, StartColor=[0.2, 0.9, 0.4, 1.0], EndColor=[0.9, 0.2, 0.4, 1.0],
              SortKey=-1)


def test_pack_line_light_is_the_scene_packing(Host):
    for have_field in (True, False):
        got = Host.LightingRenderer.PackLineLightBytes(host_line(Host, **LINE_A), 1.25, have_field)
        want = scenes.line_light((6.0, 4.5, 20.0), (40.0, 22.0, 14.0), 2.0, start_color=(1.0, 0.8, 0.6, 0.9), end_color=(0.3, 0.5, 1.0, 0.7), opacity=0.8,
                                 intensity_scale=1.25, have_distance_field=have_field, ao_radius=5.0, ao_opacity=0.6)
        assert got == bytes(want)
    assert Host.LightingRenderer.PackLineLightBytes(host_line(Host, Opacity=0.0, **{k: v for k, v in LINE_B.items()}), 1.0, True) is None
    assert Host.LightingRenderer.PackLineLightBytes(host_line(Host, Opacity=-1.0), 1.0, True) is None


def test_render_lighting_over_sphere_directional_and_line_lights_equals_the_direct_calls(Host, hctx, ctx, oracle):
    """type ordering: the sphere group clears and lights, the directional group adds, the line group adds after it (LightSourceTypeID
    Line = 4 after Directional = 2); a disabled line light and one with Opacity 0 are left out"""
    env = Host.LightingEnvironment()
    env.Ambient = list(AMBIENT)
    env.Lights = [host_sphere(Host, (30.0, 8.0, 10.0)), host_sphere(Host, (10.0, 20.0, 6.0))]
    d = Host.DirectionalLightSource()
    d.Direction, d.ShadowTraceLength, d.ShadowSoftness, d.Color = [0.55, 0.3, -0.6], 20.0, 2.0, [1.0, 0.8, 0.6, 0.5]
    env.DirectionalLights = [d]
    a, b = host_line(Host, **LINE_A), host_line(Host, **LINE_B)
    env.LineLights = [a, host_line(Host, Enabled=False, **LINE_B), b, host_line(Host, Opacity=0.0, Radius=2.0)]
    r, field = host_renderer(Host, hctx, env)
    stats = r.RenderLighting(1.0, 0, -1, True)
    got = r.ReadLightmap()
    r.RenderLighting(1.0, 0, -1, False)
    assert_bits_equal(r.ReadLightmap(), got, "the frame without statistics against the counting frame")
    packed = np.frombuffer(r.GetPackedLightVertices(), np.float32).reshape(-1, 8, 4)
    line = lambda l: np.frombuffer(Host.LightingRenderer.PackLineLightBytes(l, 1.0, True), np.float32).reshape(8, 4)
    sphere = lambda l: np.frombuffer(Host.LightingRenderer.PackSphereLightBytes(l, 1.0, True), np.float32).reshape(8, 4)
    directional = np.frombuffer(Host.LightingRenderer.PackDirectionalLightBytes(d, 1.0), np.float32).reshape(8, 4)
    # SortKey first: b (-1), then key 0 in type order: the spheres, the directional light, a
    order = [line(b), sphere(env.Lights[0]), sphere(env.Lights[1]), directional, line(a)]
    assert packed.shape[0] == 5 and all(np.array_equal(packed[i], order[i]) for i in range(5))
    dfu = abi.DistanceFieldUniforms.from_buffer_copy(r.GetDistanceFieldUniformsBytes())
    envu = abi.Environment.from_buffer_copy(r.GetEnvironmentUniformsBytes())
    assert bytes(dfu) == bytes(lc.field_uniforms())
    sdf = native.DistanceFieldTexture(ctx, lc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    lm = native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4)

    def vertices(rows):
        arr = (abi.LightVertex * len(rows))()
        for i, row in enumerate(rows):
            C.memmove(C.addressof(arr[i]), np.ascontiguousarray(row, np.float32).ctypes.data, 128)
        return arr
    total = np.zeros(3, np.int64)

    def add(st):
        total[:] += (st.SdfSamples, st.PixelLightPairs, st.TracedPairs)
        return st
    add(native.render_sphere_lights(ctx, vertices([order[1], order[2]]), envu, dfu, None, sdf, AMBIENT, lm, want_stats=True))
    add(native.render_directional_lights(ctx, vertices([order[3]]), envu, dfu, None, sdf, None, lm, want_stats=True))
    before_lines = lm.download()
    line_stats = add(native.render_line_lights(ctx, vertices([order[0], order[4]]), envu, dfu, None, sdf, None, lm, want_stats=True))
    assert_bits_equal(got, lm.download(), "RenderLighting against the direct calls")
    assert [int(x) for x in stats] == [int(x) for x in total]
    # and the line part against the restatement, on top of what the other groups left
    otex = oracle.make_texture(lc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    want = lc.render(oracle, vertices([order[0], order[4]]), envu, dfu, None, otex, None, W, H, before=before_lines)
    assert_close(got, want.image, "RenderLighting against the restatement")
    assert (line_stats.SdfSamples, line_stats.PixelLightPairs, line_stats.TracedPairs) == want.stats and want.stats[2] > 50
    # line lights alone: the clear still happens, then they add
    env.Lights = []
    env.DirectionalLights = []
    r.RenderLighting(1.0, 0, -1, False)
    alone = lc.render(oracle, vertices([order[0], order[4]]), envu, dfu, None, otex, AMBIENT, W, H)
    assert_close(r.ReadLightmap(), alone.image, "a frame of line lights alone is cleared first")
    for x in (lm, sdf):
        x.close()


def test_line_lights_with_probes_are_refused(Host, hctx):
    env = Host.LightingEnvironment()
    env.Lights = [host_sphere(Host, (10.0, 10.0, 5.0))]
    env.LineLights = [host_line(Host, **LINE_A)]
    r, field = host_renderer(Host, hctx, env)
    probe = Host.LightProbe()
    probe.Position = [12.0, 9.0, 2.0]
    r.Probes.Add(probe)
    with pytest.raises(Host.InvalidOperationException, match="line lights do not reach light probes yet"):
        r.RenderLighting()
    env.LineLights = [host_line(Host, Enabled=False, **LINE_A)]
    r.RenderLighting()
    assert r.Probes[0].Value[3] > 0
