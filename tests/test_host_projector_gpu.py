"""RenderLighting of the host mirror with projector lights: a frame with two projector textures (two groups) beside sphere and
directional lights equals, bit for bit, the same calls made directly through the C ABI in the same order."""
import ctypes as C
import types

import numpy as np
import pytest

from illuminant_amd import abi, native
from tests import directional_common as dc
from tests import projector_common as pc
from tests.test_projector_gpu import scene_facts
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

W, H = pc.WIDTH, pc.HEIGHT
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
    q.MinStepSize, q.LongStepFactor, q.MaxStepCount, q.MaxConeRadius, q.OcclusionToOpacityPower = 1.5, 0.75, dc.MAX_STEP_COUNT, 8.0, 0.8
    rc.DefaultQuality = q
    r = Host.LightingRenderer(hctx, rc, env)
    field = Host.DistanceField(hctx, 48, 32, 32.0, 12, 1.0)
    field.Load(dc.field_atlas(abi.SDF_UNORM16))
    r.DistanceField = field
    return r, field


def projector(Host, texture, **kw):
    l = Host.ProjectorLightSource()
    l.TextureRef = texture
    for k, v in kw.items():
        setattr(l, k, v)
    return l


def vertices(rows):
    arr = (abi.LightVertex * len(rows))()
    for i, row in enumerate(rows):
        C.memmove(C.addressof(arr[i]), np.ascontiguousarray(row, np.float32).ctypes.data, 128)
    return arr


def test_render_lighting_with_two_projector_textures_equals_the_direct_calls(Host, hctx, ctx, oracle):
    small, large = Host.RampTexture(pc.texture(5, 3)), Host.RampTexture(pc.texture(8, 8))
    env = Host.LightingEnvironment()
    env.Ambient = list(AMBIENT)
    sphere = Host.SphereLightSource()
    sphere.Position, sphere.Radius, sphere.RampLength, sphere.Color = [30.0, 8.0, 10.0], 3.0, 28.0, [0.9, 0.7, 0.5, 1.0]
    env.Lights = [sphere]
    directional = Host.DirectionalLightSource()
    directional.Direction, directional.ShadowTraceLength, directional.Color = [0.55, 0.3, -0.6], 20.0, [0.2, 0.3, 0.4, 0.9]
    env.DirectionalLights = [directional]
    a = projector(Host, small, Scale=[8.0, 8.0], Depth=64.0, Position=[2.3, 1.6, 0.0], Wrap=False, Origin=[24.0, 10.0, 40.0], Radius=2.0, RampLength=30.0,
                  AmbientOcclusionRadius=5.0, AmbientOcclusionOpacity=0.6, Opacity=0.9, SortKey=1)
    b = projector(Host, large, Scale=[2.0, 1.125], Position=[1.25, 0.75, 0.0], Origin=[30.0, 20.0, 35.0], Radius=1.5, RampLength=25.0, Opacity=0.8)
    c = projector(Host, small, Scale=[4.0, 6.0], Position=[18.3, 8.7, 0.0], Wrap=False, Rotation=[0.0, 0.0, float(np.sin(0.2)), float(np.cos(0.2))],
                  TextureRegion=[0.0, 0.0, 1.0, 0.5])
    off = projector(Host, large, Enabled=False)
    untextured = Host.ProjectorLightSource()
    env.ProjectorLights = [a, b, c, off, untextured]
    r, field = host_renderer(Host, hctx, env)
    stats = r.RenderLighting(1.0, 0, -1, True)
    got = r.ReadLightmap()
    r.RenderLighting(1.0, 0, -1, False)
    assert_bits_equal(r.ReadLightmap(), got, "the frame without statistics against the counting frame")
    packed = np.frombuffer(r.GetPackedLightVertices(), np.float32).reshape(-1, 8, 4)
    pack = lambda l: np.frombuffer(Host.LightingRenderer.PackProjectorLightBytes(l, 1.0, True, 128.0, [1.0, 1.0], -0.33), np.float32).reshape(8, 4)
    # SortKey 0: the sphere, the directional light, then b and c in list order; SortKey 1: a.  The untextured light is skipped.
    assert packed.shape[0] == 5
    order = [packed[0], packed[1], pack(b), pack(c), pack(a)]
    assert all(np.array_equal(packed[i], order[i]) for i in range(5))
    assert (got[..., 3] >= 3).any()
    # the same frame through the C ABI: the sphere group (it clears), the directional group, then the projector groups in the order
    # their textures first appear -- large: b; small: c, a
    dfu = abi.DistanceFieldUniforms.from_buffer_copy(r.GetDistanceFieldUniformsBytes())
    envu = abi.Environment.from_buffer_copy(r.GetEnvironmentUniformsBytes())
    sdf = native.DistanceFieldTexture(ctx, dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    lm = native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4)
    # what the two projector groups must contain, from the restatement over the mirror's own uniforms and packed vertices
    otex = oracle.make_texture(dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    scene = types.SimpleNamespace(env=envu, otex=otex, pixels=pc.decode_pixels(oracle, envu, None, W, H))
    for group, texture in (([order[2]], pc.texture(8, 8)), ([order[3], order[4]], pc.texture(5, 3))):
        lights = list(vertices(group))
        scene_facts(scene, lights, pc.render(oracle, lights, texture, envu, dfu, None, otex, None, W, H, pixels=scene.pixels), "a projector group of the host frame")
    total = np.zeros(3, np.int64)

    def add(st):
        total[:] += (st.SdfSamples, st.PixelLightPairs, st.TracedPairs)
    add(native.render_sphere_lights(ctx, vertices([order[0]]), envu, dfu, None, sdf, AMBIENT, lm, want_stats=True))
    add(native.render_directional_lights(ctx, vertices([order[1]]), envu, dfu, None, sdf, None, lm, want_stats=True))
    native.set_projector_texture(ctx, pc.texture(8, 8))
    add(native.render_projector_lights(ctx, vertices([order[2]]), envu, dfu, None, sdf, None, lm, want_stats=True))
    native.set_projector_texture(ctx, pc.texture(5, 3))
    add(native.render_projector_lights(ctx, vertices([order[3], order[4]]), envu, dfu, None, sdf, None, lm, want_stats=True))
    native.set_projector_texture(ctx, None)
    assert_bits_equal(got, lm.download(), "RenderLighting against the direct calls")
    assert [int(x) for x in stats] == [int(x) for x in total]
    assert total[2] > 500
    # projector lights alone: the clear still happens, and the lights are added to it
    env.Lights = []
    env.DirectionalLights = []
    env.ProjectorLights = [b]
    r.RenderLighting(1.0, 0, -1, False)
    lm2 = native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4)
    native.set_projector_texture(ctx, pc.texture(8, 8))
    native.render_projector_lights(ctx, vertices([order[2]]), envu, dfu, None, sdf, AMBIENT, lm2)
    native.set_projector_texture(ctx, None)
    assert_bits_equal(r.ReadLightmap(), lm2.download(), "a frame of projector lights alone")
    for x in (lm, lm2, sdf):
        x.close()


def test_projector_lights_with_probes_are_refused(Host, hctx):
    env = Host.LightingEnvironment()
    env.ProjectorLights = [projector(Host, Host.RampTexture(pc.texture(5, 3)))]
    r, field = host_renderer(Host, hctx, env)
    probe = Host.LightProbe()
    probe.Position = [12.0, 9.0, 2.0]
    r.Probes.Add(probe)
    with pytest.raises(Host.InvalidOperationException, match="projector lights do not reach light probes yet"):
        r.RenderLighting()
    env.ProjectorLights = [projector(Host, Host.RampTexture(pc.texture(5, 3)), Enabled=False)]
    r.RenderLighting()
