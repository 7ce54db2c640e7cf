"""The host mirror's volumetric lights on the device: RenderLighting over an environment with sphere, line and volumetric lights equals the
C ABI calls in the mirror's order, bit for bit -- the volumetric group last, shadowed and unshadowed lights in one call; PackVolumetricLight
is scenes.volumetric_light; volumetric lights and probes are refused.
"""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import volumetric_common as vc
from tests.util import assert_bits_equal, assert_close

pytestmark = pytest.mark.gpu

W, H = vc.WIDTH, vc.HEIGHT
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
    q.MinStepSize, q.LongStepFactor, q.MaxStepCount, q.MaxConeRadius, q.OcclusionToOpacityPower = 1.5, 0.75, vc.MAX_STEP_COUNT, 8.0, 0.8
    rc.DefaultQuality = q
    r = Host.LightingRenderer(hctx, rc, env)
    field = Host.DistanceField(hctx, 48, 32, 32.0, 12, 1.0)
    field.Load(vc.field_atlas(abi.SDF_UNORM16))
    r.DistanceField = field
    return r, field


def host_sphere(Host, position, sort_key=0):
    l = Host.SphereLightSource()
    l.Position = list(position)
    l.Radius, l.RampLength, l.SortKey = 3.0, 28.0, sort_key
    l.Color = [0.9, 0.7, 0.5, 1.0]
    return l


def host_volumetric(Host, **kw):
    l = Host.VolumetricLightSource()
    for k, v in kw.items():
        setattr(l, k, v)
    return l


CONE = dict(Shape=1, StartPosition=[8.0, 6.0, 26.0], EndPosition=[26.0, 18.0, 2.0], StartRadius=2.0, EndRadius=7.0, Color=[1.0, 0.8, 0.6, 0.9], Opacity=0.6,
            Volumetricity=0.5, RampLength=4.0, RampPower=1.5, AmbientOcclusionRadius=5.0, AmbientOcclusionOpacity=0.6)
ELLIPSOID = dict(Shape=0, StartPosition=[42.0, 4.0, 14.0], EndPosition=[24.0, 22.0, -6.0], LightDirection=[0.3, 0.2, -0.9], Color=[0.3, 0.5, 1.0, 0.7],
                 RampLength=3.0, RampPower=0.8, DistanceAttenuation=2.0, SortKey=-1)
BOX = dict(Shape=2, StartPosition=[2.0, 14.0, 0.0], EndPosition=[16.0, 26.0, 10.0], Color=[0.2, 0.9, 0.4, 1.0], RampLength=2.0, CastsShadows=False,
           Volumetricity=2.0, BlowoutFactor=0.25, RampMode=1, ShadowDistanceFalloff=3.0, FalloffYFactor=2.0)


def test_defaults_are_the_references(Host):
    l = Host.VolumetricLightSource()
    assert (l.Shape, l.Volumetricity, l.DistanceAttenuation, l.RampLength, l.RampPower, l.BlowoutFactor) == (1, 1.0, 1.0, 1.0, 1.0, 0.0)
    assert (l.StartRadius, l.EndRadius, l.RampMode, l.Opacity, l.CastsShadows, l.LightDirection) == (0.0, 0.0, 0, 1.0, True, None)
    assert l.Color == [1.0, 1.0, 1.0, 1.0]


def test_pack_volumetric_light_is_the_scene_packing(Host):
    for have_field in (True, False):
        got = Host.LightingRenderer.PackVolumetricLightBytes(host_volumetric(Host, **CONE), 1.25, have_field)
        want = scenes.volumetric_light(shape=1, start=(8.0, 6.0, 26.0), end=(26.0, 18.0, 2.0), start_radius=2.0, end_radius=7.0, color=(1.0, 0.8, 0.6, 0.9),
                                       opacity=0.6, volumetricity=0.5, ramp_length=4.0, ramp_power=1.5, ao_radius=5.0, ao_opacity=0.6,
                                       intensity_scale=1.25, have_field=have_field)
        assert got == bytes(want)
        # an ellipsoid given by its corners in any order: centre and absolute half-extent
        got = Host.LightingRenderer.PackVolumetricLightBytes(host_volumetric(Host, **ELLIPSOID), 1.0, have_field)
        want = scenes.volumetric_light(shape=0, start=(42.0, 4.0, 14.0), end=(24.0, 22.0, -6.0), direction=(0.3, 0.2, -0.9), color=(0.3, 0.5, 1.0, 0.7),
                                       ramp_length=3.0, ramp_power=0.8, distance_attenuation=2.0, have_field=have_field)
        assert got == bytes(want)
        v = np.frombuffer(got, np.float32).reshape(8, 4)
        assert list(v[0]) == [33.0, 13.0, 4.0, 0.0] and list(v[1]) == [9.0, 9.0, 10.0, 0.0] and v[3][3] == (1.0 if have_field else 0.0)
        got = Host.LightingRenderer.PackVolumetricLightBytes(host_volumetric(Host, **BOX), 1.0, have_field)
        want = scenes.volumetric_light(shape=2, start=(2.0, 14.0, 0.0), end=(16.0, 26.0, 10.0), color=(0.2, 0.9, 0.4, 1.0), ramp_length=2.0,
                                       casts_shadows=False, volumetricity=2.0, blowout=0.25, ramp_mode=1, shadow_distance_falloff=3.0, falloff_y=2.0,
                                       have_field=have_field)
        assert got == bytes(want)
    assert Host.LightingRenderer.PackVolumetricLightBytes(host_volumetric(Host, Opacity=0.0, **{k: v for k, v in BOX.items()}), 1.0, True) is None
    assert Host.LightingRenderer.PackVolumetricLightBytes(host_volumetric(Host, Opacity=-1.0), 1.0, True) is None
    assert Host.LightingRenderer.PackVolumetricLightBytes(host_volumetric(Host, Shape=3), 1.0, True) is None


def test_render_lighting_over_sphere_line_and_volumetric_lights_equals_the_direct_calls(Host, hctx, ctx, oracle):
    """type ordering: the sphere group clears and lights, the line group adds, the volumetric group adds last (LightSourceTypeID
    Volumetric = 6); shadowed and unshadowed volumetric lights share the call in sorted order; a disabled light, one with Opacity 0 and
    one of an unknown shape are left out"""
    env = Host.LightingEnvironment()
    env.Ambient = list(AMBIENT)
    env.Lights = [host_sphere(Host, (30.0, 8.0, 10.0)), host_sphere(Host, (10.0, 20.0, 6.0))]
    ll = Host.LineLightSource()
    ll.StartPosition, ll.EndPosition, ll.Radius = [6.0, 4.5, 20.0], [40.0, 22.0, 14.0], 2.0
    env.LineLights = [ll]
    a, b, c = host_volumetric(Host, **CONE), host_volumetric(Host, **ELLIPSOID), host_volumetric(Host, **BOX)
    env.VolumetricLights = [a, host_volumetric(Host, Enabled=False, **BOX), c, b, host_volumetric(Host, Opacity=0.0), host_volumetric(Host, Shape=7)]
    r, field = host_renderer(Host, hctx, env)
    stats = r.RenderLighting(1.0, 0, -1, True)
    got = r.ReadLightmap()
    r.RenderLighting(1.0, 0, -1, False)
    assert_bits_equal(r.ReadLightmap(), got, "the frame without statistics against the counting frame")
    packed = np.frombuffer(r.GetPackedLightVertices(), np.float32).reshape(-1, 8, 4)
    volumetric = lambda l: np.frombuffer(Host.LightingRenderer.PackVolumetricLightBytes(l, 1.0, True), np.float32).reshape(8, 4)
    sphere = lambda l: np.frombuffer(Host.LightingRenderer.PackSphereLightBytes(l, 1.0, True), np.float32).reshape(8, 4)
    line = np.frombuffer(Host.LightingRenderer.PackLineLightBytes(ll, 1.0, True), np.float32).reshape(8, 4)
    # SortKey first: b (-1), then key 0 in type order: the spheres, the line light, then a and c in list order
    order = [volumetric(b), sphere(env.Lights[0]), sphere(env.Lights[1]), line, volumetric(a), volumetric(c)]
    assert packed.shape[0] == 6 and all(np.array_equal(packed[i], order[i]) for i in range(6))
    dfu = abi.DistanceFieldUniforms.from_buffer_copy(r.GetDistanceFieldUniformsBytes())
    envu = abi.Environment.from_buffer_copy(r.GetEnvironmentUniformsBytes())
    assert bytes(dfu) == bytes(vc.field_uniforms())
    sdf = native.DistanceFieldTexture(ctx, vc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
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
    add(native.render_line_lights(ctx, vertices([order[3]]), envu, dfu, None, sdf, None, lm, want_stats=True))
    before = lm.download()
    group = [order[0], order[4], order[5]]
    group_stats = add(native.render_volumetric_lights(ctx, vertices(group), envu, dfu, None, sdf, None, lm, want_stats=True))
    assert_bits_equal(got, lm.download(), "RenderLighting against the direct calls")
    assert [int(x) for x in stats] == [int(x) for x in total]
    # and the volumetric part against the restatement, on top of what the other groups left
    otex = oracle.make_texture(vc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    want = vc.render(oracle, vertices(group), envu, dfu, None, otex, None, W, H, before=before)
    assert_close(got, want.image, "RenderLighting against the restatement")
    assert (group_stats.SdfSamples, group_stats.PixelLightPairs, group_stats.TracedPairs) == want.stats and want.stats[2] > 300
    # volumetric lights alone: the clear still happens, then they add
    env.Lights = []
    env.LineLights = []
    r.RenderLighting(1.0, 0, -1, False)
    alone = vc.render(oracle, vertices(group), envu, dfu, None, otex, AMBIENT, W, H)
    assert_close(r.ReadLightmap(), alone.image, "a frame of volumetric lights alone is cleared first")
    for x in (lm, sdf):
        x.close()


def test_volumetric_lights_with_probes_are_refused(Host, hctx):
    env = Host.LightingEnvironment()
    env.Lights = [host_sphere(Host, (10.0, 10.0, 5.0))]
    env.VolumetricLights = [host_volumetric(Host, **CONE)]
    r, field = host_renderer(Host, hctx, env)
    probe = Host.LightProbe()
    probe.Position = [12.0, 9.0, 2.0]
    r.Probes.Add(probe)
    with pytest.raises(Host.InvalidOperationException, match="volumetric lights do not reach light probes yet"):
        r.RenderLighting()
    env.VolumetricLights = [host_volumetric(Host, Enabled=False, **CONE)]
    r.RenderLighting()
    assert r.Probes[0].Value[3] > 0
