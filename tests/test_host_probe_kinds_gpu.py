"""LightingRenderer.ProbeLightKinds, the mirror's switch for the light kinds whose render states reach the probes: the default {Sphere}
behaves as before, {Sphere, Directional, Line} sums every state's probe call in the order RenderLighting draws the states, and
projector and volumetric lights cannot be added.  Every comparison is exact."""
import numpy as np
import pytest

from illuminant_amd import abi, native
from tests import directional_common as dc
from tests import light_blend_common as lb
from tests import projector_common as pc
from tests.test_host_render_states_gpu import AMBIENT, SPHERE, make, renderer, rows_of, uniforms, vertices
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Host():
    from illuminant_amd import _host
    return _host


@pytest.fixture(scope="module")
def hctx(Host):
    return Host.DeviceContext(0)


def probe_list(Host):
    return [make(Host.LightProbe, Position=[22.0, 14.0, 1.0]), make(Host.LightProbe, Position=[28.0, 16.0, 2.0], Normal=[0.0, 0.6, 0.8]),
            make(Host.LightProbe, Position=[12.0, 12.0, 1.0], EnableShadows=False), make(Host.LightProbe, Position=[23.5, 12.5, 0.5], Normal=[0.0, 0.0, 1.0])]


def probe_arrays(probes):
    pp = np.array([p.Position + [1.0] for p in probes], np.float32)
    pn = np.array([(p.Normal or [0.0, 0.0, 0.0]) + [1.0 if p.EnableShadows else 0.0] for p in probes], np.float32)
    return pp, pn


def values_of(r, n):
    return np.array([r.Probes[i].Value for i in range(n)], np.float32)


def direct_sum(ctx, envu, dfu, pp, pn, calls):
    """calls = [(probe entry, [packed vertices], ramp texels or None)] in group order: the parts added in fp32 as they come"""
    sdf = native.DistanceFieldTexture(ctx, dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)
    total = np.zeros((pp.shape[0], 4), np.float32)
    parts = []
    try:
        for entry, rows, ramp in calls:
            ctx.set_light_ramp(ramp)
            part = entry(ctx, vertices(rows), pp, pn, envu, dfu, sdf)
            parts.append(part)
            total = (total + part).astype(np.float32)
    finally:
        ctx.set_light_ramp(None)
        sdf.close()
    return total, parts


def sphere_scene(Host):
    ramp = dc.ramp_texture()
    env = Host.LightingEnvironment()
    env.Ambient = list(AMBIENT)
    plain = make(Host.SphereLightSource, Position=[30.0, 18.0, 6.0], **SPHERE)
    ramp_texture = Host.RampTexture(ramp)
    ramped = make(Host.SphereLightSource, Position=[20.0, 12.0, 8.0], TextureRef=ramp_texture, **SPHERE)
    off = make(Host.SphereLightSource, Position=[30.0, 30.0, 6.0], Enabled=False, **SPHERE)
    env.Lights = [plain, off, ramped]
    return env, plain, ramped, ramp, ramp_texture


def test_the_default_set_is_sphere_alone_and_behaves_as_before(Host, hctx, ctx):
    env, plain, ramped, ramp, _texture = sphere_scene(Host)
    r, field = renderer(Host, hctx, env)
    assert r.ProbeLightKinds == {Host.LightKind.Sphere}
    probes = probe_list(Host)
    for p in probes:
        r.Probes.Add(p)
    r.RenderLighting(2.0)
    frame = r.ReadLightmap()
    got = values_of(r, len(probes))
    envu, dfu = uniforms(r)
    pp, pn = probe_arrays(probes)
    pack = lambda l: rows_of(Host.LightingRenderer.PackSphereLightBytes(l, 2.0, True))[0]
    total, _parts = direct_sum(ctx, envu, dfu, pp, pn, [(native.render_light_probes, [pack(plain)], None), (native.render_light_probes, [pack(ramped)], ramp)])
    assert_bits_equal(got, lb.half(total) * np.float32(0.5), "probe values: the two sphere states")
    assert (got[:, :3] > 0).any()
    # setting the default explicitly changes nothing, in the frame or in the probes
    again, _ = renderer(Host, hctx, env)
    again.ProbeLightKinds = {Host.LightKind.Sphere}
    for p in probe_list(Host):
        again.Probes.Add(p)
    again.RenderLighting(2.0)
    assert_bits_equal(again.ReadLightmap(), frame, "the frame")
    assert_bits_equal(values_of(again, len(probes)), got, "the probe values")


def test_kinds_without_a_defined_probe_technique_cannot_be_set(Host, hctx):
    env = Host.LightingEnvironment()
    r, field = renderer(Host, hctx, env)
    K = Host.LightKind
    with pytest.raises(Host.InvalidOperationException) as refusal:
        r.ProbeLightKinds = {K.Sphere, K.Projector}
    assert "projector lights cannot reach light probes" in str(refusal.value) and "TEXCOORD6" in str(refusal.value)
    with pytest.raises(Host.InvalidOperationException) as refusal:
        r.ProbeLightKinds = {K.Sphere, K.Line, K.Volumetric}
    assert "volumetric lights cannot reach light probes" in str(refusal.value) and "VolumetricLightProbe.fx" in str(refusal.value)
    with pytest.raises(Host.InvalidOperationException) as refusal:
        r.ProbeLightKinds = {K.Directional, K.Line}
    assert "sphere lights cannot be removed" in str(refusal.value)
    assert r.ProbeLightKinds == {K.Sphere}, "a refused set leaves the switch as it was"
    r.ProbeLightKinds = {K.Sphere, K.Line}
    assert r.ProbeLightKinds == {K.Sphere, K.Line}


@pytest.mark.parametrize("allowed,refused", [("Line", "directional"), ("Directional", "line")])
def test_a_kind_outside_the_set_is_refused_as_before(Host, hctx, allowed, refused):
    env = Host.LightingEnvironment()
    env.Lights = [make(Host.SphereLightSource, Position=[10.0, 10.0, 5.0], **SPHERE)]
    env.DirectionalLights = [make(Host.DirectionalLightSource)]
    env.LineLights = [make(Host.LineLightSource, Radius=2.0)]
    r, field = renderer(Host, hctx, env)
    r.ProbeLightKinds = {Host.LightKind.Sphere, getattr(Host.LightKind, allowed)}
    r.Probes.Add(make(Host.LightProbe, Position=[12.0, 9.0, 2.0]))
    with pytest.raises(Host.InvalidOperationException) as refusal:
        r.RenderLighting()
    assert str(refusal.value) == "RenderLighting: %s lights do not reach light probes yet" % refused
    assert len(r.GetPackedLightVertices()) == 0, "refused before anything is packed"


def test_sphere_directional_and_line_states_are_summed_in_group_order(Host, hctx, ctx):
    env, s_plain, s_ramped, ramp, ramp_texture = sphere_scene(Host)
    d_ramped = make(Host.DirectionalLightSource, Direction=[0.55, 0.3, -0.6], ShadowTraceLength=20.0, ShadowSoftness=2.0, Color=[0.2, 0.3, 0.4, 0.9],
                    TextureRef=ramp_texture)
    d_plain = make(Host.DirectionalLightSource, Direction=[1.0, 0.0, -0.5], ShadowTraceLength=24.0, ShadowSoftness=2.0, Bounds=[60.0, 30.0, 70.0, 38.0],
                   Color=[0.9, 0.2, 0.7, 0.75])
    d_off = make(Host.DirectionalLightSource, Color=[1.0, 1.0, 1.0, 1.0], Enabled=False)
    env.DirectionalLights = [d_ramped, d_off, d_plain]
    line = make(Host.LineLightSource, StartPosition=[26.0, 14.0, 9.0], EndPosition=[8.0, 36.0, 12.0], Radius=12.0, StartColor=[0.4, 0.3, 0.2, 0.9],
                EndColor=[0.1, 0.2, 0.4, 0.7], TextureRef=ramp_texture)
    l_off = make(Host.LineLightSource, StartPosition=[6.0, 4.5, 20.0], EndPosition=[64.0, 34.0, 14.0], Radius=9.0, Enabled=False)
    env.LineLights = [l_off, line]
    env.ProjectorLights = [make(Host.ProjectorLightSource, TextureRef=Host.RampTexture(pc.texture(5, 3)), Enabled=False)]
    env.VolumetricLights = [make(Host.VolumetricLightSource, Enabled=False)]
    K = Host.LightKind

    without, _ = renderer(Host, hctx, env)
    without.RenderLighting(2.0)
    frame = without.ReadLightmap()

    r, field = renderer(Host, hctx, env)
    r.ProbeLightKinds = {K.Sphere, K.Directional, K.Line}
    probes = probe_list(Host)
    for p in probes:
        r.Probes.Add(p)
    r.RenderLighting(2.0)
    assert_bits_equal(r.ReadLightmap(), frame, "the lightmap with probes against the same scene without")
    got = values_of(r, len(probes))

    envu, dfu = uniforms(r)
    pp, pn = probe_arrays(probes)
    L = Host.LightingRenderer
    sphere = lambda l: rows_of(L.PackSphereLightBytes(l, 2.0, True))[0]
    directional = lambda l: rows_of(L.PackDirectionalLightBytes(l, 2.0))[0]
    packed_line = rows_of(L.PackLineLightBytes(line, 2.0, True))[0]
    assert packed_line[3][1] == 0, "PackLineLight writes ramp length 0"
    calls = [(native.render_light_probes, [sphere(s_plain)], None), (native.render_light_probes, [sphere(s_ramped)], ramp),
             (native.render_directional_light_probes, [directional(d_ramped)], ramp), (native.render_directional_light_probes, [directional(d_plain)], None),
             (native.render_line_light_probes, [packed_line], None)]
    total, parts = direct_sum(ctx, envu, dfu, pp, pn, calls)
    assert_bits_equal(got, lb.half(total) * np.float32(0.5), "probe values: half(the five calls' sum) / intensityScale")
    # every call is needed for that, the bounded directional light's included (its Bounds exclude every probe)
    for k, part in enumerate(parts):
        assert (part[:, 3] > 0).any(), "call %d lights a probe" % k
    # the directional states were under their own ramps: the ramped state's part is not what it is without the ramp, and the line's is
    _, (d_part, l_part) = direct_sum(ctx, envu, dfu, pp, pn, [calls[2], calls[4]])
    assert (direct_sum(ctx, envu, dfu, pp, pn, [(calls[2][0], calls[2][1], None)])[0] != d_part).any()
    assert_bits_equal(direct_sum(ctx, envu, dfu, pp, pn, [(calls[4][0], calls[4][1], ramp)])[0], l_part, "the line probes read no ramp")

    # a projector light in that scene is still refused
    env.ProjectorLights = [make(Host.ProjectorLightSource, TextureRef=Host.RampTexture(pc.texture(5, 3)))]
    with pytest.raises(Host.InvalidOperationException) as refusal:
        r.RenderLighting(2.0)
    assert str(refusal.value) == "RenderLighting: projector lights do not reach light probes yet"
