"""Known answers for the projector-light pass, derived by hand, against the float32 restatement of tests/projector_common.py and the
host mirror's packing.  No GPU: the entry points are looked up in the built library, nothing is launched."""
import os
import re

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import projector_common as pc

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def entry_points():
    """what the restatement restates must exist: the library exports both entry points and the binding knows them (most cases below
    pin the Python restatement alone, as the GPU tests are only as good as it is; this fixture ties them to the feature)"""
    for name in ("ilm_ctx_set_projector_texture", "ilm_render_projector_lights"):
        assert name in native.SYMBOLS
        assert hasattr(native.lib(), name)
    assert hasattr(native, "render_projector_lights") and hasattr(native, "set_projector_texture")


def axis_aligned(**kw):
    """32 x 16 world units at (4, 8), 64 deep: every entry of the inverse is a power of two or a small multiple of one -- exact in fp32"""
    return pc.projector_light(pc.forward_matrix((32.0, 16.0, 64.0), (4.0, 8.0, 0.0)), **kw)


def unit(**kw):
    """texture space = world space: the identity matrix"""
    return pc.projector_light(np.eye(4), **kw)


def test_header_binding_and_csharp_agree_on_the_symbols():
    text = open(os.path.join(ROOT, "include", "illuminant_hip.h")).read()
    decl = re.search(r"^int32_t ilm_render_projector_lights\(([^)]*)\)", text, flags=re.M).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in decl.split(",")] == [
        "IlmHandle", "const IlmLightVertex*", "int32_t", "const IlmEnvironment*", "const IlmDistanceFieldUniforms*", "IlmHandle", "IlmHandle",
        "const float", "IlmHandle", "int32_t", "int32_t", "IlmRenderStats*"]
    assert native.SYMBOLS["ilm_render_projector_lights"] == native.SYMBOLS["ilm_render_directional_lights"]
    decl = re.search(r"^int32_t ilm_ctx_set_projector_texture\(([^)]*)\)", text, flags=re.M).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in decl.split(",")] == ["IlmHandle", "const IlmFloat4*", "int32_t", "int32_t"]
    assert native.SYMBOLS["ilm_ctx_set_projector_texture"] == native.SYMBOLS["ilm_ctx_set_light_ramp"]
    cs = open(os.path.join(ROOT, "integration", "IlluminantHip.cs")).read()
    assert "ilm_render_projector_lights (ulong ctx, LightVertex* lights, int lightCount" in cs
    assert "ilm_ctx_set_projector_texture (ulong ctx, Vector4* texels, int width, int height)" in cs
    assert "#define ILM_ABI_VERSION 11" in text
    contract = text[text.index("/* The projector-light pass"):text.index("int32_t ilm_render_projector_lights")]
    for word in ("DEFINED DEVIATION", "ProjectorLightProbe.fx", "mip chains", "group entry point", "ProjectorLightWithoutDistanceField"):
        assert word in contract, word


def test_scale_and_translation_place_chosen_pixels_exactly():
    l = axis_aligned()
    rows = pc.matrix_rows(l)
    assert [float(rows[k][k]) for k in range(4)] == [1 / 32, 1 / 16, 1 / 64, 1.0]
    assert [float(c) for c in rows[3][:3]] == [-0.125, -0.5, 0.0]
    for shaded, want in (((20.0, 16.0, 32.0), (0.5, 0.5, 0.5)), ((4.0, 8.0, 0.0), (0.0, 0.0, 0.0)), ((36.0, 24.0, 64.0), (1.0, 1.0, 1.0)),
                         ((12.0, 20.0, -5.0), (0.25, 0.75, 0.0))):          # (z below 0 is forced up to 0)
        (u, v), opacity, visible, facts = pc.project(rows, l, shaded)
        assert tuple(float(c) for c in facts["projected"]) == want and (float(u), float(v)) == want[:2]
        assert visible and opacity == 1


def test_the_edge_band_of_a_clamped_light():
    l = unit()
    rows = pc.matrix_rows(l)
    (u, v), opacity, visible, _ = pc.project(rows, l, (1.0005, 0.5, 0.5))
    assert visible and abs(float(opacity) - 0.5) < 1e-3
    assert float(u) == 1.0                                    # clamped onto the region's edge
    _, opacity, visible, _ = pc.project(rows, l, (1.002, 0.5, 0.5))
    assert opacity == 0 and not visible                       # 0.002 outside: past the 0.001 band, discarded
    _, opacity, visible, _ = pc.project(rows, l, (0.5, 0.5, 1.0005))      # the band exists on z as well
    assert visible and abs(float(opacity) - 0.5) < 1e-3


def test_wrap_against_clamp_outside_the_region():
    shaded = (1.25, -0.5, 0.25)
    clamped, wrapping = unit(), unit(wrap=True)
    assert clamped.MoreLightProperties.z == 1.0 and wrapping.MoreLightProperties.z == 0.0
    assert pc.project(pc.matrix_rows(clamped), clamped, shaded)[2] is False
    (u, v), opacity, visible, _ = pc.project(pc.matrix_rows(wrapping), wrapping, shaded)
    assert visible and opacity == 1 and (float(u), float(v)) == (1.25, -0.5)
    # ... and the fetch wraps: (1.25, -0.5) reads what (0.25, 0.5) reads
    t = pc.texture(8, 8)
    assert [float(c) for c in pc.fetch(t, u, v)] == [float(c) for c in pc.fetch(t, 0.25, 0.5)]
    # an opacity of 0 hides either kind
    dark = unit(wrap=True, opacity=0.0)
    assert pc.project(pc.matrix_rows(dark), dark, (0.5, 0.5, 0.5))[2] is False


def test_without_an_origin_the_normal_factor_is_not_evaluated():
    l = unit(origin=None)
    assert tuple(l.LightPosition3.__getattribute__(k) for k in "xyzw") == (0, 0, 0, 0) and l.LightProperties.w == 0
    assert pc.normal_opacity(l, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)) == 1          # shaded == origin == 0: the reference's NaN
    assert pc.normal_opacity(l, (3.0, 4.0, 5.0), (0.6, 0.0, 0.8)) == 1
    # with an origin straight above, a surface facing up takes the full factor, one facing away none, a zero normal 1
    above = unit(origin=(0.5, 0.5, 10.0))
    assert pc.normal_opacity(above, (0.5, 0.5, 0.0), (0.0, 0.0, 1.0)) == 1
    assert pc.normal_opacity(above, (0.5, 0.5, 0.0), (0.0, 0.0, -1.0)) == 0
    assert pc.normal_opacity(above, (0.5, 0.5, 0.0), (0.0, 0.0, 0.0)) == 1
    # dot = 0 (a surface edge-on): ((0 + 0.15) / 0.15) ^ 0.85 = 1
    assert pc.normal_opacity(above, (0.5, 0.5, 0.0), (1.0, 0.0, 0.0)) == 1


def test_a_wrap_fetch_at_u_zero_mixes_the_last_and_the_first_column():
    t = pc.texture(5, 3)
    v = F(0.5) / F(3)                           # the centre of row 0: s = 0, weight 0
    got = pc.fetch(t, 0.0, v)
    for k in range(4):
        assert got[k] == pc.lerp(t[0, 4, k], t[0, 0, k], 0.5)
    # a texel centre reads that texel alone; one whole texture further on (and back) the same taps
    assert [float(c) for c in pc.fetch(t, 0.5, 0.5)] == [float(c) for c in t[1, 2]]
    assert [float(c) for c in pc.fetch(t, 2.5, -1.5)] == [float(c) for c in t[1, 2]]
    # a non-finite coordinate names tap 0 with a NaN weight
    assert all(np.isnan(c) for c in pc.fetch(t, float("inf"), v))


def test_the_bounding_box_of_an_axis_aligned_projector():
    """the world rectangle 4 .. 36 x 8 .. 24 padded in y by MaximumZ * ZToY = 128 * 0.25, then the viewport mapping"""
    l = axis_aligned()
    env = scenes.environment(maximum_z=128.0, z_to_y=0.25)
    assert tuple(float(c) for c in pc.world_rectangle(l, env)) == (4.0, 8.0 - 32.0, 36.0, 24.0 + 32.0)
    env = scenes.environment(maximum_z=128.0, z_to_y=0.25, viewport_position=(2.0, -4.0), viewport_scale=(2.0, 0.5), render_scale=(0.5, 4.0))
    assert tuple(float(c) for c in pc.footprint(l, env)) == (2.0, -40.0, 34.0, 120.0)
    fp64 = pc.footprint64(l, env)
    assert np.allclose(fp64, (2.0, -40.0, 34.0, 120.0), rtol=0, atol=1e-9)
    # a wrapping light's quad is the whole world
    assert tuple(float(c) for c in pc.world_rectangle(axis_aligned(wrap=True), env)) == (-9999.0, -9999.0, 9999.0, 9999.0)
    # a rotated one: the box of the rotated rectangle's corners (30 degrees about z, 32 x 16 at the origin)
    rotated = pc.projector_light(pc.forward_matrix((32.0, 16.0, 64.0), (0.0, 0.0, 0.0), rotation_z=np.pi / 6))
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    want = (-16.0 * s, 0.0, 32.0 * c, 32.0 * s + 16.0 * c)
    assert np.allclose([float(v) for v in pc.world_rectangle(rotated, scenes.environment())], want, rtol=0, atol=1e-4)
    # a singular matrix has no inverse: the rectangle covers nothing
    flat = pc.projector_light(np.eye(4))
    flat.LightPosition1 = abi.f4(0, 0, 0, 0)
    fp = pc.footprint(flat, scenes.environment())
    assert not any(pc.covers(fp, x, y) for x in range(0, 44, 7) for y in range(0, 27, 5))


def test_invert_matrix_inverts():
    m = pc.forward_matrix((20.0, 12.0, 32.0), (7.0, 3.0, 1.0), rotation_z=0.4, perspective_x=0.01)
    rows = [[F(v) for v in r] for r in m]
    inv = np.array(pc.invert_matrix(rows), np.float64)
    assert np.allclose(np.array(rows, np.float64) @ inv, np.eye(4), rtol=0, atol=1e-5)


# ---- the host mirror's packing -------------------------------------------------------------------------------------------------

def host_light(H, size=(8, 8), **kw):
    l = H.ProjectorLightSource()
    l.TextureRef = H.RampTexture(pc.texture(*size))
    for k, v in kw.items():
        setattr(l, k, v)
    return l


def test_pack_projector_light_scale_and_translation_in_closed_form():
    """m = Transform * Scale(texture size * Scale, Depth) * Translation(Position), inverted: an 8 x 8 texture at scale (4, 2), depth 64,
    position (4, 8, 0) -- every product a power of two times a small integer, so the closed form diag(1 / 32, 1 / 16, 1 / 64) with the
    last row -(4 / 32, 8 / 16, 0) is what fp32 gives exactly."""
    from illuminant_amd import _host as H
    d = H.ProjectorLightSource()
    assert d.Wrap and d.Origin is None and d.Depth is None and d.Radius == 0 and d.RampLength == 1 and d.Opacity == 1      # LightSource.cs:507-537
    assert d.TextureRegion == [0.0, 0.0, 1.0, 1.0] and d.Rotation == [0.0, 0.0, 0.0, 1.0] and d.Scale == [1.0, 1.0]
    assert H.LightingRenderer.PackProjectorLightBytes(d) is None                 # no texture: skipped (LightingRenderer.cs:1389-1391)
    l = host_light(H, Scale=[4.0, 2.0], Depth=64.0, Position=[4.0, 8.0, 0.0], Wrap=False, Origin=[20.0, 16.0, 90.0], Radius=3.0, RampLength=40.0,
                   AmbientOcclusionRadius=5.0, AmbientOcclusionOpacity=0.5, Opacity=0.75, TextureRegion=[0.25, 0.0, 1.0, 0.5])
    got = np.frombuffer(H.LightingRenderer.PackProjectorLightBytes(l, 2.0, True, 128.0, [1.0, 1.0], -0.33), np.float32).reshape(8, 4)
    # Vertices.cs:22-30: LightPosition1..3, LightProperties, MoreLightProperties, EvenMoreLightProperties, Color1, Color2
    assert got[0].tolist() == [1 / 32, 0, 0, 0] and got[1].tolist() == [0, 1 / 16, 0, 0]
    assert got[2].tolist() == [20.0, 16.0, 90.0, 1.0]
    assert got[6].tolist() == [0, 0, 1 / 64, 0]
    assert got[7][:3].tolist() == [-0.125, -0.5, 0.0]
    # mip bias: max(0, log2(1 / ((4 + 2) / 2)) - 0.33) = 0
    assert got[7][3] == 0
    assert got[3].tolist() == [3.0, 40.0, 0.0, 1.0]
    assert got[4].tolist() == [5.0, 1.5, 1.0, 0.5]
    assert got[5].tolist() == [0.25, 0.0, 1.0, 0.5]
    # the same members through scenes.projector_light
    same = pc.projector_light(pc.forward_matrix((32.0, 16.0, 64.0), (4.0, 8.0, 0.0)), region=(0.25, 0.0, 1.0, 0.5), origin=(20.0, 16.0, 90.0), radius=3.0,
                              ramp_length=40.0, ao_radius=5.0, ao_opacity=0.5, opacity=0.75, intensity_scale=2.0)
    assert np.array_equal(np.frombuffer(bytes(same), np.float32).reshape(8, 4), got)
    # shadows need a field and an origin (:1432); Depth defaults to MaximumZ; a small scale has a positive mip bias
    assert np.frombuffer(H.LightingRenderer.PackProjectorLightBytes(l, 1.0, False), np.float32).reshape(8, 4)[3][3] == 0
    l.Origin = None
    packed = np.frombuffer(H.LightingRenderer.PackProjectorLightBytes(l, 1.0, True), np.float32).reshape(8, 4)
    assert packed[3][3] == 0 and packed[2].tolist() == [0, 0, 0, 0]
    l.Depth = None
    l.Scale = [0.25, 0.25]
    packed = np.frombuffer(H.LightingRenderer.PackProjectorLightBytes(l, 1.0, True, 32.0), np.float32).reshape(8, 4)
    assert packed[6][2] == 1 / 32
    assert packed[7][3] == F(np.log(4.0) / np.log(2.0) + F(-0.33))
    l.Wrap = True
    assert np.frombuffer(H.LightingRenderer.PackProjectorLightBytes(l), np.float32).reshape(8, 4)[4][2] == 0


def test_pack_projector_light_with_a_rotation_inverts_the_forward_matrix():
    """with a rotation (30 degrees about z) in Transform and one as the Rotation quaternion: forward x packed inverse is the identity
    within 1e-5 -- the forward matrix restated in float64, the quaternion's part of the inverse undone by its own inverse"""
    from illuminant_amd import _host as H
    a = np.pi / 6
    c, s = np.cos(a), np.sin(a)
    transform = np.array([[c, s, 0, 0], [-s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    l = host_light(H, size=(5, 3), Transform=[float(v) for v in transform.reshape(-1)], Scale=[6.0, 7.0], Depth=48.0, Position=[9.0, 4.0, 2.0])
    got = np.frombuffer(H.LightingRenderer.PackProjectorLightBytes(l), np.float32).reshape(8, 4)
    inverse = np.array([got[0], got[1], got[6], got[7]], np.float64)
    inverse[3, 3] = 1.0
    forward = transform.astype(np.float64) @ np.diag([5 * 6.0, 3 * 7.0, 48.0, 1.0])
    forward[3, :3] += (9.0, 4.0, 2.0)
    assert np.allclose(forward @ inverse, np.eye(4), rtol=0, atol=1e-5)
    # the Rotation quaternion turns texture space about the centre of the region
    q = [0.0, 0.0, float(np.sin(a / 2)), float(np.cos(a / 2))]
    l.Rotation = q
    l.TextureRegion = [0.0, 0.0, 1.0, 0.5]
    got = np.frombuffer(H.LightingRenderer.PackProjectorLightBytes(l), np.float32).reshape(8, 4)
    rotated = np.array([got[0], got[1], got[6], got[7]], np.float64)
    rotated[3, 3] = 1.0
    spin = np.array([[c, s, 0, 0], [-s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)       # CreateFromQuaternion of q
    centre = np.eye(4)
    centre[3, :2] = (0.5, 0.25)
    back = np.eye(4)
    back[3, :2] = (-0.5, -0.25)
    assert np.allclose(rotated, inverse @ back @ spin @ centre, rtol=0, atol=1e-5)
    assert np.allclose(forward @ rotated @ np.linalg.inv(back @ spin @ centre), np.eye(4), rtol=0, atol=1e-5)
