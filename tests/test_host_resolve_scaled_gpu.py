"""The host mirror's ResolveTo / ResolveAt (RenderedLighting.Resolve's two overloads over ResolveLighting, LightingRenderer.HDR.cs:99-151,
LightingRenderer.cs:1537-1645): a frame lit at RenderScale (0.5, 0.5) reaches a target of another size with the bits of
ilm_resolve_lighting_scaled called with the quad, regions and offset ResolveLighting's formulas give (worked out here in float32)."""
import numpy as np
import pytest

from illuminant_amd import abi, native
from tests import output_common as oc
from tests import resolve_scaled_common as rs

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 80, 56
SCALE = (0.5, 0.5)


@pytest.fixture(scope="module")
def Host():
    from illuminant_amd import _host
    return _host


@pytest.fixture(scope="module")
def scene(Host):
    """A renderer at RenderScale 0.5 with a few sphere lights, its frame rendered, and a native view of its context and lightmap."""
    hctx = Host.DeviceContext(0)
    env = Host.LightingEnvironment()
    env.Ambient = [0.11, 0.09, 0.13, 0.6]
    lights = []
    for k, (position, color) in enumerate((((14.0, 12.0, 6.0), (1.0, 0.8, 0.6, 0.9)), ((41.0, 30.0, 7.0), (0.5, 0.9, 0.7, 1.0)),
                                           ((66.0, 44.0, 8.0), (0.3, 0.5, 1.0, 0.8)))):
        l = Host.SphereLightSource()
        l.Position, l.Color = list(position), list(color)
        l.Radius, l.RampLength, l.SortKey = 3.0, 22.0, k
        lights.append(l)
    env.Lights = lights
    rc = Host.RendererConfiguration(W, H)
    rc.RenderScale = list(SCALE)
    r = Host.LightingRenderer(hctx, rc, env)
    r.RenderLighting(1.0, 0, -1, False)
    own = native.Context(0, borrowed_handle=hctx.Handle)
    lightmap = native.Lightmap(own, W, H, r.LightmapFormat, borrowed_handle=r.LightmapHandle)
    lit = lightmap.download().astype(np.float32)
    assert np.ptp(lit[..., 0]) > 0.1, "the frame is lit"
    yield Host, r, own, lightmap
    del r


def _target(own, size, fmt=abi.LIGHTMAP_RGBA8):
    t = native.Lightmap(own, size[0], size[1], fmt)
    t.upload(np.full((size[1], size[0], 4), oc.SENTINEL[fmt]))
    return t


def test_resolve_to_stretches_the_lightmap_by_scale_over_render_scale(scene):
    """Resolve(width, height) without albedo: scale = (width / 80, height / 56), the quad is the lightmap's 80 x 56 texels x
    scale / RenderScale.  ResolveTo(80, 56) -- the lightmap's own size -- therefore fills a 160 x 112 back buffer at RenderScale 0.5, and
    ResolveTo(160, 112) asks for a 320 x 224 quad, of which the target shows the top left quarter."""
    Host, r, own, lightmap = scene
    hdr = oc.matrix_hdr(abi.HDR_TONE_MAP)
    size = (160, 112)
    for width, height in ((160.0, 112.0), (80.0, 56.0)):
        quad = (0.0, 0.0, F(W) * ((F(width) / F(W)) / F(SCALE[0])), F(H) * ((F(height) / F(H)) / F(SCALE[1])))
        assert quad[2:] == {160.0: (320.0, 224.0), 80.0: (160.0, 112.0)}[width]
        got, want = _target(own, size), _target(own, size)
        r.ResolveTo((got.handle.value, size[0], size[1]), width, height, hdr=bytes(hdr))
        native.resolve_lighting_scaled(lightmap, want, hdr, quad)
        g = got.download()
        assert g.tobytes() == want.download().tobytes(), (width, height)
        assert (g[..., 3] == 255).all()                                  # every pixel of the target was written: alpha 1
        got.close(); want.close()


def test_resolve_to_defaults_to_the_plain_resolve_and_honours_rows_and_the_sampler(scene):
    Host, r, own, lightmap = scene
    size = (160, 112)
    got, want = _target(own, size, abi.LIGHTMAP_FLOAT4), _target(own, size, abi.LIGHTMAP_FLOAT4)
    r.ResolveTo((got.handle.value, size[0], size[1]), 80.0, 56.0, lightmapSamplerState=abi.FILTER_POINT, rowBegin=7, rowEnd=90)
    native.resolve_lighting_scaled(lightmap, want, oc.hdr_configuration(), (0.0, 0.0, 160.0, 112.0), lightmap_filter=rs.POINT, row_begin=7, row_end=90)
    g = got.download()
    assert g.tobytes() == want.download().tobytes()
    assert (g[:7] == oc.SENTINEL[abi.LIGHTMAP_FLOAT4]).all() and (g[90:] == oc.SENTINEL[abi.LIGHTMAP_FLOAT4]).all() and (g[7:90, :, 3] == 1.0).all()
    got.close(); want.close()


def test_resolve_at_places_the_albedo_region_at_a_position(scene):
    """Resolve(position, scale) with an albedo: the quad is the albedo region's texel size x scale at `position`; the albedo region and
    the uv offset are given in UV and reach the library in texels."""
    Host, r, own, lightmap = scene
    hdr = oc.matrix_hdr(abi.HDR_GAMMA_COMPRESS)
    aw, ah = 96, 64
    texels = np.random.default_rng(81).integers(0, 256, (ah, aw, 4), dtype=np.uint8)
    albedo = native.Lightmap(own, aw, ah, abi.LIGHTMAP_RGBA8)
    albedo.upload(texels)
    size = (150, 101)
    position, scale, region_uv, uv_offset = (9.5, -6.25), (1.5, 1.25), (0.125, 0.25, 0.875, 1.0), (0.0125, -0.03125)
    region = (F(region_uv[0]) * F(aw), F(region_uv[1]) * F(ah), F(region_uv[2]) * F(aw), F(region_uv[3]) * F(ah))
    quad = (position[0], position[1], (region[2] - region[0]) * F(scale[0]), (region[3] - region[1]) * F(scale[1]))
    assert region == (12.0, 16.0, 84.0, 64.0) and quad[2:] == (108.0, 60.0)
    offset = (F(uv_offset[0]) * F(W), F(uv_offset[1]) * F(H))
    got, want = _target(own, size), _target(own, size)
    r.ResolveAt((got.handle.value, size[0], size[1]), list(position), list(scale), albedo=(albedo.handle.value, aw, ah),
                albedoTextureRegion=list(region_uv), albedoSamplerState=abi.FILTER_POINT, uvOffset=list(uv_offset), hdr=bytes(hdr))
    native.resolve_lighting_scaled(lightmap, want, hdr, quad, albedo=albedo, albedo_region=region, uv_offset=offset, albedo_filter=rs.POINT)
    g = got.download()
    assert g.tobytes() == want.download().tobytes()
    covered = rs.coverage(size, quad)
    assert 0 < covered.sum() < covered.size
    assert np.array_equal((g != oc.SENTINEL[abi.LIGHTMAP_RGBA8]).any(axis=-1), covered)
    # ResolveTo with an albedo: rw x rh is the albedo's size and Configuration.RenderScale plays no part
    got.upload(np.full((size[1], size[0], 4), oc.SENTINEL[abi.LIGHTMAP_RGBA8])); want.upload(np.full((size[1], size[0], 4), oc.SENTINEL[abi.LIGHTMAP_RGBA8]))
    r.ResolveTo((got.handle.value, size[0], size[1]), 144.0, 80.0, albedo=(albedo.handle.value, aw, ah), hdr=bytes(hdr))
    native.resolve_lighting_scaled(lightmap, want, hdr, (0.0, 0.0, F(aw) * (F(144.0) / F(aw)), F(ah) * (F(80.0) / F(ah))), albedo=albedo)
    assert got.download().tobytes() == want.download().tobytes()
    for t in (got, want, albedo):
        t.close()
