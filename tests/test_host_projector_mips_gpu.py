"""RenderLighting of the host mirror with a projector whose texture has a mip chain: a light drawn at half size packs the bias 0.67
(log2(1 / 0.5) - 0.33) and its three-level RampTexture is bound with the levels -- the frame equals, bit for bit, the same calls made
through the C ABI and the restatement of tests/projector_mip_common.py; with a one-level texture the mirror makes the call it always
made and the frame is the one-level pass's."""
import numpy as np
import pytest

from illuminant_amd import abi, native
from tests import projector_common as pc
from tests import projector_mip_common as pmc
from tests.test_host_projector_gpu import AMBIENT, H, W, host_renderer, projector, vertices
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Host():
    from illuminant_amd import _host
    return _host


@pytest.fixture(scope="module")
def hctx(Host):
    return Host.DeviceContext(0)


def frame(Host, hctx, texture):
    """a wrapping projector at Scale 0.5 (no origin: nothing traces, the arithmetic is exact) alone in the environment"""
    env = Host.LightingEnvironment()
    env.Ambient = list(AMBIENT)
    light = projector(Host, texture, Scale=[0.5, 0.5], Position=[1.25, 0.75, 0.0], Opacity=0.8)
    env.ProjectorLights = [light]
    r, field = host_renderer(Host, hctx, env)
    stats = r.RenderLighting(1.0, 0, -1, True)
    got = r.ReadLightmap()
    r.RenderLighting(1.0, 0, -1, False)
    assert_bits_equal(r.ReadLightmap(), got, "the frame without statistics against the counting frame")
    packed = np.frombuffer(r.GetPackedLightVertices(), np.float32).reshape(-1, 8, 4)
    assert packed.shape[0] == 1 and packed[0][7][3] == np.float32(np.log(2.0) / np.log(2.0) + np.float32(-0.33))
    dfu = abi.DistanceFieldUniforms.from_buffer_copy(r.GetDistanceFieldUniformsBytes())
    envu = abi.Environment.from_buffer_copy(r.GetEnvironmentUniformsBytes())
    return got, [int(x) for x in stats], vertices([packed[0]]), envu, dfu


def direct(ctx, texture, lights, envu, dfu):
    lm = native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4)
    native.set_projector_texture(ctx, texture)
    st = native.render_projector_lights(ctx, lights, envu, dfu, None, None, AMBIENT, lm, want_stats=True)
    native.set_projector_texture(ctx, None)
    out = lm.download()
    lm.close()
    return out, [int(st.SdfSamples), int(st.PixelLightPairs), int(st.TracedPairs)]


def test_a_half_size_projector_reads_its_three_level_chain(Host, hctx, ctx, oracle):
    chain = pmc.chain(8, 8, 3)
    texture = Host.RampTexture(chain[0], list(chain[1:]))
    assert texture.LevelCount == 3
    got, stats, lights, envu, dfu = frame(Host, hctx, texture)
    want, want_stats = direct(ctx, chain, lights, envu, dfu)
    assert_bits_equal(got, want, "RenderLighting against the direct calls")
    assert stats == want_stats == [0, W * H, 0]
    restated = pmc.render(oracle, list(lights), chain, envu, dfu, None, None, AMBIENT, W, H)
    assert_bits_equal(got, restated.image, "RenderLighting against the restatement: levels 0 and 1 at weight 0.67")
    assert list(restated.stats) == stats
    # ... which is neither level alone
    for level in (0, 1):
        alone = pmc.render(oracle, list(lights), [chain[level]], envu, dfu, None, None, AMBIENT, W, H)
        assert (alone.image != got).mean() > 0.5


def test_the_same_light_with_a_one_level_texture_makes_the_old_call(Host, hctx, ctx, oracle):
    chain = pmc.chain(8, 8, 3)
    got, stats, lights, envu, dfu = frame(Host, hctx, Host.RampTexture(chain[0]))
    want, want_stats = direct(ctx, chain[0], lights, envu, dfu)
    assert_bits_equal(got, want, "RenderLighting against the one-level call")
    assert stats == want_stats
    assert_bits_equal(got, pc.render(oracle, list(lights), chain[0], envu, dfu, None, None, AMBIENT, W, H).image, "one level: the bias is not read")
