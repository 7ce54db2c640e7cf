"""Known answers for the projector pass's fetch over a mip chain (ilm_ctx_set_projector_texture_mips), derived by hand, against the
float32 restatement of tests/projector_mip_common.py; the shape checks of the Python layer and of the host mirror's RampTexture.  No
GPU: the entry point is looked up in the built library, nothing is launched."""
import os
import re

import numpy as np
import pytest

from illuminant_amd import native, scenes
from tests import projector_common as pc
from tests import projector_mip_common as pmc

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def constant_chain(width, height, levels):
    """level l is the constant l in all four components"""
    return [np.full((h, w, 4), l, np.float32) for l, (w, h) in enumerate(pmc.level_sizes(width, height, levels))]


def test_header_binding_and_csharp_agree_on_the_new_symbol():
    text = open(os.path.join(ROOT, "include", "illuminant_hip.h")).read()
    decl = re.search(r"^int32_t ilm_ctx_set_projector_texture_mips\(([^)]*)\)", text, flags=re.M).group(1)
    assert [p.strip().rsplit(" ", 1) for p in decl.split(",")] == [["IlmHandle", "ctx"], ["const IlmFloat4*", "texels"], ["int32_t", "width"],
                                                                  ["int32_t", "height"], ["int32_t", "levels"]]
    result, args = native.SYMBOLS["ilm_ctx_set_projector_texture"]
    assert native.SYMBOLS["ilm_ctx_set_projector_texture_mips"] == (result, args + [args[-1]])          # ... and one more int32: levels
    assert hasattr(native.lib(), "ilm_ctx_set_projector_texture_mips")
    cs = open(os.path.join(ROOT, "integration", "IlluminantHip.cs")).read()
    assert "ilm_ctx_set_projector_texture_mips (ulong ctx, Vector4* texels, int width, int height, int levels)" in cs
    assert "#define ILM_ABI_VERSION 11" in text and "+ ilm_ctx_set_projector_texture_mips" in text[:text.index("#define ILM_ABI_VERSION")]
    # the fetch is specified where the pass is: the LOD's clamp, the untouched level at weight 0 and the deviation
    contract = text[text.index("/* The projector-light pass"):text.index("int32_t ilm_render_projector_lights")]
    for word in ("fminf(fmaxf(lod, 0), L - 1)", "l1 = min(l0 + 1, L - 1)", "NOT read", "c0 + (c1 - c0) * f", "fixed-point",
                 "ilm_ctx_set_projector_texture_mips"):
        assert word in contract, word
    assert "the bias is carried and not read" not in text


def test_a_chain_of_constant_levels_gives_the_lod_itself():
    chain = constant_chain(8, 8, 4)
    for u, v in ((0.3, 0.7), (0.0, 0.0), (-2.25, 9.5)):
        assert [float(c) for c in pmc.fetch_lod(chain, u, v, 1.25)] == [1.25] * 4          # 1 + (2 - 1) * 0.25
        assert [float(c) for c in pmc.fetch_lod(chain, u, v, 0.5)] == [0.5] * 4
        assert [float(c) for c in pmc.fetch_lod(chain, u, v, 2.0)] == [2.0] * 4
    # the mirror's bias for a light at half size: log2(1 / 0.5) - 0.33, the weight's bits included
    lod = F(np.log(2.0) / np.log(2.0) + F(-0.33))
    assert pmc.resolve_lod(lod, 4) == (0, 1, F(lod - F(0)))
    assert [c for c in pmc.fetch_lod(chain, 0.4, 0.6, lod)] == [pc.lerp(0, 1, lod)] * 4


def test_at_weight_zero_the_other_level_is_not_touched():
    """an integral LOD reads one level: with every other level NaN the texel is finite and equals the one-level fetch"""
    chain = list(pmc.chain(8, 8, 4))
    for l in range(4):
        poisoned = [t if k == l else np.full_like(t, np.nan) for k, t in enumerate(chain)]
        for u, v in ((0.3, 0.7), (0.99, -0.01)):
            got = pmc.fetch_lod(poisoned, u, v, float(l))
            assert np.isfinite(got).all() and got == pc.fetch(chain[l], u, v)
    # ... and between two levels exactly those two are read
    poisoned = [chain[0], chain[1], np.full_like(chain[2], np.nan), np.full_like(chain[3], np.nan)]
    assert np.isfinite(pmc.fetch_lod(poisoned, 0.3, 0.7, 0.5)).all()
    assert np.isnan(pmc.fetch_lod(poisoned, 0.3, 0.7, 1.5)).all()


def test_lods_outside_the_chain_clamp():
    L = 4
    assert pmc.resolve_lod(-1.0, L) == (0, 1, 0)
    assert pmc.resolve_lod(float("nan"), L) == (0, 1, 0)                # fmaxf(NaN, 0) = 0
    assert pmc.resolve_lod(float("inf"), L) == (L - 1, L - 1, 0)
    assert pmc.resolve_lod(float("-inf"), L) == (0, 1, 0)
    assert pmc.resolve_lod(L - 1, L) == (L - 1, L - 1, 0)
    assert pmc.resolve_lod(L + 3, L) == (L - 1, L - 1, 0)
    assert pmc.resolve_lod(2.75, L) == (2, 3, 0.75)
    assert pmc.resolve_lod(0.67, 1) == (0, 0, 0)                        # one level: every LOD is level 0, weight 0
    chain = constant_chain(8, 8, L)
    for lod, want in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 3.0), (L - 1, 3.0), (L + 3, 3.0)):
        assert [float(c) for c in pmc.fetch_lod(chain, 0.3, 0.7, lod)] == [want] * 4
    # a one-level chain is the one-level fetch at every LOD
    t = pc.texture(5, 3)
    for lod in (0.0, 0.67, 5.0, float("nan")):
        assert pmc.fetch_lod([t], 0.3, 0.7, lod) == pc.fetch(t, 0.3, 0.7)


def test_level_sizes_of_a_5_by_3_texture():
    assert pmc.level_sizes(5, 3, 4) == [(5, 3), (2, 1), (1, 1), (1, 1)]
    assert [t.shape for t in pmc.chain(5, 3, 4)] == [(3, 5, 4), (1, 2, 4), (1, 1, 4), (1, 1, 4)]
    assert [t.shape for t in scenes.projector_mip_chain(pc.texture(5, 3))] == [(3, 5, 4), (1, 2, 4), (1, 1, 4)]
    assert pmc.level_sizes(7, 16, 5) == [(7, 16), (3, 8), (1, 4), (1, 2), (1, 1)]
    # each level is fetched with its own size: at level 1 of the 5 x 3 chain (2 x 1) u = 0.25 is the centre of texel 0
    chain = pmc.chain(5, 3, 4)
    assert pmc.fetch_lod(chain, 0.25, 0.5, 1.0) == [c for c in chain[1][0, 0]]
    assert pmc.fetch_lod(chain, 1e9, -3e5, 3.0) == [c for c in chain[3][0, 0]]          # a 1 x 1 level: one texel, whatever the coordinate


class FakeContext:
    handle = 0


def test_the_shape_checks_of_set_projector_texture():
    """refused in Python, before the library is asked; what passes reaches the library, which refuses handle 0 (no context) by name"""
    good = list(pmc.chain(5, 3, 4))
    for bad in ([good[0], good[0]], [good[0], good[1], good[1]], [good[0], np.zeros((1, 2, 3), np.float32)], [good[0][0]], []):
        with pytest.raises(ValueError):
            native.set_projector_texture(FakeContext, bad)
    with pytest.raises(ValueError, match="mip level 1"):
        native.set_projector_texture(FakeContext, good[0], mips=[good[2]])
    with pytest.raises(ValueError):
        native.set_projector_texture(FakeContext, np.zeros((3, 5), np.float32))
    # a well-formed chain reaches the library, which refuses the handle
    for args, kw in (((good,), {}), ((tuple(good),), {}), ((good[0],), dict(mips=good[1:])), ((good[0],), {})):
        with pytest.raises(native.IlluminantError, match="context handle"):
            native.set_projector_texture(FakeContext, *args, **kw)


def test_the_host_mirror_s_ramp_texture_takes_and_checks_the_levels():
    from illuminant_amd import _host as H
    chain = pmc.chain(5, 3, 4)
    one = H.RampTexture(chain[0])
    assert (one.Width, one.Height, one.LevelCount) == (5, 3, 1)
    assert H.RampTexture(chain[0], None).LevelCount == 1 and H.RampTexture(chain[0], []).LevelCount == 1
    full = H.RampTexture(chain[0], list(chain[1:]))
    assert (full.Width, full.Height, full.LevelCount) == (5, 3, 4)
    assert H.RampTexture(chain[0], mips=[chain[1]]).LevelCount == 2
    for bad in ([chain[0]], [chain[1], chain[1]], [np.zeros((1, 2, 3), np.float32)], [chain[1][0]]):
        with pytest.raises(ValueError):
            H.RampTexture(chain[0], bad)
    with pytest.raises(ValueError):
        H.RampTexture(np.ones((1, 1, 4), np.float32), [np.ones((1, 1, 4), np.float32)] * 16)        # 17 levels
    # the packing does not depend on the levels: the bias is packed as before
    a, b = H.ProjectorLightSource(), H.ProjectorLightSource()
    a.TextureRef, b.TextureRef = one, full
    a.Scale = b.Scale = [0.5, 0.5]
    pa, pb = (np.frombuffer(H.LightingRenderer.PackProjectorLightBytes(l), np.float32).reshape(8, 4) for l in (a, b))
    assert np.array_equal(pa, pb) and pa[7][3] == F(np.log(2.0) / np.log(2.0) + F(-0.33))
