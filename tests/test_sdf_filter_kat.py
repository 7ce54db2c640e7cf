"""The distance field's bilinear filter (ilm_sdf_set_filter) without a GPU: the restatements of tests/sdf_filter_common.py are anchored
to the oracle at 0 fraction bits (the sampler bit for bit, the sphere pass with exact statistics and alpha), the quantiser is held
to known answers on an atlas whose coordinates are exact, the scene of the GPU tests is held to the conditions that make those tests
mean something, and the bindings carry the two entry points."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from illuminant_amd import abi, native
from tests import directional_common as dc
from tests import sdf_filter_common as sf
from tests.sdf_filter_common import F
from tests.util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits_of(a):
    return np.asarray(a, np.float32).view(np.uint32)


def oracle_samples(oracle, positions, dfu, texture):
    return np.array([oracle.sample_distance_field(p, dfu, texture) for p in positions], np.float32)


# ---- 1. sampler anchor -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", sf.FORMATS)
@pytest.mark.parametrize("field", ["directional_common", "multi_row"])
def test_the_sampler_port_at_0_bits_is_the_oracle_bit_for_bit(oracle, fmt, field):
    if field == "multi_row":
        atlas, dfu, layout = sf.multi_row_field(fmt)
        assert layout.row_count > 1 and layout.column_count > 1 and layout.slice_count == 33
    else:
        atlas, dfu = dc.field_atlas(fmt), sf.field_uniforms()
        assert atlas.shape == (64, 96, 4)            # 12 slices of 48 x 32 texels, 2 x 2
    pts = sf.probe_positions(dfu)
    e = np.array([dfu.Extent.x, dfu.Extent.y, dfu.Extent.z], np.float32)
    assert len(pts) >= 2000
    finite = np.isfinite(pts).all(axis=1)
    inside = finite & (pts >= 0).all(axis=1) & (pts <= e).all(axis=1)
    assert inside.sum() >= 1500
    for axis in range(3):
        assert (finite & (pts[:, axis] < 0)).sum() >= 50 and (finite & (pts[:, axis] > e[axis])).sum() >= 50
        assert np.isnan(pts[:, axis]).any() and (pts[:, axis] == np.inf).any() and (pts[:, axis] == -np.inf).any()
    got = sf.Sampler(atlas, fmt, dfu, 0).many(pts)
    want = oracle_samples(oracle, pts, dfu, oracle.make_texture(atlas, fmt))
    differ = bits_of(got) != bits_of(want)
    assert not differ.any(), "%d of %d samples differ, first at %s" % (int(differ.sum()), len(pts), pts[np.argmax(differ)])
    if field == "multi_row":      # every atlas row was visited: the wrap carried slices onto each of them
        rows = (np.floor(pts[inside, 2] * F(dfu.Packed1.y)).astype(int) // 3) // layout.column_count
        assert np.unique(rows).size == layout.row_count


# ---- 2. quantiser known answers --------------------------------------------------------------------------------------------------

kat_field, position, Z_VALUES = sf.kat_field, sf.position, sf.Z_VALUES


@pytest.mark.parametrize("fmt", sf.FORMATS)
@pytest.mark.parametrize("axis", [0, 1])
def test_fractions_of_k_256_keep_the_0_bit_result(fmt, axis):
    atlas, dfu = kat_field(fmt)
    s0, s8 = sf.Sampler(atlas, fmt, dfu, 0), sf.Sampler(atlas, fmt, dfu, 8)
    for k in (0, 1, 2, 3, 127, 128, 129, 254, 255):
        for z in Z_VALUES:
            p = position(axis, F(5.5) + F(k) / F(256), F(9.5) + F(77) / F(256), z)
            a, b = s0(p), s8(p)
            assert bits_of(a) == bits_of(b), (k, z)
            assert s8.facts["fx" if axis == 0 else "fy"] == F(k) / F(256) and s8.facts["fz"] == s0.facts["fz"]


def hand_value(atlas, fmt, dfu, x0, y0, wx, wy, z):
    """the sample whose taps are (x0, y0) .. (x0 + 1, y0 + 1) with the WEIGHTS wx, wy given: the lerps and the decode, nothing else"""
    t = sf.decode_atlas(atlas, fmt)
    sp = F(F(z) * F(dfu.Packed1.y))
    v = int(np.floor(sp))
    lerp = lambda a, b, w: sf.fmaf(w, F(b - a), a)
    packed = [lerp(lerp(t[y0, x0, c], t[y0, x0 + 1, c], wx), lerp(t[y0 + 1, x0, c], t[y0 + 1, x0 + 1, c], wx), wy) for c in (v, v + 1)]
    return sf.fmaf(F(sf.DISTANCE_ZERO - lerp(packed[0], packed[1], F(sp - F(v)))), F(dfu.Extent.w), F(0))


@pytest.mark.parametrize("fmt", sf.FORMATS)
@pytest.mark.parametrize("axis", [0, 1])
def test_ties_round_to_even_and_their_neighbours_round_to_nearest(fmt, axis):
    atlas, dfu = kat_field(fmt)
    s8 = sf.Sampler(atlas, fmt, dfu, 8)
    name = "fx" if axis == 0 else "fy"
    base, other_w = F(5.5), F(77) / F(256)
    ulp = np.spacing(base)                                 # of the COORDINATE: 2^-21, far below 1 / 512
    cases = [(F(0.5) / F(256), F(0)), (F(1.5) / F(256), F(2) / F(256)), (F(2.5) / F(256), F(2) / F(256)), (F(254.5) / F(256), F(254) / F(256)),
             (F(0.5) / F(256) - ulp, F(0)), (F(0.5) / F(256) + ulp, F(1) / F(256)),
             (F(1.5) / F(256) - ulp, F(1) / F(256)), (F(1.5) / F(256) + ulp, F(2) / F(256)),
             (F(0), F(0)), (ulp, F(0)), (F(100.25) / F(256), F(100) / F(256)), (F(100.75) / F(256), F(101) / F(256))]
    for f, weight in cases:
        coordinate = F(base + f)
        assert F(coordinate - base) == f                   # the position carries the fraction exactly
        for z in Z_VALUES[:3]:
            got = s8(position(axis, coordinate, F(9.5) + other_w, z))
            assert s8.facts[name] == weight, (f, s8.facts[name], weight)
            assert s8.facts["taps"] == ((5, 6, 9, 10) if axis == 0 else (9, 10, 5, 6))
            wx, wy = (weight, other_w) if axis == 0 else (other_w, weight)
            x0, y0 = (5, 9) if axis == 0 else (9, 5)
            assert bits_of(got) == bits_of(hand_value(atlas, fmt, dfu, x0, y0, wx, wy, z)), (f, z)


@pytest.mark.parametrize("fmt", sf.FORMATS)
@pytest.mark.parametrize("axis", [0, 1])
def test_a_fraction_of_255_5_256_or_more_is_the_weight_one_on_the_same_taps(fmt, axis):
    atlas, dfu = kat_field(fmt)
    s0, s8 = sf.Sampler(atlas, fmt, dfu, 0), sf.Sampler(atlas, fmt, dfu, 8)
    name = "fx" if axis == 0 else "fy"
    base = F(5.5)
    ulp = np.spacing(F(6.0) - np.spacing(F(5.5)))
    for f in (F(255.5) / F(256), F(255.75) / F(256), F(1) - ulp):
        coordinate = F(base + f)
        assert F(coordinate - base) == f and coordinate < F(6.5)
        for z in Z_VALUES[:3]:
            p = position(axis, coordinate, F(9.5) + F(0.3125), z)
            got = s8(p)
            s0(p)
            assert s8.facts[name] == F(1) and s8.facts["taps"] == s0.facts["taps"]          # no carry into the next texel
            assert s8.facts["taps"] == ((5, 6, 9, 10) if axis == 0 else (9, 10, 5, 6))
            wx, wy = (F(1), F(0.3125)) if axis == 0 else (F(0.3125), F(1))
            x0, y0 = (5, 9) if axis == 0 else (9, 5)
            assert bits_of(got) == bits_of(hand_value(atlas, fmt, dfu, x0, y0, wx, wy, z))
    # just below: 255.5 / 256 less one ulp of the coordinate rounds down to 255 / 256
    s8(position(axis, F(base + F(255.5) / F(256)) - np.spacing(base), F(9.5), 1.0))
    assert s8.facts[name] == F(255) / F(256)


def test_the_quantiser_is_rint_times_2_to_the_minus_8():
    f = np.random.default_rng(3).random(4096, np.float32)
    got = np.array([sf.quantise(F(v), 8) for v in f], np.float32)
    assert np.array_equal(got, (np.rint(f * F(256)) / F(256)).astype(np.float32))
    assert np.array_equal(got * F(256), np.rint(got * F(256))) and got.max() <= 1.0
    assert all(sf.quantise(F(v), 0) == F(v) for v in f[:64])


# ---- 3. sphere anchor + 4. conditions on the scene -----------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", sf.FORMATS)
@pytest.mark.parametrize("with_gbuffer", [False, True])
def test_the_sphere_port_with_the_0_bit_sampler_is_the_oracles_render(oracle, fmt, with_gbuffer):
    ref = sf.reference(fmt, with_gbuffer, 0)
    texture = oracle.make_texture(ref.atlas, fmt)
    gbuffer = oracle.make_texture(ref.gbuffer, abi.GBUFFER_FLOAT4) if with_gbuffer else None
    for light_set in sf.LIGHT_SETS:
        image, stats = ref.frame(light_set)
        lights = dc.light_array([ref.lights[i] for i in light_set])
        want, ws = oracle.render_sphere_lights(lights, ref.env, ref.dfu, gbuffer, texture, sf.AMBIENT, sf.WIDTH, sf.HEIGHT, want_stats=True)
        assert stats == (ws.SdfSamples, ws.PixelLightPairs, ws.TracedPairs), (light_set, stats)
        assert np.array_equal(image[..., 3], want[..., 3]), light_set
        assert_close(image[..., :3], want[..., :3], "lightmap rgb of lights %s" % (light_set,))


@pytest.mark.parametrize("fmt", sf.FORMATS)
@pytest.mark.parametrize("with_gbuffer", [False, True])
def test_the_scene_reaches_what_the_gpu_tests_are_about(fmt, with_gbuffer):
    """If one of these fails, change the lights, not the condition."""
    r0, r8 = sf.reference(fmt, with_gbuffer, 0), sf.reference(fmt, with_gbuffer, 8)
    e = np.array([r0.dfu.Extent.x, r0.dfu.Extent.y, r0.dfu.Extent.z], np.float32)
    inside = ((r8.visited >= 0) & (r8.visited <= e)).all(axis=1)
    assert inside.sum() >= 1000 and (~inside).sum() >= 100              # samples inside the volume and outside it
    assert (r8.visited[:, 0] > e[0]).sum() >= 100                        # light 2's traces leave through the x face
    assert r8.per_light[0].ao_samples > 0 and r8.per_light[0].traced > 0
    assert r8.per_light[1].ao_samples == 0 and r8.per_light[1].traced > 0
    assert r8.per_light[2].ao_samples > 0 and r8.per_light[2].traced == 0 and r8.per_light[2].samples == r8.per_light[2].ao_samples
    # a kernel that ignores the filter must fail the GPU test: every frame of the GPU test moves beyond the suite's criterion
    for light_set in sf.LIGHT_SETS:
        moved = sf.beyond_criterion(r8.frame(light_set)[0], r0.frame(light_set)[0])
        assert moved.sum() >= 20, (light_set, int(moved.sum()))


# ---- 5. bindings ---------------------------------------------------------------------------------------------------------------

def test_the_bindings_carry_the_two_entry_points():
    text = open(os.path.join(ROOT, "include", "illuminant_hip.h")).read()
    decl = {name: re.search(r"^int32_t %s\(([^)]*)\);" % name, text, flags=re.M).group(1) for name in ("ilm_sdf_set_filter", "ilm_sdf_get_filter")}
    assert [p.strip() for p in decl["ilm_sdf_set_filter"].split(",")] == ["IlmHandle sdf", "int32_t fraction_bits"]
    assert [p.strip() for p in decl["ilm_sdf_get_filter"].split(",")] == ["IlmHandle sdf", "int32_t* out_fraction_bits"]
    assert re.search(r"^#define ILM_SDF_FILTER_FP32\s+0\b", text, flags=re.M) and re.search(r"^#define ILM_SDF_FILTER_FIXED8\s+8\b", text, flags=re.M)
    assert (abi.SDF_FILTER_FP32, abi.SDF_FILTER_FIXED8) == (0, 8)
    import ctypes as C
    assert native.SYMBOLS["ilm_sdf_set_filter"] == (C.c_int32, [abi.Handle, C.c_int32])
    result, args = native.SYMBOLS["ilm_sdf_get_filter"]
    assert result is C.c_int32 and args[0] is abi.Handle and args[1]._type_ is C.c_int32 and len(args) == 2
    lib = native.lib()
    assert hasattr(lib, "ilm_sdf_set_filter") and hasattr(lib, "ilm_sdf_get_filter")
    # a bad handle is reported before the value is looked at
    assert lib.ilm_sdf_set_filter(abi.Handle(0), 5) == abi.ERR_INVALID_HANDLE
    assert lib.ilm_sdf_get_filter(abi.Handle(0), None) == abi.ERR_INVALID_HANDLE
    assert callable(native.DistanceFieldTexture.set_filter) and isinstance(native.DistanceFieldTexture.filter, property)
    cs = open(os.path.join(ROOT, "integration", "IlluminantHip.cs")).read()
    assert "ilm_sdf_set_filter (ulong sdf, int fractionBits)" in cs and "ilm_sdf_get_filter (ulong sdf, int* outFractionBits)" in cs
    assert "SDF_FILTER_FIXED8 = 8" in cs and "SDF_FILTER_FP32 = 0" in cs
    assert "#define ILM_ABI_VERSION 11" in text
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_csharp_binding.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr


def test_the_contract_states_the_model_the_deviation_and_what_is_not_built():
    text = open(os.path.join(ROOT, "include", "illuminant_hip.h")).read()
    contract = text[text.index("/* The field's bilinear filter"):text.index("int32_t ilm_sdf_set_filter")]
    for word in ("MODEL", "DEFINED DEVIATION", "rintf(fx * 256.0f) * (1.0f / 256.0f)", "half to even", "255.5 / 256", "NOT quantised", "Not built",
                 "not the reference's measured behaviour", "ilm_render_particle_lights", "ilm_render_light_probes", "ilm_group_render_sphere_lights",
                 "ilm_visualize_distance_field", "ilm_system_set_distance_field", "ilm_engine_step_batch", "ILM_ERR_INVALID_ARGUMENT",
                 "ILM_ERR_INVALID_HANDLE", "CellRebuilds", "one workgroup per tile"):
        assert word in contract, word
