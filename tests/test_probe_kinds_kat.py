"""The references of tests/probe_kinds_common.py on hand-evaluated pairs, the committed probe list held off the trace's knife edges, and
the two probe entry points without a device: exported, bound, and validating their handle first."""
import ctypes as C
import os

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import directional_common as dc
from tests import probe_kinds_common as pk

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ilm_render_directional_light_probes", "ilm_render_line_light_probes")


@pytest.fixture(scope="module")
def field(oracle):
    return oracle.make_texture(dc.field_atlas(abi.SDF_UNORM16), abi.SDF_UNORM16)


def one(position, normal=(0.0, 0.0, 1.0), w=1.0, shadows=1.0):
    return np.array([list(position) + [w]], np.float32), np.array([list(normal) + [shadows]], np.float32)


# ---- the ABI without a device ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ENTRIES)
def test_the_entry_point_is_exported_and_bound(name):
    assert name in native.SYMBOLS
    assert native.SYMBOLS[name] == native.SYMBOLS["ilm_render_light_probes"]
    assert hasattr(native.lib(), name)
    assert hasattr(native, name[len("ilm_"):])
    header = open(os.path.join(ROOT, "include", "illuminant_hip.h")).read()
    assert "int32_t %s(IlmHandle ctx, const IlmLightVertex* lights, int32_t light_count," % name in header
    assert name + " (ulong ctx, LightVertex* lights, int lightCount" in open(os.path.join(ROOT, "integration", "IlluminantHip.cs")).read()


@pytest.mark.parametrize("name", ENTRIES)
def test_the_handle_is_looked_up_first(name):
    lib = native.lib()
    entry = getattr(lib, name)
    env, dfu = scenes.environment(), dc.no_field_uniforms()
    out = np.full((1, 4), 7.0, np.float32)
    for handle in (0, 123456789):
        # every other argument is bad as well: the handle's refusal comes first
        assert entry(abi.Handle(handle), None, -1, None, None, -1, None, None, abi.Handle(5), None) == abi.ERR_INVALID_HANDLE
        assert b"context" in lib.ilm_last_error()
        assert entry(abi.Handle(handle), None, 0, None, None, 0, C.byref(env), C.byref(dfu), abi.Handle(0),
                     out.ctypes.data_as(C.c_void_p)) == abi.ERR_INVALID_HANDLE
    assert (out == 7.0).all()


# ---- the directional reference, pair by pair -------------------------------------------------------------------------------------------

def test_an_undirected_light_has_opacity_one_and_takes_no_samples(oracle, field):
    dfu = dc.field_uniforms()
    light = dc.directional_light(direction=None, color=(0.5, 0.25, 0.125, 0.5))      # Color2 = 0; CastsShadows = 1 all the same
    assert light.Color2.w == 0 and light.LightProperties.x == 1
    taken = []
    real = oracle.sample_distance_field
    try:
        oracle.sample_distance_field = lambda *a: taken.append(a) or real(*a)
        pp, pn = one((22.5, 12.0, 0.0), normal=(0.6, 0.0, -0.8))                    # a normal the factor would punish, next to the box
        pairs, facts = pk.directional_pairs(oracle, [light], pp, pn, dfu, field)
    finally:
        oracle.sample_distance_field = real
    assert not taken and "visibility" not in facts[(0, 0)] and facts[(0, 0)]["opacity"] == 1
    assert np.array_equal(pk.sum_pairs(pairs), [[0.25, 0.125, 0.0625, 1.0]])


def test_a_zero_normal_has_factor_one(oracle):
    light = dc.directional_light(direction=(0.0, 0.0, 1.0), color=(1.0, 0.5, 0.25, 1.0), casts_shadows=False)      # from below
    dfu = dc.no_field_uniforms()
    lit = pk.directional_probes(oracle, [light], *one((10.0, 10.0, 2.0), normal=(0.0, 0.0, 0.0)), dfu, None)
    assert np.array_equal(lit, [[1.0, 0.5, 0.25, 1.0]])
    # the same light on an upward normal: back-facing, opacity 0 -- and alpha 1 all the same (no opacity discard)
    dark = pk.directional_probes(oracle, [light], *one((10.0, 10.0, 2.0)), dfu, None)
    assert np.array_equal(dark, [[0.0, 0.0, 0.0, 1.0]])


def test_a_probe_behind_the_box_is_darker_than_one_in_the_open(oracle, field):
    """the field's box spans x 10..20, y 8..16, z 0..24; the light comes from -x (direction +x): a probe at x = 22.5 traces into the box's
    face, one at (4.5, 28.5) sees nothing within its trace (tests/test_directional_kat.py has the same two points as pixels)"""
    dfu = dc.field_uniforms()
    light = dc.directional_light(direction=(1.0, 0.0, -0.5), shadow_trace_length=24.0, shadow_softness=2.0)
    behind = pk.directional_probes(oracle, [light], *one((22.5, 12.5, 0.0)), dfu, field)
    open_ = pk.directional_probes(oracle, [light], *one((4.5, 28.5, 0.0)), dfu, field)
    assert behind[0, 3] == 1 and open_[0, 3] == 1
    assert behind[0, 0] == 0 and open_[0, 0] > 0.3
    # the trace starts at position + 1.5 normal and needs enableShadows: with normals.w = 0 the probe behind the box is lit like the other
    facts = pk.directional_pairs(oracle, [light], *one((22.5, 12.5, 0.0)), dfu, field)[1][(0, 0)]
    assert facts["start"] == [F(22.5), F(12.5), F(1.5)]
    unshadowed = pk.directional_probes(oracle, [light], *one((22.5, 12.5, 0.0), shadows=0.0), dfu, field)
    assert np.array_equal(unshadowed, open_)


def test_probes_with_no_opacity_and_invisible_probes_contribute_nothing(oracle):
    light = dc.directional_light(direction=None, color=(1, 1, 1, 1))
    dfu = dc.no_field_uniforms()
    for pp, pn in (one((10.0, 10.0, 2.0), w=0.0), one((10.0, 10.0, 2.0), w=-1.0), one((-10000.0, 10.0, 2.0)), one((-9999.0, 10.0, 2.0))):
        assert np.array_equal(pk.directional_probes(oracle, [light, light], pp, pn, dfu, None), [[0, 0, 0, 0]])
    assert np.array_equal(pk.directional_probes(oracle, [light, light], *one((-9998.5, 10.0, 2.0)), dfu, None), [[2, 2, 2, 2]])


def test_the_ramp_is_applied_before_the_probe_opacity(oracle):
    ramp = dc.ramp_texture()
    light = dc.directional_light(direction=(0.6, 0.0, 0.12), color=(1, 1, 1, 1), casts_shadows=False)       # a partial normal factor
    dfu = dc.no_field_uniforms()
    plain = pk.directional_probes(oracle, [light], *one((10.0, 10.0, 2.0)), dfu, None)[0, 0]
    assert 0.05 < plain < 0.95
    looked_up = oracle.table_lookup(1, ramp, float(plain), 0.0)[0]
    assert looked_up != plain
    half = pk.directional_probes(oracle, [light], *one((10.0, 10.0, 2.0), w=0.5), dfu, None, ramp=ramp)[0]
    assert half[0] == F(looked_up * F(0.5)) and half[3] == 1
    assert half[0] != oracle.table_lookup(1, ramp, float(plain) * 0.5, 0.0)[0], "not the ramp of the product"
    # a 1 x 1 ramp is no ramp
    tiny = pk.directional_probes(oracle, [light], *one((10.0, 10.0, 2.0)), dfu, None, ramp=np.ones((1, 1, 4), np.float32))[0, 0]
    assert tiny == plain


def test_the_filter_and_the_ao_members_are_not_read(oracle, field):
    dfu = dc.field_uniforms()
    pp, pn = pk.probes(16)
    plain = pk.shadowed_light(0)
    odd = pk.shadowed_light(0, shadow_filter=0, ao_radius=5.0, ao_opacity=0.6)      # the frame pass would discard pairs and sample AO
    assert np.array_equal(pk.directional_probes(oracle, [odd], pp, pn, dfu, field), pk.directional_probes(oracle, [plain], pp, pn, dfu, field))


def test_the_sum_runs_in_fp32_in_light_order():
    pairs = np.zeros((1, 3, 4), np.float32)
    pairs[0, 0] = (1.0, 0, 0, 1)
    pairs[0, 1] = (0, 0, 0, 0)                       # a pair that contributes nothing: skipped, no alpha
    pairs[0, 2] = (2.0 ** -24, 0, 0, 1)              # lost against 1 in fp32
    assert np.array_equal(pk.sum_pairs(pairs), [[1.0, 0, 0, 2.0]])
    assert np.array_equal(pk.sum_pairs(pairs, light_count=2), [[1.0, 0, 0, 1.0]])


# ---- the line reference ----------------------------------------------------------------------------------------------------------------

def test_the_line_reference_is_the_sphere_probe_of_the_four_members(oracle, field):
    dfu, env = dc.field_uniforms(), scenes.environment()
    pp, pn = pk.probes(24)
    for ramp_length in (0.0, 12.0):
        lines = pk.line_lights(5, ramp_length=ramp_length)
        spheres = dc.light_array([pk.sphere_vertex_of(l) for l in lines])
        want = oracle.render_light_probes(spheres, pp, pn, env, dfu, field)
        got = pk.line_probes(oracle, dc.light_array(lines), pp, pn, env, dfu, field)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (got[:, 3] > 0).any() and (got[:, 3] < 5).any(), "some pairs are lit and some are not"
    # LightPosition2 and Color2 are not read
    moved = pk.line_lights(5)
    for l in moved:
        l.LightPosition2 = abi.f4(1.0, 2.0, 3.0, 0)
        l.Color2 = abi.f4(9.0, 9.0, 9.0, 9.0)
    assert np.array_equal(pk.line_probes(oracle, dc.light_array(moved), pp, pn, env, dfu, field),
                          pk.line_probes(oracle, dc.light_array(pk.line_lights(5)), pp, pn, env, dfu, field))


# ---- the committed probe list --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [abi.SDF_UNORM16, abi.SDF_FP16])
def test_no_pair_of_the_gpu_tests_sits_on_a_knife_edge(oracle, fmt):
    """tests/test_probe_kinds_gpu.py's shadowed cases: 65 probes x 9 shadowed lights and 129 probes x 17 lights of which four cast shadows.
    A pair whose trace leaves the loop within 1e-3 of a decision has its probe moved (pk.MOVED), not its criterion loosened."""
    tex = oracle.make_texture(dc.field_atlas(fmt), fmt)
    dfu = dc.field_uniforms()
    pp, pn = pk.probes()
    cases = [(65, [pk.shadowed_light(k) for k in range(9)]), (129, pk.mixed_lights(17, 4))]
    for count, lights in cases:
        _pairs, facts = pk.directional_pairs(oracle, lights, pp[:count], pn[:count], dfu, tex)
        traced = [key for key, f in facts.items() if "visibility" in f]
        assert len(traced) > count, "the case traces"
        assert pk.knife_edges(facts, lights) == []
