"""Particle sensors without a GPU: the numpy statement of PS_CollectParticles (tests/sensor_common.py) on hand-computed cases, the
invariants of the builder the GPU tests count over, and the three entry points' place in the ABI (header, library, ctypes binding,
generated C# binding, README) with the refusals that need no device."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from illuminant_amd import abi, native
from tests import sensor_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "illuminant_hip.h")
SYMBOLS = ("ilm_system_sense", "ilm_system_sense_async", "ilm_system_poll_sense")
F = np.float32

# ---- hand-computed cases -------------------------------------------------------------------------------------------------------------
# AreaRotation = 0.5 is the unit quaternion (0.5, 0.5, 0.5, 0.5): a turn of a third about (1, 1, 1), which permutes the axes.  Every
# shape below is 10 wide along each of its own axes (the cylinder's radius is length((6, 8)) = 10, the octagon's apothem is 10), so a
# point t along a world axis from the centre is at distance t - 10 whichever axis it lands on.  With AreaFalloff = 10:
#   t = 0      d = -10    1 - saturate(-1)    = 1       counted
#   t = 15     d = 5      1 - 0.5             = 0.5     counted
#   t = 19.8   d = 9.8    1 - 0.98            = 0.02    counted
#   t = 19.95  d = 9.95   1 - 0.995           = 0.005   not counted (<= 0.01)
HAND_T = (0.0, 15.0, 19.8, 19.95)
HAND_SIZES = {1: (10.0, 10.0, 10.0), 2: (10.0, 10.0, 10.0), 3: (6.0, 8.0, 10.0), 4: (10.0, 10.0, 10.0), 5: (10.0, 10.0, 10.0)}
HAND_CENTER = (40.0, -20.0, 8.0)


def hand_case(type_id):
    """16 slots: the four points x life (1.0, 1.5) x category (2 inside the filter [1, 3], 5 outside); (sensor, pos, vel, expected mask)."""
    a = sc.sensor(type_id, center=HAND_CENTER, size=HAND_SIZES.get(type_id, (10.0, 10.0, 10.0)), falloff=0.0 if type_id == 0 else 10.0, rotation=0.5)
    pos, vel, want = np.zeros((16, 4), F), np.zeros((16, 4), F), np.zeros(16, bool)
    i = 0
    for t in HAND_T:
        for life in (1.0, 1.5):
            for category in (2.0, 5.0):
                pos[i] = (HAND_CENTER[0] + t, HAND_CENTER[1], HAND_CENTER[2], life)
                vel[i, 3] = category
                inside = True if type_id == 0 else t < 19.9
                want[i] = inside and life > 1.0 and category == 2.0
                i += 1
    return a, pos, vel, want


@pytest.mark.parametrize("type_id", [0, 1, 2, 3, 4, 5])
def test_hand_computed_case(oracle, type_id):
    a, pos, vel, want = hand_case(type_id)
    assert int(want.sum()) == (4 if type_id == 0 else 3)
    counts = sc.check_case(oracle, [a], [(pos, vel)])
    got = sc.mask(a, pos, vel, sc.scaled_distance(a, sc.oracle_distance(oracle, a, pos)))
    assert np.array_equal(got, want), (got, want)
    assert counts.tolist() == [[int(want.sum())]]
    if type_id:
        d = sc.oracle_distance(oracle, a, pos[::4])
        assert np.allclose(d, np.array(HAND_T) - 10.0, rtol=0, atol=1e-4), d


def test_life_is_tested_against_one_not_zero(oracle):
    """CollectParticles.fx:32 discards worldPosition.w <= 1: a particle that lives, with life in (0, 1], is not counted."""
    a = sc.sensor(0, falloff=0.0, category_filter=sc.EVERY_CATEGORY)
    pos, vel = np.zeros((len(sc.LIVES), 4), F), np.zeros((len(sc.LIVES), 4), F)
    pos[:, 3] = sc.LIVES
    got = sc.mask(a, pos, vel, sc.scaled_distance(a, sc.oracle_distance(oracle, a, pos)))
    assert got.tolist() == [False, False, False, True, True, True]
    assert pos[2, 3] == 1.0 and pos[3, 3] > 1.0 and pos[3, 3] - 1.0 < 2e-7


def test_no_area_counts_every_slot_the_filter_and_the_life_keep(oracle):
    """AreaType 0: evaluateByTypeId returns 0; with the effect default AreaFalloff = 0 the quotient is 0 / 0 = NaN, saturate(NaN) = 0 and the
    scaled distance is 1 -- as it is for every other finite falloff, negative ones included."""
    pos = np.zeros((5, 4), F)
    pos[:, :3] = sc.draw_positions(3, 5)
    for falloff in (0.0, -0.0, 1.0, -3.0, 1e-30):
        a = sc.sensor(0, falloff=falloff)
        d = sc.oracle_distance(oracle, a, pos)
        assert not d.any()
        assert np.array_equal(sc.scaled_distance(a, d), np.ones(5, F))
    with np.errstate(all="ignore"):
        assert np.isnan(F(0) / F(0))


# ---- the builder ---------------------------------------------------------------------------------------------------------------------

def test_builder_invariants(oracle):
    """What the GPU tests rely on: the band around the threshold is empty for every sensor and slot (check_case asserts it, with the
    agreement of the two readings), every life and category value occurs, and every area sees positions inside, in its falloff shell
    and outside of it."""
    cs = 20
    sensors, chunks, counts = sc.standard_case(oracle, cs, 3)
    assert len(sensors) == abi.MAX_SENSORS and counts.shape == (8, 3)
    assert [int(a.AreaType) for a in sensors[:6]] == [0, 1, 2, 3, 4, 5] and sensors[0].AreaFalloff == 0.0
    assert any(a.AreaRotation != 0.0 for a in sensors) and sensors[7].AreaRotation == 0.0
    for pos, vel in chunks:
        assert pos.shape == vel.shape == (cs * cs, 4)
        assert set(pos[:, 3].tolist()) == set(sc.LIVES.tolist()) and set(vel[:, 3].tolist()) == set(sc.CATEGORIES.tolist())
        for k, a in enumerate(sensors[1:6], 1):
            inside, shell, outside = sc.classes(oracle, a, pos)
            assert inside >= 8 and shell >= 8 and outside >= 8, (k, inside, shell, outside)
    assert not counts[6].any()                       # the filter that passes nothing
    assert counts[:6].all() and counts[7].all()
    # a sensor counts fewer slots than the filter and the life alone keep, and the chunks differ
    assert (counts[1:6] < counts[0]).all() and len({tuple(row) for row in counts.T.tolist()}) == 3
    # the categories on the bounds are inside the filter, their neighbours outside (checkCategoryFilter is >= and <=)
    pos, vel = chunks[0]
    a = sensors[0]
    kept = sc.mask(a, pos, vel, np.ones(cs * cs, F)) | (pos[:, 3] <= 1)
    assert kept[vel[:, 3] == F(1)].all() and kept[vel[:, 3] == F(3)].all()
    assert not kept[(vel[:, 3] < F(1)) & (pos[:, 3] > 1)].any() and not kept[(vel[:, 3] > F(3)) & (pos[:, 3] > 1)].any()


def test_builder_keeps_the_band_empty_on_an_advanced_state(oracle):
    """advance: the band is kept empty on the state the sensors will see, not on the uploaded one."""
    shift = np.array([3.0, -2.0, 1.0, 0.0], F)
    sensors = sc.standard_sensors()[1:3]
    pos, vel = sc.build_chunk(oracle, 77, 200, sensors, advance=lambda p, v: (p + shift, v))
    sc.check_case(oracle, sensors, [(pos + shift, vel)])


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------

def generator():
    spec = importlib.util.spec_from_file_location("gen_csharp_binding", os.path.join(ROOT, "tools", "gen_csharp_binding.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_header_library_and_bindings_agree():
    text = open(HEADER).read()
    assert re.search(r"#define ILM_MAX_SENSORS 8\b", text) and abi.MAX_SENSORS == 8
    assert C.sizeof(abi.AreaParams) == 64 and abi.AreaParams.CategoryFilter.offset == 48
    gen = generator()
    functions = [name for _, name, _ in gen.parse_functions(gen.strip_comments(text))]
    lib = native.lib()
    for symbol in SYMBOLS:
        assert symbol in functions and symbol in native.SYMBOLS and hasattr(lib, symbol)
        # every new entry cites the shader and the transform it replaces
        comment = text[:text.index("int32_t %s(" % symbol)].rsplit("/*", 1)[1]
        assert "CollectParticles.fx" in comment and "Transforms.cs" in comment, symbol
    binding = open(os.path.join(ROOT, "integration", "IlluminantHip.cs")).read()
    assert "ilm_system_sense (ulong system, int firstChunk, int chunkCount, IlmAreaParams* sensors, int sensorCount, uint* outCounts, int capacity)" in binding
    assert "ilm_system_sense_async (ulong system, int firstChunk, int chunkCount, IlmAreaParams* sensors, int sensorCount)" in binding
    assert "ilm_system_poll_sense (ulong system, uint* outCounts, int capacity, int* outReady)" in binding
    assert "public const int MAX_SENSORS = 8;" in binding
    assert binding == gen.generate()[0]
    # the README's entry count is the header's
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "(%d `extern \"C\"` entry points" % len(functions) in readme
    assert "all %d entry points" % len(functions) in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_entry_points_refuse_bad_handles_without_a_device():
    """The handle comes first: nothing behind it is read or written, whatever else is wrong with the call."""
    lib = native.lib()
    sensors = (abi.AreaParams * 2)()
    for handle in (0, 12345):
        out = (C.c_uint32 * 4)(7, 7, 7, 7)
        ready = C.c_int32(-7)
        assert lib.ilm_system_sense(abi.Handle(handle), 0, -1, C.cast(sensors, C.c_void_p), 2, C.cast(out, C.c_void_p), 4) == abi.ERR_INVALID_HANDLE
        assert b"system" in lib.ilm_last_error()
        assert lib.ilm_system_sense_async(abi.Handle(handle), 0, -1, C.cast(sensors, C.c_void_p), 2) == abi.ERR_INVALID_HANDLE
        assert lib.ilm_system_poll_sense(abi.Handle(handle), C.cast(out, C.c_void_p), 4, C.byref(ready)) == abi.ERR_INVALID_HANDLE
        assert list(out) == [7, 7, 7, 7] and ready.value == -7
    assert lib.ilm_system_sense(abi.Handle(0), 0, -1, None, 99, None, -1) == abi.ERR_INVALID_HANDLE
    assert lib.ilm_system_sense_async(abi.Handle(0), -5, 3, None, 0) == abi.ERR_INVALID_HANDLE
    assert lib.ilm_system_poll_sense(abi.Handle(0), None, 0, None) == abi.ERR_INVALID_HANDLE
