"""Pins the CPU oracle (and the host mirror's pure logic) on the committed known-answer vectors of tests/golden/.

The vectors come from tests/golden/make_golden.py: Python restatements of the reference's C# CPU mirrors
(Bezier.cs, DistanceField.cs, ParticleSpawner.cs, ParticleSpawning.cs, ParticleEngine.cs) and closed-form
answers derived by hand from the cited HLSL lines -- a second source, independent of the HLSL the oracle
restates.  The reference has no tests of its own for these paths ("parity unpinned"); this is the
substitute pin.  Runs without a GPU.
"""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from illuminant_amd import abi, scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_fixtures_are_reproducible(tmp_path):
    """make_golden.py regenerates the committed JSON byte for byte (the vectors are data + their generator)."""
    # (reference_constants.json has its own generator, tools/pin_reference_constants.py, checked by tests/test_reference_pin.py)
    # (full_frame_bands.json is the oracle over two whole frames: five minutes of CPU, its own generator make_full_frame_bands.py; the GPU
    # suite checks every band of it against the kernel, tests/test_full_frame_bands_gpu.py)
    own_generator = ("reference_constants.json", "full_frame_bands.json")
    before = {n: open(os.path.join(GOLDEN, n), "rb").read() for n in os.listdir(GOLDEN) if n.endswith(".json") and n not in own_generator}
    assert len(before) >= 7
    # run a copy of the generator in a scratch directory so the committed files are never rewritten by the test
    script = open(os.path.join(GOLDEN, "make_golden.py")).read()
    scratch = tmp_path / "make_golden.py"
    scratch.write_text(script)
    subprocess.run([sys.executable, str(scratch)], check=True, capture_output=True)
    for n, data in before.items():
        assert (tmp_path / n).read_bytes() == data, n


# ---- Bezier.cs C# mirror vs the oracle's Bezier.fxh restatement ------------------------------------------------------

def test_bezier_matches_csharp_mirror(oracle):
    doc = load("bezier.json")
    n1 = n4 = 0
    for c in doc["cases"]:
        rc = abi.f4(*c["range_and_count"])
        if c["kind"] == "bezier1":
            b = abi.ClampedBezier1()
            b.RangeAndCount = rc
            b.ABCD = abi.f4(*c["abcd"])
            got = [oracle.bezier1(b, c["value"])]
            n1 += 1
        else:
            b = abi.ClampedBezier4()
            b.RangeAndCount = rc
            b.A, b.B, b.C, b.D = abi.f4(*c["a"]), abi.f4(*c["b"]), abi.f4(*c["c"]), abi.f4(*c["d"])
            got = list(oracle.bezier4(b, c["value"]))
            n4 += 1
        np.testing.assert_allclose(got, c["expected"], rtol=1e-6, atol=1e-6, err_msg=json.dumps(c))
    assert n1 > 500 and n4 > 500


# ---- DistanceField ctor layout (oracle, Python scene builder, C++ host mirror) ---------------------------------------

LAYOUT_KEYS = ("slice_width", "slice_height", "slice_count", "physical_slice_count", "column_count", "row_count", "atlas_width", "atlas_height")


def test_distance_field_layout_kats(oracle):
    doc = load("distance_field_layout.json")
    # the three layouts quoted in SURVEY.md 8c, written out here so a reader sees the numbers
    hand = {(512, 512, 32, 1.0): (512, 512, 33, 11, 3, 4, 1536, 2048),
            (1920, 1080, 9, 0.25): (480, 270, 9, 3, 2, 2, 960, 540),
            (256, 256, 9, 1.0): (256, 256, 9, 3, 2, 2, 512, 512)}
    seen = 0
    for c in doc["cases"]:
        key = (c["virtual_width"], c["virtual_height"], c["requested_slice_count"], c["requested_resolution"])
        exp = c["expected"]
        if key in hand:
            assert tuple(exp[k] for k in LAYOUT_KEYS) == hand[key]
            seen += 1
        lay = oracle.distance_field_layout(key[0], key[1], 64.0, key[2], key[3])
        assert tuple(getattr(lay, k) for k in LAYOUT_KEYS) == tuple(exp[k] for k in LAYOUT_KEYS), key
        assert abs(lay.resolution - exp["resolution"]) < 1e-12
        # the scene builder used by tests and bench computes the same layout
        sl = scenes.DistanceFieldLayout(key[0], key[1], 64.0, key[2], key[3])
        assert (sl.slice_width, sl.slice_height, sl.slice_count, sl.physical_slice_count, sl.column_count, sl.row_count,
                sl.atlas_width, sl.atlas_height) == tuple(exp[k] for k in LAYOUT_KEYS), key
    assert seen == 3


def test_host_mirror_distance_field_layout():
    from illuminant_amd import _host as H
    for c in load("distance_field_layout.json")["cases"]:
        L = H.DistanceField.ComputeLayout(c["virtual_width"], c["virtual_height"], c["requested_slice_count"], c["requested_resolution"])
        exp = c["expected"]
        got = (L.SliceWidth, L.SliceHeight, L.SliceCount, L.PhysicalSliceCount, L.ColumnCount, L.RowCount, L.TextureWidth, L.TextureHeight)
        assert got == tuple(exp[k] for k in LAYOUT_KEYS), c
        assert abs(L.Resolution - exp["resolution"]) < 1e-12


def test_distance_field_uniforms_packing(oracle):
    """Uniforms.DistanceField ctor (Uniforms.cs:90-110) + DistanceFieldPacked1 (LightingRenderer.cs:1933-1939) on the cfg3 field."""
    lay = oracle.distance_field_layout(2048, 2048, 128.0, 32, 0.25)
    u = oracle.distance_field_uniforms(lay, max_cone_radius=24.0, power=0.7, step_limit=64, min_step_size=1.0, long_step_factor=0.5)
    assert (u.Extent.x, u.Extent.y, u.Extent.z, u.Extent.w) == (2048.0, 2048.0, 128.0, 128.0)
    assert (u.TextureSliceCount.x, u.TextureSliceCount.y, u.TextureSliceCount.w) == (3.0, 4.0, 33.0)
    assert u.TextureSliceCount.z == pytest.approx(128.0, rel=1e-6)          # all 33 slices valid => validZ = depth
    assert u.TextureSliceAndTexelSize.x == pytest.approx(1 / 3, rel=1e-6) and u.TextureSliceAndTexelSize.y == 0.25
    assert u.TextureSliceAndTexelSize.z == pytest.approx(1 / (2048 * 3), rel=1e-6)
    assert u.TextureSliceAndTexelSize.w == pytest.approx(1 / (2048 * 4), rel=1e-6)
    assert u.ConeAndMisc.x == 24.0 and u.ConeAndMisc.z == pytest.approx(0.7) and u.ConeAndMisc.w == 4.0   # InvScaleFactorX = 2048/512
    assert u.StepAndMisc2.x == 64.0 and u.StepAndMisc2.z == 0.5 and u.StepAndMisc2.w == 4.0
    assert u.Packed1.x == pytest.approx(1 / 9, rel=1e-6)                    # 1 / (3 * cols)
    assert u.Packed1.y == pytest.approx(33 / 128, rel=1e-6)                 # sliceCount / extentZ
    assert u.Packed1.z == pytest.approx(128.0, rel=1e-6) and u.Packed1.w == 1.0
    # and the Python scene builder packs the very same bytes
    su = scenes.DistanceFieldLayout(2048, 2048, 128.0, 32, 0.25).uniforms(power=0.7, min_step_size=1.0, long_step_factor=0.5)
    assert bytes(su) == bytes(u)


# ---- spawner tick arithmetic + slot allocation ----------------------------------------------------------------------

def test_spawner_begin_tick_traces(oracle):
    from illuminant_amd import _host as H
    for c in load("spawner.json")["cases"]:
        if c["kind"] != "begin_tick":
            continue
        st = oracle.SpawnerState()
        mt = -1 if c["maximum_total"] is None else c["maximum_total"]
        # the C++ host mirror replays the same scripted draws (count scale 2 = a Spawner with one additional position)
        sp = H.Spawner(1)
        sp.MinRate, sp.MaxRate = c["min_rate"], c["max_rate"]
        if c["maximum_total"] is not None:
            sp.MaximumTotal = c["maximum_total"]
        if c["count_scale"] == 2:
            sp.AdditionalPositions = [[1.0, 2.0, 3.0]]
        sp.ScriptedDraws = [t["draw"] for t in c["ticks"]]
        for t in c["ticks"]:
            n = oracle.spawner_begin_tick(st, c["min_rate"], c["max_rate"], c["count_scale"], t["draw"], c["dt"], mt)
            oracle.spawner_end_tick(st, n, n)
            assert n == t["count"]
            assert st.rate_error == pytest.approx(t["rate_error_after"], abs=1e-9)
            assert st.total_spawned == t["total_spawned_after"]
            hn = sp.BeginTick(0.0, c["dt"])
            sp.EndTick(hn, hn)
            assert hn == t["count"]
            assert sp.RateError == pytest.approx(t["rate_error_after"], abs=1e-9)
            assert sp.TotalSpawned == t["total_spawned_after"]
    # cfg2's spawner: 65536/s at 1/60 s alternates 1092,1092,1092,1093 through the RateError carry
    first = load("spawner.json")["cases"][0]
    assert [t["count"] for t in first["ticks"]][:8] == [1092, 1092, 1092, 1093, 1092, 1092, 1092, 1093]


def replay_allocation(oracle, case):
    """RunSpawner + PickTargetForSpawn (ParticleSpawning.cs:115-231) driven by the oracle's tick arithmetic."""
    cap = case["chunk_capacity"]
    st = oracle.SpawnerState()
    offsets, target, next_id = {}, -1, 1
    out = []
    for tick in case["trace"]:
        issued = []
        for p in range(2):
            req = oracle.spawner_begin_tick(st, case["min_rate"], case["max_rate"], case["count_scale"], tick["draws"][p], case["dt"], -1)
            if req <= 0:
                break
            count = min(req, cap)
            if target != -1 and cap - offsets[target] < 16:
                target = -1
            if target == -1:
                target, next_id = next_id, next_id + 1
                offsets[target] = 0
            count = min(count, cap - offsets[target])
            first = offsets[target]
            offsets[target] += count
            oracle.spawner_end_tick(st, req, count)
            issued.append([target, first, first + count - 1])
            if not req > count:
                break
        out.append((issued, st.rate_error, st.total_spawned))
    return out


def test_spawner_slot_allocation_traces(oracle):
    n = 0
    for c in load("spawner.json")["cases"]:
        if c["kind"] != "allocation":
            continue
        got = replay_allocation(oracle, c)
        for (issued, err, total), want in zip(got, c["trace"]):
            assert issued == want["issued"]                       # slot indices: bit-exact
            assert total == want["total_spawned_after"]
            assert err == pytest.approx(want["rate_error_after"], abs=1e-9)
        # a partial spawn must have happened (chunk roll-over + second pass), otherwise the case pins nothing
        assert any(len(w["issued"]) == 2 for w in c["trace"])
        n += 1
    assert n == 2


# ---- liveness count decode --------------------------------------------------------------------------------------------

def test_liveness_decode(oracle):
    for c in load("liveness.json")["cases"]:
        live = c["live_slots"]
        pos = np.zeros((max(live, 1) + 3, 4), np.float32)
        pos[:live, 3] = 1.0
        assert oracle.count_live(pos, saturate16=True) == c["expected_count"]
        assert oracle.count_live(pos, saturate16=False) == live


# ---- distance encoding + sampling -------------------------------------------------------------------------------------

def test_distance_encoding(oracle):
    for c in load("distance_encoding.json")["cases"]:
        e = oracle.encode_distance(c["distance"], c["max_distance"])
        assert e == pytest.approx(c["encoded"], abs=1e-6)
        assert oracle.decode_distance(e, c["max_distance"]) == pytest.approx(c["decoded"], abs=1e-4)
        assert oracle.decode_distance(e, c["max_distance"]) == pytest.approx(c["distance"], abs=1e-4)
    assert oracle.encode_distance(0.0, 128.0) == pytest.approx(192.0 / 255.0, abs=1e-7)   # DISTANCE_ZERO, DistanceFieldCommon.fxh:8


def test_sample_of_a_constant_field_decodes_to_the_constant(oracle):
    """Every texel of the atlas = encode(d): any bilinear / slice blend returns d (plus the distance to the volume outside it)."""
    lay = scenes.DistanceFieldLayout(256, 256, 64.0, 9, 1.0)
    dfu = lay.uniforms()
    for d in (0.0, 10.0, -20.0):
        q = int(round((192.0 / 255.0 - d / 128.0) * 65535.0))
        atlas = np.full((lay.atlas_height, lay.atlas_width, 4), q, np.uint16)
        tex = oracle.make_texture(atlas, abi.SDF_UNORM16)
        want = (192.0 / 255.0 - q / 65535.0) * 128.0
        for p in ((10.0, 20.0, 5.0), (128.3, 77.7, 31.9), (255.9, 0.1, 63.0)):
            assert oracle.sample_distance_field(p, dfu, tex) == pytest.approx(want, abs=2e-3)
        # 3 units left of the volume, 4 units below it => + 5 (DistanceFieldCommon.fxh:321-327)
        assert oracle.sample_distance_field((-3.0, 50.0, -4.0), dfu, tex) == pytest.approx(want + 5.0, abs=2e-3)


# ---- G-buffer decode ----------------------------------------------------------------------------------------------------

def test_gbuffer_round_trip(oracle):
    env = scenes.environment()
    for c in load("gbuffer.json")["cases"]:
        g = np.zeros((48, 64, 4), np.float32)
        px, py = int(c["pixel"][0]), int(c["pixel"][1])
        g[py, px] = c["texel"]
        env2 = scenes.environment(gbuffer_size=(64, 48))
        wp, n, shadows, fullbright, _cam = oracle.sample_gbuffer(float(px), float(py), env2, oracle.make_texture(g, abi.GBUFFER_FLOAT4))
        exp = c["expected"]
        assert fullbright == exp["fullbright"] and shadows == exp["enable_shadows"]
        np.testing.assert_allclose(n, exp["normal"], atol=1e-5)
        np.testing.assert_allclose(wp[:2], exp["world_xy"], atol=1e-4)
        assert wp[2] == pytest.approx(exp["world_z"], abs=2e-4)
    # ground plane without a G-buffer (LightCommon.fxh:130-141): normal +z, z = GroundZ
    wp, n, shadows, fullbright, _ = oracle.sample_gbuffer(5.0, 7.0, env, None)
    assert tuple(n) == (0.0, 0.0, 1.0) and wp[2] == 0.0 and shadows and not fullbright
    # the encoded ground-plane texel quoted in SURVEY 8c
    assert load("gbuffer.json")["cases"][0]["texel"] == [0.5, 1.0, 0.0, 1.0]


# ---- closed-form answers ------------------------------------------------------------------------------------------------

def one_slot_step(oracle, pos, vel, dt, op=None, update=False, friction=0.0, max_velocity=9999.0, life_decay=1.0):
    cs = 4
    p = np.zeros((cs * cs, 4), np.float32); v = np.zeros_like(p); a = np.ones_like(p)
    p[5], v[5] = pos, vel
    su = scenes.system_uniforms(cs, dt_seconds=dt, friction=friction, max_velocity=max_velocity, life_decay=life_decay)
    return cs, p, v, a, su


def test_closed_form_particles(oracle):
    rnd = scenes.randomness_table(7)
    for c in load("closed_form.json")["cases"]:
        k = c["kind"]
        if k == "gravity_linear":
            cs, p, v, a, su = one_slot_step(oracle, c["position"], c["velocity"], c["dt"])
            at = c["attractor"]
            g = scenes.gravity_params([(tuple(at["position"]), at["radius"], at["strength"], at["type"])], maximum_acceleration=c["maximum_acceleration"])
            oracle.gravity(p, v, cs, su, g)
            np.testing.assert_allclose(v[5], c["expected_velocity"], rtol=1e-5, atol=1e-6)
            np.testing.assert_array_equal(p[5], np.float32(c["position"]))
            assert not v[np.arange(16) != 5].any()                      # dead slots: passthrough
        elif k == "update_positions":
            cs, p, v, a, su = one_slot_step(oracle, c["position"], c["velocity"], c["dt"], friction=c["friction"],
                                            max_velocity=c["max_velocity"], life_decay=c["life_decay"])
            rc = np.zeros_like(p); rd = np.zeros_like(p)
            oracle.update(p, v, a, rc, rd, cs, su, abi.UpdateParams.default())
            np.testing.assert_allclose(p[5], c["expected_position"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(v[5], c["expected_velocity"], rtol=1e-5, atol=1e-6)
            if c["expected_position"][3] > 0:
                assert rd[5, 2] == pytest.approx(49.5, rel=1e-5)         # RenderData.z = |v| after friction
                assert rd[5, 3] == 3.0                                    # RenderData.w = category
            else:
                assert not rc[5].any() and not rd[5].any()
        elif k == "fma":
            cs, p, v, a, su = one_slot_step(oracle, c["position"], c["velocity"], c["dt"])
            f = scenes.fma_params(scenes.area_none(strength=c["strength"]), cycles_per_second=c["cycles_per_second"],
                                  position_add=tuple(c["position_add"]), position_multiply=tuple(c["position_multiply"]),
                                  velocity_add=tuple(c["velocity_add"]), velocity_multiply=tuple(c["velocity_multiply"]))
            oracle.fma(p, v, cs, su, f)
            np.testing.assert_allclose(p[5], c["expected_position"], rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(v[5], c["expected_velocity"], rtol=1e-5, atol=1e-5)


def test_closed_form_lights(oracle):
    env = scenes.environment()
    dfu = scenes.DistanceFieldLayout(64, 64, 64.0, 3, 1.0).uniforms()
    n = 0
    for c in load("closed_form.json")["cases"]:
        if c["kind"] not in ("light_at_pixel", "linear_ramp"):
            continue
        L = c["light"]
        lights = (abi.LightVertex * 1)(scenes.sphere_light(tuple(L["position"]), L["radius"], L["ramp"], color=tuple(L["color"]), casts_shadows=False))
        img, _ = oracle.render_sphere_lights(lights, env, dfu, None, None, tuple(c["ambient"]), 32, 16)
        px, py = c["pixel"]
        if c["kind"] == "light_at_pixel":
            np.testing.assert_allclose(img[py, px], c["expected"], rtol=1e-6)
        else:
            # the light sits on pixel (4, 4)'s VPOS: the distance to pixel (4 + d, 4) is exactly d
            assert img[py, px, 0] == pytest.approx(c["expected_rgb"], rel=1e-5)
            assert img[py, px, 3] == 2.0
        n += 1
    assert n == 4


def test_oracle_is_test_infrastructure_only():
    """Nothing in the product package may import or link the oracle (it would void every parity claim)."""
    root = os.path.dirname(GOLDEN.rstrip("/"))
    root = os.path.dirname(root)
    bad = []
    for base, _dirs, files in os.walk(os.path.join(root, "illuminant_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h", "Makefile")):
                text = open(os.path.join(base, f), errors="replace").read()
                if "oracle" in text and ("import oracle" in text or "from oracle" in text or "ilm_oracle" in text or "libilm_oracle" in text):
                    bad.append(os.path.join(base, f))
    assert not bad, bad


# ---- the oracle's distance-field sampler against a float64 restatement of LINEAR / U WRAP / V CLAMP ----------------------------

def _sampler_kat_field():
    """A 13 x 11 UNORM16 atlas whose channel r holds a distinct code per texel (row * 13 + column, 200 codes apart, all in the upper
    half): a wrong row or column is an error of at least 0.003, never a rounding difference."""
    w, h = 13, 11
    codes = 32768 + 200 * np.arange(w * h, dtype=np.int64).reshape(h, w)
    atlas = np.random.default_rng(17).integers(0, 65536, size=(h, w, 4), dtype=np.uint16)
    atlas[..., 0] = codes.astype(np.uint16)
    return atlas, codes


def _sampler_kat_uniforms(texel_u, texel_v):
    """Slice-0 uniforms that put the sampler's texture coordinate at (u, v) = (x * texel_u, y * texel_v) for any position inside a huge
    extent: Packed1 = 0 (virtual slice 0, z weight 0), no slice offsets, Extent.w = 1 -- the result is DISTANCE_ZERO - r exactly."""
    u = abi.DistanceFieldUniforms()
    u.TextureSliceAndTexelSize = abi.f4(0.0, 0.0, texel_u, texel_v)
    u.Extent = abi.f4(3e38, 3e38, 0.0, 1.0)
    return u


def _reference_tap(codes, u, v):
    """D3D's LINEAR filter with U WRAP and V CLAMP (DistanceFieldCommon.fxh:273-281), in float64 and Python integers: texel centres at
    +0.5, the tap origin floor(u * W - 0.5) -- the coordinate itself rounded once to fp32, as the sampler's fused multiply-add forms
    it -- wrapped modulo W, clamped to [0, H - 1].  Returns (blended channel r, the four taps)."""
    h, w = codes.shape
    x = float(np.float32(u * w - 0.5))       # u * w - 0.5 is exact in float64 for the coordinates drawn below
    y = float(np.float32(v * h - 0.5))
    x0f, y0f = math.floor(x), math.floor(y)
    fx, fy = x - x0f, y - y0f
    x0, x1 = x0f % w, (x0f + 1) % w
    y0, y1 = min(max(y0f, 0), h - 1), min(max(y0f + 1, 0), h - 1)
    c = codes / 65535.0
    top = (1.0 - fx) * c[y0, x0] + fx * c[y0, x1]
    bot = (1.0 - fx) * c[y1, x0] + fx * c[y1, x1]
    return (1.0 - fy) * top + fy * bot, (fx, fy, c[y0, x0])


def _kat_coordinates(rng):
    """(u, v) pairs: many U wraps both ways, V below 0 and above 1, and tap coordinates at and beyond 2^31 on both axes."""
    w, h = 13, 11
    us, vs = [], []
    small_u = rng.uniform(-40.0, 40.0, 400).astype(np.float32)           # +-40 atlas widths: hundreds of wraps, negative U
    small_v = rng.uniform(-3.0, 4.0, 400).astype(np.float32)             # V below 0, inside, above 1
    us += list(small_u); vs += list(small_v)
    # texel centres and texel edges: the tap origin and its neighbour exactly, on both sides of every wrap seam and clamp edge
    for i in range(-2 * w, 2 * w + 1):
        for j in (-3, -1, 0, 1, h - 1, h, h + 2):
            us += [np.float32((i + 0.5) / w), np.float32(i / w)]
            vs += [np.float32((j + 0.5) / h), np.float32(j / h)]
    # at and beyond 2^31 texels: integer-valued coordinates with few significant bits, so u * W is exact in fp32
    big = [2.0 ** 31, 2.0 ** 31 + 2.0 ** 16, 3.0 * 2.0 ** 31, 2.0 ** 32 - 2.0 ** 12, 2.0 ** 40, 12345.0 * 2.0 ** 30, 2.0 ** 53]
    for b in big:
        for s in (1.0, -1.0):
            for k in (0.0, 1.0, 7.0):
                us.append(np.float32(s * (b + k * 2.0 ** 20) / 2.0 ** 3)); vs.append(np.float32(rng.uniform(0.0, 1.0)))   # U only
                us.append(np.float32(rng.uniform(0.0, 1.0))); vs.append(np.float32(s * (b + k * 2.0 ** 20) / 2.0 ** 3))   # V only
        us.append(np.float32(b / 2.0 ** 3)); vs.append(np.float32(-b / 2.0 ** 3))
    us += [np.float32(2.0 ** 31 / w), np.float32(-(2.0 ** 31) / w)]; vs += [np.float32(2.0 ** 31 / h), np.float32(-(2.0 ** 31) / h)]
    return np.array(us, np.float32), np.array(vs, np.float32)


def test_distance_field_sampler_wraps_u_and_clamps_v_for_every_coordinate(oracle):
    """oracle.sample_distance_field's texture fetch against _reference_tap, written from the sampler state (LINEAR, U WRAP, V CLAMP)
    and not from the oracle: the taps must be the exact texels for every coordinate -- hundreds of wraps, negative U, V outside
    [0, 1], tap indices at and beyond 2^31, where a cast of the float to int is undefined -- and the blend within 1e-6."""
    atlas, codes = _sampler_kat_field()
    tex = oracle.make_texture(np.ascontiguousarray(atlas), abi.SDF_UNORM16)
    zero = np.float32(192.0) / np.float32(255.0)                           # DISTANCE_ZERO (DistanceFieldCommon.fxh:8), correctly rounded
    us, vs = _kat_coordinates(np.random.default_rng(23))
    n_exact = n_huge = 0
    for u, v in zip(us, vs):
        # u = x * texel_u with x >= 0 inside the extent: a negative coordinate through a negative texel size, exactly
        dfu = _sampler_kat_uniforms(-1.0 if u < 0 else 1.0, -1.0 if v < 0 else 1.0)
        got = np.float32(oracle.sample_distance_field((abs(float(u)), abs(float(v)), 0.0), dfu, tex))
        want, (fx, fy, c00) = _reference_tap(codes, float(u), float(v))
        blended = float(zero) - float(got)
        assert abs(blended - want) <= 1e-6 * abs(want), (u, v, blended, want)
        if fx == 0.0 and fy == 0.0:
            # the sample is the origin tap itself: bit for bit (the decode is code / 65535 rounded once)
            assert got == np.float32(zero - np.float32(np.float32(c00 * 65535.0) / np.float32(65535.0))), (u, v, got)
            n_exact += 1
        n_huge += abs(float(u)) * 13 >= 2.0 ** 31 or abs(float(v)) * 11 >= 2.0 ** 31
    assert n_exact > 300 and n_huge > 80, (n_exact, n_huge)


def test_distance_field_sampler_gives_nan_for_nan_coordinates(oracle):
    """A NaN or infinite texture coordinate (a NaN / infinite texel size, 0 x inf) names no texel: the sample is NaN, whatever tap the
    index arithmetic falls on."""
    atlas, _ = _sampler_kat_field()
    tex = oracle.make_texture(np.ascontiguousarray(atlas), abi.SDF_UNORM16)
    nan, inf = float("nan"), float("inf")
    cases = [((5.0, 3.0), (nan, 1.0)), ((5.0, 3.0), (1.0, nan)), ((5.0, 3.0), (inf, 1.0)), ((5.0, 3.0), (1.0, -inf)),
             ((0.0, 3.0), (inf, 1.0)), ((5.0, 0.0), (1.0, inf)), ((5.0, 3.0), (nan, nan)), ((2e38, 3.0), (1e30, 1.0))]
    for (x, y), (tu, tv) in cases:
        got = oracle.sample_distance_field((x, y, 0.0), _sampler_kat_uniforms(tu, tv), tex)
        assert math.isnan(got), ((x, y), (tu, tv), got)


# ---- every other table lookup of the particle and light paths against a float64 / Python-integer restatement -------------------------

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


def _ulp_neighbours(t):
    """t and its two fp32 neighbours."""
    t = F32(t)
    return [np.nextafter(t, F32(-np.inf)), t, np.nextafter(t, F32(np.inf))]


def lookup_tap_matrix(size):
    """The tap indices (fp32) every lookup is driven across: 0, -0, +-denormal, just below and above each table edge, +-(2^22, 2^23, 2^24)
    +- 1 ulp, +-2^31 +- 1 ulp, +-2^40, +-FLT_MAX, +-inf and NaN."""
    den = float(np.finfo(np.float32).smallest_subnormal)
    taps = [0.0, -0.0, den, -den]
    for edge in (0.0, 1.0, float(size - 1), float(size), float(2 * size)):
        taps += [edge - 0.5, edge + 0.5] + [float(x) for x in _ulp_neighbours(edge)] + [-edge]
    for e in (22, 23, 24, 31):
        for s in (1.0, -1.0):
            taps += [s * float(x) for x in _ulp_neighbours(2.0 ** e)]
    taps += [2.0 ** 40, -(2.0 ** 40), FLT_MAX, -FLT_MAX, math.inf, -math.inf, math.nan]
    return [F32(t) for t in taps]


def _wrap(t, size):
    """WRAP of an integer-valued tap (a Python float): exact for every finite value; NaN / infinity name no texel, tap 0."""
    return int(t) % size if math.isfinite(t) else 0


def _clamp(t, size):
    """CLAMP of an integer-valued tap: NaN gives tap 0, -inf tap 0, +inf the last."""
    if math.isnan(t):
        return 0
    return int(min(max(t, 0.0), float(size - 1))) if math.isfinite(t) else (0 if t < 0 else size - 1)


def _floor(t):
    return math.floor(t) if math.isfinite(t) else t


def _coded_table(w, h):
    """(h, w, 4) float32: texel (x, y) = (x / 64, y / 64, (x + 1) / 1024, 1) -- every texel names its own column and row."""
    ys, xs = np.mgrid[0:h, 0:w]
    t = np.zeros((h, w, 4), np.float32)
    t[..., 0], t[..., 1], t[..., 2], t[..., 3] = xs / 64.0, ys / 64.0, (xs + 1) / 1024.0, 1.0
    return t


def _lerp64(a, b, t):
    return a + (b - a) * t


def _linear64(texel, sx, sy, col, row):
    """float64 LINEAR blend at the fp32 tap coordinates (sx, sy); col / row map an integer tap to a texel column / row."""
    x0f, y0f = _floor(sx), _floor(sy)
    fx, fy = sx - x0f, sy - y0f
    if not (math.isfinite(fx) and math.isfinite(fy)):
        return None                                           # NaN weights: the sample is NaN
    x0, y0 = int(x0f), int(y0f)
    c0, c1, r0, r1 = col(x0), col(x0 + 1), row(y0), row(y0 + 1)
    return _lerp64(_lerp64(texel(c0, r0), texel(c1, r0), fx), _lerp64(texel(c0, r1), texel(c1, r1), fx), fy)


def _check_linear(got, want, what):
    if want is None:
        assert np.all(np.isnan(got[:3])), (what, got)
    else:
        assert np.allclose(got[:3].astype(np.float64), want[:3], rtol=1e-6, atol=1e-7), (what, got, want)


def test_life_ramp_point_clamp_u_wrap_v_for_every_coordinate(oracle):
    """readLifeRamp (POINT, U CLAMP, V WRAP): the texel is floor(u * w) clamped and floor(v * h) wrapped, exactly, for every float.  A
    cast of u * w to int is undefined from 2^31 on (x86 gives INT_MIN, which clamped to column 0 instead of the last)."""
    w, h = 7, 5
    table = _coded_table(w, h)
    n = 0
    for tu in lookup_tap_matrix(w):
        for tv in lookup_tap_matrix(h):
            u, v = F32(tu) / F32(w), F32(tv) / F32(h)
            got = oracle.table_lookup(0, table, u, v)
            x = _clamp(_floor(float(F32(u * F32(w)))), w)
            y = _wrap(_floor(float(F32(v * F32(h)))), h)
            assert np.array_equal(got, table[y, x]), (u, v, got, (x, y))
            n += 1
    assert n > 1500


def test_light_ramp_linear_clamp_u_wrap_v_for_every_coordinate(oracle):
    """SampleFromRamp2 (LINEAR, U CLAMP, V WRAP, texel centres at +0.5) against a float64 blend of the exact taps."""
    w, h = 6, 9
    table = _coded_table(w, h)
    texel = lambda c, r: table[r, c].astype(np.float64)
    for tu in lookup_tap_matrix(w):
        for tv in lookup_tap_matrix(h):
            u, v = F32(tu) / F32(w), F32(tv) / F32(h)
            got = oracle.table_lookup(1, table, u, v)
            sx, sy = float(F32(F32(u * F32(w)) - F32(0.5))), float(F32(F32(v * F32(h)) - F32(0.5)))
            want = _linear64(texel, sx, sy, lambda i: _clamp(float(i), w), lambda i: _wrap(float(i), h))
            _check_linear(got, want, (u, v))


def test_random_custom_point_wrap_for_every_offset(oracle):
    """randomCustom (POINT, WRAP) at coordinate 0 with the offset driving the tap: floor(((0 + offset) * texel) * size) wrapped, for
    every float offset (the ABI refuses |offset| >= 2^22; the oracle still decides the rest exactly)."""
    rw, rh = 13, 7
    table = _coded_table(rw, rh)
    for ox in lookup_tap_matrix(rw):
        for oy in lookup_tap_matrix(rh):
            got = oracle.table_lookup(2, table, 0.0, 0.0, ox, oy)
            tx = _floor(float(F32(F32(F32(F32(0.0) + ox) * (F32(1.0) / F32(rw))) * F32(rw))))
            ty = _floor(float(F32(F32(F32(F32(0.0) + oy) * (F32(1.0) / F32(rh))) * F32(rh))))
            want = table[_wrap(ty, rh), _wrap(tx, rw)]
            assert np.array_equal(got, want), (ox, oy, got, want)


def test_smooth_random_custom_linear_wrap_for_every_coordinate(oracle):
    """smoothRandomCustom (LINEAR, WRAP on both axes, on the Rgba64 copy) at coordinates that run to +-FLT_MAX and past: the taps are the
    exact wrapped texels; from 2^24 on the fraction is 0 and the second tap carries no weight."""
    rw, rh = 11, 5
    table = _coded_table(rw, rh)
    lp = np.round(np.clip(table, 0, 1) * 65535.0) / 65535.0
    texel = lambda c, r: lp[r, c].astype(np.float64)
    for tx in lookup_tap_matrix(rw):
        for ty in lookup_tap_matrix(rh):
            got = oracle.table_lookup(3, table, tx, ty)
            sx = float(F32(F32(F32(F32(tx * F32(1.0)) + F32(0.0)) * (F32(1.0) / F32(rw))) * F32(rw)) - F32(0.5))
            sy = float(F32(F32(F32(F32(ty * F32(1.0)) + F32(0.0)) * (F32(1.0) / F32(rh))) * F32(rh)) - F32(0.5))
            want = _linear64(texel, sx, sy, lambda i: _wrap(float(i), rw), lambda i: _wrap(float(i), rh))
            _check_linear(got, want, (tx, ty))


def test_spawner_position_index_stays_inside_the_positions(oracle):
    """The position index t % count (HLSL: fmod, then truncation) for every float t and count 1 .. 4: the exact remainder where the
    reference can produce it (t >= 0), and never an index outside [0, count) for what the ABI refuses."""
    table = _coded_table(1, 1)
    for count in (1.0, 2.0, 3.0, 4.0):
        for t in lookup_tap_matrix(4):
            got = int(oracle.table_lookup(4, table, t, count, count)[0])
            assert 0 <= got < int(count), (t, count, got)
            if math.isfinite(t) and t >= 0:
                assert got == int(math.fmod(float(t), count)), (t, count, got)


def _wrap_index_fast(t, size, rcp_ulps):
    """hlsl_math.hpp wrap_index_fast in fp32 without contraction, with v_rcp_f32 modelled as 1 / size moved by rcp_ulps ulps."""
    fs = F32(size)
    rcp = F32(1.0) / fs
    for _ in range(abs(rcp_ulps)):
        rcp = np.nextafter(rcp, F32(np.inf) if rcp_ulps > 0 else F32(-np.inf))
    q = np.floor(F32(t) * rcp)
    r = F32(F32(t) - F32(q * fs))
    r = F32(r + fs) if r < 0 else r
    r = F32(r - fs) if r >= fs else r
    return r


def test_wrap_index_fast_is_exact_only_below_the_refusal_bound():
    """randomCustom's fast WRAP is exact for |tap| < 2^23 whichever way the reciprocal errs by an ulp, which is what the ABI's refusal of
    |RandomnessOffset| >= 2^22 keeps it to; beyond, the single fold can even leave [0, size), a read outside the randomness table."""
    rng = np.random.default_rng(5)
    with np.errstate(all="ignore"):
        for size in (807, 653, 253, 127, 13, 4, 3):
            for t in list(rng.integers(-(2 ** 23) + 1, 2 ** 23, 3000)) + [0, 1, -1, size, -size, 2 ** 23 - 1, -(2 ** 23) + 1]:
                for ulps in (-1, 0, 1):
                    assert int(_wrap_index_fast(F32(t), size, ulps)) == int(t) % size, (size, t, ulps)
        outside = [(t, ulps) for t in (F32(2.0 ** 30 + 256.0 * k) for k in range(1, 64)) for ulps in (-1, 0, 1)
                   if not 0 <= _wrap_index_fast(t, 253, ulps) < 253]
    assert outside, "the fold stayed inside the table beyond 2^24: the refusal bound would no longer need its proof"
