"""Table lookups of the particle path at coordinates far past their tables, through the C ABI ("Table lookups").

The life ramp's U is CLAMP and its V is WRAP, decided exactly for every float (the device's float -> int cast saturates from 2^31 on,
where CLAMP and WRAP need the exact tap).  The ramp is built so that every texel names its own (x, y): the chosen texel is read back from
the render colour and held to a Python-integer restatement, the render colour to the oracle bit for bit, and the default step to the
interpreting step.  The randomness offsets and the spawner's position index are refused where the reference cannot produce them:
one test per refusal, each checking the message and that the refused step changed nothing.
"""
import math

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests.test_oracle_kat import F32, _clamp, _floor, _wrap, lookup_tap_matrix
from tests.test_particles_gpu import download_state, make_system, upload_state

pytestmark = pytest.mark.gpu

CS = 64
RAMP_W, RAMP_H = 7, 5


@pytest.fixture(scope="module")
def rnd():
    return scenes.randomness_table(7)


def _coded_ramp():
    """texel (x, y) = (x / 64, y / 64, (x + 1) / 1024, 1): dyadic, so lerp(1, texel, 1) and the alpha multiply are exact."""
    ys, xs = np.mgrid[0:RAMP_H, 0:RAMP_W]
    t = np.zeros((RAMP_H, RAMP_W, 4), np.float32)
    t[..., 0], t[..., 1], t[..., 2], t[..., 3] = xs / 64.0, ys / 64.0, (xs + 1) / 1024.0, 1.0
    return t


def _lives():
    """One life per slot: the non-negative, non-NaN entries of the tap matrix over the ramp width, as u * w = tap (life = tap / w)."""
    taps = [float(t) for t in lookup_tap_matrix(RAMP_W) if not math.isnan(t)]
    lives = sorted({float(F32(abs(t)) / F32(RAMP_W)) for t in taps} - {0.0})
    out = np.array([lives[i % len(lives)] for i in range(CS * CS)], np.float32)
    return out


# IndexDivisor: v = index / divisor puts V taps at 0 .. 2^14 * 5 * 2^k, at +-inf (divisor 0) and at NaN (index 0, divisor 0)
INDEX_DIVISORS = [1.0, 2.0 ** -10, 2.0 ** -20, 2.0 ** -28, 2.0 ** -60, -(2.0 ** -28), float(np.finfo(np.float32).smallest_subnormal), 0.0,
                  math.inf, math.nan]


def _update(ctx, rnd, up, lives, interpreter):
    eng, sysm = make_system(ctx, rnd, CS)
    n = CS * CS
    pos = np.zeros((n, 4), np.float32)
    pos[:, 0] = np.arange(n) % CS
    pos[:, 1] = np.arange(n) // CS
    pos[:, 3] = lives
    vel = np.zeros((n, 4), np.float32)
    attr = np.ones((n, 4), np.float32)
    su = scenes.system_uniforms(CS, friction=0.0, max_velocity=70.0, life_decay=0.0)
    prev = native.lib().ilm_debug_step_interpreter(interpreter)
    try:
        upload_state(sysm, 0, pos, vel, attr)
        sysm.set_life_ramp(_coded_ramp())
        sysm.update(0, su, up)
        got = download_state(sysm, 0)
    finally:
        native.lib().ilm_debug_step_interpreter(prev)
        sysm.close(); eng.close()
    return (pos, vel, attr), su, got


@pytest.mark.parametrize("divisor", INDEX_DIVISORS)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_life_ramp_clamps_u_and_wraps_v_at_every_coordinate(ctx, oracle, rnd, divisor, sign):
    """readLifeRamp (POINT, U CLAMP, V WRAP) with u = life / +-1 across the tap matrix and v = index / IndexDivisor from 0 to past 2^40,
    infinite and NaN: bits equal to the oracle, the decoded texel equal to the restatement, default step equal to the interpreter."""
    up = abi.UpdateParams.default()
    up.LifeRampSettings = abi.f4(1.0, 0.0, sign, divisor)
    lives = _lives()
    (pos, vel, attr), su, got = _update(ctx, rnd, up, lives, 0)
    _, _, got_interp = _update(ctx, rnd, up, lives, 1)
    n = CS * CS
    want = [pos.copy(), vel.copy(), attr.copy(), np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)]
    oracle.update(want[0], want[1], want[2], want[3], want[4], CS, su, up, life_ramp=_coded_ramp())
    rc = got[3]
    assert np.array_equal(rc.view(np.uint32), got_interp[3].view(np.uint32)), "default step and interpreter differ"
    assert np.array_equal(rc.view(np.uint32), want[3].view(np.uint32)), \
        "render colour differs from the oracle at %d slots" % int((rc.view(np.uint32) != want[3].view(np.uint32)).any(axis=1).sum())
    wrong = []
    with np.errstate(all="ignore"):
        for i in range(n):
            u = float(F32(F32(lives[i]) / F32(sign)))
            index = float(F32(F32(i % CS) + F32(F32(i // CS) * F32(256.0))))
            v = float(F32(index) / F32(divisor)) if divisor != 0.0 else (math.nan if index == 0.0 else math.inf)
            x = _clamp(_floor(float(F32(F32(u) * F32(RAMP_W)))), RAMP_W)
            y = _wrap(_floor(float(F32(F32(v) * F32(RAMP_H)))), RAMP_H)
            gx, gy = int(round(float(rc[i, 0]) * 64.0)), int(round(float(rc[i, 1]) * 64.0))
            if (gx, gy) != (x, y):
                wrong.append((i, lives[i], v, (gx, gy), (x, y)))
    assert not wrong, "%d slots read the wrong texel, e.g. %s" % (len(wrong), wrong[:4])


# ---- refusals: the randomness offsets and the spawner's position index ---------------------------------------------------------

def _state(sysm):
    return [a.copy() for a in download_state(sysm, 0)]


def _refused(ctx, rnd, desc, needle):
    eng, sysm = make_system(ctx, rnd, CS)
    try:
        pos, vel, attr = scenes.make_particles(3, CS * CS, dead_fraction=0.5)
        upload_state(sysm, 0, pos, vel, attr)
        before = _state(sysm)
        with pytest.raises(native.IlluminantError) as e:
            sysm.step(desc)
        assert e.value.code == abi.ERR_OUT_OF_RANGE, e.value
        assert needle in str(e.value), e.value
        after = _state(sysm)
        for a, b in zip(before, after):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "a refused step changed the system"
    finally:
        sysm.close(); eng.close()


def _desc():
    d = abi.StepDesc()
    d.FirstChunk, d.ChunkCount = 0, -1
    d.System = scenes.system_uniforms(CS)
    d.Update = abi.UpdateParams.default()
    d.UpdateMode = abi.UPDATE_POSITIONS
    return d


@pytest.mark.parametrize("field,value", [("RandomnessOffset", 4194304.0), ("NextRandomnessOffset", -4194304.0),
                                         ("RandomnessOffset", math.nan), ("NextRandomnessOffset", math.inf)])
def test_noise_offset_outside_the_exact_wrap_is_refused(ctx, rnd, field, value):
    d = _desc()
    d.OpCount = 1
    d.Ops[0].Type = abi.OP_NOISE
    d.Ops[0].u.Noise = scenes.noise_params(scenes.area(0, (32, 32, 0), (1e4, 1e4, 1e4)), (10.0, 20.0), (30.0, 40.0), 0.5)
    getattr(d.Ops[0].u.Noise, field)[1] = value
    _refused(ctx, rnd, d, "%s.y is" % field)


def _spawn_desc(**kw):
    d = _desc()
    d.SpawnCount = 1
    d.Spawns[0].Kind = abi.SPAWN_INLINE
    d.Spawns[0].ChunkIndex = 0
    d.Spawns[0].Params = scenes.spawn_params(CS, 0, 99, 5, (12.0, 34.0), additional_positions=((1, 2, 3), (4, 5, 6)), **kw)
    return d


def test_spawner_offset_outside_the_exact_wrap_is_refused(ctx, rnd):
    d = _spawn_desc()
    d.Spawns[0].Params.RandomnessOffset[0] = -1e30
    _refused(ctx, rnd, d, "RandomnessOffset.x is")


@pytest.mark.parametrize("w", [-1.0, 3.0, 1.5, math.nan, math.inf])
def test_spawner_position_index_offset_is_refused(ctx, rnd, w):
    d = _spawn_desc()
    d.Spawns[0].Params.ChunkSizeAndIndices[3] = w
    _refused(ctx, rnd, d, "ChunkSizeAndIndices.w")


def test_spawner_polygon_rate_not_finite_is_refused(ctx, rnd):
    d = _spawn_desc(polygon_rate=2.0)
    d.Spawns[0].Params.PolygonRate = math.inf
    _refused(ctx, rnd, d, "PolygonRate")


def test_spawner_fractional_position_count_is_refused(ctx, rnd):
    d = _spawn_desc()
    d.Spawns[0].Params.PositionConstantCount = 2.5
    _refused(ctx, rnd, d, "is not an integer")


def test_polygon_spawner_fractional_index_offset_is_accepted(ctx, rnd):
    """(TotalSpawned / rate) % count is a fraction in the reference: the polygon form keeps accepting it."""
    eng, sysm = make_system(ctx, rnd, CS)
    try:
        d = _spawn_desc(polygon_rate=3.0)
        d.Spawns[0].Params.ChunkSizeAndIndices[3] = 1.75
        sysm.step(d)
    finally:
        sysm.close(); eng.close()


# ---- the light ramp: SampleFromRamp2 (LINEAR, U CLAMP, V WRAP) at RampOffset across the tap matrix ------------------------------

LW, LH = 32, 24


def _light_ramp():
    """(5, 7) ramp: r = b = 1, g = (row + 1) / 8, so a lit pixel's g / r names the row it sampled (the U blend keeps g within a row)."""
    t = np.ones((RAMP_H, RAMP_W, 4), np.float32)
    t[..., 1] = ((np.arange(RAMP_H) + 1) / 8.0)[:, None]
    return t


def _light(offset):
    lights = (abi.LightVertex * 1)()
    lights[0] = scenes.sphere_light((16.0, 12.0, 10.0), 4.0, 30.0, color=(1, 1, 1, 1), casts_shadows=False, have_distance_field=False,
                                    )
    e = lights[0].EvenMoreLightProperties
    lights[0].EvenMoreLightProperties = abi.f4(e.x, e.y, float(offset), 1.0)     # the shader's rampOffset / rampRate themselves
    return lights


def _same_or_close(got, want, what):
    """NaN exactly where the oracle has NaN; the rest within the suite's float criterion (atan2 may differ by an ulp)."""
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), "%s: NaN at %d places, the oracle at %d" % (what, int(nan_g.sum()), int(nan_w.sum()))
    scale = float(np.abs(want[~nan_w]).max()) if (~nan_w).any() else 1.0
    np.testing.assert_allclose(got[~nan_g], want[~nan_w], rtol=1e-4, atol=1e-5 * max(scale, 1e-30), err_msg=what)


RAMP_OFFSETS = [F32(t) / F32(RAMP_H) for t in lookup_tap_matrix(RAMP_H)]


@pytest.mark.parametrize("offset", RAMP_OFFSETS, ids=["%r" % float(o) for o in RAMP_OFFSETS])
def test_light_ramp_wraps_v_at_every_ramp_offset(ctx, oracle, offset):
    """v = (angle + RampOffset) * RampRate: the culled and the instrumented light pass give the same bits, both the oracle's frame, and
    where RampOffset absorbs the angle (|offset| >= 2^26) every lit pixel's row is the exact WRAP of floor(offset * h - 0.5).  Light
    probes with the same ramp give the oracle's values."""
    env = scenes.environment()
    dfu = lc_no_field()
    lights = _light(offset)
    ramp = _light_ramp()
    frames = []
    ctx.set_light_ramp(ramp)
    try:
        for stats in (False, True):
            lm = native.Lightmap(ctx, LW, LH, abi.LIGHTMAP_FLOAT4)
            native.render_sphere_lights(ctx, lights, env, dfu, None, None, (0.0, 0.0, 0.0, 0.0), lm, want_stats=stats)
            frames.append(lm.download())
            lm.close()
        pp = np.array([[16.0 + 3.0 * math.cos(a), 12.0 + 3.0 * math.sin(a), 0.0, 0.0] for a in np.linspace(0.1, 6.2, 16)], np.float32)
        pn = np.tile(np.array([0.0, 0.0, 1.0, 0.0], np.float32), (len(pp), 1))
        probes = native.render_light_probes(ctx, lights, pp, pn, env, dfu, None)
    finally:
        ctx.set_light_ramp(None)
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32)), "culled and instrumented light passes differ"
    oracle.set_light_ramp(ramp)
    try:
        want, _ = oracle.render_sphere_lights(lights, env, dfu, None, None, (0.0, 0.0, 0.0, 0.0), LW, LH)
        want_probes = oracle.render_light_probes(lights, pp, pn, env, dfu, None)
    finally:
        oracle.set_light_ramp(None)
    _same_or_close(frames[0], want, "light frame, RampOffset %r" % float(offset))
    _same_or_close(probes, want_probes, "light probes, RampOffset %r" % float(offset))
    if math.isfinite(offset) and abs(offset) >= 2.0 ** 26:
        with np.errstate(all="ignore"):
            sy = float(F32(F32(F32(offset) * F32(RAMP_H)) - F32(0.5)))
        row = _wrap(_floor(sy), RAMP_H)
        lit = frames[0][..., 0] > 1e-3
        assert lit.sum() > 10
        rows = np.rint(8.0 * frames[0][lit][:, 1] / frames[0][lit][:, 0]).astype(np.int64) - 1
        assert np.all(rows == row), "rows sampled %s, the exact WRAP is %d" % (sorted(set(rows.tolist())), row)


def lc_no_field():
    from tests.lights_common import no_field_uniforms
    return no_field_uniforms()


# ---- SpatialNoise: smoothRandomCustom (LINEAR WRAP) at particle positions across the tap matrix ----------------------------------

def _spatial_noise_desc():
    d = _desc()
    d.System = scenes.system_uniforms(CS, friction=0.0, max_velocity=1e30, life_decay=0.0)
    d.OpCount = 1
    d.Ops[0].Type = abi.OP_SPATIAL_NOISE
    noise = scenes.noise_params(scenes.area_none(1.0), (0.0, 0.0), (0.0, 0.0), 0.0, 10.0, True,
                                position=((0.0,) * 4, (0,) * 4, (0.0, 0.0, 0.0, 0.0)), velocity=((0.0,) * 3, (0,) * 3, (1.0, 1.0, 1.0)),
                                speed=(0.0, 0.0, 1.0))
    d.Ops[0].u.SpatialNoise = scenes.spatial_noise_params(noise, (1.0, 1.0))
    return d


def _spatial_noise_state(rw, rh):
    """x over the tap matrix (one column per entry), y over it too (one row per entry): every pair once, all alive."""
    xs = [float(t) for t in lookup_tap_matrix(rw)]
    ys = [float(t) for t in lookup_tap_matrix(rh)]
    n = CS * CS
    pos = np.zeros((n, 4), np.float32)
    for i in range(n):
        pos[i, 0], pos[i, 1] = xs[i % len(xs)], ys[(i // len(xs)) % len(ys)]
    pos[:, 3] = 1.0
    vel = np.zeros((n, 4), np.float32)
    vel[:, :3] = 1.0
    return pos, vel, np.ones((n, 4), np.float32)


def test_spatial_noise_wraps_every_position(ctx, oracle):
    """SpatialNoise reads the randomness table at particle positions (state, never refused) from 0 and denormals to +-FLT_MAX, +-inf
    and NaN: the default step and the interpreting step give the same bits, and both the oracle's values (tests/test_oracle_kat.py
    holds the oracle's taps to the exact WRAP)."""
    rnd = scenes.randomness_table(4)
    rh, rw = rnd.shape[:2]
    d = _spatial_noise_desc()
    pos, vel, attr = _spatial_noise_state(rw, rh)
    outs = []
    for interpreter in (0, 1):
        eng, sysm = make_system(ctx, rnd, CS)
        prev = native.lib().ilm_debug_step_interpreter(interpreter)
        try:
            upload_state(sysm, 0, pos, vel, attr)
            sysm.step(d)
            outs.append(download_state(sysm, 0))
        finally:
            native.lib().ilm_debug_step_interpreter(prev)
            sysm.close(); eng.close()
    for k in (0, 1):
        assert np.array_equal(outs[0][k].view(np.uint32), outs[1][k].view(np.uint32)), "plane %d: default step and interpreter differ" % k
    chunk = [pos.copy(), vel.copy(), attr.copy(), np.zeros_like(pos), np.zeros_like(pos)]
    oracle.step([chunk], CS, rnd, d)
    # The op around the lookup (area weight, time scale, lerp) is held to the suite's 1e-4 criterion, not to bits (as in
    # tests/test_transforms_gpu.py); a wrong texel of this table moves a component by far more than that.
    for k, name in ((0, "position"), (1, "velocity")):
        got, want = outs[0][k].astype(np.float64), chunk[k].astype(np.float64)
        with np.errstate(all="ignore"):
            same = (got == want) | (np.isnan(got) & np.isnan(want)) | (np.abs(got - want) <= 1e-4 * np.abs(want) + 1e-6)
        assert same.all(), "%s differs from the oracle at %d slots, e.g. %s" % (
            name, int((~same).any(axis=1).sum()), [(pos[i, :2].tolist(), got[i].tolist(), want[i].tolist()) for i in np.nonzero(~same.all(axis=1))[0][:3]])
    assert (outs[0][1][:, :3] != vel[:, :3]).any(axis=1).sum() > CS * CS // 2       # the op did replace the velocities


# ---- the distance-field U WRAP of an atlas whose width is not a power of two, at tap columns from 2^22 on --------------------------

def test_distance_field_u_wrap_is_exact_from_2_22_on(ctx, oracle):
    """ilm_sdf_sample on a 13-wide atlas (the wrap is a true division) at tap columns spread over [2^21, 2^32) and at their fp32
    neighbours: the oracle's bits (which tests/test_oracle_kat.py holds to the float64 WRAP)."""
    from tests.test_oracle_kat import _sampler_kat_field, _sampler_kat_uniforms
    atlas, _ = _sampler_kat_field()
    rng = np.random.default_rng(29)
    cols = np.concatenate([2.0 ** rng.uniform(21.0, 32.0, 3000), [2.0 ** e + k for e in (22, 23, 24, 31) for k in (-3, -1, 0, 1, 2, 5)]])
    us = (cols + 0.5) / 13.0 + rng.uniform(-0.2, 0.2, cols.shape) / 13.0
    pos = np.stack([us, rng.uniform(0.0, 1.0, cols.shape), np.zeros_like(us)], axis=1).astype(np.float32)
    dfu = _sampler_kat_uniforms(1.0, 1.0)
    sdf = native.DistanceFieldTexture(ctx, np.ascontiguousarray(atlas), abi.SDF_UNORM16)
    try:
        got = sdf.sample(dfu, pos)
    finally:
        sdf.close()
    tex = oracle.make_texture(np.ascontiguousarray(atlas), abi.SDF_UNORM16)
    want = np.array([oracle.sample_distance_field(tuple(map(float, p)), dfu, tex) for p in pos], np.float32)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, "%d of %d samples differ, e.g. u = %s" % (bad.size, len(pos), pos[bad[:4], 0].tolist())
