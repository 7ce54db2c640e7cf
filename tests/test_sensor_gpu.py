"""Particle sensors on the device, through the C ABI: ilm_system_sense, ilm_system_sense_async and ilm_system_poll_sense against the
numpy statement of PS_CollectParticles (tests/sensor_common.py).  Every case first passes check_case on the CPU -- the band around the
0.01 threshold is empty and the oracle and the second reading give the same mask for every slot -- and then the counts are compared
exactly.

Chunk sizes: 8 (64 slots: a quarter of one wave's 256), 20 (400 slots: a ragged second wave), 24 (576 slots: two waves and a quarter)."""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import sensor_common as sc
from tests import test_step_batch_gpu as sb
from tests.test_sensor_kat import hand_case
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

P, V, A, RC, RD = abi.PLANE_POSITION, abi.PLANE_VELOCITY, abi.PLANE_ATTRIBUTES, abi.PLANE_RENDER_COLOR, abi.PLANE_RENDER_DATA
PLANES = (P, V, A, RC, RD)
F = np.float32


@pytest.fixture(scope="module")
def rnd():
    return scenes.randomness_table(29)


class Device:
    """An engine and a system holding `chunks` ([(pos, vel)]; used[c]: only that many slots of chunk c are uploaded), every plane filled."""

    def __init__(self, ctx, rnd, cs, chunks, used=None):
        self.eng = native.Engine(ctx, cs, rnd)
        self.s = native.System(self.eng)
        for c, (pos, vel) in enumerate(chunks):
            self.s.add_chunk()
            u = pos.shape[0] if used is None else used[c]
            self.s.upload(c, P, pos[:u]); self.s.upload(c, V, vel[:u])
            for k, plane in enumerate((A, RC, RD)):
                self.s.upload(c, plane, scenes.uniform(900 + 10 * c + k, (u, 4), -2.0, 2.0))

    def planes(self):
        return [[self.s.download(c, plane) for plane in PLANES] for c in range(self.s.chunk_count())]

    def close(self):
        self.s.close(); self.eng.close()


def assert_state_unchanged(before, after, what):
    for c, (b, a) in enumerate(zip(before, after)):
        for plane, x, y in zip(PLANES, b, a):
            assert_bits_equal(y, x, "%s: chunk %d plane %d" % (what, c, plane))


# ---- counts --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_chunks", [1, 3])
@pytest.mark.parametrize("cs", [8, 20, 24])
def test_counts_equal_the_numpy_statement(ctx, oracle, rnd, cs, n_chunks):
    """The eight standard sensors -- every area type 0..5 rotated, type 0 with AreaFalloff = 0, a filter that passes nothing, an unrotated
    box -- in one call over all chunks (chunk_count < 0 and the explicit count), over a sub-range, and the five planes before and after."""
    sensors, chunks, want = sc.standard_case(oracle, cs, n_chunks)
    d = Device(ctx, rnd, cs, chunks)
    try:
        before = d.planes()
        got = d.s.sense(sensors)
        assert got.shape == want.shape and np.array_equal(got, want), (got, want)
        assert np.array_equal(d.s.sense(sensors, 0, n_chunks), want)
        assert not got[6].any() and got[0].all()
        if n_chunks == 3:
            assert np.array_equal(d.s.sense(sensors, 1, 2), want[:, 1:3])
            assert np.array_equal(d.s.sense(sensors, 2, 1), want[:, 2:3])
            assert np.array_equal(d.s.sense(sensors[2:5], 0, 2), want[2:5, 0:2])
        assert d.s.sense(sensors, 0, 0).shape == (8, 0)
        assert_state_unchanged(before, d.planes(), "after ilm_system_sense")
    finally:
        d.close()


@pytest.mark.parametrize("type_id", [0, 1, 2, 3, 4, 5])
def test_hand_computed_cases(ctx, oracle, rnd, type_id):
    """The 16 hand-computed slots of tests/test_sensor_kat.py in the first quarter of a 64-slot chunk whose other slots were never written."""
    a, pos, vel, mask = hand_case(type_id)
    assert sc.check_case(oracle, [a], [(pos, vel)]).tolist() == [[int(mask.sum())]]
    d = Device(ctx, rnd, 8, [(pos, vel)], used=[16])
    try:
        assert d.s.sense([a]).tolist() == [[int(mask.sum())]]
    finally:
        d.close()


def test_one_two_and_eight_sensors_in_one_call_equal_single_calls(ctx, oracle, rnd):
    cs, n_chunks = 20, 3
    sensors, chunks, want = sc.standard_case(oracle, cs, n_chunks)
    d = Device(ctx, rnd, cs, chunks)
    try:
        single = np.concatenate([d.s.sense([a]) for a in sensors])
        assert np.array_equal(single, want)
        for group in (sensors[3:4], sensors[4:6], sensors):
            k0 = sensors.index(group[0])
            got = d.s.sense(group)
            assert np.array_equal(got, single[k0:k0 + len(group)]), len(group)
        # a call none of whose sensors has an area runs the instantiation without distance code
        plain = [sc.sensor(0, falloff=0.0), sc.sensor(0, falloff=5.0, category_filter=sc.EVERY_CATEGORY)]
        want_plain = sc.check_case(oracle, plain, chunks)
        assert np.array_equal(d.s.sense(plain), want_plain) and np.array_equal(want_plain[0], want[0]) and (want_plain[1] > want_plain[0]).all()
        # Strength takes no part
        strong = [sc.sensor(2, size=(30.0, 24.0, 12.0), falloff=16.0, rotation=0.5, strength=s) for s in (0.0, -3.0, float("nan"))]
        assert np.array_equal(d.s.sense(strong), np.repeat(want[2:3], 3, axis=0))
    finally:
        d.close()


def test_dead_waves_and_never_written_slots(ctx, oracle, rnd):
    """cs = 24: chunk 0 holds only its first 300 slots (the rest was never written: zeros), chunk 1's second wave (slots 256..511) holds no
    life above one -- the wave leaves before it loads a coordinate -- and its last quarter wave only categories outside the filter."""
    cs, n = 24, 576
    sensors, chunks, _ = sc.standard_case(oracle, cs, 2)
    (p0, v0), (p1, v1) = [(p.copy(), v.copy()) for p, v in chunks]
    p0[300:], v0[300:] = 0, 0
    p1[256:512, 3] = np.minimum(p1[256:512, 3], F(1))
    v1[512:, 3] = F(5)
    modified = [(p0, v0), (p1, v1)]
    want = sc.check_case(oracle, sensors, modified)
    assert (want[:6, 0] > 0).all() and (want[:6, 1] > 0).all()
    d = Device(ctx, rnd, cs, modified, used=[300, n])
    try:
        assert np.array_equal(d.s.sense(sensors), want)
    finally:
        d.close()


# ---- ordering ------------------------------------------------------------------------------------------------------------------------

def test_a_sense_directly_after_a_step_sees_the_stepped_state(ctx, oracle, rnd):
    """ilm_system_step, then ilm_system_sense with no synchronisation in between: the counts are those of the oracle's step of the same
    input.  The band around the threshold is kept empty on the STEPPED positions (the builder's `advance`)."""
    cs, n_chunks = 20, 3
    n = cs * cs
    sensors = sc.standard_sensors()
    desc = sb.base(cs)
    sb.add_op(desc, abi.OP_FMA, scenes.fma_params(scenes.area_none(0.8), position_add=(0.5, -0.25, 0.0), position_multiply=(1.001, 0.999, 1.0),
                                                  velocity_add=(0.0, 1.5, 0.0), velocity_multiply=(0.98, 0.97, 1.0)))
    attr = np.ones((n, 4), F)

    def advance(pos, vel):
        planes = [pos, vel, attr.copy(), np.zeros((n, 4), F), np.zeros((n, 4), F)]
        oracle.step([planes], cs, rnd, desc)
        return planes[0], planes[1]

    chunks = [sc.build_chunk(oracle, 700 + 100 * c, n, sensors, advance=advance) for c in range(n_chunks)]
    stepped = [advance(pos.copy(), vel.copy()) for pos, vel in chunks]
    want = sc.check_case(oracle, sensors, stepped)
    unstepped = np.array([[int(sc.mask(a, p, v, sc.scaled_distance(a, sc.oracle_distance(oracle, a, p))).sum()) for p, v in chunks] for a in sensors])
    assert (want[:6] != unstepped[:6]).any(axis=1).all()          # the step matters to every sensor that counts anything
    eng = native.Engine(ctx, cs, rnd)
    s = native.System(eng)
    try:
        for c, (pos, vel) in enumerate(chunks):
            s.add_chunk()
            s.upload(c, P, pos); s.upload(c, V, vel); s.upload(c, A, attr)
        ctx.sync()
        s.step(desc)
        s.sense_async(sensors)          # the queued form behind the same step
        got = s.sense(sensors)
        ctx.sync()
        assert np.array_equal(s.poll_sense(), got)
        for c, (pos, vel) in enumerate(stepped):
            assert np.array_equal(s.download(c, P)[:, 3] > 1, pos[:, 3] > 1) and np.array_equal(s.download(c, V)[:, 3], vel[:, 3])
        assert np.array_equal(got, want), (got, want)
    finally:
        s.close(); eng.close()


# ---- the queued form -----------------------------------------------------------------------------------------------------------------

def test_async_then_poll(ctx, oracle, rnd):
    """ilm_system_sense_async, ilm_ctx_sync, ilm_system_poll_sense: the blocking form's counts.  A poll before the synchronisation may
    say "not ready" and never blocks; a second queued count replaces the first; a blocking call in between leaves the queued one alone."""
    cs, n_chunks = 24, 3
    sensors, chunks, want = sc.standard_case(oracle, cs, n_chunks)
    d = Device(ctx, rnd, cs, chunks)
    lib = native.lib()
    try:
        out = np.zeros(64, np.uint32)
        ready = C.c_int32(5)
        assert lib.ilm_system_poll_sense(d.s.handle, out.ctypes.data, 64, C.byref(ready)) == abi.ERR_STATE and ready.value == 0
        before = d.planes()
        d.s.sense_async(sensors)
        early = d.s.poll_sense()
        assert early is None or np.array_equal(early, want)
        if early is None:
            ctx.sync()
            assert np.array_equal(d.s.poll_sense(), want)
        assert lib.ilm_system_poll_sense(d.s.handle, out.ctypes.data, 64, C.byref(ready)) == abi.ERR_STATE      # delivered once
        # a second queued count replaces the first
        d.s.sense_async(sensors)
        d.s.sense_async(sensors[1:3], 1, 2)
        assert np.array_equal(d.s.sense(sensors[4:5]), want[4:5])          # a blocking call in between
        ctx.sync()
        assert np.array_equal(d.s.poll_sense(), want[1:3, 1:3])
        assert_state_unchanged(before, d.planes(), "after the queued counts")
    finally:
        d.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def bad_sensors():
    """(what, sensors) for every refusal that concerns an IlmAreaParams: the second of two sensors is the bad one."""
    good = sc.standard_sensors()[2]
    out = []
    for what, change in (("AreaType -1", lambda a: setattr(a, "AreaType", -1)), ("AreaType 6", lambda a: setattr(a, "AreaType", 6)),
                         ("AreaRotation NaN", lambda a: setattr(a, "AreaRotation", float("nan"))),
                         ("AreaFalloff inf", lambda a: setattr(a, "AreaFalloff", float("inf"))),
                         ("AreaFalloff NaN", lambda a: setattr(a, "AreaFalloff", float("nan"))),
                         ("AreaCenter.y NaN", lambda a: a.AreaCenter.__setitem__(1, float("nan"))),
                         ("AreaCenter.z -inf", lambda a: a.AreaCenter.__setitem__(2, float("-inf"))),
                         ("AreaSize.x inf", lambda a: a.AreaSize.__setitem__(0, float("inf"))),
                         ("AreaSize.z NaN", lambda a: a.AreaSize.__setitem__(2, float("nan")))):
        bad = sc.standard_sensors()[2]
        change(bad)
        packed = (abi.AreaParams * 2)(good, bad)
        out.append((what, packed))
    return out


def test_refusals_leave_counts_and_state_untouched(ctx, oracle, rnd):
    cs, n_chunks = 20, 3
    sensors, chunks, want = sc.standard_case(oracle, cs, n_chunks)
    d = Device(ctx, rnd, cs, chunks)
    lib = native.lib()
    h = d.s.handle
    try:
        before = d.planes()
        two = (abi.AreaParams * 2)(sensors[1], sensors[2])
        nine = (abi.AreaParams * 9)(*([sensors[1]] * 9))
        p2, p9 = C.cast(two, C.c_void_p), C.cast(nine, C.c_void_p)
        SENTINEL = 0xABCD1234
        out = np.full(64, SENTINEL, np.uint32)
        po = out.ctypes.data
        # (what, first_chunk, chunk_count, sensors, sensor_count, out, capacity)
        cases = [("sensors NULL", 0, -1, None, 2, po, 64), ("out_counts NULL", 0, -1, p2, 2, None, 64),
                 ("sensor_count 0", 0, -1, p2, 0, po, 64), ("sensor_count -1", 0, -1, p2, -1, po, 64), ("sensor_count 9", 0, -1, p9, 9, po, 64),
                 ("first_chunk -1", -1, 1, p2, 2, po, 64), ("range past the end", 0, 4, p2, 2, po, 64), ("first_chunk at the end", 3, 1, p2, 2, po, 64),
                 ("range past the end from the middle", 2, 2, p2, 2, po, 64), ("a huge count", 1, 2**31 - 1, p2, 2, po, 64),
                 ("capacity one short", 0, -1, p2, 2, po, 5), ("capacity 0", 0, 3, p2, 2, po, 0), ("capacity negative", 0, 1, p2, 2, po, -1)]
        bad = bad_sensors()
        cases += [(what, 0, -1, C.cast(packed, C.c_void_p), 2, po, 64) for what, packed in bad]
        # a valid count is queued first: no refusal may replace or deliver it
        d.s.sense_async(sensors[:2])
        for what, first, count, ps, n, o, capacity in cases:
            assert lib.ilm_system_sense(h, first, count, ps, n, o, capacity) == abi.ERR_INVALID_ARGUMENT, what
            assert lib.ilm_last_error(), what
            assert (out == SENTINEL).all(), what
            if "out_counts" not in what and "capacity" not in what:
                assert lib.ilm_system_sense_async(h, first, count, ps, n) == abi.ERR_INVALID_ARGUMENT, what
        ready = C.c_int32(7)
        assert lib.ilm_system_poll_sense(h, None, 64, C.byref(ready)) == abi.ERR_INVALID_ARGUMENT and ready.value == 7
        assert lib.ilm_system_poll_sense(h, po, 64, None) == abi.ERR_INVALID_ARGUMENT
        ctx.sync()
        assert lib.ilm_system_poll_sense(h, po, 2 * n_chunks - 1, C.byref(ready)) == abi.ERR_INVALID_ARGUMENT and ready.value == 0
        assert (out == SENTINEL).all()
        # the queued count is still there, and is the one queued before the refusals
        assert np.array_equal(d.s.poll_sense(), want[:2])
        assert np.array_equal(d.s.sense(sensors), want)
        assert_state_unchanged(before, d.planes(), "after the refusals")
        # the bounds themselves are accepted: eight sensors, the last chunk alone, an empty range, the exact capacity
        exact = np.full(2 * n_chunks, SENTINEL, np.uint32)
        assert lib.ilm_system_sense(h, 0, -1, p2, 2, exact.ctypes.data, 2 * n_chunks) == abi.OK
        assert np.array_equal(exact.reshape(2, n_chunks), want[1:3])
        assert lib.ilm_system_sense(h, 3, 0, p2, 2, po, 0) == abi.OK and (out == SENTINEL).all()
    finally:
        d.close()
