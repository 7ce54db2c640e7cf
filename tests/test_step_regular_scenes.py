"""The scenes of tests/test_step_regular_body_gpu.py mean something only if they do what they claim: that every wave stays regular, that
some lanes of every wave move a curve's t while others keep it, that exactly one lane does.  Here each scene is stepped through the CPU oracle
and held to its claim by the numpy statement of the kernel's masks (tests/step_regular_common.py, predict_waves), and that statement and the
category-bound rule are pinned on hand-made planes.  No GPU: the device tests predict from the interpreter twin's own bits and stay exact; the
oracle and the device agree to 1e-4 relative, which is why the scenes keep their lives 1 % away from every edge a claim rests on.
"""
import numpy as np
import pytest

from tests import step_regular_common as S
from tests.step_regular_common import NAN, INF, STEPS, predict_waves, category_bounds, desc

ALL = dict(S.SCENES_A)
ALL.update(S.SCENES_C)
ALL.update(S.SCENES_F)


def class_steps(s, states):
    """(descriptor, before, after) of steps 2 .. STEPS -- the class's -- over the chunks the step walks."""
    for k in range(1, STEPS):
        d = s.descs[k]
        sl = S.chunk_slice(d, s)
        yield d, (states[k][0][sl], states[k][1][sl]), (states[k + 1][0][sl], states[k + 1][1][sl])


@pytest.mark.parametrize("name", list(ALL))
def test_a_scene_does_what_it_claims(oracle, name):
    s = ALL[name]()
    states = S.oracle_states(oracle, s)
    steps = list(class_steps(s, states))
    got = [predict_waves(before, after, *category_bounds(d)) for d, before, after in steps]
    if s.want is not None:
        assert got == list(s.want), (name, got)
    if s.claims.get("all_regular"):
        waves = steps[0][1][0].shape[0] // 64
        assert got == [(waves, 0)] * (STEPS - 1), (name, got)
    for curve in s.claims.get("curves", ()):
        rc = getattr(s.descs[1].Update, curve).RangeAndCount
        for k, (d, before, after) in enumerate(steps):
            moved = (S.clamp_t(rc, S.curve_input(curve, before)) != S.clamp_t(rc, S.curve_input(curve, after))).reshape(-1, 64)
            assert moved.any(axis=1).all(), "%s: step %d, %s: a wave in which no lane moves its t" % (name, k + 2, curve)
            assert (~moved).any(axis=1).all(), "%s: step %d, %s: a wave in which no lane keeps its t" % (name, k + 2, curve)
    if "one_lane" in s.claims:
        want = np.zeros(steps[0][1][0].shape[0], bool)
        want[[S.slot(place) for place in S.PLACES]] = True
        for curve in s.claims["one_lane"]:
            rc = getattr(s.descs[1].Update, curve).RangeAndCount
            for k, (d, before, after) in enumerate(steps):
                moved = S.clamp_t(rc, S.curve_input(curve, before)) != S.clamp_t(rc, S.curve_input(curve, after))
                assert np.array_equal(moved, want), "%s: step %d, %s: lanes %s move their t" % (name, k + 2, curve, np.flatnonzero(moved))
    if "rest" in s.claims and s.claims["rest"]:
        # the unit the used slots end in holds live lanes next to never-written ones: alive, so walked, and not regular
        last = (s.used[1] // 64) * 64 + s.cs * s.cs
        life = steps[0][1][0][last:last + 64, 3]
        assert (life > 0).sum() == s.claims["rest"] and (life == 0).sum() == 64 - s.claims["rest"]


@pytest.mark.parametrize("seed", S.SWEEP_SEEDS)
def test_every_sweep_seed_keeps_most_waves_regular(oracle, seed):
    s = S.sweep_scene(seed)
    states = S.oracle_states(oracle, s)
    for k, (d, before, after) in enumerate(class_steps(s, states)):
        regular, selected = predict_waves(before, after, *category_bounds(d))
        assert regular >= s.claims["min_regular"] * S.WAVES, "seed %d: step %d keeps %d of %d waves regular" % (seed, k + 2, regular, S.WAVES)


def test_the_sweep_varies_what_it_says_it_varies():
    seeds = [S.sweep_scene(seed) for seed in S.SWEEP_SEEDS]
    orders = {tuple(s.descs[1].Ops[o].Type for o in range(2)) for s in seeds}
    assert len(orders) == 2
    for curve in ("ColorFromLife", "ColorFromVelocity", "SizeFromLife", "SizeFromVelocity"):
        counts = {getattr(s.descs[1].Update, curve).RangeAndCount.z for s in seeds}
        assert 1.0 in counts and len(counts) > 1, (curve, counts)
    assert any(getattr(s.descs[1].Update, c).RangeAndCount.y < 0 for s in seeds for c in ("ColorFromLife", "ColorFromVelocity", "SizeFromLife", "SizeFromVelocity"))


def test_places_scale_to_every_unit_of_a_row():
    assert S.places_for(64) == tuple((0, wave, lane) for _, wave, lane in S.PLACES)
    for cs in (128, 256):
        places = S.places_for(cs)
        per_row = cs // 64
        assert {wave % per_row for _, wave, _ in places} == set(range(min(per_row, len(places))))
        assert all(0 <= wave < cs * cs // 64 for _, wave, _ in places) and [lane for _, _, lane in places] == [lane for _, _, lane in S.PLACES]


# ---- predict_waves and the category bounds on hand-made planes ------------------------------------------------------------------

def planes(waves=3):
    """Every lane regular: life 5, velocity (1, 2, 3), category 0."""
    pos = np.zeros((waves * 64, 4), np.float32); vel = np.zeros((waves * 64, 4), np.float32)
    pos[:, :3] = (10.0, 20.0, 30.0); pos[:, 3] = 5.0
    vel[:, :3] = (1.0, 2.0, 3.0)
    return pos, vel


def changed(state, plane, lane, component, value):
    out = (state[0].copy(), state[1].copy())
    out[plane][lane, component] = value
    return out


LIFE, VX, VY, VZ, CT, PX = (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (0, 0)
# what a lane of wave 1 holds before the step -> whether the first mask still passes it, under bounds 0 .. 0.5
LOADED = [
    (LIFE, 0.0, False), (LIFE, -0.0, False), (LIFE, -1.0, False), (LIFE, NAN, False), (LIFE, INF, False), (LIFE, np.float32(1e-45), True), (LIFE, np.float32(3e38), True),
    (CT, 0.0, True), (CT, -0.0, True), (CT, 0.5, True), (CT, np.nextafter(np.float32(0.5), np.float32(1)), False), (CT, np.float32(-1e-45), False), (CT, NAN, False),
    (CT, INF, False), (CT, -INF, False),
    (VX, NAN, False), (VY, NAN, False), (VX, INF, True), (VY, -INF, True),
    # what neither mask looks at
    (VZ, NAN, True), (VZ, INF, True), (PX, NAN, True), (PX, INF, True),
]


@pytest.mark.parametrize("where,value,passes", LOADED, ids=["%s=%r" % (w, float(v)) for w, v, _ in LOADED])
def test_each_term_of_the_first_mask(where, value, passes):
    base = planes()
    before = changed(base, where[0], 64 + 17, where[1], value)
    assert predict_waves(before, base, 0.0, 0.5) == ((3, 0) if passes else (2, 0))


UPDATED = [(LIFE, 0.0, False), (LIFE, -0.0, False), (LIFE, NAN, False), (LIFE, INF, False), (LIFE, -3.0, False), (LIFE, np.float32(1e-45), True),
           (VX, NAN, False), (VY, NAN, False), (VX, -INF, True), (VZ, NAN, True), (CT, NAN, True), (CT, 7.0, True), (PX, NAN, True)]


@pytest.mark.parametrize("where,value,passes", UPDATED, ids=["%s=%r" % (w, float(v)) for w, v, _ in UPDATED])
def test_each_term_of_the_second_mask(where, value, passes):
    """The second mask has no category term: a wave that passes the first and fails the second is `selected`."""
    base = planes()
    after = changed(base, where[0], 2 * 64 + 63, where[1], value)
    assert predict_waves(base, after, 0.0, 0.5) == ((3, 0) if passes else (2, 1))


def test_a_wave_that_fails_the_first_mask_is_neither():
    base = planes()
    before = changed(base, 0, 5, 3, 0.0)
    after = changed(base, 0, 5, 3, NAN)           # ... whatever the second mask would say
    assert predict_waves(before, after, 0.0, 0.5) == (2, 0)
    after = changed(after, 0, 64, 3, 0.0)
    assert predict_waves(before, after, 0.0, 0.5) == (1, 1)


def test_bounds_that_admit_nothing_or_everything():
    base = planes()
    assert predict_waves(base, base, NAN, 0.5) == (0, 0)
    assert predict_waves(base, base, 0.0, NAN) == (0, 0)
    assert predict_waves(base, base, 0.6, 0.5) == (0, 0)
    assert predict_waves(base, base, -0.0, 0.0) == (3, 0)
    wide = changed(changed(base, 1, 3, 3, INF), 1, 70, 3, -INF)
    assert predict_waves(wide, wide, -INF, INF) == (3, 0)
    assert predict_waves(changed(wide, 1, 130, 3, NAN), wide, -INF, INF) == (2, 0)


def bits(x):
    return np.float32(x).view(np.uint32)


def test_the_category_bounds_follow_the_host_rule():
    def bounds(*ops):
        return category_bounds(desc(ops))
    assert bounds() == (-INF, INF)                                                             # no transform: any category but NaN
    assert bounds("gravity", "noise") == (np.float32(0.0), np.float32(0.5))
    assert bounds("noise", "gravity") == (np.float32(0.0), np.float32(0.5))
    assert bounds("fma", "gravity") == (np.float32(0.0), np.float32(1.0))
    assert bounds(("gravity", dict(filter=(0.6, 1.0))), "noise") == (np.float32(0.6), np.float32(0.5))      # empty, and stated as it is
    assert bounds(("gravity", dict(filter=(-2.0, 2.0))), "noise", ("gravity", dict(filter=(-0.25, 1.0)))) == (np.float32(-0.25), np.float32(0.5))
    assert bounds(("gravity", dict(filter=(-INF, INF))), ("noise", dict(filter=(-INF, INF)))) == (-INF, INF)
    # a filter bound is compared in float32, as the kernel holds it
    assert bounds(("gravity", dict(filter=(0.1, 1.0))))[0] == np.float32(0.1)
    # -0.0 against 0.0: the rule keeps the bound it has when the new one is not greater; either zero admits both zeros
    lo, hi = bounds(("gravity", dict(filter=(-0.0, 0.0))), ("noise", dict(filter=(0.0, -0.0))))
    assert lo == 0.0 and hi == 0.0 and bits(lo) == bits(-0.0) and bits(hi) == bits(0.0)
    for ops in ((("gravity", dict(filter=(float("nan"), 1.0))), "noise"), ("gravity", ("noise", dict(filter=(float("nan"), 0.5)))),
                (("gravity", dict(filter=(0.0, float("nan")))), "noise"), ("noise", "fma", ("gravity", dict(filter=(0.0, float("nan")))))):
        lo, hi = bounds(*ops)
        assert np.isnan(lo), ops                                                               # a NaN lower bound admits no category
        assert predict_waves(planes(), planes(), lo, hi) == (0, 0)
