"""step_lean_clamp_kernel has two bodies (csrc/particles.hip, step_lean_block).  A wave whose 64 slots are all regular -- alive with a
finite life, a category every transform's filter accepts, no NaN in the velocity's x and y, before the step and after it -- runs the
transforms, the update and the store elision without the tests and selects that serve other lanes; every other wave runs the selecting
body, from the top or from the update on.  Either way the planes must hold the bits the interpreting kernel leaves.  Each case steps a
system by the default choice and a twin by the interpreter (ilm_debug_step_interpreter) five times, so that the class runs from the second
step on, compares every plane of every chunk bit for bit and the live counts, and holds ilm_debug_step_regular_waves to the number of waves
that must have taken each way in each step.

The shape: chunk size 64 (one wave per row, 64 waves per chunk), two chunks, Gravity with four attractors (linear and squared) + Noise +
UpdatePositions, OpacityFromLife as the one clamp-linear curve.  ILM_STEP_STREAMING=1 selects the HBM-resident variant for so small a system.
"""
import numpy as np
import pytest

from tests.step_regular_common import (CountingTwins, desc, regular_particles, slot, PLACES, K, LEAN, LEAN_CLAMP, N, CHUNKS, STEPS, WAVES, NAN, INF, DECAY)
from tests.test_step_store_elision_gpu import update_params, V

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def streaming_variant(monkeypatch):
    monkeypatch.setenv("ILM_STEP_STREAMING", "1")


def run(ctx, what, particles, d, want_waves, also=None):
    """STEPS steps of d; want_waves: (regular, selected) of steps 2 .. STEPS, the class's (the first step of a system stores everything
    through the general instantiation, which has one body and counts nothing)."""
    t = CountingTwins(ctx, *particles)
    try:
        t.step(d, STEPS)
        t.check(what)
        assert t.kernels == [LEAN] + [LEAN_CLAMP] * (STEPS - 1), (what, t.kernels)
        assert t.waves == [(0, 0)] + list(want_waves), (what, t.waves)
        t.check_waves(what)               # ... and what the kernel's two masks give over the twin's planes (lists without FMA)
        if also is not None:
            also(t)
    finally:
        t.close()
    return t


def test_all_regular(ctx):
    t = run(ctx, "all regular", regular_particles(), desc(), [(WAVES, 0)] * 4)
    assert all(np.array_equal(c, [N] * CHUNKS) for c in t.counts[0])


def _dead(pos, vel, i):
    pos[i, 3] = 0.0


def _life(value):
    def fn(pos, vel, i):
        pos[i, 3] = value
    return fn


def _category(value):
    def fn(pos, vel, i):
        vel[i, 3] = value
    return fn


def _velocity(x, y, z):
    def fn(pos, vel, i):
        vel[i, :3] = (x, y, z)
    return fn


ALWAYS = [(WAVES - K, 0)] * 4            # the waves with such a lane run the selecting body from the top in every step of the class
NEVER = [(WAVES, 0)] * 4                 # the lane is regular
# kind -> (what it does to a slot, (regular, selected) waves of steps 2 .. 5[, the transforms where they are not Gravity + Noise])
KINDS = {
    "dead at load": (_dead, ALWAYS),
    # 2 x decay: one decay left after the first step, exactly 0 after the class's first: regular as loaded, its life runs out in the update
    "life that runs out in this step": (_life(np.float32(2.0) * DECAY), [(WAVES - K, K)] + [(WAVES - K, 0)] * 3),
    # just above 2 x decay: survives the class's first step by a hair (a regular wave throughout), runs out in its second
    "life that runs out in the third step": (_life(np.float32(2.0) * DECAY * np.float32(1.0 + 2.0 ** -18)), [(WAVES, 0), (WAVES - K, K)] + [(WAVES - K, 0)] * 2),
    "NaN life": (_life(NAN), ALWAYS),
    "infinite life": (_life(INF), ALWAYS),
    "category outside Gravity's filter only": (_category(-0.5), ALWAYS),
    "category outside Noise's filter only": (_category(1.0), ALWAYS),
    "NaN category": (_category(NAN), ALWAYS),
    # Gravity's clamped add (min(MaximumVelocity, NaN) = MaximumVelocity) turns a NaN component into the maximum in the first step, which
    # is the general instantiation's: under the standard list the lane is regular by the time the class runs.  Noise alone keeps the NaN.
    "NaN velocity x": (lambda pos, vel, i: vel.__setitem__((i, 0), NAN), NEVER),
    "NaN velocity x, Noise alone": (lambda pos, vel, i: vel.__setitem__((i, 0), NAN), ALWAYS, ("noise",)),
    "speed at most 0.001": (_velocity(2e-4, -3e-4, 1e-4), NEVER),
    "speed above MaximumVelocity": (_velocity(300.0, -200.0, 10.0), NEVER),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_one_irregular_lane_per_wave(ctx, kind):
    change, want = KINDS[kind][:2]
    ops = KINDS[kind][2] if len(KINDS[kind]) > 2 else ("gravity", "noise")
    pos, vel, attr = regular_particles()
    for place in PLACES:
        change(pos, vel, slot(place))
    run(ctx, kind, (pos, vel, attr), desc(ops=ops), want)


def test_a_wholly_dead_wave_and_a_wholly_dead_chunk(ctx):
    pos, vel, attr = regular_particles()
    pos[N:, 3] = 0.0                              # chunk 1
    pos[5 * 64:6 * 64, 3] = 0.0                   # wave 5 of chunk 0
    t = run(ctx, "dead wave, dead chunk", (pos, vel, attr), desc(), [(63, 0)] * 4)
    assert all(np.array_equal(c, [N - 64, 0]) for c in t.counts[0])


@pytest.mark.parametrize("ops", [("noise", "gravity"), ("gravity",), ()], ids=["noise gravity", "gravity alone", "no transform"])
def test_transform_orders(ctx, ops):
    """Other lists, each with a dead lane, a filtered one (where there is a filter) and a NaN velocity next to the regular waves; without a
    transform the friction's own cases (speed <= 0.001, speed above the maximum) meet the update untouched and any category but NaN passes."""
    pos, vel, attr = regular_particles()
    _dead(pos, vel, slot(PLACES[0]))
    _category(NAN if not ops else 7.0)(pos, vel, slot(PLACES[1]))
    vel[slot(PLACES[2]), 1] = NAN
    for k in range(64):                          # wave 9 of chunk 0 stays regular
        vel[9 * 64 + k, :3] = (2e-4, 0.0, 1e-4) if k % 2 else (300.0, 150.0 + k, -20.0)
    vel[10 * 64 + 7, 3] = 7.0 if not ops else 0.0          # without a filter to fail, category 7 is regular
    # (Gravity's clamped add replaces the NaN in the first step, the general instantiation's: see KINDS)
    irregular = 2 if "gravity" in ops else 3
    run(ctx, "ops %s" % (ops,), (pos, vel, attr), desc(ops=ops), [(WAVES - irregular, 0)] * 4)


def test_rotation_from_life_keeps_both_evaluations(ctx):
    """RotationFromLifeAndIndex[0] != 0: rd.y reads the life, changes with it in every step and must be stored by the regular body too."""
    run(ctx, "rotation from life", regular_particles(), desc(update=update_params(rotation_from_life=0.25, rotation_from_index=0.001)), NEVER)


def test_fma_that_ends_a_life_restarts_the_wave(ctx):
    """FMA is the one transform that can take a life to <= 0 inside the list, and the transforms after it then skip the slot: a regular wave
    where that happens starts again in the selecting body.  Life falls by t = dtMs / TimeDivisor = 1 / 6 per step (plus the decay): a slot
    with 0.4 goes through the class's first step, crosses zero inside its second and is dead from then on."""
    pos, vel, attr = regular_particles()
    for place in PLACES:
        pos[slot(place), 3] = 0.4
    run(ctx, "fma ends a life", (pos, vel, attr), desc(ops=("fma", "gravity"), fma_life_add=-1.0), [(WAVES, 0)] + [(WAVES - K, 0)] * 3)


@pytest.mark.parametrize("multiply,add", [(1.0, 2.4), (0.5, 2.4)], ids=["category add", "category multiply and add"])
def test_fma_that_changes_the_category_restarts_the_wave(ctx, multiply, add):
    """FMA's lerp covers the velocity's w, the category: with t = 1 / 6 and VelocityAdd.w = 2.4 every slot's category rises by about 0.4 a
    step, stays inside Gravity's filter (0 .. 1) for two steps and leaves it in the third.  The selecting body filters Gravity by the new
    category and stores it (plane 7 and rd.w); the regular body takes the category as unchanged, so a wave whose FMA changes one bit of it
    starts again in the selecting body: in these launches that is every wave of every step, and no wave counts as regular."""
    def left_the_filter(t):
        assert t.systems[0].download(0, V)[:, 3].min() > 1.0            # out of Gravity's filter by the end, and stored
    run(ctx, "fma moves the category (%g, %g)" % (multiply, add), regular_particles(), desc(ops=("fma", "gravity"), fma_category=(multiply, add)),
        [(0, 0)] * 4, also=left_the_filter)


@pytest.mark.parametrize("factor", [NAN, INF, -INF], ids=["NaN", "inf", "-inf"])
def test_rotation_from_an_index_factor_that_is_not_finite(ctx, factor):
    """RotationFromLifeAndIndex[1] NaN or infinite with [0] == 0: rd.y is a NaN (or 0 x inf at index 0, then inf elsewhere) for the loaded
    and the new state alike.  The host leaves the rd.y shortcut off for such a factor, the regular body evaluates both states and stores
    a NaN rd.y like the selecting tail does; the waves are regular all the same."""
    run(ctx, "index factor %r" % factor, regular_particles(), desc(update=update_params(rotation_from_index=float(factor))), NEVER)
