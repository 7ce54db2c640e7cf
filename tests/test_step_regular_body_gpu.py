"""The select-free body of step_lean_clamp_kernel (csrc/particles.hip, step_lean_block's kBodyRegular and its tail,
store_changed_render_planes_regular) held to the interpreting kernel where tests/test_step_regular_waves_gpu.py does not reach: the tail's
four curves with t moving in some lanes and clamped in others, the colour branch, plane 16 and its NaN test, chunk sizes with two and four
units per row and partly used chunks, FMA behind other transforms, the inclusive category bounds, and the values the regular mask does not
look at -- velocity z, the position, the attributes.

Every case runs five steps of the default choice and of a twin stepped by the interpreter (ilm_debug_step_interpreter), compares all five
planes of every chunk bit for bit and the live counts, pins the kernels ([LEAN] + [LEAN_CLAMP] x 4 unless the case says otherwise) and holds
ilm_debug_step_regular_waves to what the kernel's two masks give over the twin's planes before and after each step
(tests/step_regular_common.py, predict_waves) -- and, for lists with FMA, to counts stated by hand.  The scenes themselves are checked on
the CPU by tests/test_step_regular_scenes.py.  ILM_STEP_STREAMING=1 selects the HBM-resident variant for so small a system.
"""
import numpy as np
import pytest

from illuminant_amd import abi, scenes
from tests import step_regular_common as S
from tests.step_regular_common import (CountingTwins, desc, regular_particles, slot, scene, PLACES, K, LEAN, LEAN_CLAMP, N, STEPS, WAVES, NAN, INF,
                                       all_regular, with_places)
from tests.test_step_lean_classes_gpu import curve1, curve4
from tests.test_step_store_elision_gpu import WRITERS, update_params, PLANES, P, V, A
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

CLASS = [LEAN] + [LEAN_CLAMP] * (STEPS - 1)


@pytest.fixture(autouse=True)
def streaming_variant(monkeypatch):
    monkeypatch.setenv("ILM_STEP_STREAMING", "1")


def run(ctx, what, s, kernels=CLASS, want=None, between=None, also=None):
    """The scene's steps on both twins; `want`: (regular, selected) of steps 2 .. STEPS where the case states them (the scene's own
    otherwise); `between`: {step index: what the caller does to both systems before that step}."""
    t = CountingTwins(ctx, *s.particles, cs=s.cs, chunks=s.chunks, used=s.used, rnd=s.rnd)
    try:
        for k, d in enumerate(s.descs):
            if between is not None and k in between:
                between[k](t)
            t.step(d)
        t.check(what)
        assert t.kernels == list(kernels), (what, t.kernels)
        t.check_waves(what)
        want = want if want is not None else s.want
        if want is not None:
            assert t.waves == [(0, 0)] + list(want), (what, t.waves)
        if also is not None:
            also(t)
    finally:
        t.close()
    return t


# ---- a. the tail's curves, all lanes regular -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(S.SCENES_A))
def test_the_tail_with_every_lane_regular(ctx, name):
    t = run(ctx, name, S.SCENES_A[name]())
    assert t.waves[1:] == [(WAVES, 0)] * (STEPS - 1), (name, t.waves)


@pytest.mark.parametrize("writer", ["upload RC", "upload RD"])
def test_rewritten_render_planes(ctx, writer):
    """The caller rewrites a render plane of a render-current chunk between steps 3 and 4: the launch after it is the general
    instantiation's, which stores everything; the class -- and the regular body with every curve non-constant -- comes back after it."""
    s = S.curve_scene(S.four_curves())
    run(ctx, writer, s, kernels=[LEAN, LEAN_CLAMP, LEAN_CLAMP, LEAN, LEAN_CLAMP], want=[(WAVES, 0), (WAVES, 0), (0, 0), (WAVES, 0)],
        between={3: WRITERS[writer]})


# ---- b. what the regular mask does not look at ---------------------------------------------------------------------------------

VELOCITY_CURVES = dict(rotation_from_index=0.001, ColorFromVelocity=curve4(2, **S.COLOR_V), SizeFromVelocity=curve1(2, **S.SIZE_V))


def _set(plane, component, value):
    def fn(pos, vel, attr, i):
        (pos, vel, attr)[plane][i, component] = value
    return fn


# what happens to one lane of each PLACES wave, the lists it runs under
UNSEEN = {
    "velocity z NaN": (_set(1, 2, NAN), [("gravity", "noise"), ("noise",)]),
    "velocity z +inf": (_set(1, 2, INF), [("gravity", "noise"), ("noise",)]),
    "velocity z -inf": (_set(1, 2, -INF), [("gravity", "noise"), ("noise",)]),
    "position x NaN": (_set(0, 0, NAN), [("noise",), ("gravity",)]),
    "position x inf": (_set(0, 0, INF), [("noise",), ("gravity",)]),
    "position z NaN": (_set(0, 2, NAN), [("noise",), ("gravity",)]),
    "velocity x +inf": (_set(1, 0, INF), [("noise",)]),          # infinite, not unordered: the mask passes it
}


@pytest.mark.parametrize("kind,ops", [(kind, ops) for kind in UNSEEN for ops in UNSEEN[kind][1]], ids=lambda v: v if isinstance(v, str) else " ".join(v))
def test_values_the_regular_mask_does_not_see(ctx, kind, ops):
    """Neither mask reads the velocity's z or the position: a lane the kernel calls regular may carry a NaN or infinite speed, velocity-curve
    t and rd.z through the regular tail.  One non-constant velocity curve for the colour and one for the size read that speed.  Which
    body each wave runs follows from the masks over the twin's planes."""
    pos, vel, attr = regular_particles()
    for place in PLACES:
        UNSEEN[kind][0](pos, vel, attr, slot(place))
    run(ctx, "%s under %s" % (kind, ops), scene((pos, vel, attr), desc(ops, update=update_params(**VELOCITY_CURVES))))


@pytest.mark.parametrize("value", [NAN, INF, np.float32(-0.0)], ids=["NaN", "inf", "-0.0"])
def test_odd_attributes_in_a_wave_that_stores_its_colour(ctx, value):
    """ColorFromLife moves its t in most lanes of every wave, so every wave loads its attributes and stores the colour in every step."""
    pos, vel, attr = S.curve_particles()
    for k, place in enumerate(PLACES):
        attr[slot(place), k] = value
        attr[slot(place) + (1 if place[2] < 63 else -1), :] = value
    run(ctx, "attributes %r" % value, scene((pos, vel, attr), desc(S.QUIET, update=update_params(rotation_from_index=0.001, ColorFromLife=curve4(2))), want=all_regular()))


def test_two_nan_payloads_meet_in_the_colour(ctx):
    """What kElideColor is about: with a colour-curve point the host cannot bound, the colour factor may itself be a NaN, and a NaN
    attribute times a NaN factor takes its payload from whichever operand the instruction at hand prefers.  A constant ColorFromVelocity
    of NaN (one payload) over attributes of NaN (another payload, other sign) in some lanes: the regular tail stores the colour in every
    step and must leave the interpreter's bits, whatever the first step's general instantiation left there."""
    factor = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    odd = np.array([0xFFC54321], np.uint32).view(np.float32)[0]
    c = abi.ClampedBezier4(abi.f4(0.0, 1.0, 1, 0), abi.f4(float(factor), 0.5, float(factor), 1.0), abi.f4(1, 1, 1, 1), abi.f4(1, 1, 1, 1), abi.f4(1, 1, 1, 1))
    assert np.float32(c.A.x).view(np.uint32) == 0x7FC12345          # the payload survives the way into the descriptor
    pos, vel, attr = regular_particles()
    for k, place in enumerate(PLACES):
        attr[slot(place), :] = odd
        attr[slot(place) ^ 1, k] = odd
    attr[5 * 64:6 * 64, 0] = odd                # a whole wave
    run(ctx, "NaN payloads", scene((pos, vel, attr), desc(update=update_params(rotation_from_index=0.001, ColorFromVelocity=c)), want=all_regular()))


# ---- c. category bounds -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(S.SCENES_C))
def test_category_bounds(ctx, name):
    run(ctx, name, S.SCENES_C[name]())


# ---- d. FMA away from position 0 -------------------------------------------------------------------------------------------------

FMA_LISTS = {
    "gravity noise fma": lambda fma: ("gravity", "noise", ("fma", fma)),
    "noise fma gravity gravity": lambda fma: ("noise", ("fma", fma), "gravity", "gravity"),
    # the first FMA leaves the life and the category alone, the second is the one the case is about
    "fma noise fma": lambda fma: ("fma", "noise", ("fma", fma)),
}


@pytest.mark.parametrize("ops", list(FMA_LISTS))
def test_fma_that_ends_a_life_behind_other_transforms(ctx, ops):
    """FMA takes 1 / 6 of a life a step (plus the decay): a slot with 0.4 passes the class's first step and goes below zero inside FMA in
    its second.  That wave starts again in the selecting body FROM THE LOADED STATE -- the transforms before FMA have already run on the
    registers -- counts as neither regular nor selected, and the lane is dead from then on."""
    pos, vel, attr = regular_particles()
    for place in PLACES:
        pos[slot(place), 3] = 0.4
    run(ctx, "fma ends a life, %s" % ops, scene((pos, vel, attr), desc(FMA_LISTS[ops](dict(life_add=-1.0)))), want=[(WAVES, 0)] + [(WAVES - K, 0)] * 3)


@pytest.mark.parametrize("ops", list(FMA_LISTS))
def test_fma_that_changes_one_lanes_category_behind_other_transforms(ctx, ops):
    """VelocityMultiply.w = 0.5 halves the distance of a category to 0 at t = 1 / 6: category 0 keeps its bits, 0.25 (inside every filter)
    changes them in every step and stays inside.  The waves with such a lane start again in every step; the others are regular."""
    pos, vel, attr = regular_particles()
    for place in PLACES:
        vel[slot(place), 3] = 0.25

    def still_inside(t):
        c = np.concatenate([t.systems[0].download(k, V)[:, 3] for k in range(2)])
        assert np.all(c[[slot(place) for place in PLACES]] > 0.1) and np.count_nonzero(c) == K
    run(ctx, "fma moves a category, %s" % ops, scene((pos, vel, attr), desc(FMA_LISTS[ops](dict(category=(0.5, 0.0))))), want=with_places(), also=still_inside)


@pytest.mark.parametrize("ops", list(FMA_LISTS))
def test_fma_that_takes_every_life_to_infinity(ctx, ops):
    """PositionAdd.w = inf: every life leaves FMA as +inf.  That is neither <= 0 nor a change of the category, so no wave restarts: each
    runs the regular transforms, fails the second mask and counts as `selected` once; from then on it loads an infinite life and is
    neither -- the selecting body's: FMA's lerp then forms inf - inf and the lives end as NaN.  (The first step, the general
    instantiation's, runs the list without its last FMA so that the class meets finite lives.)"""
    full = FMA_LISTS[ops](dict(life_add=float("inf")))
    s = scene(regular_particles(), desc(full), first=desc(full[:-1] if ops != "noise fma gravity gravity" else ("noise", "gravity", "gravity")))
    lives = []

    def after_the_first_class_step(t):
        lives.append(np.concatenate([t.systems[0].download(c, P)[:, 3] for c in range(2)]))

    def not_finite(t):
        assert np.all(lives[0] == INF)
        assert all(np.all(np.isnan(t.systems[0].download(c, P)[:, 3])) for c in range(2))
    run(ctx, "fma makes lives infinite, %s" % ops, s, want=[(0, WAVES), (0, 0), (0, 0), (0, 0)], between={2: after_the_first_class_step}, also=not_finite)


def test_fma_that_overflows_one_lanes_life(ctx):
    """PositionMultiply.w = 2 doubles towards the life at t = 1 / 6: lives of 50 to 90 grow by a sixth a step, a life of 3e38 overflows to
    +inf inside FMA.  The waves with such a lane count as `selected` in the class's first step and as neither afterwards."""
    pos, vel, attr = regular_particles()
    for place in PLACES:
        pos[slot(place), 3] = 3e38
    ops = ("gravity", "noise", ("fma", dict(life_multiply=2.0)))
    run(ctx, "fma overflows a life", scene((pos, vel, attr), desc(ops), first=desc(ops[:2])), want=[(WAVES - K, K)] + [(WAVES - K, 0)] * 3)


DT_MS_OVER_DIVISOR = float(S.DT_MS) / 100.0          # Strength x dtMs / TimeDivisor at 10 cycles per second


def fma_category(category, multiply, add, t):
    """apply_fma's category in float32: lerp(c, c x VelocityMultiply.w + VelocityAdd.w, t), every operation rounded on its own (the
    library is compiled without contraction; a fused multiply-add of these operands gives the same zero)."""
    f = np.float32
    c, m, a, t = f(category), f(multiply), f(add), f(t)
    b = f(f(c * m) + a)
    return f(c + f(f(b - c) * t))


def test_fma_with_a_negative_category_factor_on_category_zero(ctx):
    """VelocityMultiply.w = -1 on category +0: 0 x -1 = -0, -0 + 0 = +0, and the lerp from +0 to +0 is +0 + (+0 x t) = +0 -- the bits of
    the loaded category, so no wave restarts and all stay regular.  (A loaded -0 would come out as +0 and restart; derived, not assumed.)"""
    t = np.float32(DT_MS_OVER_DIVISOR)
    out = fma_category(0.0, -1.0, 0.0, t)
    restarts = out.view(np.uint32) != np.float32(0.0).view(np.uint32)
    assert not restarts and fma_category(-0.0, -1.0, 0.0, t).view(np.uint32) != np.float32(-0.0).view(np.uint32)
    for ops in ("gravity noise fma", "fma noise fma"):
        run(ctx, "category x -1, %s" % ops, scene(regular_particles(), desc(FMA_LISTS[ops](dict(category=(-1.0, 0.0))))),
            want=[(0, 0)] * 4 if restarts else all_regular())


# ---- e. a NaN life out of Noise ---------------------------------------------------------------------------------------------------

def infinite_w_table(but_the_first_lookup):
    """The randomness table with w = inf throughout, or throughout but for the texels Noise's first lookup reads.  With the table's
    own rate a 64 x 64 chunk moves a lookup by less than a tenth of a texel: every slot reads texel (93, 102) at the current offsets
    (0.37 x 253, 0.81 x 127) and (30, 69) at the next ones (0.12 x 253, 0.55 x 127)."""
    rnd = scenes.randomness_table(11).copy()
    w = rnd[..., 3].copy()
    rnd[..., 3] = np.inf
    if but_the_first_lookup:
        rnd[100:106, 91:97, 3] = w[100:106, 91:97]
    return rnd


def test_noise_over_a_table_whose_w_is_infinite_throughout(ctx):
    """PositionScale.w == 0 and finite factors: the host calls this Noise inert, the launch stays lean and in the class.  The life delta
    is sign(d) x max(|d|, minimum) x 0 with d = lerp(inf, inf, FrequencyLerp) + offset -- and inf - inf inside that lerp makes d a NaN,
    max(|NaN|, 0) drops it, and the delta is +-0 after all: no life changes, every wave stays regular.  (Pinned as it is: the 0 x inf
    that the host's test does not exclude needs an infinite d, the next case.)"""
    s = scene(regular_particles(), desc(), rnd=infinite_w_table(False), first=desc(("gravity",)))

    def all_finite(t):
        assert all(np.all(np.isfinite(t.systems[0].download(c, P)[:, 3])) for c in range(2))
    run(ctx, "w = inf throughout", s, want=all_regular(), also=all_finite)


def test_noise_that_makes_every_life_a_nan(ctx):
    """The same table with finite w where the first of the two lookups reads: lerp(finite, inf, 0.35) = inf, d = inf, and the life delta
    is inf x 0 = NaN.  The host still calls the Noise inert (its test reads the parameters, not the table), the launch stays lean and in
    the class, and inside the regular body every life becomes a NaN.  A NaN life is alive (`<= 0` is false) and fails the second mask
    -- every wave counts as `selected` in that step -- and from then on it fails the first.  (The first step, the general
    instantiation's, runs Gravity alone so that the class meets finite lives.)"""
    s = scene(regular_particles(), desc(), rnd=infinite_w_table(True), first=desc(("gravity",)))

    def all_nan(t):
        assert all(np.all(np.isnan(t.systems[0].download(c, P)[:, 3])) for c in range(2))
    run(ctx, "NaN lives out of Noise", s, want=[(0, WAVES), (0, 0), (0, 0), (0, 0)], also=all_nan)


# ---- f. shapes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(S.SCENES_F))
def test_shapes(ctx, name):
    s = S.SCENES_F[name]()
    run(ctx, name, s)


def test_chunks_outside_the_stepped_range_keep_every_bit(ctx):
    s = S.SCENES_F["the second of three chunks"]()
    pos, vel, attr = s.particles
    render = {}

    def keep_render_planes(t):
        for i, system in enumerate(t.systems):
            for c in (0, 2):
                for plane in PLANES[3:]:
                    render[i, c, plane] = system.download(c, plane)

    def untouched(t):
        for i, system in enumerate(t.systems):
            for c in (0, 2):
                sl = slice(c * N, (c + 1) * N)
                for plane, want in ((P, pos[sl]), (V, vel[sl]), (A, attr[sl])):
                    assert_bits_equal(system.download(c, plane), want, "chunk %d plane %d after steps of chunk 1 alone" % (c, plane))
                for plane in PLANES[3:]:
                    assert_bits_equal(system.download(c, plane), render[i, c, plane], "chunk %d render plane %d after steps of chunk 1 alone" % (c, plane))
            assert not np.array_equal(system.download(1, P), pos[N:2 * N])
    run(ctx, "one chunk of three", s, between={0: keep_render_planes}, also=untouched)


# ---- g. a seeded sweep --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", S.SWEEP_SEEDS)
def test_sweep(ctx, seed):
    t = run(ctx, "sweep seed %d" % seed, S.sweep_scene(seed))
    assert all(regular >= 0.9 * WAVES for regular, _ in t.waves[1:]), "sweep seed %d: %s" % (seed, t.waves)
