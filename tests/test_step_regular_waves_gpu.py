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
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests.test_step_store_elision_gpu import Twins, update_params, P, V, A

pytestmark = pytest.mark.gpu

LEAN, LEAN_CLAMP = 2, 3          # ILM_STEP_KERNEL_* of include/illuminant_hip.h
CS, CHUNKS, STEPS = 64, 2, 5
N = CS * CS
WAVES = CHUNKS * N // 64
NAN, INF = np.float32(np.nan), np.float32(np.inf)
MAX_VELOCITY = 100.0
LIFE_DECAY = 0.6
# one step's decay as the kernels form it: LifeDecay x (dtMs / 1000), in float32
DT_MS = np.float32(1.0 / 60 * 1000.0)
DECAY = np.float32(np.float32(LIFE_DECAY) * np.float32(DT_MS / np.float32(1000.0)))
GRAVITY_FILTER, NOISE_FILTER = (0.0, 1.0), (-1.0, 0.5)       # regular particles have category 0
# (chunk, wave of the chunk, lane) of the irregular lanes: the wave's first and last lane and both sides of the middle, in waves whose
# neighbours stay regular
PLACES = ((0, 3, 0), (0, 17, 31), (1, 40, 32), (1, 63, 63))


@pytest.fixture(autouse=True)
def streaming_variant(monkeypatch):
    monkeypatch.setenv("ILM_STEP_STREAMING", "1")


def desc(ops=("gravity", "noise"), update=None, fma_life_add=0.0, fma_category=(1.0, 0.0)):
    d = abi.StepDesc()
    d.FirstChunk, d.ChunkCount = 0, -1
    d.System = scenes.system_uniforms(CS, friction=0.02, max_velocity=MAX_VELOCITY, life_decay=LIFE_DECAY)
    # rotation from the index alone: rd.y does not read the life, the host says so and the regular body does not evaluate it
    d.Update = update if update is not None else update_params(rotation_from_index=0.001)
    d.OpCount = len(ops)
    for o, kind in enumerate(ops):
        if kind == "gravity":
            d.Ops[o].Type = abi.OP_GRAVITY
            d.Ops[o].u.Gravity = scenes.gravity_params([((60., 70., 0.), 40., 500., 1), ((200., 60., 10.), 90., 700., 2), ((100., 210., 0.), 120., 900., 1),
                                                        ((30., 180., 5.), 70., 300., 2)], maximum_acceleration=64.0, category_filter=GRAVITY_FILTER)
        elif kind == "noise":
            d.Ops[o].Type = abi.OP_NOISE
            d.Ops[o].u.Noise = scenes.noise_params(scenes.area_none(category_filter=NOISE_FILTER), (0.37 * 253, 0.81 * 127), (0.12 * 253, 0.55 * 127), 0.35)
        else:
            d.Ops[o].Type = abi.OP_FMA
            d.Ops[o].u.FMA = scenes.fma_params(scenes.area_none(category_filter=(-1.0, 1.0)), position_add=(0.5, -0.25, 0.0), velocity_multiply=(0.98, 0.97, 1.0))
            d.Ops[o].u.FMA.PositionAdd.w = fma_life_add
            d.Ops[o].u.FMA.VelocityMultiply.w, d.Ops[o].u.FMA.VelocityAdd.w = fma_category
    d.UpdateMode = abi.UPDATE_POSITIONS
    d.Flags = abi.STEP_COUNT_LIVE
    return d


def regular_particles():
    """Every slot regular and far from the end of its life."""
    return scenes.make_particles(5, N * CHUNKS, life=(50.0, 90.0), categories=(0.0,))


def slot(place):
    chunk, wave, lane = place
    return chunk * N + wave * 64 + lane


class CountingTwins(Twins):
    """Twins over given particles; records the kernel and the two wave counts of every step of the first (default choice) system."""

    def __init__(self, ctx, pos, vel, attr):
        self.ctx = ctx
        self.cs, self.n = CS, N
        self.eng = native.Engine(ctx, CS, scenes.randomness_table(11))
        self.systems = [native.System(self.eng), native.System(self.eng)]    # [default choice, interpreter]
        self.counts = [[], []]
        self.kernels, self.waves = [], []
        for s in self.systems:
            for c in range(CHUNKS):
                s.add_chunk()
                sl = slice(c * N, (c + 1) * N)
                s.upload(c, P, pos[sl]); s.upload(c, V, vel[sl]); s.upload(c, A, attr[sl])
        self.prev = native.lib().ilm_debug_step_interpreter(0)
        native.check(native.lib().ilm_debug_step_regular_waves(ctx.handle, 1, None, None))

    def step(self, d, n=1):
        for _ in range(n):
            for i, s in enumerate(self.systems):
                native.lib().ilm_debug_step_interpreter(i)
                s.step(d)
                if i == 0:
                    regular, selected = C.c_uint64(0), C.c_uint64(0)
                    native.check(native.lib().ilm_debug_step_regular_waves(self.ctx.handle, 1, C.byref(regular), C.byref(selected)))
                    self.kernels.append(native.lib().ilm_debug_last_step_kernel())
                    self.waves.append((int(regular.value), int(selected.value)))
                self.counts[i].append(s.step_counts().copy())
        native.lib().ilm_debug_step_interpreter(0)

    def close(self):
        native.check(native.lib().ilm_debug_step_regular_waves(self.ctx.handle, 0, None, None))
        super().close()


def run(ctx, what, particles, d, want_waves, also=None):
    """STEPS steps of d; want_waves: (regular, selected) of steps 2 .. STEPS, the class's (the first step of a system stores everything
    through the general instantiation, which has one body and counts nothing)."""
    t = CountingTwins(ctx, *particles)
    try:
        t.step(d, STEPS)
        t.check(what)
        assert t.kernels == [LEAN] + [LEAN_CLAMP] * (STEPS - 1), (what, t.kernels)
        assert t.waves == [(0, 0)] + list(want_waves), (what, t.waves)
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


K = len(PLACES)
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
