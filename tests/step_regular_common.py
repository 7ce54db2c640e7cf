"""What the tests of step_lean_clamp_kernel's two bodies share (tests/test_step_regular_waves_gpu.py, tests/test_step_regular_body_gpu.py on
the device, tests/test_step_regular_scenes.py on the CPU): the twins that count which body each wave ran, the descriptor and particle
builders, a numpy statement of the kernel's two masks (predict_waves) and the scenes of the body tests.  No test lives here.

A scene is the particles, one descriptor per step and what the scene claims about itself: the CPU file steps it through the oracle and holds
it to that claim, the GPU file steps it on the device against the interpreter twin.  The device and the oracle agree to 1e-4 relative, not bit
for bit, so lives and ranges are chosen with margins: nothing a claim rests on comes within 1 % of zero or of a curve's range end.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from illuminant_amd import abi, native, scenes
from tests.test_step_store_elision_gpu import Twins, update_params, P, V, A
from tests.test_step_lean_classes_gpu import curve1, curve4

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
GRAVITY_FILTER, NOISE_FILTER, FMA_FILTER = (0.0, 1.0), (-1.0, 0.5), (-1.0, 1.0)       # regular particles have category 0
# (chunk, wave of the chunk, lane) of the irregular lanes: the wave's first and last lane and both sides of the middle, in waves whose
# neighbours stay regular
PLACES = ((0, 3, 0), (0, 17, 31), (1, 40, 32), (1, 63, 63))
K = len(PLACES)
LIFE_RANGE = (0.0, 80.0)         # the range of the life curves of the body tests: lives of 50 to 90 lie on both sides of its end


def _op(entry):
    """An entry of desc's `ops`: a kind, or (kind, overrides)."""
    return (entry, {}) if isinstance(entry, str) else (entry[0], dict(entry[1]))


def desc(ops=("gravity", "noise"), update=None, fma_life_add=0.0, fma_category=(1.0, 0.0), cs=CS, first_chunk=0, chunk_count=-1):
    """ops: "gravity" | "noise" | "fma", or (kind, overrides) with `filter` (any kind), `replace` (Noise: ReplaceOldVelocity),
    `life_add`, `life_multiply`, `category` (FMA: PositionAdd.w, PositionMultiply.w, (VelocityMultiply.w, VelocityAdd.w))."""
    d = abi.StepDesc()
    d.FirstChunk, d.ChunkCount = first_chunk, chunk_count
    d.System = scenes.system_uniforms(cs, friction=0.02, max_velocity=MAX_VELOCITY, life_decay=LIFE_DECAY)
    # rotation from the index alone: rd.y does not read the life, the host says so and the regular body does not evaluate it
    d.Update = update if update is not None else update_params(rotation_from_index=0.001)
    d.OpCount = len(ops)
    for o, entry in enumerate(ops):
        kind, over = _op(entry)
        if kind == "gravity":
            d.Ops[o].Type = abi.OP_GRAVITY
            d.Ops[o].u.Gravity = scenes.gravity_params([((60., 70., 0.), 40., 500., 1), ((200., 60., 10.), 90., 700., 2), ((100., 210., 0.), 120., 900., 1),
                                                        ((30., 180., 5.), 70., 300., 2)], maximum_acceleration=64.0, category_filter=over.get("filter", GRAVITY_FILTER))
        elif kind == "noise":
            d.Ops[o].Type = abi.OP_NOISE
            d.Ops[o].u.Noise = scenes.noise_params(scenes.area_none(category_filter=over.get("filter", NOISE_FILTER)), (0.37 * 253, 0.81 * 127), (0.12 * 253, 0.55 * 127),
                                                   0.35, replace_old_velocity=over.get("replace", True))
        else:
            assert kind == "fma", kind
            d.Ops[o].Type = abi.OP_FMA
            d.Ops[o].u.FMA = scenes.fma_params(scenes.area_none(category_filter=over.get("filter", FMA_FILTER)), position_add=(0.5, -0.25, 0.0), velocity_multiply=(0.98, 0.97, 1.0))
            d.Ops[o].u.FMA.PositionAdd.w = over.get("life_add", fma_life_add)
            d.Ops[o].u.FMA.PositionMultiply.w = over.get("life_multiply", 1.0)
            d.Ops[o].u.FMA.VelocityMultiply.w, d.Ops[o].u.FMA.VelocityAdd.w = over.get("category", fma_category)
    d.UpdateMode = abi.UPDATE_POSITIONS
    d.Flags = abi.STEP_COUNT_LIVE
    return d


def regular_particles(seed=5, cs=CS, chunks=CHUNKS, life=(50.0, 90.0)):
    """Every slot regular and far from the end of its life."""
    return scenes.make_particles(seed, cs * cs * chunks, life=life, categories=(0.0,))


def slot(place, cs=CS):
    chunk, wave, lane = place
    return chunk * cs * cs + wave * 64 + lane


def places_for(cs):
    """PLACES in one chunk of size cs: the waves spread over the chunk as PLACES spreads them over 64 x 64, the k-th in the k-th unit of its
    row (a row of cs slots holds cs / 64 units), the lanes as they are."""
    per_row, scale = cs // 64, (cs * cs) // N
    return tuple((0, wave * scale - (wave * scale) % per_row + k % per_row, lane) for k, (_, wave, lane) in enumerate(PLACES))


def has_fma(d):
    return any(d.Ops[o].Type == abi.OP_FMA for o in range(d.OpCount))


def category_bounds(d):
    """regular_cat_lo / regular_cat_hi as build_lean_step forms them: the intersection of the transforms' category filters in float32;
    a NaN bound anywhere makes the lower bound a NaN, which admits no category; without a transform (-inf, +inf): any category but NaN."""
    lo, hi = np.float32(-np.inf), np.float32(np.inf)
    for o in range(d.OpCount):
        op = d.Ops[o]
        f = op.u.Gravity.CategoryFilter if op.Type == abi.OP_GRAVITY else op.u.Noise.Area.CategoryFilter if op.Type == abi.OP_NOISE else op.u.FMA.Area.CategoryFilter
        f0, f1 = np.float32(f[0]), np.float32(f[1])
        if np.isnan(f0) or np.isnan(f1):
            lo = NAN
        lo = f0 if f0 > lo else lo          # (a NaN lower bound stays: the comparison is false)
        hi = f1 if f1 < hi else hi
    return lo, hi


def wave_masks(before, after, cat_lo, cat_hi):
    """Per 64-slot wave: (every lane passes regular_lanes_loaded, every lane passes regular_lanes_updated).  before, after: (position plane,
    velocity plane), (n, 4) float32 with n a multiple of 64, as the interpreter leaves them before and after the step."""
    (p0, v0), (p1, v1) = before, after
    assert p0.shape == v0.shape == p1.shape == v1.shape and p0.shape[0] % 64 == 0 and p0.dtype == np.float32
    cat_lo, cat_hi = np.float32(cat_lo), np.float32(cat_hi)
    with np.errstate(invalid="ignore"):
        loaded = (p0[:, 3] > 0) & (p0[:, 3] < INF) & (v0[:, 3] >= cat_lo) & (v0[:, 3] <= cat_hi) & ~(np.isnan(v0[:, 0]) | np.isnan(v0[:, 1]))
        updated = (p1[:, 3] > 0) & (p1[:, 3] < INF) & ~(np.isnan(v1[:, 0]) | np.isnan(v1[:, 1]))
    return loaded.reshape(-1, 64).all(axis=1), updated.reshape(-1, 64).all(axis=1)


def predict_waves(before, after, cat_lo, cat_hi):
    """(regular, selected): how many waves of a class step run the regular body to its end, and how many run the regular transforms and
    then the selecting update and tail.  Exact for a list without FMA (only FMA sends a wave back to the top): the interpreter stores a
    lane that is alive after the step as the regular body computes it, and zeros or a NaN life exactly where the second mask fails."""
    loaded, updated = wave_masks(before, after, cat_lo, cat_hi)
    return int((loaded & updated).sum()), int((loaded & ~updated).sum())


def stepped_range(d, chunks):
    last = chunks if d.ChunkCount < 0 else d.FirstChunk + d.ChunkCount
    return range(d.FirstChunk, last)


class CountingTwins(Twins):
    """Twins over given particles; records the kernel and the two wave counts of every step of the first (default choice) system, and
    what predict_waves makes of the interpreter twin's planes before and after the step (None for a list with FMA; (0, 0) for a step
    outside the class, which counts nothing)."""

    def __init__(self, ctx, pos, vel, attr, cs=CS, chunks=CHUNKS, used=None, rnd=None):
        self.ctx = ctx
        self.cs, self.n, self.chunks = cs, cs * cs, chunks
        self.rnd = rnd if rnd is not None else scenes.randomness_table(11)
        self.eng = native.Engine(ctx, cs, self.rnd)
        self.systems = [native.System(self.eng), native.System(self.eng)]    # [default choice, interpreter]
        self.counts = [[], []]
        self.kernels, self.waves, self.predicted = [], [], []
        used = used or [self.n] * chunks
        for s in self.systems:
            for c in range(chunks):
                s.add_chunk()
                sl = slice(c * self.n, c * self.n + used[c])
                s.upload(c, P, pos[sl]); s.upload(c, V, vel[sl]); s.upload(c, A, attr[sl])
        self.prev = native.lib().ilm_debug_step_interpreter(0)
        native.check(native.lib().ilm_debug_step_regular_waves(ctx.handle, 1, None, None))

    def twin_state(self, chunk_range):
        twin = self.systems[1]
        return (np.concatenate([twin.download(c, P) for c in chunk_range]), np.concatenate([twin.download(c, V) for c in chunk_range]))

    def step(self, d, n=1):
        for _ in range(n):
            chunk_range = stepped_range(d, self.chunks)
            before = self.twin_state(chunk_range)
            for i, s in enumerate(self.systems):
                native.lib().ilm_debug_step_interpreter(i)
                s.step(d)
                if i == 0:
                    regular, selected = C.c_uint64(0), C.c_uint64(0)
                    native.check(native.lib().ilm_debug_step_regular_waves(self.ctx.handle, 1, C.byref(regular), C.byref(selected)))
                    self.kernels.append(native.lib().ilm_debug_last_step_kernel())
                    self.waves.append((int(regular.value), int(selected.value)))
                self.counts[i].append(s.step_counts().copy())
            if self.kernels[-1] != LEAN_CLAMP:
                self.predicted.append((0, 0))
            elif has_fma(d):
                self.predicted.append(None)
            else:
                self.predicted.append(predict_waves(before, self.twin_state(chunk_range), *category_bounds(d)))
        native.lib().ilm_debug_step_interpreter(0)

    def check_waves(self, what):
        for k, (got, want) in enumerate(zip(self.waves, self.predicted)):
            assert want is None or got == want, "%s: step %d counted (regular, selected) = %s, the masks over the twin's planes give %s" % (what, k + 1, got, want)

    def close(self):
        native.check(native.lib().ilm_debug_step_regular_waves(self.ctx.handle, 0, None, None))
        super().close()


# ---- the scenes of the body tests ------------------------------------------------------------------------------------------------

# particles: (pos, vel, attr) over all chunks; descs: one descriptor per step; want: the (regular, selected) waves of steps 2 .. STEPS by
# reasoning, or None where only the masks say; claims: what the CPU file holds the scene to on the oracle (test_step_regular_scenes.py)
Scene = namedtuple("Scene", "particles descs cs chunks used rnd want claims")


def scene(particles, d, cs=CS, chunks=CHUNKS, used=None, rnd=None, want=None, first=None, **claims):
    """`first`: the descriptor of the first step where it differs (a list whose first step would already spoil every life)."""
    return Scene(particles, [first if first is not None else d] + [d] * (STEPS - 1), cs, chunks, used, rnd, want, claims)


def all_regular(waves=WAVES):
    return [(waves, 0)] * (STEPS - 1)


def with_places(waves=WAVES, k=K):
    """The waves with an irregular lane run the selecting body from the top in every step of the class."""
    return [(waves - k, 0)] * (STEPS - 1)


QUIET = ("gravity", ("noise", dict(replace=False)))       # a Noise that adds to the velocity: the lanes of a wave keep speeds of their own
# velocity ranges the planted speeds straddle: slow lanes stay below both `lo`, fast ones above both upper ends (Gravity adds at most
# MaximumAcceleration x dtMs / 1000 = 1.07 a step)
COLOR_V, SIZE_V = dict(lo=20.0, inverse=1.0 / 45.0), dict(lo=25.0, inverse=1.0 / 35.0)


def curve_particles(seed=5, cs=CS, chunks=CHUNKS):
    """regular_particles with, in every wave, two slow and two fast lanes, a life clamped above the life range and one inside it, and no
    life within 1 % of the range's end."""
    pos, vel, attr = regular_particles(seed, cs, chunks)
    near = np.abs(pos[:, 3] - LIFE_RANGE[1]) < 0.011 * LIFE_RANGE[1]
    pos[near, 3] = 70.0
    vel[5::64, :3] = (1.0, -2.0, 0.5); vel[6::64, :3] = (0.5, 0.5, -0.2)
    vel[7::64, :3] = (80.0, 50.0, 10.0); vel[8::64, :3] = (-70.0, 60.0, -12.0)
    pos[9::64, 3] = 88.0; pos[10::64, 3] = 60.0
    return pos, vel, attr


def four_curves(sign=1.0):
    return dict(ColorFromLife=curve4(2, inverse=sign / 80.0), ColorFromVelocity=curve4(3, lo=COLOR_V["lo"], inverse=sign * COLOR_V["inverse"]),
                SizeFromLife=curve1(4, inverse=sign / 80.0), SizeFromVelocity=curve1(2, lo=SIZE_V["lo"], inverse=sign * SIZE_V["inverse"]))


def curve_scene(curves, **update):
    u = dict(rotation_from_index=0.001)
    u.update(curves); u.update(update)
    return scene(curve_particles(), desc(QUIET, update=update_params(**u)), want=all_regular(), all_regular=True, curves=tuple(curves))


def one_lane_scene():
    """Every life clamped far above the life range but one lane's in each PLACES wave: that lane alone moves its t."""
    pos, vel, attr = regular_particles(life=(200.0, 400.0))
    for place in PLACES:
        pos[slot(place), 3] = 40.0
    u = update_params(rotation_from_index=0.001, ColorFromLife=curve4(2), SizeFromLife=curve1(4))
    return scene((pos, vel, attr), desc(update=u), want=all_regular(), all_regular=True, one_lane=("ColorFromLife", "SizeFromLife"))


def unbounded_colour(point):
    """A constant ColorFromVelocity with a point the host cannot bound: kElideColor is off and the colour is stored in every step."""
    c = abi.ClampedBezier4(abi.f4(0.0, 1.0, 1, 0), abi.f4(1.0, 0.5, 0.25, 1.0), abi.f4(0.5, float(point), 0.5, 0.5), abi.f4(1, 1, 1, 1), abi.f4(1, 1, 1, 1))
    return scene(regular_particles(), desc(update=update_params(rotation_from_index=0.001, ColorFromVelocity=c)), want=all_regular(), all_regular=True)


def size_scene(size_from_life, size_from_velocity=None):
    u = dict(rotation_from_index=0.001, SizeFromLife=abi.ClampedBezier1.constant(float(size_from_life)))
    if size_from_velocity is not None:
        u["SizeFromVelocity"] = size_from_velocity
    return scene(curve_particles(), desc(QUIET, update=update_params(**u)), want=all_regular(), all_regular=True)


def rotation_scene(from_life, from_index):
    return scene(regular_particles(), desc(update=update_params(rotation_from_life=from_life, rotation_from_index=from_index)), want=all_regular(), all_regular=True)


SCENES_A = {
    "four clamp curves, counts 2 3 4 2": lambda: curve_scene(four_curves()),
    "negative inverse divisors": lambda: curve_scene(four_curves(-1.0)),
    "ColorFromLife alone": lambda: curve_scene(dict(ColorFromLife=curve4(3))),
    "ColorFromVelocity alone": lambda: curve_scene(dict(ColorFromVelocity=curve4(4, **COLOR_V)), ColorFromLife=abi.UpdateParams.default().ColorFromLife),
    "SizeFromLife alone": lambda: curve_scene(dict(SizeFromLife=curve1(2)), ColorFromLife=abi.UpdateParams.default().ColorFromLife),
    "SizeFromVelocity alone": lambda: curve_scene(dict(SizeFromVelocity=curve1(3, **SIZE_V)), ColorFromLife=abi.UpdateParams.default().ColorFromLife),
    "exactly one lane of a wave changes t": one_lane_scene,
    "colour curve point inf": lambda: unbounded_colour(np.inf),
    "colour curve point 0x1p61": lambda: unbounded_colour(2.0 ** 61),
    "size NaN in every lane": lambda: size_scene(np.nan),
    # a linear SizeFromVelocity from 0: the lanes at or below `lo` give inf x 0
    "size NaN in the slow lanes": lambda: size_scene(np.inf, abi.ClampedBezier1(abi.f4(SIZE_V["lo"], SIZE_V["inverse"], 2, 0), abi.f4(0.0, 2.0, 1.25, 3.0))),
    "rotation from life -0.0": lambda: rotation_scene(-0.0, 0.001),
    "rotation from life 0.25": lambda: rotation_scene(0.25, 0.001),
    "rotation from life 0.25, index factor 0": lambda: rotation_scene(0.25, 0.0),
}


def _category_scene(category, regular):
    pos, vel, attr = regular_particles()
    for place in PLACES:
        vel[slot(place), 3] = category
    return scene((pos, vel, attr), desc(), want=all_regular() if regular else with_places())


def _filter_scene(ops, lanes, want):
    """lanes: the category of the lane of each PLACES wave."""
    pos, vel, attr = regular_particles()
    for place, category in zip(PLACES, lanes):
        vel[slot(place), 3] = category
    return scene((pos, vel, attr), desc(ops), want=want)


EVERY = (-INF, INF)
SCENES_C = {
    # Gravity's filter is (0, 1), Noise's (-1, 0.5): the intersection is 0 .. 0.5, both ends included
    "category 0.0": lambda: _category_scene(0.0, True),
    "category -0.0": lambda: _category_scene(-0.0, True),
    "category 0.5": lambda: _category_scene(0.5, True),
    "category just above 0.5": lambda: _category_scene(np.nextafter(np.float32(0.5), np.float32(1.0)), False),
    "category just below 0.0": lambda: _category_scene(np.nextafter(np.float32(0.0), np.float32(-1.0)), False),
    "category +inf": lambda: _category_scene(INF, False),
    "empty intersection": lambda: _filter_scene((("gravity", dict(filter=(0.6, 1.0))), "noise"), (0.0, 0.55, 0.6, 0.5), [(0, 0)] * 4),
    "NaN bound on Gravity": lambda: _filter_scene((("gravity", dict(filter=(float("nan"), 1.0))), "noise"), (0.0, 0.25, 0.5, -0.0), [(0, 0)] * 4),
    "NaN bound on Noise": lambda: _filter_scene(("gravity", ("noise", dict(filter=(-1.0, float("nan"))))), (0.0, 0.25, 0.5, -0.0), [(0, 0)] * 4),
    "both bounds infinite": lambda: _filter_scene((("gravity", dict(filter=EVERY)), ("noise", dict(filter=EVERY))), (INF, -INF, 3e38, NAN), with_places(k=1)),
    # the lower bound is the second Gravity's, the upper one Noise's; the first Gravity accepts more than either
    "three nested filters": lambda: _filter_scene((("gravity", dict(filter=(-2.0, 2.0))), "noise", ("gravity", dict(filter=(-0.25, 1.0)))),
                                                  (-0.25, 0.5, np.nextafter(np.float32(-0.25), np.float32(-1.0)), np.nextafter(np.float32(0.5), np.float32(1.0))),
                                                  with_places(k=2)),
}


def _shape_scene(cs, kind):
    """One chunk of cs x cs, a Noise list, rotation from life and index; the PLACES lanes dead at load or of a NaN category."""
    pos, vel, attr = regular_particles(cs=cs, chunks=1)
    waves = cs * cs // 64
    for place in places_for(cs):
        if kind == "dead at load":
            pos[slot(place, cs), 3] = 0.0
        elif kind == "NaN category":
            vel[slot(place, cs), 3] = NAN
    d = desc(("noise",), update=update_params(rotation_from_life=0.25, rotation_from_index=0.001), cs=cs)
    return scene((pos, vel, attr), d, cs=cs, chunks=1, want=all_regular(waves) if kind == "all regular" else with_places(waves))


def _partly_used(used_slots):
    """The second chunk holds used_slots slots: the units past them are not walked, a unit they end in has never-written lanes."""
    whole, rest = divmod(used_slots, 64)
    return scene(regular_particles(), desc(), used=[N, used_slots], want=[(N // 64 + whole, 0)] * (STEPS - 1), rest=rest)


def _one_chunk_of_three():
    return scene(regular_particles(chunks=3), desc(first_chunk=1, chunk_count=1), chunks=3, want=all_regular(N // 64))


SCENES_F = {}
for _cs in (128, 256):
    for _kind in ("all regular", "dead at load", "NaN category"):
        SCENES_F["chunk size %d, %s" % (_cs, _kind)] = (lambda cs=_cs, kind=_kind: _shape_scene(cs, kind))
SCENES_F["second chunk of 1024 used slots"] = lambda: _partly_used(1024)
SCENES_F["second chunk of 1000 used slots"] = lambda: _partly_used(1000)
SCENES_F["the second of three chunks"] = _one_chunk_of_three


def _irregular(rng):
    """One of the kinds of irregular lane that need no FMA, as a function of (pos, vel, attr, slot)."""
    kinds = [
        lambda p, v, a, i: p.__setitem__((i, 3), 0.0), lambda p, v, a, i: p.__setitem__((i, 3), NAN), lambda p, v, a, i: p.__setitem__((i, 3), INF),
        lambda p, v, a, i: p.__setitem__((i, 3), np.float32(2.0) * DECAY), lambda p, v, a, i: v.__setitem__((i, 3), -0.5),
        lambda p, v, a, i: v.__setitem__((i, 3), 1.0), lambda p, v, a, i: v.__setitem__((i, 3), NAN), lambda p, v, a, i: v.__setitem__((i, 0), NAN),
        lambda p, v, a, i: v.__setitem__((i, 2), NAN), lambda p, v, a, i: v.__setitem__((i, 2), -INF), lambda p, v, a, i: p.__setitem__((i, 0), NAN),
        lambda p, v, a, i: p.__setitem__((i, 2), INF), lambda p, v, a, i: a.__setitem__((i, 1), NAN),
    ]
    return kinds[int(rng.integers(len(kinds)))]


SWEEP_SEEDS = tuple(range(8))


def sweep_scene(seed):
    """A random subset of the four curves made non-constant with random counts and divisor signs, Gravity and Noise in a random order, up
    to six irregular lanes at random places."""
    rng = np.random.default_rng(1000 + seed)
    u = dict(rotation_from_index=0.001, ColorFromLife=abi.UpdateParams.default().ColorFromLife)
    for name, make, rng_range in (("ColorFromLife", curve4, dict(lo=0.0, inverse=1.0 / 80.0)), ("ColorFromVelocity", curve4, COLOR_V),
                                  ("SizeFromLife", curve1, dict(lo=0.0, inverse=1.0 / 80.0)), ("SizeFromVelocity", curve1, SIZE_V)):
        if rng.integers(2):
            sign = -1.0 if rng.integers(2) else 1.0
            u[name] = make(int(rng.integers(2, 5)), lo=rng_range["lo"], inverse=sign * rng_range["inverse"])
    ops = QUIET if rng.integers(2) else QUIET[::-1]
    pos, vel, attr = curve_particles(seed=20 + seed)
    for _ in range(int(rng.integers(0, 7))):
        _irregular(rng)(pos, vel, attr, int(rng.integers(CHUNKS * N)))
    return scene((pos, vel, attr), desc(ops, update=update_params(**u)), min_regular=0.9)


# ---- the scenes on the CPU ---------------------------------------------------------------------------------------------------------

def clamp_t(rc, value):
    """t_for_clamp_bezier in float32: RangeAndCount = (lo, inverse divisor, count, mode)."""
    t = np.clip((np.asarray(value, np.float32) - np.float32(rc.x)) * np.abs(np.float32(rc.y)), np.float32(0.0), np.float32(1.0)).astype(np.float32)
    return np.float32(1.0) - t if rc.y < 0 else t


def curve_input(name, state):
    """What a curve of the update pass reads: the life, or the speed as render_data floors it."""
    pos, vel = state
    if name.endswith("Life"):
        return pos[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.maximum(np.sqrt((vel[:, :3].astype(np.float32) ** 2).sum(axis=1, dtype=np.float32)), np.float32(0.0001))


def oracle_states(orc, s):
    """The scene stepped through the oracle: [(position, velocity)] over all chunks before the first step and after every step."""
    n = s.cs * s.cs
    pos, vel, attr = s.particles
    used = s.used or [n] * s.chunks
    chunks = []
    for c in range(s.chunks):
        planes = [np.zeros((n, 4), np.float32) for _ in range(5)]
        for plane, data in zip(planes, (pos, vel, attr)):
            plane[:used[c]] = data[c * n:c * n + used[c]]
        chunks.append(planes)
    rnd = s.rnd if s.rnd is not None else scenes.randomness_table(11)

    def state():
        return np.concatenate([ch[0] for ch in chunks]).copy(), np.concatenate([ch[1] for ch in chunks]).copy()
    states = [state()]
    for d in s.descs:
        orc.step(chunks, s.cs, rnd, d)
        states.append(state())
    return states


def chunk_slice(d, s):
    r = stepped_range(d, s.chunks)
    return slice(r.start * s.cs * s.cs, r.stop * s.cs * s.cs)
