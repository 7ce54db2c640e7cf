"""The slot-walking kernels at chunk sizes that are not powers of two, against the CPU oracle.

ParticleEngineConfiguration(int chunkSize = 256) takes any integer (ParticleEngine.cs:693-695) and so does ilm_engine_create.  Nearly all
of the library's size-dependent code sits on branches that only such sizes take: the division forms of unit -> (chunk, segment) and
slot -> (x, y) with the per-lane row wrap, the padding lanes of a stride rounded up to 1 024, the live-count buckets, the wave-uniform
Noise lookups with `first / chunk_size`, the interpreter as the only step kernel, the ragged last block of the ordered compactions.
The oracle's size handling is a plain `for y .. for x ..` loop, held to a second source in tests/test_chunk_sizes.py.

Every step case has three chunks (unit -> chunk past chunk 0), counts with STEP_COUNT_LIVE and uses the suite's criterion: liveness and
counts exact, floats through assert_close with its defaults."""
import ctypes
import functools

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import lights_common as lc
from tests import output_common as oc
from tests import test_step_batch_gpu as sb
from tests.test_chunk_sizes import feedback_range, feedback_taps, slot_coordinate_source, tap_probe_desc
from tests.test_lights_ext_gpu import particle_scene
from tests.test_lights_ext_gpu import small_field as light_field
from tests.test_particles_gpu import cfg1_field
from tests.test_raster_gpu import compare_images, random_chunks, render_gpu
from tests.test_transforms_gpu import (check_matrix_multiply, check_pattern_spawner, check_position_buffer_spawner, check_spatial_noise, compare)
from tests.util import assert_bits_equal, assert_close

pytestmark = pytest.mark.gpu

P, V, A, RC, RD = abi.PLANE_POSITION, abi.PLANE_VELOCITY, abi.PLANE_ATTRIBUTES, abi.PLANE_RENDER_COLOR, abi.PLANE_RENDER_DATA
PLANES = (P, V, A, RC, RD)
INTERPRETER, LEAN, LEAN_CLAMP = 1, 2, 3          # ILM_STEP_KERNEL_* (tests/test_step_lean_classes_gpu.py holds the values to the header)
N_CHUNKS = 3
RW, RH = abi.RANDOMNESS_WIDTH, abi.RANDOMNESS_HEIGHT

# Each size is the smallest that reaches a branch of its own.
SIZES = {
    10: "100 slots in a span of 1 024: 2 units, a unit covers 7 rows (the per-lane row wrap runs 6 times), 924 padding lanes",
    33: "1 089 slots in a span of 2 048: the second 1 024-block of a compaction holds 65 slots (one full wave and one lane), 959 padding lanes",
    48: "2 304 slots, 36 units, 768 padding lanes; a unit spans two rows; units_per_chunk 48 (a division, not a shift), 4 count buckets; "
        "3 compaction blocks, the last ragged",
    96: "9 216 slots = 9 x 1 024: no padding, yet no multiple of 64 -- every division branch without the padding guard's help",
    192: "36 864 slots, a multiple of 64: the interpreter's wave-uniform Noise lookups with cs_shift < 0, units_per_chunk 576, 16 count buckets; "
         "refused by the lean kernels",
}


@pytest.fixture(scope="module")
def rnd():
    return scenes.randomness_table(23)


def host_chunks(cs, seed, used=None, n_chunks=N_CHUNKS, keep_dead_state=False, **particles):
    """[pos, vel, attr, rc, rd] per chunk; slots from used[c] on were never written (zeros).  keep_dead_state: a dead slot keeps its
    position and velocity and only loses its life (so a Noise that revives it works on finite numbers)."""
    n = cs * cs
    dead = particles.pop("dead_fraction", 0.0) if keep_dead_state else 0.0
    chunks = []
    for c in range(n_chunks):
        u = n if used is None else used[c]
        planes = [np.zeros((n, 4), np.float32) for _ in range(5)]
        pos, vel, attr = scenes.make_particles(seed + c, n, **particles)
        if keep_dead_state:
            pos[scenes.uniform(seed + 50 + c, (n,)) < dead, 3] = 0.0
        planes[0][:u], planes[1][:u], planes[2][:u] = pos[:u], vel[:u], attr[:u]
        chunks.append(planes)
    return chunks


def device_system(eng, chunks, used=None):
    s = native.System(eng)
    for c, planes in enumerate(chunks):
        s.add_chunk()
        u = planes[0].shape[0] if used is None else used[c]
        if u:
            s.upload(c, P, planes[0][:u]); s.upload(c, V, planes[1][:u]); s.upload(c, A, planes[2][:u])
    return s


def download(s):
    return [[s.download(c, plane) for plane in PLANES] for c in range(s.chunk_count())]


def step_both(ctx, oracle, cs, rnd, chunks, descs, used=None, field=None, ramp=None, kernel=None, after=None):
    """Every descriptor of `descs` in turn on the device and on the oracle (which updates `chunks` in place); the counts of every step and
    then all planes are compared.  field = (atlas, format); kernel: what ilm_debug_last_step_kernel must say after every step;
    after(system, chunks): further checks on the stepped system."""
    eng = native.Engine(ctx, cs, rnd)
    sdf = native.DistanceFieldTexture(ctx, field[0], field[1]) if field is not None else None
    otex = oracle.make_texture(field[0], field[1]) if field is not None else None
    s = device_system(eng, chunks, used)
    try:
        if sdf is not None:
            s.set_distance_field(sdf)
        if ramp is not None:
            s.set_life_ramp(ramp)
        for k, d in enumerate(descs):
            d.Flags = abi.STEP_COUNT_LIVE
            s.step(d)
            if kernel is not None:
                assert native.lib().ilm_debug_last_step_kernel() == kernel, "step %d ran kernel %d" % (k, native.lib().ilm_debug_last_step_kernel())
            got_counts = s.step_counts().copy()
            want_counts = oracle.step(chunks, cs, rnd, d, life_ramp=ramp, sdf=otex, want_counts=True)
            assert np.array_equal(got_counts, want_counts), "counts of step %d: %s on the device, %s from the oracle" % (k, got_counts, want_counts)
        compare(download(s), chunks, got_counts, want_counts)
        # count_live_kernel and the ordered list of live slots see the same chunks
        assert np.array_equal(s.live_counts(), want_counts)
        for c, planes in enumerate(chunks):
            assert np.array_equal(s.live_slots(c), np.flatnonzero(planes[0][:, 3] > 0)), "live slots of chunk %d" % c
        if after is not None:
            after(s, chunks)
    finally:
        s.close()
        if sdf is not None:
            sdf.close()
        eng.close()


FMA = dict(position_add=(0.5, -0.25, 0.0), position_multiply=(1.001, 0.999, 1.0), velocity_add=(0.0, 1.5, 0.0), velocity_multiply=(0.98, 0.97, 1.0))
LIVE = dict(life=(0.02, 2.5), dead_fraction=0.5)


def spawning_descs(cs, used_last, steps=3, mode=abi.UPDATE_POSITIONS, **uniforms):
    """Gravity, Noise, FMA, an update and an inline spawner that continues the last chunk's used prefix by an eighth of the chunk per step;
    its range ends inside the chunk, which keeps never-written units."""
    n = cs * cs
    m = max(n // 8, 3)
    descs = []
    for k in range(steps):
        d = sb.noise(sb.gravity(sb.base(cs, mode=mode, **uniforms)))
        sb.add_op(d, abi.OP_FMA, scenes.fma_params(scenes.area_none(0.8), **FMA))
        first = used_last + k * m
        sb.spawner(d, cs, N_CHUNKS - 1, first, first + m - 1, k)
        assert first + m - 1 < n - 1
        descs.append(d)
    return descs


# ---- 1a -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", list(SIZES))
def test_three_steps_with_transforms_and_an_inline_spawner(ctx, oracle, rnd, cs):
    """Three consecutive steps: dead slots are zeroed, spawned slots age, the second step reads what the first stored."""
    n = cs * cs
    used = [n, n, (2 * n) // 5]
    chunks = host_chunks(cs, 300, used, **LIVE)
    before = [int((planes[0][:, 3] > 0).sum()) for planes in chunks]

    def after(s, chunks):
        now = [int((planes[0][:, 3] > 0).sum()) for planes in chunks]
        assert 0 < now[0] < before[0] and now[2] > before[2]         # particles died, the spawner added some
    step_both(ctx, oracle, cs, rnd, chunks, spawning_descs(cs, used[2]), used, kernel=INTERPRETER, after=after)


# ---- 1b -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [abi.UPDATE_NONE, abi.UPDATE_POSITIONS], ids=["no update", "update"])
@pytest.mark.parametrize("cs", [10, 33, 48])
def test_a_noise_that_changes_life_leaves_the_padding_lanes_alone(ctx, oracle, rnd, cs, mode):
    """PositionScale.w != 0: Noise has no life check (Noise.fx:40), so it can bring a dead slot to life (noise_may_revive) -- and would do
    the same to the stride's padding lanes, which the counts and the update would then take for particles."""
    chunks = host_chunks(cs, 320, keep_dead_state=True, life=(0.02, 2.5), dead_fraction=0.5)
    dead_before = [planes[0][:, 3] <= 0 for planes in chunks]
    descs = []
    for _ in range(2):
        d = sb.base(cs, mode=mode)
        # columns 0 .. 4 of the chunk read texel column 14 of the table (a life delta of -0.86), the others column 15 (+1.25)
        sb.add_op(d, abi.OP_NOISE, scenes.noise_params(scenes.area_none(1.0), ((RW * 15 - 5) / RW, 30.0), (45.0, 61.0), 0.25, 10.0, True,
                                                        position=((-0.5,) * 4, (0,) * 4, (1.0, 1.0, 1.0, 4.0))))
        descs.append(d)

    def after(s, chunks):
        revived = sum(int((planes[0][dead, 3] > 0).sum()) for planes, dead in zip(chunks, dead_before))
        still_dead = sum(int((planes[0][dead, 3] <= 0).sum()) for planes, dead in zip(chunks, dead_before))
        assert revived > cs and still_dead > 5, (revived, still_dead)        # the op revived slots, and not all of them
    step_both(ctx, oracle, cs, rnd, chunks, descs, kernel=INTERPRETER, after=after)


# ---- 1c -----------------------------------------------------------------------------------------------------------------------------

def wrap_offset(size, j):
    """An offset of Noise's table lookup whose texel index leaves the table's last column (row) for its first at coordinate j:
    the lookup reads texel floor(coordinate / size + offset) (Noise.fx:49-52: the coordinate is scaled by the texel size twice), and
    offset = (size * size - j) / size."""
    return (size * size - j) / size


def wraps(size, j, last):
    """By integer arithmetic on the offset's numerator: the coordinates in [1, last] at which the texel index changes, each with the
    WRAPped index on its two sides.  The first is the table's wrap (last column or row -> 0) at coordinate j, a further one follows
    `size` coordinates later where the chunk is that large."""
    index = [((x + size * size - j) // size) % size for x in range(last + 1)]
    return [(x, index[x - 1], index[x]) for x in range(1, last + 1) if index[x] != index[x - 1]]


# (chunk size, wrap coordinates along x of (RandomnessOffset, NextRandomnessOffset), the same along y, inline spawner)
UNIFORM_NOISE_CASES = {
    "192, 3 x 3 tables, spawner": (192, (70, 120), (60, 130), True),
    "320, 3 x 3 tables, spawner": (320, (70, 200), (100, 250), True),
    "192, 3 x 3 tables": (192, (40, 150), (1, 191), False),
    "704, 5 x 5 tables": (704, (100, 500), (20, 300), False),
}


@pytest.mark.parametrize("name", list(UNIFORM_NOISE_CASES))
def test_wave_uniform_noise_across_the_wraps_of_the_randomness_table(ctx, oracle, rnd, name):
    """fill_noise_fast applies to every multiple of 64 up to 1 024; away from a power of two the interpreter runs it with `first /
    chunk_size` and wcode[x0 >> 6].  The offsets put the table's 807-column and 653-row wraps inside the coordinates a chunk asks for,
    x in [0, cs + 1] and y in [0, cs]: waves left and right of a step read different classes, the wave a step falls into takes the
    per-lane lookups.  The oracle knows no fast path.

    One sample set steps once per 807 columns and once per 653 rows, so below 654 the two sets give at most two steps per axis and the
    3 x 3 tables always suffice: the 5 x 5 tables (kept in the spawn records' bytes) need a third step, which the smallest multiple of 64
    past 653 + 1 rows, 704, reaches along y."""
    cs, xs, ys, spawn = UNIFORM_NOISE_CASES[name]
    n = cs * cs
    assert cs % 64 == 0 and (cs & (cs - 1)) != 0
    x_steps, y_steps = set(), set()
    for j in xs:
        w = wraps(RW, j, cs + 1)
        assert all(0 < x < cs + 1 and at == (before + 1) % RW for x, before, at in w) and (w[0][1], w[0][2]) == (RW - 1, 0), w
        x_steps |= {x for x, _, _ in w}
    for j in ys:
        w = wraps(RH, j, cs)
        assert all(0 < y < cs and at == (before + 1) % RH for y, before, at in w) and (w[0][1], w[0][2]) == (RH - 1, 0), w
        y_steps |= {y for y, _, _ in w}
    big = len(x_steps) > 2 or len(y_steps) > 2
    assert big == ("5 x 5" in name) and not (big and spawn)
    used = [n, n, (2 * n) // 5] if spawn else None
    chunks = host_chunks(cs, 340, used, **LIVE)
    descs = []
    for k in range(2):
        d = sb.gravity(sb.base(cs), 2)
        sb.add_op(d, abi.OP_NOISE, scenes.noise_params(scenes.area_none(0.9), (wrap_offset(RW, xs[0]), wrap_offset(RH, ys[0])),
                                                        (wrap_offset(RW, xs[1]), wrap_offset(RH, ys[1])), 0.35, 10.0, False,
                                                        position=((-0.5,) * 4, (0,) * 4, (3.0, 2.0, 1.0, 0.0)),
                                                        velocity=((-0.5,) * 3, (0,) * 3, (40.0, 30.0, 5.0)), speed=(-0.5, 0.0, 6.0)))
        if spawn:
            first = used[2] + k * (n // 8)
            sb.spawner(d, cs, 2, first, first + n // 8 - 1, k)
        descs.append(d)
    step_both(ctx, oracle, cs, rnd, chunks, descs, used, kernel=INTERPRETER)


# ---- 1d -----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def collision_field(fmt):
    layout, atlas, dfu = cfg1_field(fmt, packed1=False)       # the particle path's uniforms: DistanceFieldPacked1 = 0, every lookup reads slice 0
    return atlas, dfu


@pytest.mark.parametrize("cells", [True, False], ids=["cells", "ILM_DF_CELLS0=0"])
@pytest.mark.parametrize("fmt", [abi.SDF_UNORM16, abi.SDF_FP16], ids=["unorm16", "fp16"])
@pytest.mark.parametrize("cs", [48, 192])
def test_the_collision_update(ctx, oracle, rnd, monkeypatch, cs, fmt, cells):
    """UpdateWithDistanceField through the interpreter (the lean collision step refuses these sizes): particles start inside and outside
    the demo's cylinders and walls, so redirected, bounced and escaping slots all occur.  sampleDistanceFieldEx calls are counted on
    both sides and must agree exactly."""
    if cells:
        monkeypatch.delenv("ILM_DF_CELLS0", raising=False)
    else:
        monkeypatch.setenv("ILM_DF_CELLS0", "0")
    n = cs * cs
    atlas, dfu = collision_field(fmt)
    used = [n, n, (2 * n) // 5]
    chunks = host_chunks(cs, 360, used, pos_lo=(-20, -20, 0), pos_hi=(276, 276, 32), life=(0.02, 2.5), dead_fraction=0.2, categories=(0.0, 2.0))
    start = np.concatenate([planes[0][planes[0][:, 3] > 0] for planes in chunks])
    in_cylinder = (np.hypot(start[:, 0] - 64.0, start[:, 1] - 64.0) < 10.0) & (start[:, 2] < 40.0)
    in_the_open = (np.hypot(start[:, 0] - 128.0, start[:, 1] - 128.0) < 30.0)
    assert in_cylinder.any() and in_the_open.any()
    descs = spawning_descs(cs, used[2], mode=abi.UPDATE_WITH_DISTANCE_FIELD, collision=(128.0, 0.6, 0.33, 0.4))
    for d in descs:
        d.DistanceField = dfu

    def after(s, chunks):
        ctx.sync()
        lookups = ctypes.c_uint64(0)
        native.check(native.lib().ilm_debug_step_sdf_samples(ctx.handle, 0, ctypes.byref(lookups)))
        want = oracle.update_sdf_samples()
        assert int(lookups.value) == want and want > n, (int(lookups.value), want)
        assert sum(int((planes[1][:, 3] == 3.0).sum()) for planes in chunks) > 10          # BOUNCE_DELAY: redirected or bounced
    oracle.update_sdf_samples()
    native.check(native.lib().ilm_debug_step_sdf_samples(ctx.handle, 1, None))
    try:
        step_both(ctx, oracle, cs, rnd, chunks, descs, used, field=(atlas, fmt), kernel=INTERPRETER, after=after)
    finally:
        native.check(native.lib().ilm_debug_step_sdf_samples(ctx.handle, 0, None))


# ---- 1e -----------------------------------------------------------------------------------------------------------------------------

def test_matrix_multiply_at_48(ctx, oracle):
    check_matrix_multiply(ctx, oracle, 2, cs=48, n_chunks=N_CHUNKS)          # a rotated box with falloff


def test_spatial_noise_at_48(ctx, oracle):
    check_spatial_noise(ctx, oracle, False, cs=48, n_chunks=N_CHUNKS)


def test_position_buffer_spawner_at_48(ctx, oracle):
    check_position_buffer_spawner(ctx, oracle, ((3.0, True),), cs=48, n_chunks=N_CHUNKS)        # slots 700 .. 1500 of chunk 1, a polygon rate


def test_pattern_spawner_at_48(ctx, oracle):
    check_pattern_spawner(ctx, oracle, 2, None, None, False, cs=48, n_chunks=N_CHUNKS)           # 32 x 16 particles per instance from slot 300


def test_life_ramp_at_48(ctx, oracle, rnd):
    """getRampedColorForLifeValueAndIndex reads the ramp at V = index / LifeRampSettings.w with index = x + y * 256 (UpdateCommon.fxh:66-79,
    :107): w = 700 takes V through 17 wraps over the 48 rows of the chunk, and a row holds 48 of the 256 indices its pitch spans."""
    cs = 48
    ramp = scenes.uniform(77, (8, 16, 4))
    chunks = host_chunks(cs, 380, **LIVE)
    descs = []
    for _ in range(2):
        d = sb.gravity(sb.base(cs))
        d.Update.LifeRampSettings = abi.f4(-0.7, 0.5, 4.0, 700.0)
        d.Update.RotationFromLifeAndIndex[0], d.Update.RotationFromLifeAndIndex[1] = 0.25, 0.001
        descs.append(d)
    assert (cs - 1) * 256 / 700.0 > 17
    step_both(ctx, oracle, cs, rnd, chunks, descs, ramp=ramp, kernel=INTERPRETER)


# ---- 1f -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", [33, 48, 96])
def test_feedback_spawner_taps_follow_the_float_arithmetic(ctx, oracle, cs):
    """The feedback spawner reads its source at modf(sourceIndex / size, y) * size and then floor((x * texel) * size) with texel = 1 / size
    (SpawnParticles.fx:54-118): exact only for a power of two.  Elsewhere a third of the taps land one column left of sourceIndex % size;
    that is the reference's behaviour and the device has to reproduce it bit for bit -- a device that divides in integers spawns from
    another particle.  Source and destination systems share an engine; planes and counts as in test_feedback_spawner_matches_oracle,
    then a source whose positions are its slot coordinates shows the taps themselves."""
    n = cs * cs
    rnd = scenes.randomness_table(7)
    first, last, source_index = feedback_range(cs)
    multiplier = 1
    assert last < n and (last - first + 1) // multiplier >= n // 2          # the source indices cover at least half the chunk
    tx, ty, ix, iy = feedback_taps(cs, first, last, multiplier, source_index)
    assert (tx != ix).mean() >= 0.25 and np.array_equal(ty, iy)
    eng = native.Engine(ctx, cs, rnd)
    src, dst, probe = native.System(eng), native.System(eng), native.System(eng)
    try:
        src.add_chunk(); src.add_chunk(); dst.add_chunk(); probe.add_chunk()
        spos, svel, sattr = scenes.make_particles(50, n, dead_fraction=0.3)
        for plane, data in ((P, spos), (V, svel), (A, sattr)):
            src.upload(1, plane, data)
        dpos, dvel, dattr = scenes.make_particles(51, n, dead_fraction=0.7)
        for plane, data in ((P, dpos), (V, dvel), (A, dattr)):
            dst.upload(0, plane, data)
        d = abi.StepDesc()
        d.FirstChunk, d.ChunkCount = 0, -1
        d.System = scenes.system_uniforms(cs)
        d.Update = abi.UpdateParams.default()
        d.UpdateMode = abi.UPDATE_POSITIONS
        d.SpawnCount = 1
        d.Spawns[0].ChunkIndex = 0
        d.Spawns[0].Kind = abi.SPAWN_FEEDBACK
        d.Spawns[0].Params = scenes.spawn_params(cs, first, last, 0, (0.15 * 253, 0.66 * 127),
                                                 position=((1, 2, 3), (4, 4, 4), (0, 0, 0), scenes.FORMULA_SPHERICAL),
                                                 velocity=((0, 0, 0), (20, 20, 20), (0, 0, 0), scenes.FORMULA_TOWARDS), life=(1.5, 1.0, 0.0),
                                                 color=((0.5, 0.6, 0.7, 1.0), (0.1, 0.1, 0.1, 0.0), (0, 0, 0, 0)))
        d.Spawns[0].Feedback = scenes.feedback_params(src.handle.value, 1, source_index, instance_multiplier=multiplier, source_velocity_factor=0.25,
                                                      multiply_life=True, multiply_color_constant=True, source_life_range=(0.5, 5.0))
        d.Flags = abi.STEP_COUNT_LIVE
        dst.step(d)
        chunk = [dpos.copy(), dvel.copy(), dattr.copy(), np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)]
        want_counts = oracle.step([chunk], cs, rnd, d, want_counts=True, feedback_sources={0: (spos, svel, sattr)})
        compare([[dst.download(0, pl) for pl in PLANES]], [chunk], dst.step_counts(), want_counts)
        assert np.array_equal(src.download(1, P), spos)
        # the taps themselves: every spawned particle sits on the coordinates of the texel it was read from
        source = slot_coordinate_source(cs)
        for plane, data in zip((P, V, A), source):
            src.upload(0, plane, data)
        pd = tap_probe_desc(cs, first, last, src.handle.value, 0, source_index, multiplier)
        probe.step(pd)
        want = [np.zeros((n, 4), np.float32) for _ in range(5)]
        want_counts = oracle.step([want], cs, rnd, pd, want_counts=True, feedback_sources={0: source})
        assert np.array_equal(probe.step_counts(), want_counts) and int(want_counts[0]) == last - first + 1
        got = probe.download(0, P)
        spawned = want[0][first:last + 1]
        # the oracle alone meets the float arithmetic, and differs from what integer taps would have given
        assert np.array_equal(spawned[:, 0], tx.astype(np.float32)) and np.array_equal(spawned[:, 1], ty.astype(np.float32))
        assert (spawned[:, 0] != ix.astype(np.float32)).mean() >= 0.25
        assert_bits_equal(got, want[0], "positions spawned from a source that holds its slot coordinates")
    finally:
        for x in (probe, dst, src, eng):
            x.close()


# ---- 1g -----------------------------------------------------------------------------------------------------------------------------

def index_free_desc(cs):
    """Lean-shaped and reading no slot index: Gravity and FMA without an area, UpdatePositions, no life ramp, RotationFromLifeAndIndex.y = 0."""
    d = sb.gravity(sb.base(cs))
    sb.add_op(d, abi.OP_FMA, scenes.fma_params(scenes.area_none(0.8), **FMA))
    d.Update.RotationFromLifeAndIndex[0], d.Update.RotationFromLifeAndIndex[1] = 0.25, 0.0
    return d


@pytest.mark.parametrize("cs", [96, 192])
def test_sizes_the_lean_kernels_refuse_run_the_interpreter(ctx, oracle, rnd, cs):
    """build_lean_step takes powers of two from 64 on: 96 is no multiple of 64, 192 is one and still must be refused."""
    chunks = host_chunks(cs, 400, **LIVE)
    step_both(ctx, oracle, cs, rnd, chunks, [index_free_desc(cs) for _ in range(2)], kernel=INTERPRETER)


def test_a_48_chunk_and_a_64_chunk_step_the_same_particles_to_the_same_bits(ctx, rnd):
    """2 304 particles in a 48-chunk (the interpreter) and in the first 2 304 slots of a 64-chunk whose other slots are dead (the lean
    kernel): nothing the descriptor computes depends on where a slot sits, so three steps leave all five planes bit-equal.  That includes
    the render planes: index = x + y * 256 enters RenderData.y only through RotationFromLifeAndIndex.y (0 here) and RenderColor only
    through a life ramp (none here), UpdateCommon.fxh:66-79 and :107-113."""
    n = 48 * 48
    pos, vel, attr = scenes.make_particles(420, n, **LIVE)
    systems, engines, kernels = [], [], []
    try:
        for cs in (48, 64):
            eng = native.Engine(ctx, cs, rnd)
            engines.append(eng)
            s = native.System(eng)
            systems.append(s)
            s.add_chunk()
            s.upload(0, P, pos); s.upload(0, V, vel); s.upload(0, A, attr)
            for _ in range(3):
                d = index_free_desc(cs)
                d.Flags = abi.STEP_COUNT_LIVE
                s.step(d)
                kernels.append(native.lib().ilm_debug_last_step_kernel())
        assert kernels[:3] == [INTERPRETER] * 3 and all(k in (LEAN, LEAN_CLAMP) for k in kernels[3:]), kernels
        small, large = systems
        assert np.array_equal(small.step_counts(), large.step_counts()) and 0 < int(small.step_counts()[0]) < int((pos[:, 3] > 0).sum())
        for plane in PLANES:
            assert_bits_equal(small.download(0, plane), large.download(0, plane, 0, n), "plane %d of the 48-chunk and of the 64-chunk" % plane)
            assert not large.download(0, plane, n).any() or plane == A
    finally:
        for x in systems + engines:
            x.close()


# ---- 1h -----------------------------------------------------------------------------------------------------------------------------

def test_the_streaming_interpreter_at_48(ctx, rnd, monkeypatch):
    """ILM_STEP_STREAMING=1 against 0 (read per step): the interpreter's STREAM instantiation must leave the same bits in every plane."""
    cs = 48
    n = cs * cs
    used = [n, n, (2 * n) // 5]
    chunks = host_chunks(cs, 440, used, **LIVE)
    eng = native.Engine(ctx, cs, rnd)
    systems = []
    try:
        for streaming in ("0", "1"):
            monkeypatch.setenv("ILM_STEP_STREAMING", streaming)
            s = device_system(eng, chunks, used)
            systems.append(s)
            for d in spawning_descs(cs, used[2]):
                d.Flags = abi.STEP_COUNT_LIVE
                s.step(d)
                assert native.lib().ilm_debug_last_step_kernel() == INTERPRETER
        plain, stream = systems
        assert np.array_equal(plain.step_counts(), stream.step_counts()) and plain.step_counts().all()
        for c in range(N_CHUNKS):
            for plane in PLANES:
                assert_bits_equal(stream.download(c, plane), plain.download(c, plane), "chunk %d plane %d, streaming vs cache-resident interpreter" % (c, plane))
    finally:
        for x in systems + [eng]:
            x.close()


def test_the_batched_step_at_48(ctx, rnd):
    """ilm_engine_step_batch over four systems against a loop of ilm_system_step: planes and counts, three frames."""
    cs = 48
    n = cs * cs
    t = sb.Twins(ctx, cs, rnd)
    try:
        live = dict(life=(0.02, 2.5), dead_fraction=0.2)
        count = abi.STEP_COUNT_LIVE
        items = [(t.system((n, n, n), 1, **live), lambda s: sb.gravity(sb.base(cs, flags=count))),
                 (t.system((n, n, 700), 2, **live), lambda s: sb.spawner(sb.noise(sb.gravity(sb.base(cs, flags=count))), cs, 2, 724, 724 + n // 8)),
                 (t.system((n, 100, n), 3, **live), lambda s: sb.add_op(sb.noise(sb.base(cs, flags=count)), abi.OP_FMA, scenes.fma_params(scenes.area_none(0.8), **FMA))),
                 (t.system((n, n, n), 4, **live), lambda s: sb.noise(sb.gravity(sb.base(cs, first=1, count=2, flags=count), 2)))]
        for frame in range(3):
            launches, rounds, fallback = t.frame(items)
            assert rounds == 1 and fallback == 0 and launches >= 1, (launches, rounds, fallback)
            assert native.lib().ilm_debug_last_step_kernel() == sb.STEP_KERNEL_BATCH
            for i, _ in items:
                t.check_step_counts(i, "frame %d" % frame)
        t.check("four systems, chunk size 48")
    finally:
        t.close()


# ---- 2: the output side ---------------------------------------------------------------------------------------------------------------

def examined(cs):
    """Per-chunk element counts ceil(TotalSpawned / ChunkSize) * ChunkSize: a whole chunk, one that ends inside the ragged last 1 024-block
    of the compactions, and one not examined at all."""
    n = cs * cs
    k = 1024 * (n // 1024) + (n % 1024) // 3
    rows = -(-k // cs) * cs
    assert n % 1024 != 0 and 1024 * (n // 1024) < rows < n
    return [n, rows, 0]


@pytest.mark.parametrize("cs", [33, 48])
def test_readback_with_a_ragged_last_block(ctx, oracle, cs):
    """readback_count/emit_kernel walk a chunk in ceil(slots / 1024) blocks; the last holds 65 (33) or 256 (48) slots."""
    n = cs * cs
    eng = native.Engine(ctx, cs, scenes.randomness_table(7))
    sysm = native.System(eng)
    try:
        chunks = []
        for c in range(N_CHUNKS):
            sysm.add_chunk()
            pos, vel, attr = scenes.make_particles(60 + c, n, pos_lo=(0, 0, 0), pos_hi=(1920, 1080, 32), dead_fraction=0.4)
            rc = scenes.uniform(70 + c, (n, 4), 0.0, 1.2).astype(np.float32)
            rd = np.stack([scenes.uniform(80 + c, (n,), 0.2, 3.0), scenes.uniform(81 + c, (n,), -10.0, 20.0),
                           scenes.uniform(82 + c, (n,), 0.0, 90.0), np.floor(scenes.uniform(83 + c, (n,), 0.0, 6.0))], axis=1).astype(np.float32)
            sysm.upload(c, P, pos); sysm.upload(c, RC, rc); sysm.upload(c, RD, rd)
            chunks.append([pos, vel, attr, rc, rd])
        params = oc.readback_params((2.0, 3.0), (0.0, 0.0, 0.25, 0.25), (1.7, -0.6), 0.35, True, True, True, True)
        elems = examined(cs)
        got, gn = sysm.readback(params, element_counts=elems)
        want, wn = oracle.fill_readback_result(chunks, params, element_counts=elems)
        live = [int((chunks[c][0][:elems[c], 3] > 0).sum()) for c in range(N_CHUNKS)]
        assert gn == wn == sum(live) and live[1] > 0
        g, w = np.frombuffer(got, dtype=np.uint8).reshape(-1, 48)[:gn], np.frombuffer(want, dtype=np.uint8).reshape(-1, 48)[:wn]
        assert np.array_equal(g[:, 40:44], w[:, 40:44])                    # MultiplyColor bytes
        gf, wf = g[:, :40].copy().view(np.float32), w[:, :40].copy().view(np.float32)
        assert np.array_equal(gf[:, :2], wf[:, :2])                        # positions are copies: bit-equal, which also pins the order
        assert_close(gf, wf, "draw call floats", rtol=1e-6, atol=1e-6)
        # a capacity that cuts inside the ragged block of the first chunk: the total is still reported, the prefix is returned
        full_blocks = int((chunks[0][0][:1024 * (n // 1024), 3] > 0).sum())
        capacity = (full_blocks + live[0]) // 2
        assert full_blocks < capacity < live[0]
        got2, gn2 = sysm.readback(params, element_counts=elems, capacity=capacity)
        assert gn2 == gn
        assert np.array_equal(np.frombuffer(got2, dtype=np.uint8).reshape(-1, 48)[:capacity], g[:capacity])
        view = sysm.readback_view(params, element_counts=elems)
        assert view.shape == (gn, 12) and np.array_equal(view.view(np.uint8).reshape(-1, 48), g)
    finally:
        sysm.close(); eng.close()


@pytest.mark.parametrize("third", ["third chunk not examined", "all three chunks"])
@pytest.mark.parametrize("cs", [33, 48])
def test_particle_lights_with_a_ragged_last_block(ctx, oracle, cs, third):
    """particle_light_count/emit_kernel compact the live particles of each chunk into light records in 1 024-slot blocks; the records' order
    is the order of the fp32 sum per pixel, and every tile of this frame is lit by particles of every examined chunk."""
    w, h = 160, 112
    atlas, dfu = light_field()
    env = scenes.environment()
    chunks = particle_scene(cs, N_CHUNKS, w, h)
    quads = examined(cs)
    if third == "all three chunks":
        quads = [quads[1], quads[0], 5 * cs]
    params = lc.particle_light_params(2.0, 14.0, (0.9, 0.8, 0.7, 0.6), casts_shadows=True, ao_radius=4.0, ao_opacity=0.7, spec=(0.2, 0.3, 0.1), spec_power=3.0)
    ambient = (0.05, 0.06, 0.07, 1.0)
    eng = native.Engine(ctx, cs, scenes.randomness_table(7))
    sysm = native.System(eng)
    for c, planes in enumerate(chunks):
        sysm.add_chunk()
        sysm.upload(c, P, planes[0]); sysm.upload(c, RC, planes[3])
    sdf = native.DistanceFieldTexture(ctx, atlas, abi.SDF_UNORM16)
    lm = native.Lightmap(ctx, w, h, abi.LIGHTMAP_FLOAT4)
    try:
        native.render_sphere_lights(ctx, None, env, dfu, None, sdf, ambient, lm)
        stats = native.render_particle_lights(ctx, sysm, params, env, dfu, None, sdf, lm, quad_counts=quads, want_stats=True)
        got = lm.download()
        want = np.zeros((h, w, 4), np.float32)
        want[:] = ambient
        ostats = oracle.render_particle_lights(chunks, quads, params, env, dfu, None, oracle.make_texture(atlas, abi.SDF_UNORM16), want, want_stats=True)
        assert (stats.SdfSamples, stats.PixelLightPairs, stats.TracedPairs) == (ostats.SdfSamples, ostats.PixelLightPairs, ostats.TracedPairs)
        assert stats.TracedPairs > 1000
        assert_close(got, want, "lightmap")
        # the order of the records matters: tiles hold lit particles of every examined chunk
        shared = np.ones((h // 16) * (w // 16), bool)
        for c, q in enumerate(quads):
            if q:
                p = chunks[c][0][:q]
                lit = p[(p[:, 3] > 0) & (chunks[c][3][:q, 3] > 0)]
                tiles = (lit[:, 1].astype(np.int64) // 16) * (w // 16) + lit[:, 0].astype(np.int64) // 16
                shared &= np.bincount(tiles, minlength=shared.size)[:shared.size] > 0
        assert shared.sum() >= 10, int(shared.sum())
    finally:
        for x in (lm, sdf, sysm, eng):
            x.close()


@pytest.mark.parametrize("cs", [33, 48])
def test_rasteriser_with_a_ragged_last_block(ctx, oracle, cs):
    """raster_setup_kernel maps a global slot to its chunk with g / slots.  Unrotated, square-cornered, untextured sprites: sin / cos are
    exactly 0 and 1 on both sides and no pow runs, so coverage is the same IEEE arithmetic on device and oracle -- compare_images'
    allowance for pixels on a rotated edge is zero here, and the shaded-pixel counts are equal."""
    w, h = 333, 197          # not multiples of the 16-pixel tile
    chunks = random_chunks(40, cs, N_CHUNKS, w, h, size_hi=14.0)
    for planes in chunks:
        planes[4][:, 1] = 0.0
    params = scenes.rasterize_params(size=(1.0, 0.6), global_color=(0.9, 0.8, 1.0, 0.7), origin=(3.0, -2.0), scale=(1.1, 0.9), size_from_z=0.05, z_to_y=0.25,
                                     rounded=False, viewport_scale=(1.0, 1.0), viewport_position=(2.0, 1.0), blend=abi.BLEND_ALPHA)
    quads = examined(cs)
    clear = (0.05, 0.1, 0.15, 0.2)
    got, (live, pairs, shaded) = render_gpu(ctx, chunks, cs, params, w, h, abi.LIGHTMAP_FLOAT4, clear, quad_counts=quads)
    want = np.zeros((h, w, 4), np.float32); want[:] = clear
    want, (olive, oshaded) = oracle.render_particles(chunks, params, w, h, quad_counts=quads, image=want)
    assert live == olive and live > sum(quads) // 3
    assert shaded == oshaded and shaded > 20 * live
    assert pairs >= live
    compare_images(got, want, "float4 target", max_outliers=0)
    assert (np.abs(want - np.asarray(clear, np.float32)).max(axis=-1) > 1e-3).mean() > 0.5
