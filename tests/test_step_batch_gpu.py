"""ilm_engine_step_batch: a list of (system, descriptor) items stepped in one call must leave what ilm_system_step item by item leaves.

Twins throughout: two engines get the same randomness table and the same uploads; one is stepped item by item, the other with the batch.
Afterwards all 20 component planes (5 float4 planes) of every chunk are compared on their raw bits, and with them the counts the steps
publish, their readiness, and what later calls see of System::used and the render-plane records (a later step, an erase, a re-upload).
"""
import os

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes

pytestmark = pytest.mark.gpu

P, V, A, RC, RD = abi.PLANE_POSITION, abi.PLANE_VELOCITY, abi.PLANE_ATTRIBUTES, abi.PLANE_RENDER_COLOR, abi.PLANE_RENDER_DATA
PLANES = (P, V, A, RC, RD)
STEP_KERNEL_BATCH = 5        # ILM_STEP_KERNEL_BATCH of include/illuminant_hip.h (tests/test_step_batch_abi.py holds the value)
SERIAL, BATCH = 0, 1


@pytest.fixture(scope="module")
def rnd():
    return scenes.randomness_table(23)


@pytest.fixture(scope="module")
def small_field():
    """A 64 x 64 x 32 UNORM16 field (3 slices, one atlas cell) with the particle demo's obstacles scaled into it."""
    layout = scenes.DistanceFieldLayout(64, 64, 32.0, 3, 1.0, 128)
    atlas = scenes.build_sdf_atlas(layout, scenes.simple_particles_obstacles(64.0, 64.0), fmt=abi.SDF_UNORM16)
    return atlas, layout.uniforms(packed1=False)


class Twins:
    """Two engines with the same content: side SERIAL is stepped with ilm_system_step, side BATCH with ilm_engine_step_batch."""

    def __init__(self, ctx, cs, rnd):
        self.ctx, self.cs, self.n = ctx, cs, cs * cs
        self.engines = [native.Engine(ctx, cs, rnd), native.Engine(ctx, cs, rnd)]
        self.systems = [[], []]
        self.closers = []

    def system(self, chunks=(), seed=1, **particles):
        """A system on both sides; chunks = the used slots of each chunk (uploaded from one seeded particle set).  Returns its index."""
        total = sum(chunks)
        pos, vel, attr = scenes.make_particles(seed, max(total, 1), **particles)
        for side in (SERIAL, BATCH):
            s = native.System(self.engines[side])
            at = 0
            for c, used in enumerate(chunks):
                s.add_chunk()
                if used:
                    s.upload(c, P, pos[at:at + used]); s.upload(c, V, vel[at:at + used]); s.upload(c, A, attr[at:at + used])
                at += used
            self.systems[side].append(s)
        return len(self.systems[SERIAL]) - 1

    def both(self, index, fn):
        for side in (SERIAL, BATCH):
            fn(self.systems[side][index])

    def frame(self, items):
        """items = [(system index, build)]; build(systems of the side) -> abi.StepDesc (handles in a descriptor differ by side)."""
        for index, build in items:
            self.systems[SERIAL][index].step(build(self.systems[SERIAL]))
        self.engines[BATCH].step_batch([self.systems[BATCH][index] for index, _ in items], [build(self.systems[BATCH]) for _, build in items])
        return self.engines[BATCH].last_step_batch()

    def download(self, side):
        return [[[s.download(c, plane) for plane in PLANES] for c in range(s.chunk_count())] for s in self.systems[side]]

    def check(self, what):
        a, b = self.download(SERIAL), self.download(BATCH)
        for i, (sa, sb) in enumerate(zip(a, b)):
            assert len(sa) == len(sb)
            for c, (ca, cb) in enumerate(zip(sa, sb)):
                for plane, (pa, pb) in zip(PLANES, zip(ca, cb)):
                    same = pa.view(np.uint32) == pb.view(np.uint32)
                    assert same.all(), "%s: system %d chunk %d plane %d: %d of %d words differ between the steps one by one and the batch (first at %s)" % (
                        what, i, c, plane, int((~same).sum()), same.size, tuple(np.argwhere(~same)[0]))
        for i, (sa, sb) in enumerate(zip(self.systems[SERIAL], self.systems[BATCH])):
            assert np.array_equal(sa.live_counts(), sb.live_counts()), "%s: live counts of system %d" % (what, i)

    def check_step_counts(self, index, what):
        a, b = self.systems[SERIAL][index], self.systems[BATCH][index]
        self.ctx.sync()
        ra, rb = a.poll_counts(), b.poll_counts()
        assert (ra is None) == (rb is None), "%s: readiness of the counts of system %d" % (what, index)
        ca, cb = a.step_counts(), b.step_counts()
        assert np.array_equal(ca, cb), "%s: step counts of system %d: %s one by one, %s batched" % (what, index, ca, cb)
        if ra is not None:
            assert np.array_equal(ra, ca) and np.array_equal(rb, cb)
        return cb

    def close(self):
        for fn in self.closers:
            fn()
        for side in (SERIAL, BATCH):
            for s in self.systems[side]:
                s.close()
            self.engines[side].close()


ATTRACTORS = [((60., 70., 0.), 40., 500., 0), ((200., 60., 10.), 90., 700., 1), ((100., 210., 0.), 120., 900., 2), ((220., 200., 5.), 3., 300., 0)]


def base(cs, mode=abi.UPDATE_POSITIONS, first=0, count=-1, flags=0, **uniforms):
    d = abi.StepDesc()
    d.FirstChunk, d.ChunkCount = first, count
    d.System = scenes.system_uniforms(cs, **dict(dict(friction=0.05, max_velocity=900.0, life_decay=4.0), **uniforms))
    d.Update = abi.UpdateParams.default()
    d.UpdateMode = mode
    d.Flags = flags
    return d


def add_op(d, kind, params):
    d.Ops[d.OpCount].Type = kind
    setattr(d.Ops[d.OpCount].u, {abi.OP_GRAVITY: "Gravity", abi.OP_NOISE: "Noise", abi.OP_FMA: "FMA", abi.OP_MATRIX_MULTIPLY: "MatrixMultiply",
                                  abi.OP_SPATIAL_NOISE: "SpatialNoise"}[kind], params)
    d.OpCount += 1
    return d


def gravity(d, n=4):
    return add_op(d, abi.OP_GRAVITY, scenes.gravity_params(ATTRACTORS[:n], maximum_acceleration=64.0))


def noise(d, area=None):
    return add_op(d, abi.OP_NOISE, scenes.noise_params(area or scenes.area_none(), (0.37 * 253, 0.81 * 127), (0.12 * 253, 0.55 * 127), 0.35))


def spawner(d, cs, chunk, first, last, k=0):
    r = d.Spawns[d.SpawnCount]
    r.ChunkIndex = chunk
    r.Kind = abi.SPAWN_INLINE
    r.Params = scenes.spawn_params(cs, first, last, 17 * k, (0.3 * 253, 0.6 * 127), position=((128, 128, 0), (100, 90, 4), (0, 0, 0), scenes.FORMULA_SPHERICAL),
                                   velocity=((0, 0, 0), (60, 60, 10), (0, 0, 0), scenes.FORMULA_SPHERICAL), life=(1.0, 2.0, 0.0))
    d.SpawnCount += 1
    return d


def feedback(d, cs, chunk, first, last, source_handle, source_chunk=0):
    r = d.Spawns[d.SpawnCount]
    r.ChunkIndex = chunk
    r.Kind = abi.SPAWN_FEEDBACK
    r.Params = scenes.spawn_params(cs, first, last, 0, (0.2 * 253, 0.7 * 127), position=((0, 0, 0), (2, 2, 0), (0, 0, 0), scenes.FORMULA_LINEAR),
                                   velocity=((0, 0, 0), (5, 5, 0), (0, 0, 0), scenes.FORMULA_LINEAR), life=(1.5, 0.0, 0.0))
    r.Feedback = scenes.feedback_params(source_handle, source_chunk, 3, 2, 0.5, source_life_range=(0.2, 9999.0))
    d.SpawnCount += 1
    return d


def mixed_bag(t, cs, small_field, ctx, spawn_first):
    """The seven systems of the issue (and an eighth without chunks between two of them) with the descriptor builder of each."""
    n = cs * cs
    atlas, dfu = small_field
    live = dict(life=(0.02, 2.5), dead_fraction=0.2)
    items = []
    # gravity only
    items.append((t.system((n,), 1, **live), lambda s: gravity(base(cs))))
    # Noise + FMA with a box area and a category filter
    box = scenes.area(2, (128.0, 128.0, 0.0), (90.0, 70.0, 40.0), falloff=8.0, strength=0.8, category_filter=(1.0, 3.0))
    items.append((t.system((n,), 2, categories=(0.0, 2.0), **live),
                  lambda s: add_op(noise(base(cs), scenes.area_none()), abi.OP_FMA,
                                   scenes.fma_params(box, position_add=(0.5, -0.25, 0.0), position_multiply=(1.001, 0.999, 1.0), velocity_add=(0.0, 1.5, 0.0),
                                                     velocity_multiply=(0.98, 0.97, 1.0)))))
    # MatrixMultiply + SpatialNoise: the extended variant
    rot = abi.Matrix.from_rows([[0.99, 0.1, 0, 0], [-0.1, 0.99, 0, 0], [0, 0, 1, 0], [0.5, 0.25, 0, 1]])
    spatial = scenes.spatial_noise_params(scenes.noise_params(scenes.area_none(), (0.3 * 253, 0.6 * 127), (0.8 * 253, 0.1 * 127), 0.4, replace_old_velocity=False), (3.0, 2.0))
    items.append((t.system((n,), 3, **live),
                  lambda s: add_op(add_op(base(cs), abi.OP_MATRIX_MULTIPLY, scenes.matrix_multiply_params(scenes.area_none(0.7), rot, rot)), abi.OP_SPATIAL_NOISE, spatial)))
    # a system without chunks, between two others
    items.append((t.system((), 4), lambda s: gravity(base(cs))))
    # two chunks, the step covers the second alone
    items.append((t.system((n, n), 5, **live), lambda s: noise(gravity(base(cs, first=1, count=1), 2))))
    # a partly used spawn-target chunk with an inline spawner
    used = spawn_first - 24
    items.append((t.system((n, used), 6, **live), lambda s: spawner(noise(gravity(base(cs))), cs, 1, spawn_first, spawn_first + n // 8)))
    # the collision update on a small UNORM16 field
    sdf = native.DistanceFieldTexture(ctx, atlas, abi.SDF_UNORM16)
    t.closers.append(sdf.close)
    i = t.system((n,), 7, pos_lo=(-4, -4, 0), pos_hi=(68, 68, 16), vel=40.0, **live)
    t.both(i, lambda s: s.set_distance_field(sdf))

    def collide(s):
        d = gravity(base(cs, mode=abi.UPDATE_WITH_DISTANCE_FIELD, collision=(128.0, 0.6, 0.33, 0.4)), 1)
        d.DistanceField = dfu
        return d
    items.append((i, collide))
    # a life ramp, counting
    ramp = scenes.uniform(77, (8, 16, 4))
    i = t.system((n,), 8, **live)
    t.both(i, lambda s: s.set_life_ramp(ramp))

    def ramped(s):
        d = gravity(base(cs, flags=abi.STEP_COUNT_LIVE))
        d.Update.LifeRampSettings = abi.f4(-0.7, 0.5, 4.0, 8.0)
        return d
    items.append((i, ramped))
    return items


@pytest.mark.parametrize("cs,spawn_first", [(16, 120), (64, 1000)])
def test_a_mixed_bag_of_systems(ctx, rnd, small_field, cs, spawn_first):
    """Every kernel variant side by side, at the smallest grid (chunk size 16: 256 slots) and at 64 (Noise's fast tables, several blocks
    per chunk, the bucket counters, and a spawner whose first slot rotates the blocks of an item that does not start the grid)."""
    t = Twins(ctx, cs, rnd)
    try:
        items = mixed_bag(t, cs, small_field, ctx, spawn_first)
        counting = items[-1][0]
        for frame in range(3):
            launches, rounds, fallback = t.frame(items)
            assert rounds == 1 and fallback == 0, (launches, rounds, fallback)
            # plain, extended, collision, spawning: the empty system launches nothing
            assert launches == 4, launches
            t.check_step_counts(counting, "frame %d" % frame)
        t.check("mixed bag, chunk size %d" % cs)
    finally:
        t.close()


def test_items_that_depend_on_each_other_run_in_order(ctx, rnd):
    cs = 64
    n = cs * cs
    live = dict(life=(0.5, 2.5), dead_fraction=0.2)
    t = Twins(ctx, cs, rnd)
    try:
        # one system twice: spawn only, then transforms + update over what was spawned
        a = t.system((n, 512), 11, **live)
        launches, rounds, fallback = t.frame([(a, lambda s: spawner(base(cs, mode=abi.UPDATE_NONE), cs, 1, 600, 1400)),
                                              (a, lambda s: noise(gravity(base(cs, flags=abi.STEP_COUNT_LIVE))))])
        assert (launches, rounds, fallback) == (2, 2, 0)
        t.check_step_counts(a, "one system twice")
        # a feedback spawner whose source is stepped by an EARLIER item: it must read the stepped source
        src = t.system((n,), 12, **live)
        dst = t.system((n, 0), 13, **live)
        step_source = (src, lambda s: gravity(base(cs)))
        feed = (dst, lambda s: feedback(gravity(base(cs), 1), cs, 1, 64, 700, s[src].handle.value))
        launches, rounds, fallback = t.frame([step_source, feed])
        assert (rounds, fallback) == (2, 0)
        # ... and by a LATER item: it must read the source before that item rewrites it
        launches, rounds, fallback = t.frame([(dst, lambda s: feedback(gravity(base(cs), 1), cs, 1, 701, 1500, s[src].handle.value)), step_source])
        assert (rounds, fallback) == (2, 0)
        # independent items beside a dependent pair share the first round
        other = t.system((n,), 14, **live)
        launches, rounds, fallback = t.frame([step_source, (other, lambda s: gravity(base(cs))), feed])
        assert (launches, rounds, fallback) == (2, 2, 0)
        t.check("dependent items")
    finally:
        t.close()


def test_homogeneous_systems_share_one_launch(ctx, rnd):
    """What a loop over ilm_system_step cannot do: 70 systems, one launch."""
    cs = 64
    n = cs * cs
    t = Twins(ctx, cs, rnd)
    try:
        items = [(t.system((n,), 100 + k, life=(0.02, 2.5), dead_fraction=0.2), lambda s: noise(gravity(base(cs)))) for k in range(70)]
        assert t.frame(items) == (1, 1, 0)
        assert native.lib().ilm_debug_last_step_kernel() == STEP_KERNEL_BATCH
        # two variants in one round: the first five systems also spawn
        spawning = [(i, lambda s: spawner(noise(gravity(base(cs))), cs, 0, 2000, 2600)) for i, _ in items[:5]]
        assert t.frame(spawning + items[5:]) == (2, 1, 0)
        assert native.lib().ilm_debug_last_step_kernel() == STEP_KERNEL_BATCH
        t.check("70 systems")
        # an empty batch is no batch: nothing happens, the diagnostic keeps the last one
        t.engines[BATCH].step_batch([], [])
        assert t.engines[BATCH].last_step_batch() == (2, 1, 0)
    finally:
        t.close()


def test_counting_items_publish_the_counts_of_their_own_steps(ctx, rnd):
    cs = 64
    n = cs * cs
    live = dict(life=(0.05, 0.4), dead_fraction=0.3)       # lives that run out within the frames: the counts move
    t = Twins(ctx, cs, rnd)
    try:
        counted = [t.system((n, n, 700), 21, **live), t.system((n,), 22, **live)]
        plain = t.system((n,), 23, **live)
        count = lambda s: gravity(base(cs, flags=abi.STEP_COUNT_LIVE, life_decay=9.0))
        items = [(counted[0], count), (plain, lambda s: gravity(base(cs, life_decay=9.0))), (counted[1], count)]
        seen = []
        for frame in range(2):          # both parities of the counter regions
            assert t.frame(items) == (1, 1, 0)
            for i in counted:
                got = t.check_step_counts(i, "frame %d" % frame)
                assert np.array_equal(got, t.systems[BATCH][i].live_counts())
                seen.append(got.copy())
        assert not np.array_equal(seen[0], seen[2]), "the scene is meant to lose particles between the frames"
        # a chunk leaves and another arrives; the next batch counts straight away
        t.both(counted[0], lambda s: s.remove_chunk(1))
        t.both(counted[0], lambda s: s.add_chunk())
        pos, vel, attr = scenes.make_particles(24, 900, **live)
        t.both(counted[0], lambda s: (s.upload(2, P, pos), s.upload(2, V, vel), s.upload(2, A, attr)))
        assert t.frame(items) == (1, 1, 0)
        for i in counted:
            got = t.check_step_counts(i, "after the chunk table changed")
            assert np.array_equal(got, t.systems[BATCH][i].live_counts())
        t.check("counting")
    finally:
        t.close()


def test_later_calls_see_the_state_a_loop_of_steps_leaves(ctx, rnd):
    """System::used and the render-plane records after a batch: a plain step, an erase and a re-upload give the twin's bits."""
    cs = 64
    n = cs * cs
    live = dict(life=(0.5, 2.5), dead_fraction=0.2)
    t = Twins(ctx, cs, rnd)
    try:
        a = t.system((n, 300), 31, **live)
        b = t.system((n,), 32, **live)
        step_a = lambda s: spawner(noise(gravity(base(cs))), cs, 1, 320, 900)
        step_b = lambda s: gravity(base(cs))
        # (a plain step first: the item-by-item side's lean kernel records its render planes as current; the batch clears such records)
        for i, build in ((a, step_a), (b, step_b)):
            t.both(i, lambda s: s.step(build(None)))
        t.frame([(a, step_a), (b, step_b)])
        t.frame([(a, step_a), (b, step_b)])
        for i, build in ((a, step_a), (b, step_b)):
            t.both(i, lambda s: s.step(build(None)))
            t.both(i, lambda s: s.step(build(None)))
        t.check("a step after the batch")
        # erase in a batch, then spawn into the erased chunk with a plain step: `used` starts from zero on both sides
        t.frame([(a, lambda s: base(cs, mode=abi.UPDATE_ERASE, first=1, count=1)), (b, step_b)])
        t.both(a, lambda s: s.step(spawner(gravity(base(cs)), cs, 1, 10, 200)))
        pos, vel, attr = scenes.make_particles(33, 500, **live)
        t.both(b, lambda s: (s.upload(0, P, pos, 100), s.upload(0, V, vel, 100), s.upload(0, A, attr, 100)))
        t.frame([(a, step_a), (b, step_b)])
        t.both(b, lambda s: s.step(step_b(None)))
        t.check("erase and re-upload")
    finally:
        t.close()


def test_items_launched_one_by_one_keep_the_contract(ctx, rnd, small_field):
    """ILM_STEP_STREAMING=1 (read per step) sends every range to the streaming kernels, which the batch kernel does not cover."""
    cs = 64
    t = Twins(ctx, cs, rnd)
    os.environ["ILM_STEP_STREAMING"] = "1"
    try:
        items = mixed_bag(t, cs, small_field, ctx, 1000)
        for frame in range(2):
            launches, rounds, fallback = t.frame(items)
            assert (launches, rounds, fallback) == (0, 1, len(items) - 1)     # all but the system without chunks, which launches nothing
        t.check_step_counts(items[-1][0], "one by one")
        t.check("items launched one by one")
    finally:
        del os.environ["ILM_STEP_STREAMING"]
        t.close()


class Refusal:
    """A batch that must be refused as a whole: planes and counts of every listed system before and after."""

    def __init__(self, ctx, rnd):
        cs = self.cs = 64
        n = cs * cs
        self.t = t = Twins(ctx, cs, rnd)
        self.items = [(t.system((n,), 41 + k, life=(0.5, 2.5), dead_fraction=0.2), lambda s: gravity(base(cs, flags=abi.STEP_COUNT_LIVE))) for k in range(4)]
        t.frame(self.items)

    def refused(self, systems, descs, code, item):
        t = self.t
        before = t.download(BATCH)
        counts = [s.step_counts().copy() for s in t.systems[BATCH]]
        with pytest.raises(native.IlluminantError) as err:
            t.engines[BATCH].step_batch(systems, descs)
        assert err.value.code == code, str(err.value)
        assert "item %d:" % item in str(err.value), str(err.value)
        after = t.download(BATCH)
        for sa, sb in zip(before, after):
            for ca, cb in zip(sa, sb):
                for pa, pb in zip(ca, cb):
                    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), "a refused batch changed a plane"
        for s, c in zip(t.systems[BATCH], counts):
            assert np.array_equal(s.step_counts(), c) and np.array_equal(s.live_counts(), c)
        # and the batch side still steps like its twin
        t.frame(self.items)
        for i, _ in self.items:
            t.check_step_counts(i, "after the refusal")
        t.check("after the refusal")


def test_a_system_of_another_engine_is_refused(ctx, rnd):
    r = Refusal(ctx, rnd)
    try:
        t = r.t
        systems = [t.systems[BATCH][0], t.systems[BATCH][1], t.systems[SERIAL][2], t.systems[BATCH][3]]     # the twin's engine is another engine
        r.refused(systems, [gravity(base(r.cs)) for _ in systems], abi.ERR_INVALID_ARGUMENT, 2)
    finally:
        r.t.close()


def test_an_item_with_too_many_ops_is_refused(ctx, rnd):
    r = Refusal(ctx, rnd)
    try:
        t = r.t
        descs = [gravity(base(r.cs, flags=abi.STEP_COUNT_LIVE)) for _ in range(4)]
        descs[2].OpCount = abi.MAX_OPS + 1
        with pytest.raises(native.IlluminantError) as alone:
            t.systems[BATCH][2].step(descs[2])
        assert alone.value.code == abi.ERR_TOO_MANY
        r.refused(t.systems[BATCH][:4], descs, alone.value.code, 2)
    finally:
        r.t.close()


def test_a_feedback_record_naming_a_dead_handle_is_refused(ctx, rnd):
    r = Refusal(ctx, rnd)
    try:
        t = r.t
        gone = native.System(t.engines[BATCH])
        dead = gone.handle.value
        gone.close()
        descs = [gravity(base(r.cs, flags=abi.STEP_COUNT_LIVE)) for _ in range(4)]
        descs[1] = feedback(gravity(base(r.cs)), r.cs, 0, 64, 700, dead)
        with pytest.raises(native.IlluminantError) as alone:
            t.systems[BATCH][1].step(descs[1])
        assert alone.value.code == abi.ERR_INVALID_HANDLE
        r.refused(t.systems[BATCH][:4], descs, alone.value.code, 1)
    finally:
        r.t.close()
