"""The clamp class of the lean step leaves the category plane alone in a chunk whose category record -- the bounds of its categories, found
once by category_bounds_kernel (csrc/particles.hip) and kept per chunk by the host (csrc/api.hip, System::cat_current) -- lies inside the
step's category filters.  A wave of such a chunk loads the plane only when it leaves the regular body.  Whatever the record says, every
plane must hold the bits the interpreting kernel leaves: each case steps a system by the default choice and a twin by the interpreter and
compares all planes of all chunks bit for bit, and holds the library's records (ilm_debug_chunk_category_bounds) and its three wave counts
(ilm_debug_step_category_waves) to the model of tests/category_record_common.py, step by step.

The shape is that of tests/test_step_regular_waves_gpu.py: chunk size 64, two chunks, five steps, Gravity + Noise + UpdatePositions with
filters (0, 1) and (-1, 0.5) -- the intersection is 0 .. 0.5 -- so that the class runs from the second step on.
"""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import native, scenes
from tests.category_record_common import RecordTwins, EVERY
from tests.step_regular_common import desc, regular_particles, slot, PLACES, LEAN, LEAN_CLAMP, N, CHUNKS, STEPS, WAVES, NAN, DECAY, CS
from tests.test_step_store_elision_gpu import P, V, A, hip

pytestmark = pytest.mark.gpu
CLASS = [LEAN] + [LEAN_CLAMP] * (STEPS - 1)


@pytest.fixture(autouse=True)
def streaming_variant(monkeypatch):
    monkeypatch.setenv("ILM_STEP_STREAMING", "1")


def particles(categories=(0.0, 0.25, 0.5), **k):
    """Regular particles whose categories are spread over `categories`, each value present in each chunk."""
    pos, vel, attr = regular_particles(**k)
    rng = np.random.default_rng(3)
    vel[:, 3] = np.asarray(categories, np.float32)[rng.integers(len(categories), size=len(vel))]
    for c in range(len(vel) // N):
        vel[c * N + 70:c * N + 70 + len(categories), 3] = categories
    return pos, vel, attr


def run(ctx, what, parts, descs, used=None, also=None):
    t = RecordTwins(ctx, *parts, used=used)
    try:
        for d in descs:
            t.step(d)
        t.check(what)
        if also is not None:
            also(t)
    finally:
        t.close()
    return t


def test_all_categories_inside_the_filter(ctx):
    parts = particles()
    t = run(ctx, "all inside", parts, [desc()] * STEPS)
    assert t.kernels == CLASS
    assert t.category_waves == [(0, 0, 0)] + [(WAVES, 0, 0)] * (STEPS - 1)
    for c in range(CHUNKS):
        lo, hi, current = t.records[-1][c]
        assert (lo, hi, current) == (np.float32(0.0), np.float32(0.5), 1)
        assert (lo, hi) == (parts[1][c * N:(c + 1) * N, 3].min(), parts[1][c * N:(c + 1) * N, 3].max())
    assert t.records[0] == [(0.0, 0.0, 0)] * CHUNKS       # the first step is the general instantiation's: nothing was scanned


def test_one_category_outside_the_filter_in_chunk_1(ctx):
    parts = particles()
    parts[1][slot(PLACES[2]), 3] = 0.75
    t = run(ctx, "one outside", parts, [desc()] * STEPS)
    assert t.kernels == CLASS
    assert t.category_waves[1:] == [(WAVES // 2, 0, WAVES // 2)] * (STEPS - 1)
    assert t.records[-1] == [(0.0, 0.5, 1), (0.0, 0.75, 1)]


def test_a_nan_category_admits_nobody(ctx):
    parts = particles()
    parts[1][slot(PLACES[0]), 3] = NAN
    parts[1][slot(PLACES[3]), 3] = NAN
    t = run(ctx, "NaN category", parts, [desc()] * STEPS)
    assert t.kernels == CLASS
    assert t.category_waves[1:] == [(0, 0, WAVES)] * (STEPS - 1)
    for c in range(CHUNKS):
        lo, hi, current = t.records[-1][c]
        assert np.isnan(lo) and hi == np.float32(0.5) and current == 1


UP, DOWN = np.float32(np.inf), np.float32(-np.inf)
EDGES = {
    # name: (categories, Gravity's filter; Noise accepts everything), every wave skipped?
    "bounds equal to min and max": ((0.125, 0.25, 0.375), (0.125, 0.375), True),
    "lower bound one ulp inside": ((0.125, 0.25, 0.375), (np.nextafter(np.float32(0.125), UP), 0.375), False),
    "upper bound one ulp inside": ((0.125, 0.25, 0.375), (0.125, np.nextafter(np.float32(0.375), DOWN)), False),
    "category -0.0 against a bound of +0.0": ((-0.0, 0.25), (0.0, 1.0), True),
    "category +0.0 against a bound of -0.0": ((0.0, 0.25), (-0.0, 1.0), True),
    "NaN lower filter bound": ((0.125, 0.25), (float("nan"), 1.0), False),
    "NaN upper filter bound": ((0.125, 0.25), (0.0, float("nan")), False),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_filter_bound_edges(ctx, name):
    categories, gravity_filter, skipped = EDGES[name]
    d = desc((("gravity", dict(filter=gravity_filter)), ("noise", dict(filter=EVERY))))
    t = run(ctx, name, particles(categories), [d] * STEPS)
    assert t.kernels == CLASS
    assert t.category_waves[1:] == [(WAVES, 0, 0) if skipped else (0, 0, WAVES)] * (STEPS - 1)
    assert all(current == 1 for _, _, current in t.records[-1])


EXCLUDES_ZERO = (("gravity", dict(filter=(0.125, 1.0))), "noise")        # the intersection is 0.125 .. 0.5


def test_slots_dying_inside_a_proven_chunk(ctx):
    """Lanes 0, 31, 32 and 63 of four waves run out of life in the third step: their waves load the category late in that step (the second
    mask fails) and in every later one (the loaded mask is not full), the plane gets the dead slot's 0, and the record -- which speaks of
    live slots only -- stays what the scan found, under a filter that refuses 0."""
    parts = particles((0.25,))
    for place in PLACES:
        parts[0][slot(place), 3] = np.float32(2.5) * DECAY
    categories = []
    t = run(ctx, "dying slots", parts, [desc(EXCLUDES_ZERO)] * STEPS,
            also=lambda t: categories.extend(t.systems[0].download(chunk, V)[wave * 64 + lane, 3] for chunk, wave, lane in PLACES))
    assert t.kernels == CLASS
    k = len(PLACES)
    assert t.category_waves == [(0, 0, 0), (WAVES, 0, 0), (WAVES - k, k, 0), (WAVES - k, k, 0), (WAVES - k, k, 0)]
    assert t.waves == [(0, 0), (WAVES, 0), (WAVES - k, k), (WAVES - k, 0), (WAVES - k, 0)]
    assert t.records[-1] == [(0.25, 0.25, 1)] * CHUNKS
    assert len(categories) == k and all(category == 0.0 and not np.signbit(category) for category in categories)


@pytest.mark.parametrize("used", [1000, 64 * 15 + 1])
def test_a_partly_used_chunk(ctx, used):
    """The never-written slots past the high-water mark hold a category of 0 the filter refuses: the scan does not read them, the chunk is
    proven, and the wave the used slots end in -- its other lanes are dead -- loads the category late."""
    t = run(ctx, "partly used", particles((0.25, 0.375)), [desc(EXCLUDES_ZERO)] * STEPS, used=[N, used])
    assert t.kernels == CLASS
    assert t.category_waves[1:] == [(N // 64 + 15, 1, 0)] * (STEPS - 1)
    assert t.records[-1] == [(0.25, 0.375, 1)] * CHUNKS


def test_the_filter_narrows_between_steps(ctx):
    """No writer in between: the record stays current and is not scanned again; the device compare against the new filter fails it."""
    narrow = desc((("gravity", dict(filter=(0.25, 1.0))), "noise"))
    t = run(ctx, "narrower filter", particles(), [desc()] * 3 + [narrow] * 2 + [desc()])
    assert t.kernels == [LEAN] + [LEAN_CLAMP] * 5
    assert t.category_waves[1:] == [(WAVES, 0, 0)] * 2 + [(0, 0, WAVES)] * 2 + [(WAVES, 0, 0)]
    assert all(rec == [(0.0, 0.5, 1)] * CHUNKS for rec in t.records[1:])


# ---- writers between two clamp-class steps: afterwards a slot of chunk 1 has a category Gravity's filter refuses ------------------------
OUTSIDE = np.float32(2.0)
AT = 40 * 64 + 32        # the planted slot of the written chunk


def _planted(seed, count):
    pos, vel, attr = scenes.make_particles(seed, count, life=(50.0, 90.0), categories=(0.0, 0.5))
    vel[min(AT, count - 1), 3] = OUTSIDE
    return pos, vel, attr


def _upload_velocity(t):
    _, vel, _ = _planted(31, 1024)
    t.both(lambda s: s.upload(1, V, vel, first_slot=AT - 512))
    t.wrote(1)


def _erase_and_upload(t):
    pos, vel, attr = _planted(32, 3000)

    def fn(s):
        s.erase(1)
        s.upload(1, P, pos); s.upload(1, V, vel); s.upload(1, A, attr)
    t.both(fn)
    t.wrote(1, used=3000)


def _spawner_step(t):
    d = desc()
    d.Spawns[0].ChunkIndex = 1
    d.Spawns[0].Params = scenes.spawn_params(CS, 100, 300, 0, (0.3 * 253, 0.6 * 127), position=((128, 128, 0), (100, 90, 4), (0, 0, 0), scenes.FORMULA_SPHERICAL),
                                             velocity=((0, 0, 0), (60, 60, 10), (0, 0, 0), scenes.FORMULA_SPHERICAL), life=(70.0, 5.0, 0.0), category=(float(OUTSIDE), 0.0, 0.0))
    d.SpawnCount = 1
    t.step(d)


def _fma_step(t):
    # the FMA accepts every category and moves it up by two: no category passes Gravity's filter afterwards
    t.step(desc(("gravity", "noise", ("fma", dict(filter=EVERY, category=(1.0, float(OUTSIDE)))))))


def _remove_and_add(t):
    pos, vel, attr = _planted(33, N)

    def fn(s):
        s.remove_chunk(0)                   # chunk 1 becomes chunk 0 ...
        k = s.add_chunk()                   # ... and the engine's pool hands the released buffer back as chunk 1
        s.upload(k, P, pos); s.upload(k, V, vel); s.upload(k, A, attr)
    t.both(fn)
    t.wrote(0); t.wrote(1, used=N)


WRITERS = {"upload into a chunk": _upload_velocity, "erase and upload": _erase_and_upload, "a step with a spawner": _spawner_step,
           "a step with an FMA": _fma_step, "chunk removal and addition": _remove_and_add}


@pytest.mark.parametrize("name", list(WRITERS))
def test_a_writer_between_two_class_steps_ends_the_record(ctx, name):
    t = RecordTwins(ctx, *particles())
    try:
        t.step(desc(), 3)
        assert t.category_waves[-1] == (WAVES, 0, 0) and t.kernels[-1] == LEAN_CLAMP
        WRITERS[name](t)
        t.step(desc(), 3)
        t.check(name)
        # the written chunk was scanned again and no longer lies inside the filter: its waves load the category with the other planes
        assert t.kernels[-1] == LEAN_CLAMP and t.category_waves[-1][2] > 0
        assert any(current == 1 and hi > np.float32(0.5) for _, hi, current in t.records[-1])
    finally:
        t.close()


def test_the_group_chunk_exchange_ends_the_record(ctx):
    """ilm_group_gather_chunks at world 1 writes the velocity planes -- the category with them -- of both chunks."""
    g = native.Group([0])
    parts = particles()
    t = RecordTwins(g.contexts[0], *parts)
    src = native.System(t.eng)
    try:
        _, vel, _ = particles(seed=9)
        vel[AT, 3] = OUTSIDE
        for c in range(CHUNKS):
            src.add_chunk()
            src.upload(c, V, vel[c * N:(c + 1) * N])
        t.step(desc(), 3)
        assert t.category_waves[-1] == (WAVES, 0, 0)
        for s in t.systems:
            g.gather_chunks([src], [s], CHUNKS, 4, 4, native.GATHER_PEER)
        g.sync()
        t.wrote(0); t.wrote(1)
        t.step(desc(), 3)
        t.check("gathered velocity")
        assert t.category_waves[-1] == (WAVES // 2, 0, WAVES // 2)
        assert t.records[-1][0][1] == OUTSIDE
    finally:
        src.close()
        t.close()
        g.close()


# ---- systems that are never proven ----------------------------------------------------------------------------------------------------
def test_a_handed_out_chunk_pointer_leaves_no_record(ctx):
    t = RecordTwins(ctx, *particles())
    try:
        t.step(desc(), 3)
        t.both(lambda s: s.device_ptr(1, 7))
        t.wrote(1)
        t.step(desc(), 3)
        t.check("pointer handed out")
        # a launch over the chunk never elides, so the class never runs and nothing is scanned; chunk 0 keeps the record it had
        assert t.kernels == [LEAN, LEAN_CLAMP, LEAN_CLAMP, LEAN, LEAN, LEAN]
        assert [current for _, _, current in t.records[-1]] == [1, 0]
        assert t.category_waves[3:] == [(0, 0, 0)] * 3
    finally:
        t.close()


def test_a_captured_step_leaves_no_record():
    """A step captured into a graph: a replay would not keep the host's records, so from then on no chunk of the system is current.  (A
    context of its own: asking for the stream keeps every later step of a context on that stream.)"""
    ctx = native.Context(0)
    t = RecordTwins(ctx, *particles())
    h = hip()
    h.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    h.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    h.hipGraphInstantiate.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    h.hipGraphLaunch.argtypes = [C.c_void_p, C.c_void_p]
    h.hipGraphExecDestroy.argtypes = [C.c_void_p]
    h.hipGraphDestroy.argtypes = [C.c_void_p]
    try:
        t.step(desc(), 3)
        assert [current for _, _, current in t.records[-1]] == [1, 1]
        d = desc()
        d.Flags = 0
        ctx.sync()
        stream = C.c_void_p(ctx.stream())
        graph, executable = C.c_void_p(), C.c_void_p()
        assert h.hipStreamBeginCapture(stream, 2) == 0          # hipStreamCaptureModeRelaxed
        native.lib().ilm_debug_step_interpreter(0)
        t.systems[0].step(d)
        assert h.hipStreamEndCapture(stream, C.byref(graph)) == 0
        assert h.hipGraphInstantiate(C.byref(executable), graph, None, None, 0) == 0
        assert h.hipGraphLaunch(executable, stream) == 0
        ctx.sync()
        assert h.hipGraphExecDestroy(executable) == 0 and h.hipGraphDestroy(graph) == 0
        native.lib().ilm_debug_step_interpreter(1)
        t.systems[1].step(d)
        native.lib().ilm_debug_step_interpreter(0)
        t.read_category_waves()
        assert [t.record(c)[2] for c in range(CHUNKS)] == [0, 0]
        t.wrote(0); t.wrote(1)
        t.step(desc(), 3)
        t.check("after a captured step")
        assert t.kernels[3:] == [LEAN] * 3 and t.category_waves[3:] == [(0, 0, 0)] * 3
        assert [current for _, _, current in t.records[-1]] == [0, 0]
    finally:
        t.close()
        ctx.close()


# ---- the smallest step that is split over the context's two streams -----------------------------------------------------------------------
def test_the_smallest_split_step(ctx):
    """2 chunks of 512^2 are kSplitMinUnits units: each half of the step scans its own chunk on its own stream ahead of its launch (four
    workgroups of the scan per chunk).  Chunk 1 holds a category outside the filter.  The same script on one stream gives the same planes,
    records and counts."""
    cs, chunks = 512, 2
    n, waves = cs * cs, cs * cs // 64
    parts = particles(cs=cs, chunks=chunks)
    parts[1][1 * n + 3 * 65536 + 12345, 3] = 0.75
    planes, records, counts = [], [], []
    for streams in (2, 1):
        before = native.lib().ilm_debug_step_streams(streams)
        t = RecordTwins(ctx, *parts, cs=cs, chunks=chunks)
        try:
            t.step(desc(cs=cs), 3)
            t.check("%d stream(s)" % streams)
            assert t.kernels == [LEAN, LEAN_CLAMP, LEAN_CLAMP]
            assert t.category_waves[1:] == [((chunks - 1) * waves, 0, waves)] * 2
            planes.append([t.systems[0].download(c, plane) for c in range(chunks) for plane in (P, V)])
            records.append(t.records[-1]); counts.append(t.category_waves)
        finally:
            t.close()
            native.lib().ilm_debug_step_streams(before)
    assert records[0] == records[1] and counts[0] == counts[1]
    assert [r[2] for r in records[0]] == [1] * chunks and records[0][0][:2] == (0.0, 0.5) and records[0][1][:2] == (0.0, 0.75)
    for a, b in zip(*planes):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
