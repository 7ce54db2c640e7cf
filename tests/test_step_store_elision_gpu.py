"""step_lean_kernel stores a plane only where some lane changed it, and leaves the render colour / render data planes of a render-current
chunk alone where it can prove that they keep their bits (csrc/particles.hip, store_changed_render_planes; the per-chunk records in
csrc/api.hip, System::render_gen).  After every step every plane must hold what the interpreting kernel -- which stores everything --
leaves there.  Each test runs one script of steps and writes twice: on a system stepped by the lean kernel and on a twin stepped by the
interpreter (ilm_debug_step_interpreter), then compares all five planes of every chunk bit for bit and the live counts.
The elision belongs to the HBM-resident (STREAM) variant; these systems are small, so ILM_STEP_STREAMING=1 selects it.
"""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

P, V, A, RC, RD = abi.PLANE_POSITION, abi.PLANE_VELOCITY, abi.PLANE_ATTRIBUTES, abi.PLANE_RENDER_COLOR, abi.PLANE_RENDER_DATA
PLANES = (P, V, A, RC, RD)
NAN, INF = np.float32(np.nan), np.float32(np.inf)


@pytest.fixture(autouse=True)
def streaming_variant(monkeypatch):
    monkeypatch.setenv("ILM_STEP_STREAMING", "1")


def opacity_from_life(o=2.5):
    """ParticleColor.OpacityFromLife as the host class binds it: a linear, clamped ColorFromLife that saturates at life >= o."""
    return abi.ClampedBezier4(abi.f4(0.0, 1.0 / o, 2, 0), abi.f4(1, 1, 1, 0), abi.f4(1, 1, 1, 1), abi.f4(0, 0, 0, 0), abi.f4(0, 0, 0, 0))


def bezier4(count, mode, lo, hi):
    return abi.ClampedBezier4(abi.f4(lo, 1.0 / (hi - lo), count, mode), abi.f4(1.0, 0.2, 0.1, 1.0), abi.f4(0.4, 0.9, 0.3, 0.8),
                              abi.f4(0.1, 0.5, 1.0, 0.5), abi.f4(0.9, 0.1, 0.6, 0.2))


def bezier1(count, mode, lo, hi):
    return abi.ClampedBezier1(abi.f4(lo, 1.0 / (hi - lo), count, mode), abi.f4(0.5, 2.0, 1.25, 3.0))


def update_params(**k):
    """The bench's update pass (OpacityFromLife 2.5, every other curve constant) with the named parts replaced."""
    u = abi.UpdateParams.default()
    u.ColorFromLife = opacity_from_life()
    for name, value in k.items():
        if name == "rotation_from_life":
            u.RotationFromLifeAndIndex[0] = value
        elif name == "rotation_from_index":
            u.RotationFromLifeAndIndex[1] = value
        else:
            setattr(u, name, value)
    return u


def step_desc(cs, update=None, ops=("gravity", "noise"), rotation=False, life_decay=0.01, spawns=(), revive=False, count=True):
    d = abi.StepDesc()
    d.FirstChunk, d.ChunkCount = 0, -1
    d.System = scenes.system_uniforms(cs, friction=0.02, max_velocity=2048.0, life_decay=life_decay, rotation_from_velocity=rotation)
    d.Update = update if update is not None else update_params()
    d.OpCount = len(ops)
    for o, kind in enumerate(ops):
        if kind == "gravity":
            d.Ops[o].Type = abi.OP_GRAVITY
            d.Ops[o].u.Gravity = scenes.gravity_params([((60., 70., 0.), 40., 500., 1), ((200., 60., 10.), 90., 700., 1), ((100., 210., 0.), 120., 900., 2)],
                                                       maximum_acceleration=64.0)
        elif kind == "noise":
            d.Ops[o].Type = abi.OP_NOISE
            # PositionScale.w != 0 lets Noise change the life of dead slots: that step is the interpreter's
            position = ((-0.5,) * 4, (0,) * 4, (0, 0, 0, 0.5 if revive else 0))
            d.Ops[o].u.Noise = scenes.noise_params(scenes.area_none(), (0.37 * 253, 0.81 * 127), (0.12 * 253, 0.55 * 127), 0.35, position=position)
        elif kind == "fma":
            d.Ops[o].Type = abi.OP_FMA
            d.Ops[o].u.FMA = scenes.fma_params(scenes.area_none(), position_add=(0.5, -0.25, 0.0), velocity_multiply=(0.98, 0.97, 1.0))
    d.UpdateMode = abi.UPDATE_POSITIONS
    d.Flags = abi.STEP_COUNT_LIVE if count else 0
    for s, (chunk, first, last) in enumerate(spawns):
        d.Spawns[s].ChunkIndex = chunk
        d.Spawns[s].Params = scenes.spawn_params(cs, first, last, 17 * s, (0.3 * 253, 0.6 * 127),
                                                 position=((128, 128, 0), (100, 90, 4), (0, 0, 0), scenes.FORMULA_SPHERICAL),
                                                 velocity=((0, 0, 0), (60, 60, 10), (0, 0, 0), scenes.FORMULA_SPHERICAL), life=(3.0, 2.0, 0.0))
        d.SpawnCount = s + 1
    return d


def particles(seed, n, life=(50.0, 90.0), dead_fraction=0.1, specials=True):
    """Bench-like particles; with `specials`, lanes with NaN / +-inf / -0.0 in life, velocity, category and attributes."""
    pos, vel, attr = scenes.make_particles(seed, n, life=life, dead_fraction=dead_fraction, categories=(0.0, 1.0, 2.0))
    if specials and n >= 1024:
        odd = (NAN, INF, -INF, np.float32(-0.0), np.float32(1e-30))
        for k, x in enumerate(odd):
            pos[100 + k, 3] = x                       # life
            vel[200 + k, k % 3] = x                   # one velocity component
            vel[300 + k, 3] = x                       # category
            attr[400 + k, k % 4] = x                  # one attribute
            vel[500 + k, :3] = x                      # the whole velocity
        attr[600:664] = NAN                           # a whole wave of NaN attributes
        pos[700:764, 3] = -0.0                        # a whole wave of -0.0 lives (dead)
    return pos, vel, attr


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return h


def write_component(system, chunk, component, values):
    """A caller writing one component plane through ilm_chunk_device_ptr (host to device, after the library's queued work)."""
    ptr, _ = system.device_ptr(chunk, component)
    h = hip()
    assert h.hipDeviceSynchronize() == 0
    a = np.ascontiguousarray(values, np.float32)
    assert h.hipMemcpy(ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
    assert h.hipDeviceSynchronize() == 0


class Twins:
    """The same script on a lean-stepped system and an interpreter-stepped one."""

    def __init__(self, ctx, cs, n_chunks, seed=5, used=None, life=(50.0, 90.0), specials=True, engine_ctx=None):
        self.cs, self.n = cs, cs * cs
        self.rnd = scenes.randomness_table(11)
        self.eng = native.Engine(engine_ctx or ctx, cs, self.rnd)
        self.systems = [native.System(self.eng), native.System(self.eng)]    # [lean, interpreter]
        self.counts = [[], []]
        pos, vel, attr = particles(seed, self.n * n_chunks, life=life, specials=specials)
        used = used or [self.n] * n_chunks
        for s in self.systems:
            for c in range(n_chunks):
                s.add_chunk()
                sl = slice(c * self.n, c * self.n + used[c])
                s.upload(c, P, pos[sl]); s.upload(c, V, vel[sl]); s.upload(c, A, attr[sl])
        self.prev = native.lib().ilm_debug_step_interpreter(0)

    def step(self, d, n=1, lean_uses_interpreter=False):
        for _ in range(n):
            for i, s in enumerate(self.systems):
                native.lib().ilm_debug_step_interpreter(1 if (i == 1 or lean_uses_interpreter) else 0)
                s.step(d)
                if d.Flags & abi.STEP_COUNT_LIVE:
                    self.counts[i].append(s.step_counts().copy())
        native.lib().ilm_debug_step_interpreter(0)

    def both(self, fn):
        for s in self.systems:
            fn(s)

    def check(self, what):
        lean, interp = self.systems
        assert lean.chunk_count() == interp.chunk_count()
        for a, b in zip(*self.counts):
            assert np.array_equal(a, b), "%s: step counts %s vs %s" % (what, a, b)
        for c in range(lean.chunk_count()):
            for plane in PLANES:
                assert_bits_equal(lean.download(c, plane), interp.download(c, plane), "%s: chunk %d plane %d, lean vs interpreter" % (what, c, plane))
        assert np.array_equal(lean.live_counts(), interp.live_counts())

    def close(self):
        native.lib().ilm_debug_step_interpreter(self.prev)
        for s in self.systems:
            s.close()
        self.eng.close()


@pytest.mark.parametrize("streaming", ["1", "0"], ids=["HBM-resident variant", "cache-resident variant"])
@pytest.mark.parametrize("cs,n_chunks,used", [(64, 3, [4096, 4096, 1024]), (256, 8, None)], ids=["three chunks, one partly used", "two streams"])
def test_bench_like_steps_keep_every_bit(ctx, monkeypatch, cs, n_chunks, used, streaming):
    """The bench's update pass: from the second step on the render planes of living particles keep their bits and are not stored.
    256^2 x 8 chunks is large enough for the step to be split over the context's two streams."""
    monkeypatch.setenv("ILM_STEP_STREAMING", streaming)
    t = Twins(ctx, cs, n_chunks, used=used)
    try:
        d = step_desc(cs)
        t.step(d, 6)
        t.check("bench-like, 6 steps")
        t.step(step_desc(cs, count=False), 2)
        t.check("bench-like, 2 more without counting")
    finally:
        t.close()


def _upload(plane, chunk=1, first=512, count=1024):
    def fn(t):
        pos, vel, attr = particles(99, count, life=(0.5, 4.0), specials=False)
        data = {P: pos, V: vel, A: attr, RC: attr[::-1] * 0.5, RD: pos[::-1] * 0.25}[plane]
        t.both(lambda s: s.upload(chunk, plane, data, first_slot=first))
    return fn


def _device_ptr(component):
    def fn(t):
        rng = np.random.default_rng(component)
        values = rng.uniform(0.0, 3.0, t.n).astype(np.float32)
        t.both(lambda s: write_component(s, 0, component, values))
    return fn


def _transform_only(t):
    g = scenes.gravity_params([((90., 90., 0.), 60., 800., 1)], maximum_acceleration=32.0)
    sys = scenes.system_uniforms(t.cs, life_decay=0.01)
    t.both(lambda s: s.gravity(1, sys, g))


def _interpreter_step(t):
    t.step(step_desc(t.cs), 1, lean_uses_interpreter=True)


def _erase_and_upload(t):
    pos, vel, attr = particles(123, t.n, life=(1.0, 60.0), specials=False)

    def fn(s):
        s.erase(1)
        s.upload(1, P, pos[:3000]); s.upload(1, V, vel[:3000]); s.upload(1, A, attr[:3000])
    t.both(fn)


def _remove_and_add(t):
    pos, vel, attr = particles(321, t.n, life=(10.0, 60.0), specials=False)

    def fn(s):
        s.remove_chunk(0)
        k = s.add_chunk()                     # the engine's pool hands the released buffer back
        s.upload(k, P, pos[:2048]); s.upload(k, V, vel[:2048]); s.upload(k, A, attr[:2048])
    t.both(fn)


WRITERS = {
    "upload P": _upload(P), "upload V": _upload(V), "upload A": _upload(A), "upload RC": _upload(RC), "upload RD": _upload(RD),
    "device pointer, life": _device_ptr(3), "device pointer, render colour": _device_ptr(12), "device pointer, attribute": _device_ptr(9),
    "transform-only pass": _transform_only,
    "interpreter step": _interpreter_step,
    "erase, re-upload": _erase_and_upload,
    "remove, add (reused buffer)": _remove_and_add,
}


@pytest.mark.parametrize("name", list(WRITERS))
def test_every_other_writer_ends_the_render_record(ctx, name):
    cs = 64
    t = Twins(ctx, cs, 3)
    try:
        d = step_desc(cs)
        t.step(d, 3)
        WRITERS[name](t)
        t.step(d, 4)
        t.check(name)
    finally:
        t.close()


def test_gathered_chunks_end_the_render_record(ctx):
    """ilm_group_gather_chunks writes Pos+Life into a system that has been stepped: its next steps must recompute the render planes."""
    cs = 64
    g = native.Group([0])
    t = Twins(ctx, cs, 2, engine_ctx=g.contexts[0])
    src = native.System(t.eng)
    try:
        pos, vel, attr = particles(77, 2 * t.n, life=(0.5, 80.0), specials=False)
        for c in range(2):
            src.add_chunk()
            src.upload(c, P, pos[c * t.n:(c + 1) * t.n])
        d = step_desc(cs)
        t.step(d, 3)
        for s in t.systems:
            g.gather_chunks([src], [s], 2, 0, 4, native.GATHER_PEER)
        g.sync()
        t.step(d, 4)
        t.check("gathered Pos+Life")
    finally:
        src.close()
        t.close()
        g.close()


KEY_CHANGES = {
    "ColorFromLife": dict(ColorFromLife=bezier4(4, 1, 0.0, 120.0)),
    "OpacityFromLife": dict(ColorFromLife=opacity_from_life(75.0)),
    "ColorFromVelocity": dict(ColorFromVelocity=bezier4(2, 512 + 1, 0.0, 80.0)),
    "SizeFromLife": dict(SizeFromLife=bezier1(3, 256 + 2, 0.0, 100.0)),
    "SizeFromVelocity": dict(SizeFromVelocity=bezier1(2, 0, 0.0, 90.0)),
    "RotationFromLife": dict(rotation_from_life=0.25),
    "RotationFromIndex": dict(rotation_from_index=0.001),
    "RotationFromVelocity": dict(rotation=True),
}


@pytest.mark.parametrize("name", list(KEY_CHANGES))
def test_a_new_render_key_stores_everything_again(ctx, name):
    cs = 64
    change = dict(KEY_CHANGES[name])
    rotation = change.pop("rotation", False)
    t = Twins(ctx, cs, 3)
    try:
        t.step(step_desc(cs), 3)
        t.check("before the change")
        other = step_desc(cs, update=update_params(**change), rotation=rotation)
        t.step(other, 3)
        t.check("after changing %s" % name)
        t.step(step_desc(cs), 2)
        t.check("back to the first key")
    finally:
        t.close()


def test_dying_reviving_and_spawning_particles(ctx):
    """Lives that cross OpacityFromLife and zero mid-run, a Noise that revives dead slots (an interpreter step), spawns into render-current
    chunks, and every curve non-constant with rotation from life and index."""
    cs = 64
    t = Twins(ctx, cs, 3, life=(0.01, 3.0))
    try:
        dying = step_desc(cs, life_decay=30.0)
        t.step(dying, 4)
        t.check("dying")
        t.step(step_desc(cs, life_decay=30.0, revive=True), 1)
        t.step(dying, 3)
        t.check("after a reviving Noise")
        spawning = step_desc(cs, life_decay=2.0, spawns=((2, 100, 1500), (0, 4000, 4095)))
        t.step(spawning, 4)
        t.check("spawning")
        curves = update_params(ColorFromLife=bezier4(4, 1, 0.0, 2.5), ColorFromVelocity=bezier4(3, 256 + 2, 0.0, 120.0),
                               SizeFromLife=bezier1(2, 512 + 1, 0.0, 2.5), SizeFromVelocity=bezier1(4, 0, 0.0, 120.0),
                               rotation_from_life=0.7, rotation_from_index=0.001)
        t.step(step_desc(cs, update=curves, life_decay=0.5, ops=("fma", "gravity")), 5)
        t.check("non-constant curves")
    finally:
        t.close()


def test_a_chunk_handed_out_by_pointer_still_matches(ctx):
    """A chunk whose device pointer was handed out never elides its render planes again, whatever the caller writes later."""
    cs = 64
    t = Twins(ctx, cs, 2)
    try:
        d = step_desc(cs)
        t.step(d, 2)
        t.both(lambda s: s.device_ptr(1, 0))
        t.step(d, 2)
        _device_ptr(16)(t)          # render data x of chunk 0
        _device_ptr(14)(t)
        t.step(d, 3)
        t.check("after writes through the pointer")
    finally:
        t.close()
