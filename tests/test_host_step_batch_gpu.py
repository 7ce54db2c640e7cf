"""ParticleEngine.UpdateSystems of the host mirror: a frame's Update loop over the systems of an engine submitted as one
ilm_engine_step_batch.  Twins: six systems on one engine updated through UpdateSystems, six built the same way on a second engine
updated one Update at a time; after 10 frames -- liveness counts and a reap among them -- the planes are equal bit for bit and the
mirror's own bookkeeping is the same.
"""
import numpy as np
import pytest

from illuminant_amd import abi, scenes

pytestmark = pytest.mark.gpu

PLANES = (abi.PLANE_POSITION, abi.PLANE_VELOCITY, abi.PLANE_ATTRIBUTES, abi.PLANE_RENDER_COLOR, abi.PLANE_RENDER_DATA)
CS = 64
N = CS * CS


@pytest.fixture(scope="module")
def H():
    from illuminant_amd import _host
    return _host


@pytest.fixture(scope="module")
def hctx(H):
    return H.DeviceContext(0)


def inline_spawner(H, seed, rate, centre):
    sp = H.Spawner(seed)
    sp.MinRate, sp.MaxRate = rate * 0.5, rate * 1.5
    f = H.Formula3(); f.Constant = list(centre); f.RandomScale = [90, 60, 4]; f.Type = H.FormulaType.Spherical
    sp.Position = f
    g = H.Formula3(); g.RandomScale = [60, 60, 10]; g.Type = H.FormulaType.Spherical
    sp.Velocity = g
    life = H.Formula1(); life.Constant = 0.2; life.RandomScale = 2.0
    sp.Life = life
    return sp


def gravity(H):
    gr = H.Gravity(); gr.MaximumAcceleration = 1024.0
    atts = []
    for (p, r, s) in (((400., 300., 0.), 70., 600.), ((900., 500., 0.), 100., 1500.)):
        a = H.Attractor(); a.Position = list(p); a.Radius = r; a.Strength = s; a.Type = H.AttractorType.Linear
        atts.append(a)
    gr.Attractors = atts
    return gr


def build(H, hctx):
    """One engine with the six systems; returns (engine, time provider, systems, everything that must stay alive)."""
    tp = H.ManualTimeProvider()
    ecfg = H.ParticleEngineConfiguration(CS)
    ecfg.TimeProvider = tp
    engine = H.ParticleEngine(hctx, ecfg, scenes.randomness_table(7))
    keep = []

    def system(decay=1.5, transforms=()):
        cfg = H.ParticleSystemConfiguration()
        cfg.Friction = 0.1; cfg.MaximumVelocity = 2048.0; cfg.LifeDecayPerSecond = decay
        ps = H.ParticleSystem(engine, cfg)
        ps.BlockingLivenessReadback = True
        for t in transforms:
            ps.AddTransform(t)
        keep.extend(transforms)
        return ps
    systems = []
    # two systems with inline spawners
    systems.append(system(transforms=(inline_spawner(H, 3, 40000.0, (500, 300, 0)), gravity(H), H.Noise(9))))
    systems.append(system(transforms=(inline_spawner(H, 4, 9000.0, (200, 200, 0)), H.Noise(10))))
    # uploaded particles that die within a few frames: their chunk is counted empty and reaped during the run
    dying = system(decay=4.0, transforms=(gravity(H),))
    dying.DeadFrameThreshold = 1
    pos, vel, attr = scenes.make_particles(78, N, pos_hi=(1000, 600, 32), life=(0.01, 0.1))
    dying.Spawn(N, pos, vel, attr)
    systems.append(dying)
    # a position-buffer spawner (8 positions > 4 inline): its buffer is bound again every frame
    sp = inline_spawner(H, 5, 3000.0, (100, 100, 0))
    sp.MinRate = sp.MaxRate = 3000.0
    sp.RatePerPosition = False
    sp.AdditionalPositions = [[100.0 + 40.0 * i, 100.0 + 25.0 * (i % 3), float(i)] for i in range(1, 8)]
    sp.PolygonRate = 3.0
    mm = H.MatrixMultiply()
    mm.Strength = 0.5
    mm.Velocity = [0.95, 0, 0, 0, 0, 0.95, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    systems.append(system(decay=1.0, transforms=(sp, mm)))
    # a feedback pair: the source is updated before its consumer
    src_spawner = inline_spawner(H, 2, 1200.0, (200, 100, 5))
    src_spawner.MinRate = src_spawner.MaxRate = 1200.0
    src = system(decay=0.5, transforms=(src_spawner,))
    fb = H.FeedbackSpawner(6)
    fb.SourceSystem = src
    fb.MinRate = fb.MaxRate = 1800.0
    fb.InstanceMultiplier = 3
    fb.SourceVelocityFactor = 0.5
    fb.MultiplyLife = True
    pf = H.Formula3(); pf.Constant = [0, 0, 1]; pf.RandomScale = [2, 2, 0]; pf.Type = H.FormulaType.Spherical
    fb.Position = pf
    lf = H.Formula1(); lf.Constant = 0.5
    fb.Life = lf
    dst = system(decay=0.5, transforms=(fb,))
    systems += [src, dst]
    return engine, tp, systems, keep


def last_step(ps):
    """The last descriptor with the handles in it blanked (they differ between the twins by construction)."""
    d = abi.StepDesc.from_buffer_copy(ps.LastStepBytes())
    for k in range(abi.MAX_SPAWNS):
        d.Spawns[k].Feedback.SourceSystem = 0
    return bytes(d)


def test_update_systems_equals_a_loop_of_updates(H, hctx):
    one_by_one = build(H, hctx)
    batched = build(H, hctx)
    chunk_counts = []
    for frame in range(10):
        for engine, tp, systems, _ in (one_by_one, batched):
            tp.Advance(1.0 / 60.0)
        results_a = [ps.Update(frame) for ps in one_by_one[2]]
        results_b = batched[0].UpdateSystems(batched[2], frame)
        assert [(r.PerformedUpdate, r.Timestamp) for r in results_a] == [(r.PerformedUpdate, r.Timestamp) for r in results_b]
        for i, (a, b) in enumerate(zip(one_by_one[2], batched[2])):
            what = "frame %d system %d" % (frame, i)
            assert a.LiveCount == b.LiveCount, what
            assert a.TotalSpawnCount == b.TotalSpawnCount, what
            assert [(c.ID, c.NextSpawnOffset, c.TotalSpawned) for c in a.Chunks] == [(c.ID, c.NextSpawnOffset, c.TotalSpawned) for c in b.Chunks], what
            assert last_step(a) == last_step(b), what
        chunk_counts.append(len(batched[2][2].Chunks))
    hctx.Sync()
    assert chunk_counts[0] == 1 and chunk_counts[-1] == 0, "the dying system's chunk is meant to be reaped during the run: %s" % chunk_counts
    assert batched[2][0].TotalSpawnCount > 0 and len(batched[2][5].Chunks) > 0
    for i, (a, b) in enumerate(zip(one_by_one[2], batched[2])):
        assert len(a.Chunks) == len(b.Chunks)
        for ci in range(len(a.Chunks)):
            for plane in PLANES:
                pa, pb = a.Readback(ci, plane), b.Readback(ci, plane)
                same = pa.view(np.uint32) == pb.view(np.uint32)
                assert same.all(), "system %d chunk %d plane %d: %d words differ between Update one by one and UpdateSystems" % (i, ci, plane, int((~same).sum()))
    # a second update in one frame is refused with the same words, and the refusal leaves no launch behind
    with pytest.raises(Exception) as alone:
        one_by_one[2][0].Update(9)
    with pytest.raises(Exception) as together:
        batched[0].UpdateSystems(batched[2], 9)
    assert str(alone.value) == str(together.value) and "Cannot update twice in a single frame" in str(together.value)
    for engine, tp, systems, _ in (one_by_one, batched):
        tp.Advance(1.0 / 60.0)
    for ps in one_by_one[2]:
        ps.Update(10)
    batched[0].UpdateSystems(batched[2], 10)
    hctx.Sync()
    for i, (a, b) in enumerate(zip(one_by_one[2], batched[2])):
        for ci in range(len(a.Chunks)):
            pa, pb = a.Readback(ci, abi.PLANE_POSITION), b.Readback(ci, abi.PLANE_POSITION)
            assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), "system %d chunk %d after the refused frame" % (i, ci)
