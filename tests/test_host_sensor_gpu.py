"""Transforms.Sensor in the host mirror (Transforms.cs:374-486) through pybind: sensors in a system's transform list are skipped by the
step, evaluated on the state ParticleSystem.Update leaves (ilm_system_sense_async) and delivered by ParticleSystem.AfterFrame.

The state evolves on the device, so the numpy statement (tests/sensor_common.py) is applied to the DOWNLOADED state: the kernel saw
exactly those positions, lives and categories.  The particles sit in two clusters -- deep inside the sensors' areas and far outside of
them -- and every test asserts that no slot lies in the band around the threshold before it compares counts exactly."""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, scenes
from tests import sensor_common as sc
from tests.test_host_gpu import H, hctx, make_engine          # noqa: F401 (fixtures)
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

P, V, A, RC, RD = abi.PLANE_POSITION, abi.PLANE_VELOCITY, abi.PLANE_ATTRIBUTES, abi.PLANE_RENDER_COLOR, abi.PLANE_RENDER_DATA
CS = 20
N = CS * CS
CENTER = (100.0, 120.0, 16.0)


def particles():
    """Two chunks: slots alternate between a cluster around CENTER (at most 20 from it on every axis) and one 200 and more away in x;
    lives on both sides of one, categories 0 and 2."""
    pos, vel, attr = scenes.make_particles(91, 2 * N, pos_lo=(80, 100, 4), pos_hi=(120, 140, 28), vel=40.0, life=(0.6, 2.5), categories=(0.0, 2.0))
    pos[1::2, 0] += np.float32(250.0)
    return pos, vel, attr


def build(H, hctx, with_sensors, n_sensors=2):
    engine, tp, rnd = make_engine(H, hctx, CS)
    cfg = H.ParticleSystemConfiguration()
    cfg.Friction = 0.1; cfg.MaximumVelocity = 2048.0; cfg.LifeDecayPerSecond = 1.5
    ps = H.ParticleSystem(engine, cfg)
    ps.BlockingLivenessReadback = True
    ps.BlockingSensorReadback = True
    ps.Spawn(2 * N, *particles())
    sp = H.Spawner(3)
    sp.MinRate, sp.MaxRate = 2000.0, 4000.0
    f = H.Formula3(); f.Constant = list(CENTER); f.RandomScale = [8, 8, 8]; f.Type = H.FormulaType.Spherical
    sp.Position = f
    g = H.Formula3(); g.RandomScale = [30, 30, 30]; g.Type = H.FormulaType.Spherical
    sp.Velocity = g
    life = H.Formula1(); life.Constant = 0.8; life.RandomScale = 1.5
    sp.Life = life
    gr = H.Gravity(); gr.MaximumAcceleration = 256.0
    a = H.Attractor(); a.Position = [110.0, 110.0, 10.0]; a.Radius = 60.0; a.Strength = 200.0; a.Type = H.AttractorType.Linear
    gr.Attractors = [a]
    sensors = []
    for k in range(n_sensors if with_sensors else 0):
        s = H.Sensor()
        if k % 2 == 0:           # a rotated box with a filter
            area = H.TransformArea()
            area.Type = H.AreaType.Box; area.Center = list(CENTER); area.Size = [30.0 + k, 30.0 + k, 30.0 + k]; area.Falloff = 16.0; area.Rotation = 0.5
            s.Area = area
            s.CategoryFilter = [1.0, 3.0]
        else:                    # no area: every slot the filter and the life keep
            s.CategoryFilter = [-1.0, 0.5 + k]
        s.Strength = 3.0 + k     # takes no part
        sensors.append(s)
    # the sensors sit between the other transforms: the step's op list must not see them
    transforms = [sp] + sensors[:1] + [gr] + sensors[1:]
    for t in transforms:
        ps.AddTransform(t)
    return engine, tp, ps, sensors, (sp, gr)


def area_params(sensor):
    return abi.AreaParams.from_buffer_copy(sensor.GetAreaParams())


def downloaded(ps):
    return [(ps.Readback(c, P), ps.Readback(c, V)) for c in range(len(ps.Chunks))]


def numpy_counts(oracle, sensors, ps):
    """check_case on the downloaded state: the band is empty, the two readings agree, the counts summed over the chunks."""
    return sc.check_case(oracle, [area_params(s) for s in sensors], downloaded(ps)).sum(axis=1).astype(np.int64).tolist()


def test_counts_follow_the_exchange_rule_frame_by_frame(H, hctx, oracle):
    """Spawner, Gravity and two Sensors, three Updates: after every AfterFrame Count is the numpy count of the state that Update left and
    PreviousCount is the Count of the frame before (Transforms.cs:473); the planes equal those of the same system without sensors."""
    engine, tp, ps, sensors, (sp, _) = build(H, hctx, True)
    engine0, tp0, ps0, _, _ = build(H, hctx, False)
    assert [s.IsAnalyzer for s in sensors] == [True, True] and not sp.IsAnalyzer
    p0 = area_params(sensors[0])
    assert p0.AreaType == 2 and p0.AreaFalloff == 16.0 and p0.AreaRotation == 0.5 and tuple(p0.CategoryFilter) == (1.0, 3.0) and p0.Strength == 3.0
    p1 = area_params(sensors[1])
    assert p1.AreaType == 0 and p1.AreaFalloff == 0.0 and tuple(p1.CategoryFilter) == (-1.0, 1.5)
    history = [[0, 0]]
    for frame in range(3):
        for clock, system in ((tp, ps), (tp0, ps0)):
            clock.Advance(1.0 / 60.0)
            system.Update(frame)
            system.AfterFrame()
        d = abi.StepDesc.from_buffer_copy(ps.LastStepBytes())
        assert d.OpCount == 1 and d.Ops[0].Type == abi.OP_GRAVITY          # the sensors are no ops
        assert bytes(ps.LastStepBytes()) == bytes(ps0.LastStepBytes())
        hctx.Sync()
        want = numpy_counts(oracle, sensors, ps)
        assert [s.Count for s in sensors] == want, (frame, [s.Count for s in sensors], want)
        assert [s.PreviousCount for s in sensors] == history[-1], frame
        history.append(want)
    assert all(0 < c < 2 * N + sp.TotalSpawned for c in history[-1]) and history[1] != history[3] and sp.TotalSpawned > 0
    assert len(ps.Chunks) == len(ps0.Chunks)
    for c in range(len(ps.Chunks)):
        for plane in (P, V, A, RC, RD):
            assert_bits_equal(ps.Readback(c, plane), ps0.Readback(c, plane), "chunk %d plane %d with and without the sensors" % (c, plane))


def test_an_inactive_sensor_zeroes_and_reset_clears(H, hctx, oracle):
    """Nine sensors (two groups: eight counted at once, one queued).  Inactive: PreviousCount = exchange(Count, 0) (Transforms.cs:440), and
    again at the next AfterFrame; active again it counts again; Reset() clears both counts."""
    engine, tp, ps, sensors, _ = build(H, hctx, True, n_sensors=9)
    tp.Advance(1.0 / 60.0); ps.Update(0); ps.AfterFrame(); hctx.Sync()
    first = numpy_counts(oracle, sensors, ps)
    assert [s.Count for s in sensors] == first and all(c > 0 for c in first) and len(set(first)) > 2
    assert [s.PreviousCount for s in sensors] == [0] * 9
    sensors[2].IsActive = False
    sensors[8].IsActive2 = False
    tp.Advance(1.0 / 60.0); ps.Update(1); ps.AfterFrame(); hctx.Sync()
    second = numpy_counts(oracle, sensors, ps)
    for k, s in enumerate(sensors):
        if k in (2, 8):
            assert (s.Count, s.PreviousCount) == (0, first[k])
        else:
            assert (s.Count, s.PreviousCount) == (second[k], first[k])
    tp.Advance(1.0 / 60.0); ps.Update(2); ps.AfterFrame(); hctx.Sync()
    assert (sensors[2].Count, sensors[2].PreviousCount) == (0, 0)
    sensors[2].IsActive = True
    sensors[8].IsActive2 = True
    tp.Advance(1.0 / 60.0); ps.Update(3); ps.AfterFrame(); hctx.Sync()
    fourth = numpy_counts(oracle, sensors, ps)
    assert [s.Count for s in sensors] == fourth and sensors[2].PreviousCount == 0 and sensors[2].Count > 0
    sensors[0].Reset()
    assert (sensors[0].Count, sensors[0].PreviousCount) == (0, 0) and sensors[1].Count == fourth[1]
    # a frame without an Update delivers nothing: an active sensor keeps both counts
    before = [(s.Count, s.PreviousCount) for s in sensors]
    ps.AfterFrame()
    assert [(s.Count, s.PreviousCount) for s in sensors] == before
