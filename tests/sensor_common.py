"""Particle sensors (PS_CollectParticles, CollectParticles.fx:10-38): the numpy statement of the pass condition and the builder of
the chunks the sensor tests count over.

A slot is counted if and only if
    checkCategoryFilter(velocity.w, CategoryFilter)                                                  (:22)
    position.w > 1                                                                                   (:32, life against ONE)
    1 - saturate(evaluateByTypeId(AreaType, position, AreaCenter, AreaSize, AreaRotation) / AreaFalloff) > 0.01      (:27-32)
with saturate(NaN) = 0.  The distance comes from oracle.evaluate_area (the C restatement the kernels are held to) and, independently, from
tests/golden/second_reading.py's evaluate_by_type_id.

The threshold is sharp and device and CPU distances may differ in their last bits, so no test may hold a slot whose CPU value of
1 - saturate(d / falloff) lies within BAND = 1e-3 of 0.01 -- ten times the project's 1e-4 float criterion at d / falloff ~ 0.99.  The
builder resamples such positions; check_case asserts, on the CPU and for every slot, that the band is empty and that both readings give
the same mask.  Then counts are compared exactly and no slot is left out of a comparison."""
import functools

import numpy as np

from illuminant_amd import abi, scenes
from tests.test_second_reading import second

F = np.float32
THRESHOLD = F(0.01)
BAND = 1e-3

# straddling the life test: dead, alive but not above one, exactly one, the next float, above
LIVES = np.array([0.0, 0.5, 1.0, np.nextafter(F(1), F(2)), 1.5, 30.0], F)
# the filter every filtered sensor below uses, and categories on and beside both of its bounds
FILTER = (1.0, 3.0)
CATEGORIES = np.array([0.0, np.nextafter(F(1), F(0)), 1.0, np.nextafter(F(1), F(2)), 2.0, np.nextafter(F(3), F(0)), 3.0, np.nextafter(F(3), F(4)), 5.0], F)
EVERY_CATEGORY = (-9999.0, 9999.0)

CENTER = (100.0, 120.0, 16.0)
# positions are drawn from this box: it holds every area below with its falloff shell and a margin outside of it
POS_LO, POS_HI = (20.0, 40.0, -34.0), (180.0, 200.0, 66.0)


def sensor(type_id, center=CENTER, size=(30.0, 24.0, 12.0), falloff=16.0, rotation=0.0, category_filter=FILTER, strength=1.0):
    """An IlmAreaParams as ParticleAreaTransform.SetParameters fills it (ParticleTransform.cs:294-318); the falloff is taken as given
    (0 with type 0 is the effect default)."""
    a = abi.AreaParams()
    a.AreaType = type_id
    a.Strength = strength
    a.AreaFalloff = falloff
    a.AreaRotation = rotation
    for i in range(3):
        a.AreaCenter[i] = center[i]
        a.AreaSize[i] = size[i]
    a.CategoryFilter[0], a.CategoryFilter[1] = category_filter
    return a


def standard_sensors(rotation=0.5):
    """One sensor per area type 0..5 -- type 0 with the effect default AreaFalloff = 0 (0 / 0) -- then a filter that passes nothing and an
    unrotated box without a filter: eight, the most one call takes."""
    return [sensor(0, falloff=0.0),
            sensor(1, size=(34.0, 22.0, 14.0), falloff=20.0, rotation=rotation),
            sensor(2, size=(30.0, 24.0, 12.0), falloff=16.0, rotation=rotation),
            sensor(3, size=(18.0, 14.0, 15.0), falloff=12.0, rotation=rotation, category_filter=EVERY_CATEGORY),
            sensor(4, size=(28.0, 16.0, 10.0), falloff=18.0, rotation=0.45),
            sensor(5, size=(26.0, 20.0, 11.0), falloff=14.0, rotation=rotation),
            sensor(2, falloff=16.0, category_filter=(7.0, 6.0)),
            sensor(2, center=(90.0, 125.0, 10.0), size=(40.0, 12.0, 20.0), falloff=25.0, category_filter=EVERY_CATEGORY)]


def scaled_distance(a, distance):
    """1 - saturate(distance / AreaFalloff) in float32, saturate(NaN) = 0 (CollectParticles.fx:30)."""
    with np.errstate(all="ignore"):
        q = (np.asarray(distance, F) / F(a.AreaFalloff)).astype(F)
    s = np.where(np.isnan(q), F(0), np.minimum(np.maximum(q, F(0)), F(1))).astype(F)
    return (F(1) - s).astype(F)


def oracle_distance(oracle, a, pos):
    c, s = tuple(a.AreaCenter), tuple(a.AreaSize)
    return np.array([oracle.evaluate_area(int(a.AreaType), p[:3], c, s, float(a.AreaRotation)) for p in pos], F)


def second_distance(a, pos):
    return second.evaluate_by_type_id(int(a.AreaType), np.ascontiguousarray(pos[:, :3], F), np.array(tuple(a.AreaCenter), F), np.array(tuple(a.AreaSize), F),
                                      F(a.AreaRotation))


def mask(a, pos, vel, scaled):
    """The three conditions, slot by slot."""
    category = (vel[:, 3] >= F(a.CategoryFilter[0])) & (vel[:, 3] <= F(a.CategoryFilter[1]))
    return category & (pos[:, 3] > F(1)) & (scaled > THRESHOLD)


def in_band(scaled):
    return np.abs(scaled.astype(np.float64) - float(THRESHOLD)) < BAND


def check_case(oracle, sensors, chunks):
    """The CPU side of every sensor test, before the GPU is touched: for every sensor and every slot of every chunk (chunks: [(pos, vel)])
    the band around the threshold is empty and both readings of the distance functions give the same mask.  Returns the counts,
    (sensors, chunks) uint32."""
    counts = np.zeros((len(sensors), len(chunks)), np.uint32)
    for k, a in enumerate(sensors):
        for c, (pos, vel) in enumerate(chunks):
            s1, s2 = scaled_distance(a, oracle_distance(oracle, a, pos)), scaled_distance(a, second_distance(a, pos))
            assert not in_band(s1).any() and not in_band(s2).any(), "sensor %d, chunk %d: a slot within %g of the threshold" % (k, c, BAND)
            m1, m2 = mask(a, pos, vel, s1), mask(a, pos, vel, s2)
            assert np.array_equal(m1, m2), "sensor %d, chunk %d: the oracle and the second reading disagree on %d slots" % (k, c, int((m1 != m2).sum()))
            counts[k, c] = int(m1.sum())
    return counts


def draw_positions(seed, n):
    """Half of the positions from the whole box, half from the middle of it (where the areas are)."""
    u = np.stack([scenes.uniform(seed + 7 * k, (n,), -1.0, 1.0) for k in range(3)], axis=1)
    u[scenes.uniform(seed + 29, (n,)) < 0.5] *= F(0.4)
    lo, hi = np.array(POS_LO, F), np.array(POS_HI, F)
    return ((lo + hi) * F(0.5) + u * (hi - lo) * F(0.5)).astype(F)


def build_chunk(oracle, seed, n, sensors, advance=None):
    """(pos, vel) of n slots: positions inside, in the falloff shell and outside of every area of `sensors`, lives and categories cycling
    through LIVES and CATEGORIES (in a seeded order, so a wave holds every combination).  advance(pos, vel) -> (pos, vel): the state the
    sensors will see when that is not the uploaded one (a step in between); the band is kept empty on THAT state.  Positions whose
    value lies in the band of any sensor are drawn again."""
    pos, vel = np.zeros((n, 4), F), np.zeros((n, 4), F)
    pos[:, :3] = draw_positions(seed, n)
    pos[:, 3] = LIVES[(scenes.uniform(seed + 31, (n,)) * len(LIVES)).astype(np.int64) % len(LIVES)]
    vel[:, :3] = scenes.uniform(seed + 37, (n, 3), -30.0, 30.0)
    vel[:, 3] = CATEGORIES[(scenes.uniform(seed + 41, (n,)) * len(CATEGORIES)).astype(np.int64) % len(CATEGORIES)]
    for attempt in range(1, 50):
        seen_pos, _ = advance(pos.copy(), vel.copy()) if advance is not None else (pos, vel)
        bad = np.zeros(n, bool)
        for a in sensors:
            bad |= in_band(scaled_distance(a, oracle_distance(oracle, a, seen_pos))) | in_band(scaled_distance(a, second_distance(a, seen_pos)))
        if not bad.any():
            break
        pos[bad, :3] = draw_positions(seed + 1000 * attempt, n)[bad]
    else:
        raise AssertionError("the band around the threshold could not be emptied")
    return pos, vel


def classes(oracle, a, pos):
    """How many positions lie inside the area, in its falloff shell (counted by the third condition) and outside of it."""
    d = oracle_distance(oracle, a, pos)
    s = scaled_distance(a, d)
    return int((d <= 0).sum()), int(((d > 0) & (s > THRESHOLD)).sum()), int((s <= THRESHOLD).sum())


@functools.lru_cache(maxsize=None)
def _standard_case(oracle, cs, n_chunks, seed):
    sensors = standard_sensors()
    chunks = [build_chunk(oracle, seed + 100 * c, cs * cs, sensors) for c in range(n_chunks)]
    for pos, vel in chunks:
        pos.setflags(write=False); vel.setflags(write=False)
    return sensors, chunks, check_case(oracle, sensors, chunks)


def standard_case(oracle, cs, n_chunks, seed=500):
    """(sensors, chunks, counts) of the standard sensors over n_chunks chunks of cs x cs slots: built and checked once, shared, read-only."""
    return _standard_case(oracle, cs, n_chunks, seed)
