"""What tests/test_step_category_record_gpu.py shares: twins that, beside CountingTwins' bookkeeping, keep a MODEL of the per-chunk
category records (csrc/api.hip, System::cat_current) as the rule next to that field states it, read the library's own records
(ilm_debug_chunk_category_bounds) after every step, and count the clamp class's waves three ways (ilm_debug_step_category_waves) against
what the model and the interpreter twin's planes give.  No test lives here.

The model.  A chunk's record is None (not current) or the (lo, hi) numpy finds over the category of the chunk's used slots -- a NaN lo when
one is a NaN -- at the moment a clamp-class step without FMA first met the chunk without one.  A lean step with neither an FMA nor a
spawner keeps it; every other step forgets the records of its range; a test tells the model about every other writer (wrote).  A wave of a
clamp-class step over a chunk whose record lies inside the step's filter (float32 compares, so a NaN on either side fails) counts as
`skipped` when all 64 lanes are regular before and after the step, as `late` otherwise; every wave of another chunk, and of a step with an
FMA, counts as `upfront`.
"""
import ctypes as C

import numpy as np

from illuminant_amd import abi, native
from tests.step_regular_common import CountingTwins, category_bounds, has_fma, predict_waves, stepped_range, wave_masks, LEAN, LEAN_CLAMP, CS, CHUNKS, INF, NAN
from tests.test_step_store_elision_gpu import P, V

EVERY = (-INF, INF)


def numpy_bounds(categories):
    """(lo, hi) of a chunk's used categories as category_bounds_kernel states them."""
    c = np.asarray(categories, np.float32)
    nan = np.isnan(c)
    rest = c[~nan]
    lo = np.float32(rest.min()) if rest.size else INF
    hi = np.float32(rest.max()) if rest.size else -INF
    return (NAN if nan.any() else lo), hi


def same_bound(a, b):
    return (np.isnan(a) and np.isnan(b)) or np.float32(a) == np.float32(b)


def spawns_into(d, chunk_range):
    return any(d.Spawns[k].ChunkIndex in chunk_range and d.Spawns[k].Params.ChunkSizeAndIndices[2] >= d.Spawns[k].Params.ChunkSizeAndIndices[1]
               for k in range(d.SpawnCount))


class RecordTwins(CountingTwins):
    def __init__(self, ctx, pos, vel, attr, cs=CS, chunks=CHUNKS, used=None, rnd=None):
        super().__init__(ctx, pos, vel, attr, cs=cs, chunks=chunks, used=used, rnd=rnd)
        self.used = list(used or [self.n] * chunks)
        self.model = [None] * chunks
        self.category_waves, self.category_predicted = [], []        # per step: (skipped, late, upfront)
        self.records, self.models = [], []                            # per step: the library's [(lo, hi, current)], the model's copy
        native.check(native.lib().ilm_debug_step_category_waves(ctx.handle, 1, None, None, None))

    # -- the library's side
    def record(self, chunk, system=0):
        lo, hi, current = C.c_float(0), C.c_float(0), C.c_int32(-1)
        native.check(native.lib().ilm_debug_chunk_category_bounds(self.systems[system].handle, chunk, C.byref(lo), C.byref(hi), C.byref(current)))
        return np.float32(lo.value), np.float32(hi.value), int(current.value)

    def read_category_waves(self):
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        native.check(native.lib().ilm_debug_step_category_waves(self.ctx.handle, 1, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    # -- the model's side
    def wrote(self, chunk, used=None):
        """Another writer touched `chunk` (used: its high-water mark afterwards, where it moved)."""
        self.model[chunk] = None
        if used is not None:
            self.used[chunk] = used

    def walked(self, chunk):
        return min((self.used[chunk] + 63) // 64, self.n // 64)

    def predict_category_waves(self, d, chunk_range, before, after):
        if has_fma(d):
            return 0, 0, sum(self.walked(c) for c in chunk_range)
        flo, fhi = category_bounds(d)
        loaded, updated = wave_masks(before, after, -INF, INF)      # the loaded mask without its category compares ...
        skipped = late = upfront = 0
        per = self.n // 64
        for k, c in enumerate(chunk_range):
            w = slice(k * per, k * per + self.walked(c))
            rec = self.model[c]
            with np.errstate(invalid="ignore"):
                proven = rec is not None and bool(rec[0] >= flo) and bool(rec[1] <= fhi)
            if not proven:
                upfront += self.walked(c)
                continue
            # (the compares against -inf and +inf still refuse a NaN category: a live lane of a proven chunk has none, and a dead lane
            # fails the mask anyway)
            stays = loaded[w] & updated[w]
            skipped += int(stays.sum())
            late += int((~stays).sum())
        return skipped, late, upfront

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
                    self.category_waves.append(self.read_category_waves())
                if d.Flags & abi.STEP_COUNT_LIVE:
                    self.counts[i].append(s.step_counts().copy())
            native.lib().ilm_debug_step_interpreter(0)
            after = self.twin_state(chunk_range)
            kernel = self.kernels[-1]
            for k in range(d.SpawnCount):
                first, last = d.Spawns[k].Params.ChunkSizeAndIndices[1], d.Spawns[k].Params.ChunkSizeAndIndices[2]
                if last >= first:
                    self.used[d.Spawns[k].ChunkIndex] = max(self.used[d.Spawns[k].ChunkIndex], int(last) + 1)
            keeps = kernel in (LEAN, LEAN_CLAMP) and not has_fma(d) and not spawns_into(d, chunk_range)
            if kernel == LEAN_CLAMP and keeps:
                for k, c in enumerate(chunk_range):
                    if self.model[c] is None:
                        self.model[c] = numpy_bounds(before[1][k * self.n:k * self.n + self.used[c], 3])
            elif not keeps:
                for c in chunk_range:
                    self.model[c] = None
            if kernel != LEAN_CLAMP:
                self.predicted.append((0, 0)); self.category_predicted.append((0, 0, 0))
            else:
                self.predicted.append(None if has_fma(d) else predict_waves(before, after, *category_bounds(d)))
                self.category_predicted.append(self.predict_category_waves(d, chunk_range, before, after))
            self.records.append([self.record(c) for c in range(self.chunks)])
            self.models.append(list(self.model))

    def check(self, what):
        super().check(what)
        self.check_waves(what)
        assert self.category_waves == self.category_predicted, "%s: (skipped, late, upfront) per step %s, the model gives %s" % (what, self.category_waves, self.category_predicted)
        for k, (got, want) in enumerate(zip(self.records, self.models)):
            for c, ((lo, hi, current), rec) in enumerate(zip(got, want)):
                assert current == (1 if rec is not None else 0), "%s: step %d chunk %d: current = %d, the model holds %s" % (what, k + 1, c, current, rec)
                if rec is not None:
                    assert same_bound(lo, rec[0]) and same_bound(hi, rec[1]), "%s: step %d chunk %d: bounds (%r, %r), numpy gives %s" % (what, k + 1, c, lo, hi, rec)

    def close(self):
        native.check(native.lib().ilm_debug_step_category_waves(self.ctx.handle, 0, None, None, None))
        super().close()
