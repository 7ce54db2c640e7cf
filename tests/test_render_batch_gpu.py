"""ilm_engine_render_particles_batch: a frame's particle systems as ONE draw list.  Held to the device loop of ilm_render_particles (bit
for bit on a FLOAT4 target while no tile's run exceeds a segment) and to the CPU oracle applied item after item on one fp32 image."""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import render_batch_common as bc

pytestmark = pytest.mark.gpu

CS, W, H = 64, 77, 45              # 5 x 3 tiles, partial on both rims
CLEAR = (0.05, 0.1, 0.15, 0.2)
# whole-fragment outliers at rotated edges (render_batch_common.compare_images): tests/test_raster_gpu.py allows 8 for ~8 000 on-screen
# sprites; the scenes here hold fewer, the cap is kept
OUTLIERS = 8


def mixed_items(eng):
    """Five items over four systems, differing in everything an item can differ in; the first system comes back last with another origin.
    A few hundred live quads each, so that the whole batch stays under one segment's 2 048 pairs."""
    sheet_a = scenes.uniform(500, (16, 32, 4), 0.0, 1.0)
    sheet_b = scenes.uniform(501, (8, 8, 4), 0.0, 1.0)
    ca = bc.random_chunks(40, CS, 1, W, H, size_hi=5.0)
    cb = bc.random_chunks(41, CS, 2, W, H, size_hi=1.2)
    cc = bc.random_chunks(42, CS, 1, W, H, size_hi=1.5)
    cd = bc.random_chunks(43, CS, 1, W, H, size_hi=6.0, dead_fraction=0.95)
    for c, planes in enumerate(cb):
        planes[4][:, 3] = np.floor(scenes.uniform(400 + c, (CS * CS,), -1.0, 3.0))       # RenderData.w: the frame row
    bezier = abi.ClampedBezier1.linear(0.2, 0.9, 0.0, 3.0)
    pa = scenes.rasterize_params(size=(1.0, 0.6), global_color=(0.9, 0.8, 1.0, 0.7), origin=(3.0, -2.0), scale=(1.1, 0.9), size_from_z=0.05,
                                 z_to_y=0.25, rounded=True, rounding_power=bezier, viewport_position=(2.0, 1.0), blend=abi.BLEND_ALPHA)
    pb = scenes.rasterize_params(global_color=(1.0, 0.9, 0.8, 0.9), texture_size=(32, 16), offset_px=(0.0, 0.0), size_px=(8.0, 8.0), bilinear=True,
                                 animation_rate=(-0.7, 1.5), column_from_velocity=True, blend=abi.BLEND_ADDITIVE)
    pc = scenes.rasterize_params(global_color=(0.9, 0.8, 1.0, 0.8), texture_size=(8, 8), size_px=(4.0, 4.0), offset_px=(4.0, 0.0), bilinear=False,
                                 dithered_opacity=True, rounded=True, blend=abi.BLEND_ALPHA)
    pd = scenes.rasterize_params(global_color=(0.6, 0.7, 0.5, 0.5), rounded=False, blend=abi.BLEND_ADDITIVE)
    pa2 = scenes.rasterize_params(size=(0.8, 1.0), global_color=(0.5, 1.0, 0.6, 0.9), origin=(-11.0, 6.0), rounded=True, blend=abi.BLEND_ALPHA)
    sa, sb = bc.make_system(eng, ca), bc.make_system(eng, cb, sheet_a)
    sc, sd = bc.make_system(eng, cc, sheet_b), bc.make_system(eng, cd)
    items = [bc.Item(sa, ca, pa, [250]), bc.Item(sb, cb, pb, [200, 120], sheet_a), bc.Item(sc, cc, pc, [260], sheet_b),
             bc.Item(sd, cd, pd, None), bc.Item(sa, ca, pa2, [230])]
    return items, [sa, sb, sc, sd]


def render_both(ctx, eng, items, fmt=abi.LIGHTMAP_FLOAT4, clear=CLEAR, w=W, h=H):
    """(batch picture, batch stats, loop picture, loop stats) on two targets with the same start."""
    one, loop = native.Lightmap(ctx, w, h, fmt), native.Lightmap(ctx, w, h, fmt)
    one.clear(clear); loop.clear(clear)
    stats = eng.render_particles_batch([it.native() for it in items], one, want_stats=True)
    loop_stats = bc.device_loop(items, loop)
    got, want = one.download(), loop.download()
    one.close(); loop.close()
    return got, stats, want, loop_stats


def test_bit_equal_to_the_sequential_calls(ctx, oracle):
    eng = native.Engine(ctx, CS, scenes.randomness_table(7))
    items, systems = mixed_items(eng)
    pictures = []
    for order in (items, items[::-1]):
        got, (live, pairs, shaded), want, loop_stats = render_both(ctx, eng, order)
        assert 0 < pairs <= 2048, pairs                     # one segment per tile whatever the tile: the bit-equal case
        assert live > 500 and shaded > live
        assert (live, pairs, shaded) == loop_stats
        assert got.tobytes() == want.tobytes()
        assert eng.last_render_batch() == (5, 1, 1)
        ref, (olive, oshaded) = bc.oracle_loop(oracle, order, bc.filled(W, H, CLEAR))
        assert live == olive and abs(shaded - oshaded) <= OUTLIERS
        bc.compare_images(got, ref, "five items", OUTLIERS)
        pictures.append(got)
    # the scene is order-sensitive: the reversed batch is another picture
    assert pictures[0].tobytes() != pictures[1].tobytes()
    assert np.abs(pictures[0] - pictures[1]).max() > 1e-2
    for s in systems:
        s.close()
    eng.close()


def crowded_chunk(seed, counts, centres):
    """One chunk whose first counts[0] slots crowd around centres[0], the next counts[1] around centres[1]; the rest is dead.  Every
    sprite's centre lies well inside its cluster's tile, so each of them is on that tile's run."""
    n = CS * CS
    planes = bc.random_chunks(seed, CS, 1, W, H, size_hi=3.0, dead_fraction=0.0)[0]
    planes[0][:, 3] = 0.0
    at = 0
    for k, (count, (cx, cy)) in enumerate(zip(counts, centres)):
        planes[0][at:at + count, 0] = cx + scenes.uniform(seed + 100 + k, (count,), -3.0, 3.0)
        planes[0][at:at + count, 1] = cy + scenes.uniform(seed + 110 + k, (count,), -3.0, 3.0)
        planes[0][at:at + count, 3] = 1.0
        at += count
    planes[0][:, 2] = 0.0
    planes[3][:] *= 0.15                       # faint sprites: thousands of layers still change the pixel
    assert at <= n
    return [planes], at


def test_runs_that_cross_items(ctx, oracle):
    """Tile (1, 1) holds 3 x 1 500 pairs: the batch's run is cut at 2 048 and 4 096, inside the second and the third item.  Tile (3, 1) holds
    1 024 + 1 024 + 1 000: its cut falls exactly between the second and the third item.  No item exceeds a segment on its own, so the device
    loop blends every tile directly and only the composition's rounding differs."""
    eng = native.Engine(ctx, CS, scenes.randomness_table(7))
    centres = ((24.0, 24.0), (56.0, 24.0))
    items, systems, expect_live = [], [], 0
    for k, (second, blend) in enumerate(((1024, abi.BLEND_ALPHA), (1024, abi.BLEND_ADDITIVE), (1000, abi.BLEND_ALPHA))):
        chunks, used = crowded_chunk(200 + 7 * k, (1500, second), centres)
        params = scenes.rasterize_params(rounded=True, blend=blend, global_color=(1.0, 0.9, 0.8, 0.9))
        s = bc.make_system(eng, chunks)
        systems.append(s)
        items.append(bc.Item(s, chunks, params, [used]))
        expect_live += used
    clear = (0.2, 0.1, 0.3, 1.0)
    got, (live, pairs, shaded), want, loop_stats = render_both(ctx, eng, items, clear=clear)
    assert live == expect_live == loop_stats[0] and pairs == loop_stats[1] >= live
    assert shaded == loop_stats[2]                              # a fragment's discard does not depend on what lies beneath it
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max(axis=-1)
    assert not (err > 1e-4 * np.maximum(1.0, np.abs(want).max(axis=-1))).any(), float(err.max())
    ref, (olive, oshaded) = bc.oracle_loop(oracle, items, bc.filled(W, H, clear))
    assert live == olive and abs(shaded - oshaded) <= OUTLIERS
    bc.compare_images(got, ref, "crowded runs across items", OUTLIERS)
    assert np.abs(ref[24, 24] - np.asarray(clear, np.float32)).max() > 0.05 and np.abs(ref[24, 56] - np.asarray(clear, np.float32)).max() > 0.05
    assert eng.last_render_batch() == (3, 1, 1)
    for s in systems:
        s.close()
    eng.close()


@pytest.mark.parametrize("fmt,tol", [(abi.LIGHTMAP_HALF4, 2e-3), (abi.LIGHTMAP_RGBA8, 0.5 / 255 + 1e-6)])
def test_half_and_byte_targets_round_once(ctx, oracle, fmt, tol):
    """The batch on a HALF4 / RGBA8 target is the oracle's loop on an fp32 image, converted once (tolerances of
    tests/test_raster_gpu.py::test_half_and_byte_targets)."""
    eng = native.Engine(ctx, CS, scenes.randomness_table(7))
    items, systems = mixed_items(eng)
    target = native.Lightmap(ctx, W, H, fmt)
    target.clear((0.0, 0.0, 0.0, 0.0))
    eng.render_particles_batch([it.native() for it in items], target)
    got = target.download()
    want, _ = bc.oracle_loop(oracle, items, np.zeros((H, W, 4), np.float32))
    if fmt == abi.LIGHTMAP_HALF4:
        g = got.view(np.float16).astype(np.float32).reshape(H, W, 4)
        assert (np.abs(g - want) > tol * np.maximum(1.0, np.abs(want))).sum() <= OUTLIERS * 4
    else:
        g = got.reshape(H, W, 4).astype(np.float32) / 255.0
        assert (np.abs(g - np.clip(want, 0.0, 1.0)) > tol).sum() <= OUTLIERS * 4
    assert np.abs(want).max() > 0.5
    target.close()
    for s in systems:
        s.close()
    eng.close()


def test_byte_target_is_rounded_once_not_per_system(ctx):
    """The defined difference to the sequential calls: eight additive items of 0.001 each.  Every call of the loop stores
    round(0.001 * 255) = 0, so the loop's target stays black; the batch sums 0.008 in fp32 and stores round(2.04) = 2."""
    eng = native.Engine(ctx, 16, scenes.randomness_table(7))
    n = 16 * 16
    pos = np.zeros((n, 4), np.float32); pos[0] = (30.0, 20.0, 0.0, 1.0)
    col = np.zeros((n, 4), np.float32); col[0] = 0.001
    rd = np.zeros((n, 4), np.float32); rd[0, 0] = 10.0
    chunks = [[pos, np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), col, rd]]
    s = bc.make_system(eng, chunks)
    params = scenes.rasterize_params(rounded=False, blend=abi.BLEND_ADDITIVE)
    items = [bc.Item(s, chunks, params)] * 8
    got, stats, want, loop_stats = render_both(ctx, eng, items, fmt=abi.LIGHTMAP_RGBA8, clear=(0.0, 0.0, 0.0, 0.0))
    assert stats == loop_stats and stats[0] == 8 and stats[2] == 8 * 20 * 20
    assert not want.any()
    assert got[20, 30].tolist() == [2, 2, 2, 2] and (got[10:30, 20:40] == 2).all() and int((got != 0).sum()) == 4 * 20 * 20
    s.close(); eng.close()


@pytest.mark.parametrize("cs,n_chunks", [(16, 1), (10, 3)])
def test_many_items(ctx, cs, n_chunks):
    """256 systems, a handful of live particles each.  16 x 16 slots are exactly one setup block per item; 3 chunks of 10 x 10 are 300
    slots: two blocks, the second mostly padding."""
    eng = native.Engine(ctx, cs, scenes.randomness_table(7))
    n, w, h = cs * cs, 64, 64
    items, systems = [], []
    for i in range(256):
        chunks = bc.random_chunks(1000 + 40 * i, cs, n_chunks, w, h, size_hi=4.0, dead_fraction=0.0)
        for c, planes in enumerate(chunks):
            planes[0][:, 3] = 0.0
            planes[0][(7 * i + c) % n, 3] = 1.0; planes[0][n - 1 - c, 3] = 0.5; planes[0][(3 * i) % n, 3] = 2.0
        params = scenes.rasterize_params(rounded=bool(i & 1), blend=abi.BLEND_ADDITIVE if (i % 3 == 0) else abi.BLEND_ALPHA,
                                         global_color=(1.0, 0.5 + (i % 5) * 0.1, 0.8, 0.9), origin=(float(i % 7) - 3.0, 0.0))
        s = bc.make_system(eng, chunks)
        systems.append(s)
        items.append(bc.Item(s, chunks, params))
    got, stats, want, loop_stats = render_both(ctx, eng, items, w=w, h=h)
    assert stats == loop_stats and stats[0] > 256 * n_chunks
    assert got.tobytes() == want.tobytes()
    assert (np.abs(got - np.asarray(CLEAR, np.float32)).max(axis=-1) > 1e-3).mean() > 0.3
    assert eng.last_render_batch() == (256, 1, 1)
    for s in systems:
        s.close()
    eng.close()


def test_nothing_to_draw(ctx):
    eng = native.Engine(ctx, 16, scenes.randomness_table(7))
    w, h = 40, 24
    target = native.Lightmap(ctx, w, h, abi.LIGHTMAP_HALF4)
    start = scenes.uniform(9, (h, w, 4), 0.0, 2.0).astype(np.float16)
    target.upload(start)
    params = scenes.rasterize_params(rounded=True)
    dead = bc.random_chunks(5, 16, 1, w, h, size_hi=4.0)
    dead[0][0][:, 3] = 0.0
    away = bc.random_chunks(6, 16, 1, w, h, size_hi=4.0, dead_fraction=0.0)
    away[0][0][:, 0] += 500.0
    s_dead, s_away, s_empty = bc.make_system(eng, dead), bc.make_system(eng, away), native.System(eng)
    cases = [([], 0), ([(s_dead, params, None, 0), (s_empty, params), (s_away, params, None, 0)], 0),
             ([(s_dead, params), (s_dead, params)], 0), ([(s_away, params), (s_dead, params), (s_away, params)], 2 * int((away[0][4][:, 0] > 0.0).sum()))]
    for batch, live in cases:
        assert eng.render_particles_batch(batch, target, want_stats=True) == (live, 0, 0)
        assert eng.last_render_batch() == (len(batch), 0, 0)
        assert eng.render_particles_batch(batch, target) is None
        assert target.download().tobytes() == start.tobytes()
    for x in (s_dead, s_away, s_empty, target):
        x.close()
    eng.close()


def test_refusals_leave_the_target_alone(ctx, oracle):
    """Every item is judged before anything is queued: the bad item comes last, behind items that would already have drawn."""
    eng, other = native.Engine(ctx, 16, scenes.randomness_table(7)), native.Engine(ctx, 16, scenes.randomness_table(7))
    w, h = 40, 24
    chunks = bc.random_chunks(8, 16, 1, w, h, size_hi=5.0, dead_fraction=0.0)
    good, foreign, bare = bc.make_system(eng, chunks), bc.make_system(other, chunks), bc.make_system(eng, chunks)
    target = native.Lightmap(ctx, w, h, abi.LIGHTMAP_FLOAT4)
    target.clear(CLEAR)
    start = target.download()
    ok = scenes.rasterize_params(rounded=True)
    eng.render_particles_batch([(good, ok)], target)
    first = target.download()
    assert first.tobytes() != start.tobytes() and eng.last_render_batch() == (1, 1, 1)
    target.clear(CLEAR)

    def params(**changes):
        p = scenes.rasterize_params(rounded=True)
        for k, v in changes.items():
            setattr(p, k, v)
        return p

    empty_region = scenes.rasterize_params(texture_size=(8, 8)); empty_region.BitmapTextureRegion = abi.f4(0.5, 0.0, 0.5, 1.0)
    good.set_bitmap(np.ones((8, 8, 4), np.float32))
    lib = native.lib()
    bad_items = [
        ((good, scenes.rasterize_params(stipple_factor=0.5)), abi.ERR_INVALID_ARGUMENT),
        ((good, params(BlendMode=7)), abi.ERR_INVALID_ARGUMENT),
        ((good, params(BitmapFilter=3)), abi.ERR_INVALID_ARGUMENT),
        ((bare, scenes.rasterize_params(texture_size=(8, 8))), abi.ERR_STATE),
        ((good, empty_region), abi.ERR_INVALID_ARGUMENT),
        ((good, ok, None, 2), abi.ERR_OUT_OF_RANGE),
        ((good, ok, None, -1), abi.ERR_OUT_OF_RANGE),
        ((good, ok, [16 * 16 + 1]), abi.ERR_OUT_OF_RANGE),
        ((good, ok, [-1]), abi.ERR_OUT_OF_RANGE),
        ((foreign, ok), abi.ERR_INVALID_ARGUMENT),
        ((target, ok, None, 1), abi.ERR_INVALID_HANDLE),          # a live handle, but not a system's
    ]
    for bad, code in bad_items:
        with pytest.raises(native.IlluminantError) as e:
            eng.render_particles_batch([(good, ok), (good, ok), bad], target, want_stats=True)
        assert e.value.code == code and "item 2:" in str(e.value), str(e.value)
        assert target.download().tobytes() == start.tobytes()
        assert eng.last_render_batch() == (1, 1, 1)               # a refused batch is not the engine's latest
    # the call's own arguments
    packed = (abi.RasterizeItem * 1)()
    packed[0].System, packed[0].ChunkCount = good.handle.value, 1
    C.memmove(C.byref(packed[0], abi.RasterizeItem.Params.offset), C.byref(ok), C.sizeof(ok))
    assert lib.ilm_engine_render_particles_batch(eng.handle, None, 1, target.handle, None) == abi.ERR_INVALID_ARGUMENT
    assert lib.ilm_engine_render_particles_batch(eng.handle, C.cast(packed, C.c_void_p), -1, target.handle, None) == abi.ERR_INVALID_ARGUMENT
    assert lib.ilm_engine_render_particles_batch(eng.handle, C.cast(packed, C.c_void_p), 1, good.handle, None) == abi.ERR_INVALID_HANDLE
    assert lib.ilm_engine_render_particles_batch(good.handle, C.cast(packed, C.c_void_p), 1, target.handle, None) == abi.ERR_INVALID_HANDLE
    sibling = ctx.sibling()
    elsewhere = native.Lightmap(sibling, w, h, abi.LIGHTMAP_FLOAT4)
    assert lib.ilm_engine_render_particles_batch(eng.handle, C.cast(packed, C.c_void_p), 1, elsewhere.handle, None) == abi.ERR_INVALID_ARGUMENT
    elsewhere.close(); sibling.close()
    assert target.download().tobytes() == start.tobytes()
    # nothing is left behind: the packed array itself renders, and renders what the first call did
    assert lib.ilm_engine_render_particles_batch(eng.handle, C.cast(packed, C.c_void_p), 1, target.handle, None) == 0
    got = target.download()
    assert got.tobytes() == first.tobytes()
    ref, _ = bc.oracle_loop(oracle, [bc.Item(good, chunks, ok)], bc.filled(w, h, CLEAR))
    bc.compare_images(got, ref, "after the refusals", OUTLIERS)
    for x in (target, good, foreign, bare):
        x.close()
    eng.close(); other.close()
