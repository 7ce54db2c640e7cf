"""The particle rasteriser's machinery (raster.hip) at its run, tile-table and format edges, against the CPU oracle.

Every scene of tests/raster_structure_common.py is made of axis-aligned, square-cornered, untextured sprites: sin / cos are exactly 0
and 1 and pow never runs, so device and oracle execute the same IEEE operations.  Criteria:
  * every tile on the direct path (<= 2048 sprites) and a FLOAT4 target: live, pairs and shaded equal, the image bit-identical;
  * a segmented tile: `over` is bracketed differently, a few ulps -- test_raster_gpu.compare_images at 1e-4 x max(1, |want|) with no
    outlier, the shaded count exact;
  * HALF4: every channel within one float16 step of the converted reference;
  * RGBA8: every channel equal to rint(sat(want) * 255), one code either way where want * 255 lies within 1e-3 of a tie.
tests/test_raster_structure.py checks, without a GPU, that the scenes reach the edges they are named after."""
import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import raster_structure_common as rs
from tests.test_raster_gpu import compare_images

pytestmark = pytest.mark.gpu

P, RCOL, RD = abi.PLANE_POSITION, abi.PLANE_RENDER_COLOR, abi.PLANE_RENDER_DATA
RANDOMNESS = scenes.randomness_table(7)


def render(ctx, scene, fmt=abi.LIGHTMAP_FLOAT4, initial=None, want_stats=True):
    """-> (the target's texels, (live, pairs, shaded) or None).  initial: texels in the target's format (default: cleared to rs.CLEAR)."""
    chunks, quads, params, w, h = scene[:5]
    eng = native.Engine(ctx, int(round(chunks[0][0].shape[0] ** 0.5)), RANDOMNESS)
    sysm = native.System(eng)
    lm = native.Lightmap(ctx, w, h, fmt)
    try:
        for c, planes in enumerate(chunks):
            sysm.add_chunk()
            sysm.upload(c, P, planes[0]); sysm.upload(c, RCOL, planes[3]); sysm.upload(c, RD, planes[4])
        if initial is None:
            lm.clear(rs.CLEAR)
        else:
            lm.upload(initial)
        stats = native.render_particles(sysm, params, lm, quad_counts=quads, want_stats=want_stats)
        return lm.download(), stats
    finally:
        lm.close(); sysm.close(); eng.close()


def check_float4(ctx, oracle, key, scene, what):
    """The FLOAT4 criterion the scene's run lengths call for; returns the largest error relative to max(1, |want|)."""
    want, (olive, oshaded), (runs, opairs) = rs.reference(oracle, key, scene)
    got, (live, pairs, shaded) = render(ctx, scene)
    err = float((np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max())
    print("%s: live %d / %d, pairs %d / %d, shaded %d / %d, longest run %d, largest error %.3g"
          % (what, live, olive, pairs, opairs, shaded, oshaded, int(runs.max()), err))
    assert (live, pairs, shaded) == (olive, opairs, oshaded), what
    if rs.is_direct(runs):
        differ = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).ravel())
        assert differ.size == 0, "%s: %d pixels are not bit-identical, the first at (%d, %d): %r != %r" % (
            what, differ.size, differ[0] % got.shape[1], differ[0] // got.shape[1],
            got.reshape(-1, 4)[differ[0]].tolist(), want.reshape(-1, 4)[differ[0]].tolist())
    else:
        compare_images(got, want, what, max_outliers=0)
    return err


# ---- a. run lengths on one tile ------------------------------------------------------------------------------------------------------

BLENDS = {"alpha": abi.BLEND_ALPHA, "additive": abi.BLEND_ADDITIVE}


@pytest.mark.parametrize("n,blend", [(n, "alpha") for n in rs.RUN_LENGTHS] + [(n, "additive") for n in (257, 2049, 4097)])
def test_run_length_on_one_tile(ctx, oracle, n, blend):
    """n sprites on tile (2, 1) of a 64 x 48 target: 255 / 256 / 257 around the LDS batch, 2047 / 2048 / 2049 / 4096 / 4097 around the
    segment (direct path against partials + combine; 4097 also crosses a chunk boundary)."""
    check_float4(ctx, oracle, ("a", n, BLENDS[blend]), rs.one_tile_scene(n, BLENDS[blend]), "%d sprites on one tile, %s" % (n, blend))


def test_dithered_segments_replace_each_other(ctx, oracle):
    """Dithered fragments are opaque: a segment's transmittance is exactly 0 wherever it drew, and a later segment replaces the earlier
    ones there.  Alpha is exactly 1 on the whole tile."""
    n = rs.SEGMENT + 1
    scene = rs.one_tile_scene(n, abi.BLEND_ALPHA, True)
    want, (olive, oshaded), (runs, opairs) = rs.reference(oracle, ("a dithered", n), scene)
    got, stats = render(ctx, scene)
    assert stats == (olive, opairs, oshaded)
    compare_images(got, want, "dithered, 2049 sprites", max_outliers=0)
    assert np.all(got[16:32, 32:48, 3] == 1.0)


# ---- b. neighbouring tiles cut at different sprites ------------------------------------------------------------------------------------

def test_neighbouring_tiles_cut_at_different_sprites(ctx, oracle):
    """Tiles (2, 1) and (3, 1) share 2048 sprites and hold 2049 each: one is cut after a shared sprite, the other before its own."""
    check_float4(ctx, oracle, ("b", abi.BLEND_ALPHA), rs.straddle_scene(), "straddling sprites")


# ---- c. quadrant lists ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arrangement", rs.QUADRANT_ARRANGEMENTS)
def test_quadrant_lists(ctx, oracle, arrangement):
    """Sprites that pass the box test of one quadrant only: one list takes a whole batch while the other waves idle; the lists filled
    round-robin; each loader wave feeding one list; a 257th sprite alone in its batch and alone in quadrant 0; a border tile whose
    quadrants 1-3 lie outside the image."""
    scene = rs.quadrant_scene(arrangement)
    _, _, (runs, _) = rs.reference(oracle, ("c", arrangement), scene)
    assert rs.is_direct(runs)
    check_float4(ctx, oracle, ("c", arrangement), scene, "quadrants, " + arrangement)


# ---- d. every format on both paths, over existing content -----------------------------------------------------------------------------

@pytest.mark.parametrize("blend", ["alpha", "additive"])
@pytest.mark.parametrize("n", [300, 2049])
@pytest.mark.parametrize("fmt", [abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8], ids=["half4", "rgba8"])
def test_half_and_byte_targets_over_existing_content(ctx, oracle, fmt, n, blend):
    """load_target on non-zero half / byte texels (the direct path at 300 sprites, raster_combine_kernel at 2049) and the store back."""
    scene = rs.one_tile_scene(n, BLENDS[blend])
    content = rs.initial_content(rs.A_W, rs.A_H, fmt)
    want, (olive, oshaded), (runs, opairs) = rs.reference(oracle, ("d", fmt, n, blend), scene, initial=rs.from_target(content, fmt))
    assert rs.is_direct(runs) == (n == 300)
    got, stats = render(ctx, scene, fmt, initial=content)
    assert stats == (olive, opairs, oshaded)
    untouched = np.ones((rs.A_H, rs.A_W), bool)
    untouched[0:48, 16:64] = False                         # the crowded tile and the neighbours its covers reach
    assert np.array_equal(got[untouched], content[untouched])
    if fmt == abi.LIGHTMAP_HALF4:
        steps = rs.half_steps(got, rs.to_target(want, fmt))
        print("half4, %d sprites, %s: %d channels one step off" % (n, blend, int((steps == 1).sum())))
        assert steps.max() <= 1, "%d channels more than one float16 step off (largest %d)" % (int((steps > 1).sum()), int(steps.max()))
    else:
        code, near_tie = rs.unorm8_codes(want)
        off = np.abs(got.astype(np.int32) - code)
        print("rgba8, %d sprites, %s: %d channels near a tie, %d of them one code off" % (n, blend, int(near_tie.sum()), int((off == 1).sum())))
        assert np.all(off <= np.where(near_tie, 1, 0)), "%d channels differ from rint(sat(want) * 255)" % int((off > np.where(near_tie, 1, 0)).sum())
    # the picture is not the content it started from
    assert (rs.to_target(want, fmt)[16:32, 32:48] != content[16:32, 32:48]).mean() > 0.5


def test_statistics_do_not_change_the_picture(ctx, oracle):
    """count_shaded == 0 compiles the counters out of setup and tiles: the texels are the same bytes."""
    scene = rs.one_tile_scene(rs.SEGMENT + 1)
    with_stats, stats = render(ctx, scene, want_stats=True)
    without, none = render(ctx, scene, want_stats=False)
    assert none is None and stats[0] == rs.SEGMENT + 1
    assert with_stats.tobytes() == without.tobytes()
    want, _, _ = rs.reference(oracle, ("a", rs.SEGMENT + 1, abi.BLEND_ALPHA), scene)
    compare_images(without, want, "no statistics", max_outliers=0)


# ---- e. tile-table sizes and two crowded tiles ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tiles,height", rs.STRIPS)
def test_tile_table_sizes_with_two_crowded_tiles(ctx, oracle, tiles, height):
    """raster_tile_scan_kernel over tiles + 1 = 1023, 1024, 1025 and 9217 entries (1, 1, 2 and 10 per thread: the last one full group of
    eight and a ragged one), a 2049-sprite tile a third of the way along and a 4097-sprite tile at the very end: the last tile's first
    work item and first partial slot are both non-zero, and differ."""
    check_float4(ctx, oracle, ("e", tiles, height), rs.strip_scene(tiles, height), "strip of %d tiles, %d rows" % (tiles, height))


@pytest.mark.parametrize("width,height", rs.TINY_TARGETS)
def test_tiny_targets(ctx, oracle, width, height):
    check_float4(ctx, oracle, ("tiny", width, height), rs.tiny_scene(width, height), "%d x %d target" % (width, height))


# ---- f. the pair cap --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["one_over", "wrap"])
def test_pair_cap_refuses_and_draws_nothing(ctx, oracle, kind):
    """2^28 + 1 pairs, and a total of exactly 2^32 whose 32-bit sum is 0 (the scan saturates instead): ILM_ERR_TOO_MANY, the target
    untouched, and the context renders the next frame as if nothing had happened."""
    chunks, quads, params, w, h = rs.cap_scene(kind)
    clear = (0.25, 0.5, 0.75, 1.0)
    eng = native.Engine(ctx, 256, RANDOMNESS)
    sysm = native.System(eng)
    lm = native.Lightmap(ctx, w, h, abi.LIGHTMAP_RGBA8)
    try:
        for c, planes in enumerate(chunks):
            sysm.add_chunk()
            sysm.upload(c, P, planes[0]); sysm.upload(c, RCOL, planes[3]); sysm.upload(c, RD, planes[4])
        lm.clear(clear)
        with pytest.raises(native.IlluminantError) as e:
            native.render_particles(sysm, params, lm, quad_counts=quads, want_stats=True)
        assert e.value.code == abi.ERR_TOO_MANY
        sample = lm.download(first_row=2016, row_count=64)
        assert np.all(sample == rs.to_target(np.asarray(clear, np.float32), abi.LIGHTMAP_RGBA8))
    finally:
        lm.close(); sysm.close(); eng.close()
    check_float4(ctx, oracle, ("a", 257, abi.BLEND_ALPHA), rs.one_tile_scene(257), "257 sprites after the refusal")


# ---- g. non-finite and degenerate slots -------------------------------------------------------------------------------------------------

def test_non_finite_and_degenerate_slots(ctx, oracle):
    """NaN / -0 / +0 / denormal / negative life, size 0 / negative / 1e18 / 1e30 / inf, positions NaN, inf or 1e30 away, alpha 0 /
    negative / 1.5, among ordinary sprites.  Far-off finite sprites are live without a pair; degenerate ones are not live."""
    scene = rs.degenerate_scene()
    _, (olive, _), _ = rs.reference(oracle, ("g",), scene)
    assert olive == rs.degenerate_live_claim()
    check_float4(ctx, oracle, ("g",), scene, "degenerate slots")


# ---- h. scratch reuse in one context ----------------------------------------------------------------------------------------------------

def test_scratch_is_reused_without_stale_tables(ctx, oracle):
    """A crowded frame, a tiny one, the crowded one again, a larger frame with fewer sprites: the context's tile tables, partials and
    counts only ever grow, and what an earlier frame left in them must not show."""
    crowded = rs.one_tile_scene(2 * rs.SEGMENT + 1)
    check_float4(ctx, oracle, ("a", 2 * rs.SEGMENT + 1, abi.BLEND_ALPHA), crowded, "crowded frame")
    check_float4(ctx, oracle, ("h", 20), rs.scattered_scene(20, 20, 16, 9100), "20 x 20 frame")
    check_float4(ctx, oracle, ("a", 2 * rs.SEGMENT + 1, abi.BLEND_ALPHA), crowded, "crowded frame again")
    check_float4(ctx, oracle, ("h", 640), rs.scattered_scene(640, 360, 900, 9200), "640 x 360 frame")
