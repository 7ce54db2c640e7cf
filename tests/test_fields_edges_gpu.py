"""The generation kernels of csrc/fields.hip (render_slices_kernel, render_gbuffer_kernel) at their list, batch and range edges:
every comparison is exact equality with the CPU oracle.  tests/test_fields_kat.py asserts, without a GPU, that each scene reaches
the edge it is named after (tests/fields_common.py builds them)."""
import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import fields_common as fc

pytestmark = pytest.mark.gpu

FORMATS = [abi.SDF_UNORM16, abi.SDF_FP16]


def assert_same(got, want):
    assert np.array_equal(got, want), "%d texel channels differ" % int((got != want).sum())


def check_scene(ctx, oracle, name, fmt):
    d, inputs, slices = fc.edge_scene(name)
    assert_same(fc.render_gpu_desc(ctx, d, inputs, slices, fmt), fc.edge_scene_oracle(oracle, name, fmt))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["sort-512", "sort-513", "sort-tied"])
def test_sort_threshold(ctx, oracle, name, fmt):
    """512 entries on every tile (the longest list that is ordered nearest-first), 513 (the shortest that is not), and 300 equal keys."""
    check_scene(ctx, oracle, name, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["batch-2048", "batch-2049", "batch-4097", "batch-4097-dynamic"])
def test_obstruction_batches(ctx, oracle, name, fmt):
    """One full batch, a second batch of one record, three batches, and a filtered array whose batches do not start at the caller's
    indices; the running maxima carry from batch to batch."""
    check_scene(ctx, oracle, name, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["volumes-2048", "volumes-2049", "volumes-4100", "volumes-2049-far"])
def test_volume_batches(ctx, oracle, name, fmt):
    """Height volumes through the same batching with the tile-level circle cull live (MaximumEncodedDistance 24), and with no cull
    at all (1400)."""
    check_scene(ctx, oracle, name, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["range-large-world", "range-large-world-long-reach", "range-z-offset", "range-small-shapes",
                                  "range-reach-2^-10", "range-reach-2^-11"])
def test_ordinary_range_guards(ctx, oracle, name, fmt):
    """Which division a wave and a record take: coordinates, sizes and reach on both sides of 2^20 and 2^-10, waves that mix both
    kinds of record.  Either choice must give the correctly rounded quotient of the oracle."""
    check_scene(ctx, oracle, name, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["cull-12", "cull-48"])
def test_cull_bound(ctx, oracle, name, fmt):
    """Needles, discs, a negative size and a non-unit orientation under a short and a long reach: the bound of fill_cull_bound may
    never reject a record that decides a texel."""
    check_scene(ctx, oracle, name, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("slices", [[9, 0], [3, 3]])
def test_descending_and_repeated_slice_lists(ctx, oracle, slices, fmt):
    """A list in descending order and one that names a triplet twice, over an atlas filled with a sentinel: the listed triplets equal
    the oracle's, the others keep the sentinel."""
    d, inputs, _ = fc.edge_scene("lists")
    sentinel = np.full(fc.atlas_shape(d), 7, np.uint16)
    got = fc.render_gpu_desc(ctx, d, inputs, slices, fmt, initial=sentinel)
    want = fc.render_oracle_desc(oracle, d, inputs, slices, fmt, initial=sentinel)
    assert_same(got, want)
    full = fc.edge_scene_oracle(oracle, "lists", fmt)
    listed = np.zeros(sentinel.shape[:2], bool)
    for s in slices:
        p = s // 3
        ys = slice((p // d.ColumnCount) * d.SliceHeight, (p // d.ColumnCount + 1) * d.SliceHeight)
        xs = slice((p % d.ColumnCount) * d.SliceWidth, (p % d.ColumnCount + 1) * d.SliceWidth)
        listed[ys, xs] = True
    assert (got[~listed] == 7).all() and np.array_equal(got[listed], full[listed])


def test_dynamic_partition_in_fp16(ctx, oracle):
    """The sequence of test_partial_update_and_dynamic_partition on half-float codes: the merge with the clear source compares stored
    codes as integers, which orders non-negative halves like their values."""
    layout, obs, volumes = fc.mixed_scene(dynamic_fraction=0.4)
    vols, poly = scenes.height_volume_arrays(volumes)
    inputs = (scenes.obstruction_array(obs), vols, poly)
    slices = fc.all_triplets(layout)
    fmt = abi.SDF_FP16
    static, static_tex = fc.render_gpu_desc(ctx, scenes.render_desc(layout, dynamic_flag_filter=0), inputs, slices, fmt, keep=True)
    dynamic = fc.render_gpu_desc(ctx, scenes.render_desc(layout, dynamic_flag_filter=1), inputs, slices, fmt, clear_source=static_tex)
    static_tex.close()
    want_static = fc.render_oracle_desc(oracle, scenes.render_desc(layout, dynamic_flag_filter=0), inputs, slices, fmt)
    assert_same(static, want_static)
    assert_same(dynamic, fc.render_oracle_desc(oracle, scenes.render_desc(layout, dynamic_flag_filter=1), inputs, slices, fmt, clear_source=want_static))
    assert_same(dynamic, fc.render_oracle_desc(oracle, scenes.render_desc(layout), inputs, slices, fmt))
    assert (static < dynamic).any()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["slices-20x5", "slices-33x9"])
def test_slices_around_one_tile(ctx, oracle, name, fmt):
    """Slices smaller than one 32 x 8 tile and one texel past it each way, on an atlas of 4 x 3 slices: lanes outside the slice must
    not write into the neighbouring slice."""
    check_scene(ctx, oracle, name, fmt)


# ---- render_gbuffer_kernel ---------------------------------------------------------------------------------------------------------

def gbuffer_pair(ctx, oracle, d, vols, poly, fmt):
    w, h = fc.GBUFFER_EDGE_SIZE
    gb = native.GBufferTexture(ctx, None, fmt, size=(w, h))
    gb.render(d, vols, poly)
    got = gb.download()
    gb.close()
    want = oracle.render_gbuffer(w, h, d, vols, poly)
    return got, (want if fmt == abi.GBUFFER_FLOAT4 else want.astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("fmt", [abi.GBUFFER_FLOAT4, abi.GBUFFER_HALF4])
@pytest.mark.parametrize("name", ["mirrored-x", "mirrored-y", "no-ground-plane", "no-ground-shadows", "nan-scale"])
def test_gbuffer_views_and_ground_switches(ctx, oracle, name, fmt):
    """A 130 x 37 target (ragged against the 64 x 4 tile): a negative scale on either axis (the tile's bounds come out swapped), no
    ground plane, no ground shadows over a raised ground (one volume's top below it), and a NaN scale, where no tile bound can be
    trusted and every volume is listed for every tile: the ground alone, as in the oracle."""
    vols, poly = fc.gbuffer_edge_volumes()
    got, want = gbuffer_pair(ctx, oracle, fc.gbuffer_edge_descs()[name], vols, poly, fmt)
    assert np.array_equal(got, want), "%d texel channels differ" % int((got != want).sum())


@pytest.mark.parametrize("count", [256, 257])
def test_gbuffer_tile_list_batch_edge(ctx, oracle, count):
    """Exactly one full batch of 256 volumes on one tile, and one more: each overlaps the next, so the order of the list decides."""
    vols, poly = fc.gbuffer_stack_volumes(count)
    got, want = gbuffer_pair(ctx, oracle, scenes.gbuffer_render_desc(), vols, poly, abi.GBUFFER_FLOAT4)
    assert np.array_equal(got, want), "%d texel channels differ" % int((got != want).sum())


def test_gbuffer_zero_scale_is_refused(ctx):
    gb = native.GBufferTexture(ctx, None, abi.GBUFFER_FLOAT4, size=(16, 8))
    for scale in ((0.0, 1.0), (1.0, -0.0)):
        with pytest.raises(native.IlluminantError) as e:
            gb.render(scenes.gbuffer_render_desc(viewport_scale=scale))
        assert e.value.code == abi.ERR_INVALID_ARGUMENT
    gb.close()
