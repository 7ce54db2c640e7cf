"""Pins the oracle's distance-field generation (oracle/ilm_oracle_fields.c) without a GPU:
closed-form fixture codes, an independent numpy rasteriser, and the pass's structural properties."""
import numpy as np
import pytest

from illuminant_amd import abi, scenes
from tests import fields_common as fc


def render_oracle(oracle, layout, obs=None, vols=None, poly=None, slices=None, fmt=abi.SDF_UNORM16, flt=-1, clear_source=None, atlas=None):
    if atlas is None:
        atlas = np.zeros((layout.atlas_height, layout.atlas_width, 4), np.uint16)
    d = scenes.render_desc(layout, dynamic_flag_filter=flt)
    return oracle.render_distance_field_slices(atlas, fmt, d, fc.all_triplets(layout) if slices is None else slices, obs, vols, poly,
                                               clear_source=clear_source)


def test_closed_form_codes(oracle):
    doc = fc.load_generation_fixture()
    layout = fc.fixture_layout(doc)
    assert (layout.slice_width, layout.slice_height, layout.slice_count) == (128, 128, 9)
    for case in doc["cases"]:
        obs, vols, poly = fc.fixture_case_inputs(case)
        atlas = render_oracle(oracle, layout, obs, vols, poly)
        got = fc.texel_of(atlas, layout, case["texel"][0], case["texel"][1], case["slice"])
        assert abs(got - case["expected_code"]) <= 1, (case, got)


def test_matches_independent_numpy_rasteriser(oracle):
    """scenes.build_sdf_atlas (float64 numpy, written for the lighting tests) rasterises unrotated ellipsoids, boxes and
    cylinders on its own; the two agree to one code."""
    layout = scenes.DistanceFieldLayout(256, 192, 96.0, 12, 0.5, 128)
    old = scenes.random_obstacles(5, 14, (256, 192), size_lo=8.0, size_hi=30.0, z_hi=40.0)
    want = scenes.build_sdf_atlas(layout, old)
    got = render_oracle(oracle, layout, scenes.obstruction_array([(t - 1, c, s) for (t, c, s) in old]))
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert diff.max() <= 1, int(diff.max())
    assert (want > 0).mean() > 0.3


def test_alpha_of_slice_is_red_of_next(oracle):
    """A texel's RGBA holds virtual slices 3p..3p+3, so A of physical slice p == R of p+1 (SliceZ, DistanceFunction.fx:14)."""
    layout, obs, volumes = fc.mixed_scene()
    vols, poly = scenes.height_volume_arrays(volumes)
    atlas = render_oracle(oracle, layout, scenes.obstruction_array(obs), vols, poly)
    L = layout
    for p in range(L.physical_slice_count - 1):
        a = atlas[(p // L.column_count) * L.slice_height:(p // L.column_count + 1) * L.slice_height,
                  (p % L.column_count) * L.slice_width:(p % L.column_count + 1) * L.slice_width, 3]
        q = p + 1
        r = atlas[(q // L.column_count) * L.slice_height:(q // L.column_count + 1) * L.slice_height,
                  (q % L.column_count) * L.slice_width:(q % L.column_count + 1) * L.slice_width, 0]
        assert np.array_equal(a, r)


def test_max_blend_is_order_free_and_monotone(oracle):
    layout, obs, volumes = fc.mixed_scene()
    vols, poly = scenes.height_volume_arrays(volumes)
    full = render_oracle(oracle, layout, scenes.obstruction_array(obs), vols, poly)
    rev = render_oracle(oracle, layout, scenes.obstruction_array(obs[::-1]), vols, poly)
    assert np.array_equal(full, rev)
    fewer = render_oracle(oracle, layout, scenes.obstruction_array(obs[:10]))
    assert (full >= fewer).all() and (full > fewer).any()
    # per-obstruction renders MAX-combined == one render of all (BlendFunction.Max, LoadMaterials.cs:164-176)
    acc = render_oracle(oracle, layout, None, vols, poly)
    for o in obs:
        acc = np.maximum(acc, render_oracle(oracle, layout, scenes.obstruction_array([o])))
    assert np.array_equal(acc, full)


def test_partial_update_touches_only_the_listed_triplets(oracle):
    layout, obs, _ = fc.mixed_scene()
    arr = scenes.obstruction_array(obs)
    full = render_oracle(oracle, layout, arr)
    sentinel = np.full_like(full, 7)
    part = render_oracle(oracle, layout, arr, slices=[3], atlas=sentinel.copy())
    L = layout
    p = 1
    ys = slice((p // L.column_count) * L.slice_height, (p // L.column_count + 1) * L.slice_height)
    xs = slice((p % L.column_count) * L.slice_width, (p % L.column_count + 1) * L.slice_width)
    assert np.array_equal(part[ys, xs], full[ys, xs])
    mask = np.ones(full.shape[:2], bool)
    mask[ys, xs] = False
    assert (part[mask] == 7).all()


def test_dynamic_field_is_static_clear_plus_dynamic_obstructions(oracle):
    """DynamicDistanceField: the static partition renders IsDynamic == false, the dynamic one clears each slice to the
    static texture and MAX-blends IsDynamic == true on top (LightingRenderer.DistanceField.cs:20-30,117-119)."""
    layout, obs, volumes = fc.mixed_scene(dynamic_fraction=0.4)
    vols, poly = scenes.height_volume_arrays(volumes)
    arr = scenes.obstruction_array(obs)
    assert 0 < sum(1 for o in obs if o[4]) < len(obs)
    static = render_oracle(oracle, layout, arr, vols, poly, flt=0)
    dynamic = render_oracle(oracle, layout, arr, vols, poly, flt=1, clear_source=static)
    everything = render_oracle(oracle, layout, arr, vols, poly, flt=-1)
    assert np.array_equal(dynamic, everything)
    assert (static < everything).any()


@pytest.mark.parametrize("fmt", [abi.SDF_UNORM16, abi.SDF_FP16])
def test_generated_field_samples_back_the_analytic_distance(oracle, fmt):
    """encode -> store -> sampleDistanceFieldEx round trip: the sampled distance of a generated sphere field is the analytic one
    (within the quantisation of the format and the bilinear / slice interpolation of a curved function)."""
    layout = scenes.DistanceFieldLayout(128, 128, 64.0, 16, 1.0, 128)
    sph = [(abi.OBSTRUCTION_SPHEROID, (64.0, 64.0, 20.0), (18.0, 18.0, 18.0), 0.0)]
    atlas = render_oracle(oracle, layout, scenes.obstruction_array(sph), fmt=fmt)
    tex = oracle.make_texture(atlas, fmt)
    dfu = layout.uniforms()
    pts = scenes.uniform(3, (200, 3), 0.0, 1.0) * np.array([127.0, 127.0, 50.0], np.float32)
    for p in pts:
        want = float(np.linalg.norm(p - np.array([64.0, 64.0, 20.0]))) - 18.0
        got = oracle.sample_distance_field(p, dfu, tex)
        if want < 90.0:     # beyond ~96 the encoding saturates
            assert abs(got - want) < (1.2 if fmt == abi.SDF_UNORM16 else 1.6), (p, got, want)


# ---- the edge scenes of tests/test_fields_edges_gpu.py: what makes the device's comparison with the oracle meaningful, asserted on the
# oracle's output and on the inputs alone.  Measured on the oracle when the scenes were written (the tests print them: pytest -s):
#
#   scene                          distinct codes      what the scene is for
#                                  UNORM16   fp16
#   sort-512 / sort-513            10129/10261  3964/3792   every tile list holds exactly 512 / 513 entries
#   sort-tied                      13435     2242      tile lists of 335 .. 387 entries, 300 of them one record
#   batch-2048                     12090     2494      record 2047 decides 1113 texel channels
#   batch-2049                     11852     2901      record 2047: 1154, record 2048: 1048
#   batch-4097                     10874     2114      record 2047: 1005, 2048: 973, 4096: 1015
#   batch-4097-dynamic             10963     2539      2270 of 4097 records pass the filter; record 4096: 1158
#   volumes-2048 / -2049 / -4100   23690/24002/23634  4958/4896/4797   volume 2047: 962 / 970 / 881, the last one: 962 / 865 / 782
#   volumes-2049-far               9241      700       volume 2047: 43252, volume 2048: 4713
#   range-large-world              2518      1971      4 ordinary records, 7 others; 2 of 64 waves ordinary, both see both kinds
#   range-large-world-long-reach   3716      2382      the same records; no wave ordinary (MaximumEncodedDistance 1.5 x 2^20)
#   range-z-offset                 2477      1850      4 + 4 records; 32 of 64 waves ordinary, all 32 see both kinds
#   range-small-shapes             19163     3161      6 ordinary records, 34 others; all 128 waves ordinary and see both kinds
#   range-reach-2^-10 / 2^-11      1787/1792 1773/1670 2 + 1 records; all 128 waves ordinary / none
#   cull-12 / cull-48              9708/11450  4077/1399
#   lists                          8237      2317
#   slices-20x5 / slices-33x9      1571/7486 711/1886

@pytest.mark.parametrize("fmt", [abi.SDF_UNORM16, abi.SDF_FP16])
@pytest.mark.parametrize("name", sorted(fc.EDGE_SCENES))
def test_edge_scene_is_not_degenerate(oracle, name, fmt):
    """Neither all zero nor all saturated, and at least 1000 distinct UNORM16 codes (500 fp16 codes: the format has fewer in [0, 1])."""
    atlas = fc.edge_scene_oracle(oracle, name, fmt)
    distinct = len(np.unique(atlas))
    print("%s fmt %d: %d distinct codes, %.1f %% zero" % (name, fmt, distinct, 100.0 * (atlas == 0).mean()))
    one = 65535 if fmt == abi.SDF_UNORM16 else 0x3C00
    assert (atlas != 0).any() and (atlas != one).any()
    assert distinct >= (1000 if fmt == abi.SDF_UNORM16 else 500), distinct


def test_dynamic_partition_scene_is_not_degenerate_in_fp16(oracle):
    layout, obs, volumes = fc.mixed_scene(dynamic_fraction=0.4)
    vols, poly = scenes.height_volume_arrays(volumes)
    atlas = render_oracle(oracle, layout, scenes.obstruction_array(obs), vols, poly, fmt=abi.SDF_FP16)
    assert len(np.unique(atlas)) >= 500 and (atlas != 0).any() and (atlas != 0x3C00).any()


def test_sort_scenes_lie_on_both_sides_of_the_sort_capacity():
    """Every tile's list holds exactly 512 entries (ordered nearest-first) or exactly 513 (left in index order); the tied scene's lists
    all hold the 300 equal records and stay below the capacity."""
    for n in (512, 513):
        d, inputs, _ = fc.edge_scene("sort-%d" % n)
        assert set(fc.tile_list_lengths(d, inputs[0])) == {n}
    assert fc.FIELD_SORT_CAPACITY == 512
    d, inputs, _ = fc.edge_scene("sort-tied")
    lengths = fc.tile_list_lengths(d, inputs[0])
    assert 300 < min(lengths) and max(lengths) <= fc.FIELD_SORT_CAPACITY          # 335 .. 387
    arr = inputs[0]
    assert all(bytes(arr[50 + k]) == bytes(arr[50]) for k in range(300))


@pytest.mark.parametrize("name,records,batches,placed", [
    ("batch-2048", 2048, 1, (2047,)), ("batch-2049", 2049, 2, (2047, 2048)), ("batch-4097", 4097, 3, (2047, 2048, 4096)),
    ("batch-4097-dynamic", None, 2, (4096,))])
def test_obstruction_batch_scenes_depend_on_their_late_records(oracle, name, records, batches, placed):
    """The last record of the first batch of 2048 and the last record of the array each decide at least 16 texel channels (a record
    that is dropped, or read at the wrong index, shows).  Under the dynamic
    filter more than 2048 records remain, fewer than the caller passed: the batch boundary is no longer at the caller's index 2048."""
    d, inputs, slices = fc.edge_scene(name)
    kept = len(fc.filtered_records(d, inputs[0]))
    if records is None:
        assert fc.FIELD_LIST_CAPACITY < kept < len(inputs[0]) - 1000            # 2270 of 4097
    else:
        assert kept == records == len(inputs[0])
    assert (kept + fc.FIELD_LIST_CAPACITY - 1) // fc.FIELD_LIST_CAPACITY == batches
    lengths = fc.tile_list_lengths(d, inputs[0])
    assert max(lengths) > fc.FIELD_SORT_CAPACITY                                # full batches are walked in index order
    full = fc.edge_scene_oracle(oracle, name, abi.SDF_UNORM16)
    for index in placed:
        changed = fc.channels_changed_by(oracle, full, d, inputs, slices, index)
        print("%s: record %d decides %d channels" % (name, index, changed))
        assert changed >= 16, (index, changed)                                  # 973 .. 1154


@pytest.mark.parametrize("name,count", [("volumes-2048", 2048), ("volumes-2049", 2049), ("volumes-4100", 4100), ("volumes-2049-far", 2049)])
def test_volume_batch_scenes_depend_on_their_late_volumes(oracle, name, count):
    d, inputs, slices = fc.edge_scene(name)
    assert len(inputs[1]) == count
    # the tile-level and texel-level culls of fields.hip are live unless the reach passes sdPolygon's cap
    widest_need = fc.F(fc.F(192.0 / 255.0) * fc.F(d.MaximumEncodedDistance)) + fc.F(1.0)
    assert (widest_need <= 999.0) == (name != "volumes-2049-far")
    full = fc.edge_scene_oracle(oracle, name, abi.SDF_UNORM16)
    for index in sorted({2047, count - 1}):
        changed = fc.channels_changed_by(oracle, full, d, inputs, slices, index)
        print("%s: volume %d decides %d channels" % (name, index, changed))
        assert changed >= 16, (index, changed)


@pytest.mark.parametrize("name,waves", [
    ("range-large-world", "both"), ("range-large-world-long-reach", "none"), ("range-z-offset", "both"), ("range-small-shapes", "all"),
    ("range-reach-2^-10", "all"), ("range-reach-2^-11", "none")])
def test_range_scenes_hold_both_kinds_of_record_and_wave(name, waves):
    """The per-record bit of api.hip (sizes in [2^-10, 2^20], centre within 2^20) takes both values in every scene.  The per-wave
    predicate of fields.hip takes both values inside the large world and across the z offset, where some ordinary wave also sees
    both kinds of record; it is true for every wave at MaximumEncodedDistance 2 and 2^-10, and false for every wave above 2^20 and
    below 2^-10 (the reach is a uniform of the launch: those two pairs of scenes are its two sides)."""
    d, inputs, slices = fc.edge_scene(name)
    bits = [fc.record_is_ordinary(o) for o in inputs[0]]
    assert any(bits) and not all(bits)
    ordinary, other, mixed = fc.wave_census(d, slices, inputs[0])
    print("%s: %d ordinary records, %d others; %d ordinary waves, %d others, %d ordinary waves see both kinds" %
          (name, sum(bits), len(bits) - sum(bits), ordinary, other, mixed))
    if waves == "both":
        assert ordinary > 0 and other > 0 and mixed > 0
    elif waves == "all":
        assert ordinary > 0 and other == 0 and mixed > 0
    else:
        assert ordinary == 0 and other > 0


def test_range_scene_sizes_sit_on_the_thresholds():
    sizes = lambda name: np.array([[o.Size[k] for k in range(3)] for o in fc.edge_scene(name)[1][0]], np.float32)
    centres = lambda name: np.array([[o.Center[k] for k in range(3)] for o in fc.edge_scene(name)[1][0]], np.float32)
    big, above = np.float32(2.0 ** 20), np.nextafter(np.float32(2.0 ** 20), np.float32(np.inf))
    s, c = sizes("range-large-world"), centres("range-large-world")
    assert (s == big).any() and (s == above).any() and (c == big).any() and (c == above).any() and (c < big).any() and (c > above).any()
    assert s.min() >= 2.0 ** 17
    s = sizes("range-small-shapes")
    assert (s == np.float32(2.0 ** -10)).any() and (s < np.float32(2.0 ** -10)).any() and (s > np.float32(2.0 ** -10)).any()
    assert s.min() >= 2.0 ** -11 and s.max() <= 2.0 ** -9
    c = centres("range-z-offset")
    assert (c[:, 2] == big).any() and (c[:, 2] > big).any() and (c[:, 2] < big).any()


def test_cull_scene_holds_the_irregular_records():
    arr = fc.edge_scene("cull-12")[1][0]
    sizes = np.array([[o.Size[k] for k in range(3)] for o in arr], np.float64)
    assert (sizes < 0).any() and np.isfinite(sizes).all() and (sizes != 0).all()
    ratio = np.abs(sizes).max(axis=1) / np.abs(sizes).min(axis=1)
    types = np.array([o.Type for o in arr])
    for t in (abi.OBSTRUCTION_ELLIPSOID, abi.OBSTRUCTION_BOX):
        assert ratio[types == t].max() >= 100.0
    for t in (abi.OBSTRUCTION_CYLINDER, abi.OBSTRUCTION_SPHEROID, abi.OBSTRUCTION_OCTAGON):
        assert ratio[types == t].max() >= 50.0
    norms = np.array([sum(float(o.Orientation[k]) ** 2 for k in range(4)) for o in arr])
    assert (np.abs(norms - 1.0) > 1e-3).sum() == 1 and abs(norms.max() - 1.69) < 1e-3      # fill_cull_bound's unit test: |q|^2 within 1e-3 of 1


def test_gbuffer_edge_scenes(oracle):
    """The G-buffer descs of the device test on the oracle: mirrored views show the volumes, a volume whose top lies below GroundZ is
    discarded, a NaN scale leaves the ground alone, and in the stack of 257 the last volume is visible."""
    w, h = fc.GBUFFER_EDGE_SIZE
    vols, poly = fc.gbuffer_edge_volumes()
    got = {name: oracle.render_gbuffer(w, h, d, vols, poly) for name, d in fc.gbuffer_edge_descs().items()}
    plain = oracle.render_gbuffer(w, h, scenes.gbuffer_render_desc(), vols, poly)
    assert np.array_equal(got["mirrored-x"], plain[:, ::-1])                    # (i + 0.5) / -1 + 130 = 129 - i + 0.5, exactly
    below = (-6.0 + 1024.0) / 1024.0
    for name, g in got.items():
        assert not np.isclose(np.abs(g[..., 3]), below).any() and not np.isclose(np.abs(g[..., 3]) - 1.0, below).any(), name
    assert len(np.unique(got["mirrored-y"][..., 3])) == 5 and len(np.unique(plain[..., 3])) == 5
    assert np.isclose(got["no-ground-plane"][..., 3].max(), (99999.0 + 1024.0) / 1024.0)
    assert len(np.unique(got["no-ground-shadows"][..., 3])) == 4                # the low volume (top 2 < GroundZ 3) is gone
    assert np.isclose(got["no-ground-shadows"][..., 3].min(), -((30.0 + 6.0 + 1024.0) / 1024.0) - 1.0)
    assert np.array_equal(got["nan-scale"], np.broadcast_to(np.float32([0.5, 1.0, 0.0, 1.0]), (h, w, 4)))
    stacks = [oracle.render_gbuffer(w, h, scenes.gbuffer_render_desc(), *fc.gbuffer_stack_volumes(n)) for n in (256, 257)]
    assert (stacks[0] != stacks[1]).any()
    assert len(np.unique(stacks[1][..., 3])) == 3          # the ground and the highest tops (7) with shadows on and off, by array order
    assert np.allclose(stacks[1][1, 55], [0.5, 1.0, 0.0, (7.0 + 1024.0) / 1024.0])          # volume 256: top 7, shadows on


def test_gbuffer_ground_plane_and_volume_tops(oracle):
    """RenderGBuffer, non-2.5D: the ground-plane texel is the fixture's (0.5, 1, 0, 1) (GBufferShaderCommon.fxh:21-33: normal +z,
    relativeY 0, w = (z + 1024) / 1024); volume tops overwrite it lowest to highest; shadows disabled => w = -(z + 1024) / 1024 - 1."""
    w, h = 64, 48
    g = oracle.render_gbuffer(w, h, scenes.gbuffer_render_desc(ground_z=0.0))
    assert np.allclose(g, np.broadcast_to(np.float32([0.5, 1.0, 0.0, 1.0]), g.shape), rtol=0, atol=1e-7)
    vols, poly = scenes.height_volume_arrays([
        ([(10, 10), (40, 10), (40, 30), (10, 30)], 0.0, 20.0, True, True),
        ([(30, 20), (60, 20), (60, 44), (30, 44)], 5.0, 40.0, True, False),      # higher, shadows off: drawn last
        ([(2, 36), (12, 36), (7, 46)], 0.0, 8.0, True, True)])
    g = oracle.render_gbuffer(w, h, scenes.gbuffer_render_desc(ground_z=0.0), vols, poly)
    assert np.allclose(g[15, 20], [0.5, 1.0, 0.0, (20.0 + 1024.0) / 1024.0])                     # inside the first box only
    assert np.allclose(g[25, 35], [0.5, 1.0, 0.0, -((45.0 + 1024.0) / 1024.0) - 1.0])            # overlap: the higher volume wins
    assert np.allclose(g[40, 7], [0.5, 1.0, 0.0, (8.0 + 1024.0) / 1024.0])                       # inside the triangle
    assert np.allclose(g[2, 2], [0.5, 1.0, 0.0, 1.0])                                            # bare ground
    # pixel (i, j) is covered iff its centre (i + .5, j + .5) is inside: column 9 is out, column 10 is in
    assert np.allclose(g[15, 9], [0.5, 1.0, 0.0, 1.0]) and not np.allclose(g[15, 10], g[15, 9])
    # the view transform: position 100,50 at scale 0.5 moves the first box to pixels ((10-100)*.5 ...): off screen; RenderGroundPlane off lifts the plane
    g2 = oracle.render_gbuffer(w, h, scenes.gbuffer_render_desc(0.0, (100.0, 50.0), (0.5, 0.5), render_ground_plane=False), vols, poly)
    assert np.allclose(g2, np.broadcast_to(np.float32([0.5, 1.0, 0.0, (99999.0 + 1024.0) / 1024.0]), g2.shape))
    # ground shadows off
    g3 = oracle.render_gbuffer(w, h, scenes.gbuffer_render_desc(3.0, enable_ground_shadows=False))
    assert np.allclose(g3[0, 0], [0.5, 1.0, 0.0, -((3.0 + 1024.0) / 1024.0) - 1.0])
