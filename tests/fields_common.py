"""Shared scene builders of the distance-field generation tests (CPU oracle and HIP path run the same cases)."""
import json
import os

import numpy as np

from illuminant_amd import abi, scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_generation_fixture():
    with open(os.path.join(GOLDEN, "distance_field_generation.json")) as f:
        return json.load(f)


def fixture_layout(doc):
    fd = doc["field"]
    return scenes.DistanceFieldLayout(fd["virtual_width"], fd["virtual_height"], fd["virtual_depth"], fd["requested_slices"],
                                      fd["resolution"], int(fd["maximum_encoded_distance"]))


def fixture_case_inputs(case):
    """(obstruction array | None, volumes | None, polygon | None) of one fixture case."""
    if case["kind"] == "obstruction":
        o = case["obstruction"]
        return scenes.obstruction_array([(o["type"], o["center"], o["size"], o["rotation"])]), None, None
    v = case["volume"]
    vols, poly = scenes.height_volume_arrays([(v["polygon"], v["z_base"], v["height"])])
    return None, vols, poly


def texel_of(atlas, layout, x, y, virtual_slice):
    """Stored code of virtual slice `virtual_slice` at slice-local texel (x, y): channel s % 3 of physical slice s // 3."""
    p, c = virtual_slice // 3, virtual_slice % 3
    ox = (p % layout.column_count) * layout.slice_width
    oy = (p // layout.column_count) * layout.slice_height
    return int(atlas[oy + y, ox + x, c])


def all_triplets(layout):
    return list(range(0, layout.slice_count, 3))


def mixed_scene(seed=21, n=24, extent=(256, 192), depth=96.0, slices=12, resolution=0.5, dynamic_fraction=0.0):
    """Every obstruction type with rotations + two height volumes (one concave)."""
    layout = scenes.DistanceFieldLayout(extent[0], extent[1], depth, slices, resolution, 128)
    obs = scenes.random_obstructions(seed, n, extent, size_lo=6.0, size_hi=40.0, z_hi=48.0, dynamic_fraction=dynamic_fraction)
    # a big rotated box whose corners poke out of DistanceFunctionVertexShader's quad (the cut is part of the semantics)
    obs.append((abi.OBSTRUCTION_BOX, (extent[0] * 0.5, extent[1] * 0.5, 10.0), (90.0, 90.0, 90.0), 0.78539816, False))
    volumes = [
        ([(20.0, 30.0), (90.0, 24.0), (100.0, 80.0), (60.0, 50.0), (24.0, 90.0)], 0.0, 30.0, True),    # concave
        ([(150.0, 100.0), (230.0, 110.0), (200.0, 170.0)], 8.0, 20.0, False),
    ]
    return layout, obs, volumes


# ---- edge scenes of the generation kernels (csrc/fields.hip): list, batch and range edges ------------------------------------------
# Each builder returns (desc, (obstruction array | None, volumes | None, polygon | None), first slices).  The census functions restate
# the host's and the kernel's own comparisons (api.hip, fields.hip) in float32, so a CPU test can assert that a scene reaches both sides
# of the threshold it was built for.

FIELD_TILE_W, FIELD_TILE_H = 32, 8          # kFieldTileW, kFieldTileH
FIELD_LIST_CAPACITY = 2048                  # kFieldListCapacity
FIELD_SORT_CAPACITY = 512                   # kFieldSortCapacity
F = np.float32


def field_desc(virtual, depth, slice_size, slice_count, columns, rows, max_encoded, z_offset=0.0, flt=-1):
    """abi.DistanceFieldRenderDesc filled directly, for what DistanceFieldLayout cannot express (it clamps the resolution to [0.05, 1]):
    the atlas is (slice width x columns) x (slice height x rows); the inverse scale factors are float32(virtual / slice) as in
    scenes.render_desc."""
    assert slice_count % 3 == 0 and slice_count // 3 <= columns * rows
    d = abi.DistanceFieldRenderDesc()
    d.VirtualWidth, d.VirtualHeight, d.VirtualDepth, d.ZOffset = int(virtual[0]), int(virtual[1]), float(depth), float(z_offset)
    d.SliceWidth, d.SliceHeight, d.SliceCount = int(slice_size[0]), int(slice_size[1]), int(slice_count)
    d.ColumnCount, d.RowCount = int(columns), int(rows)
    d.MaximumEncodedDistance = float(max_encoded)
    d.InvScaleFactorX = float(F(virtual[0] / slice_size[0]))
    d.InvScaleFactorY = float(F(virtual[1] / slice_size[1]))
    d.DynamicFlagFilter = flt
    return d


def desc_triplets(d):
    return list(range(0, d.SliceCount, 3))


def atlas_shape(d):
    return (d.SliceHeight * d.RowCount, d.SliceWidth * d.ColumnCount, 4)


def render_oracle_desc(oracle, d, inputs, slices, fmt=abi.SDF_UNORM16, clear_source=None, initial=None):
    atlas = np.zeros(atlas_shape(d), np.uint16) if initial is None else initial.copy()
    return oracle.render_distance_field_slices(atlas, fmt, d, slices, inputs[0], inputs[1], inputs[2], clear_source=clear_source)


def render_gpu_desc(ctx, d, inputs, slices, fmt=abi.SDF_UNORM16, clear_source=None, initial=None, keep=False):
    from illuminant_amd import native
    h, w, _ = atlas_shape(d)
    sdf = native.DistanceFieldTexture(ctx, initial, fmt, size=(w, h))
    sdf.render_slices(d, slices, inputs[0], inputs[1], inputs[2], clear_source=clear_source)
    out = sdf.download()
    if keep:
        return out, sdf
    sdf.close()
    return out


_ORACLE_ATLASES = {}


def cached_oracle_atlas(oracle, key, d, inputs, slices, fmt):
    """One oracle render per (scene, format) and session, shared by the tests that need it; callers must not write into it."""
    k = (key, fmt)
    if k not in _ORACLE_ATLASES:
        a = render_oracle_desc(oracle, d, inputs, slices, fmt)
        a.setflags(write=False)
        _ORACLE_ATLASES[k] = a
    return _ORACLE_ATLASES[k]


def scattered_obstructions(seed, n, lo, hi, size_lo, size_hi, rotated_fraction=0.5, dynamic_fraction=0.0, types=(0, 1, 2, 3, 4)):
    """n obstructions of every type, centres uniform in the box lo .. hi, sizes uniform per axis, about `rotated_fraction` of them rotated."""
    c = scenes.uniform(seed + 1, (n, 3))
    s = scenes.uniform(seed + 2, (n, 3), size_lo, size_hi)
    t = scenes.uniform(seed + 3, (n,))
    r = scenes.uniform(seed + 4, (n, 2))
    dy = scenes.uniform(seed + 5, (n,))
    out = []
    for i in range(n):
        centre = tuple(float(lo[k] + c[i, k] * (hi[k] - lo[k])) for k in range(3))
        rot = float((r[i, 1] * 2.0 - 1.0) * np.pi) if r[i, 0] < rotated_fraction else 0.0
        out.append((types[min(int(t[i] * len(types)), len(types) - 1)], centre, tuple(float(x) for x in s[i]), rot, bool(dy[i] < dynamic_fraction)))
    return out


def set_orientation(o, q):
    for k in range(4):
        o.Orientation[k] = float(F(q[k]))


# -- a. sort threshold, b. obstruction batches: a 72 x 40 world at resolution 1, 6 slices 4 units apart, MaximumEncodedDistance 16

def small_world_layout():
    return scenes.DistanceFieldLayout(72, 40, 24.0, 6, 1.0, 16)


def sort_scene(n):
    """n small obstructions whose centres lie in (44.5, 51.5) x (12.5, 27.5): a quad reaches max|size| + 16 + 4 >= 20.5 units from its
    centre, so every quad touches every 32 x 8 tile of the 72 x 40 slice and every tile's list holds exactly n entries."""
    layout = small_world_layout()
    obs = scattered_obstructions(700 + n, n, (44.5, 12.5, 0.0), (51.5, 27.5, 24.0), 0.5, 3.0)
    return scenes.render_desc(layout), (scenes.obstruction_array(obs), None, None), all_triplets(layout)


def tied_sort_scene():
    """300 copies of one rotated box (one centre, one size: equal sort keys on every tile, ranked by list position alone) between two
    halves of 100 scattered obstructions."""
    layout = small_world_layout()
    others = scattered_obstructions(811, 100, (0.0, 0.0, 0.0), (72.0, 40.0, 24.0), 0.5, 3.0)
    tied = [(abi.OBSTRUCTION_BOX, (48.0, 20.0, 12.0), (2.0, 1.5, 1.0), 0.3, False)] * 300
    return scenes.render_desc(layout), (scenes.obstruction_array(others[:50] + tied + others[50:]), None, None), all_triplets(layout)


# the deliberately placed records: clearly larger shapes in the corners, around z = 21 where the scattered ones (z <= 10, sizes <= 3) leave room
PLACED_OBSTRUCTIONS = {
    2047: (abi.OBSTRUCTION_BOX, (8.0, 6.0, 21.0), (7.0, 5.0, 2.0), 0.0, True),
    2048: (abi.OBSTRUCTION_ELLIPSOID, (64.0, 6.0, 21.0), (7.0, 5.0, 2.5), 0.4, True),
    4096: (abi.OBSTRUCTION_CYLINDER, (8.0, 34.0, 21.0), (6.0, 6.0, 2.0), 0.0, True),
}


def batch_scene_list(n, dynamic_fraction=0.0):
    obs = scattered_obstructions(900 + n, n, (0.0, 0.0, 0.0), (72.0, 40.0, 10.0), 0.5, 3.0, dynamic_fraction=dynamic_fraction)
    placed = sorted(i for i in PLACED_OBSTRUCTIONS if i < n)
    for i in placed:
        obs[i] = PLACED_OBSTRUCTIONS[i]
    return obs, placed


def batch_scene(n, dynamic_fraction=0.0, flt=-1):
    """n obstructions scattered over the whole world below z = 13; the records at indices 2047, 2048 and 4096 (those below n) are the
    placed ones.  With a dynamic fraction and flt = 1 the host drops the static records first, which moves the batch boundary away
    from the caller's indices (the placed records are dynamic)."""
    layout = small_world_layout()
    obs, _ = batch_scene_list(n, dynamic_fraction)
    return scenes.render_desc(layout, dynamic_flag_filter=flt), (scenes.obstruction_array(obs), None, None), all_triplets(layout)


# -- c. volume batches: a 200 x 120 world at resolution 0.5

def volume_world_layout(max_encoded=24):
    return scenes.DistanceFieldLayout(200, 120, 24.0, 6, 0.5, max_encoded)


def placed_volume_indices(n):
    return sorted({i for i in (2047, 2048, 4095) if i < n} | {n - 1})


def volume_batch_list(n):
    r = scenes.uniform(1500 + n, (n, 6))
    volumes = []
    for v in range(n):
        cx, cy, rad = r[v, 0] * 200.0, r[v, 1] * 120.0, 0.5 + r[v, 2] * 2.5
        nv = 1 + (v % 5)
        ang = np.sort(scenes.uniform(40000 + v, (nv,)) * 2 * np.pi)
        volumes.append(([(float(cx + rad * np.cos(a_)), float(cy + rad * np.sin(a_))) for a_ in ang], float(r[v, 3] * 6), float(1 + r[v, 4] * 3)))
    corners = [(14.0, 12.0), (186.0, 12.0), (14.0, 108.0), (186.0, 108.0)]
    for k, i in enumerate(placed_volume_indices(n)):
        cx, cy = corners[k]
        volumes[i] = ([(float(cx + 9.0 * np.cos(a_)), float(cy + 9.0 * np.sin(a_))) for a_ in np.arange(5) * (2 * np.pi / 5) + 0.2 * k], 17.0, 5.0)
    return volumes


def volume_batch_scene(n, max_encoded=24):
    """n small height volumes (1 to 5 vertices, radii 0.5 to 3, tops below z = 10); the last volume of each batch of 2048 and of the
    array is a pentagon of radius 9 in a corner at z 17 .. 22."""
    layout = volume_world_layout(max_encoded)
    vols, poly = scenes.height_volume_arrays(volume_batch_list(n))
    return scenes.render_desc(layout), (None, vols, poly), all_triplets(layout)


def far_volume_scene():
    """MaximumEncodedDistance 1400 (beyond sdPolygon's distance cap of 999: no culling at all) with 2049 volumes.  Across a 200 x 120
    world a distance changes by at most 233 units, a sixth of that reach, and the fp16 codes near DISTANCE_ZERO are 0.7 units apart;
    so the volumes lie off the world, 400 to 640 units from its texels (their bounds are expanded by 520 units: every quad still
    covers every tile), where the codes fall below 0.5 and lie twice as dense.  The placed pentagons (indices 2047, 2048) lie
    between the cluster and the world, one nearest to its lower texels and one to its upper ones."""
    layout = volume_world_layout(1400)
    r = scenes.uniform(3549, (2049, 6))
    volumes = []
    for v in range(2049):
        cx, cy, rad = 500.0 + r[v, 0] * 20.0, 380.0 + r[v, 1] * 20.0, 0.5 + r[v, 2] * 2.5
        nv = 1 + (v % 5)
        ang = np.sort(scenes.uniform(50000 + v, (nv,)) * 2 * np.pi)
        volumes.append(([(float(cx + rad * np.cos(a_)), float(cy + rad * np.sin(a_))) for a_ in ang], float(r[v, 3] * 6), float(1 + r[v, 4] * 3)))
    for i, (cx, cy) in ((2047, (455.0, 375.0)), (2048, (492.0, 340.0))):
        volumes[i] = ([(float(cx + 9.0 * np.cos(a_)), float(cy + 9.0 * np.sin(a_))) for a_ in np.arange(5) * (2 * np.pi / 5)], 17.0, 5.0)
    vols, poly = scenes.height_volume_arrays(volumes)
    return scenes.render_desc(layout), (None, vols, poly), all_triplets(layout)


# -- d. ordinary-range guards

def large_world_scene(max_encoded):
    """Virtual 2^22 x 2^22 x 2^21 on 64 x 32 slices (one texel = 2^16 x 2^17 units): of the first triplet (z = 0 .. 2^20) the waves whose
    8 x 8 footprint stays within x, y <= 2^20 (texel columns 0 .. 16, rows 0 .. 8: the first two waves of the first tile) are ordinary,
    every other wave and the whole second triplet (z up to 2^21) is not.  Sizes 2^17 .. 2^19, some exactly 2^20 and one ulp above;
    centres on both sides of 2^20."""
    d = field_desc((1 << 22, 1 << 22), float(1 << 21), (64, 32), 6, 2, 1, max_encoded)
    M = float(1 << 20)
    above = float(np.nextafter(F(M), F(np.inf)))
    obs = [
        (abi.OBSTRUCTION_BOX, (0.5 * M, 0.5 * M, 0.5 * M), (0.25 * M, 0.25 * M, 0.125 * M), 0.0),             # ordinary, unrotated
        (abi.OBSTRUCTION_ELLIPSOID, (0.25 * M, 0.75 * M, 0.25 * M), (0.5 * M, 0.125 * M, 0.25 * M), 0.6),     # ordinary, rotated
        (abi.OBSTRUCTION_SPHEROID, (0.5 * M, 0.25 * M, 0.25 * M), (M, M, M), 0.0),                            # a size of exactly 2^20: still ordinary
        (abi.OBSTRUCTION_CYLINDER, (0.75 * M, 0.5 * M, 0.5 * M), (above, 0.25 * M, 0.25 * M), 0.0),           # one ulp above: not
        (abi.OBSTRUCTION_BOX, (M, M, 0.75 * M), (0.25 * M, 0.5 * M, 0.25 * M), 0.0),                          # centre exactly 2^20: ordinary
        (abi.OBSTRUCTION_OCTAGON, (above, 0.5 * M, 0.5 * M), (0.5 * M, 0.5 * M, 0.25 * M), 0.0),              # centre one ulp beyond: not
        (abi.OBSTRUCTION_ELLIPSOID, (1.5 * M, 1.25 * M, M), (0.5 * M, 0.25 * M, 0.5 * M), -0.9),
        (abi.OBSTRUCTION_BOX, (2.5 * M, 2.0 * M, 1.5 * M), (0.5 * M, 0.25 * M, 0.5 * M), 1.1),
        (abi.OBSTRUCTION_CYLINDER, (3.0 * M, 3.0 * M, 0.5 * M), (0.5 * M, 0.5 * M, 0.5 * M), 0.0),
        (abi.OBSTRUCTION_SPHEROID, (2.0 * M, 3.5 * M, 1.75 * M), (0.375 * M, 0.375 * M, 0.375 * M), 0.0),
        (abi.OBSTRUCTION_OCTAGON, (3.5 * M, 1.0 * M, 1.25 * M), (0.25 * M, 0.25 * M, 0.5 * M), 0.3),
    ]
    return d, (scenes.obstruction_array(obs), None, None), desc_triplets(d)


def z_offset_scene():
    """ZOffset = 2^20 - 24 with depth 48 over 6 slices: the first triplet's slices end at exactly 2^20 (ordinary waves), the second
    triplet's lie above (not); the obstructions' centres straddle z = 2^20 the same way (record bit)."""
    z0 = float((1 << 20) - 24)
    d = field_desc((64, 32), 48.0, (64, 32), 6, 1, 2, 16.0, z_offset=z0)
    obs = [(t, (c[0], c[1], z0 + c[2]), s, r) for (t, c, s, r) in [
        (abi.OBSTRUCTION_BOX, (12.0, 10.0, 4.0), (6.0, 4.0, 5.0), 0.0),
        (abi.OBSTRUCTION_ELLIPSOID, (30.0, 8.0, 20.0), (9.0, 4.0, 6.0), 0.5),
        (abi.OBSTRUCTION_CYLINDER, (50.0, 20.0, 24.0), (5.0, 5.0, 7.0), 0.0),          # cz exactly 2^20: ordinary
        (abi.OBSTRUCTION_SPHEROID, (20.0, 24.0, 24.125), (6.0, 6.0, 6.0), 0.0),        # cz one ulp above: not
        (abi.OBSTRUCTION_OCTAGON, (40.0, 14.0, 36.0), (5.0, 5.0, 6.0), 0.0),
        (abi.OBSTRUCTION_BOX, (56.0, 6.0, 44.0), (4.0, 5.0, 6.0), -0.7),
        (abi.OBSTRUCTION_ELLIPSOID, (8.0, 26.0, 30.0), (5.0, 3.0, 8.0), 0.0),
        (abi.OBSTRUCTION_CYLINDER, (34.0, 26.0, 10.0), (4.0, 4.0, 3.0), 1.2)]]
    return d, (scenes.obstruction_array(obs), None, None), desc_triplets(d)


def small_shapes_scene():
    """A 4 x 4 world on 64 x 64 slices (1/16 unit per texel), MaximumEncodedDistance 2: shapes whose sizes are drawn per axis from
    2^-11 .. 2^-9 -- below 2^-10 a record is not ordinary -- and four with all sizes exactly 2^-10 (ordinary)."""
    d = field_desc((4, 4), 3.0, (64, 64), 6, 2, 1, 2.0)
    n = 40
    obs = scattered_obstructions(1700, n, (0.0, 0.0, 0.0), (4.0, 4.0, 3.0), 0.0, 1.0)
    e = scenes.uniform(1701, (n, 3), -11.0, -9.0)
    obs = [(t, c, tuple(float(F(2.0) ** F(x)) for x in e[i]), r, dyn) for i, (t, c, s, r, dyn) in enumerate(obs)]
    for i in range(4):
        t, c, s, r, dyn = obs[10 * i]
        obs[10 * i] = (t, c, (2.0 ** -10, 2.0 ** -10, 2.0 ** -10), r, dyn)
    return d, (scenes.obstruction_array(obs), None, None), desc_triplets(d)


def tiny_reach_scene(max_encoded):
    """MaximumEncodedDistance at or below 2^-10 on a 1 x 1 world (1/64 unit per texel): a code leaves 0 and 1 only within about
    max_encoded / 2 of a surface, so the surface is the top face of one wide box tilted by fractions of max_encoded across the
    slice, with slices max_encoded / 6 apart around it: the distance changes from texel to texel and slice to slice and stays inside
    the encoded range nearly everywhere.  A box of size 2^-11 (not an ordinary record) lies on the surface."""
    m = float(max_encoded)
    d = field_desc((1, 1), m, (64, 64), 6, 2, 1, m, z_offset=-0.25 * m)
    obs = [(abi.OBSTRUCTION_BOX, (0.5, 0.5, -1.0), (4.0, 4.0, 1.0), 0.0),
           (abi.OBSTRUCTION_BOX, (0.25, 0.75, 0.0), (2.0 ** -11, 2.0 ** -11, 2.0 ** -11), 0.0),
           (abi.OBSTRUCTION_SPHEROID, (0.75, 0.25, 0.25 * m), (2.0 ** -7, 2.0 ** -7, 2.0 ** -7), 0.0)]
    arr = scenes.obstruction_array(obs)
    a, b = 0.15 * m, 0.1 * m                     # half the tilt angles about x and y
    set_orientation(arr[0], (a, b, 0.0, 1.0))    # a unit quaternion to within 1e-6
    return d, (arr, None, None), desc_triplets(d)


# -- e. cull bound

def cull_bound_scene(max_encoded):
    """A 160 x 96 world at resolution 0.5, 9 slices: needles and discs of every type (aspect ratios of 100 : 1 and more, rotated), a
    negative size component, an orientation scaled by 1.3, among ordinary obstructions."""
    layout = scenes.DistanceFieldLayout(160, 96, 36.0, 9, 0.5, max_encoded)
    obs = scattered_obstructions(1900, 24, (0.0, 0.0, 0.0), (160.0, 96.0, 30.0), 2.0, 9.0)
    obs += [
        (abi.OBSTRUCTION_ELLIPSOID, (50.0, 30.0, 8.0), (60.0, 0.5, 0.6), 0.5),          # 120 : 1 needle
        (abi.OBSTRUCTION_ELLIPSOID, (110.0, 60.0, 16.0), (0.25, 40.0, 30.0), -0.8),     # 160 : 1 disc on edge
        (abi.OBSTRUCTION_BOX, (80.0, 70.0, 4.0), (70.0, 0.5, 0.5), 0.25),               # 140 : 1 beam
        (abi.OBSTRUCTION_BOX, (40.0, 60.0, 20.0), (0.3, 30.0, 12.0), 1.0),              # 100 : 1 wall
        (abi.OBSTRUCTION_CYLINDER, (120.0, 20.0, 12.0), (0.4, 0.4, 20.0), 0.0),         # needle along z
        (abi.OBSTRUCTION_CYLINDER, (30.0, 20.0, 26.0), (28.0, 28.0, 0.25), 0.0),        # disc
        (abi.OBSTRUCTION_SPHEROID, (140.0, 70.0, 10.0), (0.3, 0.3, 25.0), 0.0),         # needle
        (abi.OBSTRUCTION_SPHEROID, (90.0, 30.0, 30.0), (30.0, 30.0, 0.3), 0.0),         # disc
        (abi.OBSTRUCTION_OCTAGON, (20.0, 80.0, 14.0), (25.0, 0.4, 10.0), 0.6),          # thin axis
        (abi.OBSTRUCTION_BOX, (130.0, 40.0, 18.0), (10.0, -6.0, 8.0), 0.3),             # negative size component
        (abi.OBSTRUCTION_ELLIPSOID, (70.0, 48.0, 22.0), (12.0, 5.0, 7.0), 0.9),         # orientation scaled by 1.3 below
    ]
    arr = scenes.obstruction_array(obs)
    last = arr[len(obs) - 1]
    set_orientation(last, [1.3 * float(last.Orientation[k]) for k in range(4)])
    return scenes.render_desc(layout), (arr, None, None), all_triplets(layout)


# -- f. slice lists, small slices

def list_scene():
    """12 slices on a 2 x 2 atlas of 48 x 32 slices, for partial lists ([9, 0], [3, 3]) over a sentinel-filled atlas."""
    layout = scenes.DistanceFieldLayout(96, 64, 36.0, 12, 0.5, 32)
    obs = scattered_obstructions(2100, 14, (0.0, 0.0, 0.0), (96.0, 64.0, 36.0), 3.0, 14.0)
    return scenes.render_desc(layout), (scenes.obstruction_array(obs), None, None), all_triplets(layout)


def small_slice_scene(slice_w, slice_h):
    """Slices of slice_w x slice_h texels at 2 units per texel, 36 virtual slices on a 4 x 3 atlas (many slices: a slice this small
    holds few texels), MaximumEncodedDistance 24 so that the codes use the whole range down to 0."""
    d = field_desc((2 * slice_w, 2 * slice_h), 36.0, (slice_w, slice_h), 36, 4, 3, 24.0)
    obs = scattered_obstructions(2200 + slice_w, 10, (0.0, 0.0, 0.0), (2.0 * slice_w, 2.0 * slice_h, 36.0), 1.0, 6.0)
    return d, (scenes.obstruction_array(obs), None, None), desc_triplets(d)


# -- the host's and the kernel's decisions, restated

def px_per_unit(d):
    return F(d.SliceWidth) / F(d.VirtualWidth), F(d.SliceHeight) / F(d.VirtualHeight)


def filtered_records(d, arr):
    """The records ilm_sdf_render_slices keeps, in its order (DynamicFlagFilter)."""
    if arr is None:
        return []
    if d.DynamicFlagFilter < 0:
        return list(arr)
    return [o for o in arr if (o.IsDynamic != 0) == (d.DynamicFlagFilter != 0)]


def quad_bounds(d, records):
    """(n, 4) float32 x0, x1, y0, y1 of DistanceFunctionVertexShader's quads in slice pixels, with api.hip's operations."""
    sx, sy = px_per_unit(d)
    out = np.zeros((len(records), 4), np.float32)
    for k, o in enumerate(records):
        msize = F(F(max(abs(F(o.Size[0])), abs(F(o.Size[1])), abs(F(o.Size[2]))) + F(d.MaximumEncodedDistance)) + F(4.0))
        out[k] = (F(F(o.Center[0]) - msize) * sx, F(F(o.Center[0]) + msize) * sx, F(F(o.Center[1]) - msize) * sy, F(F(o.Center[1]) + msize) * sy)
    return out


def tile_list_lengths(d, arr):
    """Length of every (batch of 2048, tile) obstruction list, by render_slices_kernel's tile test."""
    q = quad_bounds(d, filtered_records(d, arr))
    lengths = []
    for b0 in range(0, len(q), FIELD_LIST_CAPACITY):
        qb = q[b0:b0 + FIELD_LIST_CAPACITY]
        for ty0 in range(0, d.SliceHeight, FIELD_TILE_H):
            for tx0 in range(0, d.SliceWidth, FIELD_TILE_W):
                tminx, tmaxx = F(tx0) + F(0.5), F(tx0 + FIELD_TILE_W - 1) + F(0.5)
                tminy, tmaxy = F(ty0) + F(0.5), F(ty0 + FIELD_TILE_H - 1) + F(0.5)
                lengths.append(int(((qb[:, 0] <= tmaxx) & (qb[:, 1] > tminx) & (qb[:, 2] <= tmaxy) & (qb[:, 3] > tminy)).sum()))
    return lengths


def record_is_ordinary(o):
    """Flag bit 1 of api.hip: sizes in [2^-10, 2^20], centre within 2^20."""
    return all(F(2.0 ** -10) <= F(o.Size[k]) <= F(2.0 ** 20) for k in range(3)) and all(abs(F(o.Center[k])) <= F(2.0 ** 20) for k in range(3))


def wave_census(d, slices, arr):
    """Per 8 x 8 wave footprint of every listed triplet (lanes past the slice's edge vote too, as in the kernel): is it `ordinary`
    (ordinary_coordinates of fields.hip), and do both an ordinary and a non-ordinary record cover one of its texels inside the slice?
    Returns (ordinary waves, other waves, ordinary waves that see both kinds of record)."""
    records = filtered_records(d, arr)
    q = quad_bounds(d, records)
    bits = np.array([record_is_ordinary(o) for o in records], bool)
    lim = F(2.0 ** 20)
    med_ok = F(2.0 ** -10) <= F(d.MaximumEncodedDistance) <= lim
    denom = max(F(d.SliceCount), F(1.0))
    ordinary = other = mixed = 0
    for first in slices:
        physical = first // 3
        col, row = physical % d.ColumnCount, physical // d.ColumnCount
        vpx, vpy = -F(col * d.VirtualWidth), -F(row * d.VirtualHeight)
        z = [F(F(F(first + k) / denom) * F(d.VirtualDepth)) + F(d.ZOffset) for k in (0, 3)]
        z_ok = all(abs(v) <= lim for v in z)
        for ty0 in range(0, d.SliceHeight, FIELD_TILE_H):
            for wx0 in range(0, ((d.SliceWidth + FIELD_TILE_W - 1) // FIELD_TILE_W) * FIELD_TILE_W, 8):
                i = np.arange(wx0, wx0 + 8)
                j = np.arange(ty0, ty0 + 8)
                wx = (F(col * d.SliceWidth) + i.astype(np.float32)) * F(d.InvScaleFactorX) + vpx      # (float)ax: exact integers
                wy = (F(row * d.SliceHeight) + j.astype(np.float32)) * F(d.InvScaleFactorY) + vpy
                is_ordinary = bool(med_ok and z_ok and (np.abs(wx) <= lim).all() and (np.abs(wy) <= lim).all())
                if not is_ordinary:
                    other += 1
                    continue
                ordinary += 1
                ii, jj = i[i < d.SliceWidth], j[j < d.SliceHeight]
                if len(ii) == 0 or len(jj) == 0 or len(q) == 0:
                    continue
                cxp, cyp = ii.astype(np.float32) + F(0.5), jj.astype(np.float32) + F(0.5)
                covers = ((cxp[None, :] >= q[:, 0:1]) & (cxp[None, :] < q[:, 1:2])).any(axis=1) & \
                         ((cyp[None, :] >= q[:, 2:3]) & (cyp[None, :] < q[:, 3:4])).any(axis=1)
                if (covers & bits).any() and (covers & ~bits).any():
                    mixed += 1
    return ordinary, other, mixed


def channels_changed_by(oracle, full, d, inputs, slices, index, fmt=abi.SDF_UNORM16):
    """Texel channels of the oracle's atlas `full` that change when record `index` (of the obstruction array, or of the volume array
    where there are no obstructions) is taken out of the scene."""
    arr, vols, poly = inputs
    src = arr if arr is not None else vols
    keep = [k for k in range(len(src)) if k != index]
    less = (type(src[0]) * len(keep))(*[src[k] for k in keep])
    without = render_oracle_desc(oracle, d, (less, None, None) if arr is not None else (None, less, poly), slices, fmt)
    return int((without != full).sum())


# -- g. G-buffer generation (render_gbuffer_kernel)

GBUFFER_EDGE_SIZE = (130, 37)        # not a multiple of the 64 x 4 tile either way


def gbuffer_edge_volumes():
    """A few volumes on the 130 x 37 target; the fourth's top (-6) lies below every GroundZ used, the fifth's (2) below GroundZ = 3 only."""
    return scenes.height_volume_arrays([
        ([(5, 4), (60, 6), (50, 30), (25, 18), (8, 33)], 0.0, 24.0, True, True),        # concave
        ([(40, 10), (125, 12), (120, 35), (45, 30)], 6.0, 30.0, True, False),
        ([(90, 2), (128, 3), (110, 20)], 0.0, 12.0, True, True),
        ([(62, 2), (80, 2), (80, 16), (62, 16)], -10.0, 4.0, True, True),
        ([(2, 20), (20, 20), (20, 36), (2, 36)], 0.0, 2.0, True, False),
    ])


def gbuffer_edge_descs():
    """name -> desc: mirrored on x, mirrored and stretched on y, no ground plane, no ground shadows over a raised ground, a NaN scale."""
    g = scenes.gbuffer_render_desc
    return {
        "mirrored-x": g(0.0, (130.0, 0.0), (-1.0, 1.0)),
        "mirrored-y": g(0.0, (0.0, 37.0), (1.0, -0.5)),
        "no-ground-plane": g(0.0, render_ground_plane=False),
        "no-ground-shadows": g(3.0, enable_ground_shadows=False),
        "nan-scale": g(0.0, (0.0, 0.0), (float("nan"), 1.0)),
    }


def gbuffer_stack_volumes(n):
    """n squares inside the first 64 x 4 tile, each shifted 0.2 pixels from the one before (every neighbour overlaps), tops 5, 6, 7
    by (index + 1) modulo 3 and the shadow flag by index modulo 2: among equal tops the array order decides which one a pixel shows
    (volume 256 is one of the highest, and the last of them in the array: where it lies, it is the visible one)."""
    return scenes.height_volume_arrays([
        ([(2.0 + 0.2 * k, 0.0), (8.0 + 0.2 * k, 0.0), (8.0 + 0.2 * k, 4.0), (2.0 + 0.2 * k, 4.0)], 0.0, 5.0 + ((k + 1) % 3), True, k % 2 == 0)
        for k in range(n)])


EDGE_SCENES = {
    "sort-512": lambda: sort_scene(512),
    "sort-513": lambda: sort_scene(513),
    "sort-tied": tied_sort_scene,
    "batch-2048": lambda: batch_scene(2048),
    "batch-2049": lambda: batch_scene(2049),
    "batch-4097": lambda: batch_scene(4097),
    "batch-4097-dynamic": lambda: batch_scene(4097, dynamic_fraction=0.55, flt=1),
    "volumes-2048": lambda: volume_batch_scene(2048),
    "volumes-2049": lambda: volume_batch_scene(2049),
    "volumes-4100": lambda: volume_batch_scene(4100),
    "volumes-2049-far": far_volume_scene,
    "range-large-world": lambda: large_world_scene(2.0 ** 20),
    "range-large-world-long-reach": lambda: large_world_scene(1.5 * 2.0 ** 20),
    "range-z-offset": z_offset_scene,
    "range-small-shapes": small_shapes_scene,
    "range-reach-2^-10": lambda: tiny_reach_scene(2.0 ** -10),
    "range-reach-2^-11": lambda: tiny_reach_scene(2.0 ** -11),
    "cull-12": lambda: cull_bound_scene(12),
    "cull-48": lambda: cull_bound_scene(48),
    "lists": list_scene,
    "slices-20x5": lambda: small_slice_scene(20, 5),
    "slices-33x9": lambda: small_slice_scene(33, 9),
}
_SCENES = {}


def edge_scene(name):
    """(desc, inputs, first slices) of EDGE_SCENES[name], built once."""
    if name not in _SCENES:
        _SCENES[name] = EDGE_SCENES[name]()
    return _SCENES[name]


def edge_scene_oracle(oracle, name, fmt):
    d, inputs, slices = edge_scene(name)
    return cached_oracle_atlas(oracle, name, d, inputs, slices, fmt)
