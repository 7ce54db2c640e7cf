"""The context's grow-on-demand device scratch across a regrow: on ONE context a small call, then a call whose buffer no longer fits
(the old block is freed behind whatever still reads it and a larger one allocated), then the small call again -- every result must be,
bit for bit, what the same call returns on a fresh context.  Nothing here looks at a capacity; the comment at each case names the buffer
and the arithmetic by which the large call crosses that buffer's first capacity (api.hip, `reserve` and its callers)."""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests.lights_common import no_field_uniforms, particle_light_params
from tests.output_common import readback_params

pytestmark = pytest.mark.gpu

CS = 64                                 # chunk size of the particle cases: 4 096 slots = four 1 024-slot blocks per chunk
P, V, A, RC, RD = abi.PLANE_POSITION, abi.PLANE_VELOCITY, abi.PLANE_ATTRIBUTES, abi.PLANE_RENDER_COLOR, abi.PLANE_RENDER_DATA
AMBIENT = (0.03, 0.05, 0.04, 1.0)
_RND = scenes.randomness_table(7)
LAYOUT = scenes.DistanceFieldLayout(16, 16, 16.0, 6, 1.0, 32)       # 16 x 16 slices, six of them
_ATLAS = scenes.build_sdf_atlas(LAYOUT, [(2, (8.0, 8.0, 4.0), (3.0, 2.0, 3.0)), (1, (3.0, 12.0, 9.0), (2.0, 2.0, 4.0))])      # a box and an ellipsoid


def leaves(x):
    """A result (arrays, ctypes records, numbers, tuples of them) as a flat list of byte strings: NaNs and zeros of either sign count by their bits."""
    if isinstance(x, (tuple, list)):
        return [leaf for v in x for leaf in leaves(v)]
    if isinstance(x, np.ndarray):
        return [repr((x.dtype.str, x.shape)).encode(), np.ascontiguousarray(x).tobytes()]
    if isinstance(x, (C.Structure, C.Array)):
        return [bytes(x)]
    return [repr(x).encode()]


def same(got, want):
    got, want = leaves(got), leaves(want)
    return len(got) == len(want) and all(np.array_equal(np.frombuffer(g, np.uint8), np.frombuffer(w, np.uint8)) for g, w in zip(got, want))


def check_sequence(calls):
    """calls: [(name, f(ctx) -> result)] made in order on one context; each result against the same call on a context of its own."""
    warm = native.Context(0)
    got = [f(warm) for _, f in calls]
    warm.close()
    for (name, f), g in zip(calls, got):
        fresh = native.Context(0)
        want = f(fresh)
        fresh.close()
        assert same(g, want), "%s: differs from the same call on a fresh context" % name


# ---- c->staging ---------------------------------------------------------------------------------------------------------------------
def divide(n):
    num = scenes.uniform(31 + n, (n,), -50.0, 50.0)
    den = scenes.uniform(32 + n, (n,), 0.5, 9.0)
    return lambda c: c.debug_divide(num, den)


def sample(n):
    pos = scenes.uniform(41 + n, (n, 3), -2.0, 18.0)
    dfu = LAYOUT.uniforms()

    def run(c):
        sdf = native.DistanceFieldTexture(c, _ATLAS)
        out = sdf.sample(dfu, pos)
        sdf.close()
        return out
    return run


def test_staging_regrown_by_debug_divide():
    # staging starts at max(need, 1 MiB): 16 pairs need 4 arrays x 4 B x 16 = 256 B (1 MiB block); 70 000 pairs need 4 x 4 x 70 000 =
    # 1 120 000 B > 1 048 576
    check_sequence([("divide 16", divide(16)), ("divide 70 000", divide(70000)), ("divide 16 again", divide(16))])


def test_staging_regrown_by_sdf_sample():
    # 8 positions go through a pinned slot; the 16 pairs put staging at 1 MiB; 300 000 positions are 16 B x 300 000 = 4 800 000 B > 4 MiB,
    # so the call leaves the pinned path and needs 4 800 000 B of staging > 1 048 576
    check_sequence([("sample 8", sample(8)), ("divide 16", divide(16)), ("sample 300 000", sample(300000)), ("sample 8 again", sample(8)),
                    ("divide 16 again", divide(16))])


# ---- lights: pinned ring slots, c->d_recs, tickets and partials ----------------------------------------------------------------------
def lights(n, w=32, h=32, fmt=abi.LIGHTMAP_FLOAT4, split=0, radius=3.0, ramp=(6.0, 14.0), seed=5):
    arr = scenes.random_lights(seed + n, n, w, h, z=(2.0, 12.0), radius=radius, ramp=ramp, casts_shadows=False)

    def run(c):
        c.set_light_split(split)
        lm = native.Lightmap(c, w, h, fmt)
        native.render_sphere_lights(c, arr, scenes.environment(), no_field_uniforms(), None, None, AMBIENT, lm)
        out = lm.download()
        lm.close()
        c.set_light_split(0)
        return out
    return run


def probes(n_lights, n_probes):
    arr = scenes.random_lights(77 + n_lights, n_lights, 32, 32, z=(2.0, 12.0), radius=3.0, ramp=(6.0, 14.0), casts_shadows=False)
    pp = np.ones((n_probes, 4), np.float32)
    pp[:, :3] = scenes.uniform(78 + n_probes, (n_probes, 3), 0.0, 32.0)
    pn = np.zeros((n_probes, 4), np.float32)
    pn[:, 2] = 1.0
    return lambda c: native.render_light_probes(c, arr, pp, pn, scenes.environment(), no_field_uniforms(), None)


def test_light_records_regrown_by_sphere_lights():
    # d_recs starts at 256 records (n < 256): 8 lights fit, 300 > 256
    check_sequence([("8 lights", lights(8)), ("300 lights", lights(300)), ("8 lights again", lights(8))])


def test_light_records_and_pairs_regrown_by_light_probes():
    # d_recs: 2 lights fit the first 256 records, 300 > 256.  d_probe_pairs starts at 65 536 pairs: 2 x 8 = 16 fit; 300 lights x 300
    # probes = 90 000 > 65 536
    check_sequence([("2 lights x 8 probes", probes(2, 8)), ("300 lights x 8 probes", probes(300, 8)), ("300 lights x 300 probes", probes(300, 300)),
                    ("2 lights x 8 probes again", probes(2, 8))])


def test_pinned_ring_slots_regrown_and_reused():
    # a ring slot starts at 64 KiB: 8 light vertices are 8 x 128 B = 1 KiB; 600 are 76 800 B > 65 536.  A probe block of 2 lights and
    # 2 000 probes is 256 + 3 x 16 B x 2 000 = 96 256 B > 65 536.  Then six small calls in a row: more than the ring's four slots, so
    # every slot -- the regrown ones included -- is taken again.
    assert C.sizeof(abi.LightVertex) == 128
    calls = [("8 lights", lights(8)), ("600 lights", lights(600)), ("2 x 8 probes", probes(2, 8)), ("2 x 2 000 probes", probes(2, 2000))]
    calls += [("small call %d" % i, lights(8 + i) if i % 2 == 0 else probes(2, 8 + i)) for i in range(6)]
    check_sequence(calls)


def test_tickets_and_partials_regrown_by_a_larger_lightmap():
    # d_light_tickets holds tiles x 4 words, exact: a 32 x 32 lightmap is 2 x 2 = 4 tiles of 16 x 16, one of 256 x 256 is 16 x 16 = 256 > 4.
    # The forced split (two workgroups per tile; 32 lights lie inside its 16 .. 1 024 range) puts every block slot of the launch into
    # d_light_partials, which therefore grows with the tiles as well.  d_group_order is NOT reached by these sizes: a launch gets a
    # group order from 512 groups of tiles on (test_group_order_regrown_by_a_larger_lightmap).
    for split in (0, 2):
        check_sequence([("32 x 32, split %d" % split, lights(32, 32, 32, split=split)),
                        ("256 x 256, split %d" % split, lights(32, 256, 256, split=split, radius=20.0, ramp=(40.0, 90.0))),
                        ("32 x 32 again, split %d" % split, lights(32, 32, 32, split=split))])


def test_group_order_regrown_by_a_larger_lightmap():
    # d_group_order holds 2 x groups entries.  Whole frames are dealt in groups of 6 x 6 tiles = 96 x 96 pixels, and a table is made
    # from 512 groups on: 2 208 x 2 208 is 23 x 23 = 529 groups (room for 1 058), 3 168 x 3 168 is 33 x 33 = 1 089 > 1 058.  (The only
    # sizes at which this buffer can be regrown at all; RGBA8 lightmaps and 16 small lights keep the case short.)
    big = dict(fmt=abi.LIGHTMAP_RGBA8, radius=40.0, ramp=(80.0, 160.0))
    check_sequence([("2 208 x 2 208", lights(16, 2208, 2208, **big)), ("3 168 x 3 168", lights(16, 3168, 3168, **big)),
                    ("2 208 x 2 208 again", lights(16, 2208, 2208, **big))])


def test_records_regrown_under_a_pass_in_flight():
    # The synchronise-before-free: a pass of 8 lights is queued on lightmap A (no statistics: the call returns with the pass in flight)
    # and at once one of 300 lights on lightmap B, which frees the 256 records A's pass may still be reading (300 > 256).
    few = scenes.random_lights(13, 8, 32, 32, z=(2.0, 12.0), radius=3.0, ramp=(6.0, 14.0), casts_shadows=False)
    many = scenes.random_lights(305, 300, 32, 32, z=(2.0, 12.0), radius=3.0, ramp=(6.0, 14.0), casts_shadows=False)
    env, dfu = scenes.environment(), no_field_uniforms()
    c = native.Context(0)
    a, b = native.Lightmap(c, 32, 32), native.Lightmap(c, 32, 32)
    native.render_sphere_lights(c, few, env, dfu, None, None, AMBIENT, a)
    native.render_sphere_lights(c, many, env, dfu, None, None, AMBIENT, b)
    got_a, got_b = a.download(), b.download()
    a.close(); b.close(); c.close()
    for name, arr, got in (("A", few, got_a), ("B", many, got_b)):
        fresh = native.Context(0)
        lm = native.Lightmap(fresh, 32, 32)
        native.render_sphere_lights(fresh, arr, env, dfu, None, None, AMBIENT, lm)
        want = lm.download()
        lm.close(); fresh.close()
        assert same(got, want), "lightmap %s differs from the same pass on a fresh context" % name


# ---- c->d_field_params: one block shared by three entry points -----------------------------------------------------------------------
def slices(n_obstructions):
    obs = scenes.obstruction_array(scenes.random_obstructions(60 + n_obstructions, n_obstructions, (16, 16), size_lo=1.0, size_hi=4.0, z_hi=14.0))
    desc = scenes.render_desc(LAYOUT)

    def run(c):
        sdf = native.DistanceFieldTexture(c, None, abi.SDF_UNORM16, size=(LAYOUT.atlas_width, LAYOUT.atlas_height))
        sdf.render_slices(desc, list(range(0, LAYOUT.slice_count, 3)), obs)
        out = sdf.download()
        sdf.close()
        return out
    return run


def gbuffer_volumes(padded_vertices):
    volumes = [([(3.0, 4.0), (14.0, 5.0), (12.0, 13.0), (5.0, 11.0)], 0.0, 6.0), ([(18.0, 17.0), (29.0, 19.0), (24.0, 30.0)], 2.0, 9.0),
               ([(2.0, 20.0), (12.0, 21.0), (13.0, 29.0), (6.0, 25.0), (3.0, 30.0)], 1.0, 3.0)]
    vols, poly = scenes.height_volume_arrays(volumes)
    poly = np.ascontiguousarray(poly, np.float32).reshape(-1, 2)
    # vertices no volume names still travel in the polygon array
    poly = np.concatenate([poly, scenes.uniform(9, (max(0, padded_vertices - len(poly)), 2), 0.0, 32.0)])
    desc = scenes.gbuffer_render_desc()

    def run(c):
        gb = native.GBufferTexture(c, None, abi.GBUFFER_FLOAT4, size=(32, 32))
        gb.render(desc, vols, poly)
        out = gb.download()
        gb.close()
        return out
    return run


def gbuffer_meshes(boxes):
    r = scenes.uniform(500 + boxes, (boxes, 4))
    top = []
    for k in range(boxes):
        x, y = 1.0 + r[k, 0] * 24.0, 1.0 + r[k, 1] * 24.0
        top.append(scenes.top_face_mesh([(x, y), (x + 5.0, y), (x + 5.0, y + 4.0), (x, y + 4.0)], 0.0, float(np.float32(1.0 + 20.0 * r[k, 2]))))
    top = np.concatenate(top)
    desc = scenes.gbuffer_mesh_desc(extent_z=64.0)

    def run(c):
        gb = native.GBufferTexture(c, None, abi.GBUFFER_FLOAT4, size=(32, 32))
        gb.render_meshes(desc, top, None, None, [])
        out = gb.download()
        gb.close()
        return out
    return run, len(top) // 3


def test_field_params_regrown_by_its_three_users():
    # The block starts at 64 KiB and is then regrown to twice what the call needs.
    #   render_slices: 4 obstruction records are 4 x 80 B (the 64 KiB block); 900 are 72 000 B > 65 536 -> a block of ~144 KB.
    #   GBufferTexture.render: a polygon array of 20 000 vertices is 160 000 B > 2 x (72 000 + 128) -> a block of ~320 KB.
    #   render_meshes on 32 x 32 (one 64 x 64 block of pixels): 192 + 16 + 32 + 4 = 244 B per triangle and 2 + 1 500 triangles make
    #   366 488 B > 2 x (160 000 + 192 + 64).
    # One context, in this order, because the three share the buffer; a small call of each kind before and after.
    meshes_small, _ = gbuffer_meshes(2)
    meshes_large, triangles = gbuffer_meshes(750)
    assert triangles == 1500
    check_sequence([("4 obstructions", slices(4)), ("3 volumes", gbuffer_volumes(0)), ("4 triangles", meshes_small),
                    ("900 obstructions", slices(900)), ("20 000 polygon vertices", gbuffer_volumes(20000)), ("1 500 triangles", meshes_large),
                    ("4 obstructions again", slices(4)), ("3 volumes again", gbuffer_volumes(0)), ("4 triangles again", meshes_small)])


# ---- particle lights, read-back and raster: block counts, per-chunk counts, records ------------------------------------------------
_PARTICLES = []
for _c in range(3):
    _pos, _vel, _ = scenes.make_particles(300 + _c, CS * CS, pos_hi=(32, 32, 8))
    _color = scenes.uniform(310 + _c, (CS * CS, 4), 0.05, 0.6)
    _data = np.zeros((CS * CS, 4), np.float32)
    _data[:, 0] = scenes.uniform(320 + _c, (CS * CS,), 0.5, 2.0)
    _data[:, 1] = scenes.uniform(330 + _c, (CS * CS,), 0.0, 6.0)
    _PARTICLES.append(((P, _pos), (V, _vel), (RC, _color), (RD, _data)))


def with_system(c, chunks, f):
    eng = native.Engine(c, CS, _RND)
    sysm = native.System(eng)
    for k in range(chunks):
        sysm.add_chunk()
        for plane, data in _PARTICLES[k]:
            sysm.upload(k, plane, data)
    out = f(sysm)
    sysm.close(); eng.close()
    return out


def particle_lights(chunks):
    params = particle_light_params(2.0, 5.0, color=(0.02, 0.03, 0.025, 1.0))

    def run(c):
        def f(sysm):
            lm = native.Lightmap(c, 32, 32)
            lm.clear(AMBIENT)
            native.render_particle_lights(c, sysm, params, scenes.environment(), no_field_uniforms(), None, None, lm, quad_counts=[CS * CS] * chunks)
            out = lm.download()
            lm.close()
            return out
        return with_system(c, chunks, f)
    return run


def readback(chunks, capacity):
    params = readback_params(size=(2.0, 3.0))

    def run(c):
        def f(sysm):
            recs, n = sysm.readback(params, element_counts=[CS * CS - 7] * chunks, capacity=capacity)
            return n, np.frombuffer(bytes(recs), np.uint8)[:min(n, capacity) * C.sizeof(abi.ReadbackDrawCall)].copy()
        return with_system(c, chunks, f)
    return run


def raster(chunks):
    params = scenes.rasterize_params(size=(1.5, 1.5), global_color=(1.0, 0.9, 0.8, 0.5))

    def run(c):
        def f(sysm):
            lm = native.Lightmap(c, 32, 32)
            lm.clear((0.0, 0.0, 0.0, 0.0))
            stats = native.render_particles(sysm, params, lm, quad_counts=[CS * CS - 5] * chunks, want_stats=True)
            out = lm.download()
            lm.close()
            return stats, out
        return with_system(c, chunks, f)
    return run


def test_particle_light_scratch_regrown_by_more_chunks():
    # d_pl_blocks holds 2 x blocks: one chunk is 4 blocks (room for 8), three chunks are 12 > 8.  d_pl_quads holds 2 x chunk_count:
    # room for 2, then 3 > 2.  d_pl_recs starts at 4 096 records: one full chunk is exactly 4 096, three are 12 288 > 4 096 (every
    # particle is alive).
    check_sequence([("one chunk", particle_lights(1)), ("three chunks", particle_lights(3)), ("one chunk again", particle_lights(1))])


def test_readback_scratch_regrown_by_more_chunks_and_a_larger_capacity():
    # d_rb_blocks: 4 blocks (room for 8), then 12 > 8.  d_rb_elems: room for 2, then 3 > 2.  d_rb is exactly `capacity` records:
    # 1 000 (fewer than the chunk's live particles: the list is cut), then 13 000 > 1 000.
    check_sequence([("one chunk, capacity 1 000", readback(1, 1000)), ("three chunks, capacity 13 000", readback(3, 13000)),
                    ("one chunk again", readback(1, 1000))])


def test_raster_quads_regrown_by_more_chunks():
    # d_raster_quads holds 2 x chunk_count: room for 2 after one chunk, then 3 > 2
    check_sequence([("one chunk", raster(1)), ("three chunks", raster(3)), ("one chunk again", raster(1))])


# ---- brightness ---------------------------------------------------------------------------------------------------------------------
def brightness(size, accuracy):
    rng = np.random.RandomState(size + accuracy)
    texels = rng.uniform(0.0, 3.0, (size, size, 4)).astype(np.float32)
    table = np.linspace(0.05, 3.2, 64).astype(np.float32)

    def run(c):
        lm = native.Lightmap(c, size, size)
        lm.upload(texels)
        level, values = lm.luminance(accuracy_factor=accuracy)
        result, buckets = lm.histogram(table, accuracy_factor=accuracy)
        lm.close()
        return level, values, result, buckets
    return run


def test_brightness_scratch_regrown_by_a_larger_lightmap():
    # level (exact): at AccuracyFactor 0 a 32 x 32 lightmap's level is 16 x 16 = 256 values, a 256 x 256 one's 128 x 128 = 16 384 > 256.
    # partials (256 floats per workgroup of 1 024 values): 1 workgroup, then 16 > 1.
    # mip (2 x level 3, used past level 3): at AccuracyFactor 5 the 32 x 32 lightmap stops at level 4 with 2 x (2 x 2) = 8 floats, the
    # 256 x 256 one reaches level 5 with 2 x (16 x 16) = 512 > 8.
    check_sequence([("32 x 32, level 0", brightness(32, 0)), ("32 x 32, level 4", brightness(32, 5)), ("256 x 256, level 0", brightness(256, 0)),
                    ("256 x 256, level 5", brightness(256, 5)), ("32 x 32, level 0 again", brightness(32, 0)), ("32 x 32, level 4 again", brightness(32, 5))])


# ---- System: spawn positions and the chunk table -------------------------------------------------------------------------------------
# (System::d_slots is left to the existing tests: its copying path starts at 8 MiB of slot indices, a chunk size of 1 449)
def spawn_stage(sysm, count):
    positions = [(2.0 + 0.09 * i, 30.0 - 0.07 * i, 0.5 + 0.01 * i) for i in range(count)]
    p, buf = scenes.position_buffer_spawn_params(CS, 100, 1900, 4321, (0.42 * 253, 0.77 * 127), positions, life_constant=3.3,
                                                 position=((0, 0, 0), (1, 1, 1), (0, 0, 0), scenes.FORMULA_SPHERICAL),
                                                 velocity=((1, 2, 3), (6, 6, 6), (0, 0, 0), scenes.FORMULA_SPHERICAL), life=(3.3, 2.7, 0.0))
    d = abi.StepDesc()
    d.FirstChunk, d.ChunkCount = 0, -1
    d.System = scenes.system_uniforms(CS)
    d.Update = abi.UpdateParams.default()
    d.UpdateMode = abi.UPDATE_POSITIONS
    d.SpawnCount = 1
    d.Spawns[0].ChunkIndex = 0
    d.Spawns[0].Kind = abi.SPAWN_POSITION_BUFFER
    d.Spawns[0].Params = p
    zero = np.zeros((CS * CS, 4), np.float32)
    for plane in (P, V, A):
        sysm.upload(0, plane, zero)                 # every stage starts from the same (empty) chunk
    sysm.set_spawn_positions(0, buf)
    sysm.step(d)
    return [sysm.download(0, plane) for plane in (P, V, A)]


def with_fresh_system(c, cs, f):
    eng = native.Engine(c, cs, _RND)
    sysm = native.System(eng)
    out = f(sysm)
    sysm.close(); eng.close()
    return out


def check_system_stages(cs, stages):
    """stages: [(name, f(system) -> result)] on ONE system (the buffers are the system's); each against a new system on a fresh context."""
    warm = native.Context(0)
    got = with_fresh_system(warm, cs, lambda s: [f(s) for _, f in stages])
    warm.close()
    for (name, f), g in zip(stages, got):
        fresh = native.Context(0)
        want = with_fresh_system(fresh, cs, f)
        fresh.close()
        assert same(g, want), "%s: differs from a new system on a fresh context" % name
    return got


def test_spawn_positions_regrown_on_one_system():
    # spawn_positions[k] holds the count rounded up to 128: 100 positions leave room for 128, then 300 > 128
    def stage(n):
        def f(sysm):
            if sysm.chunk_count() == 0:
                sysm.add_chunk()
            return spawn_stage(sysm, n)
        return ("%d positions" % n, f)
    got = check_system_stages(CS, [stage(100), stage(300), stage(100)])
    for g in got:
        assert (g[0][100:1901, 3] > 0).all(), "the spawn range is alive"


def test_chunk_table_regrown_by_the_65th_chunk():
    # System::d_table starts at 64 pointers (n < 64 ? 64 : 2 n): 64 chunks fit, the 65th does not.  An 8 x 8 chunk size keeps it small.
    cs = 8
    pos, vel, attr = scenes.make_particles(900, cs * cs, dead_fraction=0.3)
    d = abi.StepDesc()
    d.FirstChunk, d.ChunkCount = 0, -1
    d.System = scenes.system_uniforms(cs, friction=0.1, life_decay=1.2)
    d.Update = abi.UpdateParams.default()
    d.UpdateMode = abi.UPDATE_POSITIONS
    d.OpCount = 1
    d.Ops[0].Type = abi.OP_GRAVITY
    d.Ops[0].u.Gravity = scenes.gravity_params([((16.0, 16.0, 0.0), 150.0, 60.0, 1)])

    def stage(n):
        def f(sysm):
            while sysm.chunk_count() < n:
                sysm.add_chunk()
            for k in range(n):                      # every stage starts from the same particles
                for plane, data in ((P, pos + np.float32(k)), (V, vel), (A, attr)):
                    sysm.upload(k, plane, data)
            sysm.step(d)
            return sysm.live_counts(), [sysm.download(k, plane) for k in (0, n - 1) for plane in (P, V)]
        return ("%d chunks" % n, f)
    got = check_system_stages(cs, [stage(64), stage(65), stage(65)])
    assert got[1][0].shape == (65,) and (got[1][0] > 0).all()
