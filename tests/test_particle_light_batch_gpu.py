"""ilm_engine_render_particle_lights_batch on the device: a frame's particle light sources as ONE light list through ONE launch of the
tile kernel, against the chained oracle (tests/particle_light_batch_common.py), against the loop of single calls where the header
promises its bits, and every refusal.  The scenes: `mixed` -- 70 x 45, chunks of 144 slots, six items of 0 / 1 / 3 / 2 / 6 / 1 chunks with
their own templates, one all dead, one system twice -- and `crowded` -- 64 x 48, chunks of 1 600 slots, 5 182 records in three items."""
import ctypes as C
import types

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import light_blend_common as lb
from tests import lights_common as lc
from tests import particle_light_batch_common as bc
from tests.util import ATOL_TIGHT, RTOL, assert_close

pytestmark = pytest.mark.gpu

F4, H4, B4 = abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8


@pytest.fixture(scope="module")
def devices(ctx):
    """(scene name, field format, with G-buffer) -> the scene on the device; made once per module"""
    made = {}

    def get(name, sfmt=abi.SDF_UNORM16, with_gbuffer=False):
        key = (name, sfmt, with_gbuffer)
        if key not in made:
            made[key] = bc.Device(ctx, bc.scene(name), sfmt, with_gbuffer)
        return made[key]
    yield get
    for d in made.values():
        d.close()


def rendered(d, how, fmt=F4, base=None, which=None, rows=(0, None), want_stats=False):
    """the lightmap after d.batch / d.loop onto `base` (None: the ambient frame) -> (texels as downloaded, statistics)"""
    lm = d.lightmap(fmt, base)
    try:
        st = (d.batch if how == "batch" else d.loop)(lm, which, rows, want_stats)
        if how == "batch" and want_stats:
            st = bc.stats_triple(st)
        return lm.download(), st
    finally:
        lm.close()


# ---- 1. against the chained oracle ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,sfmt,with_gbuffer", [("mixed", abi.SDF_UNORM16, False), ("crowded", abi.SDF_UNORM16, False),
                                                    ("mixed", abi.SDF_FP16, False), ("crowded", abi.SDF_FP16, False),
                                                    ("mixed", abi.SDF_UNORM16, True)])
def test_the_batch_is_the_chained_oracle(devices, oracle, name, sfmt, with_gbuffer):
    d = devices(name, sfmt, with_gbuffer)
    want, want_stats = bc.chained_oracle(oracle, d.scene, sfmt, with_gbuffer)
    got, stats = rendered(d, "batch", want_stats=True)
    print("%s: statistics %s, the oracle's %s; largest |got - want| %.3g" % (name, stats, want_stats, float(np.abs(got - want).max())))
    assert stats == want_stats and stats[2] > 1000
    assert_close(got, want, "%s batch vs the chained oracle" % name)
    assert d.engine.last_particle_light_batch()[0::2] == (len(d.scene.items), 1)
    if with_gbuffer:
        assert np.array_equal(got[10:14], bc.ambient_frame(d.scene)[10:14]), "the fullbright band is discarded"
    # without statistics the same bits
    again, _ = rendered(d, "batch")
    assert np.array_equal(again, got)


def test_the_preparation_count_does_not_depend_on_the_items(devices):
    counts = []
    for name, which in (("mixed", None), ("crowded", None), ("mixed", [4])):
        d = devices(name)
        rendered(d, "batch", which=which)
        items, prepare, tile = d.engine.last_particle_light_batch()
        assert items == (len(d.scene.items) if which is None else len(which)) and tile == 1 and prepare > 0
        counts.append(prepare)
    assert counts[0] == counts[1] == counts[2]


# ---- 2., 3. where the batch is the single call's bits ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [F4, H4, B4])
@pytest.mark.parametrize("item", [2, 4])
def test_a_batch_of_one_item_is_the_single_call(devices, fmt, item):
    d = devices("mixed")
    base = bc.ambient_frame(d.scene, bc.HALF_AMBIENT)
    for rows in ((0, None), (16, 40)):
        got, _ = rendered(d, "batch", fmt, base, [item], rows)
        want, _ = rendered(d, "loop", fmt, base, [item], rows)
        assert np.array_equal(got, want), "item %d, format %d, rows %s" % (item, fmt, rows)
        assert (lb.from_stored(got, fmt) != lb.from_stored(lb.to_stored(base, fmt), fmt)).any()
        if rows[1] is not None:
            stored = lb.to_stored(base, fmt)
            assert np.array_equal(got[:16], stored[:16]) and np.array_equal(got[40:], stored[40:])


@pytest.mark.parametrize("fmt", [F4, H4])
def test_items_that_split_one_system_are_the_single_call_on_it(devices, fmt):
    d = devices("crowded")
    sc = d.scene
    assert sum(sc.emitting(it) for it in sc.items) >= 4097, "item boundaries must fall inside the tile kernel's list batches"
    base = bc.ambient_frame(sc, bc.HALF_AMBIENT)
    got, stats = rendered(d, "batch", fmt, base, want_stats=True)
    lm = d.lightmap(fmt, base)
    st = native.render_particle_lights(d.ctx, d.systems[3], sc.items[0].params, d.env, d.dfu, None, d.sdf, lm, want_stats=True)
    want = lm.download()
    lm.close()
    assert np.array_equal(got, want)
    assert stats == bc.stats_triple(st)


# ---- 4. the blend functions ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("function", [lb.MAX, lb.MIN])
def test_max_and_min_are_the_loop_of_single_calls(devices, ctx, function):
    d = devices("mixed")
    base = scenes.uniform(19, (d.scene.height, d.scene.width, 4), 0.0, 1.25)
    ctx.set_light_blend_function(function, function)
    try:
        got, _ = rendered(d, "batch", base=base)
        want, _ = rendered(d, "loop", base=base)
    finally:
        ctx.set_light_blend_function()
    assert np.array_equal(got, want)
    assert (got != base).any() and (got == base).any()


def test_reverse_subtract_is_base_minus_the_chained_sum(devices, ctx, oracle):
    d = devices("mixed")
    chain, _ = bc.chained_oracle(oracle, d.scene)
    base = bc.ambient_frame(d.scene)
    want = (base - (chain - base)).astype(np.float32)
    ctx.set_light_blend_function(lb.REVERSE_SUBTRACT, lb.REVERSE_SUBTRACT)
    try:
        got, _ = rendered(d, "batch")
    finally:
        ctx.set_light_blend_function()
    assert_close(got, want, "REVERSE_SUBTRACT batch vs base - (chained ADD frame - base)")
    assert (got[..., :3] < 0).any()


# ---- 5., 6. the half formats ------------------------------------------------------------------------------------------------------------

def test_the_fp16_model_is_one_chain_in_item_order(devices, ctx):
    d = devices("mixed")
    base = bc.ambient_frame(d.scene, bc.HALF_AMBIENT)
    ctx.set_lightmap_blend(True)
    try:
        got, _ = rendered(d, "batch", H4, base)
        want, _ = rendered(d, "loop", H4, base)
    finally:
        ctx.set_lightmap_blend(False)
    assert np.array_equal(got, want)
    assert (got.astype(np.float32)[..., 3] > 3.5).any()


def test_half4_under_fp32_accumulation_rounds_once(devices, oracle):
    """The HALF4 batch is half(FLOAT4 batch).  Against the oracle: a value f within the float criterion of `want` and rounded to half
    r times on the way up (the sums only grow: every contribution is >= 0) is within criterion + r * 2^-11 |want| (half an ulp of
    half per rounding, relative to a value that never exceeds the result); r = 1 for the batch, one per item for the loop."""
    d = devices("mixed")
    base = bc.ambient_frame(d.scene, bc.HALF_AMBIENT)
    want, _ = bc.chained_oracle(oracle, d.scene, ambient=bc.HALF_AMBIENT)
    full, _ = rendered(d, "batch", F4, base)
    half_batch, _ = rendered(d, "batch", H4, base)
    half_loop, _ = rendered(d, "loop", H4, base)
    assert np.array_equal(half_batch, full.astype(np.float16))
    assert_close(full, want, "FLOAT4 batch from a half-representable ambient")
    scale = np.abs(want).reshape(-1, 4).max(axis=0)
    for what, got, roundings in (("batch", half_batch, 1), ("loop", half_loop, len(d.scene.items))):
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        bound = (RTOL + roundings * 2.0 ** -11 * (1.0 + RTOL)) * np.abs(want.astype(np.float64)) + ATOL_TIGHT * scale
        print("HALF4 %s: largest error / bound %.3g" % (what, float((err / bound).max())))
        assert (err <= bound).all(), "HALF4 %s: %d texels outside the criterion + %d half roundings" % (what, int((err > bound).sum()), roundings)


# ---- 7. degenerate batches ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [F4, H4])
def test_degenerate_batches_leave_every_bit_alone(devices, fmt):
    d = devices("mixed")
    sc = d.scene
    start = scenes.uniform(9, (sc.height, sc.width, 4), -1.0, 2.0)
    lm = d.lightmap(fmt, start)
    before = lm.download()
    zero_quads = [(d.systems[it.system], it.params, [0] * it.chunk_count, it.chunk_count) for it in sc.items]
    no_chunks = [(d.systems[it.system], it.params, None, 0) for it in sc.items]
    for what, items in (("count 0", []), ("an empty and a dead item", d.items([0, 3])), ("a dead item", d.items([3])),
                        ("quad counts all 0", zero_quads), ("ChunkCount 0", no_chunks)):
        rendered(d, "batch", which=[4])          # so that the diagnostic has something to forget
        assert d.engine.last_particle_light_batch()[2] == 1
        for want_stats in (False, True):
            st = d.engine.render_particle_lights_batch(items, d.env, d.dfu, None, d.sdf, lm, want_stats=want_stats)
            assert d.engine.last_particle_light_batch() == (len(items), 0, 0), what
            if want_stats:
                assert bc.stats_triple(st) == (0, 0, 0), what
        assert lm.download().tobytes() == before.tobytes(), what
    lm.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------

def refused(call, code, *words):
    with pytest.raises(native.IlluminantError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_every_refusal_leaves_the_lightmap_alone(devices, ctx):
    d = devices("mixed")
    sc = d.scene
    lm = d.lightmap()
    before = lm.download()
    good = d.items([1, 2])
    params = sc.items[1].params
    fake = types.SimpleNamespace(handle=abi.Handle(0x123456789), height=sc.height)
    batch = native.Engine.render_particle_lights_batch
    raw = native.lib().ilm_engine_render_particle_lights_batch
    env, dfu = C.cast(C.byref(d.env), C.c_void_p), C.cast(C.byref(d.dfu), C.c_void_p)

    # handles first
    refused(lambda: batch(fake, good, d.env, d.dfu, None, d.sdf, lm), abi.ERR_INVALID_HANDLE, "engine")
    refused(lambda: batch(d.engine, good, d.env, d.dfu, None, d.sdf, fake), abi.ERR_INVALID_HANDLE, "lightmap")
    refused(lambda: batch(d.engine, good, d.env, d.dfu, None, d.sdf, d.systems[1], 0, sc.height), abi.ERR_INVALID_HANDLE, "lightmap")
    # the item array
    one = (abi.ParticleLightItem * 1)()
    assert raw(d.engine.handle, C.cast(one, C.c_void_p), -1, env, dfu, abi.Handle(0), d.sdf.handle, lm.handle, 0, sc.height, None) == abi.ERR_INVALID_ARGUMENT
    assert raw(d.engine.handle, None, 2, env, dfu, abi.Handle(0), d.sdf.handle, lm.handle, 0, sc.height, None) == abi.ERR_INVALID_ARGUMENT
    # what the single call refuses about the frame
    refused(lambda: batch(d.engine, good, None, d.dfu, None, d.sdf, lm), abi.ERR_INVALID_ARGUMENT)
    refused(lambda: batch(d.engine, good, d.env, None, None, d.sdf, lm), abi.ERR_INVALID_ARGUMENT)
    refused(lambda: batch(d.engine, good, d.env, d.dfu, fake, d.sdf, lm), abi.ERR_INVALID_HANDLE, "G-buffer")
    refused(lambda: batch(d.engine, good, d.env, d.dfu, None, fake, lm), abi.ERR_INVALID_HANDLE, "distance field")
    refused(lambda: batch(d.engine, good, d.env, d.dfu, None, d.sdf, lm, 3, sc.height + 1), abi.ERR_OUT_OF_RANGE, "rows")
    refused(lambda: batch(d.engine, good, d.env, d.dfu, None, d.sdf, lm, 9, 8), abi.ERR_OUT_OF_RANGE, "rows")
    refused(lambda: batch(d.engine, good, d.env, d.dfu, None, d.sdf, lm, -1, 8), abi.ERR_OUT_OF_RANGE, "rows")
    other = native.Context(0)
    foreign = native.Lightmap(other, sc.width, sc.height)
    refused(lambda: batch(d.engine, good, d.env, d.dfu, None, d.sdf, foreign), abi.ERR_INVALID_ARGUMENT, "another context")
    foreign.close()
    atlas, _ = bc.field()
    filtered = native.DistanceFieldTexture(ctx, atlas)
    filtered.set_filter(abi.SDF_FILTER_FIXED8)
    refused(lambda: batch(d.engine, good, d.env, d.dfu, None, filtered, lm), abi.ERR_INVALID_ARGUMENT, "ilm_engine_render_particle_lights_batch")
    filtered.close()

    # per item: the item is named
    refused(lambda: batch(d.engine, good + [(fake, params, None, 1)], d.env, d.dfu, None, d.sdf, lm), abi.ERR_INVALID_HANDLE, "item 2:", "system")
    refused(lambda: batch(d.engine, [good[0], (d.engine, params, None, 1)], d.env, d.dfu, None, d.sdf, lm), abi.ERR_INVALID_HANDLE, "item 1:")
    other_engine = native.Engine(ctx, sc.cs, scenes.randomness_table(7))
    stranger = native.System(other_engine)
    stranger.add_chunk()
    refused(lambda: batch(d.engine, good + [(stranger, params)], d.env, d.dfu, None, d.sdf, lm), abi.ERR_INVALID_ARGUMENT, "item 2:", "another engine")
    stranger.close(); other_engine.close()
    stippled = lc.particle_light_params(2.0, 5.0)
    stippled.StippleFactor = 0.5
    refused(lambda: batch(d.engine, [good[0], (d.systems[2], stippled)] + good, d.env, d.dfu, None, d.sdf, lm), abi.ERR_INVALID_ARGUMENT, "item 1:", "StippleReject")
    stippled.StippleFactor = float("nan")
    refused(lambda: batch(d.engine, [(d.systems[2], stippled)], d.env, d.dfu, None, d.sdf, lm), abi.ERR_INVALID_ARGUMENT, "item 0:", "StippleReject")
    for chunk_count in (-1, 4):         # system 2 has three chunks
        refused(lambda: batch(d.engine, good + [(d.systems[2], params, None, chunk_count)], d.env, d.dfu, None, d.sdf, lm), abi.ERR_OUT_OF_RANGE,
                "item 2:", "chunk_count %d" % chunk_count)
    for q in (-1, sc.slots + 1):
        refused(lambda: batch(d.engine, good + [(d.systems[2], params, [sc.slots, q, 5])], d.env, d.dfu, None, d.sdf, lm), abi.ERR_OUT_OF_RANGE,
                "item 2:", "quad_counts[1] = %d" % q)
    assert lm.download().tobytes() == before.tobytes()
    # the engine's diagnostic still describes the latest ACCEPTED batch
    rendered(d, "batch", which=[1, 2])
    refused(lambda: batch(d.engine, good + [(fake, params, None, 1)], d.env, d.dfu, None, d.sdf, lm), abi.ERR_INVALID_HANDLE, "item 2:")
    assert d.engine.last_particle_light_batch()[0::2] == (2, 1)
    lm.close()
    other.close()


def test_more_than_four_million_quads_are_refused_before_anything_is_launched(devices):
    """one item of 4 x 1 600 quads listed 656 times: 4 198 400 > 2^22 = 4 194 304"""
    d = devices("crowded")
    sc = d.scene
    n = (1 << 22) // (4 * sc.slots) + 1
    assert (n - 1) * 4 * sc.slots <= (1 << 22) < n * 4 * sc.slots
    items = (abi.ParticleLightItem * n)()
    for i in range(n):
        items[i].System = d.systems[3].handle.value
        items[i].ChunkCount = 4
        items[i].Params = sc.items[0].params
    lm = d.lightmap()
    before = lm.download()
    rendered(d, "batch", which=[0])
    refused(lambda: d.engine.render_particle_lights_batch(items, d.env, d.dfu, None, d.sdf, lm), abi.ERR_TOO_MANY, "item %d:" % (n - 1), "4198400")
    assert d.engine.last_particle_light_batch()[0::2] == (1, 1), "nothing was accepted, nothing launched"
    assert lm.download().tobytes() == before.tobytes()
    lm.close()


# ---- 9. the scratch grows and is reused ---------------------------------------------------------------------------------------------------

def test_the_scratch_grows_and_is_reused():
    """On ONE context of its own: a small batch (4 entries and 2 parameter blocks: 256 bytes of table, room for 512; 4 workgroup counts,
    room for 8; 388 quads, room for 4 096 records); the crowded batch (6 400 quads > 4 096; 28 counts > 8); the whole mixed batch (11
    entries and 6 parameter blocks: 744 bytes > 512); then the small batch again -- the first result's bits -- and every result against the
    shared context's."""
    c = native.Context(0)
    mixed, crowded = bc.Device(c, bc.mixed_scene()), bc.Device(c, bc.crowded_scene())
    frames = [rendered(mixed, "batch", which=[1, 2], want_stats=True), rendered(crowded, "batch", want_stats=True),
              rendered(mixed, "batch", want_stats=True), rendered(mixed, "batch", which=[1, 2], want_stats=True)]
    assert frames[3][1] == frames[0][1] and frames[3][0].tobytes() == frames[0][0].tobytes()
    mixed.close(); crowded.close(); c.close()
    for k, (dev, which) in enumerate((("mixed", [1, 2]), ("crowded", None), ("mixed", None))):
        fresh = native.Context(0)
        d = bc.Device(fresh, bc.scene(dev))
        want = rendered(d, "batch", which=which, want_stats=True)
        d.close(); fresh.close()
        assert frames[k][1] == want[1] and frames[k][0].tobytes() == want[0].tobytes(), "call %d differs from the same call on a fresh context" % k
