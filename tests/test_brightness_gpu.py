"""Brightness estimation on the device (ilm_lightmap_luminance, ilm_lightmap_histogram) against the float32 restatement of the reference's
CalculateLuminance + Histogram.Add (tests/brightness_common.py).  The luminance level, counts, minima, maxima and the median are integers
and selected values: bit-equal.  Sums and means meet the suite's float criterion (tests/util.py) against the restatement's sequential
float32 sum; for every input used here that sum is itself within 1e-5 of a float64 sum (asserted), so the criterion prices the device.

Shapes: 40 x 24 with a 38 x 22 render size (smaller than the lightmap; level 0 is 19 x 11, so every level drops a row or a column),
41 x 23 (the odd-size point-sample map), 272 x 144 with 264 x 136 (level-0 columns 128..131 lie past the last whole group of four 8 x 8
blocks), 512 x 256 at level 0 (32 768 values: 32 workgroups of the statistics, every pass of the select), 24 x 24 (AccuracyFactor
clamped onto a level that has a texel), 2944 x 1472 at level 0 (the one size at which a statistics workgroup takes more than one chunk).
"""
import ctypes as C

import numpy as np
import pytest

from illuminant_amd import abi, native, scenes
from tests import brightness_common as bc
from tests.util import assert_bits_equal, assert_close

pytestmark = pytest.mark.gpu

F = np.float32
FORMATS = {"float4": abi.LIGHTMAP_FLOAT4, "half4": abi.LIGHTMAP_HALF4, "rgba8": abi.LIGHTMAP_RGBA8}
_frames = {}        # (kind, width, height, format) -> (Lightmap, texels as downloaded)
_levels = {}        # (frame key, render size, accuracy) -> (level index, level or None)


def frame(ctx, kind, width, height, fmt):
    """A lightmap and the texels it holds (read back: the reference works on what the device stores)."""
    key = (kind, width, height, fmt)
    if key in _frames:
        return key, _frames[key][0], _frames[key][1]
    lm = native.Lightmap(ctx, width, height, FORMATS[fmt])
    if kind == "lit":
        lights = scenes.random_lights(width * 100 + height, 7, width, height, z=(6.0, 40.0), radius=max(width, height) / 12.0,
                                      ramp=(max(width, height) / 6.0, max(width, height) / 2.0))
        lights = (abi.LightVertex * len(lights))(*lights)
        dfu = scenes.DistanceFieldLayout(64, 64, 32.0, 3, 1.0, 64).uniforms()
        native.render_sphere_lights(ctx, lights, scenes.environment(), dfu, None, None, (0.03, 0.05, 0.04, 1.0), lm)
    else:
        dt = {"float4": np.float32, "half4": np.float16, "rgba8": np.uint8}[fmt]
        one = 255 if fmt == "rgba8" else 1.0
        t = np.zeros((height, width, 4), dt)
        if kind == "constant":
            t[...] = (np.array([0.25, 0.5, 0.75, 1.0]) * one).astype(dt)
        elif kind == "blue":
            t[..., 2] = one
        elif kind == "bytes":           # every byte value in every channel
            t[...] = (np.arange(height * width * 4, dtype=np.int64) * 7 % 256).reshape(height, width, 4).astype(dt)
        elif kind == "signed":          # mostly light, a few negative texels and zeros of both signs: finite sums
            rng = np.random.RandomState(11)
            t[..., :3] = rng.uniform(0.0, 3.0, (height, width, 3)).astype(dt)
            t[rng.rand(height, width) < 0.05, :3] = dt(-0.004)
            t[rng.rand(height, width) < 0.10, :3] = dt(0.0)
            t[rng.rand(height, width) < 0.03, :3] = dt(-0.0)
        elif kind == "specials":        # the same with a NaN and an Inf among the texels that are sampled
            rng = np.random.RandomState(12)
            t[..., :3] = rng.uniform(0.0, 3.0, (height, width, 3)).astype(dt)
            t[rng.rand(height, width) < 0.05, :3] = dt(-1.5)
            t[rng.rand(height, width) < 0.10, :3] = dt(0.0)
            t[rng.rand(height, width) < 0.03, :3] = dt(-0.0)
            t[5, 7, 0] = np.nan
            t[9, 3, 1] = np.inf
        elif kind == "sparse":          # black with a lattice of blue texels among those that are sampled: sums of a few equal terms
            t[1::74, 1::82, 2] = one
        elif kind != "zero":
            raise KeyError(kind)
        lm.upload(t)
    texels = lm.download()
    _frames[key] = (lm, texels)
    return key, lm, texels


def reference_level(key, texels, fmt, render, accuracy):
    k = (key, render, accuracy)
    if k not in _levels:
        _levels[k] = bc.luminance_level(texels, {"float4": bc.FORMAT_FLOAT4, "half4": bc.FORMAT_HALF4, "rgba8": bc.FORMAT_RGBA8}[fmt],
                                        render[0], render[1], accuracy)
    return _levels[k]


LEVEL_CASES = [(40, 24, (38, 22), fmt, kind, level) for fmt in ("float4", "half4", "rgba8") for kind, level in (("lit", 0), ("lit", 1), ("lit", 3), ("bytes", 1))]
LEVEL_CASES += [(41, 23, (41, 23), "float4", "lit", 0), (41, 23, (41, 23), "half4", "lit", 1), (41, 23, (41, 23), "rgba8", "bytes", 0),
                (41, 23, (39, 21), "float4", "lit", 0),
                (272, 144, (264, 136), "half4", "lit", 3), (272, 144, (264, 136), "float4", "lit", 5), (272, 144, (264, 136), "rgba8", "lit", 4),
                (512, 256, (512, 256), "half4", "lit", 0), (512, 256, (512, 256), "float4", "lit", 7),
                (24, 24, (24, 24), "float4", "lit", 9),
                (40, 24, (38, 22), "float4", "blue", 0), (40, 24, (38, 22), "rgba8", "blue", 1), (40, 24, (38, 22), "half4", "constant", 1),
                (40, 24, (38, 22), "float4", "specials", 0), (40, 24, (38, 22), "float4", "specials", 1), (40, 24, (38, 22), "half4", "zero", 0)]


@pytest.mark.parametrize("width,height,render,fmt,kind,accuracy", LEVEL_CASES)
def test_luminance_level_is_bit_equal(ctx, width, height, render, fmt, kind, accuracy):
    key, lm, texels = frame(ctx, kind, width, height, fmt)
    level, want = reference_level(key, texels, fmt, render, accuracy)
    assert want is not None
    got_level, got = lm.luminance(accuracy, render)
    assert got_level == level == min(accuracy, bc.level_index(width, height, 99))
    assert_bits_equal(got, want, "luminance level %d of %s %s %dx%d" % (level, kind, fmt, width, height))
    if kind == "blue":
        assert np.all(got == F(0.144))            # (exact at every level: four equal texels average to themselves)
    if accuracy == 9:
        assert got.shape == (1, 1)          # 24 x 24: LevelCount = floor(log2(12)) + 1 = 4, so 9 clamps to level 3 of 12 x 12


def test_every_byte_value_decodes_as_an_ieee_division(ctx):
    """A Color lightmap whose sampled texel x carries byte x in one channel: level 0 is float(x) / 255.0f times that channel's weight."""
    lm = native.Lightmap(ctx, 512, 2, abi.LIGHTMAP_RGBA8)
    for channel, weight in enumerate((0.299, 0.587, 0.144)):
        t = np.zeros((2, 512, 4), np.uint8)
        t[1, 1::2, channel] = np.arange(256)
        lm.upload(t)
        level, got = lm.luminance(0)
        assert level == 0 and got.shape == (1, 256)
        want = np.array([F(F(x) / F(255.0)) * F(weight) for x in range(256)], np.float32)
        assert_bits_equal(got[0], want, "byte / 255 in channel %d" % channel)
        assert_bits_equal(got, bc.luminance_level(t, bc.FORMAT_RGBA8, 512, 2, 0)[1], "the restatement agrees")
    lm.close()


@pytest.mark.parametrize("fmt", ["float4", "half4", "rgba8"])
def test_accuracy_factor_clamps_and_an_empty_level_is_out_of_range(ctx, fmt):
    """40 x 24: LevelCount = floor(log2(20)) + 1 = 5, so AccuracyFactor 9 means level 4 -- which for the 19 x 11 level 0 is 1 x 0 texels."""
    key, lm, texels = frame(ctx, "lit", 40, 24, fmt)
    level, want = reference_level(key, texels, fmt, (38, 22), 9)
    assert level == 4 and want is None
    lvl, w, h = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    rc = native.lib().ilm_lightmap_luminance(lm.handle, 38, 22, 9, None, 0, C.byref(lvl), C.byref(w), C.byref(h))
    assert rc == abi.ERR_OUT_OF_RANGE and b"level 4" in native.lib().ilm_last_error()
    assert (lvl.value, w.value, h.value) == (-7, -7, -7)
    with pytest.raises(native.IlluminantError) as e:
        lm.histogram(bc.bucket_table(4.0, 2.0, 4), 9, render_size=(38, 22))
    assert e.value.code == abi.ERR_OUT_OF_RANGE
    # the size query alone
    rc = native.lib().ilm_lightmap_luminance(lm.handle, 38, 22, 3, None, 0, C.byref(lvl), C.byref(w), C.byref(h))
    assert rc == 0 and (lvl.value, w.value, h.value) == (3, 2, 1)


def same_or_both_nan(got, want, what):
    assert_bits_equal(np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1), what)


def sums_close(got, want, what):
    """The suite's float criterion where the reference's sum is finite; the same non-finite class elsewhere."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    finite = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    odd = ~finite & ~np.isnan(want)
    assert np.array_equal(got[odd], want[odd]), what
    if finite.any():
        assert_close(got[finite], want[finite], what)


def sequential_sum_is_sound(level, table, scale, ignore, want):
    """On this input the restatement's sequential float32 sums agree with float64 sums to 1e-5: the 1e-4 criterion tests the device."""
    buf = bc.sort_values(level)
    kept = buf[~(buf <= 0)] if ignore else buf
    with np.errstate(all="ignore"):
        v = (kept * F(scale)).astype(np.float32)
        exact = float(np.sum(v.astype(np.float64)))
        if np.isfinite(exact) and np.isfinite(want.total_sum):
            assert abs(float(want.total_sum) - exact) <= 1e-5 * abs(exact), (float(want.total_sum), exact)
        b = np.array([bc.pick_bucket(table, x) for x in v]) if v.size <= 4096 else None
        if b is not None:
            for j in range(len(table)):
                e = float(np.sum(v[b == j].astype(np.float64)))
                if np.isfinite(e) and np.isfinite(want.sum[j]):
                    assert abs(float(want.sum[j]) - e) <= 1e-5 * abs(e) + 1e-30, (j, float(want.sum[j]), e)


STAT_CASES = [
    # width, height, render, format, contents, accuracy, buckets, scale, ignore zeroes
    (40, 24, (38, 22), "half4", "lit", 0, 64, 1.0, False), (40, 24, (38, 22), "half4", "lit", 0, 64, 0.5, True),
    (40, 24, (38, 22), "float4", "lit", 1, 2, 0.5, False), (40, 24, (38, 22), "rgba8", "lit", 0, 256, 1.0, True),
    (40, 24, (38, 22), "rgba8", "bytes", 0, 64, 1.0, False), (40, 24, (38, 22), "float4", "lit", 3, 64, 1.0, False),
    (41, 23, (41, 23), "float4", "lit", 0, 64, 1.0, False),
    (272, 144, (264, 136), "half4", "lit", 3, 64, 1.0, False), (272, 144, (264, 136), "half4", "lit", 3, 2, 0.5, True),
    (512, 256, (512, 256), "float4", "lit", 0, 64, 1.0, False), (512, 256, (512, 256), "float4", "lit", 0, 256, 0.5, True),
    (512, 256, (512, 256), "float4", "lit", 0, 2, 1.0, False), (512, 256, (512, 256), "half4", "signed", 0, 64, 0.5, False),
    (512, 256, (512, 256), "half4", "signed", 0, 256, 1.0, True),
    (40, 24, (38, 22), "float4", "zero", 0, 64, 1.0, False), (40, 24, (38, 22), "float4", "zero", 0, 64, 1.0, True),
    (40, 24, (38, 22), "half4", "constant", 0, 64, 0.5, False), (40, 24, (38, 22), "float4", "blue", 0, 64, 1.0, True),
    (40, 24, (38, 22), "float4", "signed", 0, 64, 1.0, False), (40, 24, (38, 22), "float4", "signed", 0, 64, 0.5, True),
    (40, 24, (38, 22), "float4", "specials", 0, 64, 1.0, False), (40, 24, (38, 22), "float4", "specials", 0, 2, 0.5, True),
    (40, 24, (38, 22), "float4", "specials", 1, 256, 1.0, False),
    (24, 24, (24, 24), "float4", "lit", 9, 64, 1.0, True),
    # 1 083 392 values: more chunks than the statistics launch has workgroups, so every workgroup walks on to a second chunk
    (2944, 1472, (2944, 1472), "half4", "sparse", 0, 64, 1.0, False), (2944, 1472, (2944, 1472), "half4", "sparse", 0, 64, 0.5, True),
]


@pytest.mark.parametrize("width,height,render,fmt,kind,accuracy,count,scale,ignore", STAT_CASES)
def test_statistics_match_the_restatement(ctx, width, height, render, fmt, kind, accuracy, count, scale, ignore):
    key, lm, texels = frame(ctx, kind, width, height, fmt)
    level, values = reference_level(key, texels, fmt, render, accuracy)
    table = bc.bucket_table(4.0, 2.0, count)
    want = bc.histogram_add(values, table, scale, ignore)
    sequential_sum_is_sound(values, table, scale, ignore, want)
    got, buckets = lm.histogram(table, accuracy, scale, ignore, render)
    again, buckets_again = lm.histogram(table, accuracy, scale, ignore, render)
    assert bytes(got) == bytes(again) and bytes(buckets) == bytes(buckets_again), "the same call twice returns other bits"
    what = "%s %s %dx%d level %d, %d buckets" % (kind, fmt, width, height, level, count)
    assert (got.LevelIndex, got.Width, got.Height) == (level, values.shape[1], values.shape[0])
    b = np.frombuffer(bytes(buckets), dtype=[("Count", "<i4"), ("Min", "<f4"), ("Max", "<f4"), ("Sum", "<f4")])
    assert len(b) == count
    assert np.array_equal(b["Count"], want.count), (what, b["Count"], want.count)
    assert got.SampleCount == want.sample_count == int(want.count.sum())
    same_or_both_nan(b["Min"], want.min, what + " bucket Min")
    same_or_both_nan(b["Max"], want.max, what + " bucket Max")
    same_or_both_nan([got.Min, got.Max, got.Median], [want.total_min, want.total_max, want.median], what + " Min / Max / Median")
    sums_close(b["Sum"], want.sum, what + " bucket Sum")
    sums_close([got.Sum], [want.total_sum], what + " Sum")
    sums_close([got.Mean], [want.mean], what + " Mean")
    with np.errstate(all="ignore"):
        means = np.where(b["Count"] > 0, b["Sum"] / np.maximum(b["Count"], 1).astype(np.float32), F(0)).astype(np.float32)
    sums_close(means, [x[4] for x in want.buckets()], what + " bucket Mean")
    if kind == "blue" and fmt == "float4":
        assert got.Min == got.Max == got.Median == F(0.144)
    if kind == "zero":
        assert got.SampleCount == (0 if ignore else values.size) and got.Median == 0 and got.Min == 0 and got.Max == 0
    if kind == "specials" and accuracy == 0:
        assert np.isnan(got.Min) and np.isnan(got.Max) and np.isnan(b["Min"][0]) and b["Count"][-1] >= 1


def test_refusals_leave_the_outputs_untouched(ctx):
    _, lm, _ = frame(ctx, "lit", 40, 24, "float4")
    lib = native.lib()
    good = bc.bucket_table(4.0, 2.0, 4)

    def call(rw, rh, accuracy, count, table):
        params = abi.HistogramParams(rw, rh, accuracy, count, 0, 1.0)
        t = np.ascontiguousarray(table, np.float32)
        buckets = (abi.HistogramBucket * 300)()
        C.memset(buckets, 0x5A, C.sizeof(buckets))
        result = abi.HistogramResult()
        C.memset(C.byref(result), 0x5A, C.sizeof(result))
        rc = lib.ilm_lightmap_histogram(lm.handle, C.cast(C.byref(params), C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                        C.cast(buckets, C.c_void_p), C.cast(C.byref(result), C.c_void_p))
        untouched = bytes(buckets) == b"\x5A" * C.sizeof(buckets) and bytes(result) == b"\x5A" * C.sizeof(result)
        return rc, untouched, lib.ilm_last_error()

    big = np.arange(1, 301, dtype=np.float32)
    for args, word in (((38, 22, 0, 1, big), b"BucketCount"), ((38, 22, 0, 257, big), b"BucketCount"), ((38, 22, 0, 0, big), b"BucketCount"),
                       ((1, 22, 0, 4, good), b"render size"), ((38, 1, 0, 4, good), b"render size"), ((41, 22, 0, 4, good), b"render size"),
                       ((38, 25, 0, 4, good), b"render size"), ((38, 22, -1, 4, good), b"accuracy"),
                       ((38, 22, 0, 4, [0.5, np.nan, 2.0, 3.0]), b"NaN"), ((38, 22, 0, 4, [0.5, 1.0, 1.0, 3.0]), b"predecessor"),
                       ((38, 22, 0, 4, [0.5, 1.0, 0.75, 3.0]), b"predecessor"), ((38, 22, 0, 2, [1.0, 0.5]), b"predecessor")):
        rc, untouched, message = call(*args)
        assert rc == abi.ERR_INVALID_ARGUMENT and untouched and word in message, (args[:4], rc, message)
    rc, untouched, _ = call(38, 22, 9, 4, good)
    assert rc == abi.ERR_OUT_OF_RANGE and untouched
    rc, untouched, _ = call(38, 22, 0, 4, good)
    assert rc == 0 and not untouched
    # ilm_lightmap_luminance: the same render-size rules, and a capacity below the level's size
    values = np.full(8, -7.0, np.float32)
    lvl, w, h = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    for rw, rh, accuracy, capacity in ((1, 22, 0, 8), (41, 22, 0, 8), (38, 22, -1, 8), (38, 22, 0, 8), (38, 22, 3, 1)):
        rc = lib.ilm_lightmap_luminance(lm.handle, rw, rh, accuracy, values.ctypes.data_as(C.c_void_p), capacity, C.byref(lvl), C.byref(w), C.byref(h))
        assert rc == abi.ERR_INVALID_ARGUMENT and np.all(values == -7.0) and (lvl.value, w.value, h.value) == (-7, -7, -7)


def test_host_mirror_try_compute_histogram(ctx):
    """TryComputeHistogram after RenderLighting(intensityScale = 2) is the direct ABI call with ScaleFactor = 0.5; false without the flag."""
    from illuminant_amd import _host as H
    hctx = H.DeviceContext(0)
    w, h = 160, 96
    env = H.LightingEnvironment()
    env.Ambient = [0.05, 0.04, 0.03, 1.0]
    lv = scenes.random_lights(21, 9, w, h, z=(8.0, 40.0), radius=8.0, ramp=(40.0, 90.0))
    lights = []
    for i in range(len(lv)):
        l = H.SphereLightSource()
        l.Position = [lv[i].LightPosition1.x, lv[i].LightPosition1.y, lv[i].LightPosition1.z]
        l.Radius = lv[i].LightProperties.x; l.RampLength = lv[i].LightProperties.y
        l.Color = [lv[i].Color1.x, lv[i].Color1.y, lv[i].Color1.z, 1.0]
        lights.append(l)
    env.Lights = lights
    rc = H.RendererConfiguration(w, h)
    assert rc.EnableBrightnessEstimation is False
    off = H.LightingRenderer(hctx, rc, env)
    hist = H.Histogram(4.0, 2.0, 64, True)
    off.RenderLighting(2.0, 0, -1, False)
    assert off.TryComputeHistogram(hist) is False and hist.SampleCount == 0
    rc.EnableBrightnessEstimation = True
    r = H.LightingRenderer(hctx, rc, env)
    assert r.TryComputeHistogram(hist) is False            # no frame yet: LuminanceBuffer == null
    r.RenderLighting(2.0, 0, -1, False)
    for accuracy in (3, 1):
        assert (r.TryComputeHistogram(hist) if accuracy == 3 else r.TryComputeHistogram(hist, accuracy)) is True
        direct = native.Lightmap(None, w, h, r.LightmapFormat, borrowed_handle=r.LightmapHandle)
        table = bc.bucket_table(4.0, 2.0, 64)
        assert np.asarray(hist.BucketMaxValues, np.float32).tobytes() == table.tobytes()
        got, buckets = direct.histogram(table, accuracy, 0.5, True)
        assert hist.States == bytes(buckets) and hist.SampleCount == got.SampleCount > 0
        same_or_both_nan([hist.Min, hist.Max, hist.Mean, hist.Median], [got.Min, got.Max, got.Mean, got.Median], "host mirror totals")
        # GetPercentile and Buckets on the device's states are the restatement's on the same counts
        level, values = bc.luminance_level(direct.download(), bc.FORMAT_HALF4 if r.LightmapFormat == abi.LIGHTMAP_HALF4 else bc.FORMAT_FLOAT4, w, h, accuracy)
        want = bc.histogram_add(values, table, 0.5, True)
        assert got.LevelIndex == level == accuracy and np.array_equal([b.Count for b in buckets], want.count)
        for percent in (0.0, 50.0, 90.0):
            ok, bucket, value = hist.GetPercentile(percent)
            wok, wbucket, wvalue = want.get_percentile(percent)
            assert (ok, bucket) == (wok, wbucket) and F(value) == wvalue
        for mine, theirs in zip(hist.Buckets, want.buckets()):
            assert mine[5] == theirs[5] and F(mine[0]) == theirs[0] and F(mine[1]) == theirs[1] and F(mine[2]) == theirs[2] and F(mine[3]) == theirs[3]
