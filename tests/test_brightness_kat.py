"""Brightness estimation without a GPU: known answers of the restatement (tests/brightness_common.py) derived by hand from the reference's
text, the host mirror's Histogram against it, the ABI's three structs against the C header, and the no-device behaviour of both entry points.
"""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from illuminant_amd import abi, native
from tests import brightness_common as bc

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "illuminant_hip.h")


def ulp_up(x):
    return np.nextafter(F(x), F(np.inf))


def ulp_down(x):
    return np.nextafter(F(x), F(-np.inf))


def test_ctor_table_of_histogram_4_2():
    """Histogram(4, 2, bucketCount = 4): log2(5) / 4 * (i + 1) -> 5^(1/4), 5^(1/2), 5^(3/4), 5, each cast to float BEFORE the `- 1`."""
    t = bc.bucket_table(4.0, 2.0, 4)
    l5 = math.log(5.0) / math.log(2.0)
    want = [F(2.0 ** (l5 / 4 * (i + 1))) - F(1) for i in range(4)]
    assert t.dtype == np.float32 and [x.tobytes() for x in t] == [F(x).tobytes() for x in want]
    # the last entry is float32(5.0...) - 1 -- pow lands within an ulp of 5, the cast may or may not hide it, the subtraction comes after
    assert t[3] == F(2.0 ** l5) - F(1) and abs(float(t[3]) - 4.0) < 1e-6
    assert abs(float(t[0]) - (5 ** 0.25 - 1)) < 1e-7 and abs(float(t[1]) - (5 ** 0.5 - 1)) < 1e-7
    assert np.all(np.diff(t) > 0)
    # the default 64 buckets of the reference's scenes
    t64 = bc.bucket_table(8.0, 2.0)
    assert len(t64) == 64 and np.all(np.diff(t64) > 0) and abs(float(t64[-1]) - 8.0) < 1e-5


@pytest.mark.parametrize("count", [2, 4, 64])
def test_pick_bucket_at_every_entry(count):
    t = bc.bucket_table(4.0, 2.0, count)
    for i in range(count):
        # entries <= value, except: below the first maximum -> 0, at or above entry count - 2 -> the last bucket
        at = count - 1 if i >= count - 2 else i + 1
        below = 0 if i == 0 else (count - 1 if i == count - 1 else i)
        assert bc.pick_bucket(t, t[i]) == at, i
        assert bc.pick_bucket(t, ulp_up(t[i])) == at, i
        assert bc.pick_bucket(t, ulp_down(t[i])) == below, i
    assert bc.pick_bucket(t, F(0)) == 0 and bc.pick_bucket(t, F(-0.0)) == 0 and bc.pick_bucket(t, F(-3.5)) == 0
    assert bc.pick_bucket(t, F(-np.inf)) == 0 and bc.pick_bucket(t, F(np.inf)) == count - 1
    assert bc.pick_bucket(t, F(np.nan)) == 0            # every comparison is false: the search ends at 0


def test_get_percentile():
    t = bc.bucket_table(4.0, 2.0, 4)
    r = bc.histogram_add_scalar(np.array([0.1, 0.2, 0.6, 0.7, 0.8, 3.0, 3.5, 9.0], np.float32), t, 1.0, False)
    assert list(r.count) == [2, 3, 0, 3] and r.sample_count == 8
    assert r.get_percentile(0) == (True, 0, F(0))
    ok, bucket, value = r.get_percentile(50)            # sample 4: the third of bucket 1's three
    assert ok and bucket == 1 and value == F(t[0] + ((t[1] - t[0]) * (F(2) / F(3))))
    ok, bucket, value = r.get_percentile(99.9)          # sample 7: the third of bucket 3's three
    assert ok and bucket == 3 and value == F(t[2] + ((t[3] - t[2]) * (F(2) / F(3))))
    with pytest.raises(RuntimeError):                   # 100 % names sample 8 of 8: the reference throws (Histogram.cs:162)
        r.get_percentile(100)
    assert r.get_percentile(-1) == (False, 0, F(0)) and r.get_percentile(100.5) == (False, 0, F(0))
    empty = bc.histogram_add_scalar(np.zeros(4, np.float32), t, 1.0, True)
    assert empty.sample_count == 0 and empty.get_percentile(50) == (False, 0, F(0))
    assert empty.total_min == 0 and empty.total_max == 0 and empty.mean == 0
    # Buckets: Min is 0 for an empty bucket, Max is the state's, Mean = Sum / Count
    b = r.buckets()
    assert b[2] == (t[1], t[2], F(0), F(0), F(0), 0)
    assert b[0][:2] == (F(0), t[0]) and b[0][2] == F(0.1) and b[0][3] == F(0.2) and b[0][4] == F(F(F(0.1) + F(0.2)) / F(2))


def test_median_index():
    s = bc.sort_values
    assert bc.median_index(s([5.0]), False) == 0 and bc.median_index(s([5.0, 6.0]), False) == 1        # count / 2
    assert bc.median_index(s([1.0, 2.0, 3.0, 4.0]), False) == 2 and bc.median_index(s([1.0, 2.0, 3.0]), False) == 1
    # IgnoreZeroes without a zero: Array.LastIndexOf gives -1 and the reference uses it: (count + 1) / 2 - 1
    assert bc.median_index(s([5.0]), True) == 0 and bc.median_index(s([5.0, 6.0]), True) == 0
    assert bc.median_index(s([1.0, 2.0, 3.0, 4.0]), True) == 1 and bc.median_index(s([1.0, 2.0, 3.0]), True) == 1
    # with zeros: the offset is the index of the last one in sort order -- NaNs and negatives come first, -0 is a zero
    v = s([0.0, 3.0, np.nan, -1.0, -0.0, 2.0, 7.0, 0.0])
    assert np.isnan(v[0]) and v[1] == -1 and np.signbit(v[2]) and not np.signbit(v[3]) and list(v[5:]) == [2.0, 3.0, 7.0]
    assert bc.median_index(v, True) == (8 - 4) // 2 + 4 == 6
    assert bc.median_index(s([0.0, 0.0]), True) == 1 and bc.median_index(s([0.0]), True) == 0
    r = bc.histogram_add_scalar(v, bc.bucket_table(4.0, 2.0, 4), 0.5, True)
    assert r.median == F(1.5) and r.sample_count == 4 and np.isnan(r.total_min) and np.isnan(r.total_max) and np.isnan(r.total_sum)


def test_vectorised_restatement_equals_the_scalar_one():
    rng = np.random.RandomState(5)
    v = rng.exponential(0.8, 3000).astype(np.float32)
    v[rng.randint(0, 3000, 200)] = 0.0
    v[7], v[8], v[9], v[10] = -0.0, -2.5, np.inf, 1e-30
    for special in (False, True):
        if special:
            v[11] = np.nan
        for count in (2, 64, 256):
            t = bc.bucket_table(6.0, 2.0, count)
            for ignore in (False, True):
                a, b = bc.histogram_add_scalar(v, t, 0.5, ignore), bc.histogram_add(v, t, 0.5, ignore)
                assert np.array_equal(a.count, b.count)
                for x, y in ((a.min, b.min), (a.max, b.max), (a.sum, b.sum)):
                    assert x.tobytes() == y.tobytes() or (np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~np.isnan(x)], y[~np.isnan(y)]))
                for name in ("sample_count", "total_min", "total_max", "mean", "median", "total_sum"):
                    x, y = getattr(a, name), getattr(b, name)
                    assert (np.isnan(x) and np.isnan(y)) or F(x).tobytes() == F(y).tobytes(), name


@pytest.mark.parametrize("r", [2, 3, 22, 23, 38, 41, 264, 4095])
def test_point_sample_map(r):
    """Pixel centre (i + 1/2) / n0 of the half-size target times r source texels, floored: exact in Fractions; 2i + 1 for even sizes."""
    n0 = r // 2
    for i in range(n0):
        want = min(r - 1, math.floor(Fraction(2 * i + 1, 2 * n0) * r))
        assert bc.source_index(i, r, n0) == want
        if r % 2 == 0:
            assert want == 2 * i + 1
    assert bc.source_index(n0 - 1, r, n0) <= r - 1


def test_luminance_and_levels_by_hand():
    texels = np.zeros((4, 8, 4), np.float32)
    texels[..., 2] = 1.0
    level, a = bc.luminance_level(texels, bc.FORMAT_FLOAT4, 8, 4, 0)
    assert level == 0 and a.shape == (2, 4) and np.all(a == F(0.144))        # Resolve.fx:15: 0.144, not HDR.fxh's 0.114
    texels = np.arange(4 * 8 * 4, dtype=np.float32).reshape(4, 8, 4)
    _, a = bc.luminance_level(texels, bc.FORMAT_FLOAT4, 8, 4, 0)
    t = texels[3, 5]                                                          # level-0 texel (2, 1) is source texel (5, 3)
    assert a[1, 2] == F(F(t[0] * F(0.299)) + F(t[1] * F(0.587))) + F(t[2] * F(0.144))
    level, b = bc.luminance_level(texels, bc.FORMAT_FLOAT4, 8, 4, 5)          # LevelCount = floor(log2(4)) + 1 = 3; level 2 of 4 x 2 is empty
    assert level == 2 and b is None
    level, b = bc.luminance_level(texels, bc.FORMAT_FLOAT4, 8, 4, 1)
    assert level == 1 and b.shape == (1, 2) and b[0, 1] == F(F(F(a[0, 2] + a[0, 3]) + F(a[1, 2] + a[1, 3])) * F(0.25))
    # Color decodes as byte / 255 in IEEE single, all 256 values
    bytes_ = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(4, axis=2)
    dec = bc.decode_texels(bytes_, bc.FORMAT_RGBA8)
    assert all(dec[0, i, 0] == F(F(i) / F(255.0)) for i in range(256))
    assert bc.level_index(40, 24, 9) == 4 and bc.level_index(24, 24, 9) == 3 and bc.level_index(3840, 2160, 3) == 3


def test_host_mirror_histogram_matches_the_restatement():
    from illuminant_amd import _host as H
    for max_value, power, count in ((4.0, 2.0, 4), (8.0, 2.0, 64), (16.0, 3.0, 256), (1.5, 10.0, 2)):
        h = H.Histogram(max_value, power, count, True)
        assert h.BucketCount == count and h.MaxInputValue == F(max_value) and h.IgnoreZeroes
        assert np.asarray(h.BucketMaxValues, np.float32).tobytes() == bc.bucket_table(max_value, power, count).tobytes()
        assert h.SampleCount == 0 and h.GetPercentile(50) == (False, 0, 0.0)
        states = np.frombuffer(h.States, dtype=[("Count", "<i4"), ("Min", "<f4"), ("Max", "<f4"), ("Sum", "<f4")])
        assert len(states) == count and np.all(states["Min"] == bc.FLOAT_MAX) and not states["Count"].any() and not states["Max"].any()
        assert all(b[2:] == (0.0, 0.0, 0.0, 0) for b in h.Buckets)
    assert H.Histogram(1.0, 2.0).BucketCount == 64 and not H.Histogram(1.0, 2.0).IgnoreZeroes
    with pytest.raises(Exception):
        H.Histogram(1.0, 2.0, 1)


def test_struct_layouts_match_the_c_header(tmp_path):
    structs = {"IlmHistogramBucket": abi.HistogramBucket, "IlmHistogramParams": abi.HistogramParams, "IlmHistogramResult": abi.HistogramResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void) {"]
    for cname, mirror in structs.items():
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in mirror._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.splitlines():
        cname, what, value = line.split()
        if what == "sizeof":
            assert C.sizeof(structs[cname]) == int(value) == abi.EXPECTED_SIZES[cname][1], cname
        else:
            assert getattr(structs[cname], what).offset == int(value), (cname, what)
        seen += 1
    assert seen == 3 + 4 + 6 + 9


def test_entry_points_refuse_bad_handles_without_a_device():
    lib = native.lib()
    level, w, h = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    values = (C.c_float * 4)(9, 9, 9, 9)
    for handle in (0, 12345):
        assert lib.ilm_lightmap_luminance(abi.Handle(handle), 8, 8, 0, values, 4, C.byref(level), C.byref(w), C.byref(h)) == abi.ERR_INVALID_HANDLE
        assert b"lightmap" in lib.ilm_last_error()
        assert (level.value, w.value, h.value) == (-7, -7, -7) and list(values) == [9, 9, 9, 9]
        params = abi.HistogramParams(8, 8, 0, 4, 0, 1.0)
        table = (C.c_float * 4)(1, 2, 3, 4)
        buckets = (abi.HistogramBucket * 4)()
        result = abi.HistogramResult(SampleCount=-7)
        rc = lib.ilm_lightmap_histogram(abi.Handle(handle), C.cast(C.byref(params), C.c_void_p), C.cast(table, C.c_void_p),
                                        C.cast(buckets, C.c_void_p), C.cast(C.byref(result), C.c_void_p))
        assert rc == abi.ERR_INVALID_HANDLE and b"lightmap" in lib.ilm_last_error()
        assert result.SampleCount == -7 and not any(b.Count for b in buckets)
    # the handle comes first: NULL arguments behind a bad handle are still a handle error
    assert lib.ilm_lightmap_histogram(abi.Handle(0), None, None, None, None) == abi.ERR_INVALID_HANDLE
