"""Brightness estimation restated in float32 numpy from the reference's text: technique CalculateLuminance, the level chain and
Histogram.Add / GetPercentile / Buckets.  Test infrastructure: imports nothing from the product or the oracle; every operation rounds to
float32 (np.float32 scalars, or numpy's sequential float32 accumulate where the loop is vectorised -- test_brightness_kat.py holds the
two forms together).

Decisions that are this project's and not the reference's: the rational point-sample map for odd sizes, the
2 x 2 box in the order ((a + b) + (c + d)) * 0.25f for the level chain, and the order of equal zeros: -0 sorts before +0, Math.Min of a
(-0, +0) pair is -0 and Math.Max is +0 (the reference's unstable sort and the runtimes' Math.Min leave these open).
"""
import math

import numpy as np

F = np.float32
FLOAT_MAX = F(3.4028234663852886e38)
FORMAT_FLOAT4, FORMAT_HALF4, FORMAT_RGBA8 = 0, 1, 2


# ---- the luminance target ---------------------------------------------------------------------------------------------------------
def decode_texels(texels, fmt):
    """What the sampler returns: float4 as stored, HalfVector4 widened exactly, Color as byte / 255 (IEEE single division)."""
    if fmt == FORMAT_RGBA8:
        return np.asarray(texels, np.uint8).astype(np.float32) / F(255.0)
    return np.asarray(texels).astype(np.float32)


def source_index(i, r, n0):
    """Destination pixel centre i of n0 through the draw of LightingRenderer.cs:888-893 onto r source texels, POINT sampled, in integers."""
    return min(r - 1, ((2 * i + 1) * r) // (2 * n0))


def luminance_level0(rgb, rw, rh):
    """CalculateLuminancePixelShader, Resolve.fx:15,212-227: dot(rgb, float3(0.299, 0.587, 0.144)) as (r * .299 + g * .587) + b * .144."""
    w0, h0 = rw // 2, rh // 2
    xs = np.array([source_index(x, rw, w0) for x in range(w0)], np.int64)
    ys = np.array([source_index(y, rh, h0) for y in range(h0)], np.int64)
    t = np.asarray(rgb, np.float32)[ys][:, xs]
    with np.errstate(all="ignore"):
        return ((t[..., 0] * F(0.299) + t[..., 1] * F(0.587)) + t[..., 2] * F(0.144)).astype(np.float32)


def next_level(a):
    """Level k from level k - 1: ((a + b) + (c + d)) * 0.25f over (2x, 2y) (2x+1, 2y) (2x, 2y+1) (2x+1, 2y+1); odd last row / column dropped."""
    h, w = a.shape[0] // 2, a.shape[1] // 2
    a = np.asarray(a, np.float32)
    with np.errstate(all="ignore"):
        top = a[0:2 * h:2, 0:2 * w:2] + a[0:2 * h:2, 1:2 * w:2]
        bottom = a[1:2 * h:2, 0:2 * w:2] + a[1:2 * h:2, 1:2 * w:2]
        return ((top + bottom) * F(0.25)).astype(np.float32)


def level_index(lightmap_w, lightmap_h, accuracy_factor):
    """min(accuracyFactor, LuminanceBuffer.LevelCount - 1), LightingRenderer.HDR.cs:164; the target is (W / 2) x (H / 2) with a full chain."""
    level_count = int(math.floor(math.log2(max(lightmap_w // 2, lightmap_h // 2)))) + 1
    return min(accuracy_factor, level_count - 1)


def luminance_level(texels, fmt, rw, rh, accuracy_factor):
    """(level index, level) as HistogramUpdateTask reads it (HDR.cs:38-41,176-177), or (level index, None) when the level has no texels."""
    texels = np.asarray(texels)
    level = level_index(texels.shape[1], texels.shape[0], accuracy_factor)
    if ((rw // 2) >> level) == 0 or ((rh // 2) >> level) == 0:
        return level, None
    a = luminance_level0(decode_texels(texels, fmt), rw, rh)
    for _ in range(level):
        a = next_level(a)
    assert a.shape == ((rh // 2) >> level, (rw // 2) >> level)
    return level, a


# ---- Histogram.cs -----------------------------------------------------------------------------------------------------------------
def bucket_table(max_value, power, bucket_count=64):
    """The ctor's BucketMaxValues, Histogram.cs:69-75: doubles; `1 + maxValue` is a float sum; the cast binds before the `- 1`."""
    max_value_plus_one_log = math.log(float(F(1) + F(max_value))) / math.log(float(F(power)))
    out = np.zeros(bucket_count, np.float32)
    for i in range(bucket_count):
        value_log = (max_value_plus_one_log / bucket_count) * (i + 1)
        out[i] = F(math.pow(float(F(power)), value_log)) - F(1)
    return out


def pick_bucket(table, value):
    """PickBucketForValue, Histogram.cs:115-133."""
    n = len(table)
    value = F(value)
    if value < table[0]:
        return 0
    elif value >= table[n - 2]:
        return n - 1
    i, mx = 0, n - 1
    while i <= mx:
        pivot = i + ((mx - i) >> 1)
        if table[pivot] <= value:
            i = pivot + 1
        else:
            mx = pivot - 1
    return i


def order_key(values):
    """Array.Sort's order (Single.CompareTo) as an integer key: NaN first, then -inf .. +inf; -0 before +0 (our decision)."""
    v = np.ascontiguousarray(values, np.float32)
    u = v.view(np.uint32).astype(np.uint64)
    key = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(v), 0, key).astype(np.uint64)


def sort_values(values):
    v = np.ascontiguousarray(values, np.float32).reshape(-1)
    return v[np.argsort(order_key(v), kind="stable")]


def median_index(sorted_values, ignore_zeroes):
    """Histogram.cs:176-180: offset 0, or with IgnoreZeroes Array.LastIndexOf(buffer, 0) (-0 equals 0; -1 when there is no zero)."""
    count = len(sorted_values)
    offset = 0
    if ignore_zeroes:
        zeros = np.flatnonzero(np.asarray(sorted_values) == 0)
        offset = int(zeros[-1]) if zeros.size else -1
    index = int((count - offset) / 2) + offset          # C# integer division truncates; count - offset > 0 here
    return max(0, min(index, count - 1))


def cs_min(a, b):
    """Math.Min(float, float): NaN if either is; -0 below +0."""
    if np.isnan(a) or np.isnan(b):
        return F(np.nan)
    if a == b:
        return a if np.signbit(a) else b
    return a if a < b else b


def cs_max(a, b):
    if np.isnan(a) or np.isnan(b):
        return F(np.nan)
    if a == b:
        return b if np.signbit(a) else a
    return a if a > b else b


class Result:
    """Histogram's state after Clear + Add: States (Count, Min, Max, Sum per bucket) and the totals."""

    def __init__(self, table):
        n = len(table)
        self.table = np.asarray(table, np.float32)
        self.count = np.zeros(n, np.int64)
        self.min = np.full(n, FLOAT_MAX, np.float32)
        self.max = np.zeros(n, np.float32)
        self.sum = np.zeros(n, np.float32)
        self.sample_count, self.total_min, self.total_max, self.mean, self.median, self.total_sum = 0, F(0), F(0), F(0), F(0), F(0)

    def get_percentile(self, percent):
        """GetPercentile, Histogram.cs:135-163 -> (ok, bucketIndex, value); Arithmetic.Lerp(a, b, x) = a + ((b - a) * x) (Squared.Util)."""
        percent = F(percent)
        if self.sample_count < 1 or percent < 0 or percent > 100:
            return False, 0, F(0)
        sample_index = int(F(self.sample_count) * percent / F(100.0))
        first = 0
        for i in range(len(self.table)):
            count = int(self.count[i])
            local = sample_index - first
            if 0 <= local < count:
                lo = self.table[i - 1] if i > 0 else F(0)
                hi = self.table[i]
                return True, i, F(lo + ((hi - lo) * (F(local) / F(count))))
            first += count
        raise RuntimeError("no bucket holds the sample")        # `throw new Exception()`, :162

    def buckets(self):
        """Buckets, Histogram.cs:221-245: (BucketStart, BucketEnd, Min, Max, Mean, Count)."""
        out = []
        for i in range(len(self.table)):
            c = int(self.count[i])
            out.append((self.table[i - 1] if i > 0 else F(0), self.table[i], self.min[i] if c > 0 else F(0), self.max[i],
                        F(self.sum[i] / F(c)) if c > 0 else F(0), c))
        return out


def _finish(r):
    """Histogram.cs:202-218."""
    r.mean = F(r.total_sum / F(r.sample_count)) if r.sample_count > 0 else F(0)
    mn, mx = FLOAT_MAX, F(0)
    for j in range(len(r.table)):
        mn = cs_min(r.min[j], mn)
        mx = cs_max(r.max[j], mx)
    r.total_min = mn if r.sample_count > 0 else F(0)
    r.total_max = mx
    return r


def histogram_add_scalar(values, table, scale_factor, ignore_zeroes):
    """Histogram.Clear + Histogram.Add (Histogram.cs:98-112,165-219), statement for statement."""
    r = Result(table)
    scale_factor = F(scale_factor)
    buf = sort_values(values)
    with np.errstate(all="ignore"):
        r.median = F(buf[median_index(buf, ignore_zeroes)] * scale_factor)
        for raw in buf:
            if ignore_zeroes and raw <= 0:
                continue
            value = F(raw * scale_factor)
            r.total_sum = F(r.total_sum + value)
            r.sample_count += 1
            j = pick_bucket(r.table, value)
            r.count[j] += 1
            r.sum[j] = F(r.sum[j] + value)
            r.min[j] = cs_min(r.min[j], value)
            r.max[j] = cs_max(r.max[j], value)
    return _finish(r)


def histogram_add(values, table, scale_factor, ignore_zeroes):
    """The same, vectorised: np.add.accumulate on float32 adds one element after the other, each sum rounded -- the C# loop's arithmetic."""
    r = Result(table)
    scale_factor = F(scale_factor)
    buf = sort_values(values)
    n = len(r.table)
    with np.errstate(all="ignore"):
        r.median = F(buf[median_index(buf, ignore_zeroes)] * scale_factor)
        kept = buf[~(buf <= 0)] if ignore_zeroes else buf
        v = (kept * scale_factor).astype(np.float32)
        r.sample_count = int(v.size)
        if v.size:
            r.total_sum = F(np.add.accumulate(np.concatenate([np.zeros(1, np.float32), v]), dtype=np.float32)[-1])
        b = np.searchsorted(r.table, v, side="right")             # entries <= value (the table increases)
        b = np.where(v < r.table[0], 0, np.where(v >= r.table[n - 2], n - 1, b))
        b = np.where(np.isnan(v), 0, b)
        for j in np.unique(b):
            vj = v[b == j]
            r.count[j] = vj.size
            r.sum[j] = F(np.add.accumulate(np.concatenate([np.zeros(1, np.float32), vj]), dtype=np.float32)[-1])
            if np.isnan(vj).any():
                r.min[j] = r.max[j] = F(np.nan)
            else:
                k = order_key(vj)
                r.min[j] = cs_min(FLOAT_MAX, vj[np.argmin(k)])
                r.max[j] = cs_max(F(0), vj[np.argmax(k)])
    return _finish(r)
