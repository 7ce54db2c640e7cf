// brightness.hip -- brightness estimation on the device: the luminance target of technique CalculateLuminance
// (Illuminant/Shaders/Resolve.fx:15,212-227,337-343; drawn by Illuminant/Lighting/LightingRenderer.cs:839-898), one level of its mip
// chain (RenderedLighting.TryComputeHistogram, Illuminant/Lighting/LightingRenderer.HDR.cs:154-183) and Histogram.Clear + Histogram.Add
// over that level (Illuminant/Histogram.cs:94-219).
//
// Numerics: every operation rounds (this file is compiled with -ffp-contract=off).  Level 0 is a POINT sample of
// the lightmap at the destination pixel centre, mapped in exact integer arithmetic; level k is the 2 x 2 box ((a + b) + (c + d)) * 0.25f
// of level k - 1, an odd last row / column dropped.  The statistics are integers and selected values, so they are exact: counts by
// integer atomics, minima / maxima on order-preserving integer keys, the median by a radix select on the same key.  Sums are the only
// floating-point reduction: every partial sum has one owner and the partials meet in a fixed order -- no float atomics, so two calls
// on the same lightmap return the same bits.
//
// Array.Sort's order (Single.CompareTo): NaNs first, then -inf .. +inf with -0 == 0.  The key sends every NaN to 0 and orders -0 before
// +0 (the reference's unstable sort leaves the order of equal zeros open; so do Math.Min / Math.Max of a +0 / -0 pair across runtimes:
// here min(-0, +0) = -0 and max = +0).  The reference searches the whole, possibly longer, scratch array for the last zero
// (Array.LastIndexOf(buffer, 0), Histogram.cs:178); there is no stale tail here: exactly the level's n values are looked at.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "internal.hpp"

namespace ilm {

namespace {

// The statistics / select kernels walk the level in chunks of 4 waves x 4 steps x 64 lanes; workgroup b of G takes chunks b, b + G, ...
// (G = min(chunks, kStatBlocksMax): a function of n alone, so the partial sums and their order are too).
constexpr int kStatItems = 1024;
constexpr int kStatBlocksMax = 1024;

ILM_DEV uint32_t order_key(float f) {
    const uint32_t u = __float_as_uint(f);
    if (f != f) return 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
ILM_DEV float key_value(uint32_t k) {
    if (k == 0u) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// float3(0.299, 0.587, 0.144): Resolve.fx:15 (the reference's constant; HDR.fxh's 0.114 is another one)
ILM_DEV float luminance_of(float r, float g, float b) { return (r * 0.299f + g * 0.587f) + b * 0.144f; }

template <int FORMAT>
ILM_DEV float load_luminance(const void* texels, size_t o) {
    if (FORMAT == ILM_LIGHTMAP_FLOAT4) {
        const float4 v = reinterpret_cast<const float4*>(texels)[o];
        return luminance_of(v.x, v.y, v.z);
    } else if (FORMAT == ILM_LIGHTMAP_HALF4) {
        const uint2 v = reinterpret_cast<const uint2*>(texels)[o];
        return luminance_of(__half2float(__ushort_as_half((unsigned short)(v.x & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(v.x >> 16))),
                            __half2float(__ushort_as_half((unsigned short)(v.y & 0xFFFFu))));
    } else {
        const uint32_t v = reinterpret_cast<const uint32_t*>(texels)[o];
        return luminance_of((float)(v & 0xFFu) / 255.0f, (float)((v >> 8) & 0xFFu) / 255.0f, (float)((v >> 16) & 0xFFu) / 255.0f);
    }
}

// One wave per 8 x 8 block of level 0, four blocks side by side per workgroup.  Lane l holds the texel at the Morton position of l
// (x bits 0, 2, 4 of l; y bits 1, 3, 5), so the four children of a level-k texel sit in lanes that differ in bits 2k - 2 and 2k - 1:
// one __shfl_xor per tree stage, and the lowest lane of each group computes (a + b) + (c + d) in exactly that order.  A level-k texel
// inside the level has all of its children inside level k - 1, so what lanes outside level 0 hold is never read by a texel that is stored.
// Only the odd rows of the lightmap are read (for even sizes source texel (2x + 1, 2y + 1)).
template <int FORMAT>
__global__ __launch_bounds__(256) void luminance_kernel(const LuminanceLaunch a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lx = (lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4);
    const int ly = ((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4);
    const int x = ((int)blockIdx.x * 4 + wave) * 8 + lx, y = (int)blockIdx.y * 8 + ly;
    const bool inside = x < a.w0 && y < a.h0;
    float l = 0.0f;
    if (inside) {
        int sx, sy;
        if (a.rw == 2 * a.w0) sx = 2 * x + 1;
        else { const long long q = ((long long)(2 * x + 1) * a.rw) / (2ll * a.w0); sx = q < a.rw - 1 ? (int)q : a.rw - 1; }
        if (a.rh == 2 * a.h0) sy = 2 * y + 1;
        else { const long long q = ((long long)(2 * y + 1) * a.rh) / (2ll * a.h0); sy = q < a.rh - 1 ? (int)q : a.rh - 1; }
        l = load_luminance<FORMAT>(a.texels, (size_t)sy * (size_t)a.pitch + (size_t)sx);
    }
    if (a.level == 0) {
        if (inside) a.out[(size_t)y * (size_t)a.w0 + (size_t)x] = l;
        return;
    }
    const int last = a.level < 3 ? a.level : 3;
#pragma unroll
    for (int k = 1; k <= 3; k++) {
        float s = l + __shfl_xor(l, 1 << (2 * k - 2));
        s = s + __shfl_xor(s, 1 << (2 * k - 1));
        l = s * 0.25f;
        if (k == last) {
            const int wk = a.w0 >> k, hk = a.h0 >> k, xk = x >> k, yk = y >> k;
            if ((lane & ((1 << (2 * k)) - 1)) == 0 && xk < wk && yk < hk) a.out[(size_t)yk * (size_t)wk + (size_t)xk] = l;
        }
    }
}

// levels past 3, one at a time on the <= 1/64-size buffer
__global__ __launch_bounds__(256) void luminance_mip_kernel(const float* __restrict__ src, int sw, float* __restrict__ dst, int dw, int dh) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= dw * dh) return;
    const int x = i % dw, y = i / dw;
    const float* p = src + (size_t)(2 * y) * (size_t)sw + (size_t)(2 * x);
    dst[i] = ((p[0] + p[1]) + (p[sw] + p[sw + 1])) * 0.25f;
}

// ---- statistics ------------------------------------------------------------------------------------------------------------------
// `work` (uint32 words, zero on entry): [0, 256) bucket counts, [256, 512) ~key of each bucket's smallest value, [512, 768) key of its
// largest, [768, 1792) the four digit histograms of the radix select, [1792, 1796) raw NaNs, raw values < 0, raw zeros, NaN samples.
constexpr int kWorkCount = 0, kWorkMin = 256, kWorkMax = 512, kWorkSelect = 768, kWorkCounters = 1792;

// PickBucketForValue, Histogram.cs:115-133
ILM_DEV int pick_bucket(float value, const float* table, int bucket_count) {
    if (value < table[0]) return 0;
    if (value >= table[bucket_count - 2]) return bucket_count - 1;
    int i = 0, max = bucket_count - 1;
    while (i <= max) {
        const int pivot = i + ((max - i) >> 1);
        if (table[pivot] <= value) i = pivot + 1; else max = pivot - 1;
    }
    return i;
}

// Histogram.Add's loop (Histogram.cs:183-200) over the workgroup's chunks, and the first digit of the select
__global__ __launch_bounds__(256) void histogram_stats_kernel(const HistogramLaunch a) {
    __shared__ float s_table[256];
    __shared__ uint32_t s_count[256], s_min[256], s_max[256], s_select[256], s_counters[4];
    __shared__ float s_sum[4][256];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    s_table[t] = t < a.bucket_count ? a.table[t] : 0.0f;
    s_count[t] = 0u; s_min[t] = 0u; s_max[t] = 0u; s_select[t] = 0u;
    for (int w = 0; w < 4; w++) s_sum[w][t] = 0.0f;
    if (t < 4) s_counters[t] = 0u;
    __syncthreads();
    uint32_t nans = 0u, negatives = 0u, zeros = 0u, nan_samples = 0u;       // wave-uniform
    for (int chunk = (int)blockIdx.x * kStatItems; chunk < a.n; chunk += (int)gridDim.x * kStatItems)
    for (int step = 0; step < kStatItems / 256; step++) {
        const int at = chunk + wave * (kStatItems / 4) + step * 64;
        if (at >= a.n) break;
        const int i = at + lane;
        const bool in = i < a.n;
        const float raw = in ? a.values[i] : 0.0f;
        if (in) atomicAdd(&s_select[order_key(raw) >> 24], 1u);
        nans += (uint32_t)__popcll(__ballot(in && raw != raw));
        negatives += (uint32_t)__popcll(__ballot(in && raw < 0.0f));
        zeros += (uint32_t)__popcll(__ballot(in && raw == 0.0f));
        const bool valid = in && !(a.ignore_zeroes && raw <= 0.0f);
        const float value = raw * a.scale;
        const int bucket = valid ? pick_bucket(value, s_table, a.bucket_count) : 0;
        if (valid && value == value) {
            const uint32_t k = order_key(value);
            atomicMax(&s_min[bucket], ~k);
            atomicMax(&s_max[bucket], k);
        }
        nan_samples += (uint32_t)__popcll(__ballot(valid && value != value));
        // the wave's samples bucket by bucket: the count by one integer atomic, the sum by a butterfly whose order is fixed, added by one lane
        // to the wave's own row
        unsigned long long todo = __ballot(valid);
        while (todo) {
            const int b = __shfl(bucket, (int)__ffsll((long long)todo) - 1);
            const bool mine = valid && bucket == b;
            const unsigned long long same = __ballot(mine);
            float c = mine ? value : 0.0f;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
            if (lane == 0) {
                atomicAdd(&s_count[b], (uint32_t)__popcll(same));
                s_sum[wave][b] += c;
            }
            todo &= ~same;
        }
    }
    if (lane == 0) {
        if (nans) atomicAdd(&s_counters[0], nans);
        if (negatives) atomicAdd(&s_counters[1], negatives);
        if (zeros) atomicAdd(&s_counters[2], zeros);
        if (nan_samples) atomicAdd(&s_counters[3], nan_samples);
    }
    __syncthreads();
    if (t < a.bucket_count) {
        if (s_count[t]) atomicAdd(&a.work[kWorkCount + t], s_count[t]);
        if (s_min[t]) atomicMax(&a.work[kWorkMin + t], s_min[t]);
        if (s_max[t]) atomicMax(&a.work[kWorkMax + t], s_max[t]);
        a.partials[(size_t)t * (size_t)gridDim.x + (size_t)blockIdx.x] = (s_sum[0][t] + s_sum[1][t]) + (s_sum[2][t] + s_sum[3][t]);
    }
    if (s_select[t]) atomicAdd(&a.work[kWorkSelect + t], s_select[t]);
    if (t < 4 && s_counters[t]) atomicAdd(&a.work[kWorkCounters + t], s_counters[t]);
}

// medianIndex, Histogram.cs:176-180: the offset is 0 unless IgnoreZeroes, then Array.LastIndexOf(buffer, 0) -- the index of the last zero
// in sort order, or -1 when there is none (kept as the reference has it)
ILM_DEV int median_index(const HistogramLaunch& a) {
    int offset = 0;
    if (a.ignore_zeroes) {
        const uint32_t* c = a.work + kWorkCounters;
        offset = c[2] > 0u ? (int)(c[0] + c[1] + c[2]) - 1 : -1;
    }
    const int index = (a.n - offset) / 2 + offset;
    return index < 0 ? 0 : (index > a.n - 1 ? a.n - 1 : index);
}

// the digit whose run of the histogram holds rank k (256 threads): prefix <- prefix * 256 + digit, k <- rank inside the run
ILM_DEV void pick_digit(const uint32_t* hist, uint32_t* s_scan, uint32_t* s_state, uint32_t& prefix, uint32_t& k) {
    const int t = threadIdx.x;
    const uint32_t h = hist[t];
    s_scan[t] = h;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const uint32_t v = t >= o ? s_scan[t - o] : 0u;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    const uint32_t inclusive = s_scan[t], exclusive = inclusive - h;
    if (h > 0u && exclusive <= k && k < inclusive) { s_state[0] = (uint32_t)t; s_state[1] = k - exclusive; }
    __syncthreads();
    prefix = (prefix << 8) | s_state[0];
    k = s_state[1];
    __syncthreads();
}

// digit `pass` (1..3) of the select: the histogram of the next 8 key bits over the values whose leading digits are the ones picked so far
__global__ __launch_bounds__(256) void histogram_select_kernel(const HistogramLaunch a, int pass) {
    __shared__ uint32_t s_hist[256], s_scan[256], s_state[2];
    const int t = threadIdx.x;
    s_hist[t] = 0u;
    if (t < 2) s_state[t] = 0u;
    uint32_t prefix = 0u, k = (uint32_t)median_index(a);
    for (int q = 0; q < pass; q++) pick_digit(a.work + kWorkSelect + 256 * q, s_scan, s_state, prefix, k);
    const int high = 32 - 8 * pass, low = 24 - 8 * pass;
    for (int begin = (int)blockIdx.x * kStatItems; begin < a.n; begin += (int)gridDim.x * kStatItems) {
        const int end = begin + kStatItems < a.n ? begin + kStatItems : a.n;
        for (int i = begin + t; i < end; i += 256) {
            const uint32_t key = order_key(a.values[i]);
            if ((key >> high) == prefix) atomicAdd(&s_hist[(key >> low) & 255u], 1u);
        }
    }
    __syncthreads();
    if (s_hist[t]) atomicAdd(&a.work[kWorkSelect + 256 * pass + t], s_hist[t]);
}

// One workgroup per bucket: the workgroups' partial sums of that bucket, added in a fixed order (thread t takes partials t, t + 256, ...
// in that order, the 256 threads meet in a fixed tree)
__global__ __launch_bounds__(256) void histogram_reduce_kernel(const HistogramLaunch a) {
    __shared__ double s_sum[256];
    const int t = threadIdx.x;
    const float* p = a.partials + (size_t)blockIdx.x * (size_t)a.blocks;
    double sum = 0.0;
    for (int b = t; b < a.blocks; b += 256) sum += (double)p[b];
    s_sum[t] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) s_sum[t] = s_sum[t] + s_sum[t + o];
        __syncthreads();
    }
    if (t == 0) a.sums[blockIdx.x] = s_sum[0];
}

// One workgroup: the last digit of the select, the per-bucket states (BucketState, Histogram.cs:32-35) and the totals of Histogram.Add
// (:202-218) into the block the host reads: bucket_count x IlmHistogramBucket, then { SampleCount, Min, Max, Sum, Median }.
__global__ __launch_bounds__(256) void histogram_finish_kernel(const HistogramLaunch a) {
    __shared__ uint32_t s_scan[256], s_state[2], s_count[256], s_min[256], s_max[256];
    __shared__ double s_sum[256];
    const int t = threadIdx.x;
    if (t < 2) s_state[t] = 0u;
    uint32_t prefix = 0u, k = (uint32_t)median_index(a);
    for (int q = 0; q < 4; q++) pick_digit(a.work + kWorkSelect + 256 * q, s_scan, s_state, prefix, k);
    const bool nan_sample = a.work[kWorkCounters + 3] > 0u;
    const uint32_t key_float_max = order_key(3.402823466e+38f), key_zero = 0x80000000u;
    uint32_t count = 0u, min_key = 0u, max_key = 0u;
    double sum = 0.0;
    if (t < a.bucket_count) {
        count = a.work[kWorkCount + t]; min_key = a.work[kWorkMin + t]; max_key = a.work[kWorkMax + t];
        sum = a.sums[t];
        // Min starts at float.MaxValue, Max at 0 (Histogram.cs:108-111); Math.Min / Math.Max keep a NaN, and a NaN sample is in bucket 0
        float mn = key_value(min_key ? (~min_key < key_float_max ? ~min_key : key_float_max) : key_float_max);
        float mx = key_value(max_key > key_zero ? max_key : key_zero);
        if (t == 0 && nan_sample) mn = mx = key_value(0u);
        IlmHistogramBucket out;
        out.Count = (int32_t)count; out.Min = mn; out.Max = mx; out.Sum = (float)sum;
        a.out_buckets[t] = out;
    }
    s_count[t] = count; s_min[t] = min_key; s_max[t] = max_key; s_sum[t] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            s_count[t] += s_count[t + o];
            s_sum[t] = s_sum[t] + s_sum[t + o];
            s_min[t] = s_min[t] > s_min[t + o] ? s_min[t] : s_min[t + o];
            s_max[t] = s_max[t] > s_max[t + o] ? s_max[t] : s_max[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        const uint32_t samples = s_count[0];
        float mn = key_value(s_min[0] ? (~s_min[0] < key_float_max ? ~s_min[0] : key_float_max) : key_float_max);
        float mx = key_value(s_max[0] > key_zero ? s_max[0] : key_zero);
        if (nan_sample) mn = mx = key_value(0u);
        if (samples == 0u) mn = 0.0f;
        a.out_totals[0] = __uint_as_float(samples);
        a.out_totals[1] = mn;
        a.out_totals[2] = mx;
        a.out_totals[3] = (float)s_sum[0];
        a.out_totals[4] = key_value(prefix) * a.scale;          // Median = buffer[medianIndex] * scaleFactor, Histogram.cs:181
    }
}

}  // namespace

hipError_t launch_luminance_level(const LuminanceLaunch& a, hipStream_t stream) {
    LuminanceLaunch first = a;
    if (a.level > 3) first.out = a.mip[0];
    const dim3 grid((unsigned)((a.w0 + 31) / 32), (unsigned)((a.h0 + 7) / 8));
    if (a.format == ILM_LIGHTMAP_FLOAT4) hipLaunchKernelGGL(luminance_kernel<ILM_LIGHTMAP_FLOAT4>, grid, dim3(256), 0, stream, first);
    else if (a.format == ILM_LIGHTMAP_HALF4) hipLaunchKernelGGL(luminance_kernel<ILM_LIGHTMAP_HALF4>, grid, dim3(256), 0, stream, first);
    else hipLaunchKernelGGL(luminance_kernel<ILM_LIGHTMAP_RGBA8>, grid, dim3(256), 0, stream, first);
    hipError_t e = hipGetLastError();
    for (int k = 4; k <= a.level && e == hipSuccess; k++) {
        const float* src = a.mip[k & 1];
        float* dst = k == a.level ? a.out : a.mip[(k + 1) & 1];
        const int dw = a.w0 >> k, dh = a.h0 >> k;
        hipLaunchKernelGGL(luminance_mip_kernel, dim3((unsigned)((dw * dh + 255) / 256)), dim3(256), 0, stream, src, a.w0 >> (k - 1), dst, dw, dh);
        e = hipGetLastError();
    }
    return e;
}

int histogram_blocks(int n) { const int chunks = (n + kStatItems - 1) / kStatItems; return chunks < kStatBlocksMax ? chunks : kStatBlocksMax; }
size_t histogram_work_bytes() { return sizeof(uint32_t) * (size_t)(kWorkCounters + 8); }

hipError_t launch_histogram(const HistogramLaunch& a, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(a.work, 0, histogram_work_bytes(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(histogram_stats_kernel, dim3((unsigned)a.blocks), dim3(256), 0, stream, a);
    for (int pass = 1; pass <= 3; pass++) hipLaunchKernelGGL(histogram_select_kernel, dim3((unsigned)a.blocks), dim3(256), 0, stream, a, pass);
    hipLaunchKernelGGL(histogram_reduce_kernel, dim3((unsigned)a.bucket_count), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(histogram_finish_kernel, dim3(1), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ilm
