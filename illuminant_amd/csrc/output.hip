// output.hip -- the callers on the output side of the two hot paths, for gfx950:
//   * particle read-back: FillReadbackResult (Illuminant/Particles/ParticleReadback.cs:73-167) as an ordered device-side
//     compaction of the live particles into draw-call records (the reference copies three float4 planes per chunk to the host
//     and filters there: 48 B/slot over PCIe; here 48 B per LIVE particle);
//   * lightmap resolve: the LightingResolve[WithAlbedo] techniques of Illuminant/Shaders/Resolve.fx:25-233 + HDR.fxh, a pure stream
//     (8 B read + 4..16 B written per pixel): no LDS, no MFMA; at 0.6 of HBM's rate it is as close to the VALU's issue limit.
#include "internal.hpp"

namespace ilm {

constexpr int kRbBlock = 1024;

ILM_DEV bool readback_live(const ReadbackLaunch& a, int chunk, int slot, float& life) {
    const int count = (a.element_counts != nullptr) ? a.element_counts[chunk] : a.slots;
    if (slot >= count || slot >= a.slots)
        return false;
    life = a.chunk_bases[chunk][3 * a.stride + slot];
    return life > 0.0f;
}

__global__ __launch_bounds__(kRbBlock) void readback_count_kernel(const ReadbackLaunch a, int blocks_per_chunk) {
    __shared__ int wave_counts[kRbBlock / 64];
    const int chunk = (int)blockIdx.x / blocks_per_chunk, blk = (int)blockIdx.x - chunk * blocks_per_chunk;
    float life;
    const bool live = readback_live(a, chunk, blk * kRbBlock + (int)threadIdx.x, life);
    const unsigned long long m = __ballot(live);
    if ((threadIdx.x & 63u) == 0u) wave_counts[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < kRbBlock / 64; w++) n += wave_counts[w];
        a.block_counts[blockIdx.x] = n;
    }
}

__global__ __launch_bounds__(kRbBlock) void readback_emit_kernel(const ReadbackLaunch a, int blocks_per_chunk) {
    __shared__ int wave_counts[kRbBlock / 64];
    __shared__ int partial[kRbBlock / 64];
    __shared__ int block_base;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    int sum = 0;
    for (int i = (int)threadIdx.x; i < (int)blockIdx.x; i += kRbBlock) sum += a.block_counts[i];
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if (lane == 0) partial[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int b = 0;
        for (int w = 0; w < kRbBlock / 64; w++) b += partial[w];
        block_base = b;
        if (blockIdx.x == gridDim.x - 1)
            *a.out_count = b + a.block_counts[blockIdx.x];      // the TOTAL, even beyond the capacity
    }
    const int chunk = (int)blockIdx.x / blocks_per_chunk, blk = (int)blockIdx.x - chunk * blocks_per_chunk;
    const int slot = blk * kRbBlock + (int)threadIdx.x;
    float life;
    const bool live = readback_live(a, chunk, slot, life);
    const unsigned long long m = __ballot(live);
    if (lane == 0) wave_counts[wave] = __popcll(m);
    __syncthreads();
    if (!live)
        return;
    int index = block_base + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) index += wave_counts[w];
    if (index >= a.capacity)
        return;

    // FillReadbackResult's loop body, ParticleReadback.cs:118-163
    const IlmReadbackParams& p = a.params;
    const float* base = a.chunk_bases[chunk];
    const int64_t S = a.stride;
    const float px = base[slot], py = base[S + slot];
    const float4 rc = mk4(base[12 * S + slot], base[13 * S + slot], base[14 * S + slot], base[15 * S + slot]);
    const float4 rd = mk4(base[16 * S + slot], base[17 * S + slot], base[18 * S + slot], base[19 * S + slot]);
    const float sz = rd.x;
    const float rot = fmodf(rd.y, 6.28318530717958647692f);          // (float)(2 * Math.PI)
    IlmReadbackDrawCall dc;
    dc.TextureRegion[0] = p.TextureRegion[0]; dc.TextureRegion[1] = p.TextureRegion[1];
    dc.TextureRegion[2] = p.TextureRegion[2]; dc.TextureRegion[3] = p.TextureRegion[3];
    if ((a.frame_count_x > 1) || (a.frame_count_y > 1)) {
        float fx = floorf(fabsf(p.AnimationRate[0]) * life), fy = floorf(fabsf(p.AnimationRate[1]) * life);
        fy += (float)floor((double)rd.w);
        if (p.ColumnFromVelocity) fx += (float)rint((double)rot / a.max_angle_x);        // Math.Round: half to even, in double
        if (p.RowFromVelocity)    fy += (float)rint((double)rot / a.max_angle_y);
        fx = fmodf(fmaxf(0.0f, fx), (float)a.frame_count_x);
        fy = clampf(fy, 0.0f, (float)(a.frame_count_y - 1));
        if (p.AnimationRate[0] < 0.0f) fx = (float)a.frame_count_x - fx;
        if (p.AnimationRate[1] < 0.0f) fy = (float)a.frame_count_y - fy;
        const float ox = fx * a.region_w, oy = fy * a.region_h;
        dc.TextureRegion[0] += ox; dc.TextureRegion[1] += oy; dc.TextureRegion[2] += ox; dc.TextureRegion[3] += oy;
    }
    dc.Position[0] = px; dc.Position[1] = py;
    dc.SortOrder = p.SortedReadback ? (py + p.ZToY) : 0.0f;
    dc.Scale[0] = p.Size[0] * sz; dc.Scale[1] = p.Size[1] * sz;
    dc.MultiplyColor[0] = (uint8_t)(int32_t)(rc.x * 255.0f);
    dc.MultiplyColor[1] = (uint8_t)(int32_t)(rc.y * 255.0f);
    dc.MultiplyColor[2] = (uint8_t)(int32_t)(rc.z * 255.0f);
    dc.MultiplyColor[3] = (uint8_t)(int32_t)(rc.w * 255.0f);
    dc.Rotation = (float)((p.RotationFromVelocity ? 1.0 : 0.0) * (double)rot);
    dc._pad = 0;
    a.out[index] = dc;
}

hipError_t launch_readback(const ReadbackLaunch& a, hipStream_t stream) {
    const int blocks_per_chunk = (a.slots + kRbBlock - 1) / kRbBlock;
    const int blocks = a.chunk_count * blocks_per_chunk;
    if (blocks <= 0) return hipMemsetAsync(a.out_count, 0, sizeof(int32_t), stream);
    hipLaunchKernelGGL(readback_count_kernel, dim3(blocks), dim3(kRbBlock), 0, stream, a, blocks_per_chunk);
    hipLaunchKernelGGL(readback_emit_kernel, dim3(blocks), dim3(kRbBlock), 0, stream, a, blocks_per_chunk);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// lightmap resolve
// ---------------------------------------------------------------------------------------------
ILM_DEV float4 load_lightmap_texel(const void* texels, int format, size_t o) {
    if (format == ILM_LIGHTMAP_FLOAT4)
        return reinterpret_cast<const float4*>(texels)[o];
    if (format == ILM_LIGHTMAP_HALF4) {
        const uint2 v = reinterpret_cast<const uint2*>(texels)[o];
        return mk4(__half2float(__ushort_as_half((unsigned short)(v.x & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(v.x >> 16))),
                   __half2float(__ushort_as_half((unsigned short)(v.y & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(v.y >> 16))));
    }
    const uint32_t v = reinterpret_cast<const uint32_t*>(texels)[o];
    return mk4((float)(v & 0xFFu) / 255.0f, (float)((v >> 8) & 0xFFu) / 255.0f, (float)((v >> 16) & 0xFFu) / 255.0f, (float)(v >> 24) / 255.0f);
}

ILM_DEV void store_lightmap_texel(void* texels, int format, size_t o, float4 c) {
    if (format == ILM_LIGHTMAP_FLOAT4) {
        reinterpret_cast<float4*>(texels)[o] = c;
    } else if (format == ILM_LIGHTMAP_HALF4) {
        uint2 v;
        v.x = (uint32_t)__half_as_ushort(__float2half_rn(c.x)) | ((uint32_t)__half_as_ushort(__float2half_rn(c.y)) << 16);
        v.y = (uint32_t)__half_as_ushort(__float2half_rn(c.z)) | ((uint32_t)__half_as_ushort(__float2half_rn(c.w)) << 16);
        reinterpret_cast<uint2*>(texels)[o] = v;
    } else {
        const uint32_t r = (uint32_t)rintf(sat(c.x) * 255.0f), g = (uint32_t)rintf(sat(c.y) * 255.0f);
        const uint32_t b = (uint32_t)rintf(sat(c.z) * 255.0f), al = (uint32_t)rintf(sat(c.w) * 255.0f);
        reinterpret_cast<uint32_t*>(texels)[o] = r | (g << 8) | (b << 16) | (al << 24);
    }
}

// pow_pos: hlsl_math.hpp

ILM_DEV float4 resolve_texel(const ResolveLaunch& a, float4 color, float4 albedo) {
    float r, g, b, alpha;
    if (a.albedo != nullptr) {
        // ResolveWithAlbedoCommon, Resolve.fx:43-60 (AlbedoIsSRGB = 0): light *= InverseScaleFactor * 2, then
        // lerp(albedo.rgb, albedo.rgb * light.rgb, saturate(light.a)); the alpha is the albedo's
        const float k = a.inverse_scale * 2.0f;
        const float t = sat(color.w * k);
        r = lerp(albedo.x, albedo.x * (color.x * k), t); g = lerp(albedo.y, albedo.y * (color.y * k), t); b = lerp(albedo.z, albedo.z * (color.z * k), t);
        alpha = albedo.w;
    } else {
        // ResolveCommon, Resolve.fx:25-40 (scale 1: the pixel's own texel)
        r = color.x * a.inverse_scale; g = color.y * a.inverse_scale; b = color.z * a.inverse_scale;
        alpha = 1.0f;
    }
    if (a.mode == ILM_HDR_GAMMA_COMPRESS) {
        // GammaCompress, HDR.fxh:11-18
        r = fmaxf(r + a.offset, 0.0f); g = fmaxf(g + a.offset, 0.0f); b = fmaxf(b + a.offset, 0.0f);
        const float result_luminance = r * 0.299f + g * 0.587f + b * 0.114f;
        const float scaled = (result_luminance * a.middle_gray) * a.inv_average_luminance;
        const float compressed = (scaled * (1.0f + (scaled * a.inv_maximum_luminance_squared))) * fast_rcp(1.0f + scaled);
        const float rescale = compressed * fast_rcp(result_luminance);
        // 0 / 0 at a black pixel is NaN in the shader as well (compressedLuminance / resultLuminance)
        r *= rescale; g *= rescale; b *= rescale;
    } else if (a.mode == ILM_HDR_TONE_MAP) {
        // ToneMappedLightingResolve[WithAlbedo]PixelShader, Resolve.fx:113-139,209-233; Uncharted2Tonemap, HDR.fxh:38-44
        const float kA = 0.15f, kB = 0.50f, kC = 0.10f, kD = 0.20f, kE = 0.02f, kF = 0.30f, kExactBelow = 0.03125f;
        const float e = a.exposure_minus_one + 1.0f, gm = a.gamma_minus_one + 1.0f;
        float v[3] = { fmaxf(0.0f, r + a.offset) * e, fmaxf(0.0f, g + a.offset) * e, fmaxf(0.0f, b + a.offset) * e };
        // num / den - kE / kF cancels as v goes to 0: at a black pixel the quotient is ONE ulp (2^-27) above kE / kF and the difference is
        // all rounding, so a dim pixel needs the IEEE quotient: t then equals the shader's bit for bit.  (With num * fast_rcp(den) an ulp
        // was lost at every seventh dim texel or so: 0.4 % off after pow with Gamma 0.1, 2 - 5 % with 0.45 and 0.8; two ulps low at v = 0
        // would be pow of a negative number.)  From kExactBelow = 1 / 32 on, t >= 0.0086, and the 1.5 ulp of the fast quotient (1.8e-7 q,
        // q = 0.0754 there and q / t falling) are at most 1.6e-6 of t, 6.3e-6 after Gamma <= 4.  Which quotient a channel gets depends on
        // its own value alone (a strip resolves to the bits of the whole frame), but a WAVE without a dim pixel branches round the
        // division (left to the compiler the select computes both everywhere): a lit frame over an ambient term pays nothing for it.
        // The kernel is as close to the VALU's limit as to HBM's: eleven more instructions per channel in every wave cost 20 % of its time.
        float num[3], den[3], q[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            num[k] = v[k] * (kA * v[k] + kC * kB) + kD * kE;
            den[k] = v[k] * (kA * v[k] + kB) + kD * kF;
        }
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = num[k] * fast_rcp(den[k]);
        if (__any(fminf(fminf(v[0], v[1]), v[2]) < kExactBelow)) {
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (v[k] < kExactBelow) q[k] = num[k] / den[k];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = pow_pos((q[k] - kE / kF) * a.inv_white, gm);
        r = v[0]; g = v[1]; b = v[2];
    } else {
        // LightingResolve[WithAlbedo]PixelShader, Resolve.fx:62-83,141-158
        const float e = a.exposure_minus_one + 1.0f, gm = a.gamma_minus_one + 1.0f;
        r = pow_pos(fmaxf(0.0f, r + a.offset) * e, gm);
        g = pow_pos(fmaxf(0.0f, g + a.offset) * e, gm);
        b = pow_pos(fmaxf(0.0f, b + a.offset) * e, gm);
    }
    return mk4(r, g, b, alpha);
}

// Pure stream: 2 pixels per lane (16 B half4 loads, 8 B RGBA8 stores; a wave moves 1 KiB / 512 B per instruction).
__global__ __launch_bounds__(256) void resolve_kernel(const ResolveLaunch a) {
    const size_t pair = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)(a.row_end - a.row_begin) * (size_t)a.width;
    const size_t i = pair * 2;
    if (i >= n) return;
    const size_t o = (size_t)a.row_begin * (size_t)a.width + i;
    const bool two = (i + 1 < n) && ((o & 1) == 0);
    if (two && a.src_format == ILM_LIGHTMAP_HALF4 && a.dst_format == ILM_LIGHTMAP_RGBA8 && (a.albedo == nullptr || a.albedo_format == ILM_LIGHTMAP_RGBA8)) {
        // the back-buffer case: one 16-byte load, one 8-byte store
        const uint4 v = reinterpret_cast<const uint4*>(a.src)[o >> 1];
        const float4 c0 = mk4(__half2float(__ushort_as_half((unsigned short)(v.x & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(v.x >> 16))),
                              __half2float(__ushort_as_half((unsigned short)(v.y & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(v.y >> 16))));
        const float4 c1 = mk4(__half2float(__ushort_as_half((unsigned short)(v.z & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(v.z >> 16))),
                              __half2float(__ushort_as_half((unsigned short)(v.w & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(v.w >> 16))));
        float4 a0 = mk4(0.0f, 0.0f, 0.0f, 0.0f), a1 = a0;
        if (a.albedo != nullptr) {       // a Color texture: one 8-byte load for the two texels
            const uint2 av = reinterpret_cast<const uint2*>(a.albedo)[o >> 1];
            a0 = mk4((float)(av.x & 0xFFu) / 255.0f, (float)((av.x >> 8) & 0xFFu) / 255.0f, (float)((av.x >> 16) & 0xFFu) / 255.0f, (float)(av.x >> 24) / 255.0f);
            a1 = mk4((float)(av.y & 0xFFu) / 255.0f, (float)((av.y >> 8) & 0xFFu) / 255.0f, (float)((av.y >> 16) & 0xFFu) / 255.0f, (float)(av.y >> 24) / 255.0f);
        }
        const float4 r0 = resolve_texel(a, c0, a0), r1 = resolve_texel(a, c1, a1);
        uint2 out;
        out.x = (uint32_t)rintf(sat(r0.x) * 255.0f) | ((uint32_t)rintf(sat(r0.y) * 255.0f) << 8) | ((uint32_t)rintf(sat(r0.z) * 255.0f) << 16) | ((uint32_t)rintf(sat(r0.w) * 255.0f) << 24);
        out.y = (uint32_t)rintf(sat(r1.x) * 255.0f) | ((uint32_t)rintf(sat(r1.y) * 255.0f) << 8) | ((uint32_t)rintf(sat(r1.z) * 255.0f) << 16) | ((uint32_t)rintf(sat(r1.w) * 255.0f) << 24);
        reinterpret_cast<uint2*>(a.dst)[o >> 1] = out;
        return;
    }
    const float4 none = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    store_lightmap_texel(a.dst, a.dst_format, o, resolve_texel(a, load_lightmap_texel(a.src, a.src_format, o),
                                                                a.albedo ? load_lightmap_texel(a.albedo, a.albedo_format, o) : none));
    if (i + 1 < n)
        store_lightmap_texel(a.dst, a.dst_format, o + 1, resolve_texel(a, load_lightmap_texel(a.src, a.src_format, o + 1),
                                                                        a.albedo ? load_lightmap_texel(a.albedo, a.albedo_format, o + 1) : none));
}

hipError_t launch_resolve(const ResolveLaunch& a, hipStream_t stream) {
    const size_t n = (size_t)(a.row_end - a.row_begin) * (size_t)a.width;
    if (n == 0) return hipSuccess;
    const size_t pairs = (n + 1) / 2;
    hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// scaled, filtered resolve (ilm_resolve_lighting_scaled): source size != destination size
// ---------------------------------------------------------------------------------------------
// One axis of the fetch: the clamped texel-space coordinate of destination pixel p, then the taps and the weight (the header defines
// every operation and its order).  u lies in [r0, r1] within [0, size] -- a NaN became r0 -- so the conversions to int are exact and
// every index is clamped into the texture by integer arithmetic.
struct AxisTaps { int i0, i1; float f; };

ILM_DEV AxisTaps scaled_axis(int p, float origin, float extent, float r0, float r1, const float* offset, int size, int filter) {
    float u = r0 + (((float)p + 0.5f) - origin) * (r1 - r0) / extent;
    if (offset != nullptr) u += *offset;                      // LightmapUVOffset: the lightmap only, Resolve.fx:34,49
    u = fminf(fmaxf(u, r0), r1);                              // clamp2(texCoord, texRgn.xy, texRgn.zw)
    AxisTaps t;
    if (filter == ILM_FILTER_LINEAR) {
        const float s = u - 0.5f, fl = floorf(s);
        t.f = s - fl;
        t.i0 = min(max((int)fl, 0), size - 1);
        t.i1 = min(max((int)fl + 1, 0), size - 1);
    } else {
        t.f = 0.0f;
        t.i0 = t.i1 = min(max((int)floorf(u), 0), size - 1);
    }
    return t;
}

// byte / 255.0f without the division: q = x * fl(1 / 255), then one correction by the residual x - 255 q (two fused operations, written
// as such: the library is built without contraction).  The result is the IEEE quotient load_lightmap_texel forms for EVERY one of the 256
// bytes (tests/test_resolve_scaled_kat.py evaluates all of them in exact arithmetic), three instructions for a division's ten or so: a
// LINEAR fetch of a Color texture decodes sixteen bytes per pixel, and with divisions the resolve over a Color albedo ran 455 vector
// instructions per pixel instead of 303 (0.132 -> 0.098 ms at 4K).
ILM_DEV float unorm8(uint32_t byte) {
    const float x = (float)byte, r = 1.0f / 255.0f;
    const float q = x * r;
    return __builtin_fmaf(__builtin_fmaf(-q, 255.0f, x), r, q);
}

ILM_DEV float4 load_tap(const void* texels, int format, size_t o) {
    if (format != ILM_LIGHTMAP_RGBA8) return load_lightmap_texel(texels, format, o);
    const uint32_t v = reinterpret_cast<const uint32_t*>(texels)[o];
    return mk4(unorm8(v & 0xFFu), unorm8((v >> 8) & 0xFFu), unorm8((v >> 16) & 0xFFu), unorm8(v >> 24));
}

// The loads of one fetch, all issued before any of them is used; LINEAR's four taps or POINT's one (launch-uniform).
struct TexelTaps { float4 t00, t10, t01, t11; };

ILM_DEV TexelTaps load_taps(const void* texels, int format, int width, int filter, const AxisTaps& x, const AxisTaps& y) {
    const size_t row0 = (size_t)y.i0 * (size_t)width, row1 = (size_t)y.i1 * (size_t)width;
    TexelTaps t;
    t.t00 = load_tap(texels, format, row0 + (size_t)x.i0);
    if (filter == ILM_FILTER_LINEAR) {
        t.t10 = load_tap(texels, format, row0 + (size_t)x.i1);
        t.t01 = load_tap(texels, format, row1 + (size_t)x.i0);
        t.t11 = load_tap(texels, format, row1 + (size_t)x.i1);
    } else {
        t.t10 = t.t01 = t.t11 = t.t00;
    }
    return t;
}

ILM_DEV float4 filter_taps(const TexelTaps& t, int filter, float fx, float fy) {
    if (filter != ILM_FILTER_LINEAR) return t.t00;
    return lerp4(lerp4(t.t00, t.t10, fx), lerp4(t.t01, t.t11, fx), fy);
}

// A block owns a span of kScaledSpan destination pixels of ONE row: consecutive lanes are consecutive pixels (256 B RGBA8 or 1 KiB float4
// stored per wave instruction), and the row's own coordinate, taps and weight are computed once per wave and span, not once per pixel --
// they are wave-uniform and the tap rows go to scalar registers.  The source is re-read through the caches (magnified 2 x 2, every texel is
// fetched by about sixteen neighbouring pixels), so nothing is staged in LDS.  Format, filter and albedo branches are launch-uniform.
// Eight waves per SIMD (the second launch bound: 61 VGPRs instead of 76, nothing spilled): a wave waits for its taps and for the quotient
// of its coordinate two thirds of its life, and the two further waves took 13 % off the call (0.0623 -> 0.0547 ms at 4K).  A span of 256
// pixels, a block without the loop, was no faster (0.059).
constexpr int kScaledBlock = 256, kScaledSpan = 1024;

__global__ __launch_bounds__(kScaledBlock, 8) void resolve_scaled_kernel(const ResolveScaledLaunch a) {
    const ResolveLaunch& r = a.r;
    const int py = a.y0 + (int)blockIdx.y;
    const int span_begin = a.x0 + (int)blockIdx.x * kScaledSpan;
    const int span_end = min(span_begin + kScaledSpan, a.x1);
    const bool with_albedo = r.albedo != nullptr;
    AxisTaps ly = scaled_axis(py, a.quad[1], a.quad[3], a.lightmap_region[1], a.lightmap_region[3], &a.uv_offset[1], a.src_h, a.lightmap_filter);
    ly.i0 = __builtin_amdgcn_readfirstlane(ly.i0); ly.i1 = __builtin_amdgcn_readfirstlane(ly.i1);
    AxisTaps ay = { 0, 0, 0.0f };
    if (with_albedo) {
        ay = scaled_axis(py, a.quad[1], a.quad[3], a.albedo_region[1], a.albedo_region[3], nullptr, a.albedo_h, a.albedo_filter);
        ay.i0 = __builtin_amdgcn_readfirstlane(ay.i0); ay.i1 = __builtin_amdgcn_readfirstlane(ay.i1);
    }
    const size_t dst_row = (size_t)py * (size_t)r.width;
    for (int px = span_begin + (int)threadIdx.x; px < span_end; px += kScaledBlock) {
        const AxisTaps lx = scaled_axis(px, a.quad[0], a.quad[2], a.lightmap_region[0], a.lightmap_region[2], &a.uv_offset[0], a.src_w, a.lightmap_filter);
        const TexelTaps lt = load_taps(r.src, r.src_format, a.src_w, a.lightmap_filter, lx, ly);
        float4 albedo = mk4(0.0f, 0.0f, 0.0f, 0.0f);
        if (with_albedo) {
            const AxisTaps ax = scaled_axis(px, a.quad[0], a.quad[2], a.albedo_region[0], a.albedo_region[2], nullptr, a.albedo_w, a.albedo_filter);
            const TexelTaps at = load_taps(r.albedo, r.albedo_format, a.albedo_w, a.albedo_filter, ax, ay);
            albedo = filter_taps(at, a.albedo_filter, ax.f, ay.f);
        }
        const float4 light = filter_taps(lt, a.lightmap_filter, lx.f, ly.f);
        store_lightmap_texel(r.dst, r.dst_format, dst_row + (size_t)px, resolve_texel(r, light, albedo));
    }
}

hipError_t launch_resolve_scaled(const ResolveScaledLaunch& a, hipStream_t stream) {
    if (a.x0 >= a.x1 || a.y0 >= a.y1) return hipSuccess;
    const dim3 grid((unsigned)((a.x1 - a.x0 + kScaledSpan - 1) / kScaledSpan), (unsigned)(a.y1 - a.y0));
    hipLaunchKernelGGL(resolve_scaled_kernel, grid, dim3(kScaledBlock), 0, stream, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// LUT-blended resolve (ilm_resolve_lighting_lut): LUTBlendedResolveWithAlbedoCommon, Illuminant/Shaders/LUTResolve.fx:61-115
// ---------------------------------------------------------------------------------------------
// One channel of ReadLUT's lattice fetch as the header defines it: a is saturated (a NaN became 0), so s lies in [0, n - 1], the conversion
// is exact and both indices are inside the slice / the LUT row by integer arithmetic.
ILM_DEV AxisTaps lut_axis(float a, int n) {
    const float s = a * (float)(n - 1), fl = floorf(s);
    AxisTaps t;
    t.f = s - fl;
    t.i0 = min((int)fl, n - 1);
    t.i1 = min(t.i0 + 1, n - 1);
    return t;
}

// The eight lattice points round one colour, t[ri + 2 gi + 4 bi]: column bi * n + ri, texel row row0 + gi.
struct LutTaps { float4 t[8]; };

ILM_DEV LutTaps load_lut(const ResolveLutTexture& l, const AxisTaps& r, const AxisTaps& g, const AxisTaps& b) {
    const size_t g0 = (size_t)(l.row0 + g.i0) * (size_t)l.pitch, g1 = (size_t)(l.row0 + g.i1) * (size_t)l.pitch;
    const size_t c00 = (size_t)(b.i0 * l.n + r.i0), c10 = (size_t)(b.i0 * l.n + r.i1);
    const size_t c01 = (size_t)(b.i1 * l.n + r.i0), c11 = (size_t)(b.i1 * l.n + r.i1);
    LutTaps v;
    v.t[0] = load_tap(l.texels, l.format, g0 + c00); v.t[1] = load_tap(l.texels, l.format, g0 + c10);
    v.t[2] = load_tap(l.texels, l.format, g1 + c00); v.t[3] = load_tap(l.texels, l.format, g1 + c10);
    v.t[4] = load_tap(l.texels, l.format, g0 + c01); v.t[5] = load_tap(l.texels, l.format, g0 + c11);
    v.t[6] = load_tap(l.texels, l.format, g1 + c01); v.t[7] = load_tap(l.texels, l.format, g1 + c11);
    return v;
}

ILM_DEV f3 blend_lut(const LutTaps& v, float fr, float fg, float fb) {
    return xyz(lerp4(lerp4(lerp4(v.t[0], v.t[1], fr), lerp4(v.t[2], v.t[3], fr), fg),
                     lerp4(lerp4(v.t[4], v.t[5], fr), lerp4(v.t[6], v.t[7], fr), fg), fb));
}

// The shape of resolve_scaled_kernel (a span of one row per block, the row's taps wave-uniform), a kernel of its own so that that one keeps
// its instruction stream.  Per pixel: four lightmap taps and four albedo taps, then -- once the albedo is known -- the sixteen LUT taps,
// all issued before the first of their lerps; the light's filter and the weight are computed while they are in flight.  The two LUTs (19.6 KB
// each at 17^3 RGBA8) are read through the caches: every wave of the frame reads the same few kilobytes.  Band, normalize, ramp, LUTOnly
// and the formats are launch-uniform branches.  docs/experiments.md ("LUT-blended resolve") has the registers and the measurement.
__global__ __launch_bounds__(kScaledBlock, 4) void resolve_lut_kernel(const ResolveLutLaunch a) {
    const ResolveScaledLaunch& s = a.s;
    const ResolveLaunch& r = s.r;
    const int py = s.y0 + (int)blockIdx.y;
    const int span_begin = s.x0 + (int)blockIdx.x * kScaledSpan;
    const int span_end = min(span_begin + kScaledSpan, s.x1);
    AxisTaps ly = scaled_axis(py, s.quad[1], s.quad[3], s.lightmap_region[1], s.lightmap_region[3], &s.uv_offset[1], s.src_h, s.lightmap_filter);
    ly.i0 = __builtin_amdgcn_readfirstlane(ly.i0); ly.i1 = __builtin_amdgcn_readfirstlane(ly.i1);
    AxisTaps ay = scaled_axis(py, s.quad[1], s.quad[3], s.albedo_region[1], s.albedo_region[3], nullptr, s.albedo_h, s.albedo_filter);
    ay.i0 = __builtin_amdgcn_readfirstlane(ay.i0); ay.i1 = __builtin_amdgcn_readfirstlane(ay.i1);
    const size_t dst_row = (size_t)py * (size_t)r.width;
    const float k = r.inverse_scale * 2.0f;
    const float e = r.exposure_minus_one + 1.0f, gm = r.gamma_minus_one + 1.0f;
    for (int px = span_begin + (int)threadIdx.x; px < span_end; px += kScaledBlock) {
        const AxisTaps lx = scaled_axis(px, s.quad[0], s.quad[2], s.lightmap_region[0], s.lightmap_region[2], &s.uv_offset[0], s.src_w, s.lightmap_filter);
        const TexelTaps lt = load_taps(r.src, r.src_format, s.src_w, s.lightmap_filter, lx, ly);
        const AxisTaps ax = scaled_axis(px, s.quad[0], s.quad[2], s.albedo_region[0], s.albedo_region[2], nullptr, s.albedo_w, s.albedo_filter);
        const TexelTaps at = load_taps(r.albedo, r.albedo_format, s.albedo_w, s.albedo_filter, ax, ay);
        const float4 albedo = filter_taps(at, s.albedo_filter, ax.f, ay.f);
        const f3 c = mk3(sat(albedo.x), sat(albedo.y), sat(albedo.z));             // saturate3(albedo.rgb), :87
        const AxisTaps dr = lut_axis(c.x, a.dark.n), dg = lut_axis(c.y, a.dark.n), db = lut_axis(c.z, a.dark.n);
        const AxisTaps br = lut_axis(c.x, a.bright.n), bg = lut_axis(c.y, a.bright.n), bb = lut_axis(c.z, a.bright.n);
        const LutTaps dt = load_lut(a.dark, dr, dg, db), bt = load_lut(a.bright, br, bg, bb);
        const float4 tap = filter_taps(lt, s.lightmap_filter, lx.f, ly.f);
        const f3 light = mk3(tap.x * k, tap.y * k, tap.z * k);                      // light *= InverseScaleFactor * 2, :75
        f3 w = light;
        if (a.normalize) w.x = w.y = w.z = (light.x * 0.299f + light.y * 0.587f) + light.z * 0.144f;     // RgbToGray, :16,82-85
        const f3 dark = blend_lut(dt, dr.f, dg.f, db.f), bright = blend_lut(bt, br.f, bg.f, bb.f);
        f3 blended;
        if (a.has_band) {
            // :93-98
            const float v = w.x - a.dark_level, v3 = (v - a.transition) - a.neutral;
            const float t1 = sat(v * a.inv_transition), t2 = sat(v3 * a.inv_transition);
            blended = mk3(lerp(lerp(dark.x, c.x, t1), bright.x, t2), lerp(lerp(dark.y, c.y, t1), bright.y, t2), lerp(lerp(dark.z, c.z, t1), bright.z, t2));
        } else {
            // :100-110
            if (a.ramp) w = mk3(sat(fmaxf(0.0f, w.x - a.dark_level) * a.inv_range), sat(fmaxf(0.0f, w.y - a.dark_level) * a.inv_range),
                                sat(fmaxf(0.0f, w.z - a.dark_level) * a.inv_range));
            else        w = mk3(sat(w.x - a.dark_level), sat(w.y - a.dark_level), sat(w.z - a.dark_level));
            blended = mk3(lerp(dark.x, bright.x, w.x), lerp(dark.y, bright.y, w.y), lerp(dark.z, bright.z, w.z));
        }
        if (!a.lut_only) blended = mk3(blended.x * light.x, blended.y * light.y, blended.z * light.z);     // :113
        // LUTBlendedLightingResolveWithAlbedoPixelShader, :129-131: resolve_texel's plain epilogue
        const float4 out = mk4(pow_pos(fmaxf(0.0f, blended.x + r.offset) * e, gm), pow_pos(fmaxf(0.0f, blended.y + r.offset) * e, gm),
                               pow_pos(fmaxf(0.0f, blended.z + r.offset) * e, gm), albedo.w);
        store_lightmap_texel(r.dst, r.dst_format, dst_row + (size_t)px, out);
    }
}

hipError_t launch_resolve_lut(const ResolveLutLaunch& a, hipStream_t stream) {
    if (a.s.x0 >= a.s.x1 || a.s.y0 >= a.s.y1) return hipSuccess;
    const dim3 grid((unsigned)((a.s.x1 - a.s.x0 + kScaledSpan - 1) / kScaledSpan), (unsigned)(a.s.y1 - a.s.y0));
    hipLaunchKernelGGL(resolve_lut_kernel, grid, dim3(kScaledBlock), 0, stream, a);
    return hipGetLastError();
}

// Sixteen bytes written by the DEVICE at `where` (group.hip, prove_ipc_mappings: the proof goes through the same kind of access the
// store mode's mirror stores use -- a kernel's store through the mapping -- not through a copy engine).
__global__ void stamp16_kernel(uint4* where, uint4 stamp) { *where = stamp; }

hipError_t launch_stamp16(void* where, const uint32_t stamp[4], hipStream_t stream) {
    hipLaunchKernelGGL(stamp16_kernel, dim3(1), dim3(1), 0, stream, static_cast<uint4*>(where), make_uint4(stamp[0], stamp[1], stamp[2], stamp[3]));
    return hipGetLastError();
}

}  // namespace ilm
