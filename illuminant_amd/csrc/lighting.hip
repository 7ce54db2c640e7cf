// lighting.hip -- LightingRenderer sphere-light pass (SDF cone trace) for gfx950.
//
// The reference draws one instanced quad per light and lets the ROP add the
// results (Illuminant/Lighting/LightingRenderer.cs:1004-1169, technique
// SphereLight in Illuminant/Shaders/SphereLight.fx:7-46): every light re-reads
// the G-buffer and rounds through the lightmap format.  Here a 16x16 pixel tile
// is one workgroup: wave 0 bins the lights whose raster footprint touches the
// tile into an LDS list (wave64 ballot + popcount, light order preserved), then
// every thread decodes its G-buffer texel once and walks the list, accumulating
// in fp32 registers and storing the lightmap texel once.  The sum runs over eight
// index-defined parts of the light list combined as a tree, so that several
// workgroups can share a tile without changing a bit (r04: "the order of the sum"
// in sphere_lights_kernel; short launches end tapered, api.hip plan_light_split).
//
// Per-light constants (footprint rectangles, cone config, premultiplied colour)
// are prepared once per call by prepare_lights_kernel and fetched through the
// scalar cache (the list index is wave-uniform), so they cost no VGPRs.
// The cone trace is a chain of dependent SDF fetches: latency-bound, served by
// L1/L2/MALL (the 25 MB atlas is cache resident); no MFMA (no dense contraction).
#include "internal.hpp"

namespace ilm {

struct LightRec {
    float cx, cy, cz, radius;
    float ramp, falloff_mode, casts_shadows, ao_radius;
    float falloff_y, ao_opacity, shadow_filter, spec_power;
    float col_r, col_g, col_b, flags;           // Color1.rgb * Color1.a; kLightHasSpecular | kLightFastTrace | kLightFastDivide (as a float)
    float spec_r, spec_g, spec_b, ramp_rcp;     // refined_rcp(ramp) for the distance ramp's division when kLightFastDivide
    float fx0, fx1, fx2, fx3;                   // raster footprint (screen px), see light_covers
    float fy0, fy1, fy2, fy3;
    float cfg_x, cfg_y, ramp_offset, ramp_rate; // createTraceConfig: maxRadius, radiusGrowthPerPixel; EvenMoreLightProperties.zw
};
static_assert(sizeof(LightRec) == 128, "LightRec is one 128-byte record");
constexpr int kLightHasSpecular = 1;    // Color2.rgb != 0
constexpr int kLightFastTrace = 2;      // light + field admit the in-volume trace loop (uniform half of shade_light's test; see light_flags)
constexpr int kLightFastDivide = 4;     // radius and ramp lie in the operand range of the unscaled division

// What the in-volume trace loop asks of a light and the field, decided once per light (prepare kernels): the centre inside the table
// sampler's box with the margin for rounding, a cone radius of ordinary size, a sane encoded distance, a trace that does not
// overshoot the light (radius >= 0), a step budget the uniform counter can count.
ILM_DEV int light_flags(const LightRec& r, const TraceGate& g) {
    int f = 0;
    if ((r.spec_r != 0.0f) || (r.spec_g != 0.0f) || (r.spec_b != 0.0f)) f |= kLightHasSpecular;
    const bool inside = (r.cx >= g.x0) & (r.cx <= g.x1) & (r.cy >= g.y0) & (r.cy <= g.y1) & (r.cz >= g.z0) & (r.cz <= g.z1);
    if (inside && (g.field_ok != 0.0f) && (r.cfg_x >= 0x1p-60f) && (r.cfg_x <= 0x1p60f) && (r.radius >= 0.0f)) f |= kLightFastTrace;
    if ((r.ramp >= 0x1p-60f) && (r.ramp <= 0x1p60f) && (fabsf(r.radius) <= 0x1p59f)) f |= kLightFastDivide;
    return f;
}

// SphereLightVertexShader (SphereLightCore.fxh:13-56) over the 12-vertex cut-corner
// quad (FillSphereBuffer, LightingRenderer.cs:636-656) + createTraceConfig (ConeTrace.fxh:128-146)
__global__ __launch_bounds__(64) void prepare_lights_kernel(const IlmLightVertex* __restrict__ lights, int count, IlmEnvironment env,
                                                             float max_cone_radius, TraceGate gate, LightRec* __restrict__ out) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= count) return;
    const IlmLightVertex L = lights[i];
    LightRec r;
    r.cx = L.LightPosition1.x; r.cy = L.LightPosition1.y; r.cz = L.LightPosition1.z;
    r.radius = L.LightProperties.x; r.ramp = L.LightProperties.y; r.falloff_mode = L.LightProperties.z; r.casts_shadows = L.LightProperties.w;
    r.ao_radius = L.MoreLightProperties.x; r.falloff_y = L.MoreLightProperties.z; r.ao_opacity = L.MoreLightProperties.w;
    r.shadow_filter = L.EvenMoreLightProperties.x;
    r.col_r = L.Color1.x * L.Color1.w; r.col_g = L.Color1.y * L.Color1.w; r.col_b = L.Color1.z * L.Color1.w;
    r.spec_r = L.Color2.x; r.spec_g = L.Color2.y; r.spec_b = L.Color2.z; r.spec_power = L.Color2.w;

    const float cOne = 1.0f / 7.0f, mOne = 6.0f / 7.0f;
    const float radius = L.LightProperties.x + L.LightProperties.y + 1.0f;
    const float delta_y = radius - (radius / L.MoreLightProperties.z);
    const float rx = radius, ry = radius - (delta_y / 2.0f);
    const float tlx = r.cx - rx, tly = r.cy - ry, brx = r.cx + rx, bry = r.cy + ry;
    const float off = radius * env.ZToY.y + r.cz * env.ZToY.x;
    const float sx = env.GBufferTexelSizeAndMisc.z * env.ZAndScale.z, sy = env.GBufferTexelSizeAndMisc.w * env.ZAndScale.w;
    r.fx0 = (lerp(tlx, brx, 0.0f) - env.ViewportPosition[0]) * sx;
    r.fx1 = (lerp(tlx, brx, cOne) - env.ViewportPosition[0]) * sx;
    r.fx2 = (lerp(tlx, brx, mOne) - env.ViewportPosition[0]) * sx;
    r.fx3 = (lerp(tlx, brx, 1.0f) - env.ViewportPosition[0]) * sx;
    r.fy0 = ((lerp(tly, bry, 0.0f) - off) - env.ViewportPosition[1]) * sy;
    r.fy1 = ((lerp(tly, bry, cOne) - off) - env.ViewportPosition[1]) * sy;
    r.fy2 = ((lerp(tly, bry, mOne) - 0.0f) - env.ViewportPosition[1]) * sy;
    r.fy3 = ((lerp(tly, bry, 1.0f) - 0.0f) - env.ViewportPosition[1]) * sy;

    const float max_radius = clampf(r.radius, ref::kMinConeRadius, max_cone_radius);
    r.cfg_x = max_radius;
    r.cfg_y = max_radius / fmaxf(r.ramp, 16.0f) * 1.0f;  // getConeGrowthFactor() == 1 (DistanceFieldCommon.fxh:233-236)
    r.ramp_offset = L.EvenMoreLightProperties.z; r.ramp_rate = L.EvenMoreLightProperties.w;
    const int flags = light_flags(r, gate);
    r.flags = (float)flags;
    r.ramp_rcp = (flags & kLightFastDivide) ? refined_rcp(r.ramp) : 0.0f;
    out[i] = r;
}

// decodeNormalSpherical, EnvironmentCommon.fxh:40-51
ILM_DEV f3 decode_normal(float ex, float ey) {
    const float ax = ex * 2.0f - 1.0f, ay = ey * 2.0f - 1.0f;
    const float s = sinf(ax * kPi), c = cosf(ax * kPi);
    const float phx = sqrtf(1.0f - ay * ay);
    return mk3(c * phx, s * phx, ay);
}

struct Pixel {
    f3 shaded, normal;
    // the camera position (sampleGBuffer's third output, read by the specular term alone) is a function of the pixel's coordinates:
    // not kept per lane -- the pixel of lane l is (origin_x + (l & 7), origin_y + (l >> 3)), and shade_light forms it where a light has a
    // specular colour (the same operations on the same values)
    int origin_x, origin_y;
    bool enable_shadows, fullbright;
    // light-independent half of the in-volume trace test: the trace start (shaded + normal * SELF_OCCLUSION_HACK) lies in the table
    // sampler's box with the start-side margin (set by trace_start_inside once per pixel)
    bool start_inside;
};

// Samples lie on the segment start -> light centre, or (trace shorter than the minimum length 1) within 1 of start: the start must
// keep 1 + the rounding margin from the box faces, the light centre (TraceGate, per light) the rounding margin alone.
ILM_DEV bool trace_start_inside(const Pixel& P, const IlmDistanceFieldUniforms& df, const SdfView& sdf) {
    const f3 start = P.shaded + (P.normal * ref::kSelfOcclusionHack);
    const float mx = 1.0625f + df.Extent.x * 0x1p-16f, my = 1.0625f + df.Extent.y * 0x1p-16f, mz = 1.0625f + df.Extent.z * 0x1p-16f;
    return (start.x >= sdf.box_x0 + mx) & (start.x <= sdf.box_x1 - mx) & (start.y >= sdf.box_y0 + my) & (start.y <= sdf.box_y1 - my) &
           (start.z >= sdf.box_z0 + mz) & (start.z <= sdf.box_z1 - mz);
}

// sampleGBuffer, LightCommon.fxh:58-144
ILM_DEV Pixel sample_gbuffer(float spx, float spy, const IlmEnvironment& env, const GBufferView& g) {
    Pixel p;
    p.enable_shadows = true;
    p.fullbright = false;
    const float vsx = env.GBufferTexelSizeAndMisc.z, vsy = env.GBufferTexelSizeAndMisc.w;
    const float rsx = env.ZAndScale.z, rsy = env.ZAndScale.w;
    if (g.texels != nullptr && ((env.GBufferTexelSizeAndMisc.x != 0.0f) || (env.GBufferTexelSizeAndMisc.y != 0.0f))) {
        float sx = spx, sy = spy;
        if (env.GBufferViewportRelative != 0.0f) {
            sx /= vsx; sy /= vsy;
            sx += env.ViewportPosition[0]; sy += env.ViewportPosition[1];
        }
        const float u = (sx + 0.5f) * env.GBufferTexelSizeAndMisc.x;
        const float v = (sy + 0.5f) * env.GBufferTexelSizeAndMisc.y;
        const int tx = clamp_tap(floorf(u * (float)g.width), g.width);
        const int ty = clamp_tap(floorf(v * (float)g.height), g.height);
        float4 s;
        if (g.format == ILM_GBUFFER_HALF4) {
            const uint2 raw = reinterpret_cast<const uint2*>(g.texels)[(size_t)ty * (size_t)g.width + (size_t)tx];
            s = mk4(__half2float(__ushort_as_half((unsigned short)(raw.x & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(raw.x >> 16))),
                    __half2float(__ushort_as_half((unsigned short)(raw.y & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(raw.y >> 16))));
        } else {
            s = reinterpret_cast<const float4*>(g.texels)[(size_t)ty * (size_t)g.width + (size_t)tx];
        }
        const float relative_y = s.z;
        float world_z = s.w;
        if (world_z < 0.0f) {
            world_z += 1.0f;
            world_z = -world_z;
            p.enable_shadows = false;
        } else if (world_z >= 9999.0f) {
            world_z = 0.0f;
            p.enable_shadows = false;
            p.fullbright = true;
        }
        world_z *= ref::kGBufferZScale;
        world_z -= ref::kGBufferZOffset;
        spx /= rsx; spy /= rsy;
        p.shaded = mk3((spx + 0.0f) / vsx + env.ViewportPosition[0], (spy + relative_y) / vsy + env.ViewportPosition[1], world_z);
        if ((s.x != 0.0f) || (s.y != 0.0f))
            p.normal = decode_normal(s.x, s.y);
        else
            p.normal = mk3(0.0f, 0.0f, 0.0f);
    } else {
        spx /= rsx; spy /= rsy;
        p.shaded = mk3(spx / vsx + env.ViewportPosition[0], spy / vsy + env.ViewportPosition[1], env.ZAndScale.x);
        p.normal = mk3(0.0f, 0.0f, 1.0f);
    }
    return p;
}

// computeSphereLightOpacity + computeNormalFactor, LightCommon.fxh:154-214.
// SHARED: every divisor of this function lies in the operand range of the unscaled division (the caller's wave-uniform test):
// the three divisions by `distance` share one refined reciprocal, the division by the light's ramp uses the one its record carries,
// the division by DOT_RAMP_RANGE the constant's -- the same correctly rounded quotients as `/` (tests: ilm_debug_divide,
// ilm_debug_divide_by_constant over all 2^32 numerators), 9 + 9 + 6 + 6 instructions instead of five 12-instruction sequences.
constexpr float kDotRampRangeRcp = (float)(1.0 / (double)ref::kDotRampRange);
constexpr float kVisibilityRange = ref::kUnshadowedThreshold - ref::kFullyShadowedThreshold;
constexpr float kVisibilityRangeRcp = (float)(1.0 / (double)kVisibilityRange);
// FLAT (with SHARED only): every lane's normal has x = y = 0 (the ground plane, flat G-buffer texels; the caller's wave-uniform test).
// dot(-lightNormal, normal) is then ((-ln.x * 0) + (-ln.y * 0)) + (-ln.z * normal.z) = -ln.z * normal.z exactly -- the two vanishing
// products are signed zeros (all components are finite: SHARED's range test bounds `distance`, hence d3), and a zero added to the third
// product leaves it unchanged (the sign of a zero RESULT may differ, which the following + DOT_OFFSET erases) -- so the x and y
// components of lightNormal, two 6-instruction divisions, are never formed.
template <bool SHARED, bool FLAT = false>
ILM_DEV float sphere_light_opacity(f3 d3, float distance, f3 normal, const LightRec& L, float light_occlusion) {
    const float over = distance - L.radius;
    float distance_factor = 1.0f - sat(SHARED ? div_with_rcp(over, L.ramp, L.ramp_rcp) : (over / L.ramp));
    if (light_occlusion > 0.0f)
        distance_factor *= 1.0f - sat(d3.z / light_occlusion);
    float normal_factor = 1.0f;
    if ((normal.x != 0.0f) || (normal.y != 0.0f) || (normal.z != 0.0f)) {
        float d;
        if (SHARED && FLAT) {
            const float y = refined_rcp(distance);
            d = (div_with_rcp(d3.z, distance, y) * -1.0f) * normal.z;
        } else {
            f3 ln;
            if (SHARED) {
                const float y = refined_rcp(distance);
                ln = mk3(div_with_rcp(d3.x, distance, y), div_with_rcp(d3.y, distance, y), div_with_rcp(d3.z, distance, y));
            } else {
                ln = mk3(d3.x / distance, d3.y / distance, d3.z / distance);
            }
            d = dot3(ln * -1.0f, normal);
        }
        const float ramped = SHARED ? div_with_rcp(d + ref::kDotOffset, ref::kDotRampRange, kDotRampRangeRcp) : ((d + ref::kDotOffset) / ref::kDotRampRange);
        normal_factor = pow_pos(sat(ramped), ref::kDotExponent);
    }
    if (L.falloff_mode >= 2.0f) {
        distance_factor = 1.0f - sat(distance - L.radius);
        normal_factor = 1.0f;
    } else if (L.falloff_mode >= 1.0f) {
        distance_factor *= distance_factor;
    }
    return sat((normal_factor * distance_factor) + sat(L.radius - distance));
}

struct LightStats { unsigned long long samples = 0, pairs = 0, traced = 0; };

// The partial sums of a light split travel between workgroups (any XCD) as device-scope accesses: `sc1` stores are written through the
// XCD's L2, `sc1` loads are served past the CU's L1 -- valid without cache write-backs or invalidates when BOTH sides use them
// (MI355X_MICROARCH.md, "inter-workgroup visibility") -- as ONE 16-byte access per lane (a dword `sc1` store is a fabric write of its
// own, ~6 x the time per byte).  Written as instructions: the compiler has no 16-byte device-scope access to offer.  The store is not
// waited for here (the caller's `s_waitcnt vmcnt(0)` before the ticket is); the loads of a tile's sums are issued together and waited for.
ILM_DEV void store_partial(float4* where, float r, float g, float b, float a) {
    const f32x4 v = { r, g, b, a };
    asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(where), "v"(v) : "memory");
}
// K = 2 or 4 partial sums `stride` float4 apart, all requested before the first is waited for (for callers with registers to spare)
template <int K>
ILM_DEV void load_partials(const float4* first, size_t stride, float4 (&out)[K]) {
    f32x4 v[K];
    if constexpr (K == 2) {
        asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %3, off sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(v[0]), "=&v"(v[1]) : "v"(first), "v"(first + stride) : "memory");
    } else if constexpr (K == 4) {
        asm volatile("global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %5, off sc1\n\tglobal_load_dwordx4 %2, %6, off sc1\n\t"
                     "global_load_dwordx4 %3, %7, off sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
                     : "v"(first), "v"(first + stride), "v"(first + 2 * stride), "v"(first + 3 * stride) : "memory");
    }
#pragma unroll
    for (int i = 0; i < K; i++) out[i] = mk4(v[i].x, v[i].y, v[i].z, v[i].w);
}
// the sums of a tile's K = 2, 4 or 8 members, `stride` float4 apart, combined as the upper levels of the tree over the parts:
// ((m0 + m1) + (m2 + m3)) + ((m4 + m5) + (m6 + m7)), left operand first as in close_part
ILM_DEV float4 combine_partials(const float4* first, size_t stride, int count) {
    auto add4 = [](const float4& l, const float4& r) { return mk4(l.x + r.x, l.y + r.y, l.z + r.z, l.w + r.w); };
    if (count == 2) { float4 m[2]; load_partials<2>(first, stride, m); return add4(m[0], m[1]); }
    if (count == 4) { float4 m[4]; load_partials<4>(first, stride, m); return add4(add4(m[0], m[1]), add4(m[2], m[3])); }
    // (eight: two requests of four -- 32 registers of sums at once push the kernel's allocation into scratch)
    float4 m[4], n[4];
    load_partials<4>(first, stride, m);
    const float4 lower = add4(add4(m[0], m[1]), add4(m[2], m[3]));
    load_partials<4>(first + 4 * stride, stride, n);
    return add4(lower, add4(add4(n[0], n[1]), add4(n[2], n[3])));
}
// What a trace needs besides the light: the field (general sampler) and, for the in-volume loop, its uniform constants and the
// workgroup's slice table in LDS (table == nullptr: no in-volume loop -- light probes, fields the table cannot describe)
struct TraceField {
    const IlmDistanceFieldUniforms& df;
    const TraceSdfView& sdf;
    const InsideConsts& inside;
    const SliceEntry* table;
};

// The cone-trace loop (coneTraceAdvance + coneTraceStep, ConeTrace.fxh:52-85).  FAST: every sample of every active lane lies inside the
// box of the field's in-volume sampler and the light's cone radius is of ordinary size (shade_light decides per wave): the table
// sampler, division without the range scaling, the step budget as a uniform counter.
template <int FMT, bool STATS, bool FAST>
ILM_DEV void cone_trace_loop(const f3& start, const f3& dir, float data_y, float cfg_z, float cone_growth, float cone_max_radius,
                             const TraceField& F, float& data_x, float& data_z, float& steps_remaining, bool alive, LightStats& st) {
    // liveness = stepsRemaining * (saturate(visibility - FULLY_SHADOWED) * saturate(length - position)) > 0 is, factor by factor,
    // stepsRemaining > 0 && visibility > FULLY_SHADOWED && length > position: the smallest positive factors (ulp(0.075), ulp(0.5),
    // 1) cannot underflow their product, and a NaN factor saturates to 0 and fails its compare alike.
    const float long_step = F.df.StepAndMisc2.z;
    if (FAST) {
        // Every lane enters with the same budget S (a uniform) and loses 1 per iteration: after k iterations a lane that is still
        // in the loop holds S - k, exactly (S < 2^24: subtracting 1 from a positive float towards zero is exact, and the last step,
        // which may cross zero, rounds once either way).  So `stepsRemaining > 0` is the scalar test k < S, and a lane's budget at its
        // exit is S - (iterations it ran).
        const float budget = steps_remaining;
        const int most = (int)ceilf(budget);          // iterations k = 1 .. with S - k > 0 beforehand: k < S
        int k = 0;
        float ran = 0.0f;
        constexpr float kVisibilityGuard = 1.00000095367431640625f;      // 1 + 2^-20
        float guard_z = data_z * kVisibilityGuard;
        bool lit = data_z > ref::kFullyShadowedThreshold;
        while (alive) {
            k++;
            ran = (float)k;
            const f3 sp = mk3(__builtin_fmaf(dir.x, data_x, start.x), __builtin_fmaf(dir.y, data_x, start.y), __builtin_fmaf(dir.z, data_x, start.z));
            const float s = sample_inside_table<FMT>(sp, F.inside, F.sdf, F.table);
            if (STATS) st.samples++;
            const float local_radius = __builtin_elementwise_minimum(__builtin_fmaf(cone_growth, data_x, ref::kMinConeRadius), cone_max_radius);
            // visibility = min(visibility, n / r) with n = distance + HACK_DISTANCE_OFFSET (coneTraceStep, ConeTrace.fxh:62-63).  The quotient
            // only matters when it is below the running minimum v, and away from obstacles it never is.  With g = fl(v (1 + 2^-20)), kept
            // beside v: n >= fl(g r) implies n / r > v (the two roundings lose at most 2^-23 relative, r > 0, v > FULLY_SHADOWED_THRESHOLD
            // while the lane is alive), hence RN(n / r) >= v and the minimum keeps v -- exactly.  When NO lane of the wave can lower its
            // visibility the 11-instruction division is skipped (a multiply and a compare decide); a NaN fails the test and takes the
            // division like everything else.  cfg5 10.65 -> 10.01 ms; cfg3 (four times the obstacle density, 2 x 2 texels per wave) unchanged.
            const float n = s + ref::kHackDistanceOffset;
            if (__builtin_amdgcn_ballot_w64(!(n >= guard_z * local_radius)) != 0ull) {
                const float local_visibility = div_no_scale(n, local_radius);
                asm("v_min_f32 %0, %0, %1" : "+v"(data_z) : "v"(local_visibility));
                guard_z = data_z * kVisibilityGuard;
                lit = data_z > ref::kFullyShadowedThreshold;       // (visibility changes here and nowhere else)
            }
            float step = fabsf(s) * long_step;
            asm("v_max_f32 %0, %0, %1" : "+v"(step) : "v"(cfg_z));
            data_x += step;
            alive = (k < most) & lit & (data_y > data_x);
        }
        steps_remaining = budget - ran;
        return;
    }
    while (alive) {
        steps_remaining -= 1.0f;
        const f3 sp = mk3(__builtin_fmaf(dir.x, data_x, start.x), __builtin_fmaf(dir.y, data_x, start.y), __builtin_fmaf(dir.z, data_x, start.z));
        const float s = sample_distance_field<FMT, false>(sp, F.df, F.sdf);
        if (STATS) st.samples++;
        // (both operands are finite: v_minimum3_f32 needs no canonicalising v_max in front of it, unlike IEEE minNum)
        const float local_radius = __builtin_elementwise_minimum(__builtin_fmaf(cone_growth, data_x, ref::kMinConeRadius), cone_max_radius);
        // (the same exact skip of the division as in the in-volume loop; a cone radius that is not positive -- the general path admits
        // any light -- always divides)
        const float n = s + ref::kHackDistanceOffset;
        if (__builtin_amdgcn_ballot_w64(!((n >= (data_z * 1.00000095367431640625f) * local_radius) & (local_radius > 0.0f) & (data_z > 0.0f))) != 0ull) {
            const float local_visibility = n / local_radius;
            // fminf / fmaxf as the bare instructions: the same minNum / maxNum result without the v_max x, x canonicalisation the
            // compiler puts in front of each loop-carried operand (no signalling NaN can reach them)
            asm("v_min_f32 %0, %0, %1" : "+v"(data_z) : "v"(local_visibility));
        }
        float step = fabsf(s) * long_step;
        asm("v_max_f32 %0, %0, %1" : "+v"(step) : "v"(cfg_z));
        data_x += step;
        alive = (steps_remaining > 0.0f) & (data_z > ref::kFullyShadowedThreshold) & (data_y > data_x);
    }
}

// One light on one shaded point: SphereLightPixelShader (SphereLight.fx:7-46) after the raster test.  Returns false when the shader
// discards (nothing is blended); otherwise the light's rgb contribution in (out_r, out_g, out_b).
// flat_normals: wave-uniform, every lane's normal has x = y = 0 (see sphere_light_opacity)
template <int FMT, bool STATS>
ILM_DEV bool shade_light(const Pixel& P, const LightRec& L, const IlmEnvironment& env, const TraceField& F,
                         bool have_sdf, const RampView& ramp, LightStats& st, float& out_r, float& out_g, float& out_b, bool flat_normals = false) {
    const IlmDistanceFieldUniforms& df = F.df;
    const SdfView& sdf = F.sdf;
    // checkShadowFilter, LightCommon.fxh:146-152
    const bool filtered = (L.shadow_filter < 0.0f) ? false : ((L.shadow_filter > 0.5f) != P.enable_shadows);
    if (P.fullbright || filtered)
        return false;

    const float casts = L.casts_shadows * (P.enable_shadows ? 1.0f : 0.0f);
    const int light_flags_i = (int)L.flags;
    f3 d3 = P.shaded - mk3(L.cx, L.cy, L.cz);
    d3.y *= L.falloff_y;
    const float distance = len3(d3);
    // the shared-reciprocal divisions need distance (a divisor, and with the radius the ramp's numerator) inside their operand range:
    // one wave-uniform test, the IEEE form otherwise
    const bool divisors_ordinary = (distance >= 0x1p-60f) & (distance <= 0x1p59f);
    const bool shared = (light_flags_i & kLightFastDivide) && __builtin_amdgcn_ballot_w64(!divisors_ordinary) == 0ull;
    const float distance_opacity = shared ? (flat_normals ? sphere_light_opacity<true, true>(d3, distance, P.normal, L, env.ZToY.z)
                                                          : sphere_light_opacity<true>(d3, distance, P.normal, L, env.ZToY.z))
                                          : sphere_light_opacity<false>(d3, distance, P.normal, L, env.ZToY.z);
    const bool visible = (distance_opacity > 0.0f) && (P.shaded.x > -9999.0f);
    if (!visible)
        return false;

    // computeAO, AOCommon.fxh:1-19 (aoRadius scaled by max(0, normal.z), SphereLightCore.fxh:78)
    float ao_opacity = 1.0f;
    const float ao_radius = L.ao_radius * fmaxf(0.0f, P.normal.z);
    if ((ao_radius >= 0.5f) && have_sdf) {
        const float distance = sample_distance_field<FMT>(mk3(P.shaded.x, P.shaded.y, P.shaded.z + P.normal.z * ao_radius), df, sdf);
        if (STATS) st.samples++;
        float r = 1.0f - sat(clampf(distance, 0.0f, ao_radius) / ao_radius);
        r *= r;
        r = 1.0f - r;
        ao_opacity = (1.0f - L.ao_opacity) + (r * L.ao_opacity);
    }
    const float pre_trace = distance_opacity * ao_opacity;

    // coneTrace, ConeTrace.fxh:148-191
    float cone_opacity = 1.0f;
    const bool trace = (casts != 0.0f) && (pre_trace >= ref::kShadowOpacityThreshold);
    if (trace) {
        if (STATS) st.traced++;
        f3 start = P.shaded + (P.normal * ref::kSelfOcclusionHack);
        const f3 tv = mk3(L.cx, L.cy, L.cz) - start;
        const float trace_length = len3(tv);
        const float data_y = fmaxf(trace_length - L.radius, 1.0f);
        float data_x = ref::kTraceInitialOffsetPx;
        float data_z = 1.0f;
        const float cfg_z = fmaxf(1.0f, df.Packed1.w);
        float steps_remaining = df.StepAndMisc2.x;
        const bool alive = have_sdf;
        // The light's cone configuration is read every iteration; with ~104 SGPRs live the compiler re-loads it from memory inside the
        // loop (s_load + s_waitcnt per sample).  Two VGPRs keep it resident.
        float cone_max_radius = L.cfg_x, cone_growth = L.cfg_y;
        asm volatile("" : "+v"(cone_max_radius), "+v"(cone_growth));
        // In-volume loop when, for every tracing lane of the wave, every sample lies in the box of the table sampler: the light's half of
        // the test was decided when its record was prepared (kLightFastTrace), the pixel's half once per pixel (start_inside); what is
        // left per pair is a trace of ordinary length (a divisor of the unscaled division; > 0 also means a finite direction).
        const bool pair_ok = P.start_inside & (trace_length >= 0x1p-60f);
        if ((F.table != nullptr) && (light_flags_i & kLightFastTrace) && __builtin_amdgcn_ballot_w64(!pair_ok) == 0ull) {
            const float y = refined_rcp(trace_length);
            const f3 dir = mk3(div_with_rcp(tv.x, trace_length, y), div_with_rcp(tv.y, trace_length, y), div_with_rcp(tv.z, trace_length, y));
            cone_trace_loop<FMT, STATS, true>(start, dir, data_y, cfg_z, cone_growth, cone_max_radius, F, data_x, data_z, steps_remaining, alive, st);
        } else {
            f3 dir = mk3(tv.x / trace_length, tv.y / trace_length, tv.z / trace_length);
            // The sampler treats a NaN coordinate as 0.  start + dir * x is NaN for every x exactly when start or dir is (x stays
            // finite), so the test is hoisted: such an axis becomes start = dir = 0 and the loop samples with CHECK_NAN = false.
            if ((start.x != start.x) || (dir.x != dir.x)) { start.x = 0.0f; dir.x = 0.0f; }
            if ((start.y != start.y) || (dir.y != dir.y)) { start.y = 0.0f; dir.y = 0.0f; }
            if ((start.z != start.z) || (dir.z != dir.z)) { start.z = 0.0f; dir.z = 0.0f; }
            cone_trace_loop<FMT, STATS, false>(start, dir, data_y, cfg_z, cone_growth, cone_max_radius, F, data_x, data_z, steps_remaining, alive, st);
        }
        const float visibility = fminf(data_z, steps_remaining / ref::kMaxStepRampWindow);
        // (the numerator is a saturate: always inside the unscaled division's range; the divisor is a constant)
        cone_opacity = pow_pos(sat(div_with_rcp(sat(visibility - ref::kFullyShadowedThreshold), kVisibilityRange, kVisibilityRangeRcp)), df.ConeAndMisc.z);
    }
    // SphereLightPixelEpilogue / ...WithRamp (SphereLightCore.fxh:83-119): with a ramp texture the opacity becomes a colour,
    // SampleFromRamp2(preTraceOpacity, (angle + rampOffset) * rampRate).rgb * coneOpacity -- tex2Dlod level 0, LINEAR, U CLAMP, V WRAP
    float opacity_r = pre_trace * cone_opacity, opacity_g = opacity_r, opacity_b = opacity_r;
    if (ramp.texels != nullptr) {
        const float angle = atan2f(P.shaded.y - L.cy, P.shaded.x - L.cx);
        const float u = pre_trace, v = (angle + L.ramp_offset) * L.ramp_rate;
        const int w = ramp.width, h = ramp.height;
        const float sx = u * (float)w - 0.5f, sy = v * (float)h - 0.5f;
        float x0f = floorf(sx);
        const float y0f = floorf(sy);
        const float fx = sx - x0f, fy = sy - y0f;
        float x1f = x0f + 1.0f;
        x0f = (x0f >= 0.0f) ? x0f : 0.0f; x0f = fminf(x0f, (float)(w - 1));
        x1f = (x1f >= 0.0f) ? x1f : 0.0f; x1f = fminf(x1f, (float)(w - 1));
        // U is clamped in float before the cast (NaN: column 0).  V WRAP is exact for every float; y1 is the integer y0 + 1 wrapped, the
        // tap the sampler takes (y0f + 1.0f would round back onto y0f from 2^24 on).
        const int x0 = (int)x0f, x1 = (int)x1f;
        const int y0 = wrap_index(y0f, h), y1 = (y0 + 1 == h) ? 0 : y0 + 1;
        const float4 t00 = ramp.texels[y0 * w + x0], t10 = ramp.texels[y0 * w + x1], t01 = ramp.texels[y1 * w + x0], t11 = ramp.texels[y1 * w + x1];
        opacity_r = lerp(lerp(t00.x, t10.x, fx), lerp(t01.x, t11.x, fx), fy) * cone_opacity;
        opacity_g = lerp(lerp(t00.y, t10.y, fx), lerp(t01.y, t11.y, fx), fy) * cone_opacity;
        opacity_b = lerp(lerp(t00.z, t10.z, fx), lerp(t01.z, t11.z, fx), fy) * cone_opacity;
    }

    // SphereLightPixelShader epilogue, SphereLight.fx:37-45.  The specular term is
    // skipped when Color2.rgb == 0: it then contributes exactly 0 unless
    // pow() produced inf/NaN (negative SpecularPower), which the reference does not guard.
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    if (light_flags_i & kLightHasSpecular) {
        const f3 light_direction = P.shaded - mk3(L.cx, L.cy, L.cz);
        const int l = (int)(threadIdx.x & 63u);
        const f3 camera = mk3((float)(P.origin_x + (l & 7)) / env.ZAndScale.z, (float)(P.origin_y + (l >> 3)) / env.ZAndScale.w, env.ZAndScale.y + 0.01f);
        const f3 h = norm3(norm3(camera - P.shaded) - light_direction);
        const float specularity = pow_pos(sat(dot3(h, P.normal)), L.spec_power);
        sr = L.spec_r * specularity * opacity_r;
        sg = L.spec_g * specularity * opacity_g;
        sb = L.spec_b * specularity * opacity_b;
    }
    out_r = (L.col_r * opacity_r) + sr;
    out_g = (L.col_g * opacity_g) + sg;
    out_b = (L.col_b * opacity_b) + sb;
    return true;
}

constexpr int kTile = kLightTile;                   // internal.hpp
constexpr int kLightThreads = kLightTileThreads;
constexpr int kListCapacity = 1024;

// ---------------------------------------------------------------------------------------------
// Light blend functions (ilm_ctx_set_light_blend_function; the header has the contract) -- one channel of the BLEND instantiations of
// the light kernels, f the channel's ILM_LIGHT_BLEND_* (wave-uniform: a scalar compare and branch per use).  The additive
// instantiations (BLEND = false) do not call these: their instruction streams are what they were.
// MAX / MIN are comparisons and selects, not fmaxf / fminf: a NaN source is never selected, a NaN base is kept.
// ---------------------------------------------------------------------------------------------
// A BLEND instantiation is named by its field format + kBlendVariant in the kernel's first template argument: the additive
// instantiations keep the names they had (<FMT, STATS[, WIDE_BIN]>: what profiles and tools look kernels up by).
constexpr int kBlendVariant = 2;
static_assert((ILM_SDF_UNORM16 & kBlendVariant) == 0 && (ILM_SDF_FP16 & kBlendVariant) == 0, "the field formats leave the variant bit free");
// what a channel's running value starts from in the fp32 model (a part, a call)
ILM_DEV float blend_identity(int f) {
    return (f == ILM_LIGHT_BLEND_MAX) ? -__builtin_inff() : (f == ILM_LIGHT_BLEND_MIN) ? __builtin_inff() : 0.0f;
}
// a contributing pair's value c -- or a later part's running value -- into the running value (fp32 model); REVERSE_SUBTRACT gathers
// the sum ADD forms
ILM_DEV float blend_gather(int f, float running, float c) {
    if (f == ILM_LIGHT_BLEND_MAX) return (c > running) ? c : running;
    if (f == ILM_LIGHT_BLEND_MIN) return (c < running) ? c : running;
    return running + c;
}
// the call's running value onto the base value (fp32 model): one operation, one rounding
ILM_DEV float blend_onto_base(int f, float base, float running) {
    if (f == ILM_LIGHT_BLEND_MAX) return (running > base) ? running : base;
    if (f == ILM_LIGHT_BLEND_MIN) return (running < base) ? running : base;
    if (f == ILM_LIGHT_BLEND_REVERSE_SUBTRACT) return base - running;
    return base + running;
}
// one pair in the fp16-per-light model: dst (an fp16 value) and s = half(c)
ILM_DEV float blend_half_step(int f, float dst, float c) {
    const float s = __half2float(__float2half_rn(c));
    if (f == ILM_LIGHT_BLEND_MAX) return (s > dst) ? s : dst;
    if (f == ILM_LIGHT_BLEND_MIN) return (s < dst) ? s : dst;
    return __half2float(__float2half_rn((f == ILM_LIGHT_BLEND_REVERSE_SUBTRACT) ? dst - s : dst + s));
}
// the pair (cr, cg, cb, 1) into the four running values of a BLEND instantiation, in the call's model
ILM_DEV void blend_pair(int fc, int fa, bool blend_fp16, float cr, float cg, float cb, float& acc_r, float& acc_g, float& acc_b, float& acc_a) {
    if (blend_fp16) {
        acc_r = blend_half_step(fc, acc_r, cr); acc_g = blend_half_step(fc, acc_g, cg); acc_b = blend_half_step(fc, acc_b, cb);
        acc_a = blend_half_step(fa, acc_a, 1.0f);
    } else {
        acc_r = blend_gather(fc, acc_r, cr); acc_g = blend_gather(fc, acc_g, cg); acc_b = blend_gather(fc, acc_b, cb);
        acc_a = blend_gather(fa, acc_a, 1.0f);
    }
}

// Eight waves per SIMD (64 VGPRs; the fp16 kernel without scratch, the unorm16 one with 8 bytes outside the loop).  History, tools/ab_lib.sh:
// r02, table-driven sampler: five waves (81 VGPRs, the allocator's own need) cfg5 11.93 ms, six 11.26, seven 10.89, eight (48 bytes of
// scratch) 10.93.  r03, cell array + exact skips + tile groups: six 9.29, seven 8.82, eight 8.67 on cfg5 but 0.61 -> 0.66 on cfg3 (spills
// in the per-pair code).  With the launch descriptor read where it is needed (the light loop below) the spills are gone:
// seven 0.616 | 8.93, **eight 0.602 | 8.54**.
// WIDE_BIN: the tile list is built by all the workgroup's waves, 256 lights per round (frames of particle lights: thousands per tile);
// otherwise by wave 0 alone, 64 per round, while the others wait -- a frame of a few hundred lights bins in 1-4 rounds either way, and
// the wide form's extra code costs the sphere-light frames 1-2 % through register allocation, so it is its own instantiation.
// BLEND (VARIANT = the field format + kBlendVariant): the launch's blend functions are not ADD / ADD (blend_pair and its neighbours
// above; the functions are read from the launch descriptor where they are used).  An instantiation of its own for the same reason:
// with BLEND = false every line it adds is compiled out.  Such a launch comes with one workgroup per tile (api.hip plan_light_split),
// so the partial hand-off only ever carries sums.
template <int VARIANT, bool STATS, bool WIDE_BIN>
__global__ __launch_bounds__(kLightThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void sphere_lights_kernel(const LightLaunch a, const LightRec* __restrict__ recs, int tiles_x, int tiles_y, int tile_count) {
    constexpr int FMT = VARIANT & ~kBlendVariant;
    constexpr bool BLEND = (VARIANT & kBlendVariant) != 0;
    __shared__ uint16_t list[kListCapacity];
    __shared__ int list_count;
    __shared__ int bin_count[2][kLightThreads / 64];
    __shared__ SliceEntry slice_table[kMaxTableSlices];
    __shared__ float4 tree[3][kLightThreads];       // the part sums waiting for their right-hand neighbours (levels 0-2 of the tree over 8 parts)
    __shared__ float4 wave_box[kLightThreads / 64];  // circle cull: (min x, max x, min y, max y) of the shaded points of each wave's 8 x 8 pixels

    // The dispatcher places block b on XCD b % 8.  Which tiles an XCD gets decides both its L2 locality and its share of the work
    // (lights are not spread evenly): square groups of tile_macro x tile_macro tiles, dealt round-robin to the XCDs (api.hip has the
    // measurements of this and the other mappings tried).
    // Light split: consecutive blocks of an XCD serve one tile (they share its L2: cells, light records, the tile's partial sums);
    // b is the tile's block number as the maps below see it, `member` which of the tile's workgroups this is.
    // (the launch descriptor through a pointer the compiler cannot see through -- see the light loop: what is read here is not kept
    // in scalar registers across the kernel)
    typedef const LightLaunch __attribute__((address_space(4))) CLightLaunch;
    auto kernargs = []() -> const LightLaunch& {
        CLightLaunch* ap = (CLightLaunch*)__builtin_amdgcn_kernarg_segment_ptr();      // the descriptor is the kernel's FIRST parameter: offset 0
        asm volatile("" : "+s"(ap));
        return *(const LightLaunch*)ap;
    };
    // Which of an XCD's block slots this is, and what it serves: slots [0, taper[0]) are whole tiles, the next 2 (taper[1] - taper[0]) the
    // two members of a tile each, then four, then eight (tile_split): the launch ends in its smallest pieces.
    auto tile_split = [&](int& slot, int& member) -> int {
        const LightLaunch& A = kernargs();
        const int k = (int)blockIdx.x / 8;
        const int t0 = A.taper[0], t1 = A.taper[1], t2 = A.taper[2];
        const int b1 = t0 + 2 * (t1 - t0), b2 = b1 + 4 * (t2 - t1);
        if (k < t0) { slot = k; member = 0; return 1; }
        if (k < b1) { slot = t0 + (k - t0) / 2; member = (k - t0) % 2; return 2; }
        if (k < b2) { slot = t1 + (k - b1) / 4; member = (k - b1) % 4; return 4; }
        slot = t2 + (k - b2) / 8; member = (k - b2) % 8; return 8;
    };
    int member, b;
    {
        int slot;
        (void)tile_split(slot, member);
        b = slot * 8 + ((int)blockIdx.x % 8);
    }
    int tile;
    {
        // square groups of M x M tiles, dealt round-robin to the XCDs; an XCD walks its groups one after the other, so the tiles it
        // runs side by side lie side by side
        const int M = a.tile_macro, MM = M * M;
        const int xcd = b % 8, k = b / 8;
        int g = (k / MM) * 8 + xcd;
        const int t = k % MM;
        const int mx = (tiles_x + M - 1) / M;
        if (a.group_order != nullptr && g < mx * ((tiles_y + M - 1) / M)) g = (int)a.group_order[g];
        const int ty = (g / mx) * M + t / M, tx = (g % mx) * M + t % M;
        tile = (tx < tiles_x && ty < tiles_y) ? ty * tiles_x + tx : tile_count;
    }
    if (tile >= tile_count)
        return;
    // the in-volume sampler's per-slice table (hlsl_math.hpp): one entry per virtual slice, visible to the tile's waves after the
    // first barrier of the light loop below
    const int table_n = a.sdf.table_slices;
    for (int i = (int)threadIdx.x; i < table_n; i += kLightThreads) slice_table[i] = make_slice_entry((uint32_t)i, a.df, a.sdf);
    const InsideConsts inside = make_inside_consts(a.df, a.sdf);
    const int tx0 = (tile % tiles_x) * kTile, ty0 = a.row_begin + (tile / tiles_x) * kTile;

    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int px = tx0 + (wave & 1) * 8 + (lane & 7);
    const int py = ty0 + (wave >> 1) * 8 + (lane >> 3);
    const bool in_image = (px < a.width) && (py < a.row_end);

    Pixel P = sample_gbuffer((float)px, (float)py, a.env, a.gbuffer);
    P.origin_x = tx0 + (wave & 1) * 8; P.origin_y = ty0 + (wave >> 1) * 8;
    P.start_inside = (table_n > 0) && trace_start_inside(P, a.df, a.sdf);
    const float cxp = (float)px + 0.5f, cyp = (float)py + 0.5f;
    const bool have_sdf = (a.sdf.texels != nullptr) && (a.df.Extent.x > 0.0f);
    // Circle cull (r05).  A light adds nothing to a point whose distance from its centre (y scaled by the light's falloffY) is at least
    // radius + max(ramp, 1): computeSphereLightOpacity's distance factor and its saturate(radius - distance) term are both exactly 0
    // there (LightCommon.fxh:174-214; every falloff mode), the shader discards.  The raster footprint is a square (particle lights) or a
    // cut-corner square (sphere lights) around that circle: 21 % / 13 % of its pixels lie outside it.  Each wave publishes the xy bounding
    // box of the SHADED POINTS of its 8 x 8 pixels (whatever the G-buffer made of them: no assumption about ZToY or relativeY), and the
    // binning marks, per list entry, the waves whose box lies wholly outside the light's circle (4 bits of the 16-bit entry): those waves
    // skip the entry on a scalar test, an entry no wave needs is not listed.  Not in the statistics variant, whose pair count is the
    // raster footprint's (so that variant is also the reference the culled frames are held to, bit for bit).  Only in the wide-binning
    // (particle-light) instantiations.
    constexpr bool kCircleCull = !STATS && WIDE_BIN;
    if constexpr (kCircleCull) {
        const bool finite_xy = (fabsf(P.shaded.x) <= 0x1p100f) && (fabsf(P.shaded.y) <= 0x1p100f);
        const float inf = __builtin_inff();
        // (a lane outside the image shades nothing: neutral; a lane whose point is not finite opens the box to everything)
        float lo_x = in_image ? (finite_xy ? P.shaded.x : -inf) : inf, hi_x = in_image ? (finite_xy ? P.shaded.x : inf) : -inf;
        float lo_y = in_image ? (finite_xy ? P.shaded.y : -inf) : inf, hi_y = in_image ? (finite_xy ? P.shaded.y : inf) : -inf;
        for (int off = 32; off > 0; off >>= 1) {
            lo_x = fminf(lo_x, __shfl_xor(lo_x, off)); hi_x = fmaxf(hi_x, __shfl_xor(hi_x, off));
            lo_y = fminf(lo_y, __shfl_xor(lo_y, off)); hi_y = fmaxf(hi_y, __shfl_xor(hi_y, off));
        }
        if (lane == 0) wave_box[wave] = mk4(lo_x, hi_x, lo_y, hi_y);      // read after the first barrier of the light loop
    }
    // the waves of the workgroup whose box lies wholly outside the circle of light R (bit w = wave w), by whoever bins R
    auto culled_waves = [&](const LightRec& R) -> int {
        if constexpr (!kCircleCull) return 0;
        const float reach = R.radius + fmaxf(R.ramp, 1.0f), fy = fabsf(R.falloff_y);
        // (a ramp that is not positive never fades; NaNs fail every comparison below: no cull)
        const bool cullable = (R.ramp > 0.0f) & (R.radius >= 0.0f) & (reach <= 0x1p60f) & (fy <= 0x1p60f);
        const float limit = reach * 1.0001f + 0.01f, limit2 = limit * limit;
        int mask = 0;
#pragma unroll 1      // (one box at a time: the pass runs with the pixel's whole state live, 64 registers)
        for (int w = 0; w < kLightThreads / 64; w++) {
            const float4 b = wave_box[w];
            const float dx = fmaxf(fmaxf(b.x - R.cx, R.cx - b.y), 0.0f), dy = fmaxf(fmaxf(b.z - R.cy, R.cy - b.w), 0.0f) * fy;
            if (cullable && (dx * dx + dy * dy >= limit2)) mask |= 1 << w;
        }
        return mask;
    };
    // Entry layout of the LDS list: the light's index within the batch, the four cull bits above it, bit 15 = the tile lies wholly inside
    // the footprint.  The wide binning with the cull (r06, BIG): a batch holds up to 4 096 lights -- 12 index bits, the cull bits above,
    // no bit 15 (the walk always takes the per-pixel footprint test) -- and ends early when another round of 256 lights might not fit the
    // list: 4 096 particle lights were four batches of 1 024, four lists of ten entries with the tile's waves meeting at the end of each;
    // one list of forty, one meeting: 0.991 -> 0.978 ms per frame, the same bits (tools/particle_lights_ab.py, profiles/r06_lane_queue_ab.txt).
    constexpr bool BIG = WIDE_BIN && kCircleCull;
    constexpr int kCullShift = BIG ? 12 : 10, kIndexMask = (1 << kCullShift) - 1;
    const int cull_bit = __builtin_amdgcn_readfirstlane(kCullShift + wave);      // (uniform by construction; said so, so that the walk's test is scalar)

    // What the lights are added to: the clear colour, or the lightmap's contents (additive blend onto an earlier pass of the same frame:
    // another light-type render state, LightingRenderer.cs:1100-1169).  Read when it is needed -- at the end, where the tile's sum is
    // added to it; in the fp16-per-light model at the start, where the chain of roundings begins.
    // The reference's lightmap is a HalfVector4 surface blended into by the ROP light after light (LightingRenderer.cs:476-479): in that
    // model the clear colour and every partial sum pass through fp16.  Off by default (fp32 accumulation, one rounding at the store).
    auto through_half = [](float v) { return __half2float(__float2half_rn(v)); };
    auto base_value = [&](const LightLaunch& A) -> float4 {
        float4 v = mk4(A.ambient[0], A.ambient[1], A.ambient[2], A.ambient[3]);
        if (A.accumulate != 0 && in_image) {
            const size_t o = (size_t)py * (size_t)A.width + (size_t)px;
            if (A.format == ILM_LIGHTMAP_FLOAT4) {
                v = reinterpret_cast<const float4*>(A.lightmap)[o];
            } else if (A.format == ILM_LIGHTMAP_HALF4) {
                const uint2 h = reinterpret_cast<const uint2*>(A.lightmap)[o];
                v = mk4(__half2float(__ushort_as_half((unsigned short)(h.x & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(h.x >> 16))),
                        __half2float(__ushort_as_half((unsigned short)(h.y & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(h.y >> 16))));
            } else {
                const uint32_t c = reinterpret_cast<const uint32_t*>(A.lightmap)[o];
                v = mk4((float)(c & 0xFFu) / 255.0f, (float)((c >> 8) & 0xFFu) / 255.0f, (float)((c >> 16) & 0xFFu) / 255.0f, (float)(c >> 24) / 255.0f);
            }
        }
        if (A.blend_fp16 != 0) v = mk4(through_half(v.x), through_half(v.y), through_half(v.z), through_half(v.w));
        return v;
    };
    const bool blend_fp16 = a.blend_fp16 != 0;
    // the running sum of the current part of the light list (the whole chain in the fp16-per-light model)
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, acc_a = 0.0f;
    if constexpr (BLEND) { acc_r = acc_g = acc_b = blend_identity(a.blend_color); acc_a = blend_identity(a.blend_alpha); }
    if (blend_fp16) { const float4 v = base_value(a); acc_r = v.x; acc_g = v.y; acc_b = v.z; acc_a = v.w; }
    // wave-uniform: every pixel of this wave has a flat normal (no G-buffer, or ground / top-face texels): the normal factor needs one
    // component of the light direction instead of three (sphere_light_opacity<.., FLAT>)
    const bool flat_normals = __builtin_amdgcn_ballot_w64((P.normal.x != 0.0f) | (P.normal.y != 0.0f)) == 0ull;
    LightStats st;
    const int light_count = (a.light_count_ptr != nullptr) ? __builtin_amdgcn_readfirstlane(*a.light_count_ptr) : a.light_count;

    // ---- the order of the sum -------------------------------------------------------------------------------------------------------
    // The reference adds the lights of a pixel in draw order through the ROP (LightingRenderer.cs:1149-1166 cuts the list into draws of
    // 128 instances; SphereLight.fx:42-45 is what each adds).  Here the launch's light list is cut, BY LIGHT INDEX, into kLightParts parts
    // (part p = lights [L p / 8, L (p + 1) / 8)); a pixel's contributions are summed part by part in light order, each part from zero,
    // the part sums are combined as a balanced binary tree ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7)), and the tree's root is
    // added to the base value.  That order depends on the light list and the pixel alone -- not on the tile grid (strips may start on
    // any row), nor on how many workgroups serve a tile: with `split` = K of them, member m bins and walks the lights of its 8 / K parts
    // only, its subtree's sum goes to memory, and the member that arrives last adds the K subtree sums (the tree's upper levels).
    // (The fp16-per-light model is one chain of roundings in light order: no parts, split 1.)
    int part, part_end;
    {
        int slot_, member_;
        const int parts_each = kLightParts / tile_split(slot_, member_);
        part = member * parts_each; part_end = part + parts_each;
    }
    const int light_lo = blend_fp16 ? 0 : (int)(((long long)light_count * part) / kLightParts);
    const int light_hi = blend_fp16 ? light_count : (int)(((long long)light_count * part_end) / kLightParts);
    const int part_first = part;
    // closes the current part: its sum joins the tree (a sum whose index in the member's range is odd has its left-hand neighbour waiting
    // one level down: left + right, then one level up), and the registers start the next part from zero
    auto close_part = [&]() {
        int r = part - part_first, level = 0;
        while (r & 1) {
            const float4 left = tree[level][threadIdx.x];
            if constexpr (BLEND) {
                const int fc = kernargs().blend_color, fa = kernargs().blend_alpha;
                acc_r = blend_gather(fc, left.x, acc_r); acc_g = blend_gather(fc, left.y, acc_g); acc_b = blend_gather(fc, left.z, acc_b);
                acc_a = blend_gather(fa, left.w, acc_a);
            } else {
                acc_r = left.x + acc_r; acc_g = left.y + acc_g; acc_b = left.z + acc_b; acc_a = left.w + acc_a;
            }
            level++; r >>= 1;
        }
        part++;
        if (part < part_end) {
            tree[level][threadIdx.x] = mk4(acc_r, acc_g, acc_b, acc_a);
            acc_r = 0.0f; acc_g = 0.0f; acc_b = 0.0f; acc_a = 0.0f;
            if constexpr (BLEND) { acc_r = acc_g = acc_b = blend_identity(kernargs().blend_color); acc_a = blend_identity(kernargs().blend_alpha); }
        }       // else: the member's subtree is summed, its root stays in the registers
    };
    int part_bound = blend_fp16 ? 0x7FFFFFFF : (int)(((long long)light_count * (part + 1)) / kLightParts);   // first light of the next part

    for (int batch = light_lo, batch_step = kListCapacity; batch < light_hi; batch += batch_step) {
        int batch_n = min(BIG ? 4096 : kListCapacity, light_hi - batch);
        if constexpr (WIDE_BIN) {
        __syncthreads();                                        // the previous batch's list has been walked
        {
            // ordered compaction of the lights whose footprint bounding box touches the tile: all the workgroup's threads test one light
            // each per round (a frame of particle lights bins thousands per tile), the waves' counts meet in LDS, the list keeps light order
            const float tminx = (float)tx0 + 0.5f, tmaxx = (float)(tx0 + kTile - 1) + 0.5f;
            const float tminy = (float)ty0 + 0.5f, tmaxy = (float)(ty0 + kTile - 1) + 0.5f;
            constexpr int kWaves = kLightThreads / 64;
            int base = 0, l0 = 0;
            for (; l0 < batch_n && (!BIG || base + kLightThreads <= kListCapacity); l0 += kLightThreads) {
                const int li = l0 + (int)threadIdx.x;
                bool hit = false, whole = false;
                if (li < batch_n) {
                    const LightRec& R = recs[batch + li];
                    const float4 fx = *reinterpret_cast<const float4*>(&R.fx0), fy = *reinterpret_cast<const float4*>(&R.fy0);
                    hit = (fx.x <= tmaxx) && (fx.w > tminx) && (fy.x <= tmaxy) && (fy.w > tminy);
                    // the whole tile inside one of the footprint's two rectangles: every pixel centre passes the per-pixel test below (the
                    // same comparisons, taken on the tile's extreme centres), so the walk skips it for this entry (bit 15)
                    whole = ((tminx >= fx.y) && (tmaxx < fx.z) && (tminy >= fy.x) && (tmaxy < fy.w)) ||
                            ((tminx >= fx.x) && (tmaxx < fx.w) && (tminy >= fy.y) && (tmaxy < fy.z));
                }
                const unsigned long long m = __ballot(hit);
                const int round = (l0 / kLightThreads) & 1;     // two sets of counters: a wave may be a round ahead of the slowest reader
                if (lane == 0) bin_count[round][wave] = __popcll(m);
                __syncthreads();
                int before = 0, total = 0;
#pragma unroll
                for (int w = 0; w < kWaves; w++) { const int c = bin_count[round][w]; total += c; if (w < wave) before += c; }
                if (hit)
                    list[base + before + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)(li | ((whole && !BIG) ? 0x8000 : 0));
                base += total;
            }
            // (the batch ends where the binning stopped: `base` is the same in every thread, so is l0)
            if constexpr (BIG) { batch_n = min(batch_n, l0); batch_step = (batch_n > 0) ? batch_n : 4096; }
            if (threadIdx.x == 0) list_count = base;
        }
        __syncthreads();
        } else {
        __syncthreads();
        if (threadIdx.x == 0) list_count = 0;
        __syncthreads();
        if (wave == 0) {
            // ordered compaction of the lights whose footprint bounding box touches the tile
            const float tminx = (float)tx0 + 0.5f, tmaxx = (float)(tx0 + kTile - 1) + 0.5f;
            const float tminy = (float)ty0 + 0.5f, tmaxy = (float)(ty0 + kTile - 1) + 0.5f;
            int base = 0;
            for (int l0 = 0; l0 < batch_n; l0 += 64) {
                const int li = l0 + lane;
                bool hit = false, whole = false;
                if (li < batch_n) {
                    const LightRec& R = recs[batch + li];
                    hit = (R.fx0 <= tmaxx) && (R.fx3 > tminx) && (R.fy0 <= tmaxy) && (R.fy3 > tminy);
                    // the whole tile inside one of the footprint's two rectangles: every pixel centre passes the per-pixel test below (the
                    // same comparisons, taken on the tile's extreme centres), so the walk skips it for this entry (bit 15)
                    whole = ((tminx >= R.fx1) && (tmaxx < R.fx2) && (tminy >= R.fy0) && (tmaxy < R.fy3)) ||
                            ((tminx >= R.fx0) && (tmaxx < R.fx3) && (tminy >= R.fy1) && (tmaxy < R.fy2));
                }
                const unsigned long long m = __ballot(hit);
                if (hit)
                    list[base + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)(li | (whole ? 0x8000 : 0));
                base += __popcll(m);
            }
            if (lane == 0) list_count = base;
        }
        __syncthreads();
        }

        const int n = list_count;
        if constexpr (kCircleCull) {
            // the cull bits of the LISTED lights only (the binning looks at every light of the launch -- thousands of particle lights per
            // tile, of which a few dozen are listed: computing the bits there cost more than the skipped entries gave back)
            for (int t = (int)threadIdx.x; t < n; t += kLightThreads) {
                const int e = (int)list[t];
                list[t] = (uint16_t)(e | (culled_waves(recs[batch + (e & kIndexMask)]) << kCullShift));
            }
            __syncthreads();
        }

        for (int k = 0; k < n; k++) {
            // The launch descriptor lives in the kernarg segment.  Read through a pointer the compiler cannot see through, its fields are
            // fetched (scalar-cache hits) where a pair needs them instead of being hoisted out of the light loop and held in SGPRs across
            // the whole kernel: 32-42 scalar registers were spilled to vector lanes that way, now 2 -- by itself worth nothing (cfg5
            // 8.82 -> 8.93 ms), but the vector registers it frees are what lets EIGHT waves per SIMD run without spilling in the loop.
            // (the descriptor is the kernel's FIRST parameter: offset 0 of the segment)
            const LightLaunch& A = kernargs();
            const TraceField field = { A.df, A.sdf, inside, (table_n > 0) ? slice_table : nullptr };
            const IlmEnvironment& env_k = A.env;
            const RampView& ramp_k = A.ramp;
            const int entry = __builtin_amdgcn_readfirstlane((int)list[k]);
            const int li = entry & (kCircleCull ? kIndexMask : 0x7FFF);
            if (kCircleCull && ((entry >> cull_bit) & 1))      // this wave's points are outside the light's circle (see culled_waves): a scalar test
                continue;
            while (batch + li >= part_bound) {      // (never in the fp16-per-light model)
                close_part();
                part_bound = (int)(((long long)light_count * (part + 1)) / kLightParts);
            }
            // (r05: fetching the whole 128-byte record at once for the wide-binning walk -- two 64-byte scalar loads, one wait instead of
            // seven -- was measured a loss like r04's hot / cold record on cfg3: particle lights 1.035 / 1.055 -> 1.071 / 1.088 ms; the 32
            // scalar registers it holds spill 40 more to vector lanes)
            const LightRec& L = recs[batch + li];

            bool covered = in_image;
            if (BIG || (entry & 0x8000) == 0) {
                // raster footprint: pixel centre inside the cross-shaped quad
                // (all eight bounds fetched together and combined without short-circuits: as written with && / || the compiler issued
                // eight dependent scalar loads, each behind its own wait and branch)
                const float fx0 = L.fx0, fx1 = L.fx1, fx2 = L.fx2, fx3 = L.fx3, fy0 = L.fy0, fy1 = L.fy1, fy2 = L.fy2, fy3 = L.fy3;
                const bool tall = (cxp >= fx1) & (cxp < fx2) & (cyp >= fy0) & (cyp < fy3);
                const bool wide = (cxp >= fx0) & (cxp < fx3) & (cyp >= fy1) & (cyp < fy2);
                covered = in_image & (tall | wide);
            }
            // (r06) A wave NONE of whose lanes the entry covers leaves on a scalar branch.  Without it such a wave runs the head of the
            // pair code masked off -- the compiler only branches around blocks it finds long enough -- ~31 vector instructions per
            // list entry on the particle-light frame (the tile lists a light whose footprint misses this quadrant, and the cull's box
            // test did not catch it): 468 M -> 429 M vector instructions per launch, **0.979 -> 0.931 ms per frame**
            // (profiles/r06_particle_lights_wave_skip_ab.txt).  On the sphere-light instantiations it changes nothing
            // -- cfg3 0.625 / 0.625 -> 0.625 / 0.622, cfg5 8.691 / 8.695 -> 8.701 / 8.704 ms -- their lists are short and their lights
            // large: the branch is paid by every entry and almost never taken.
            if (WIDE_BIN && __builtin_amdgcn_ballot_w64(covered) == 0ull)
                continue;
            if (!covered)
                continue;
            if (STATS) st.pairs++;
            float cr, cg, cb;
            if (!shade_light<FMT, STATS>(P, L, env_k, field, have_sdf, ramp_k, st, cr, cg, cb, flat_normals))
                continue;
            if constexpr (BLEND) {
                blend_pair(A.blend_color, A.blend_alpha, blend_fp16, cr, cg, cb, acc_r, acc_g, acc_b, acc_a);
            } else if (blend_fp16) {      // dst = half(float(dst) + float(half(src))): the shader's output is converted to the target format, then blended
                acc_r = through_half(acc_r + through_half(cr));
                acc_g = through_half(acc_g + through_half(cg));
                acc_b = through_half(acc_b + through_half(cb));
                acc_a = through_half(acc_a + 1.0f);
            } else {
                acc_r += cr;
                acc_g += cg;
                acc_b += cb;
                acc_a += 1.0f;
            }
        }
    }
    if (!blend_fp16) {
        while (part < part_end) close_part();       // the parts behind the last listed light (empty ones add their zeros: the same additions whatever the split)
    }

    int slot_end, member_end;
    const int split = tile_split(slot_end, member_end);
    if (split > 1) {
        // The members of a tile meet at its tickets, wave by wave: the waves of a workgroup own a quadrant each, so quadrant q of member m
        // only ever needs quadrant q of the other members -- no barrier, every wave leaves when ITS part is delivered.  A wave writes its
        // subtree's sums (device-scope stores, sc1: written through this XCD's L2), waits until the write is acknowledged, draws the
        // quadrant's ticket (device-scope atomic); the one that draws the last reads the K sums back with device-scope loads -- no cache
        // write-back or invalidate is involved, the light pass's L2 contents (the field's cells) stay where they are.
        // (scratch is indexed by the tile's place among the SPLIT block slots of the launch -- slot - taper[0] of this XCD -- not by the tile:
        // the untapered head of a launch needs none, api.hip plan_light_split sizes it so)
        const size_t split_slot = (size_t)(slot_end - kernargs().taper[0]) * 8u + (size_t)((int)blockIdx.x % 8);
        float4* tile_sums = kernargs().partials + split_slot * (size_t)kLightParts * (size_t)kLightThreads + threadIdx.x;
        store_partial(tile_sums + (size_t)member_end * (size_t)kLightThreads, acc_r, acc_g, acc_b, acc_a);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t drawn = 0;
        uint32_t* ticket = kernargs().tickets + (size_t)tile * (size_t)(kLightThreads / 64) + (size_t)wave;
        if (lane == 0) drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        drawn = (uint32_t)__builtin_amdgcn_readfirstlane((int)drawn);
        if (drawn != (uint32_t)(split - 1))
            goto tile_done;
        if (lane == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // ready for the next launch
        asm volatile("" ::: "memory");
        const float4 v = combine_partials(tile_sums, (size_t)kLightThreads, split);
        acc_r = v.x; acc_g = v.y; acc_b = v.z; acc_a = v.w;
    }
    if (!blend_fp16) {
        const float4 v = base_value(kernargs());
        if constexpr (BLEND) {
            const int fc = kernargs().blend_color, fa = kernargs().blend_alpha;
            acc_r = blend_onto_base(fc, v.x, acc_r); acc_g = blend_onto_base(fc, v.y, acc_g); acc_b = blend_onto_base(fc, v.z, acc_b);
            acc_a = blend_onto_base(fa, v.w, acc_a);
        } else {
            acc_r = v.x + acc_r; acc_g = v.y + acc_g; acc_b = v.z + acc_b; acc_a = v.w + acc_a;
        }
    }

    if (in_image) {
        const size_t o = (size_t)py * (size_t)a.width + (size_t)px;
        // the texel, once; then wherever it goes: the lightmap, and in store mode the same offset of every other member's copy of the
        // frame (peer-mapped; 8 x 8 pixels of a wave are eight 64-byte runs of half4 texels)
        const float4 v32 = mk4(acc_r, acc_g, acc_b, acc_a);
        uint2 v16 = make_uint2(0u, 0u);
        uint32_t v8 = 0u;
        if (a.format == ILM_LIGHTMAP_HALF4) {
            v16.x = (uint32_t)__half_as_ushort(__float2half_rn(acc_r)) | ((uint32_t)__half_as_ushort(__float2half_rn(acc_g)) << 16);
            v16.y = (uint32_t)__half_as_ushort(__float2half_rn(acc_b)) | ((uint32_t)__half_as_ushort(__float2half_rn(acc_a)) << 16);
        } else if (a.format != ILM_LIGHTMAP_FLOAT4) {
            const uint32_t r = (uint32_t)rintf(sat(acc_r) * 255.0f), g = (uint32_t)rintf(sat(acc_g) * 255.0f);
            const uint32_t bl = (uint32_t)rintf(sat(acc_b) * 255.0f), al = (uint32_t)rintf(sat(acc_a) * 255.0f);
            v8 = r | (g << 8) | (bl << 16) | (al << 24);
        }
        auto store_texel = [&](void* base) {
            if (a.format == ILM_LIGHTMAP_FLOAT4) reinterpret_cast<float4*>(base)[o] = v32;
            else if (a.format == ILM_LIGHTMAP_HALF4) reinterpret_cast<uint2*>(base)[o] = v16;
            else reinterpret_cast<uint32_t*>(base)[o] = v8;
        };
        store_texel(a.lightmap);
        const LightLaunch& A = kernargs();
        const int mirror_count = A.mirror_count;
        for (int m = 0; m < mirror_count; m++) store_texel(A.mirrors[m]);
    }

tile_done:
    if (STATS) {
        // wave reduce, one atomic per wave and counter
        for (int off = 32; off > 0; off >>= 1) {
            st.samples += __shfl_down(st.samples, off);
            st.pairs += __shfl_down(st.pairs, off);
            st.traced += __shfl_down(st.traced, off);
        }
        if (lane == 0) {
            atomicAdd(&a.stats[0], st.samples);
            atomicAdd(&a.stats[1], st.pairs);
            atomicAdd(&a.stats[2], st.traced);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Particle lights -- ParticleLightVertexShader, ParticleLight.fx:16-83, for every slot below the chunk's quad count:
// a light record is emitted iff life > 0 and the un-premultiplied render colour x LightColor has alpha > 0.
// Two passes over 1024-slot blocks: counts, then an ordered emit (block base = sum of the counts before it; inside a
// block: wave64 ballot + popcount prefix, wave bases through LDS), so the records come out in chunk / slot order --
// the order the reference's instanced draw blends them in.
// ---------------------------------------------------------------------------------------------
constexpr int kPlBlock = 1024;

// What makes a slot a light source once its chunk's base pointer is known and the slot lies below the quad count: the eight loads, the
// un-premultiply, life > 0, the product with the call's or the item's LightColor, alpha > 0.  Called by particle_emits_light (the single
// call's front end over the chunk table) and by both batch kernels (front end: slot >= e.quads); the order of the statements is the order
// of the shader's (:43-45 before the life test) and stays.
ILM_DEV bool particle_slot_emits_light(const float* base, int64_t S, int slot, const IlmFloat4& item_color, float4& position, float4& light_color) {
    position = mk4(base[slot], base[S + slot], base[2 * S + slot], base[3 * S + slot]);
    float4 rc = mk4(base[12 * S + slot], base[13 * S + slot], base[14 * S + slot], base[15 * S + slot]);   // Chunk.RenderColor
    if (rc.w > 0.0f) {   // unpremultiply, :43-45
        rc.x /= rc.w; rc.y /= rc.w; rc.z /= rc.w;
    }
    if (position.w <= 0.0f)
        return false;
    light_color = mul4(rc, ld4(item_color));
    return light_color.w > 0.0f;
}

ILM_DEV bool particle_emits_light(const ParticleLightLaunch& a, int chunk, int slot, float4& position, float4& light_color) {
    const int quads = (a.quad_counts != nullptr) ? a.quad_counts[chunk] : a.slots;
    if (slot >= quads || slot >= a.slots)
        return false;
    return particle_slot_emits_light(a.chunk_bases[chunk], a.stride, slot, a.params.LightColor, position, light_color);
}

// The record of one emitting particle, for particle_light_emit_kernel (P = the call's parameters) and particle_light_batch_emit_kernel
// (P = params[e.item], a reference into the table: wave-uniform, so its loads stay scalar).  Every operation stays as it is written and
// in this order, the `* 1.0f` included: contraction is off and the records' bits are what the tile pass and the oracle tests see.
ILM_DEV LightRec particle_light_record(const float4& pos, const float4& col, const IlmParticleLightParams& P, const IlmEnvironment& env,
                                       float max_cone_radius, const TraceGate& gate) {
    LightRec r;
    r.cx = pos.x; r.cy = pos.y; r.cz = pos.z;
    r.radius = P.LightProperties.x; r.ramp = P.LightProperties.y; r.falloff_mode = P.LightProperties.z; r.casts_shadows = P.LightProperties.w;
    r.ao_radius = P.MoreLightProperties.x; r.falloff_y = P.MoreLightProperties.z; r.ao_opacity = P.MoreLightProperties.w;
    r.shadow_filter = -1.0f;                                                   // ParticleLightPixelShader has no shadow filter
    r.col_r = col.x * col.w; r.col_g = col.y * col.w; r.col_b = col.z * col.w; // lightColor.rgb * lightColor.a, :113-116
    r.spec_r = P.LightSpecularColor.x; r.spec_g = P.LightSpecularColor.y; r.spec_b = P.LightSpecularColor.z; r.spec_power = P.LightSpecularColor.w;
    // the quad, :55-70: a plain rectangle (fx1 = fx0, fx2 = fx3 collapse the sphere light's cross shape onto it)
    const float radius = P.LightProperties.x + P.LightProperties.y + 1.0f;
    const float tlx = r.cx - radius, brx = r.cx + radius, bry = r.cy + radius;
    float tly = r.cy - radius;
    tly -= radius * env.ZToY.y;
    tly -= r.cz * env.ZToY.x;
    const float sx = env.GBufferTexelSizeAndMisc.z * env.ZAndScale.z, sy = env.GBufferTexelSizeAndMisc.w * env.ZAndScale.w;
    r.fx0 = r.fx1 = (tlx - env.ViewportPosition[0]) * sx;
    r.fx2 = r.fx3 = (brx - env.ViewportPosition[0]) * sx;
    r.fy0 = r.fy1 = (tly - env.ViewportPosition[1]) * sy;
    r.fy2 = r.fy3 = (bry - env.ViewportPosition[1]) * sy;
    const float max_radius = clampf(r.radius, ref::kMinConeRadius, max_cone_radius);
    r.cfg_x = max_radius;
    r.cfg_y = max_radius / fmaxf(r.ramp, 16.0f) * 1.0f;
    r.ramp_offset = r.ramp_rate = 0.0f;
    const int flags = light_flags(r, gate);
    r.flags = (float)flags;
    r.ramp_rcp = (flags & kLightFastDivide) ? refined_rcp(r.ramp) : 0.0f;
    return r;
}

__global__ __launch_bounds__(kPlBlock) void particle_light_count_kernel(const ParticleLightLaunch a, int blocks_per_chunk) {
    __shared__ int wave_counts[kPlBlock / 64];
    const int chunk = (int)blockIdx.x / blocks_per_chunk, blk = (int)blockIdx.x - chunk * blocks_per_chunk;
    const int slot = blk * kPlBlock + (int)threadIdx.x;
    float4 pos, col;
    const bool emit = particle_emits_light(a, chunk, slot, pos, col);
    const unsigned long long m = __ballot(emit);
    if ((threadIdx.x & 63u) == 0u) wave_counts[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < kPlBlock / 64; w++) n += wave_counts[w];
        a.block_counts[blockIdx.x] = n;
    }
}

__global__ __launch_bounds__(kPlBlock) void particle_light_emit_kernel(const ParticleLightLaunch a, int blocks_per_chunk) {
    __shared__ int wave_counts[kPlBlock / 64];
    __shared__ int partial[kPlBlock / 64];
    __shared__ int block_base;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    // exclusive prefix of the block counts before this block (a few thousand ints at most)
    int sum = 0;
    for (int i = (int)threadIdx.x; i < (int)blockIdx.x; i += kPlBlock) sum += a.block_counts[i];
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if (lane == 0) partial[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int b = 0;
        for (int w = 0; w < kPlBlock / 64; w++) b += partial[w];
        block_base = b;
        if (blockIdx.x == gridDim.x - 1)
            *a.out_count = min(b + a.block_counts[blockIdx.x], a.capacity);
    }
    const int chunk = (int)blockIdx.x / blocks_per_chunk, blk = (int)blockIdx.x - chunk * blocks_per_chunk;
    const int slot = blk * kPlBlock + (int)threadIdx.x;
    float4 pos, col;
    const bool emit = particle_emits_light(a, chunk, slot, pos, col);
    const unsigned long long m = __ballot(emit);
    if (lane == 0) wave_counts[wave] = __popcll(m);
    __syncthreads();
    if (!emit)
        return;
    int index = block_base + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) index += wave_counts[w];
    if (index >= a.capacity)
        return;
    reinterpret_cast<LightRec*>(a.recs)[index] = particle_light_record(pos, col, a.params, a.env, a.max_cone_radius, a.gate);
}

hipError_t launch_prepare_particle_lights(const ParticleLightLaunch& a, hipStream_t stream) {
    const int blocks_per_chunk = (a.slots + kPlBlock - 1) / kPlBlock;
    const int blocks = a.chunk_count * blocks_per_chunk;
    if (blocks <= 0) return hipMemsetAsync(a.out_count, 0, sizeof(int32_t), stream);
    hipLaunchKernelGGL(particle_light_count_kernel, dim3(blocks), dim3(kPlBlock), 0, stream, a, blocks_per_chunk);
    hipLaunchKernelGGL(particle_light_emit_kernel, dim3(blocks), dim3(kPlBlock), 0, stream, a, blocks_per_chunk);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Particle lights of MANY systems as one record list (ilm_engine_render_particle_lights_batch): the compaction above over a table of
// (item, chunk) entries, every record built from its own item's parameters by particle_light_record.  A workgroup is 256 slots
// of ONE entry, so its entry and its item's parameters are wave-uniform (scalar loads); an entry owns ceil(quads / 256) consecutive
// workgroups from first_block on, found by a uniform bisection of the table.  Three launches whatever the number of items: the
// workgroups' counts, ONE workgroup that turns them into exclusive bases (a frame of many systems has more counts than the single
// call's "every block sums what lies before it" is meant for), the ordered emit.  No workgroup waits for another.
// ---------------------------------------------------------------------------------------------
constexpr int kPlBatchBlock = 256;
constexpr int kPlScanBlock = 1024;
static_assert(kPlBatchBlock == kParticleLightBatchBlock, "the host counts an entry's workgroups in kParticleLightBatchBlock slots");

// the last entry whose first_block <= block (first_block rises strictly: every entry has at least one workgroup)
ILM_DEV int particle_light_batch_entry(const ParticleLightBatchEntry* __restrict__ entries, int entry_count, int block) {
    int lo = 0, hi = entry_count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (entries[mid].first_block <= block) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// particle_emits_light's counterpart for a slot of an entry: the front end is the entry's quad count (quads <= slots: the entry point's check)
ILM_DEV bool particle_light_batch_emits(const ParticleLightBatchEntry& e, int64_t S, int slot, const IlmFloat4& item_color, float4& position,
                                        float4& light_color) {
    if (slot >= e.quads)
        return false;
    return particle_slot_emits_light(e.base, S, slot, item_color, position, light_color);
}

__global__ __launch_bounds__(kPlBatchBlock) void particle_light_batch_count_kernel(const ParticleLightBatchLaunch a,
                                                                                   const ParticleLightBatchEntry* __restrict__ entries,
                                                                                   const IlmParticleLightParams* __restrict__ params,
                                                                                   int32_t* __restrict__ block_counts) {
    __shared__ int wave_counts[kPlBatchBlock / 64];
    const ParticleLightBatchEntry e = entries[particle_light_batch_entry(entries, a.entry_count, (int)blockIdx.x)];
    const int slot = ((int)blockIdx.x - e.first_block) * kPlBatchBlock + (int)threadIdx.x;
    float4 pos, col;
    const bool emit = particle_light_batch_emits(e, a.stride, slot, params[e.item].LightColor, pos, col);
    const unsigned long long m = __ballot(emit);
    if ((threadIdx.x & 63u) == 0u) wave_counts[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < kPlBatchBlock / 64; w++) n += wave_counts[w];
        block_counts[blockIdx.x] = n;
    }
}

// counts[0 .. n) -> their exclusive prefix sums, in place; the total (at most `capacity`) -> *out_count and *out_count_host.  One
// workgroup walks the array 1 024 counts at a time: a wave's inclusive scan by shuffles, the sixteen wave totals through LDS, the
// carry in a register every lane keeps alike.
__global__ __launch_bounds__(kPlScanBlock) void particle_light_batch_scan_kernel(int32_t* __restrict__ counts, int n, int capacity,
                                                                                 int32_t* __restrict__ out_count, int32_t* __restrict__ out_count_host) {
    __shared__ int wave_sums[kPlScanBlock / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    int carry = 0;
    for (int first = 0; first < n; first += kPlScanBlock) {
        const int i = first + (int)threadIdx.x;
        const int v = (i < n) ? counts[i] : 0;
        int x = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63) wave_sums[wave] = x;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kPlScanBlock / 64; w++) {
            const int s = wave_sums[w];
            if (w < wave) before += s;
            total += s;
        }
        if (i < n) counts[i] = carry + before + x - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int total = min(carry, capacity);
        *out_count = total;
        *out_count_host = total;
    }
}

__global__ __launch_bounds__(kPlBatchBlock) void particle_light_batch_emit_kernel(const ParticleLightBatchLaunch a,
                                                                                  const ParticleLightBatchEntry* __restrict__ entries,
                                                                                  const IlmParticleLightParams* __restrict__ params,
                                                                                  const int32_t* __restrict__ block_bases, LightRec* __restrict__ recs) {
    __shared__ int wave_counts[kPlBatchBlock / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const ParticleLightBatchEntry e = entries[particle_light_batch_entry(entries, a.entry_count, (int)blockIdx.x)];
    const IlmParticleLightParams& P = params[e.item];
    const int slot = ((int)blockIdx.x - e.first_block) * kPlBatchBlock + (int)threadIdx.x;
    float4 pos, col;
    const bool emit = particle_light_batch_emits(e, a.stride, slot, P.LightColor, pos, col);
    const unsigned long long m = __ballot(emit);
    if (lane == 0) wave_counts[wave] = __popcll(m);
    __syncthreads();
    if (!emit)
        return;
    int index = block_bases[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) index += wave_counts[w];
    if (index >= a.capacity)
        return;
    recs[index] = particle_light_record(pos, col, P, a.env, a.max_cone_radius, a.gate);
}

hipError_t launch_prepare_particle_lights_batch(const ParticleLightBatchLaunch& a, hipStream_t stream) {
    hipLaunchKernelGGL(particle_light_batch_count_kernel, dim3(a.block_count), dim3(kPlBatchBlock), 0, stream, a, a.entries, a.params, a.block_counts);
    hipLaunchKernelGGL(particle_light_batch_scan_kernel, dim3(1), dim3(kPlScanBlock), 0, stream, a.block_counts, a.block_count, a.capacity, a.out_count,
                       a.out_count_host);
    hipLaunchKernelGGL(particle_light_batch_emit_kernel, dim3(a.block_count), dim3(kPlBatchBlock), 0, stream, a, a.entries, a.params, a.block_counts,
                       reinterpret_cast<LightRec*>(a.recs));
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Light probes -- SphereLightProbePixelShader, SphereLightProbe.fx:19-44: one lane per probe walks every light record
// (uniform index -> scalar loads), fp32 accumulation in light order.
// ---------------------------------------------------------------------------------------------
// r04: one WAVE per (block of 64 probes, light) instead of one lane walking every light (256 probes under 64 lights were four waves
// tracing 64 lights one after the other: 1.2 ms of latency); the pair's contribution goes to scratch [light][probe] and a second kernel
// adds a probe's contributions in light order -- the same additions in the same order.  `pairs` = nullptr: the one-kernel form (scratch
// for probe_count x light_count contributions was not to be had).
template <int FMT>
ILM_DEV bool probe_light(const float4 pp, const float4 pn, LightRec L, const IlmEnvironment& env, const TraceField& field, bool have_sdf, const RampView& ramp,
                         float& cr, float& cg, float& cb) {
    Pixel P;
    P.shaded = xyz(pp); P.normal = xyz(pn); P.origin_x = 0; P.origin_y = 0;      // (no specular term: SphereLightProbe.fx:33-42)
    P.fullbright = false;
    P.start_inside = false;
    // lightProperties.w *= enableShadows (a float here, not the G-buffer's flag); no AO, no specular, no shadow filter (:33-42)
    L.casts_shadows *= pn.w;
    P.enable_shadows = true;
    L.ao_radius = 0.0f; L.ao_opacity = 0.0f;
    L.shadow_filter = -1.0f;
    L.flags = (float)((int)L.flags & kLightFastDivide);     // no specular; probes use the general trace loop (no slice table here)
    LightStats st;
    return shade_light<FMT, false>(P, L, env, field, have_sdf, ramp, st, cr, cg, cb);
}

// What a probe kind supplies to light_probes_kernel: its record type, whether the field's InsideConsts are made (false: they stay {}),
// and shade(): whether the record lights the probe, and its contribution before the factor probe_opacity.
struct SphereProbes {      // ilm_render_light_probes, and ilm_render_line_light_probes through the sphere vertices the host makes
    using Rec = LightRec;
    static constexpr bool kInsideConsts = true;
    template <int FMT>
    static ILM_DEV bool shade(const float4 pp, const float4 pn, const LightRec& L, const IlmEnvironment& env, const TraceField& field, bool have_sdf,
                              const RampView& ramp, float& cr, float& cg, float& cb) {
        return probe_light<FMT>(pp, pn, L, env, field, have_sdf, ramp, cr, cg, cb);
    }
};

// The frame of every probe kind (KIND: SphereProbes above, DirectionalProbes below; launch_light_probes picks it): one lane per probe,
// the plain trace view without the cell array, then one contribution per wave in the pair form, or the one-kernel loop in light order.
// Both forms multiply the kind's contribution by probe_opacity afterwards -- (col * opacity) * probe_opacity -- and add in light order:
// neither the association nor the order may change, light_probes_sum_kernel and the oracle tests hold the two forms to the same bits.
template <int FMT, typename KIND>
__global__ __launch_bounds__(64) void light_probes_kernel(const typename KIND::Rec* __restrict__ recs, int light_count,
                                                           const float4* __restrict__ probe_positions, const float4* __restrict__ probe_normals,
                                                           int probe_count, IlmEnvironment env, IlmDistanceFieldUniforms df, SdfView sdf,
                                                           RampView ramp, float4* __restrict__ values, float4* __restrict__ pairs) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    const bool valid = i < probe_count;
    const float4 pp = valid ? probe_positions[i] : mk4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 pn = valid ? probe_normals[i] : mk4(0.0f, 0.0f, 0.0f, 0.0f);
    // sampleLightProbeBuffer, LightCommon.fxh:233-254
    const float probe_opacity = pp.w;
    const bool have_sdf = (sdf.texels != nullptr) && (df.Extent.x > 0.0f);
    TraceSdfView trace_sdf;                                       // probes are few: the general sampler, no cell array
    static_cast<SdfView&>(trace_sdf) = sdf;
    trace_sdf.cells = nullptr; trace_sdf.cells_bytes = 0; trace_sdf.slice_w = 0; trace_sdf.slice_h = 0;
    InsideConsts inside = {};
    if (KIND::kInsideConsts) inside = make_inside_consts(df, trace_sdf);
    const TraceField field = { df, trace_sdf, inside, nullptr };
    if (pairs != nullptr) {
        const int k = (int)blockIdx.y;                            // this wave's light
        float cr = 0.0f, cg = 0.0f, cb = 0.0f;
        bool lit = false;
        if (valid && probe_opacity > 0.0f)
            lit = KIND::template shade<FMT>(pp, pn, recs[k], env, field, have_sdf, ramp, cr, cg, cb);
        if (valid)
            pairs[(size_t)k * (size_t)probe_count + (size_t)i] = lit ? mk4(cr * probe_opacity, cg * probe_opacity, cb * probe_opacity, 1.0f) : mk4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, acc_a = 0.0f;
    for (int k = 0; k < light_count; k++) {
        const typename KIND::Rec& L = recs[k];
        if (!(valid && probe_opacity > 0.0f))
            continue;
        float cr, cg, cb;
        if (!KIND::template shade<FMT>(pp, pn, L, env, field, have_sdf, ramp, cr, cg, cb))
            continue;
        acc_r += cr * probe_opacity;
        acc_g += cg * probe_opacity;
        acc_b += cb * probe_opacity;
        acc_a += 1.0f;
    }
    if (valid)
        values[i] = mk4(acc_r, acc_g, acc_b, acc_a);
}

// a probe's contributions, added in light order (w = 1: the pair was lit and its products are added; w = 0: nothing is)
__global__ __launch_bounds__(64) void light_probes_sum_kernel(const float4* __restrict__ pairs, int light_count, int probe_count, float4* __restrict__ values) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= probe_count) return;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, acc_a = 0.0f;
    // (eight loads in flight; the additions stay one after the other, in light order)
    for (int k0 = 0; k0 < light_count; k0 += 8) {
        float4 c[8];
#pragma unroll
        for (int u = 0; u < 8; u++) c[u] = pairs[(size_t)min(k0 + u, light_count - 1) * (size_t)probe_count + (size_t)i];
#pragma unroll
        for (int u = 0; u < 8; u++)
            if ((k0 + u < light_count) && (c[u].w != 0.0f)) { acc_r += c[u].x; acc_g += c[u].y; acc_b += c[u].z; acc_a += 1.0f; }
    }
    values[i] = mk4(acc_r, acc_g, acc_b, acc_a);
}

template <int FMT>
__global__ __launch_bounds__(256) void sdf_sample_kernel(SdfView sdf, IlmDistanceFieldUniforms df, const float* __restrict__ positions, int count,
                                                          float* __restrict__ out) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= count) return;
    out[i] = sample_distance_field<FMT>(mk3(positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]), df, sdf);
}

// the cone trace's in-volume sampler on caller-supplied positions (diagnostic entry point ilm_debug_sdf_sample_inside): positions inside
// the sampler's box go through sample_inside_table exactly as the trace loop calls it (used = 1), the others through the general sampler
template <int FMT>
__global__ __launch_bounds__(256) void sdf_sample_inside_kernel(TraceSdfView sdf, IlmDistanceFieldUniforms df, const float* __restrict__ positions, int count,
                                                                 float* __restrict__ out, int32_t* __restrict__ used) {
    __shared__ SliceEntry slice_table[kMaxTableSlices];
    for (int i = (int)threadIdx.x; i < sdf.table_slices; i += 256) slice_table[i] = make_slice_entry((uint32_t)i, df, sdf);
    __syncthreads();
    const InsideConsts inside = make_inside_consts(df, sdf);
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= count) return;
    const f3 p = mk3(positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]);
    const bool in_box = (sdf.table_slices > 0) & (p.x >= sdf.box_x0) & (p.x <= sdf.box_x1) & (p.y >= sdf.box_y0) & (p.y <= sdf.box_y1) &
                        (p.z >= sdf.box_z0) & (p.z <= sdf.box_z1);
    used[i] = in_box ? 1 : 0;
    // positions outside the box keep the general sampler's value, which launch_sdf_sample_inside has already written to out[] (both
    // samplers in one kernel make the backend carry the typed loads' scalar operands through a divergent phi: "illegal VGPR to SGPR copy")
    // No divergent branch around the sampler either (its uniform operands -- tap row bases, the typed loads' resource -- are pinned to
    // scalar registers): lanes outside the box sample the box's centre and drop the result.
    const f3 q = in_box ? p : mk3(0.5f * (sdf.box_x0 + sdf.box_x1), 0.5f * (sdf.box_y0 + sdf.box_y1), 0.5f * (sdf.box_z0 + sdf.box_z1));
    const float value = (sdf.table_slices > 0) ? sample_inside_table<FMT>(q, inside, sdf, slice_table) : 0.0f;
    if (in_box) out[i] = value;
}

hipError_t launch_sdf_sample_inside(const TraceSdfView& sdf, const IlmDistanceFieldUniforms& df, const float* positions, int count, float* out, int32_t* used,
                                    hipStream_t stream, int sdf_filter) {
    if (count <= 0) return hipSuccess;
    const dim3 grid((unsigned)((count + 255) / 256)), block(256);
    const hipError_t general = launch_sdf_sample(sdf, df, positions, count, out, stream, sdf_filter);
    if (general != hipSuccess) return general;
    if (sdf_filter == ILM_SDF_FILTER_FIXED8) {
        if (sdf.format == ILM_SDF_FP16) hipLaunchKernelGGL(sdf_sample_inside_kernel<ILM_SDF_FP16 + kSdfFixed8>, grid, block, 0, stream, sdf, df, positions, count, out, used);
        else hipLaunchKernelGGL(sdf_sample_inside_kernel<ILM_SDF_UNORM16 + kSdfFixed8>, grid, block, 0, stream, sdf, df, positions, count, out, used);
    } else if (sdf_filter != ILM_SDF_FILTER_FP32) return hipErrorInvalidValue;
    else if (sdf.format == ILM_SDF_FP16) hipLaunchKernelGGL(sdf_sample_inside_kernel<ILM_SDF_FP16>, grid, block, 0, stream, sdf, df, positions, count, out, used);
    else hipLaunchKernelGGL(sdf_sample_inside_kernel<ILM_SDF_UNORM16>, grid, block, 0, stream, sdf, df, positions, count, out, used);
    return hipGetLastError();
}

// The cell array of a field (SdfView::cells): cell (v, y, x) = the four taps (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1) of virtual
// slice v's grid, each as the 32-bit channel pair (slice v, slice v + 1) -- exactly the words sample_distance_field's taps would fetch
// from the atlas for a sample whose floor coordinates are (x, y) in that slice (sdf_pair_word).  The last column / row of a slice
// repeat their neighbour (never sampled: the table sampler's box keeps every tap inside the slice).  One thread per cell, 16-byte stores.
__global__ __launch_bounds__(256) void build_sdf_cells_kernel(const uint2* __restrict__ atlas, int atlas_w, int slice_w, int slice_h, int columns, int first_slice,
                                                               uint4* __restrict__ cells) {
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x, y = (int)blockIdx.y, v = first_slice + (int)blockIdx.z;
    if (x >= slice_w) return;
    const uint32_t third = (uint32_t)v / 3u, m = (uint32_t)v - 3u * third;
    const int col = (int)(third % (uint32_t)columns), row = (int)(third / (uint32_t)columns);
    const int ax0 = col * slice_w + x, ax1 = col * slice_w + min(x + 1, slice_w - 1);
    const size_t r0 = (size_t)(row * slice_h + y) * (size_t)atlas_w, r1 = (size_t)(row * slice_h + min(y + 1, slice_h - 1)) * (size_t)atlas_w;
    uint4 c;
    c.x = sdf_pair_word(atlas[r0 + ax0], m); c.y = sdf_pair_word(atlas[r0 + ax1], m);
    c.z = sdf_pair_word(atlas[r1 + ax0], m); c.w = sdf_pair_word(atlas[r1 + ax1], m);
    cells[((size_t)v * (size_t)slice_h + (size_t)y) * (size_t)slice_w + (size_t)x] = c;
}

// (re)builds the cells of virtual slices [first_slice, first_slice + slice_count)
hipError_t launch_build_sdf_cells(const TraceSdfView& sdf, void* cells, int first_slice, int slice_count, hipStream_t stream) {
    if (sdf.table_slices <= 0 || slice_count <= 0) return hipSuccess;
    const dim3 grid((unsigned)((sdf.slice_w + 255) / 256), (unsigned)sdf.slice_h, (unsigned)slice_count), block(256);
    hipLaunchKernelGGL(build_sdf_cells_kernel, grid, block, 0, stream, sdf.texels, sdf.width, sdf.slice_w, sdf.slice_h, sdf.columns, first_slice,
                       reinterpret_cast<uint4*>(cells));
    return hipGetLastError();
}

hipError_t launch_sdf_sample(const SdfView& sdf, const IlmDistanceFieldUniforms& df, const float* positions, int count, float* out, hipStream_t stream,
                             int sdf_filter) {
    if (count <= 0) return hipSuccess;
    const dim3 grid((unsigned)((count + 255) / 256)), block(256);
    if (sdf_filter == ILM_SDF_FILTER_FIXED8) {
        if (sdf.format == ILM_SDF_FP16) hipLaunchKernelGGL(sdf_sample_kernel<ILM_SDF_FP16 + kSdfFixed8>, grid, block, 0, stream, sdf, df, positions, count, out);
        else hipLaunchKernelGGL(sdf_sample_kernel<ILM_SDF_UNORM16 + kSdfFixed8>, grid, block, 0, stream, sdf, df, positions, count, out);
    } else if (sdf_filter != ILM_SDF_FILTER_FP32) return hipErrorInvalidValue;
    else if (sdf.format == ILM_SDF_FP16) hipLaunchKernelGGL(sdf_sample_kernel<ILM_SDF_FP16>, grid, block, 0, stream, sdf, df, positions, count, out);
    else hipLaunchKernelGGL(sdf_sample_kernel<ILM_SDF_UNORM16>, grid, block, 0, stream, sdf, df, positions, count, out);
    return hipGetLastError();
}

// device scratch for the prepared light records, owned by the caller (api.hip)
// the light-side half of the in-volume trace test (see light_flags)
TraceGate make_trace_gate(const IlmDistanceFieldUniforms& df, const SdfView& sdf) {
    TraceGate g;
    const float mx = 0.0625f + df.Extent.x * 0x1p-16f, my = 0.0625f + df.Extent.y * 0x1p-16f, mz = 0.0625f + df.Extent.z * 0x1p-16f;
    g.x0 = sdf.box_x0 + mx; g.x1 = sdf.box_x1 - mx;
    g.y0 = sdf.box_y0 + my; g.y1 = sdf.box_y1 - my;
    g.z0 = sdf.box_z0 + mz; g.z1 = sdf.box_z1 - mz;
    const bool ok = (sdf.table_slices > 0) && (df.Extent.w > 0.0f) && (df.Extent.w <= 0x1p20f) && (df.Extent.x <= 0x1p20f) && (df.Extent.y <= 0x1p20f) &&
                    (df.Extent.z <= 0x1p20f) && (df.StepAndMisc2.x >= 0.0f) && (df.StepAndMisc2.x <= 0x1p23f);
    g.field_ok = ok ? 1.0f : 0.0f;
    return g;
}

hipError_t launch_prepare_lights(const IlmLightVertex* lights, int count, const IlmEnvironment& env, const IlmDistanceFieldUniforms& df,
                                 const SdfView& sdf, void* recs, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(prepare_lights_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, lights, count, env, df.ConeAndMisc.x, make_trace_gate(df, sdf),
                       reinterpret_cast<LightRec*>(recs));
    return hipGetLastError();
}

// block slots per XCD of a launch over `a`'s rows (each slot = one tile of the block -> tile map, padding included)
int light_block_slots(const LightLaunch& a) {
    const int rows = a.row_end - a.row_begin;
    if (rows <= 0 || a.width <= 0) return 0;
    const int tiles_x = (a.width + kTile - 1) / kTile, tiles_y = (rows + kTile - 1) / kTile;
    const int M = a.tile_macro, groups = ((tiles_x + M - 1) / M) * ((tiles_y + M - 1) / M);
    return ((groups + 7) / 8) * M * M;
}

// workgroups the tile kernel is launched with for `a` (split and taper as planned; what SQ_WAVES / 4 of the launch counts)
int light_launch_blocks(const LightLaunch& a) {
    const int slots = light_block_slots(a);
    if (slots <= 0) return 0;
    if (a.split <= 1) return slots * 8;
    return (a.taper[0] + 2 * (a.taper[1] - a.taper[0]) + 4 * (a.taper[2] - a.taper[1]) + 8 * (slots - a.taper[2])) * 8;
}

hipError_t launch_sphere_lights_prepared(const LightLaunch& launch, const void* recs, hipStream_t stream, int sdf_filter) {
    const int rows = launch.row_end - launch.row_begin;
    if (rows <= 0 || launch.width <= 0) return hipSuccess;
    LightLaunch a = launch;
    const int tiles_x = (a.width + kTile - 1) / kTile, tiles_y = (rows + kTile - 1) / kTile;
    const int tile_count = tiles_x * tiles_y;
    const int slots = light_block_slots(a);
    if (a.split <= 1) { a.split = 1; a.taper[0] = a.taper[1] = a.taper[2] = slots; a.taper_slots = slots; }     // one workgroup per tile throughout
    if (a.split > 1 && (a.blend_color != ILM_LIGHT_BLEND_ADD || a.blend_alpha != ILM_LIGHT_BLEND_ADD)) return hipErrorInvalidValue;      // (planned so: the hand-off adds)
    const int t0 = a.taper[0], t1 = a.taper[1], t2 = a.taper[2];
    if (a.taper_slots != slots || t0 < 0 || t0 > t1 || t1 > t2 || t2 > slots) return hipErrorInvalidValue;
    const int per_xcd_blocks = t0 + 2 * (t1 - t0) + 4 * (t2 - t1) + 8 * (slots - t2);
    const LightRec* r = reinterpret_cast<const LightRec*>(recs);
    const bool stats = a.stats != nullptr;
    const bool fp16 = a.sdf.format == ILM_SDF_FP16;
    const dim3 grid(per_xcd_blocks * 8), block(kLightThreads);
    // anything but ADD / ADD: the BLEND instantiation of the same variant
    const bool blend = a.blend_color != ILM_LIGHT_BLEND_ADD || a.blend_alpha != ILM_LIGHT_BLEND_ADD;
    // The field's FIXED8 filter (hlsl_math.hpp, kSdfFixed8): four instantiations -- the format x counting or plain -- of the narrow-binning
    // kernel, for launches of one workgroup per tile in the fp32 model under ADD / ADD (api.hip plans and refuses so)
    if (sdf_filter == ILM_SDF_FILTER_FIXED8) {
        if (a.split > 1 || blend || a.blend_fp16 != 0 || a.light_count_ptr != nullptr) return hipErrorInvalidValue;
        if (fp16 && stats) hipLaunchKernelGGL((sphere_lights_kernel<ILM_SDF_FP16 + kSdfFixed8, true, false>), grid, block, 0, stream, a, r, tiles_x, tiles_y, tile_count);
        else if (fp16) hipLaunchKernelGGL((sphere_lights_kernel<ILM_SDF_FP16 + kSdfFixed8, false, false>), grid, block, 0, stream, a, r, tiles_x, tiles_y, tile_count);
        else if (stats) hipLaunchKernelGGL((sphere_lights_kernel<ILM_SDF_UNORM16 + kSdfFixed8, true, false>), grid, block, 0, stream, a, r, tiles_x, tiles_y, tile_count);
        else hipLaunchKernelGGL((sphere_lights_kernel<ILM_SDF_UNORM16 + kSdfFixed8, false, false>), grid, block, 0, stream, a, r, tiles_x, tiles_y, tile_count);
        return hipGetLastError();
    }
    if (sdf_filter != ILM_SDF_FILTER_FP32) return hipErrorInvalidValue;
#define ILM_LAUNCH_LIGHTS(F, S, W) do { \
        if (blend) hipLaunchKernelGGL((sphere_lights_kernel<F + kBlendVariant, S, W>), grid, block, 0, stream, a, r, tiles_x, tiles_y, tile_count); \
        else hipLaunchKernelGGL((sphere_lights_kernel<F, S, W>), grid, block, 0, stream, a, r, tiles_x, tiles_y, tile_count); } while (0)
    // device-side counts are particle lights: thousands
    const bool wide = (a.light_count_ptr != nullptr) || (a.light_count > 512);
    const int variant = (wide ? 4 : 0) | (fp16 ? 2 : 0) | (stats ? 1 : 0);
    switch (variant) {
        case 0: ILM_LAUNCH_LIGHTS(ILM_SDF_UNORM16, false, false); break;
        case 1: ILM_LAUNCH_LIGHTS(ILM_SDF_UNORM16, true, false); break;
        case 2: ILM_LAUNCH_LIGHTS(ILM_SDF_FP16, false, false); break;
        case 3: ILM_LAUNCH_LIGHTS(ILM_SDF_FP16, true, false); break;
        case 4: ILM_LAUNCH_LIGHTS(ILM_SDF_UNORM16, false, true); break;
        case 5: ILM_LAUNCH_LIGHTS(ILM_SDF_UNORM16, true, true); break;
        case 6: ILM_LAUNCH_LIGHTS(ILM_SDF_FP16, false, true); break;
        default: ILM_LAUNCH_LIGHTS(ILM_SDF_FP16, true, true); break;
    }
#undef ILM_LAUNCH_LIGHTS
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The full-frame light passes (directional, projector, line, volumetric) -- one thread per pixel, one wave per 8 x 8 pixels, a wave-uniform
// loop over the prepared records (uniform index: scalar loads), the G-buffer texel decoded once, the sum in registers, the lightmap texel
// read at most once (accumulate mode) and stored once.  Shared by the five kernels: the store with its mirrors, the statistics and
// the launcher.  Each kernel states its own pixel mapping, base value, blend chains and light loop: as device functions these change
// the instruction streams of the kernels, and the passes then run up to 3 % slower (docs/experiments.md 7.24).  A change to one of
// those parts is made in directional_lights_kernel, projector_lights_kernel, projector_mip_lights_kernel, line_lights_kernel and
// volumetric_lights_kernel alike.  The BLEND instantiations (a launch whose blend functions are not ADD / ADD) are such a change:
// the same three lines in each of the five -- the identities, blend_pair, blend_onto_base -- compiled out where BLEND is false
// (VARIANT = the field format, + kBlendVariant for BLEND).
// ---------------------------------------------------------------------------------------------
// the texel into the lightmap and into every mirror (store-mode exchange of a group lightmap, as the sphere pass)
ILM_DEV void store_light_texel(const LightLaunch& a, size_t o, const float4& v) {
    auto store_texel = [&](void* base) {
        if (a.format == ILM_LIGHTMAP_FLOAT4) store_target<ILM_LIGHTMAP_FLOAT4>(base, o, v);
        else if (a.format == ILM_LIGHTMAP_HALF4) store_target<ILM_LIGHTMAP_HALF4>(base, o, v);
        else store_target<ILM_LIGHTMAP_RGBA8>(base, o, v);
    };
    store_texel(a.lightmap);
    for (int m = 0; m < a.mirror_count; m++) store_texel(a.mirrors[m]);
}

// the wave's statistics: three sums over the lanes, three atomics
ILM_DEV void add_light_stats(LightStats st, unsigned long long* stats, int lane) {
    for (int off = 32; off > 0; off >>= 1) {
        st.samples += __shfl_down(st.samples, off);
        st.pairs += __shfl_down(st.pairs, off);
        st.traced += __shfl_down(st.traced, off);
    }
    if (lane == 0) {
        atomicAdd(&stats[0], st.samples);
        atomicAdd(&stats[1], st.pairs);
        atomicAdd(&stats[2], st.traced);
    }
}

// one workgroup per 16 x 16 tile of the rows; the pass's kernel by field format and by whether the call counts
template <class Rec>
using FullFrameKernel = void (*)(LightLaunch, const Rec*, int);
template <class Rec>
hipError_t launch_full_frame_lights(const LightLaunch& a, const void* recs, hipStream_t stream, FullFrameKernel<Rec> fp16, FullFrameKernel<Rec> fp16_stats,
                                    FullFrameKernel<Rec> unorm16, FullFrameKernel<Rec> unorm16_stats, const FullFrameKernel<Rec> (&blend)[4]) {
    const int rows = a.row_end - a.row_begin;
    if (rows <= 0 || a.width <= 0) return hipSuccess;
    if (a.light_count == 0 && a.accumulate != 0) return hipSuccess;      // nothing to add: no texel (and no mirror) would change
    const int tiles_x = (a.width + kTile - 1) / kTile, tiles_y = (rows + kTile - 1) / kTile;
    const bool stats = a.stats != nullptr;
    FullFrameKernel<Rec> kernel = (a.sdf.format == ILM_SDF_FP16) ? (stats ? fp16_stats : fp16) : (stats ? unorm16_stats : unorm16);
    // anything but ADD / ADD: the BLEND instantiation of the same variant (in the order of the four above)
    if (a.blend_color != ILM_LIGHT_BLEND_ADD || a.blend_alpha != ILM_LIGHT_BLEND_ADD)
        kernel = blend[((a.sdf.format == ILM_SDF_FP16) ? 0 : 2) + (stats ? 1 : 0)];
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(kLightThreads), 0, stream, a, reinterpret_cast<const Rec*>(recs), tiles_x);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Directional lights -- techniques DirectionalLight / DirectionalLightWithRamp, DirectionalLight.fx:19-161, drawn by
// RenderDirectionalLightSource (LightingRenderer.cs:1256-1307) as one full-frame (or Bounds-sized) quad per light.
// A footprint is a rectangle: no tile lists, no light split -- one thread per pixel, one wave per 8 x 8 pixels, the light loop is
// wave-uniform over the prepared records (uniform index: scalar loads), the G-buffer texel is decoded once, the sum lives in
// registers, the lightmap texel is read at most once (accumulate mode) and stored once.  The trace is the general loop
// (cone_trace_loop<.., false>): the in-volume loop is not built for this pass (docs/experiments.md 7.21 has what it costs: about
// twice the vector instructions per sample).
// ---------------------------------------------------------------------------------------------
constexpr float kDirectionalDotOffset = 0.35f;          // LightCommon.fxh:7 DIRECTIONAL_DOT_OFFSET
constexpr float kDirectionalDotRampRange = 0.35f;       // LightCommon.fxh:8 DIRECTIONAL_DOT_RAMP_RANGE
constexpr float kDirectionalSelfOcclusionHack = 1.5f;   // DirectionalLight.fx:13 SELF_OCCLUSION_HACK
constexpr float kDirectionalTraceThreshold = 1.0f / 256.0f;      // DirectionalLight.fx:73 (lightOpacity >= 1 / 256.0)
constexpr float kDirectionalMinimumW = 0.1f;            // DirectionalLight.fx:73, LightCommon.fxh:227 (lightDirection.w < 0.1: no direction)

struct DirectionalRec {
    float x0, y0, x1, y1;                                       // footprint in screen pixels: centre in [x0, x1) x [y0, y1)
    float dir_x, dir_y, dir_z, dir_w;                           // Color2
    float casts_shadows, trace_length, softness, shadow_filter; // LightProperties.xyz, EvenMoreLightProperties.x
    float ao_radius, ao_opacity, cfg_x, cfg_y;                  // MoreLightProperties.xw; createTraceConfig: maxRadius, radiusGrowthPerPixel
    float col_r, col_g, col_b, _pad0;                           // Color1.rgb * Color1.a
    float _pad[12];
};
static_assert(sizeof(DirectionalRec) == kLightRecBytes, "a directional record fills the slot of a LightRec (reserve_light_recs)");

// DirectionalLightVertexShader (DirectionalLight.fx:32-34) at the quad's two extreme corners + createTraceConfig (ConeTrace.fxh:122-139)
// with lightRamp = (ShadowSoftness, shadowDistanceFalloff) and cone growth = ShadowRampRate (DirectionalLight.fx:77-80)
__global__ __launch_bounds__(64) void prepare_directional_lights_kernel(const IlmLightVertex* __restrict__ lights, int count, IlmEnvironment env,
                                                                         float max_cone_radius, DirectionalRec* __restrict__ out) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= count) return;
    const IlmLightVertex L = lights[i];
    DirectionalRec r = {};
    const float sx = env.GBufferTexelSizeAndMisc.z * env.ZAndScale.z, sy = env.GBufferTexelSizeAndMisc.w * env.ZAndScale.w;
    r.x0 = (L.LightPosition1.x - env.ViewportPosition[0]) * sx; r.y0 = (L.LightPosition1.y - env.ViewportPosition[1]) * sy;
    r.x1 = (L.LightPosition2.x - env.ViewportPosition[0]) * sx; r.y1 = (L.LightPosition2.y - env.ViewportPosition[1]) * sy;
    r.dir_x = L.Color2.x; r.dir_y = L.Color2.y; r.dir_z = L.Color2.z; r.dir_w = L.Color2.w;
    r.casts_shadows = L.LightProperties.x; r.trace_length = L.LightProperties.y; r.softness = L.LightProperties.z;
    r.shadow_filter = L.EvenMoreLightProperties.x;
    r.ao_radius = L.MoreLightProperties.x; r.ao_opacity = L.MoreLightProperties.w;
    const float max_radius = clampf(L.LightProperties.z, ref::kMinConeRadius, max_cone_radius);
    r.cfg_x = max_radius;
    r.cfg_y = max_radius / fmaxf(L.MoreLightProperties.y, 16.0f) * L.LightProperties.w;
    r.col_r = L.Color1.x * L.Color1.w; r.col_g = L.Color1.y * L.Color1.w; r.col_b = L.Color1.z * L.Color1.w;
    out[i] = r;
}

// SampleFromRamp (RampCommon.fxh:15-17): channel r at (x, v = 0) through RampTextureSampler -- the sphere pass's lookup (shade_light:
// tex2Dlod level 0, LINEAR, U CLAMP, V WRAP) with its v fixed at 0.  A COPY of shade_light's tap and weight arithmetic, to be kept in
// step with it: one helper for both was built in two forms (taps returned in a struct; columns, rows and weights through references) and
// each changed the instruction streams of sphere_lights_kernel and light_probes_kernel (tools/isa_compare.py: 10 of 21 kernels `diff`,
// same instruction counts, another schedule), which the existing passes are held not to do.  tests/test_directional_gpu.py holds this
// copy to the oracle's lookup, tests/test_lighting_gpu.py the other.
ILM_DEV float sample_from_ramp(const RampView& ramp, float u) {
    const int w = ramp.width, h = ramp.height;
    const float sx = u * (float)w - 0.5f, sy = 0.0f * (float)h - 0.5f;
    float x0f = floorf(sx);
    const float y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    float x1f = x0f + 1.0f;
    x0f = (x0f >= 0.0f) ? x0f : 0.0f; x0f = fminf(x0f, (float)(w - 1));
    x1f = (x1f >= 0.0f) ? x1f : 0.0f; x1f = fminf(x1f, (float)(w - 1));
    const int x0 = (int)x0f, x1 = (int)x1f;
    const int y0 = wrap_index(y0f, h), y1 = (y0 + 1 == h) ? 0 : y0 + 1;
    return lerp(lerp(ramp.texels[y0 * w + x0].x, ramp.texels[y0 * w + x1].x, fx), lerp(ramp.texels[y1 * w + x0].x, ramp.texels[y1 * w + x1].x, fx), fy);
}

// One directional light on one shaded point: DirectionalLightPixelShader / ...WithRamp (DirectionalLight.fx:95-161) over
// DirectionalLightPixelCore (:52-93), after the footprint test.  Returns false when the shader discards (fullbright, the shadow
// filter, clip(!visible)); otherwise the opacity that multiplies color.rgb * color.a.  Unlike the sphere light's shader this one has no
// opacity discard: a visible pixel with opacity 0 is blended (alpha + 1).
template <int FMT, bool STATS>
ILM_DEV bool shade_directional(const Pixel& P, const DirectionalRec& L, const TraceField& F, bool have_sdf, const RampView& ramp, LightStats& st,
                               float& opacity) {
    const bool filtered = (L.shadow_filter < 0.0f) ? false : ((L.shadow_filter > 0.5f) != P.enable_shadows);      // checkShadowFilter, LightCommon.fxh:146-152
    if (P.fullbright || filtered)
        return false;
    const bool visible = P.shaded.x > -9999.0f;
    if (!visible)      // clip(visible ? 1 : -1), :91 -- nothing the core computes for such a pixel is seen
        return false;
    const float casts = L.casts_shadows * (P.enable_shadows ? 1.0f : 0.0f);
    const bool directed = L.dir_w >= kDirectionalMinimumW;
    // computeDirectionalLightOpacity -> computeNormalFactorEx, LightCommon.fxh:154-165,224-231
    float light_opacity = 1.0f;
    if (directed && ((P.normal.x != 0.0f) || (P.normal.y != 0.0f) || (P.normal.z != 0.0f))) {
        const float d = dot3(mk3(L.dir_x, L.dir_y, L.dir_z) * -1.0f, P.normal);
        light_opacity = pow_pos(sat((d + kDirectionalDotOffset) / kDirectionalDotRampRange), ref::kDotExponent);
    }
    // computeAO, AOCommon.fxh:1-19 (aoRadius scaled by max(0, normal.z), :68)
    const float ao_radius = L.ao_radius * fmaxf(0.0f, P.normal.z);
    if ((ao_radius >= 0.5f) && have_sdf) {
        const float distance = sample_distance_field<FMT>(mk3(P.shaded.x, P.shaded.y, P.shaded.z + P.normal.z * ao_radius), F.df, F.sdf);
        if (STATS) st.samples++;
        float r = 1.0f - sat(clampf(distance, 0.0f, ao_radius) / ao_radius);
        r *= r;
        r = 1.0f - r;
        light_opacity *= (1.0f - L.ao_opacity) + (r * L.ao_opacity);
    }
    // coneTrace towards the fake light centre, :73-83 + ConeTrace.fxh:141-191
    const bool trace = (casts != 0.0f) && (light_opacity >= kDirectionalTraceThreshold) && directed;
    if (trace) {
        if (STATS && have_sdf) st.traced++;
        f3 start = P.shaded + (P.normal * kDirectionalSelfOcclusionHack);
        const f3 centre = P.shaded - (mk3(L.dir_x, L.dir_y, L.dir_z) * L.trace_length);
        const f3 tv = centre - start;
        const float trace_length = len3(tv);
        const float data_y = fmaxf(trace_length - L.softness, 1.0f);
        float data_x = ref::kTraceInitialOffsetPx;
        float data_z = 1.0f;
        const float cfg_z = fmaxf(1.0f, F.df.Packed1.w);
        float steps_remaining = F.df.StepAndMisc2.x;
        // (two VGPRs keep the cone configuration resident across the loop, as in shade_light)
        float cone_max_radius = L.cfg_x, cone_growth = L.cfg_y;
        asm volatile("" : "+v"(cone_max_radius), "+v"(cone_growth));
        f3 dir = mk3(tv.x / trace_length, tv.y / trace_length, tv.z / trace_length);
        // (the sampler treats a NaN coordinate as 0: hoisted as in shade_light's general path)
        if ((start.x != start.x) || (dir.x != dir.x)) { start.x = 0.0f; dir.x = 0.0f; }
        if ((start.y != start.y) || (dir.y != dir.y)) { start.y = 0.0f; dir.y = 0.0f; }
        if ((start.z != start.z) || (dir.z != dir.z)) { start.z = 0.0f; dir.z = 0.0f; }
        cone_trace_loop<FMT, STATS, false>(start, dir, data_y, cfg_z, cone_growth, cone_max_radius, F, data_x, data_z, steps_remaining, have_sdf, st);
        const float visibility = fminf(data_z, steps_remaining / ref::kMaxStepRampWindow);
        light_opacity *= pow_pos(sat(div_with_rcp(sat(visibility - ref::kFullyShadowedThreshold), kVisibilityRange, kVisibilityRangeRcp)), F.df.ConeAndMisc.z);
    }
    if (ramp.texels != nullptr)
        light_opacity = sample_from_ramp(ramp, light_opacity);
    opacity = light_opacity;
    return true;
}

template <int VARIANT, bool STATS>
__global__ __launch_bounds__(kLightThreads) void directional_lights_kernel(const LightLaunch a, const DirectionalRec* __restrict__ recs, int tiles_x) {
    constexpr int FMT = VARIANT & ~kBlendVariant;
    constexpr bool BLEND = (VARIANT & kBlendVariant) != 0;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int tile_x = (int)blockIdx.x % tiles_x, tile_y = (int)blockIdx.x / tiles_x;
    const int px = tile_x * kTile + (wave & 1) * 8 + (lane & 7);
    const int py = a.row_begin + tile_y * kTile + (wave >> 1) * 8 + (lane >> 3);
    const bool in_image = (px < a.width) && (py < a.row_end);
    if (__builtin_amdgcn_ballot_w64(in_image) == 0ull)
        return;
    Pixel P = sample_gbuffer((float)px, (float)py, a.env, a.gbuffer);
    P.origin_x = 0; P.origin_y = 0; P.start_inside = false;
    const float cxp = (float)px + 0.5f, cyp = (float)py + 0.5f;
    const bool have_sdf = (a.sdf.texels != nullptr) && (a.df.Extent.x > 0.0f);
    const InsideConsts no_table = {};
    const TraceField field = { a.df, a.sdf, no_table, nullptr };
    const size_t o = (size_t)py * (size_t)a.width + (size_t)px;
    auto through_half = [](float v) { return __half2float(__float2half_rn(v)); };
    // what the lights are added to: the clear colour, or the lightmap's contents; in the fp16-per-light model it passes through fp16
    // and starts the chain of roundings, otherwise the call's sum (from zero, in list order) is added to it at the end
    auto base_value = [&]() -> float4 {
        float4 v = mk4(a.ambient[0], a.ambient[1], a.ambient[2], a.ambient[3]);
        if (a.accumulate != 0 && in_image) {
            if (a.format == ILM_LIGHTMAP_FLOAT4) v = load_target<ILM_LIGHTMAP_FLOAT4>(a.lightmap, o);
            else if (a.format == ILM_LIGHTMAP_HALF4) v = load_target<ILM_LIGHTMAP_HALF4>(a.lightmap, o);
            else v = load_target<ILM_LIGHTMAP_RGBA8>(a.lightmap, o);
        }
        if (a.blend_fp16 != 0) v = mk4(through_half(v.x), through_half(v.y), through_half(v.z), through_half(v.w));
        return v;
    };
    const bool blend_fp16 = a.blend_fp16 != 0;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, acc_a = 0.0f;
    if constexpr (BLEND) { acc_r = acc_g = acc_b = blend_identity(a.blend_color); acc_a = blend_identity(a.blend_alpha); }
    if (blend_fp16) { const float4 v = base_value(); acc_r = v.x; acc_g = v.y; acc_b = v.z; acc_a = v.w; }
    LightStats st;
    const int light_count = a.light_count;
    for (int k = 0; k < light_count; k++) {
        const DirectionalRec& L = recs[k];
        const float x0 = L.x0, y0 = L.y0, x1 = L.x1, y1 = L.y1;
        const bool covered = in_image & (cxp >= x0) & (cxp < x1) & (cyp >= y0) & (cyp < y1);
        // a wave none of whose lanes the light covers leaves on a scalar branch (r06's finding for particle lights)
        if (__builtin_amdgcn_ballot_w64(covered) == 0ull)
            continue;
        if (!covered)
            continue;
        if (STATS) st.pairs++;
        float opacity;
        if (!shade_directional<FMT, STATS>(P, L, field, have_sdf, a.ramp, st, opacity))
            continue;
        const float cr = L.col_r * opacity, cg = L.col_g * opacity, cb = L.col_b * opacity;
        if constexpr (BLEND) {
            blend_pair(a.blend_color, a.blend_alpha, blend_fp16, cr, cg, cb, acc_r, acc_g, acc_b, acc_a);
        } else if (blend_fp16) {
            acc_r = through_half(acc_r + through_half(cr));
            acc_g = through_half(acc_g + through_half(cg));
            acc_b = through_half(acc_b + through_half(cb));
            acc_a = through_half(acc_a + 1.0f);
        } else {
            acc_r += cr; acc_g += cg; acc_b += cb; acc_a += 1.0f;
        }
    }
    if (!blend_fp16) {
        const float4 v = base_value();
        if constexpr (BLEND) {
            acc_r = blend_onto_base(a.blend_color, v.x, acc_r); acc_g = blend_onto_base(a.blend_color, v.y, acc_g);
            acc_b = blend_onto_base(a.blend_color, v.z, acc_b); acc_a = blend_onto_base(a.blend_alpha, v.w, acc_a);
        } else {
            acc_r = v.x + acc_r; acc_g = v.y + acc_g; acc_b = v.z + acc_b; acc_a = v.w + acc_a;
        }
    }
    if (in_image) {
        const float4 v = mk4(acc_r, acc_g, acc_b, acc_a);
        store_light_texel(a, o, v);
    }
    if (STATS) add_light_stats(st, a.stats, lane);
}

hipError_t launch_prepare_directional_lights(const IlmLightVertex* lights, int count, const IlmEnvironment& env, const IlmDistanceFieldUniforms& df,
                                             void* recs, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(prepare_directional_lights_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, lights, count, env, df.ConeAndMisc.x,
                       reinterpret_cast<DirectionalRec*>(recs));
    return hipGetLastError();
}

hipError_t launch_directional_lights_prepared(const LightLaunch& a, const void* recs, hipStream_t stream) {
    static const FullFrameKernel<DirectionalRec> blend[4] = { directional_lights_kernel<ILM_SDF_FP16 + kBlendVariant, false>, directional_lights_kernel<ILM_SDF_FP16 + kBlendVariant, true>,
                                                  directional_lights_kernel<ILM_SDF_UNORM16 + kBlendVariant, false>, directional_lights_kernel<ILM_SDF_UNORM16 + kBlendVariant, true> };
    return launch_full_frame_lights<DirectionalRec>(a, recs, stream, directional_lights_kernel<ILM_SDF_FP16, false>, directional_lights_kernel<ILM_SDF_FP16, true>,
                                           directional_lights_kernel<ILM_SDF_UNORM16, false>, directional_lights_kernel<ILM_SDF_UNORM16, true>, blend);
}

// ---------------------------------------------------------------------------------------------
// Directional light probes -- DirectionalLightProbePixelShader / ...WithRampPixelShader, DirectionalLight.fx:163-219: the core of
// the frame pass (shade_directional) on a Pixel built from the probe, inside light_probes_kernel's frame (DirectionalProbes below).
// The records are the frame pass's (prepare_directional_lights_kernel); their footprint is not read (the probe vertex shader covers
// the target, :39-50, "FIXME: Clip to region" :175).
// ---------------------------------------------------------------------------------------------
template <int FMT>
ILM_DEV bool probe_directional(const float4 pp, const float4 pn, DirectionalRec L, const TraceField& field, bool have_sdf, const RampView& ramp,
                               float& opacity) {
    Pixel P;
    P.shaded = xyz(pp); P.normal = xyz(pn); P.origin_x = 0; P.origin_y = 0;
    P.fullbright = false;
    P.start_inside = false;
    // lightProperties.x *= enableShadows (a float here, not the G-buffer's flag); moreLightProperties.x = .w = 0: no AO (:182-183); the
    // probe shaders do not take evenMoreLightProperties: no shadow filter
    L.casts_shadows *= pn.w;
    P.enable_shadows = true;
    L.ao_radius = 0.0f; L.ao_opacity = 0.0f;
    L.shadow_filter = -1.0f;
    LightStats st;
    return shade_directional<FMT, false>(P, L, field, have_sdf, ramp, st, opacity);
}

struct DirectionalProbes {      // ilm_render_directional_light_probes; env is not read, and shade_directional reads no InsideConsts
    using Rec = DirectionalRec;
    static constexpr bool kInsideConsts = false;
    template <int FMT>
    static ILM_DEV bool shade(const float4 pp, const float4 pn, const DirectionalRec& L, const IlmEnvironment&, const TraceField& field, bool have_sdf,
                              const RampView& ramp, float& cr, float& cg, float& cb) {
        float opacity;
        if (!probe_directional<FMT>(pp, pn, L, field, have_sdf, ramp, opacity))
            return false;
        cr = L.col_r * opacity; cg = L.col_g * opacity; cb = L.col_b * opacity;
        return true;
    }
};

// The launcher of every probe kind (the line kind's records are sphere records): the pair form when there is scratch, more than one light
// and a grid for them, then the sum in light order; else the one-kernel form.  `env` is not read by the directional kind.
template <typename KIND>
static hipError_t launch_light_probes_of(const void* recs, int light_count, const float4* probe_positions, const float4* probe_normals, int probe_count,
                                         const IlmEnvironment& env, const IlmDistanceFieldUniforms& df, const SdfView& sdf, const RampView& ramp,
                                         float4* values, float4* pairs, hipStream_t stream) {
    const bool by_pair = (pairs != nullptr) && (light_count > 1) && (light_count <= 65535);
    const dim3 grid((unsigned)((probe_count + 63) / 64), by_pair ? (unsigned)light_count : 1u), block(64);
    const typename KIND::Rec* r = reinterpret_cast<const typename KIND::Rec*>(recs);
    float4* p = by_pair ? pairs : nullptr;
    if (sdf.format == ILM_SDF_FP16)
        hipLaunchKernelGGL((light_probes_kernel<ILM_SDF_FP16, KIND>), grid, block, 0, stream, r, light_count, probe_positions, probe_normals, probe_count, env, df, sdf, ramp, values, p);
    else
        hipLaunchKernelGGL((light_probes_kernel<ILM_SDF_UNORM16, KIND>), grid, block, 0, stream, r, light_count, probe_positions, probe_normals, probe_count, env, df, sdf, ramp, values, p);
    if (by_pair)
        hipLaunchKernelGGL(light_probes_sum_kernel, dim3((unsigned)((probe_count + 63) / 64)), block, 0, stream, p, light_count, probe_count, values);
    return hipGetLastError();
}

hipError_t launch_light_probes(bool directional, const void* recs, int light_count, const float4* probe_positions, const float4* probe_normals,
                               int probe_count, const IlmEnvironment& env, const IlmDistanceFieldUniforms& df, const SdfView& sdf, const RampView& ramp,
                               float4* values, float4* pairs, hipStream_t stream) {
    if (probe_count <= 0) return hipSuccess;
    return directional ? launch_light_probes_of<DirectionalProbes>(recs, light_count, probe_positions, probe_normals, probe_count, env, df, sdf, ramp, values, pairs, stream)
                       : launch_light_probes_of<SphereProbes>(recs, light_count, probe_positions, probe_normals, probe_count, env, df, sdf, ramp, values, pairs, stream);
}

// ---------------------------------------------------------------------------------------------
// Projector lights -- technique ProjectorLight, ProjectorLight.fx:14-56 over ProjectorLightCore.fxh:20-151,290-302, drawn by
// RenderProjectorLightSource (LightingRenderer.cs:1386-1446) as one quad per light: the whole frame for a wrapping light, the bounding
// box of the projector's volume for a clamped one (ProjectorLightVertexShader, ProjectorLightCore.fxh:251-278).  The frame of the
// directional pass: one thread per pixel, one wave per 8 x 8 pixels, a wave-uniform loop over the prepared records (scalar loads: the
// 16 matrix entries of a light cost no vector registers), the G-buffer texel decoded once, the sum in registers, one store.  The
// shadow is the sphere light's trace towards one point in its general form (cone_trace_loop<.., false>); the group's texture (LINEAR,
// WRAP on both axes) travels in the launch descriptor's `ramp` member, which this pass reads as nothing else.  A texture bound with
// more than one level (ilm_ctx_set_projector_texture_mips) runs the MIPS instantiations: the record then names the light's two levels
// and the weight between them (prepare_projector_mips_kernel), all wave-uniform -- scalar loads, a scalar branch at weight 0.
// ---------------------------------------------------------------------------------------------
constexpr float kProjectorSelfOcclusionHack = 1.5f;              // ProjectorLightCore.fxh:7 SELF_OCCLUSION_HACK
constexpr float kProjectorTraceThreshold = 0.75f / 255.0f;       // ProjectorLightCore.fxh:8 SHADOW_OPACITY_THRESHOLD
constexpr float kProjectorEdgeThreshold = 0.001f;                // ProjectorLightCore.fxh:62
constexpr float kProjectorEdgeScale = 1.0f / 0.001f;             // (1 / threshold), :63 -- the fp32 quotient

struct ProjectorRec {
    float x0, y0, x1, y1;                                       // footprint in screen pixels: centre in [x0, x1) x [y0, y1)
    float m[16];                                                // rows 1-4 of the inverse matrix, m[15] = 1 (the mip bias: lod_* below)
    float origin_x, origin_y, origin_z, origin_w;               // LightPosition3
    float region_x0, region_y0, region_x1, region_y1;           // EvenMoreLightProperties
    float clamp, opacity, ao_radius, ao_opacity;                // MoreLightProperties.z, .y, .x, .w
    float shadows, radius, cfg_x, cfg_y;                        // LightProperties.w, .x; createTraceConfig: maxRadius, radiusGrowthPerPixel
    // the explicit LOD (Color2.w) over the bound chain, written by prepare_projector_mips_kernel alone (one level: all zero, not
    // read): levels l0 and l1 = min(l0 + 1, L - 1), the weight of l1, and each level's first texel, width and height from the host's table
    int32_t lod_l0, lod_l1; float lod_f;
    int32_t l0_offset, l0_width, l0_height, l1_offset, l1_width, l1_height;
    float _pad[3];
};
static_assert(sizeof(ProjectorRec) == kProjectorRecBytes, "a projector record is 192 bytes (internal.hpp: one and a half slots of reserve_light_recs)");

// invertMatrix (ProjectorLightCore.fxh:155-192) as a table: entry [i][j] of the result is the sum of six signed triple products,
// added in the order the shader writes them, times 1 / det.  A term +-abcdef names the factors n_ab * n_cd * n_ef with the shader's
// n_rc = m[c - 1][r - 1]; entries [i][0] are its t11 .. t14, and det = n11 t11 + n21 t12 + n31 t13 + n41 t14.
__constant__ const int kInverseTerms[16][6] = {
    { 233442, -243342, 243243, -223443, -233244, 223344 }, { 243341, -233441, -243143, 213443, 233144, -213344 },
    { 223441, -243241, 243142, -213442, -223144, 213244 }, { 233241, -223341, -233142, 213342, 223143, -213243 },
    { 143342, -133442, -143243, 123443, 133244, -123344 }, { 133441, -143341, 143143, -113443, -133144, 113344 },
    { 143241, -123441, -143142, 113442, 123144, -113244 }, { 123341, -133241, 133142, -113342, -123143, 113243 },
    { 132442, -142342, 142243, -122443, -132244, 122344 }, { 142341, -132441, -142143, 112443, 132144, -112344 },
    { 122441, -142241, 142142, -112442, -122144, 112244 }, { 132241, -122341, -132142, 112342, 122143, -112243 },
    { 142332, -132432, -142233, 122433, 132234, -122334 }, { 132431, -142331, 142133, -112433, -132134, 112334 },
    { 142231, -122431, -142132, 112432, 122134, -112234 }, { 122331, -132231, 132132, -112332, -122133, 112233 },
};
ILM_DEV void invert_matrix(const float (&m)[16], float (&out)[16]) {
    auto n = [&](int rc) { return m[(rc % 10 - 1) * 4 + (rc / 10 - 1)]; };
    float sums[16];
    for (int e = 0; e < 16; e++) {
        float acc = 0.0f;
        for (int t = 0; t < 6; t++) {
            const int code = kInverseTerms[e][t], a = code < 0 ? -code : code;
            const float product = (n(a / 10000) * n((a / 100) % 100)) * n(a % 100);
            acc = (t == 0) ? product : ((code < 0) ? (acc - product) : (acc + product));
        }
        sums[e] = acc;
    }
    const float det = ((n(11) * sums[0] + n(21) * sums[4]) + n(31) * sums[8]) + n(41) * sums[12];
    const float idet = 1.0f / det;
    for (int e = 0; e < 16; e++) out[e] = sums[e] * idet;
}

// component c of mul(float4(x, y, z, 1), M), M's rows in m[0..3], [4..7], [8..11], [12..15]
ILM_DEV float row_times_matrix(const float (&m)[16], int c, float x, float y, float z) {
    return ((x * m[c] + y * m[4 + c]) + z * m[8 + c]) + 1.0f * m[12 + c];
}

// ProjectorLightVertexShader (ProjectorLightCore.fxh:244-287) at the quad's two extreme corners + createTraceConfig
// (ConeTrace.fxh:122-139) with lightRamp = (Radius, RampLength) and cone growth getConeGrowthFactor() == 1
__global__ __launch_bounds__(64) void prepare_projector_lights_kernel(const IlmLightVertex* __restrict__ lights, int count, IlmEnvironment env,
                                                                       float max_cone_radius, ProjectorRec* __restrict__ out) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= count) return;
    const IlmLightVertex L = lights[i];
    ProjectorRec r = {};
    const IlmFloat4 rows[4] = { L.LightPosition1, L.LightPosition2, L.Color1, L.Color2 };
    for (int k = 0; k < 4; k++) { r.m[k * 4] = rows[k].x; r.m[k * 4 + 1] = rows[k].y; r.m[k * 4 + 2] = rows[k].z; r.m[k * 4 + 3] = rows[k].w; }
    r.m[15] = 1.0f;                                   // mat4.w carries the mip bias; the matrix's m44 is 1 (:244-245)
    r.origin_x = L.LightPosition3.x; r.origin_y = L.LightPosition3.y; r.origin_z = L.LightPosition3.z; r.origin_w = L.LightPosition3.w;
    r.region_x0 = L.EvenMoreLightProperties.x; r.region_y0 = L.EvenMoreLightProperties.y;
    r.region_x1 = L.EvenMoreLightProperties.z; r.region_y1 = L.EvenMoreLightProperties.w;
    r.clamp = L.MoreLightProperties.z; r.opacity = L.MoreLightProperties.y;
    r.ao_radius = L.MoreLightProperties.x; r.ao_opacity = L.MoreLightProperties.w;
    r.shadows = L.LightProperties.w; r.radius = L.LightProperties.x;
    const float max_radius = clampf(L.LightProperties.x, ref::kMinConeRadius, max_cone_radius);
    r.cfg_x = max_radius;
    r.cfg_y = max_radius / fmaxf(L.LightProperties.y, 16.0f) * 1.0f;

    float wx0, wy0, wx1, wy1;                         // the quad's world rectangle
    if (r.clamp > 0.5f) {
        float world[16];
        invert_matrix(r.m, world);
        const float sx = r.region_x1 - r.region_x0, sy = r.region_y1 - r.region_y0;
        float tlx = 999999.0f, tly = 999999.0f, brx = -999999.0f, bry = -999999.0f;
        for (int k = 0; k < 4; k++) {
            const float cx = (k == 1 || k == 2) ? 1.0f : 0.0f, cy = (k >= 2) ? 1.0f : 0.0f;      // LightCorners, LightCommon.fxh:12-17
            const float ix = lerp(0.0f, sx, cx), iy = lerp(0.0f, sy, cy);
            // projectBoundingBoxEdge (:194-221): the corner at z = 0 and z = 1, each divided by its w
            const float w1 = row_times_matrix(world, 3, ix, iy, 0.0f), w2 = row_times_matrix(world, 3, ix, iy, 1.0f);
            const float ax = row_times_matrix(world, 0, ix, iy, 0.0f) / w1, ay = row_times_matrix(world, 1, ix, iy, 0.0f) / w1;
            const float bx = row_times_matrix(world, 0, ix, iy, 1.0f) / w2, by = row_times_matrix(world, 1, ix, iy, 1.0f) / w2;
            const float px = lerp(fminf(ax, bx), fmaxf(ax, bx), cx), py = lerp(fminf(ay, by), fmaxf(ay, by), cy);
            tlx = fminf(tlx, px); tly = fminf(tly, py); brx = fmaxf(brx, px); bry = fmaxf(bry, py);
        }
        const float z_offset = env.ZAndScale.y * env.ZToY.x;
        wx0 = lerp(tlx, brx, 0.0f); wx1 = lerp(tlx, brx, 1.0f);
        wy0 = lerp(tly, bry, 0.0f) + (z_offset * ((0.0f * 2.0f) - 1.0f));
        wy1 = lerp(tly, bry, 1.0f) + (z_offset * ((1.0f * 2.0f) - 1.0f));
    } else {
        wx0 = lerp(-9999.0f, 9999.0f, 0.0f); wx1 = lerp(-9999.0f, 9999.0f, 1.0f);
        wy0 = wx0; wy1 = wx1;
    }
    const float scale_x = env.GBufferTexelSizeAndMisc.z * env.ZAndScale.z, scale_y = env.GBufferTexelSizeAndMisc.w * env.ZAndScale.w;
    r.x0 = (wx0 - env.ViewportPosition[0]) * scale_x; r.y0 = (wy0 - env.ViewportPosition[1]) * scale_y;
    r.x1 = (wx1 - env.ViewportPosition[0]) * scale_x; r.y1 = (wy1 - env.ViewportPosition[1]) * scale_y;
    out[i] = r;
}

// ... and, for a texture of mips.levels > 1 levels, a second kernel behind it on the stream fills in the record's lod_* members: the
// light's LOD = Color2.w (RenderProjectorLightSource, LightingRenderer.cs:1417-1428) resolved against the chain -- c = min(max(lod, 0),
// L - 1), where a NaN becomes 0 through fmaxf and an infinity clamps; l0 = floor(c), f = c - floor(c), l1 = min(l0 + 1, L - 1) -- and
// both levels' rows of the host's table.  The table arrives by value (kernel arguments: scalar registers) and is walked with compares,
// not indexed, so it stays there.  A kernel of its own: prepare_projector_lights_kernel keeps the instruction stream it had.
__global__ __launch_bounds__(64) void prepare_projector_mips_kernel(const IlmLightVertex* __restrict__ lights, int count, const ProjectorMips mips,
                                                                     ProjectorRec* __restrict__ out) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= count) return;
    const float c = fminf(fmaxf(lights[i].Color2.w, 0.0f), (float)(mips.levels - 1));
    const float whole = floorf(c);
    const int l0 = (int)whole, l1 = (l0 + 1 < mips.levels) ? l0 + 1 : mips.levels - 1;
    ProjectorRec& r = out[i];
    r.lod_l0 = l0; r.lod_l1 = l1; r.lod_f = c - whole;
    for (int l = 0; l < kMaxProjectorLevels; l++) {
        if (l == l0) { r.l0_offset = mips.offset[l]; r.l0_width = mips.width[l]; r.l0_height = mips.height[l]; }
        if (l == l1) { r.l1_offset = mips.offset[l]; r.l1_width = mips.width[l]; r.l1_height = mips.height[l]; }
    }
}

// tex2Dlod(ProjectorTextureSampler, (u, v, 0, mip)) on a one-level texture: LINEAR, WRAP on both axes.  The tap and weight arithmetic
// of the ramp lookup's V axis (shade_light) on both axes: the second tap is the integer first tap + 1 wrapped, wrap_index is exact for
// every finite float and names tap 0 for a non-finite one -- every index lies inside the texture by integer arithmetic.
ILM_DEV float4 sample_projector_texture(const RampView& tex, float u, float v) {
    const int w = tex.width, h = tex.height;
    const float sx = u * (float)w - 0.5f, sy = v * (float)h - 0.5f;
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    const int x0 = wrap_index(x0f, w), x1 = (x0 + 1 == w) ? 0 : x0 + 1;
    const int y0 = wrap_index(y0f, h), y1 = (y0 + 1 == h) ? 0 : y0 + 1;
    const float4 t00 = tex.texels[y0 * w + x0], t10 = tex.texels[y0 * w + x1], t01 = tex.texels[y1 * w + x0], t11 = tex.texels[y1 * w + x1];
    return lerp4(lerp4(t00, t10, fx), lerp4(t01, t11, fx), fy);
}

// The same fetch with the explicit LOD over a chain (MipFilter LINEAR): sample_projector_texture's taps and weights on level l0 with
// that level's own size and, unless the weight f is 0, on level l1; the texel is c0 + (c1 - c0) * f.  At f == 0 -- one level read: an
// integral or a clamped LOD -- level l1 is not touched, so nothing of it (a NaN texel) can show.  l0, l1 and f are the light's, hence
// wave-uniform: the branch is a scalar one.  With two levels all eight taps are issued before the first lerp, to be in flight together.
struct ProjectorTaps { int i00, i10, i01, i11; float fx, fy; };
ILM_DEV ProjectorTaps projector_taps(int w, int h, float u, float v) {
    const float sx = u * (float)w - 0.5f, sy = v * (float)h - 0.5f;
    const float x0f = floorf(sx), y0f = floorf(sy);
    const int x0 = wrap_index(x0f, w), x1 = (x0 + 1 == w) ? 0 : x0 + 1;
    const int y0 = wrap_index(y0f, h), y1 = (y0 + 1 == h) ? 0 : y0 + 1;
    return { y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1, sx - x0f, sy - y0f };
}
ILM_DEV float4 sample_projector_mips(const RampView& tex, const ProjectorRec& L, float u, float v) {
    const float4* level0 = tex.texels + L.l0_offset;
    const ProjectorTaps a = projector_taps(L.l0_width, L.l0_height, u, v);
    if (L.lod_f == 0.0f) {
        const float4 t00 = level0[a.i00], t10 = level0[a.i10], t01 = level0[a.i01], t11 = level0[a.i11];
        return lerp4(lerp4(t00, t10, a.fx), lerp4(t01, t11, a.fx), a.fy);
    }
    const float4* level1 = tex.texels + L.l1_offset;
    const ProjectorTaps b = projector_taps(L.l1_width, L.l1_height, u, v);
    const float4 a00 = level0[a.i00], a10 = level0[a.i10], a01 = level0[a.i01], a11 = level0[a.i11];
    const float4 b00 = level1[b.i00], b10 = level1[b.i10], b01 = level1[b.i01], b11 = level1[b.i11];
    const float4 c0 = lerp4(lerp4(a00, a10, a.fx), lerp4(a01, a11, a.fx), a.fy);
    const float4 c1 = lerp4(lerp4(b00, b10, b.fx), lerp4(b01, b11, b.fx), b.fy);
    return lerp4(c0, c1, L.lod_f);
}

// One projector light on one shaded point: ProjectorLightPixelShader (ProjectorLight.fx:14-56) after the footprint test.  Returns false
// when the shader discards (fullbright, !visible); otherwise the rgb it adds.  No shadow filter and no opacity discard: a visible
// pixel whose opacity is 0 is blended (alpha + 1).
template <int FMT, bool STATS, bool MIPS>
ILM_DEV bool shade_projector(const Pixel& P, const ProjectorRec& L, const TraceField& F, bool have_sdf, const RampView& tex, LightStats& st,
                             float& out_r, float& out_g, float& out_b) {
    if (P.fullbright)
        return false;
    // ProjectorLightPixelCoreNoDF, ProjectorLightCore.fxh:20-85
    const f3 p = P.shaded;
    const float tw = ((p.x * L.m[3] + p.y * L.m[7]) + p.z * L.m[11]) + 1.0f * L.m[15];
    float tx = (((p.x * L.m[0] + p.y * L.m[4]) + p.z * L.m[8]) + 1.0f * L.m[12]) / tw;
    float ty = (((p.x * L.m[1] + p.y * L.m[5]) + p.z * L.m[9]) + 1.0f * L.m[13]) / tw;
    float tz = (((p.x * L.m[2] + p.y * L.m[6]) + p.z * L.m[10]) + 1.0f * L.m[14]) / tw;
    tx += L.region_x0; ty += L.region_y0;
    tz = fmaxf(0.0f, tz);
    const f3 clamped = mk3(clampf(tx, L.region_x0, L.region_x1), clampf(ty, L.region_y0, L.region_y1), clampf(tz, 0.0f, 1.0f));
    const float distance_to_volume = fminf(len3(clamped - mk3(tx, ty, tz)), kProjectorEdgeThreshold) * kProjectorEdgeScale;
    float distance_opacity = 1.0f;
    if (L.clamp > 0.5f)
        distance_opacity = fmaxf(1.0f - distance_to_volume, 0.0f);
    const bool visible = (distance_opacity > 0.0f) && (p.x > -9999.0f) && (L.opacity > 0.0f);
    if (!visible)
        return false;
    tx = lerp(tx, clamped.x, L.clamp); ty = lerp(ty, clamped.y, L.clamp);
    // lerp(1, computeNormalFactor(normalize(shaded - origin), normal), origin.w); at origin.w == 0 the factor is not evaluated (the
    // header's defined deviation: the lerp's value for every finite factor, and no NaN at shaded == origin == 0)
    float normal_opacity = 1.0f;
    if (L.origin_w != 0.0f) {
        float factor = 1.0f;
        if ((P.normal.x != 0.0f) || (P.normal.y != 0.0f) || (P.normal.z != 0.0f)) {
            const f3 ln = norm3(p - mk3(L.origin_x, L.origin_y, L.origin_z));
            const float d = dot3(ln * -1.0f, P.normal);
            factor = pow_pos(sat((d + ref::kDotOffset) / ref::kDotRampRange), ref::kDotExponent);
        }
        normal_opacity = lerp(1.0f, factor, L.origin_w);
    }
    // computeAO, AOCommon.fxh:1-19 (aoRadius scaled by max(0, normal.z), ProjectorLightCore.fxh:127)
    float ao_opacity = 1.0f;
    const float ao_radius = L.ao_radius * fmaxf(0.0f, P.normal.z);
    if ((ao_radius >= 0.5f) && have_sdf) {
        const float distance = sample_distance_field<FMT>(mk3(p.x, p.y, p.z + P.normal.z * ao_radius), F.df, F.sdf);
        if (STATS) st.samples++;
        float r = 1.0f - sat(clampf(distance, 0.0f, ao_radius) / ao_radius);
        r *= r;
        r = 1.0f - r;
        ao_opacity = (1.0f - L.ao_opacity) + (r * L.ao_opacity);
    }
    float opacity = ((distance_opacity * normal_opacity) * L.opacity) * ao_opacity;
    // coneTrace towards the origin, :133-139 + ConeTrace.fxh:141-191: shade_light's general path
    const float casts = L.shadows * (P.enable_shadows ? 1.0f : 0.0f);
    if ((casts != 0.0f) && (opacity >= kProjectorTraceThreshold)) {
        if (STATS && have_sdf) st.traced++;
        f3 start = p + (P.normal * kProjectorSelfOcclusionHack);
        const f3 tv = mk3(L.origin_x, L.origin_y, L.origin_z) - start;
        const float trace_length = len3(tv);
        const float data_y = fmaxf(trace_length - L.radius, 1.0f);
        float data_x = ref::kTraceInitialOffsetPx;
        float data_z = 1.0f;
        const float cfg_z = fmaxf(1.0f, F.df.Packed1.w);
        float steps_remaining = F.df.StepAndMisc2.x;
        // (two VGPRs keep the cone configuration resident across the loop, as in shade_light)
        float cone_max_radius = L.cfg_x, cone_growth = L.cfg_y;
        asm volatile("" : "+v"(cone_max_radius), "+v"(cone_growth));
        f3 dir = mk3(tv.x / trace_length, tv.y / trace_length, tv.z / trace_length);
        // (the sampler treats a NaN coordinate as 0: hoisted as in shade_light's general path)
        if ((start.x != start.x) || (dir.x != dir.x)) { start.x = 0.0f; dir.x = 0.0f; }
        if ((start.y != start.y) || (dir.y != dir.y)) { start.y = 0.0f; dir.y = 0.0f; }
        if ((start.z != start.z) || (dir.z != dir.z)) { start.z = 0.0f; dir.z = 0.0f; }
        cone_trace_loop<FMT, STATS, false>(start, dir, data_y, cfg_z, cone_growth, cone_max_radius, F, data_x, data_z, steps_remaining, have_sdf, st);
        const float visibility = fminf(data_z, steps_remaining / ref::kMaxStepRampWindow);
        opacity *= pow_pos(sat(div_with_rcp(sat(visibility - ref::kFullyShadowedThreshold), kVisibilityRange, kVisibilityRangeRcp)), F.df.ConeAndMisc.z);
    }
    // ProjectorLightColorCore, :290-302
    const float4 t = MIPS ? sample_projector_mips(tex, L, tx, ty) : sample_projector_texture(tex, tx, ty);
    out_r = (t.x * t.w) * opacity; out_g = (t.y * t.w) * opacity; out_b = (t.z * t.w) * opacity;
    return true;
}

// (pixel mapping, base value and blend chains as in directional_lights_kernel: see the note at the head of the full-frame passes)
template <int VARIANT, bool STATS>
__global__ __launch_bounds__(kLightThreads) void projector_lights_kernel(const LightLaunch a, const ProjectorRec* __restrict__ recs, int tiles_x) {
    constexpr int FMT = VARIANT & ~kBlendVariant;
    constexpr bool BLEND = (VARIANT & kBlendVariant) != 0;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int tile_x = (int)blockIdx.x % tiles_x, tile_y = (int)blockIdx.x / tiles_x;
    const int px = tile_x * kTile + (wave & 1) * 8 + (lane & 7);
    const int py = a.row_begin + tile_y * kTile + (wave >> 1) * 8 + (lane >> 3);
    const bool in_image = (px < a.width) && (py < a.row_end);
    if (__builtin_amdgcn_ballot_w64(in_image) == 0ull)
        return;
    Pixel P = sample_gbuffer((float)px, (float)py, a.env, a.gbuffer);
    P.origin_x = 0; P.origin_y = 0; P.start_inside = false;
    const float cxp = (float)px + 0.5f, cyp = (float)py + 0.5f;
    const bool have_sdf = (a.sdf.texels != nullptr) && (a.df.Extent.x > 0.0f);
    const InsideConsts no_table = {};
    const TraceField field = { a.df, a.sdf, no_table, nullptr };
    const size_t o = (size_t)py * (size_t)a.width + (size_t)px;
    auto through_half = [](float v) { return __half2float(__float2half_rn(v)); };
    auto base_value = [&]() -> float4 {
        float4 v = mk4(a.ambient[0], a.ambient[1], a.ambient[2], a.ambient[3]);
        if (a.accumulate != 0 && in_image) {
            if (a.format == ILM_LIGHTMAP_FLOAT4) v = load_target<ILM_LIGHTMAP_FLOAT4>(a.lightmap, o);
            else if (a.format == ILM_LIGHTMAP_HALF4) v = load_target<ILM_LIGHTMAP_HALF4>(a.lightmap, o);
            else v = load_target<ILM_LIGHTMAP_RGBA8>(a.lightmap, o);
        }
        if (a.blend_fp16 != 0) v = mk4(through_half(v.x), through_half(v.y), through_half(v.z), through_half(v.w));
        return v;
    };
    const bool blend_fp16 = a.blend_fp16 != 0;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, acc_a = 0.0f;
    if constexpr (BLEND) { acc_r = acc_g = acc_b = blend_identity(a.blend_color); acc_a = blend_identity(a.blend_alpha); }
    if (blend_fp16) { const float4 v = base_value(); acc_r = v.x; acc_g = v.y; acc_b = v.z; acc_a = v.w; }
    LightStats st;
    const int light_count = a.light_count;
    for (int k = 0; k < light_count; k++) {
        const ProjectorRec& L = recs[k];
        const float x0 = L.x0, y0 = L.y0, x1 = L.x1, y1 = L.y1;
        const bool covered = in_image & (cxp >= x0) & (cxp < x1) & (cyp >= y0) & (cyp < y1);
        if (__builtin_amdgcn_ballot_w64(covered) == 0ull)
            continue;
        if (!covered)
            continue;
        if (STATS) st.pairs++;
        float cr, cg, cb;
        if (!shade_projector<FMT, STATS, false>(P, L, field, have_sdf, a.ramp, st, cr, cg, cb))
            continue;
        if constexpr (BLEND) {
            blend_pair(a.blend_color, a.blend_alpha, blend_fp16, cr, cg, cb, acc_r, acc_g, acc_b, acc_a);
        } else if (blend_fp16) {
            acc_r = through_half(acc_r + through_half(cr));
            acc_g = through_half(acc_g + through_half(cg));
            acc_b = through_half(acc_b + through_half(cb));
            acc_a = through_half(acc_a + 1.0f);
        } else {
            acc_r += cr; acc_g += cg; acc_b += cb; acc_a += 1.0f;
        }
    }
    if (!blend_fp16) {
        const float4 v = base_value();
        if constexpr (BLEND) {
            acc_r = blend_onto_base(a.blend_color, v.x, acc_r); acc_g = blend_onto_base(a.blend_color, v.y, acc_g);
            acc_b = blend_onto_base(a.blend_color, v.z, acc_b); acc_a = blend_onto_base(a.blend_alpha, v.w, acc_a);
        } else {
            acc_r = v.x + acc_r; acc_g = v.y + acc_g; acc_b = v.z + acc_b; acc_a = v.w + acc_a;
        }
    }
    if (in_image) {
        const float4 v = mk4(acc_r, acc_g, acc_b, acc_a);
        store_light_texel(a, o, v);
    }
    if (STATS) add_light_stats(st, a.stats, lane);
}

// The same kernel over a mip chain: the records are prepare_projector_mips_kernel's, the fetch sample_projector_mips.  A copy of the frame,
// as each full-frame pass has its own (the note at their head): as a device function shared with projector_lights_kernel the frame changed
// that kernel's schedule (tools/isa_compare.py: four of four `diff`, same counts), which the one-level pass is held not to do.
template <int VARIANT, bool STATS>
__global__ __launch_bounds__(kLightThreads) void projector_mip_lights_kernel(const LightLaunch a, const ProjectorRec* __restrict__ recs, int tiles_x) {
    constexpr int FMT = VARIANT & ~kBlendVariant;
    constexpr bool BLEND = (VARIANT & kBlendVariant) != 0;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int tile_x = (int)blockIdx.x % tiles_x, tile_y = (int)blockIdx.x / tiles_x;
    const int px = tile_x * kTile + (wave & 1) * 8 + (lane & 7);
    const int py = a.row_begin + tile_y * kTile + (wave >> 1) * 8 + (lane >> 3);
    const bool in_image = (px < a.width) && (py < a.row_end);
    if (__builtin_amdgcn_ballot_w64(in_image) == 0ull)
        return;
    Pixel P = sample_gbuffer((float)px, (float)py, a.env, a.gbuffer);
    P.origin_x = 0; P.origin_y = 0; P.start_inside = false;
    const float cxp = (float)px + 0.5f, cyp = (float)py + 0.5f;
    const bool have_sdf = (a.sdf.texels != nullptr) && (a.df.Extent.x > 0.0f);
    const InsideConsts no_table = {};
    const TraceField field = { a.df, a.sdf, no_table, nullptr };
    const size_t o = (size_t)py * (size_t)a.width + (size_t)px;
    auto through_half = [](float v) { return __half2float(__float2half_rn(v)); };
    auto base_value = [&]() -> float4 {
        float4 v = mk4(a.ambient[0], a.ambient[1], a.ambient[2], a.ambient[3]);
        if (a.accumulate != 0 && in_image) {
            if (a.format == ILM_LIGHTMAP_FLOAT4) v = load_target<ILM_LIGHTMAP_FLOAT4>(a.lightmap, o);
            else if (a.format == ILM_LIGHTMAP_HALF4) v = load_target<ILM_LIGHTMAP_HALF4>(a.lightmap, o);
            else v = load_target<ILM_LIGHTMAP_RGBA8>(a.lightmap, o);
        }
        if (a.blend_fp16 != 0) v = mk4(through_half(v.x), through_half(v.y), through_half(v.z), through_half(v.w));
        return v;
    };
    const bool blend_fp16 = a.blend_fp16 != 0;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, acc_a = 0.0f;
    if constexpr (BLEND) { acc_r = acc_g = acc_b = blend_identity(a.blend_color); acc_a = blend_identity(a.blend_alpha); }
    if (blend_fp16) { const float4 v = base_value(); acc_r = v.x; acc_g = v.y; acc_b = v.z; acc_a = v.w; }
    LightStats st;
    const int light_count = a.light_count;
    for (int k = 0; k < light_count; k++) {
        const ProjectorRec& L = recs[k];
        const float x0 = L.x0, y0 = L.y0, x1 = L.x1, y1 = L.y1;
        const bool covered = in_image & (cxp >= x0) & (cxp < x1) & (cyp >= y0) & (cyp < y1);
        if (__builtin_amdgcn_ballot_w64(covered) == 0ull)
            continue;
        if (!covered)
            continue;
        if (STATS) st.pairs++;
        float cr, cg, cb;
        if (!shade_projector<FMT, STATS, true>(P, L, field, have_sdf, a.ramp, st, cr, cg, cb))
            continue;
        if constexpr (BLEND) {
            blend_pair(a.blend_color, a.blend_alpha, blend_fp16, cr, cg, cb, acc_r, acc_g, acc_b, acc_a);
        } else if (blend_fp16) {
            acc_r = through_half(acc_r + through_half(cr));
            acc_g = through_half(acc_g + through_half(cg));
            acc_b = through_half(acc_b + through_half(cb));
            acc_a = through_half(acc_a + 1.0f);
        } else {
            acc_r += cr; acc_g += cg; acc_b += cb; acc_a += 1.0f;
        }
    }
    if (!blend_fp16) {
        const float4 v = base_value();
        if constexpr (BLEND) {
            acc_r = blend_onto_base(a.blend_color, v.x, acc_r); acc_g = blend_onto_base(a.blend_color, v.y, acc_g);
            acc_b = blend_onto_base(a.blend_color, v.z, acc_b); acc_a = blend_onto_base(a.blend_alpha, v.w, acc_a);
        } else {
            acc_r = v.x + acc_r; acc_g = v.y + acc_g; acc_b = v.z + acc_b; acc_a = v.w + acc_a;
        }
    }
    if (in_image) {
        const float4 v = mk4(acc_r, acc_g, acc_b, acc_a);
        store_light_texel(a, o, v);
    }
    if (STATS) add_light_stats(st, a.stats, lane);
}

hipError_t launch_prepare_projector_lights(const IlmLightVertex* lights, int count, const IlmEnvironment& env, const IlmDistanceFieldUniforms& df,
                                           void* recs, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(prepare_projector_lights_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, lights, count, env, df.ConeAndMisc.x,
                       reinterpret_cast<ProjectorRec*>(recs));
    return hipGetLastError();
}

hipError_t launch_projector_lights_prepared(const LightLaunch& a, const void* recs, hipStream_t stream) {
    static const FullFrameKernel<ProjectorRec> blend[4] = { projector_lights_kernel<ILM_SDF_FP16 + kBlendVariant, false>, projector_lights_kernel<ILM_SDF_FP16 + kBlendVariant, true>,
                                                  projector_lights_kernel<ILM_SDF_UNORM16 + kBlendVariant, false>, projector_lights_kernel<ILM_SDF_UNORM16 + kBlendVariant, true> };
    return launch_full_frame_lights<ProjectorRec>(a, recs, stream, projector_lights_kernel<ILM_SDF_FP16, false>, projector_lights_kernel<ILM_SDF_FP16, true>,
                                           projector_lights_kernel<ILM_SDF_UNORM16, false>, projector_lights_kernel<ILM_SDF_UNORM16, true>, blend);
}

hipError_t launch_prepare_projector_mip_lights(const IlmLightVertex* lights, int count, const IlmEnvironment& env, const IlmDistanceFieldUniforms& df,
                                               const ProjectorMips& mips, void* recs, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    const hipError_t e = launch_prepare_projector_lights(lights, count, env, df, recs, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(prepare_projector_mips_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, lights, count, mips, reinterpret_cast<ProjectorRec*>(recs));
    return hipGetLastError();
}

hipError_t launch_projector_mip_lights_prepared(const LightLaunch& a, const void* recs, hipStream_t stream) {
    static const FullFrameKernel<ProjectorRec> blend[4] = { projector_mip_lights_kernel<ILM_SDF_FP16 + kBlendVariant, false>, projector_mip_lights_kernel<ILM_SDF_FP16 + kBlendVariant, true>,
                                                  projector_mip_lights_kernel<ILM_SDF_UNORM16 + kBlendVariant, false>, projector_mip_lights_kernel<ILM_SDF_UNORM16 + kBlendVariant, true> };
    return launch_full_frame_lights<ProjectorRec>(a, recs, stream, projector_mip_lights_kernel<ILM_SDF_FP16, false>,
                                           projector_mip_lights_kernel<ILM_SDF_FP16, true>, projector_mip_lights_kernel<ILM_SDF_UNORM16, false>,
                                           projector_mip_lights_kernel<ILM_SDF_UNORM16, true>, blend);
}

// ---------------------------------------------------------------------------------------------
// Line lights -- technique LineLight, LineLight.fx:7-42 over LineLightCore.fxh:17-120, drawn by RenderLineLightSource
// (LightingRenderer.cs:1309-1337) as one quad per light whose vertex shader pads the segment's bounds by 9999 (LineLightCore.fxh:142-152):
// every pixel of the rows is covered, so there is no footprint test.  The full-frame passes' frame: one thread per pixel, one wave
// per 8 x 8 pixels, a wave-uniform loop over the prepared records (scalar loads), the G-buffer texel decoded once, the sum in registers,
// one store.  New here: the closed-form area-light term (computeLineLightOpacity, FBPBR.fxh:53-101) in the exact forms of hlsl_math.hpp with
// acos_defined, and a cone trace of three rays in lock-step (lineConeTrace over coneTraceAdvanceEx, ConeTrace.fxh:84-96): three
// independent sample chains per lane.  No ramp technique, no texture.
// ---------------------------------------------------------------------------------------------
constexpr float kLineSelfOcclusionHack = 1.5f;              // LineLightCore.fxh:10 SELF_OCCLUSION_HACK
constexpr float kLineTraceThreshold = 0.75f / 255.0f;       // LineLightCore.fxh:11 SHADOW_OPACITY_THRESHOLD
constexpr float kLineMinimumOffset = 0.03f;                 // LineLightCore.fxh:30
constexpr float kLineIlluminanceWeight = 0.2f;              // FBPBR.fxh:76

struct LineRec {
    float ax, ay, az, radius;                   // LightPosition1.xyz (start); LightProperties.x
    float bx, by, bz, radius_sq;                // LightPosition2.xyz (end); radius * radius
    float dx, dy, dz, ab_dot;                   // delta = end - start; dot(delta, delta), the divisor of closestPointOnLineSegment3
    float lx, ly, lz, offset;                   // lightLeft = normalize(delta); max(saturate((radius + 1) / |delta|), 0.03)
    float mx, my, mz, casts;                    // lightCenter = lerp(start, end, 0.5); LightProperties.w
    float cfg_x, cfg_y, ao_radius, ao_opacity;  // createTraceConfig: maxRadius, radiusGrowthPerPixel; MoreLightProperties.xw
    float c1[4], c2[4];                         // Color1, Color2
};
static_assert(sizeof(LineRec) == kLightRecBytes, "a line record fills the slot of a LightRec (reserve_light_recs)");

// What of computeLineLightOpacity (FBPBR.fxh:60-63), lineConeTrace (LineLightCore.fxh:28-30) and createTraceConfig (ConeTrace.fxh:122-139,
// lightRamp = LightProperties.xy, cone growth 1) depends on the light alone, with the roundings the per-pixel code would make
__global__ __launch_bounds__(64) void prepare_line_lights_kernel(const IlmLightVertex* __restrict__ lights, int count, float max_cone_radius,
                                                                  LineRec* __restrict__ out) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= count) return;
    const IlmLightVertex L = lights[i];
    LineRec r;
    const f3 a = mk3(L.LightPosition1.x, L.LightPosition1.y, L.LightPosition1.z), b = mk3(L.LightPosition2.x, L.LightPosition2.y, L.LightPosition2.z);
    const f3 delta = b - a;
    const f3 left = norm3(delta);
    const f3 centre = a + ((b - a) * 0.5f);
    r.ax = a.x; r.ay = a.y; r.az = a.z; r.bx = b.x; r.by = b.y; r.bz = b.z;
    r.dx = delta.x; r.dy = delta.y; r.dz = delta.z; r.ab_dot = dot3(delta, delta);
    r.lx = left.x; r.ly = left.y; r.lz = left.z;
    r.mx = centre.x; r.my = centre.y; r.mz = centre.z;
    r.radius = L.LightProperties.x; r.radius_sq = L.LightProperties.x * L.LightProperties.x;
    r.offset = fmaxf(sat((L.LightProperties.x + 1.0f) / len3(delta)), kLineMinimumOffset);
    r.casts = L.LightProperties.w;
    const float max_radius = clampf(L.LightProperties.x, ref::kMinConeRadius, max_cone_radius);
    r.cfg_x = max_radius;
    r.cfg_y = max_radius / fmaxf(L.LightProperties.y, 16.0f) * 1.0f;  // getConeGrowthFactor() == 1 (DistanceFieldCommon.fxh:233-236)
    r.ao_radius = L.MoreLightProperties.x; r.ao_opacity = L.MoreLightProperties.w;
    r.c1[0] = L.Color1.x; r.c1[1] = L.Color1.y; r.c1[2] = L.Color1.z; r.c1[3] = L.Color1.w;
    r.c2[0] = L.Color2.x; r.c2[1] = L.Color2.y; r.c2[2] = L.Color2.z; r.c2[3] = L.Color2.w;
    out[i] = r;
}

// lineConeTrace's loop (LineLightCore.fxh:41-50): every iteration advances ALL three rays with coneTraceAdvanceEx (ConeTrace.fxh:84-96) --
// a ray that has reached its end (x = y) keeps sampling there and keeps lowering its own visibility while another ray lives -- then
// takes one step off the shared budget.  Three independent chains of sample -> step per lane.
// liveness = stepsRemaining * (la + lb + lc) > 0 with l = saturate(visibility - FULLY_SHADOWED) * saturate((length - position) * 100) is
// stepsRemaining > 0 && any ray has visibility > FULLY_SHADOWED && length > position: the factors are never negative, the smallest
// positive ones (ulp(0.075) = 2^-27; ulp(0.5) * 100, since 0.5 <= position < length; a budget's fraction >= ulp(1) once it has run) cannot
// underflow their product, a sum of non-negative terms is positive iff a term is, and a NaN factor saturates to 0 and fails its compare
// alike (as in cone_trace_loop).
// The division is skipped as in cone_trace_loop's general form, for all three rays at once: when for every lane and ray
// n >= fl(fl(v (1 + 2^-20)) r) with v > FULLY_SHADOWED and r >= 2^-60, n / r > v, so RN(n / r) >= v and min() keeps v -- exactly.  A ray
// whose visibility has fallen to the threshold or below (it may still be advanced here, unlike there) always divides.
template <int FMT, bool STATS, bool CHECK_NAN>
ILM_DEV void line_trace_loop(const f3& start, const f3 (&dir)[3], const float (&data_y)[3], float cfg_z, float cone_growth, float cone_max_radius,
                             const TraceField& F, float (&data_x)[3], float (&data_z)[3], float& steps_remaining, bool alive, LightStats& st) {
    const float long_step = F.df.StepAndMisc2.z;
    while (alive) {
        float s[3], n[3], local_radius[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const f3 sp = mk3(__builtin_fmaf(dir[i].x, data_x[i], start.x), __builtin_fmaf(dir[i].y, data_x[i], start.y), __builtin_fmaf(dir[i].z, data_x[i], start.z));
            s[i] = sample_distance_field<FMT, CHECK_NAN>(sp, F.df, F.sdf);
        }
        if (STATS) st.samples += 3;
        bool keeps = true;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            local_radius[i] = __builtin_elementwise_minimum(__builtin_fmaf(cone_growth, data_x[i], ref::kMinConeRadius), cone_max_radius);
            n[i] = s[i] + ref::kHackDistanceOffset;
            keeps = keeps & (n[i] >= (data_z[i] * 1.00000095367431640625f) * local_radius[i]) & (local_radius[i] >= 0x1p-60f) &
                    (data_z[i] > ref::kFullyShadowedThreshold);
        }
        if (__builtin_amdgcn_ballot_w64(!keeps) != 0ull) {
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const float local_visibility = n[i] / local_radius[i];
                asm("v_min_f32 %0, %0, %1" : "+v"(data_z[i]) : "v"(local_visibility));      // (minNum without the canonicalising v_max, as cone_trace_loop)
            }
        }
        bool any = false;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            float step = fabsf(s[i]) * long_step;
            asm("v_max_f32 %0, %0, %1" : "+v"(step) : "v"(cfg_z));
            data_x[i] = fminf(data_x[i] + step, data_y[i]);
            any = any | ((data_z[i] > ref::kFullyShadowedThreshold) & (data_y[i] > data_x[i]));
        }
        steps_remaining -= 1.0f;
        alive = (steps_remaining > 0.0f) & any;
    }
}

// One line light on one shaded point: LineLightPixelShader (LineLight.fx:7-42) over LineLightPixelCore (LineLightCore.fxh:70-120).
// Returns false when the shader discards (fullbright; clip(!visible): distance opacity not > 0, or shaded x <= -9999); otherwise the
// rgb it adds.  Every operation of the opacity term is an exact form, in the order the HLSL writes it: degenerate geometry (radius 0, a
// pixel on the segment's axis, start == end, a NaN position) makes norm3(0) = NaN, the NaN reaches the final saturate, sat(NaN) = 0
// and the pair is discarded before anything is sampled.
template <int FMT, bool STATS>
ILM_DEV bool shade_line(const Pixel& P, const LineRec& L, const TraceField& F, bool have_sdf, LightStats& st, float& out_r, float& out_g, float& out_b) {
    const f3 pos = P.shaded, a = mk3(L.ax, L.ay, L.az), b = mk3(L.bx, L.by, L.bz), ab = mk3(L.dx, L.dy, L.dz);
    // closestPointOnLineSegment3, DistanceFieldCommon.fxh:151-155
    const float u = sat(dot3(pos - a, ab) / L.ab_dot);
    const f3 sphere = a + (ab * u);
    // computeLineLightOpacity, FBPBR.fxh:53-101
    const f3 to_sphere = sphere - pos;
    const f3 forward = norm3(to_sphere);
    const f3 up = cross3(mk3(L.lx, L.ly, L.lz), forward);
    const f3 ru = up * L.radius;
    const f3 v0 = (a + ru) - pos, v1 = (a - ru) - pos, v2 = (b - ru) - pos, v3 = (b + ru) - pos;
    // rectangleSolidAngle, FBPBR.fxh:33-51
    const f3 n0 = norm3(cross3(v0, v1)), n1 = norm3(cross3(v1, v2)), n2 = norm3(cross3(v2, v3)), n3 = norm3(cross3(v3, v0));
    const float g0 = acos_defined(dot3(n0 * -1.0f, n1)), g1 = acos_defined(dot3(n1 * -1.0f, n2));
    const float g2 = acos_defined(dot3(n2 * -1.0f, n3)), g3 = acos_defined(dot3(n3 * -1.0f, n0));
    const float solid_angle = (((g0 + g1) + g2) + g3) - (2.0f * kPi);
    const float facing = (((sat(dot3(norm3(v0), P.normal)) + sat(dot3(norm3(v1), P.normal))) + sat(dot3(norm3(v2), P.normal))) +
                          sat(dot3(norm3(v3), P.normal))) + sat(dot3(norm3(mk3(L.mx, L.my, L.mz) - pos), P.normal));
    const float illuminance = (solid_angle * kLineIlluminanceWeight) * facing;
    // (sphereL = normalize(spherePosition - worldPos) is `forward`: the same operations on the same values)
    const float illuminance_sphere = (kPi * sat(dot3(forward, P.normal))) * (L.radius_sq / dot3(to_sphere, to_sphere));
    const float distance_opacity = sat(illuminance + illuminance_sphere);
    const bool visible = (distance_opacity > 0.0f) && (pos.x > -9999.0f);
    if (!visible)
        return false;

    // computeAO, AOCommon.fxh:1-19 (aoRadius scaled by max(0, normal.z), LineLightCore.fxh:98)
    float ao_opacity = 1.0f;
    const float ao_radius = L.ao_radius * fmaxf(0.0f, P.normal.z);
    if ((ao_radius >= 0.5f) && have_sdf) {
        const float distance = sample_distance_field<FMT>(mk3(pos.x, pos.y, pos.z + P.normal.z * ao_radius), F.df, F.sdf);
        if (STATS) st.samples++;
        float r = 1.0f - sat(clampf(distance, 0.0f, ao_radius) / ao_radius);
        r *= r;
        r = 1.0f - r;
        ao_opacity = (1.0f - L.ao_opacity) + (r * L.ao_opacity);
    }
    const float pre_trace = distance_opacity * ao_opacity;

    // lineConeTrace, LineLightCore.fxh:17-68
    float cone_opacity = 1.0f;
    const float casts = L.casts * (P.enable_shadows ? 1.0f : 0.0f);
    if ((casts != 0.0f) && (pre_trace >= kLineTraceThreshold)) {
        if (STATS && have_sdf) st.traced++;
        const f3 start = pos + (P.normal * kLineSelfOcclusionHack);
        const float along[3] = { sat(u - L.offset), u, sat(u + L.offset) };
        f3 dir[3];
        float data_x[3], data_y[3], data_z[3];
        bool any_nan = (start.x != start.x) | (start.y != start.y) | (start.z != start.z);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            // coneTraceInitialize, ConeTrace.fxh:37-49
            const f3 tv = (a + (ab * along[i])) - start;
            const float trace_length = len3(tv);
            dir[i] = mk3(tv.x / trace_length, tv.y / trace_length, tv.z / trace_length);
            data_y[i] = fmaxf(trace_length - L.radius, 1.0f);
            data_x[i] = ref::kTraceInitialOffsetPx;
            data_z[i] = 1.0f;
            any_nan = any_nan | (dir[i].x != dir[i].x) | (dir[i].y != dir[i].y) | (dir[i].z != dir[i].z);
        }
        const float cfg_z = fmaxf(1.0f, F.df.Packed1.w);
        float steps_remaining = F.df.StepAndMisc2.x;
        // (two VGPRs keep the cone configuration resident across the loop, as in shade_light)
        float cone_max_radius = L.cfg_x, cone_growth = L.cfg_y;
        asm volatile("" : "+v"(cone_max_radius), "+v"(cone_growth));
        // The sampler treats a NaN coordinate as 0, and start + dir * x is NaN for every x exactly when start or dir is.  The three rays
        // share their start, so the hoist of shade_light (start = dir = 0 on such an axis) would need a start per ray: instead a wave with
        // such a lane (a target equal to the start: length 0) takes the loop whose sampler tests its coordinates.
        if (__builtin_amdgcn_ballot_w64(any_nan) != 0ull)
            line_trace_loop<FMT, STATS, true>(start, dir, data_y, cfg_z, cone_growth, cone_max_radius, F, data_x, data_z, steps_remaining, have_sdf, st);
        else
            line_trace_loop<FMT, STATS, false>(start, dir, data_y, cfg_z, cone_growth, cone_max_radius, F, data_x, data_z, steps_remaining, have_sdf, st);
        // (no stepsRemaining == 0 fix-up here, unlike coneTrace)
        const float visibility = fminf(((data_z[0] + data_z[1]) + data_z[2]) / 3.0f, steps_remaining / ref::kMaxStepRampWindow);
        cone_opacity = pow_pos(sat(div_with_rcp(sat(visibility - ref::kFullyShadowedThreshold), kVisibilityRange, kVisibilityRangeRcp)), F.df.ConeAndMisc.z);
    }
    const float opacity = pre_trace * cone_opacity;
    // color = lerp(startColor, endColor, u); result = (color.rgb * color.a * opacity, 1), LineLight.fx:40-41
    const float ca = lerp(L.c1[3], L.c2[3], u);
    out_r = (lerp(L.c1[0], L.c2[0], u) * ca) * opacity;
    out_g = (lerp(L.c1[1], L.c2[1], u) * ca) * opacity;
    out_b = (lerp(L.c1[2], L.c2[2], u) * ca) * opacity;
    return true;
}

// (pixel mapping, base value and blend chains as in directional_lights_kernel: see the note at the head of the full-frame passes.)
// No footprint: the vertex shader's quad, min(P) - 9999 .. max(P) + 9999, is defined here as every pixel of the rows.
template <int VARIANT, bool STATS>
__global__ __launch_bounds__(kLightThreads) void line_lights_kernel(const LightLaunch a, const LineRec* __restrict__ recs, int tiles_x) {
    constexpr int FMT = VARIANT & ~kBlendVariant;
    constexpr bool BLEND = (VARIANT & kBlendVariant) != 0;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int tile_x = (int)blockIdx.x % tiles_x, tile_y = (int)blockIdx.x / tiles_x;
    const int px = tile_x * kTile + (wave & 1) * 8 + (lane & 7);
    const int py = a.row_begin + tile_y * kTile + (wave >> 1) * 8 + (lane >> 3);
    const bool in_image = (px < a.width) && (py < a.row_end);
    if (__builtin_amdgcn_ballot_w64(in_image) == 0ull)
        return;
    Pixel P = sample_gbuffer((float)px, (float)py, a.env, a.gbuffer);
    P.origin_x = 0; P.origin_y = 0; P.start_inside = false;
    const bool have_sdf = (a.sdf.texels != nullptr) && (a.df.Extent.x > 0.0f);
    const InsideConsts no_table = {};
    const TraceField field = { a.df, a.sdf, no_table, nullptr };
    const size_t o = (size_t)py * (size_t)a.width + (size_t)px;
    auto through_half = [](float v) { return __half2float(__float2half_rn(v)); };
    auto base_value = [&]() -> float4 {
        float4 v = mk4(a.ambient[0], a.ambient[1], a.ambient[2], a.ambient[3]);
        if (a.accumulate != 0 && in_image) {
            if (a.format == ILM_LIGHTMAP_FLOAT4) v = load_target<ILM_LIGHTMAP_FLOAT4>(a.lightmap, o);
            else if (a.format == ILM_LIGHTMAP_HALF4) v = load_target<ILM_LIGHTMAP_HALF4>(a.lightmap, o);
            else v = load_target<ILM_LIGHTMAP_RGBA8>(a.lightmap, o);
        }
        if (a.blend_fp16 != 0) v = mk4(through_half(v.x), through_half(v.y), through_half(v.z), through_half(v.w));
        return v;
    };
    const bool blend_fp16 = a.blend_fp16 != 0;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, acc_a = 0.0f;
    if constexpr (BLEND) { acc_r = acc_g = acc_b = blend_identity(a.blend_color); acc_a = blend_identity(a.blend_alpha); }
    if (blend_fp16) { const float4 v = base_value(); acc_r = v.x; acc_g = v.y; acc_b = v.z; acc_a = v.w; }
    LightStats st;
    const int light_count = a.light_count;
    // (a fullbright pixel is discarded before anything of a light is read, LineLight.fx:25-29: it forms no pair)
    const bool shades = in_image && !P.fullbright;
    for (int k = 0; k < light_count; k++) {
        const LineRec& L = recs[k];
        if (!shades)
            continue;
        if (STATS) st.pairs++;
        float cr, cg, cb;
        if (!shade_line<FMT, STATS>(P, L, field, have_sdf, st, cr, cg, cb))
            continue;
        if constexpr (BLEND) {
            blend_pair(a.blend_color, a.blend_alpha, blend_fp16, cr, cg, cb, acc_r, acc_g, acc_b, acc_a);
        } else if (blend_fp16) {
            acc_r = through_half(acc_r + through_half(cr));
            acc_g = through_half(acc_g + through_half(cg));
            acc_b = through_half(acc_b + through_half(cb));
            acc_a = through_half(acc_a + 1.0f);
        } else {
            acc_r += cr; acc_g += cg; acc_b += cb; acc_a += 1.0f;
        }
    }
    if (!blend_fp16) {
        const float4 v = base_value();
        if constexpr (BLEND) {
            acc_r = blend_onto_base(a.blend_color, v.x, acc_r); acc_g = blend_onto_base(a.blend_color, v.y, acc_g);
            acc_b = blend_onto_base(a.blend_color, v.z, acc_b); acc_a = blend_onto_base(a.blend_alpha, v.w, acc_a);
        } else {
            acc_r = v.x + acc_r; acc_g = v.y + acc_g; acc_b = v.z + acc_b; acc_a = v.w + acc_a;
        }
    }
    if (in_image) {
        const float4 v = mk4(acc_r, acc_g, acc_b, acc_a);
        store_light_texel(a, o, v);
    }
    if (STATS) add_light_stats(st, a.stats, lane);
}

hipError_t launch_prepare_line_lights(const IlmLightVertex* lights, int count, const IlmDistanceFieldUniforms& df, void* recs, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(prepare_line_lights_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, lights, count, df.ConeAndMisc.x,
                       reinterpret_cast<LineRec*>(recs));
    return hipGetLastError();
}

hipError_t launch_line_lights_prepared(const LightLaunch& a, const void* recs, hipStream_t stream) {
    static const FullFrameKernel<LineRec> blend[4] = { line_lights_kernel<ILM_SDF_FP16 + kBlendVariant, false>, line_lights_kernel<ILM_SDF_FP16 + kBlendVariant, true>,
                                                  line_lights_kernel<ILM_SDF_UNORM16 + kBlendVariant, false>, line_lights_kernel<ILM_SDF_UNORM16 + kBlendVariant, true> };
    return launch_full_frame_lights<LineRec>(a, recs, stream, line_lights_kernel<ILM_SDF_FP16, false>, line_lights_kernel<ILM_SDF_FP16, true>,
                                           line_lights_kernel<ILM_SDF_UNORM16, false>, line_lights_kernel<ILM_SDF_UNORM16, true>, blend);
}

// ---------------------------------------------------------------------------------------------
// Volumetric lights -- techniques VolumetricLight / ShadowedVolumetricLight (VolumetricLight.fx:7-51, ShadowedVolumetricLight.fx:7-52) over
// VolumetricLightCore.fxh:25-88,281-298,315-549, drawn by RenderVolumetricLightSource (LightingRenderer.cs:1339-1384) as one quad per light
// over the bounding rectangle of its shape.  The full-frame passes' frame with the directional pass's footprint test.  New here: per pair a
// column of up to MaxStepCount + 1 points through the shape (volumetricTrace), each of which evaluates the shape's distance function and --
// for a light that casts shadows -- marches the field towards the light with up to MaxStepCount samples; then a contact term at the shaded
// point.  The shape is uniform per light (a scalar branch around three copies of the column loop, never a test per sample); the column's trip
// count is nearly uniform over a wave, the march's is not and stays a plain per-lane loop.  `intersect` (:300-313) returns true on its
// second line, so the early-out never fires: the five ray / shape intersections, sdCappedCone and sdCapsule are dead code and not built.
// ---------------------------------------------------------------------------------------------
constexpr float kVolumetricDitherScale = 0.66f;             // VolumetricLightCore.fxh:361
constexpr float kVolumetricStepScale = 0.99f;               // :361
constexpr float kVolumetricHit = -0.1f;                     // :388
constexpr float kVolumetricProjectThreshold = 0.01f;        // :327
constexpr float kVolumetricConeDot = 0.33f;                 // :469,476
constexpr float kVolumetricBoxFloor = 0.0001f;              // :87
constexpr int kVolumetricLoopGuard = 4;                     // the column loop runs at most (int)MaxStepCount + 4 times (illuminant_hip.h)
constexpr int kVolumetricShapeMask = 3, kVolumetricProject = 4, kVolumetricCasts = 8, kVolumetricCastsUnshadowed = 16;

// 32 floats: what the record cannot hold is made per pair from what it does hold, with the roundings of the definition -- the cone's
// rr = r1 - r2, the dot constants (one value: DOT_OFFSET == DOT_RAMP_RANGE) and the march direction trace / md (three divisions, "traceAlong /=
// md" as written).  fullLength is md: the same operations on the same values (:339,343 and :465-467).
struct VolumetricRec {
    float x0, y0, x1, y1;                                       // footprint in screen pixels: centre in [x0, x1) x [y0, y1)
    float sx, sy, sz; int flags;                                // LightPosition1.xyz; shape | project from the origin | casts (w * 1 != 0, w * 0 != 0)
    float z_hi, z_lo, md, full_att;                             // the shape's z extent (:335-344); defaultTraceDistance; fullLength * DistanceAttenuation
    float tx, ty, tz, volumetricity;                            // traceAlong = rayNormal * defaultTraceDistance (:372); LightProperties.x
    float ramp_length, ramp_power, blowout, ao_radius;          // LightProperties.y, EvenMoreLightProperties.yx, MoreLightProperties.x
    float ao_opacity, col_r, col_g, col_b;                      // MoreLightProperties.w; Color1.rgb * Color1.a
    float u[8];                                                 // cone: ba, l2, a2, il2, r1, r2; ellipsoid: r, r * r; box: b
};
static_assert(sizeof(VolumetricRec) == kLightRecBytes, "a volumetric record fills the slot of a LightRec (reserve_light_recs)");

// VolumetricLightVertexShader (VolumetricLightCore.fxh:510-549) at the quad's two extreme corners, and what volumetricTrace, eval and the
// contact term compute from the light alone.  Shape is 0, 1 or 2 (ilm_render_volumetric_lights refuses every other value).
__global__ __launch_bounds__(64) void prepare_volumetric_lights_kernel(const IlmLightVertex* __restrict__ lights, int count, IlmEnvironment env,
                                                                        VolumetricRec* __restrict__ out) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= count) return;
    const IlmLightVertex L = lights[i];
    VolumetricRec r = {};
    const int shape = (int)L.EvenMoreLightProperties.w;
    const f3 s = mk3(L.LightPosition1.x, L.LightPosition1.y, L.LightPosition1.z), e = mk3(L.LightPosition2.x, L.LightPosition2.y, L.LightPosition2.z);
    const float r1 = L.LightPosition1.w, r2 = L.LightPosition2.w;
    float p1x, p1y, p2x, p2y;
    if (shape == 1) {
        const float m = fmaxf(r1, r2);
        p1x = fminf(s.x, e.x) - m; p1y = fminf(s.y, e.y) - m;
        p2x = fmaxf(s.x, e.x) + m; p2y = fmaxf(s.y, e.y) + m;
        r.z_hi = fmaxf(s.z, e.z) + m; r.z_lo = fminf(s.z, e.z) - m;
        r.md = len3(e - s);
        const f3 ba = e - s;
        const float l2 = dot3(ba, ba), rr = r1 - r2;
        r.u[0] = ba.x; r.u[1] = ba.y; r.u[2] = ba.z; r.u[3] = l2; r.u[4] = l2 - rr * rr; r.u[5] = 1.0f / l2; r.u[6] = r1; r.u[7] = r2;
    } else {
        p1x = s.x - e.x; p1y = s.y - e.y;
        p2x = s.x + e.x; p2y = s.y + e.y;
        r.z_hi = s.z + e.z; r.z_lo = s.z - e.z;
        r.md = len3(e);
        r.u[0] = e.x; r.u[1] = e.y; r.u[2] = e.z;
        if (shape == 0) { r.u[3] = e.x * e.x; r.u[4] = e.y * e.y; r.u[5] = e.z * e.z; }
    }
    const float scale_x = env.GBufferTexelSizeAndMisc.z * env.ZAndScale.z, scale_y = env.GBufferTexelSizeAndMisc.w * env.ZAndScale.w;
    r.x0 = (fminf(p1x, p2x) - env.ViewportPosition[0]) * scale_x; r.y0 = (fminf(p1y, p2y) - env.ViewportPosition[1]) * scale_y;
    r.x1 = (fmaxf(p1x, p2x) - env.ViewportPosition[0]) * scale_x; r.y1 = (fmaxf(p1y, p2y) - env.ViewportPosition[1]) * scale_y;
    // (fminf / fmaxf return the operand that is not a NaN: a rectangle keeps a NaN only where both candidates of a bound are NaN)
    r.sx = s.x; r.sy = s.y; r.sz = s.z;
    const f3 ray = mk3(L.LightPosition3.x, L.LightPosition3.y, L.LightPosition3.z);
    const float w = L.LightProperties.w;
    r.flags = shape | ((len3(ray) < kVolumetricProjectThreshold) ? kVolumetricProject : 0) | ((w * 1.0f != 0.0f) ? kVolumetricCasts : 0) |
              ((w * 0.0f != 0.0f) ? kVolumetricCastsUnshadowed : 0);
    r.full_att = r.md * L.EvenMoreLightProperties.z;
    r.tx = ray.x * r.md; r.ty = ray.y * r.md; r.tz = ray.z * r.md;
    r.volumetricity = L.LightProperties.x; r.ramp_length = L.LightProperties.y;
    r.ramp_power = L.EvenMoreLightProperties.y; r.blowout = L.EvenMoreLightProperties.x;
    r.ao_radius = L.MoreLightProperties.x; r.ao_opacity = L.MoreLightProperties.w;
    r.col_r = L.Color1.x * L.Color1.w; r.col_g = L.Color1.y * L.Color1.w; r.col_b = L.Color1.z * L.Color1.w;
    out[i] = r;
}

// Dither17 (Fracture's DitherCommon.fxh, outside the reference tree; Jimenez: frac(dot(float3(pos, frame), float3(2, 7, 23) / 17))) as a
// DEFINED function at frame value 0.5 (FrameIndex stays at its default 0): k = 2 x + 7 y + 11.5 is exact, k mod 17 = ((2 x + 7 y + 11) mod 17)
// + 0.5 is exact, and the result is that value / 17 -- one IEEE division.
ILM_DEV float dither17(int px, int py) {
    return ((float)((2 * px + 7 * py + 11) % 17) + 0.5f) / 17.0f;
}

// eval (VolumetricLightCore.fxh:281-298) along one pixel's column: x and y of the position are the shaded point's for every point of
// volumetricTrace and for the contact term, so what depends on them alone is made once per pair -- the leading terms of the sums stay the
// leading terms (dot = (x + y) + z), no rounding changes.
struct EllipsoidColumn {        // sdEllipsoid, :25-29
    float k0xy, k1xy, cz, rz, rrz;
    ILM_DEV EllipsoidColumn(const f3& p, const VolumetricRec& L) {
        const float ax = (p.x - L.sx) / L.u[0], ay = (p.y - L.sy) / L.u[1], bx = (p.x - L.sx) / L.u[3], by = (p.y - L.sy) / L.u[4];
        k0xy = ax * ax + ay * ay; k1xy = bx * bx + by * by; cz = L.sz; rz = L.u[2]; rrz = L.u[5];
    }
    ILM_DEV float operator()(float z) const {
        const float az = (z - cz) / rz, bz = (z - cz) / rrz;
        const float k0 = sqrtf(k0xy + az * az), k1 = sqrtf(k1xy + bz * bz);
        return k0 * (k0 - 1.0f) / k1;
    }
};
struct ConeColumn {             // sdRoundCone, :31-54
    float pax, pay, yxy, az, bax, bay, baz, l2, rr, a2, il2, r1, r2;
    ILM_DEV ConeColumn(const f3& p, const VolumetricRec& L) {
        pax = p.x - L.sx; pay = p.y - L.sy; az = L.sz; bax = L.u[0]; bay = L.u[1]; baz = L.u[2]; l2 = L.u[3]; a2 = L.u[4]; il2 = L.u[5];
        r1 = L.u[6]; r2 = L.u[7]; rr = r1 - r2;
        yxy = pax * bax + pay * bay;
    }
    ILM_DEV float operator()(float pz) const {
        const float paz = pz - az;
        const float y = yxy + paz * baz;
        const float z = y - l2;
        const float vx = pax * l2 - bax * y, vy = pay * l2 - bay * y, vz = paz * l2 - baz * y;
        const float x2 = (vx * vx + vy * vy) + vz * vz;
        const float y2 = y * y * l2, z2 = z * z * l2;
        const float k = sgn(rr) * rr * rr * x2;
        if (sgn(z) * a2 * z2 > k) return sqrtf(x2 + z2) * il2 - r2;
        if (sgn(y) * a2 * y2 < k) return sqrtf(x2 + y2) * il2 - r1;
        return (sqrtf(x2 * a2 * il2) + y * rr) * il2 - r1;
    }
};
struct BoxColumn {              // sdBox, :85-88
    float lxy, mxy, cz, bz;
    ILM_DEV BoxColumn(const f3& p, const VolumetricRec& L) {
        const float dx = fabsf(p.x - L.sx) - L.u[0], dy = fabsf(p.y - L.sy) - L.u[1];
        const float ex = fmaxf(dx, kVolumetricBoxFloor), ey = fmaxf(dy, kVolumetricBoxFloor);
        lxy = ex * ex + ey * ey; mxy = fmaxf(dx, dy); cz = L.sz; bz = L.u[2];
    }
    ILM_DEV float operator()(float z) const {
        const float dz = fabsf(z - cz) - bz, ez = fmaxf(dz, kVolumetricBoxFloor);
        return sqrtf(lxy + ez * ez) + fminf(fmaxf(mxy, dz), kVolumetricBoxFloor);
    }
};

// volumetricTrace (VolumetricLightCore.fxh:315-409) for one pair.  `march`: traceShadows with a bound field (without one occlusion = 1 and
// nothing is sampled).  The body always runs once; z -= step stops making progress once step falls below an ulp of z, so the loop is also
// bounded by an integer: (int)steps + 4 bodies (with a valid MaxStepCount the arithmetic ends it after at most steps + 1).  A NaN z ends it:
// the comparison is false.
template <int FMT, bool STATS, class Column>
ILM_DEV float volumetric_trace(const Column& eval, const Pixel& P, const VolumetricRec& L, const TraceField& F, bool march, float dither, float ground_z,
                               float maximum_z, LightStats& st) {
    const float steps = F.df.StepAndMisc2.x, min_step = F.df.Packed1.w;
    float z2 = fmaxf(P.shaded.z, ground_z), z1 = fmaxf(maximum_z, z2);
    z1 = fminf(z1, L.z_hi);
    z2 = fmaxf(z2, L.z_lo);
    const float step = fmaxf(fabsf(z2 - z1), 1.0f) / steps;
    float z = z1 + (dither * step);
    float hits = 0.0f;
    const int trace_steps = (int)steps;
    int guard = trace_steps + kVolumetricLoopGuard;
    const bool project = (L.flags & kVolumetricProject) != 0;
    const f3 origin = mk3(L.sx, L.sy, L.sz), trace = mk3(L.tx, L.ty, L.tz);
    f3 fixed_along = mk3(0.0f, 0.0f, 0.0f);
    if (march && !project)
        fixed_along = mk3(trace.x / L.md, trace.y / L.md, trace.z / L.md);
    do {
        const float sd = eval(z);
        float occlusion = 1.0f;
        if (march) {
            const f3 pos = mk3(P.shaded.x, P.shaded.y, z);
            f3 from, along;
            float md;
            if (project) {
                along = pos - origin;
                from = origin;
                md = len3(along);
                along = mk3(along.x / md, along.y / md, along.z / md);
            } else {
                from = pos - trace;
                along = fixed_along;
                md = L.md;
            }
            // (the sampler treats a NaN coordinate as 0: hoisted as in shade_directional)
            if ((from.x != from.x) || (along.x != along.x)) { from.x = 0.0f; along.x = 0.0f; }
            if ((from.y != from.y) || (along.y != along.y)) { from.y = 0.0f; along.y = 0.0f; }
            if ((from.z != from.z) || (along.z != along.z)) { from.z = 0.0f; along.z = 0.0f; }
            float d = dither * kVolumetricDitherScale;
            int remaining = trace_steps;
            while (remaining > 0) {
                const f3 sp = mk3(__builtin_fmaf(along.x, d, from.x), __builtin_fmaf(along.y, d, from.y), __builtin_fmaf(along.z, d, from.z));
                const float s = sample_distance_field<FMT, false>(sp, F.df, F.sdf);
                if (STATS) st.samples++;
                occlusion = sat(s * 0.5f);
                if (s <= kVolumetricHit) { remaining = 0; occlusion = 0.0f; }
                d += fmaxf(fabsf(s) * kVolumetricStepScale, min_step);
                if (d >= md) remaining = 0; else remaining--;
            }
        }
        const float ramp = pow_pos(sat(-sd / L.ramp_length), L.ramp_power);
        hits += ramp * occlusion;
        z -= step;
    } while ((z >= z2) && (--guard > 0));
    return sat(hits / steps / L.volumetricity);
}

// One volumetric light on one shaded point inside its footprint: the two pixel shaders over VolumetricLightPixelCore (:411-508).  Returns
// false when the shader discards (fullbright; not visible: the core returns 0; opacity <= 0); otherwise the opacity that multiplies
// color.rgb * color.a.  The RampMode >= 1 squaring of distanceOpacity (:495-498) follows the last read of it and is not computed.
template <int FMT, bool STATS>
ILM_DEV bool shade_volumetric(const Pixel& P, int px, int py, const VolumetricRec& L, const TraceField& F, bool have_sdf, float ground_z, float maximum_z,
                              LightStats& st, float& opacity) {
    if (P.fullbright)
        return false;
    if (!(P.shaded.x > -9999.0f))
        return false;
    // computeAO, AOCommon.fxh:1-19 (aoRadius scaled by max(0, normal.z), :448)
    float ao_opacity = 1.0f;
    const float ao_radius = L.ao_radius * fmaxf(0.0f, P.normal.z);
    if ((ao_radius >= 0.5f) && have_sdf) {
        const float distance = sample_distance_field<FMT>(mk3(P.shaded.x, P.shaded.y, P.shaded.z + P.normal.z * ao_radius), F.df, F.sdf);
        if (STATS) st.samples++;
        float r = 1.0f - sat(clampf(distance, 0.0f, ao_radius) / ao_radius);
        r *= r;
        r = 1.0f - r;
        ao_opacity = (1.0f - L.ao_opacity) + (r * L.ao_opacity);
    }
    // traceShadows = (lightProperties.w * enableShadows != 0) && Extent.z > 0 (:451; VolumetricLight.fx passes w = 0)
    const bool casts = (L.flags & (P.enable_shadows ? kVolumetricCasts : kVolumetricCastsUnshadowed)) != 0;
    const bool march = casts && (F.df.Extent.z > 0.0f) && have_sdf;
    if (STATS && march) st.traced++;
    const float dither = dither17(px, py);
    const int shape = L.flags & kVolumetricShapeMask;
    float volumetric_opacity, contact_distance, cone_dot = 0.0f;
    if (shape == 0) {
        const EllipsoidColumn eval(P.shaded, L);
        volumetric_opacity = volumetric_trace<FMT, STATS>(eval, P, L, F, march, dither, ground_z, maximum_z, st);
        contact_distance = eval(P.shaded.z);
    } else if (shape == 1) {
        const ConeColumn eval(P.shaded, L);
        volumetric_opacity = volumetric_trace<FMT, STATS>(eval, P, L, F, march, dither, ground_z, maximum_z, st);
        contact_distance = eval(P.shaded.z);
        cone_dot = fmaxf(L.u[6], L.u[7]) / 64.0f;
    } else {
        const BoxColumn eval(P.shaded, L);
        volumetric_opacity = volumetric_trace<FMT, STATS>(eval, P, L, F, march, dither, ground_z, maximum_z, st);
        contact_distance = eval(P.shaded.z);
    }
    const float pre_trace = ao_opacity * volumetric_opacity;
    // the contact term, :464-507
    const float dot_range = lerp(ref::kDotRampRange, kVolumetricConeDot, cone_dot), dot_offset = lerp(ref::kDotOffset, kVolumetricConeDot, cone_dot);
    const f3 to_point = P.shaded - mk3(L.sx, L.sy, L.sz);
    const float distance = len3(to_point);
    float normal_opacity = 1.0f;
    if ((P.normal.x != 0.0f) || (P.normal.y != 0.0f) || (P.normal.z != 0.0f)) {
        const f3 light_normal = mk3(to_point.x / distance, to_point.y / distance, to_point.z / distance);
        const float d = dot3(light_normal * -1.0f, P.normal);
        normal_opacity = pow_pos(sat((d + dot_offset) / dot_range), ref::kDotExponent);
    }
    normal_opacity = lerp(normal_opacity, normal_opacity * 2.0f - 1.0f, L.blowout);
    const float shape_opacity = (contact_distance < 0.0f) ? pow_pos(sat(-contact_distance / L.ramp_length), L.ramp_power) : 0.0f;
    const float distance_opacity = 1.0f - sat(distance / L.full_att);
    const float diffuse = normal_opacity * shape_opacity * distance_opacity;
    opacity = (diffuse < 0.0f) ? (pre_trace + diffuse) : fmaxf(pre_trace, diffuse);
    return !(opacity <= 0.0f);
}

// (pixel mapping, base value, blend chains and footprint test as in directional_lights_kernel: see the note at the head of the full-frame
// passes.)
template <int VARIANT, bool STATS>
__global__ __launch_bounds__(kLightThreads) void volumetric_lights_kernel(const LightLaunch a, const VolumetricRec* __restrict__ recs, int tiles_x) {
    constexpr int FMT = VARIANT & ~kBlendVariant;
    constexpr bool BLEND = (VARIANT & kBlendVariant) != 0;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int tile_x = (int)blockIdx.x % tiles_x, tile_y = (int)blockIdx.x / tiles_x;
    const int px = tile_x * kTile + (wave & 1) * 8 + (lane & 7);
    const int py = a.row_begin + tile_y * kTile + (wave >> 1) * 8 + (lane >> 3);
    const bool in_image = (px < a.width) && (py < a.row_end);
    if (__builtin_amdgcn_ballot_w64(in_image) == 0ull)
        return;
    Pixel P = sample_gbuffer((float)px, (float)py, a.env, a.gbuffer);
    P.origin_x = 0; P.origin_y = 0; P.start_inside = false;
    const float cxp = (float)px + 0.5f, cyp = (float)py + 0.5f;
    const bool have_sdf = (a.sdf.texels != nullptr) && (a.df.Extent.x > 0.0f);
    const InsideConsts no_table = {};
    const TraceField field = { a.df, a.sdf, no_table, nullptr };
    const size_t o = (size_t)py * (size_t)a.width + (size_t)px;
    auto through_half = [](float v) { return __half2float(__float2half_rn(v)); };
    auto base_value = [&]() -> float4 {
        float4 v = mk4(a.ambient[0], a.ambient[1], a.ambient[2], a.ambient[3]);
        if (a.accumulate != 0 && in_image) {
            if (a.format == ILM_LIGHTMAP_FLOAT4) v = load_target<ILM_LIGHTMAP_FLOAT4>(a.lightmap, o);
            else if (a.format == ILM_LIGHTMAP_HALF4) v = load_target<ILM_LIGHTMAP_HALF4>(a.lightmap, o);
            else v = load_target<ILM_LIGHTMAP_RGBA8>(a.lightmap, o);
        }
        if (a.blend_fp16 != 0) v = mk4(through_half(v.x), through_half(v.y), through_half(v.z), through_half(v.w));
        return v;
    };
    const bool blend_fp16 = a.blend_fp16 != 0;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, acc_a = 0.0f;
    if constexpr (BLEND) { acc_r = acc_g = acc_b = blend_identity(a.blend_color); acc_a = blend_identity(a.blend_alpha); }
    if (blend_fp16) { const float4 v = base_value(); acc_r = v.x; acc_g = v.y; acc_b = v.z; acc_a = v.w; }
    LightStats st;
    const int light_count = a.light_count;
    const float ground_z = a.env.ZAndScale.x, maximum_z = a.env.ZAndScale.y;
    for (int k = 0; k < light_count; k++) {
        const VolumetricRec& L = recs[k];
        const float x0 = L.x0, y0 = L.y0, x1 = L.x1, y1 = L.y1;
        const bool covered = in_image & (cxp >= x0) & (cxp < x1) & (cyp >= y0) & (cyp < y1);
        if (__builtin_amdgcn_ballot_w64(covered) == 0ull)
            continue;
        if (!covered)
            continue;
        if (STATS) st.pairs++;
        float opacity;
        if (!shade_volumetric<FMT, STATS>(P, px, py, L, field, have_sdf, ground_z, maximum_z, st, opacity))
            continue;
        const float cr = L.col_r * opacity, cg = L.col_g * opacity, cb = L.col_b * opacity;
        if constexpr (BLEND) {
            blend_pair(a.blend_color, a.blend_alpha, blend_fp16, cr, cg, cb, acc_r, acc_g, acc_b, acc_a);
        } else if (blend_fp16) {
            acc_r = through_half(acc_r + through_half(cr));
            acc_g = through_half(acc_g + through_half(cg));
            acc_b = through_half(acc_b + through_half(cb));
            acc_a = through_half(acc_a + 1.0f);
        } else {
            acc_r += cr; acc_g += cg; acc_b += cb; acc_a += 1.0f;
        }
    }
    if (!blend_fp16) {
        const float4 v = base_value();
        if constexpr (BLEND) {
            acc_r = blend_onto_base(a.blend_color, v.x, acc_r); acc_g = blend_onto_base(a.blend_color, v.y, acc_g);
            acc_b = blend_onto_base(a.blend_color, v.z, acc_b); acc_a = blend_onto_base(a.blend_alpha, v.w, acc_a);
        } else {
            acc_r = v.x + acc_r; acc_g = v.y + acc_g; acc_b = v.z + acc_b; acc_a = v.w + acc_a;
        }
    }
    if (in_image) {
        const float4 v = mk4(acc_r, acc_g, acc_b, acc_a);
        store_light_texel(a, o, v);
    }
    if (STATS) add_light_stats(st, a.stats, lane);
}

hipError_t launch_prepare_volumetric_lights(const IlmLightVertex* lights, int count, const IlmEnvironment& env, const IlmDistanceFieldUniforms& df,
                                            void* recs, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    (void)df;
    hipLaunchKernelGGL(prepare_volumetric_lights_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, lights, count, env,
                       reinterpret_cast<VolumetricRec*>(recs));
    return hipGetLastError();
}

hipError_t launch_volumetric_lights_prepared(const LightLaunch& a, const void* recs, hipStream_t stream) {
    static const FullFrameKernel<VolumetricRec> blend[4] = { volumetric_lights_kernel<ILM_SDF_FP16 + kBlendVariant, false>, volumetric_lights_kernel<ILM_SDF_FP16 + kBlendVariant, true>,
                                                  volumetric_lights_kernel<ILM_SDF_UNORM16 + kBlendVariant, false>, volumetric_lights_kernel<ILM_SDF_UNORM16 + kBlendVariant, true> };
    return launch_full_frame_lights<VolumetricRec>(a, recs, stream, volumetric_lights_kernel<ILM_SDF_FP16, false>,
                                                   volumetric_lights_kernel<ILM_SDF_FP16, true>, volumetric_lights_kernel<ILM_SDF_UNORM16, false>,
                                                   volumetric_lights_kernel<ILM_SDF_UNORM16, true>, blend);
}

__global__ __launch_bounds__(256) void divide_probe_kernel(const float* __restrict__ n, const float* __restrict__ d, int count,
                                                            float* __restrict__ out_fast, float* __restrict__ out_ieee) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= count) return;
    out_fast[i] = div_no_scale(n[i], d[i]);
    out_ieee[i] = n[i] / d[i];
}

// every one of the 2^32 float bit patterns as the numerator of a division by one constant: div_with_rcp with the constant's
// host-computed reciprocal against `/` (proof by exhaustion for the two constant divisors of shade_light)
__global__ __launch_bounds__(256) void divide_by_constant_kernel(float divisor, float reciprocal, unsigned long long* __restrict__ mismatches) {
    const uint32_t first = ((uint32_t)blockIdx.x * 256u + (uint32_t)threadIdx.x) << 12;      // 2^20 threads x 4096 numerators
    uint32_t bad_inside = 0, bad_outside = 0;
    for (uint32_t k = 0; k < 4096u; k++) {
        const float n = __uint_as_float(first + k);
        const float a = div_with_rcp(n, divisor, reciprocal), b = n / divisor;
        const bool differ = (__float_as_uint(a) != __float_as_uint(b)) && !((a != a) && (b != b));
        // the range the unscaled division is specified for: 2^-60 <= |n| <= 2^60, or zero / infinite / NaN
        const float m = fabsf(n);
        const bool admitted = !(m < 0x1p-60f && m > 0.0f) && !(m > 0x1p60f && m < __builtin_inff());
        bad_inside += (differ && admitted) ? 1u : 0u;
        bad_outside += (differ && !admitted) ? 1u : 0u;
    }
    if (bad_inside) atomicAdd(&mismatches[0], (unsigned long long)bad_inside);
    if (bad_outside) atomicAdd(&mismatches[1], (unsigned long long)bad_outside);
}
hipError_t launch_divide_by_constant(float divisor, float reciprocal, unsigned long long* mismatches, hipStream_t stream) {
    hipLaunchKernelGGL(divide_by_constant_kernel, dim3(4096), dim3(256), 0, stream, divisor, reciprocal, mismatches);
    return hipGetLastError();
}
// the (divisor, reciprocal) pairs shade_light uses
void light_constant_divisors(float out[2][2]) {
    out[0][0] = ref::kDotRampRange; out[0][1] = kDotRampRangeRcp;
    out[1][0] = kVisibilityRange; out[1][1] = kVisibilityRangeRcp;
}

hipError_t launch_divide_probe(const float* n, const float* d, int count, float* out_fast, float* out_ieee, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(divide_probe_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, n, d, count, out_fast, out_ieee);
    return hipGetLastError();
}

}  // namespace ilm
