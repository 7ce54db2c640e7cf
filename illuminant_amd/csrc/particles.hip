// particles.hip -- ParticleEngine per-chunk state update for gfx950.
//
// One launch = one ParticleSystem.Update (Illuminant/Particles/ParticleSystem.cs:725-745):
// the spawner pass, every active transform and the update pass are applied to a
// slot in registers, in the reference's pass order, so a chunk streams through
// HBM once (48 B read + 64 B written per live slot) instead of once per pass.
// State is SoA; one wave = one unit of 64 consecutive slots (one lane = one slot), so every
// access is one dword per lane on an SGPR plane base: 256 contiguous bytes per instruction.
// The hardware dispatcher balances the waves; nothing is persistent or software-pipelined.
//
// Three kernels run a step (launch_step chooses; ilm_debug_last_step_kernel reports), a fourth a batch of steps:
//   step_kernel            interprets any IlmStepDesc: every transform, spawner kind and update mode.  Runs what
//                          the lean kernels do not accept, and everything under ILM_STEP_LEAN=0 / ILM_DF_LEAN=0.
//   step_lean_kernel,      the common shape of a step (power-of-two chunks, UpdatePositions, Gravity / Noise /
//   step_lean_clamp_kernel FMA, inline spawners) from a pre-digested descriptor; the clamp class is the
//                          streaming launch whose curves all have the clamp range.
//   step_lean_df_kernel    the same shape with UpdateWithDistanceField: K units per wave, the colliding
//                          lanes parked and finished at full width.
//   step_batch_kernel      step_kernel's body over the items of ilm_engine_step_batch: many small systems' steps in one
//                          grid, each block finding its item's StepLaunch in a device table.  The lean kernels are not batched.
// The per-slot arithmetic is stated once and shared by all of them (gravity_term, apply_noise, apply_fma,
// spawn_slot, df_long, render_data): the GPU tests hold the kernels to each other bit for bit.
//
// HBM-bound integer/float streaming work: no MFMA; LDS only for the parked lanes of the collision kernel.
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include <atomic>
#include <type_traits>
#include "internal.hpp"
#include "distance_functions.hpp"
#include "bezier.hpp"

namespace ilm {

// ---------------------------------------------------------------------------------------------
// ParticleCommon.fxh:54-72 accessors
// ---------------------------------------------------------------------------------------------
ILM_DEV float dt_seconds(const IlmParticleSystemUniforms& s) { return s.GlobalSettings.x / kVelocityConstantScale; }

// checkCategoryFilter, ParticleCommon.fxh:187-189
ILM_DEV bool category_ok(float type, const float mm[2]) { return (type >= mm[0]) && (type <= mm[1]); }

// randomCustom, RandomCommon.fxh:27-30 (POINT, WRAP)
ILM_DEV float4 random_custom(const float4* __restrict__ rnd, int rw, int rh, float texel_x, float texel_y, float x, float y,
                             float off_x, float off_y, float rate_x, float rate_y) {
#pragma clang fp contract(off)   // table indices are bit-exact
    const float u = ((x * rate_x) + off_x) * texel_x;
    const float v = ((y * rate_y) + off_y) * texel_y;
    const int tx = wrap_index_fast(floorf(u * (float)rw), rw);
    const int ty = wrap_index_fast(floorf(v * (float)rh), rh);
    return rnd[ty * rw + tx];
}

// ---------------------------------------------------------------------------------------------
// DistanceFunctionCommon.fxh -- area weights for FMA / Noise
// ---------------------------------------------------------------------------------------------
// evaluateByTypeId, DistanceFunctionCommon.fxh:170-187
ILM_DEV float evaluate_area(int type_id, f3 wp, const IlmAreaParams& a) {
    const int t = abs(type_id);
    if (t < 1 || t > 5)
        return 0.0f;
    const f3 center = mk3(a.AreaCenter[0], a.AreaCenter[1], a.AreaCenter[2]);
    const f3 size = mk3(a.AreaSize[0], a.AreaSize[1], a.AreaSize[2]);
    const f3 p = rotate_local(wp - center, a.AreaRotation);
    return evaluate_shape(t, p, size);
}
// computeWeight, FMA.fx:15-20 / Noise.fx:21-26
ILM_DEV float compute_weight(const IlmAreaParams& a, f3 wp) {
#pragma clang fp contract(off)
    const float distance = evaluate_area(a.AreaType, wp, a);
    return (1.0f - sat(distance / a.AreaFalloff)) * a.Strength;
}
// weight and time factor of an area transform.  Without an area evaluateByTypeId returns 0, so
// weight = (1 - saturate(0 / falloff)) * Strength = Strength and t = Strength * dtMs / TimeDivisor are uniform:
// both come from the host (StepDerived), computed with the same operations.  AREA = false: the caller's launches never carry an area
// (build_lean_step), so the instantiation holds no evaluateByTypeId code.
template <bool AREA = true>
ILM_DEV void area_weight_and_t(const IlmAreaParams& a, const StepDerived::Op& dv, f3 wp, float dt_ms, float time_divisor, float& weight, float& t) {
#pragma clang fp contract(off)
    if (!AREA || dv.area_none) {
        weight = a.Strength;
        t = dv.t;
    } else {
        weight = compute_weight(a, wp);
        t = weight * dt_ms / time_divisor;
    }
}

// ---------------------------------------------------------------------------------------------
// transforms
// ---------------------------------------------------------------------------------------------
// PS_Gravity, Gravity.fx:12-61.  Every +, -, * rounds as the oracle's (this file is compiled with -ffp-contract=off like the rest of
// the library), so d^2 and the type-0 branch's d^2 - radius are bit-identical to it.  normalize(toCenter), distance / radius and the
// acceleration cap use v_rsq_f32 / v_rcp_f32 (1 ulp -- the accuracy Direct3D itself grants the reference's rcp / rsq / div): relative
// error of each attractor's term <= 4e-7, velocities only.  The gravity-exact build (the Makefile's second library) takes the IEEE
// sqrt / division form, bit-identical to the oracle, at +14 % step time on cfg2 and cfg4 (measured r02: 25.9 -> 29.3 us, 175 -> 201 us).
// One attractor's term of the acceleration (Gravity.fx:36-52); type 0 physical, 1 linear, 2 squared.  The interpreter, the lean
// kernels' loop and their four-at-a-time block all form it here.
ILM_DEV f3 gravity_term(f3 to_center, uint32_t type, float radius, float strength, float dt_ms) {
    float attraction;
    const float d2 = dot3(to_center, to_center);
#ifndef ILM_GRAVITY_EXACT
    const float inv_len = fast_rsq(d2);
    if (type != 0u) {
        const float distance = d2 * inv_len;
        attraction = 1.0f - sat(distance * fast_rcp(radius));
        if (type == 2u)
            attraction *= attraction;
        attraction = attraction * dt_ms * (1.0f / kVelocityConstantScale);
    } else {
        // the one place of this pass where an operand can cancel (d^2 - radius just above its 0.001 floor): the reference's own
        // operations, IEEE division included (the attractor type is uniform: physical-type attractors pay, the others do not)
        const float distance_squared = fmaxf(d2 - radius, 0.001f);
        attraction = 1.0f / distance_squared;
    }
    return ((to_center * inv_len) * attraction) * strength;
#else
    const float distance = sqrtf(d2);
    if (type != 0u) {
        attraction = 1.0f - sat(distance / radius);
        if (type == 2u)
            attraction *= attraction;
        attraction = attraction * dt_ms / kVelocityConstantScale;
    } else {
        const float distance_squared = fmaxf(d2 - radius, 0.001f);
        attraction = 1.0f / distance_squared;
    }
    const f3 n = mk3(to_center.x / distance, to_center.y / distance, to_center.z / distance);
    return (n * attraction) * strength;
#endif
}
// The acceleration cap and the clamped add to the velocity (Gravity.fx:54-60); mv = the system's maximum velocity
ILM_DEV void gravity_finish(float4& vel, f3 acceleration, float maximum_acceleration, float mv) {
#ifndef ILM_GRAVITY_EXACT
    const float a2 = dot3(acceleration, acceleration);
    if (a2 > maximum_acceleration * maximum_acceleration)
        acceleration = acceleration * (fast_rsq(a2) * maximum_acceleration);
#else
    const float current_length = len3(acceleration);
    if (current_length > maximum_acceleration)
        acceleration = mk3(acceleration.x / current_length, acceleration.y / current_length, acceleration.z / current_length) * maximum_acceleration;
#endif
    vel.x = fminf(mv, vel.x + acceleration.x);
    vel.y = fminf(mv, vel.y + acceleration.y);
    vel.z = fminf(mv, vel.z + acceleration.z);
}
ILM_DEV void apply_gravity(float4& pos, float4& vel, const IlmParticleSystemUniforms& sys, const IlmGravityParams& p, const StepDerived::Op& dv) {
    if ((pos.w <= 0.0f) || !category_ok(vel.w, p.CategoryFilter))
        return;
    const float dt_ms = sys.GlobalSettings.x;
    f3 acceleration = mk3(0.0f, 0.0f, 0.0f);
    for (int i = 0; i < p.AttractorCount; i++) {
        const f3 apos = mk3(p.AttractorPositions[i][0], p.AttractorPositions[i][1], p.AttractorPositions[i][2]);
        const float type = p.AttractorRadiusesAndStrengths[i][2];
        acceleration = acceleration + gravity_term(apos - xyz(pos), (type >= 1.5f) ? 2u : ((type >= 0.5f) ? 1u : 0u),
                                                   p.AttractorRadiusesAndStrengths[i][0], p.AttractorRadiusesAndStrengths[i][1], dt_ms);
    }
    gravity_finish(vel, acceleration, dv.max_accel, sys.GlobalSettings.z);
}

ILM_DEV float fma_term_exact(float v, float m, float a) {
#pragma clang fp contract(off)
    return (v * m) + a;
}
// PS_FMA, FMA.fx:22-51.  FILTER = false: the caller has proven that every lane is alive and passes the category filter (the clamp
// class's regular waves, step_lean_block).
template <bool FILTER = true, bool AREA = true>
ILM_DEV void apply_fma(float4& pos, float4& vel, const IlmParticleSystemUniforms& sys, const IlmFMAParams& p, const StepDerived::Op& dv) {
    if (FILTER && ((pos.w <= 0.0f) || !category_ok(vel.w, p.Area.CategoryFilter)))
        return;
    float weight, t;
    area_weight_and_t<AREA>(p.Area, dv, xyz(pos), sys.GlobalSettings.x, p.TimeDivisor, weight, t);
    float4 np = lerp4(pos, add4(mul4(pos, ld4(p.PositionMultiply)), ld4(p.PositionAdd)), t);
    np.w = lerp_exact(pos.w, fma_term_exact(pos.w, p.PositionMultiply.w, p.PositionAdd.w), t);   // life
    const float4 nv = lerp4(vel, add4(mul4(vel, ld4(p.VelocityMultiply)), ld4(p.VelocityAdd)), t);
    pos = np;
    vel = nv;
}

ILM_DEV float4 noise_shape(float4 r, const IlmFloat4& offset, const IlmFloat4& minimum, const IlmFloat4& scale) {
    const float4 d = add4(r, ld4(offset));
    return mk4(sign_times(d.x, fmaxf(fabsf(d.x), minimum.x)) * scale.x, sign_times(d.y, fmaxf(fabsf(d.y), minimum.y)) * scale.y,
               sign_times(d.z, fmaxf(fabsf(d.z), minimum.z)) * scale.z, sign_times(d.w, fmaxf(fabsf(d.w), minimum.w)) * scale.w);
}

// The two noise vectors of a wave whose 64 slots read the same texel in each of the four table lookups
// (StepDerived::NoiseFast): uniform values, held in SGPRs.
struct NoiseDeltas {
    bool valid;
    float4 position, velocity;
};

// positionDelta / velocityDelta of Noise.fx:49-60 from the four table samples
ILM_DEV void noise_deltas(float4 p1, float4 p2, float4 v1, float4 v2, const IlmNoiseParams& p, float4& position_delta, float4& velocity_delta) {
    position_delta = noise_shape(lerp4(p1, p2, p.FrequencyLerp), p.PositionOffset, p.PositionMinimum, p.PositionScale);
    velocity_delta = noise_shape(lerp4(v1, v2, p.FrequencyLerp), p.VelocityOffset, p.VelocityMinimum, p.VelocityScale);
}

// PS_Noise, Noise.fx:28-72 (no life check: dead slots go through the math, :40).  FILTER = false: as for apply_fma.
template <bool FILTER = true, bool AREA = true>
ILM_DEV void apply_noise(float4& pos, float4& vel, float x, float y, const float4* __restrict__ rnd, int rw, int rh,
                         const IlmParticleSystemUniforms& sys, const IlmNoiseParams& p, float inv_rw, float inv_rh, const StepDerived::Op& dv,
                         const NoiseDeltas& uniform) {
    if (FILTER && !category_ok(vel.w, p.Area.CategoryFilter))
        return;
    float weight, t;
    area_weight_and_t<AREA>(p.Area, dv, xyz(pos), sys.GlobalSettings.x, p.TimeDivisor, weight, t);

    float4 position_delta, velocity_delta;
    if (uniform.valid) {
        position_delta = uniform.position;
        velocity_delta = uniform.velocity;
    } else {
        const float rate_x = inv_rw, rate_y = inv_rh;  // rate = RandomnessTexel (Noise.fx:49-52)
        const float4 p1 = random_custom(rnd, rw, rh, rate_x, rate_y, x, y, p.RandomnessOffset[0], p.RandomnessOffset[1], rate_x, rate_y);
        const float4 p2 = random_custom(rnd, rw, rh, rate_x, rate_y, x, y, p.NextRandomnessOffset[0], p.NextRandomnessOffset[1], rate_x, rate_y);
        const float4 v1 = random_custom(rnd, rw, rh, rate_x, rate_y, x + 2.0f, y + 1.0f, p.RandomnessOffset[0], p.RandomnessOffset[1], rate_x, rate_y);
        const float4 v2 = random_custom(rnd, rw, rh, rate_x, rate_y, x + 2.0f, y + 1.0f, p.NextRandomnessOffset[0], p.NextRandomnessOffset[1], rate_x, rate_y);
        noise_deltas(p1, p2, v1, v2, p, position_delta, velocity_delta);
    }

    float4 np = lerp4(pos, add4(pos, position_delta), t);
    np.w = lerp_exact(pos.w, pos.w + position_delta.w, t);   // life
    f3 nv;
    if (p.ReplaceOldVelocity != 0.0f)
        nv = mk3(lerp(vel.x, velocity_delta.x, weight), lerp(vel.y, velocity_delta.y, weight), lerp(vel.z, velocity_delta.z, weight));
    else
        nv = mk3(lerp(vel.x, vel.x + velocity_delta.x, t), lerp(vel.y, vel.y + velocity_delta.y, t), lerp(vel.z, vel.z + velocity_delta.z, t));
    nv = nv + (norm3_fast(xyz(vel)) * velocity_delta.w);
    pos = np;
    vel = mk4(nv.x, nv.y, nv.z, vel.w);
}

// The wave-uniform form of the four lookups (StepDerived::NoiseFast): (x0, row) = slot coordinates of the wave's first lane, the wave
// covers x0 .. x0 + 63 of that row (chunk size a multiple of 64).  Scalar integer code only; the deltas arrive in SGPRs.  The class
// counts are sign bits (2 scalar instructions per boundary); `big` = where the launch keeps the 5 x 5 tables (kNoiseBigClasses).
ILM_DEV NoiseDeltas noise_prepare(const StepDerived::NoiseFast& nf, const IlmFloat4* big, int x0, int row) {
    NoiseDeltas out;
    const uint32_t code = nf.wcode[x0 >> 6];
    out.valid = (code & 64u) != 0u;
    uint32_t yc0 = 0, yc1 = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int b = nf.yb[k];                              // a row >= 0 or INT32_MAX
        yc0 += (uint32_t)(b - 1 - row) >> 31;                // row >= b
        yc1 += (uint32_t)(b - 2 - row) >> 31;                // row + 1 >= b
    }
    const uint32_t xc0 = code & 7u, xc1 = (code >> 3) & 7u;
    const uint32_t n = (uint32_t)nf.classes;
    const IlmFloat4* table = (n == (uint32_t)kNoiseBigClasses) ? big : &nf.position[0][0];   // position[n][n] then velocity[n][n]
    out.position = ld4(table[yc0 * n + xc0]);
    out.velocity = ld4(table[n * n + yc1 * n + xc1]);
    return out;
}
static_assert(offsetof(StepDerived::NoiseFast, velocity) == offsetof(StepDerived::NoiseFast, position) + 9 * sizeof(IlmFloat4), "velocity[3][3] follows position[3][3]");

// mul3, ParticleCommon.fxh:183-196
ILM_DEV float4 mul_point(f3 v, const IlmMatrix& M);
ILM_DEV float4 mul3(float4 old_value, const IlmMatrix& mat, float w) {
    const float4 temp = mul_point(xyz(old_value), mat);
    if (w != 0.0f)
        return mk4(temp.x / temp.w, temp.y / temp.w, temp.z / temp.w, old_value.w);
    return mk4(temp.x, temp.y, temp.z, old_value.w);
}

// PS_MatrixMultiply, MatrixMultiply.fx:22-52
ILM_DEV void apply_matrix_multiply(float4& pos, float4& vel, const IlmParticleSystemUniforms& sys, const IlmMatrixMultiplyParams& p) {
#pragma clang fp contract(off)
    if ((pos.w <= 0.0f) || !category_ok(vel.w, p.Area.CategoryFilter))
        return;
    const float time_scale = (p.TimeDivisor >= 0.0f) ? sys.GlobalSettings.x / p.TimeDivisor : 1.0f;
    const float distance = evaluate_area(p.Area.AreaType, xyz(pos), p.Area);
    const float w = ((1.0f - clampf(distance / p.Area.AreaFalloff, 0.0f, 1.0f)) * p.Area.Strength) * time_scale;
    const float4 np = lerp4(pos, mul3(pos, p.PositionMatrix, 1.0f), w);
    const float4 nv = lerp4(vel, mul3(vel, p.VelocityMatrix, 0.0f), w);
    pos = np;
    vel = nv;
}

// smoothRandomCustom, RandomCommon.fxh:36-39: bilinear, WRAP on both axes, on the Rgba64 copy of the randomness table
ILM_DEV float4 smooth_random_custom(const uint2* __restrict__ lp, int rw, int rh, float texel_x, float texel_y, float x, float y,
                                    float off_x, float off_y, float rate_x, float rate_y) {
#pragma clang fp contract(off)
    const float u = ((x * rate_x) + off_x) * texel_x;
    const float v = ((y * rate_y) + off_y) * texel_y;
    const float sx = u * (float)rw - 0.5f, sy = v * (float)rh - 0.5f;
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    // The index follows particle positions (state, not a uniform), so it is decided exactly for every float.  x1 is the integer x0 + 1
    // wrapped (x0f + 1.0f would round back onto x0f from 2^24 on, where the fraction is 0).
    const int x0 = wrap_index(x0f, rw), y0 = wrap_index(y0f, rh);
    const int x1 = (x0 + 1 == rw) ? 0 : x0 + 1, y1 = (y0 + 1 == rh) ? 0 : y0 + 1;
    const uint2 t00 = lp[y0 * rw + x0], t10 = lp[y0 * rw + x1], t01 = lp[y1 * rw + x0], t11 = lp[y1 * rw + x1];
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint32_t w00 = (c < 2) ? t00.x : t00.y, w10 = (c < 2) ? t10.x : t10.y, w01 = (c < 2) ? t01.x : t01.y, w11 = (c < 2) ? t11.x : t11.y;
        const int sh = (c & 1) * 16;
        const float a = unorm16_to_float((float)((w00 >> sh) & 0xFFFFu)), b = unorm16_to_float((float)((w10 >> sh) & 0xFFFFu));
        const float cc = unorm16_to_float((float)((w01 >> sh) & 0xFFFFu)), d = unorm16_to_float((float)((w11 >> sh) & 0xFFFFu));
        r[c] = lerp(lerp(a, b, fx), lerp(cc, d, fx), fy);
    }
    return mk4(r[0], r[1], r[2], r[3]);
}

// PS_SpatialNoise, Noise.fx:74-116 (no life check, no Minimum shaping)
ILM_DEV void apply_spatial_noise(float4& pos, float4& vel, const uint2* __restrict__ lp, int rw, int rh,
                                 const IlmParticleSystemUniforms& sys, const IlmSpatialNoiseParams& sp, const StepDerived& sd) {
#pragma clang fp contract(off)
    const IlmNoiseParams& p = sp.Noise;
    if (!category_ok(vel.w, p.Area.CategoryFilter))
        return;
    const float weight = compute_weight(p.Area, xyz(pos));
    const float t = weight * sys.GlobalSettings.x / p.TimeDivisor;
    const float rx = pos.x, ry = pos.y, sx = sp.SpaceScale[0], sy = sp.SpaceScale[1];
    const float4 p1 = smooth_random_custom(lp, rw, rh, sd.inv_rw, sd.inv_rh, rx, ry, p.RandomnessOffset[0], p.RandomnessOffset[1], sx, sy);
    const float4 p2 = smooth_random_custom(lp, rw, rh, sd.inv_rw, sd.inv_rh, rx, ry, p.NextRandomnessOffset[0], p.NextRandomnessOffset[1], sx, sy);
    const float4 v1 = smooth_random_custom(lp, rw, rh, sd.inv_rw, sd.inv_rh, rx + 2.0f, ry + 1.0f, p.RandomnessOffset[0], p.RandomnessOffset[1], sx, sy);
    const float4 v2 = smooth_random_custom(lp, rw, rh, sd.inv_rw, sd.inv_rh, rx + 2.0f, ry + 1.0f, p.NextRandomnessOffset[0], p.NextRandomnessOffset[1], sx, sy);
    const float4 position_delta = mul4(add4(lerp4(p1, p2, p.FrequencyLerp), ld4(p.PositionOffset)), ld4(p.PositionScale));
    const float4 velocity_delta = mul4(add4(lerp4(v1, v2, p.FrequencyLerp), ld4(p.VelocityOffset)), ld4(p.VelocityScale));
    const float4 np = lerp4(pos, add4(pos, position_delta), t);
    f3 nv;
    if (p.ReplaceOldVelocity != 0.0f)
        nv = mk3(lerp(vel.x, velocity_delta.x, weight), lerp(vel.y, velocity_delta.y, weight), lerp(vel.z, velocity_delta.z, weight));
    else
        nv = mk3(lerp(vel.x, vel.x + velocity_delta.x, t), lerp(vel.y, vel.y + velocity_delta.y, t), lerp(vel.z, vel.z + velocity_delta.z, t));
    nv = nv + (norm3(xyz(vel)) * velocity_delta.w);
    pos = np;
    vel = mk4(nv.x, nv.y, nv.z, vel.w);
}

// ---------------------------------------------------------------------------------------------
// spawner -- SpawnerCommon.fxh + PS_Spawn (SpawnParticles.fx:10-30)
// ---------------------------------------------------------------------------------------------
ILM_DEV f3 random_normal3(float rx, float ry) {
    const float phi = rx * kPi * 2.0f;
    const float costheta = (ry - 0.5f) * 2.0f;
    const float theta = acosf(costheta);
    float st, ct, sp, cp;
    st = sinf(theta); ct = cosf(theta); sp = sinf(phi); cp = cosf(phi);
    return mk3(st * cp, st * sp, ct);
}

// evaluateFormula, SpawnerCommon.fxh:59-104
ILM_DEV float4 evaluate_formula(float4 origin, float4 constant, float4 scale, float4 offset, float4 randomness,
                                float type, const float axis_mask[3]) {
    const float4 type0 = add4(constant, mul4(add4(randomness, offset), scale));
    const unsigned itype = (unsigned)fabsf(floorf(type));
    if (itype == 1u || itype == 3u) {
        f3 rn = random_normal3(randomness.x, randomness.y);
        rn = norm3(mk3(rn.x * axis_mask[0], rn.y * axis_mask[1], rn.z * axis_mask[2]));
        f3 circular = mk3(rn.x * randomness.z * scale.x, rn.y * randomness.z * scale.y, rn.z * randomness.z * scale.z);
        f3 result;
        if (itype == 3u) {
            const float sqrt2 = 1.41421356237f;
            const f3 edge = mk3(fabsf(offset.x), fabsf(offset.y), fabsf(offset.z));
            result = mk3(clampf(offset.x * rn.x * sqrt2, -edge.x, edge.x), clampf(offset.y * rn.y * sqrt2, -edge.y, edge.y),
                         clampf(offset.z * rn.z * sqrt2, -edge.z, edge.z));
            result = result + (xyz(constant) + circular);
        } else {
            circular = circular + (rn * xyz(offset));
            result = xyz(constant) + circular;
        }
        return mk4(result.x, result.y, result.z, type0.w);
    }
    if (itype == 2u) {
        const f3 distance = xyz(constant) - xyz(origin);
        const float ldistance = len3(distance);
        if (ldistance < 0.1f)
            return mk4(0.0f, 0.0f, 0.0f, constant.w);
        const f3 direction = mk3(distance.x / ldistance, distance.y / ldistance, distance.z / ldistance);
        const f3 random_speed = mk3(randomness.x * scale.x * direction.x, randomness.x * scale.y * direction.y, randomness.x * scale.z * direction.z);
        const f3 s = random_speed + (xyz(offset) * direction);
        return mk4(s.x, s.y, s.z, type0.w);
    }
    return type0;
}

ILM_DEV float4 mul_point(f3 v, const IlmMatrix& M) {
    const float* m = M.m;
    return mk4(v.x * m[0] + v.y * m[4] + v.z * m[8] + m[12], v.x * m[1] + v.y * m[5] + v.z * m[9] + m[13],
               v.x * m[2] + v.y * m[6] + v.z * m[10] + m[14], v.x * m[3] + v.y * m[7] + v.z * m[11] + m[15]);
}

// index % m for an integer-valued index in [0, 2^24) and a literal integer m: HLSL's float % is exact here, and so
// is the integer remainder (which the compiler turns into a multiply-high); OCML's fmodf is a ~100-instruction loop.
template <unsigned M>
ILM_DEV float mod_const(float index) { return (float)((unsigned)index % M); }

// evaluateRandomForIndex, SpawnerCommon.fxh:106-117
ILM_DEV void evaluate_random_for_index(const float4* __restrict__ rnd, int rw, int rh, float tx_, float ty_, float index, const IlmSpawnParams& p,
                                       float4& random1, float4& random2, float4& random3) {
    const float ox = p.RandomnessOffset[0], oy = p.RandomnessOffset[1];
    random1 = random_custom(rnd, rw, rh, tx_, ty_, mod_const<ref::kRandom1XModulus>(index), 0.0f + mod_const<ref::kRandom1YModulus>(index), ox, oy, 1.0f, 1.0f);
    random2 = random_custom(rnd, rw, rh, tx_, ty_, mod_const<ref::kRandom2XModulus>(index), 1.0f + mod_const<ref::kRandom2YModulus>(index), ox, oy, 1.0f, 1.0f);
    random3 = random_custom(rnd, rw, rh, tx_, ty_, mod_const<ref::kRandom3XModulus>(index), 2.0f + mod_const<ref::kRandom3YModulus>(index), ox, oy, 1.0f, 1.0f);
    // "The x and y element of random samples determines the normal" (:114-116): inside evaluateRandomForIndex, so the feedback and
    // pattern spawners (SpawnParticles.fx:83, PatternSpawner.fx:63) align too
    if (p.AlignVelocityAndPosition != 0.0f) {
        random2.x = random1.x;
        random2.y = random1.y;
    }
}

// Spawn_Stage1, SpawnerCommon.fxh:119-160: the slot test, the three random vectors and the position-constant indices
ILM_DEV bool spawn_stage1(float x, float y, const float4* __restrict__ rnd, int rw, int rh, float tx_, float ty_, const IlmSpawnParams& p,
                          float4& random1, float4& random2, float4& random3, int& index1, int& index2, float& position_index_t) {
    const float index = x + (y * p.ChunkSizeAndIndices[0]);
    if ((index < p.ChunkSizeAndIndices[1]) || (index > p.ChunkSizeAndIndices[2]))
        return false;
    evaluate_random_for_index(rnd, rw, rh, tx_, ty_, index, p, random1, random2, random3);
    const float relative_index = index - p.ChunkSizeAndIndices[1];
    if (p.PolygonRate > 0.05f) {
        const float position_index_f = (relative_index / p.PolygonRate) + p.ChunkSizeAndIndices[3];
        const float divisor = p.PositionConstantCount;
        float position_index_i;
        position_index_t = modff(position_index_f, &position_index_i);
        // position_index_i is finite and >= 0 and divisor an integer in [1, count] (validate_step): fmodf is exact and in [0, divisor)
        index1 = (int)fmodf(position_index_i, divisor);
        if (p.PolygonLoop != 0.0f)
            index2 = (int)fmodf(position_index_i + 1.0f, divisor);
        else
            index2 = (int)fminf((float)(index1 + 1), divisor - 1.0f);
    } else {
        // integer-valued operands (slot index + TotalSpawned % count, the position count; validate_step refuses any other .w or
        // count), >= 0 and below 2^24 + 2^20.  wrap_index_fast is exact below 2^23 (every inline spawner); a position buffer's larger
        // indices take the exact integer remainder.
        const float t = relative_index + p.ChunkSizeAndIndices[3];
        const int count = (int)p.PositionConstantCount;
        index1 = index2 = (t < 0x1p23f) ? wrap_index_fast(t, count) : wrap_index(t, count);
        position_index_t = 0.0f;
    }
    return true;
}

// Spawn_Stage2, SpawnerCommon.fxh:162-190.  Returns false on the alpha discard.
ILM_DEV bool spawn_stage2(float4 position1, float4 position2, float position_index_t, float4 random1, float4 random2, float4 random3,
                          const IlmSpawnParams& p, float4& pos, float4& vel, float4& attr) {
    const float4 position_constant = lerp4(position1, position2, position_index_t);
    const float4 towards_next = sub4(position2, position1);

    const float4 zero = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 temp_position = evaluate_formula(zero, position_constant, ld4(p.Configuration[0]), ld4(p.Configuration[1]),
                                                  random1, p.FormulaTypes[0], p.AxisMask);
    float4 new_position = mul_point(xyz(temp_position), p.PositionMatrix);
    new_position.w = temp_position.w;

    float4 temp_velocity = evaluate_formula(temp_position, ld4(p.Configuration[2]), ld4(p.Configuration[3]), ld4(p.Configuration[4]),
                                            random2, p.FormulaTypes[1], p.AxisMask);
    const float4 new_attributes = evaluate_formula(zero, ld4(p.Configuration[5]), ld4(p.Configuration[6]), ld4(p.Configuration[7]),
                                                   random3, p.FormulaTypes[2], p.AxisMask);

    const float towards_distance = sqrtf(towards_next.x * towards_next.x + towards_next.y * towards_next.y +
                                         towards_next.z * towards_next.z + towards_next.w * towards_next.w);
    if (towards_distance > 0.0001f) {
        const float c = p.Configuration[8].x, s = p.Configuration[8].y, o = p.Configuration[8].z, r = random3.w;
        const float towards_speed = evaluate_formula(zero, mk4(c, c, c, c), mk4(s, s, s, s), mk4(o, o, o, o), mk4(r, r, r, r),
                                                     p.FormulaTypes[3], p.AxisMask).x;
        temp_velocity = add4(temp_velocity, mk4((towards_next.x / towards_distance) * towards_speed, (towards_next.y / towards_distance) * towards_speed,
                                                (towards_next.z / towards_distance) * towards_speed, (towards_next.w / towards_distance) * towards_speed));
    }
    float4 new_velocity = mul_point(xyz(temp_velocity), p.VelocityMatrix);
    new_velocity.w = temp_velocity.w;

    if (new_attributes.w < p.AttributeDiscardThreshold)
        return false;
    pos = new_position;
    vel = new_velocity;
    attr = new_attributes;
    return true;
}

// PS_Spawn, SpawnParticles.fx:10-30.  Returns true when the slot was (re)written by the spawner.
ILM_DEV bool spawn_slot(float4& pos, float4& vel, float4& attr, float x, float y,
                        const float4* __restrict__ rnd, int rw, int rh, float tx_, float ty_, const IlmSpawnParams& p) {
    float4 random1, random2, random3;
    int index1, index2;
    float position_index_t;
    if (!spawn_stage1(x, y, rnd, rw, rh, tx_, ty_, p, random1, random2, random3, index1, index2, position_index_t))
        return false;
    index1 = min(max(index1, 0), ILM_MAX_INLINE_POSITION_CONSTANTS - 1);
    index2 = min(max(index2, 0), ILM_MAX_INLINE_POSITION_CONSTANTS - 1);
    return spawn_stage2(ld4(p.InlinePositionConstants[index1]), ld4(p.InlinePositionConstants[index2]), position_index_t,
                        random1, random2, random3, p, pos, vel, attr);
}

// tex2Dlod(PositionConstantSampler, index * PositionConstantTexel.x): POINT / CLAMP on the Spawner's PositionBuffer, whose width is
// the count rounded up to a multiple of 128 and whose padding stays zero (ParticleSpawner.cs:301-314, SpawnParticles.fx:47-48)
ILM_DEV float4 position_constant_fetch(const float4* __restrict__ positions, int count, int index) {
#pragma clang fp contract(off)
    const int width = (count + 127) / 128 * 128;
    const float texel = 1.0f / (float)width;
    const float u = (float)index * texel;
    const int tx = clamp_tap(floorf(u * (float)width), width);
    return (tx < count) ? positions[tx] : mk4(0.0f, 0.0f, 0.0f, 0.0f);
}

// PS_SpawnFromPositionTexture, SpawnParticles.fx:32-52
ILM_DEV bool spawn_slot_position_buffer(float4& pos, float4& vel, float4& attr, float x, float y, const float4* __restrict__ rnd, int rw, int rh,
                                        float tx_, float ty_, const IlmSpawnParams& p, const float4* __restrict__ positions, int count) {
    float4 random1, random2, random3;
    int index1, index2;
    float position_index_t;
    if (!spawn_stage1(x, y, rnd, rw, rh, tx_, ty_, p, random1, random2, random3, index1, index2, position_index_t))
        return false;
    return spawn_stage2(position_constant_fetch(positions, count, index1), position_constant_fetch(positions, count, index2), position_index_t,
                        random1, random2, random3, p, pos, vel, attr);
}

// PS_SpawnFeedback, SpawnParticles.fx:54-118.  `src` = plane 0 of the source chunk (same stride S and chunk size as the target:
// SourceChunkSizeAndTexel = (size, 1/size, 1/size), ParticleTransform.cs:129-141).
ILM_DEV bool spawn_slot_feedback(float4& pos, float4& vel, float4& attr, float x, float y, const float4* __restrict__ rnd, int rw, int rh,
                                 float tx_, float ty_, const IlmSpawnParams& p, const IlmFeedbackParams& fb,
                                 const float* __restrict__ src, int64_t S, int chunk_size) {
#pragma clang fp contract(off)
    const float index = x + (y * p.ChunkSizeAndIndices[0]);
    if ((index < p.ChunkSizeAndIndices[1]) || (index > p.ChunkSizeAndIndices[2]))
        return false;
    const float size = (float)chunk_size, texel = 1.0f / (float)chunk_size;
    const float source_index = ((index - p.ChunkSizeAndIndices[1]) / fb.InstanceMultiplier) + fb.FeedbackSourceIndex;
    float source_y;
    const float source_x = modff(source_index / size, &source_y) * size;
    // readStateUv: POINT / CLAMP at uv = sourceXy * texel
    const int tx = clamp_tap(floorf((source_x * texel) * size), chunk_size);
    const int ty = clamp_tap(floorf((source_y * texel) * size), chunk_size);
    const int si = ty * chunk_size + tx;
    const float4 source_position = mk4(src[si], src[S + si], src[2 * S + si], src[3 * S + si]);
    if ((source_position.w <= fb.SourceLifeRange[0]) || (source_position.w >= fb.SourceLifeRange[1]))
        return false;
    const float4 source_velocity = mk4(src[4 * S + si], src[5 * S + si], src[6 * S + si], src[7 * S + si]);
    const float4 source_attributes = mk4(src[8 * S + si], src[9 * S + si], src[10 * S + si], src[11 * S + si]);

    float4 random1, random2, random3;
    evaluate_random_for_index(rnd, rw, rh, tx_, ty_, index, p, random1, random2, random3);

    const float4 zero = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 position_constant = ld4(p.InlinePositionConstants[0]);
    if (fb.AlignPositionConstant != 0.0f) {
        position_constant.x += source_position.x; position_constant.y += source_position.y; position_constant.z += source_position.z;
    }
    const float4 temp_position = evaluate_formula(zero, position_constant, ld4(p.Configuration[0]), ld4(p.Configuration[1]),
                                                  random1, p.FormulaTypes[0], p.AxisMask);
    float4 attribute_constant = ld4(p.Configuration[5]);
    if (fb.MultiplyAttributeConstant != 0.0f)
        attribute_constant = mul4(attribute_constant, source_attributes);
    float4 new_position = mul_point(xyz(temp_position), p.PositionMatrix);
    new_position.w = temp_position.w;
    if (fb.MultiplyLife != 0.0f)
        new_position.w *= source_position.w;
    float4 temp_velocity = evaluate_formula(temp_position, ld4(p.Configuration[2]), ld4(p.Configuration[3]), ld4(p.Configuration[4]),
                                            random2, p.FormulaTypes[1], p.AxisMask);
    temp_velocity = add4(temp_velocity, mk4(source_velocity.x * fb.SourceVelocityFactor, source_velocity.y * fb.SourceVelocityFactor,
                                            source_velocity.z * fb.SourceVelocityFactor, source_velocity.w * fb.SourceVelocityFactor));
    float4 new_velocity = mul_point(xyz(temp_velocity), p.VelocityMatrix);
    new_velocity.w = temp_velocity.w;
    const float4 new_attributes = evaluate_formula(temp_position, attribute_constant, ld4(p.Configuration[6]), ld4(p.Configuration[7]),
                                                   random3, p.FormulaTypes[2], p.AxisMask);
    if (new_attributes.w < p.AttributeDiscardThreshold)
        return false;
    pos = new_position;
    vel = new_velocity;
    attr = new_attributes;
    return true;
}

// tex2Dlod(PatternSampler, float4(uv, 0, lod)): CLAMP, LINEAR min / mag, POINT mip (PatternSpawner.fx:11-19).  `tex` holds the mip
// levels back to back (include/illuminant_hip.h, ilm_system_set_spawn_pattern); texel centres sit at integer + 0.5.
ILM_DEV float4 pattern_fetch(const float4* __restrict__ tex, int w, int h, int levels, float u, float v, float lod) {
#pragma clang fp contract(off)
    const int level = clamp_tap(floorf(lod + 0.5f), levels);
    int lw = w, lh = h;
    for (int l = 0; l < level; l++) {
        tex += lw * lh;
        lw = max(1, lw >> 1); lh = max(1, lh >> 1);
    }
    const float sx = u * (float)lw - 0.5f, sy = v * (float)lh - 0.5f;
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    // clamp in float first: u, v are unbounded below (the caller only rejects coordinates above 1)
    const int x0 = (int)fminf(fmaxf(x0f, 0.0f), (float)(lw - 1)), x1 = (int)fminf(fmaxf(x0f + 1.0f, 0.0f), (float)(lw - 1));
    const int y0 = (int)fminf(fmaxf(y0f, 0.0f), (float)(lh - 1)), y1 = (int)fminf(fmaxf(y0f + 1.0f, 0.0f), (float)(lh - 1));
    const float4 t00 = tex[y0 * lw + x0], t10 = tex[y0 * lw + x1], t01 = tex[y1 * lw + x0], t11 = tex[y1 * lw + x1];
    return lerp4(lerp4(t00, t10, fx), lerp4(t01, t11, fx), fy);
}

// PS_SpawnPattern, PatternSpawner.fx:21-97
ILM_DEV bool spawn_slot_pattern(float4& pos, float4& vel, float4& attr, float x, float y, const float4* __restrict__ rnd, int rw, int rh,
                                float tx_, float ty_, const IlmSpawnParams& p, const IlmPatternParams& pt,
                                const float4* __restrict__ tex, int tw, int th, int levels) {
#pragma clang fp contract(off)
    const float index = x + (y * p.ChunkSizeAndIndices[0]);
    if ((index < p.ChunkSizeAndIndices[1]) || (index > p.ChunkSizeAndIndices[2]))
        return false;
    const float relative_index = floorf(index - p.ChunkSizeAndIndices[1]);
    const float particles_per_row = pt.StepWidthAndSizeScale[1];
    // integer-valued operands below 2^24: the quotient's floor and the remainder are exact (HLSL's float %)
    const float row = floorf(relative_index / particles_per_row);
    float ix = floorf(relative_index - (particles_per_row * row)), iy = row;
    iy += pt.YOffsetsAndCoordScale[0];
    const float u = (ix * pt.StepWidthAndSizeScale[2]) + pt.TexelOffsetAndMipBias[0];
    const float v = ((iy * pt.StepWidthAndSizeScale[3]) + pt.TexelOffsetAndMipBias[1]) + pt.YOffsetsAndCoordScale[1];
    const float position_x = ix * pt.YOffsetsAndCoordScale[2] + pt.CenteringOffset[0];
    const float position_y = iy * pt.YOffsetsAndCoordScale[3] + pt.CenteringOffset[1];
    if ((u > 1.0f) || (v > 1.0f))
        return false;
    const float4 pattern_color = pattern_fetch(tex, tw, th, levels, u, v, pt.TexelOffsetAndMipBias[3]);

    float4 random1, random2, random3;
    evaluate_random_for_index(rnd, rw, rh, tx_, ty_, index, p, random1, random2, random3);

    const float4 zero = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 temp_position = evaluate_formula(zero, ld4(p.InlinePositionConstants[0]), ld4(p.Configuration[0]), ld4(p.Configuration[1]),
                                            random1, p.FormulaTypes[0], p.AxisMask);
    temp_position.x += position_x;
    temp_position.y += position_y;
    float4 attribute_constant = pattern_color;
    if (pt.MultiplyAttributeConstant != 0.0f)
        attribute_constant = mul4(attribute_constant, ld4(p.Configuration[5]));
    else
        attribute_constant = add4(attribute_constant, ld4(p.Configuration[5]));
    float4 new_position = mul_point(xyz(temp_position), p.PositionMatrix);
    new_position.w = temp_position.w;
    const float4 temp_velocity = evaluate_formula(temp_position, ld4(p.Configuration[2]), ld4(p.Configuration[3]), ld4(p.Configuration[4]),
                                                  random2, p.FormulaTypes[1], p.AxisMask);
    float4 new_velocity = mul_point(xyz(temp_velocity), p.VelocityMatrix);
    new_velocity.w = temp_velocity.w;
    const float4 new_attributes = evaluate_formula(temp_position, attribute_constant, ld4(p.Configuration[6]), ld4(p.Configuration[7]),
                                                   random3, p.FormulaTypes[2], p.AxisMask);
    if (new_attributes.w < p.AttributeDiscardThreshold)
        return false;
    pos = new_position;
    vel = new_velocity;
    attr = new_attributes;
    return true;
}

// ---------------------------------------------------------------------------------------------
// update -- Bezier.fxh, UpdateCommon.fxh, UpdateParticleSystem*.fx
// ---------------------------------------------------------------------------------------------
// applyFrictionAndMaximum, UpdateCommon.fxh:20-35
ILM_DEV f3 friction_and_maximum(f3 velocity, const IlmParticleSystemUniforms& sys, float dts) {
    // v_sqrt_f32 / v_rcp_f32 (1 ulp; only velocities depend on them) behave like the reference's length() / normalize() at the
    // edges: a NaN or infinite speed fails `l <= 0.001` and poisons the same components as dividing by it would
    float l = len3_fast(velocity);
    const float inv_l = fast_rcp(l);
    if (l <= 0.001f)
        return mk3(0.0f, 0.0f, 0.0f);
    const float mv = sys.GlobalSettings.z;
    if (l > mv)
        l = mv;
    const float friction = l * sys.GlobalSettings.y;
    l -= (friction * dts);
    l = clampf(l, 0.0f, mv);
    return velocity * (inv_l * l);
}

// Pieces of computeRenderData that step_lean_kernel also evaluates for the state it loaded (its store elision).
ILM_DEV float render_index(float vx, float vy) { return vx + (vy * ref::kRenderDataIndexRowPitch); }   // reference quirk: 256 regardless of ChunkSize (:107)
// getRotationForVelocity x getVelocityRotation() when the latter is 0 (update_bits bit 1): 0, or NaN for a NaN velocity (see render_data)
ILM_DEV float rotation_unscaled(float vx, float vy) { return ((vx != vx) || (vy != vy)) ? __builtin_nanf("") : 0.0f; }
ILM_DEV float render_rotation(float rotation, float life, float index, const IlmParticleSystemUniforms& sys, const IlmUpdateParams& p) {
    return (rotation * sys.AnimationRateAndRotationAndZToY.z) + ((life * p.RotationFromLifeAndIndex[0]) + (index * p.RotationFromLifeAndIndex[1]));
}

// computeRenderData, UpdateCommon.fxh:96-117.  `codes` / `bits`: the uniform decisions of the four curves, the life ramp and the
// velocity rotation, taken on the host (StepDerived::bezier_codes / update_bits).
ILM_DEV void render_data(float vx, float vy, float4 position, float4 velocity, float4 attributes,
                         const IlmParticleSystemUniforms& sys, const IlmUpdateParams& p, uint32_t codes, uint32_t bits,
                         const float4* __restrict__ ramp, int ramp_w, int ramp_h,
                         float4& render_color, float4& rdata) {
    if (position.w <= 0.0f) {
        render_color = rdata = mk4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float index = render_index(vx, vy);
    const float velocity_length = fmaxf(len3_fast(xyz(velocity)), 0.0001f);

    float4 color = mul4(bezier4_coded(p.ColorFromLife, position.w, codes & 0xFFu), bezier4_coded(p.ColorFromVelocity, velocity_length, (codes >> 8) & 0xFFu));
    if (bits & 1u) {    // p.LifeRampSettings.x != 0
        float u = (position.w - p.LifeRampSettings.y) / p.LifeRampSettings.z;
        if (bits & 4u)  // p.LifeRampSettings.x < 0
            u = 1.0f - sat(u);
        const float v = index / p.LifeRampSettings.w;
        float4 texel = mk4(1.0f, 1.0f, 1.0f, 1.0f);
        if (ramp != nullptr && ramp_w > 0 && ramp_h > 0) {
            // U CLAMP, decided in float before the cast (NaN: column 0); V WRAP, exact for every float
            const int tx = clamp_tap(floorf(u * (float)ramp_w), ramp_w);
            const int ty = wrap_index(floorf(v * (float)ramp_h), ramp_h);             // V WRAP
            texel = ramp[ty * ramp_w + tx];
        }
        color = lerp4(color, mul4(texel, color), sat(fabsf(p.LifeRampSettings.x)));
    }

    float4 rc = mul4(attributes, color);
    rc.w = sat(rc.w);
    rc.x *= rc.w; rc.y *= rc.w; rc.z *= rc.w;
    render_color = rc;

    // getRotationForVelocity, UpdateCommon.fxh:81-94
    float rotation = 0.0f;
    // the angle is multiplied by getVelocityRotation(): skipping atan2 when that is 0 is exact for every finite or infinite velocity
    // (the angle is finite); a NaN velocity (normalize(0) upstream) makes the angle NaN and NaN * 0 stays NaN
    if (bits & 2u) {    // sys.AnimationRateAndRotationAndZToY.z == 0
        rotation = rotation_unscaled(velocity.x, velocity.y);
    } else if (!((fabsf(velocity.x) < 0.01f) && (fabsf(velocity.y) < 0.01f))) {
        rotation = atan2f(velocity.y, velocity.x);
        if (rotation < 0.0f)
            rotation += 2.0f * kPi;
    }
    rdata.x = bezier1_coded(p.SizeFromLife, position.w, (codes >> 16) & 0xFFu) * bezier1_coded(p.SizeFromVelocity, velocity_length, codes >> 24);
    rdata.y = render_rotation(rotation, position.w, index, sys, p);
    rdata.z = velocity_length;
    rdata.w = velocity.w;
}

// PS_Update, UpdateParticleSystem.fx:9-38 (live slot)
ILM_DEV void update_positions(float4& pos, float4& vel, const IlmParticleSystemUniforms& sys, float dts) {
#pragma clang fp contract(off)   // life arithmetic is bit-exact
    const f3 velocity = friction_and_maximum(xyz(vel), sys, dts);
    const float new_life = pos.w - (sys.GlobalSettings.w * dts);
    if (new_life <= 0.0f) {
        pos = vel = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
        pos = mk4(pos.x + velocity.x * dts, pos.y + velocity.y * dts, pos.z + velocity.z * dts, new_life);
        vel = mk4(velocity.x, velocity.y, velocity.z, vel.w);
    }
}
// The same for every lane at once: `live` says which lanes are a live slot after the transforms, the others (and a life that runs out
// here) come out as the cleared target's zeros.  One select per component where nested lane-divergent branches would each zero all eight.
ILM_DEV void update_positions_select(float4& pos, float4& vel, const IlmParticleSystemUniforms& sys, float dts, bool live) {
#pragma clang fp contract(off)   // life arithmetic is bit-exact
    const f3 velocity = friction_and_maximum(xyz(vel), sys, dts);
    const float new_life = pos.w - (sys.GlobalSettings.w * dts);
    const bool keep = live && !(new_life <= 0.0f);
    pos = mk4(keep ? pos.x + velocity.x * dts : 0.0f, keep ? pos.y + velocity.y * dts : 0.0f, keep ? pos.z + velocity.z * dts : 0.0f, keep ? new_life : 0.0f);
    vel = mk4(keep ? velocity.x : 0.0f, keep ? velocity.y : 0.0f, keep ? velocity.z : 0.0f, keep ? vel.w : 0.0f);
}
// update_positions_select's values before its selects: what it keeps for a lane that is alive after the transforms and after the decay.
ILM_DEV void update_positions_unselected(float4& pos, float4& vel, const IlmParticleSystemUniforms& sys, float dts) {
#pragma clang fp contract(off)   // life arithmetic is bit-exact
    const f3 velocity = friction_and_maximum(xyz(vel), sys, dts);
    const float new_life = pos.w - (sys.GlobalSettings.w * dts);
    pos = mk4(pos.x + velocity.x * dts, pos.y + velocity.y * dts, pos.z + velocity.z * dts, new_life);
    vel = mk4(velocity.x, velocity.y, velocity.z, vel.w);
}

// Diagnostic (ilm_debug_step_sdf_samples): how many sampleDistanceFieldEx calls the collision update makes -- the unit of its roofline
// (bench.py collision_step_1m).  The flag is read by a scalar load; the counter costs nothing while it is off.
__device__ unsigned long long g_step_sdf_samples;
__device__ int g_step_count_sdf_samples;
// Diagnostic (ilm_debug_step_regular_waves): which body the waves of step_lean_clamp_kernel ran.  [0]: the regular body to its end,
// [1]: the regular transforms, then the selecting update and tail (the second ballot failed).  Every other wave ran the selecting body
// from the top.  The flag is read by one scalar load per wave; off, that load and a branch are the whole cost.
__device__ unsigned long long g_step_regular_waves[2];
__device__ int g_step_count_regular_waves;      // bit 0: count g_step_regular_waves, bit 1: count g_step_category_waves (one flag, one load)
// Diagnostic (ilm_debug_step_category_waves): what the waves of step_lean_clamp_kernel did about the category plane.  [0]: never loaded it
// (the chunk's category record admits every live slot and the wave stayed regular), [1]: loaded it late (such a wave that left the
// regular path), [2]: loaded it up front with the other planes (no record, or one the launch's filter does not contain).  Behind bit 1 of
// the flag above: a regular wave reads that flag once, as before.
__device__ unsigned long long g_step_category_waves[3];

// PS_Update, UpdateParticleSystemWithDistanceField.fx:29-147, behind its first lookup: the sweep and the bounce / redirect / escape
// arithmetic for a live slot whose life does not run out in this step, given initial_distance (the field at the particle) and, when
// `first_done`, the lookup of the sweep's first iteration (step_distance0) too.  The only statement of them: the interpreter comes
// here from update_with_distance_field, the lean collision kernel with a parked particle (df_common_path made its lookups).
template <int FMT>
ILM_DEV void df_long(float4& pos, float4& vel, float x, float y, float initial_distance, float step_distance0, bool first_done,
                     const IlmParticleSystemUniforms& sys, float dts, const IlmDistanceFieldUniforms& df, const SdfView& sdf, int& samples) {
#pragma clang fp contract(off)
    const float4 zero = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    float new_life = pos.w - (sys.GlobalSettings.w * dts);
    const float collision_distance = sys.CollisionSettings.z;
    const float max_velocity = sys.GlobalSettings.z;
    const f3 old_xyz = xyz(pos);
    const f3 unit_vector = norm3(xyz(vel));
    const f3 velocity = friction_and_maximum(xyz(vel), sys, dts);
    const f3 scaled_velocity = velocity * dts;

    bool collided = false, escaping = false;
    f3 collision_position = mk3(0.0f, 0.0f, 0.0f), new_position = old_xyz;
    float4 new_velocity = zero;

    const bool was_colliding = initial_distance < collision_distance;
    float travel_distance = fmaxf(0.0f, fminf(initial_distance, len3(scaled_velocity)));
    int step_count = ref::kMaxStepCount;
    if (was_colliding)
        step_count = 1;
    else if (travel_distance <= 0.001f)
        step_count = 0;

    for (int i = 0; i < step_count; i++) {
        const f3 test_position = old_xyz + (unit_vector * travel_distance);
        float step_distance = step_distance0;
        if (!(first_done && i == 0)) {
            step_distance = sample_distance_field<(FMT & 1), true, (FMT & 2) != 0, (FMT & 4) != 0>(test_position, df, sdf);
            samples++;
        }
        if (step_distance < collision_distance) {
            collided = true;
            collision_position = test_position;
        }
        escaping = step_distance > initial_distance;
        if (collided && !escaping) {
            collision_position = test_position;
            const float offset = clampf(step_distance + collision_distance, 0.05f, 16.0f);
            travel_distance = fmaxf(0.0f, travel_distance - offset);
        } else
            step_count = 0;
        if (travel_distance <= 0.001f)
            step_count = 0;
    }

    if (collided) {
        const bool bounce = vel.w <= 0.0f;
        const bool redirect = was_colliding && !escaping;
        f3 normal = mk3(0.0f, 0.0f, 0.0f);
        if (bounce || redirect) {
            normal = estimate_normal4<FMT>(collision_position, df, sdf);
            samples += 4;
        }
        const float escape_speed = fminf(max_velocity, sys.CollisionSettings.x);
        if (redirect) {
            normal = normal * mk3(1.0f, 1.0f, 0.0f);  // ESCAPE_MASK
            if (len3(normal) < ref::kNoNormalThreshold) {
                const float a = (x / 67.0f) + (y / 13.0f);
                normal = mk3(sinf(a), cosf(a), 0.0f);
            }
            const f3 nv = (norm3(normal) * escape_speed) * ref::kInitialEscapeSpeed;
            new_velocity = mk4(nv.x, nv.y, nv.z, ref::kBounceDelay);
            new_position = old_xyz + (nv * dts);
        } else if (bounce) {
            const float d2 = 2.0f * dot3(normal, unit_vector);
            f3 bounce_vector = ((normal - unit_vector) * d2) * -1.0f;
            if (len3(bounce_vector) < ref::kNoNormalThreshold)
                bounce_vector = unit_vector * -1.0f;
            else
                bounce_vector = norm3(bounce_vector);
            new_position = collision_position;
            const f3 nv = bounce_vector * fminf(max_velocity, len3(velocity) * sys.CollisionSettings.y);
            new_velocity = mk4(nv.x, nv.y, nv.z, ref::kBounceDelay);
            new_life -= sys.CollisionSettings.w;
        } else {
            const float new_speed = fmaxf(len3(xyz(vel)) * ref::kEscapeSpeedAcceleration, escape_speed);
            const f3 nv = unit_vector * new_speed;
            new_velocity = mk4(nv.x, nv.y, nv.z, 0.0f);
            new_position = old_xyz + (unit_vector * travel_distance);
        }
    } else {
        new_velocity = mk4(velocity.x, velocity.y, velocity.z, fmaxf(vel.w - 1.0f, 0.0f));
        new_position = old_xyz + (unit_vector * travel_distance);
    }
    if (new_life <= 0.0f) {
        new_position = mk3(0.0f, 0.0f, 0.0f);
        new_velocity = zero;
    }
    pos = mk4(new_position.x, new_position.y, new_position.z, new_life);
    vel = new_velocity;
}

// PS_Update with the distance field for a live slot: the life test, the first lookup, then df_long
template <int FMT>
ILM_DEV void update_with_distance_field(float4& pos, float4& vel, float x, float y, const IlmParticleSystemUniforms& sys, float dts,
                                        const IlmDistanceFieldUniforms& df, const SdfView& sdf, int& samples) {
#pragma clang fp contract(off)   // discontinuous collision state machine + life arithmetic: keep IEEE-exact
    if (pos.w - (sys.GlobalSettings.w * dts) <= 0.0f) {
        pos = vel = mk4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float initial_distance = sample_distance_field<(FMT & 1), true, (FMT & 2) != 0, (FMT & 4) != 0>(xyz(pos), df, sdf);
    samples++;
    df_long<FMT>(pos, vel, x, y, initial_distance, 0.0f, false, sys, dts, df, sdf, samples);
}

// ---------------------------------------------------------------------------------------------
// the fused step kernel
// ---------------------------------------------------------------------------------------------
// One wave = one unit of 64 consecutive slots, one lane = one slot: a wave reads / writes 256 contiguous bytes of each component
// plane per instruction.

struct SlotIn {
    float px, py, pz, life, vx, vy, vz, ct, ar, ag, ab, aa;
};

// The 20 planes of one unit through ONE buffer resource (the chunk's allocation) and one lane offset: plane c of the unit is
// `buffer_load/store_dword v, v_lane_offset, s[rsrc], s_plane_offset offen` with s_plane_offset = (first slot + c * stride) * 4 in an
// SGPR -- twenty 32-bit scalar adds per wave.  (The flat form, `global_load_dword v, v_lane_offset, s[base:base+1]`, needs a 64-bit
// base per plane: 2 scalar instructions per plane, computed once for the loads and again for the stores -- 80 of the ~370 scalar
// instructions a wave issued, and the scalar pipe, one instruction per cycle per CU against the four SIMDs' vector issue, is what
// the step's issue phase is bound by: tools/ubench/salu.)
struct UnitPlanes {
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t so[kComponents];
};

ILM_DEV UnitPlanes unit_planes(const float* chunk_base, int64_t stride, int first_slot) {
    UnitPlanes u;
    // raw buffer (stride 0), num_records = the chunk's bytes, DATA_FORMAT = 32 bits (0x00020000, the word gfx9 wants for untyped access)
    u.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)chunk_base, 0, (int)(stride * (kComponents * 4)), 0x00020000);
    const uint32_t s4 = (uint32_t)stride * 4u;
    u.so[0] = (uint32_t)first_slot * 4u;
#pragma unroll
    for (int c = 1; c < kComponents; c++) u.so[c] = u.so[c - 1] + s4;
    return u;
}

// STREAM: the launch's working set is larger than the Infinity Cache (api.hip decides), every plane is touched once per step: loads and
// stores carry the non-temporal hint so they do not evict each other on the way through (tools/ubench/stream: 8.4 M slots 187 -> 170 us;
// on a cache-resident working set the same hint costs 25 %, so small systems keep the default policy).
// Cache policy bits of the plane accesses (buffer intrinsic aux word on gfx94x / gfx950: 1 = sc0, 2 = nt, 16 = sc1).
// Stores of the cache-resident variant carry sc1: they write through the XCD's L2 instead of leaving dirty lines there.  Every L2 is
// private to its XCD, so a kernel's release writes back whatever is still dirty before the next launch of the stream may start --
// up to 8 x 4 MB after a cfg2 step, ~6 us during which nothing runs (per-wave timestamps of an instrumented build: the waves of a
// 16-chunk launch span 17.5 us, back-to-back launches took 24).  The written planes are read next by another launch, on whichever XCD,
// after an invalidate: keeping them in this L2 buys nothing.  tools/step_ab.py: cfg2 without a spawner 20.3 -> 17.5 us per step, with
// 23.4 -> 22.0 (21.0 -> 19.4 / 24.5 -> 23.5 on one stream); sc0, nt, nt + sc1 and non-temporal loads all lose on a resident working set.
constexpr int kLdAux = 0, kStAux = 16, kLdAuxStream = 2, kStAuxStream = 2;
template <bool STREAM>
ILM_DEV float ld_plane(const UnitPlanes& u, int c, unsigned lane4) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(u.rsrc, (int)lane4, (int)u.so[c], STREAM ? kLdAuxStream : kLdAux));
}
template <bool STREAM>
ILM_DEV void st_plane(const UnitPlanes& u, int c, unsigned lane4, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), u.rsrc, (int)lane4, (int)u.so[c], STREAM ? kStAuxStream : kStAux);
}

// The plane groups of a unit (internal.hpp): position and velocity, the attributes, renderColor and renderData
template <bool STREAM>
ILM_DEV float4 load_attributes(const UnitPlanes& u, unsigned lane4) {
    return mk4(ld_plane<STREAM>(u, 8, lane4), ld_plane<STREAM>(u, 9, lane4), ld_plane<STREAM>(u, 10, lane4), ld_plane<STREAM>(u, 11, lane4));
}
template <bool STREAM>
ILM_DEV void store_state(const UnitPlanes& u, unsigned lane4, float4 pos, float4 vel) {
    st_plane<STREAM>(u, 0, lane4, pos.x); st_plane<STREAM>(u, 1, lane4, pos.y); st_plane<STREAM>(u, 2, lane4, pos.z); st_plane<STREAM>(u, 3, lane4, pos.w);
    st_plane<STREAM>(u, 4, lane4, vel.x); st_plane<STREAM>(u, 5, lane4, vel.y); st_plane<STREAM>(u, 6, lane4, vel.z); st_plane<STREAM>(u, 7, lane4, vel.w);
}
template <bool STREAM>
ILM_DEV void store_attributes(const UnitPlanes& u, unsigned lane4, float4 attr) {
    st_plane<STREAM>(u, 8, lane4, attr.x); st_plane<STREAM>(u, 9, lane4, attr.y); st_plane<STREAM>(u, 10, lane4, attr.z); st_plane<STREAM>(u, 11, lane4, attr.w);
}
template <bool STREAM>
ILM_DEV void store_render_color(const UnitPlanes& u, unsigned lane4, float4 rc) {
    st_plane<STREAM>(u, 12, lane4, rc.x); st_plane<STREAM>(u, 13, lane4, rc.y); st_plane<STREAM>(u, 14, lane4, rc.z); st_plane<STREAM>(u, 15, lane4, rc.w);
}
template <bool STREAM>
ILM_DEV void store_render(const UnitPlanes& u, unsigned lane4, float4 rc, float4 rd) {
    store_render_color<STREAM>(u, lane4, rc);
    st_plane<STREAM>(u, 16, lane4, rd.x); st_plane<STREAM>(u, 17, lane4, rd.y); st_plane<STREAM>(u, 18, lane4, rd.z); st_plane<STREAM>(u, 19, lane4, rd.w);
}
// the cleared target of the update pass (the attributes keep what they hold)
template <bool STREAM>
ILM_DEV void store_zero_state_and_render(const UnitPlanes& u, unsigned lane4) {
    const float4 zero = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    store_state<STREAM>(u, lane4, zero, zero);
    store_render<STREAM>(u, lane4, zero, zero);
}

template <bool ATTR, bool STREAM>
ILM_DEV SlotIn load_slot(const UnitPlanes& u, unsigned lane4) {
    SlotIn s;
    s.life = ld_plane<STREAM>(u, 3, lane4);
    s.px = ld_plane<STREAM>(u, 0, lane4); s.py = ld_plane<STREAM>(u, 1, lane4); s.pz = ld_plane<STREAM>(u, 2, lane4);
    s.vx = ld_plane<STREAM>(u, 4, lane4); s.vy = ld_plane<STREAM>(u, 5, lane4); s.vz = ld_plane<STREAM>(u, 6, lane4); s.ct = ld_plane<STREAM>(u, 7, lane4);
    const float4 attr = ATTR ? load_attributes<STREAM>(u, lane4) : mk4(0.0f, 0.0f, 0.0f, 0.0f);
    s.ar = attr.x; s.ag = attr.y; s.ab = attr.z; s.aa = attr.w;
    return s;
}

// The launch descriptor lives in the kernarg segment (constant address space) and the per-unit body reads
// every parameter through a pointer to it (s_load from a uniform address).
typedef const StepLaunch __attribute__((address_space(4))) CStepLaunch;

// DF: the update pass is UpdateWithDistanceField (pulls in the SDF sampler); SPAWN: spawn records present.
// Both are compile-time so the common no-field / no-spawn step does not pay their registers.
template <int FMT, bool DF, bool SPAWN, bool EXT, bool STREAM>
ILM_DEV bool process_unit(CStepLaunch* ap, const UnitPlanes& up, int chunk, int i, unsigned lane, int seg, SlotIn cur, const NoiseDeltas& noise) {
    const StepLaunch& a = *(const StepLaunch*)ap;
    const IlmStepDesc& d = a.desc;
    const int64_t S = a.stride;
    const unsigned lane4 = lane * 4u;
    const int mode = d.UpdateMode;
    const bool need_attr = (mode == ILM_UPDATE_POSITIONS) || (mode == ILM_UPDATE_WITH_DISTANCE_FIELD);
    // Noise has no life check (Noise.fx:40): dead slots go through it.  That only matters when its result survives --
    // no update pass follows (single-pass ilm_noise), or the op can bring a dead slot back to life (StepDerived).
    const uint32_t noise_ops = EXT ? ((1u << ILM_OP_NOISE) | (1u << ILM_OP_SPATIAL_NOISE)) : (1u << ILM_OP_NOISE);
    const bool has_noise = ((a.op_mask & noise_ops) != 0u) && ((mode == ILM_UPDATE_NONE) || (a.derived.noise_may_revive != 0));
    const float4 zero = mk4(0.0f, 0.0f, 0.0f, 0.0f);

    bool spawn_here = false;
    if constexpr (SPAWN) {
        for (int s = 0; s < d.SpawnCount; s++) {
            const IlmSpawnRecord& r = d.Spawns[s];
            if (r.ChunkIndex == chunk && (float)i >= r.Params.ChunkSizeAndIndices[1] && (float)i <= r.Params.ChunkSizeAndIndices[2])
                spawn_here = true;
        }
    }
    bool live_after = false;
    int sdf_samples = 0;
    // Stride padding (chunk sizes whose square is not a multiple of 1024: 10, 16, 48 ...): not a slot of the chunk.  Noise has no life
    // check, so without this a padding lane could be given a life, be updated and be counted (CountLiveParticles.fx counts ChunkSize^2 pixels).
    if (i >= a.slots)
        return false;
    if (mode == ILM_UPDATE_ERASE) {
        // PS_Erase, UpdateParticleSystem.fx:40-49
        store_zero_state_and_render<STREAM>(up, lane4);
    } else if ((cur.life <= 0.0f) && !spawn_here && !has_noise) {     // `<= 0` as the shaders test it: a NaN life is not dead
        // dead and nothing writes it: the update pass leaves the cleared target
        // (UpdateHandler._BeforeDraw clears, ParticleTransform.cs:164-165; readStateOrDiscard discards)
        if (mode != ILM_UPDATE_NONE)
            store_zero_state_and_render<STREAM>(up, lane4);
        else {
            live_after = cur.life > 0.0f;   // untouched slots keep their liveness when no update pass ran
        }
    } else {
        float4 pos = mk4(cur.px, cur.py, cur.pz, cur.life);
        float4 vel = mk4(cur.vx, cur.vy, cur.vz, cur.ct);
        float4 attr = mk4(cur.ar, cur.ag, cur.ab, cur.aa);
        // slot (x, y): the unit's first slot is divided on the scalar unit, lanes only fold the row wrap
        const int cs = a.chunk_size;
        const int row0 = (a.derived.cs_shift >= 0) ? ((seg * 64) >> a.derived.cs_shift) : __builtin_amdgcn_readfirstlane((seg * 64) / cs);
        int sy = row0, sx = (seg * 64 - row0 * cs) + (int)lane;
        while (sx >= cs) { sx -= cs; sy++; }
        const float fx = (float)sx, fy = (float)sy;
        bool spawned = false;

        if constexpr (SPAWN) {
            if (spawn_here) {
                for (int s = 0; s < d.SpawnCount; s++) {
                    if (d.Spawns[s].ChunkIndex == chunk) {
                        bool wrote;
                        if (EXT && d.Spawns[s].Kind == ILM_SPAWN_POSITION_BUFFER)
                            wrote = spawn_slot_position_buffer(pos, vel, attr, fx, fy, a.rnd, a.rw, a.rh, a.derived.inv_rw, a.derived.inv_rh,
                                                               d.Spawns[s].Params, a.spawn_positions[s], a.spawn_position_count[s]);
                        else if (EXT && d.Spawns[s].Kind == ILM_SPAWN_FEEDBACK)
                            wrote = spawn_slot_feedback(pos, vel, attr, fx, fy, a.rnd, a.rw, a.rh, a.derived.inv_rw, a.derived.inv_rh,
                                                        d.Spawns[s].Params, d.Spawns[s].Feedback, a.source_base[s], S, cs);
                        else if (EXT && d.Spawns[s].Kind == ILM_SPAWN_PATTERN)
                            wrote = spawn_slot_pattern(pos, vel, attr, fx, fy, a.rnd, a.rw, a.rh, a.derived.inv_rw, a.derived.inv_rh,
                                                       d.Spawns[s].Params, d.Spawns[s].Pattern, a.spawn_pattern[s], a.pattern_w[s],
                                                       a.pattern_h[s], a.pattern_levels[s]);
                        else
                            wrote = spawn_slot(pos, vel, attr, fx, fy, a.rnd, a.rw, a.rh, a.derived.inv_rw, a.derived.inv_rh, d.Spawns[s].Params);
                        if (wrote)
                            spawned = true;
                    }
                }
            }
        }

        for (int o = 0; o < d.OpCount; o++) {
            const IlmTransformOp& op = d.Ops[o];
            if (op.Type == ILM_OP_GRAVITY)
                apply_gravity(pos, vel, d.System, op.u.Gravity, a.derived.op[o]);
            else if (op.Type == ILM_OP_NOISE)
                apply_noise(pos, vel, fx, fy, a.rnd, a.rw, a.rh, d.System, op.u.Noise, a.derived.inv_rw, a.derived.inv_rh, a.derived.op[o],
                            (o == a.derived.noise.op) ? noise : NoiseDeltas{ false, zero, zero });
            else if (op.Type == ILM_OP_FMA)
                apply_fma(pos, vel, d.System, op.u.FMA, a.derived.op[o]);
            else if (EXT && op.Type == ILM_OP_MATRIX_MULTIPLY)
                apply_matrix_multiply(pos, vel, d.System, op.u.MatrixMultiply);
            else if (EXT && op.Type == ILM_OP_SPATIAL_NOISE)
                apply_spatial_noise(pos, vel, a.rnd_lp, a.rw, a.rh, d.System, op.u.SpatialNoise, a.derived);
        }

        float4 rc = zero, rd = zero;
        if (need_attr) {
            if (pos.w <= 0.0f) {
                pos = vel = zero;  // readStateOrDiscard: discard => cleared target
            } else {
                if constexpr (DF)
                    update_with_distance_field<FMT>(pos, vel, fx, fy, d.System, a.derived.dt_s, d.DistanceField, a.sdf, sdf_samples);
                else
                    update_positions(pos, vel, d.System, a.derived.dt_s);
                render_data(fx, fy, pos, vel, attr, d.System, d.Update, a.derived.bezier_codes, a.derived.update_bits, a.ramp, a.ramp_w, a.ramp_h, rc, rd);
            }
        }
        store_state<STREAM>(up, lane4, pos, vel);
        if (spawned)
            store_attributes<STREAM>(up, lane4, attr);
        if (need_attr)
            store_render<STREAM>(up, lane4, rc, rd);
        live_after = pos.w > 0.0f;
    }
    if constexpr (DF) {
        // diagnostic count (one atomic per lane: only ever on while bench.py takes the collision row's sample count)
        if ((__builtin_amdgcn_readfirstlane(g_step_count_sdf_samples) != 0) && (sdf_samples != 0))
            atomicAdd(&g_step_sdf_samples, (unsigned long long)sdf_samples);
    }

    return live_after;
}

// CountLiveParticles.fx for a block of the step kernels: LDS sum over the block's waves, ONE 64-bit atomic per block on a bucket
// counter of its chunk (live particles in the low word, a ticket in the high word); the block that draws a bucket's last ticket
// carries the bucket's sum to the chunk's counter the same way, and the one that completes the chunk stores the total, tagged with
// the step's sequence number, straight into the host's table.  (Per-wave atomics on one address serialise at ~11 ns each: 1024 of
// them per chunk made the step 7x slower; one per block on ONE address per chunk still queued 4096 deep on 1024^2 chunks.)  The
// units of a block always belong to one chunk.
// `zero_block`: this block zeroes the other counter region (one block per launch; per item in step_batch_kernel).
ILM_DEV void publish_block_count_at(bool zero_block, uint32_t* wave_live, uint32_t n_live, unsigned lane, int wave, bool block_in_range, int chunk, int block_in_chunk,
                                    int blocks_per_chunk, int buckets, unsigned long long* live_counts, unsigned long long* zero_counts, int zero_n,
                                    unsigned long long* host_counts, uint32_t seq) {
    if (zero_block)
        for (int i = (int)threadIdx.x; i < zero_n; i += kStepThreads) zero_counts[i * kCountStride] = 0ull;
    if (lane == 0) wave_live[wave] = n_live;
    __syncthreads();
    if (threadIdx.x == 0 && block_in_range) {
        uint32_t block_live = 0;
#pragma unroll
        for (int w = 0; w < kStepThreads / 64; w++) block_live += wave_live[w];
        unsigned long long* lines = live_counts + (size_t)chunk * (kCountLines * kCountStride);
        const int bucket = block_in_chunk & (buckets - 1);
        const unsigned long long old = atomicAdd(&lines[(1 + bucket) * kCountStride], (1ull << 32) | (unsigned long long)block_live);
        if ((int)(old >> 32) + 1 == blocks_per_chunk / buckets) {
            const unsigned long long sum = (old & 0xFFFFFFFFull) + (unsigned long long)block_live;
            const unsigned long long old2 = atomicAdd(&lines[0], (1ull << 32) | sum);
            if ((int)(old2 >> 32) + 1 == buckets) {
                const unsigned long long total = (old2 & 0xFFFFFFFFull) + sum;
                __hip_atomic_store(&host_counts[chunk], ((unsigned long long)seq << 32) | (total & 0xFFFFFFFFull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

ILM_DEV void publish_block_count(uint32_t* wave_live, uint32_t n_live, unsigned lane, int wave, bool block_in_range, int chunk, int block_in_chunk,
                                 int blocks_per_chunk, int buckets, unsigned long long* live_counts, unsigned long long* zero_counts, int zero_n,
                                 unsigned long long* host_counts, uint32_t seq) {
    publish_block_count_at(blockIdx.x == 0, wave_live, n_live, lane, wave, block_in_range, chunk, block_in_chunk, blocks_per_chunk, buckets, live_counts,
                           zero_counts, zero_n, host_counts, seq);
}

// The launch descriptor is written by the host into the kernarg ring just before the launch, so the first wave of every scalar cache
// misses on each of its 64-byte lines all the way to memory -- and the step reads them one dependent phase after another (decode,
// planes, noise tables, each transform, the update pass): a chain of ~20 serial misses at the head of every launch.  One load per
// line, all in flight at once, turns the chain into a single miss; for every later wave they are ~60 cache hits the scalar pipe has
// room for (tools/step_ab.py with 200 extra scalar instructions per wave: no change in step time).  Measured (r02): a one-chunk launch
// 7.7 -> 6.0 us back to back (10.8 -> 8.3 us when it spawns), cfg2 without a spawner 24.0 -> 21.4 us per step.
constexpr int kTouchBlocks = 2048 / (kStepThreads / 64);      // the launch's first 2 048 waves
// The chunk table is read through the constant address space in both kernels: see step_lean_kernel.
typedef float* const __attribute__((address_space(4))) CBase;
#define ILM_T1(o) "s_load_dword %0, %1, " #o "\n"
#define ILM_T4(o) ILM_T1(o) ILM_T1(o + 0x40) ILM_T1(o + 0x80) ILM_T1(o + 0xc0)
#define ILM_T16(o) ILM_T4(o) ILM_T4(o + 0x100) ILM_T4(o + 0x200) ILM_T4(o + 0x300)
ILM_DEV void touch_kernarg_lines_lean() {       // LeanStep: 51 lines
    const auto kp = __builtin_amdgcn_kernarg_segment_ptr();
    uint32_t sink;
    asm volatile(ILM_T16(0x0) ILM_T16(0x400) ILM_T16(0x800) ILM_T1(0xc00) ILM_T1(0xc40) ILM_T1(0xc80) "s_waitcnt lgkmcnt(0)"
                 : "=&s"(sink) : "s"(kp));
}
ILM_DEV void touch_kernarg_lines_step() {       // StepLaunch: 63 lines
    const auto kp = __builtin_amdgcn_kernarg_segment_ptr();
    uint32_t sink;
    asm volatile(ILM_T16(0x0) ILM_T16(0x400) ILM_T16(0x800) ILM_T4(0xc00) ILM_T4(0xd00) ILM_T4(0xe00) ILM_T1(0xf00) ILM_T1(0xf40) ILM_T1(0xf80)
                 "s_waitcnt lgkmcnt(0)" : "=&s"(sink) : "s"(kp));
}
static_assert(sizeof(StepLaunch) >= 0xf84 && sizeof(StepLaunch) <= 0xfc0, "touch_kernarg_lines_step reads one dword of each 64-byte line of StepLaunch");

// One wave = one unit of 64 consecutive slots; the hardware dispatcher balances the waves.  (A persistent,
// software-pipelined variant of this kernel measured 12-25 % slower: the body is a long dependent chain --
// state loads, scalar parameter fetches, randomness gathers -- whose latency is hidden by wave occupancy,
// not by prefetching; see DESIGN.md.)  MINW = minimum waves per SIMD requested from the register allocator.
template <int FMT, bool DF, bool SPAWN, int MINW, bool EXT = false, bool STREAM = false>
__global__ __launch_bounds__(kStepThreads, MINW) void step_kernel(const StepLaunch a) {
    __shared__ uint32_t wave_live[kStepThreads / 64];
    CStepLaunch* ap = (CStepLaunch*)__builtin_amdgcn_kernarg_segment_ptr();
    if (blockIdx.x < kTouchBlocks) touch_kernarg_lines_step();
    // the wave index is uniform by construction; saying so keeps the unit / chunk / base-pointer arithmetic on the
    // scalar unit and lets every plane access use the SGPR-base + 32-bit lane-offset addressing form
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    // Blocks are rotated so that block 0 holds the first unit of the first spawn range: a spawning wave is a long
    // dependent chain (randomness gathers, sin/cos/acos), so it has to start first to finish under the cover of
    // the streaming waves instead of forming the tail of the launch.  unit_rotate is a multiple of the units per block; those
    // divide units_per_chunk (a multiple of 16), so a block lies in one chunk.
    int v = (int)blockIdx.x * (kStepThreads / 64) + a.unit_rotate;          // first unit of the block
    const int total = a.unit_end - a.unit_begin;
    if (v >= a.total_padded) v -= a.total_padded;
    const int u = a.unit_begin + v + wave;
    uint32_t n_live = 0;
    if (v + wave < total) {
        // (a scalar integer division costs ~35 instructions per wave)
        const int chunk_rel = (a.upc_shift >= 0) ? (u >> a.upc_shift) : (u / a.units_per_chunk);
        const int seg = u - chunk_rel * a.units_per_chunk;
        const int chunk = a.first_chunk + chunk_rel;
        // never-written tail of a spawn-target chunk: all planes are zero and stay zero (scalar compares, uniform branch)
        bool untouched = false;
        for (int k = 0; k < a.partial_count; k++)
            untouched = untouched || ((a.partial_chunk[k] == chunk) && (seg >= a.partial_units[k]));
        if (!untouched) {
            const UnitPlanes up = unit_planes(((CBase*)a.chunk_bases)[chunk], a.stride, seg * 64);
            // (a wave that loads K > 1 units up front and processes them in turn loses more occupancy to the extra registers than the
            // loads in flight return: cfg2 26.1 / 30.5 / 36.5 us per step for K = 1 / 2 / 4, docs/experiments.md)
            const SlotIn cur = load_slot<true, STREAM>(up, lane * 4u);
            NoiseDeltas noise;
            noise.valid = false;
            if (a.derived.noise.op >= 0) {
                // first slot of the unit -> (x0, y): scalar; the unit lies in one row (chunk size a multiple of 64)
                const int first = seg * 64;
                const int row = (a.derived.cs_shift >= 0) ? (first >> a.derived.cs_shift) : (first / a.chunk_size);
                noise = noise_prepare(((const StepLaunch*)ap)->derived.noise, reinterpret_cast<const IlmFloat4*>(&((const StepLaunch*)ap)->desc.Spawns[0]), first - row * a.chunk_size, row);
            }
            const bool live_after = process_unit<FMT, DF, SPAWN, EXT, STREAM>(ap, up, chunk, seg * 64 + (int)lane, lane, seg, cur, noise);
            n_live = (uint32_t)__popcll(__ballot(live_after));
        }
    }
    if (a.desc.Flags & ILM_STEP_COUNT_LIVE) {
        const int first_unit = a.unit_begin + v;
        const int chunk_rel = (a.upc_shift >= 0) ? (first_unit >> a.upc_shift) : (first_unit / a.units_per_chunk);
        constexpr int kUnitsPerBlock = kStepThreads / 64;
        publish_block_count(wave_live, n_live, lane, wave, v < total, a.first_chunk + chunk_rel, (first_unit - chunk_rel * a.units_per_chunk) / kUnitsPerBlock,
                            a.units_per_chunk / kUnitsPerBlock, a.count_buckets, a.live_counts, a.zero_counts, a.zero_n, a.host_counts, a.count_seq);
    }
}

// The interpreter over MANY launches' worth of work in one grid (ilm_engine_step_batch): the StepLaunch records of the items lie in a
// device table, and a block finds its item with one scalar load of item_of_block[blockIdx.x].  From there it is step_kernel's body with
// the item's LOCAL block index where step_kernel has blockIdx.x -- the rotation, the range test, the counters' buckets and the zeroing
// of the item's other counter region all come from the item, none from the grid -- so an item's planes and counts get the bits its own
// launch of step_kernel would have given them.  The table and the records are read-only here.  No STREAM variant: a range that large
// is launched on its own.
typedef const StepBatchItem __attribute__((address_space(4))) CStepBatchItem;
typedef const int32_t __attribute__((address_space(4))) CInt32;
ILM_DEV void touch_record_lines_step(CStepLaunch* ap) {     // touch_kernarg_lines_step for a record in the table: its lines are as cold
    uint32_t sink;
    asm volatile(ILM_T16(0x0) ILM_T16(0x400) ILM_T16(0x800) ILM_T4(0xc00) ILM_T4(0xd00) ILM_T4(0xe00) ILM_T1(0xf00) ILM_T1(0xf40) ILM_T1(0xf80)
                 "s_waitcnt lgkmcnt(0)" : "=&s"(sink) : "s"(ap));
}
template <int FMT, bool DF, bool SPAWN, int MINW, bool EXT = false>
__global__ __launch_bounds__(kStepThreads, MINW) void step_batch_kernel(const StepBatchItem* table, const int32_t* item_of_block) {
    __shared__ uint32_t wave_live[kStepThreads / 64];
    const int item = ((CInt32*)item_of_block)[blockIdx.x];
    CStepBatchItem* ip = (CStepBatchItem*)table + item;
    CStepLaunch* ap = (CStepLaunch*)ip;
    const StepLaunch& a = *(const StepLaunch*)ap;
    const int block = (int)blockIdx.x - ip->first_block;     // the block's index in its item
    if (block < kTouchBlocks) touch_record_lines_step(ap);
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    int v = block * (kStepThreads / 64) + a.unit_rotate;      // first unit of the block (rotation: see step_kernel)
    const int total = a.unit_end - a.unit_begin;
    if (v >= a.total_padded) v -= a.total_padded;
    const int u = a.unit_begin + v + wave;
    uint32_t n_live = 0;
    if (v + wave < total) {
        const int chunk_rel = (a.upc_shift >= 0) ? (u >> a.upc_shift) : (u / a.units_per_chunk);
        const int seg = u - chunk_rel * a.units_per_chunk;
        const int chunk = a.first_chunk + chunk_rel;
        bool untouched = false;
        for (int k = 0; k < a.partial_count; k++)
            untouched = untouched || ((a.partial_chunk[k] == chunk) && (seg >= a.partial_units[k]));
        if (!untouched) {
            const UnitPlanes up = unit_planes(((CBase*)a.chunk_bases)[chunk], a.stride, seg * 64);
            const SlotIn cur = load_slot<true, false>(up, lane * 4u);
            NoiseDeltas noise;
            noise.valid = false;
            if (a.derived.noise.op >= 0) {
                const int first = seg * 64;
                const int row = (a.derived.cs_shift >= 0) ? (first >> a.derived.cs_shift) : (first / a.chunk_size);
                noise = noise_prepare(a.derived.noise, reinterpret_cast<const IlmFloat4*>(&a.desc.Spawns[0]), first - row * a.chunk_size, row);
            }
            const bool live_after = process_unit<FMT, DF, SPAWN, EXT, false>(ap, up, chunk, seg * 64 + (int)lane, lane, seg, cur, noise);
            n_live = (uint32_t)__popcll(__ballot(live_after));
        }
    }
    if (a.desc.Flags & ILM_STEP_COUNT_LIVE) {
        const int first_unit = a.unit_begin + v;
        const int chunk_rel = (a.upc_shift >= 0) ? (first_unit >> a.upc_shift) : (first_unit / a.units_per_chunk);
        constexpr int kUnitsPerBlock = kStepThreads / 64;
        publish_block_count_at(block == 0, wave_live, n_live, lane, wave, v < total, a.first_chunk + chunk_rel,
                               (first_unit - chunk_rel * a.units_per_chunk) / kUnitsPerBlock, a.units_per_chunk / kUnitsPerBlock, a.count_buckets,
                               a.live_counts, a.zero_counts, a.zero_n, a.host_counts, a.count_seq);
    }
}

// ---------------------------------------------------------------------------------------------
// the lean step kernel
// ---------------------------------------------------------------------------------------------
// step_kernel above interprets an arbitrary IlmStepDesc: per wave ~370 scalar-ALU instructions, ~70 scalar loads and ~60 branches next
// to ~365 vector instructions.  The scalar pipe issues one instruction per cycle per CU against the four SIMDs' vector issue
// (tools/ubench/salu: ~550 G/s against ~950 G/s), and every dependent scalar load the interpreter waits for is latency in the life of
// a wave whose whole launch is only two to three wave generations long -- so on a cache-resident system (cfg2) the step's time
// follows the scalar work, not the bytes.  step_lean_kernel runs the common shape of a step -- power-of-two chunk size >= 64,
// UpdatePositions, Gravity / Noise (no area, wave-uniform deltas available) / FMA (no area) in any order, inline spawners, no life
// ramp, no Noise that can revive a slot -- from a pre-digested descriptor (LeanStep, built by launch_step from the same StepLaunch):
// every uniform decision arrives as an integer, the attractors as one 32-byte record each, the spawn ranges as unit ranges.  The
// per-slot arithmetic is the interpreter's own (same functions or the same operations in the same order): ILM_STEP_LEAN=0 runs the
// interpreter instead and tests/test_properties_gpu.py requires the two to agree bit for bit.
struct LeanAttractor { float x, y, z, radius, strength, _p0, _p1, _p2; };
constexpr int kLeanMaxAttractors = 8;
struct LeanGravity {
    int32_t count; uint32_t types;   // 2 bits per attractor: 0 physical (ars.z < 0.5), 1 linear, 2 squared (Gravity.fx:36-52)
    float max_accel, _pad0;
    float cat_lo, cat_hi, _pad1, _pad2;
    LeanAttractor a[kLeanMaxAttractors];
};
union LeanOp {
    LeanGravity gravity;
    IlmNoiseParams noise;
    IlmFMAParams fma;
};
struct LeanStep {
    // decode
    float* const* chunk_bases;
    unsigned long long* live_counts; unsigned long long* zero_counts; unsigned long long* host_counts;
    int64_t stride;
    int32_t upc_shift, unit_rotate, total_padded, total_units;
    int32_t first_chunk, cs_shift, zero_n; uint32_t flags;
    uint32_t count_seq; int32_t count_buckets;
    float regular_cat_lo, regular_cat_hi;       // the intersection of the transforms' category filters (NaN lo: no category passes); step_lean_clamp_kernel
    int32_t partial_chunk[kMaxPartialChunks], partial_units[kMaxPartialChunks];     // unused entries: chunk -1
    int32_t partial_count, op_count, spawn_count; uint32_t elide;      // elide: kElideDerived / kElideColor (step_lean_kernel)
    int32_t op_type[ILM_MAX_OPS];
    int32_t spawn_chunk[ILM_MAX_SPAWNS], spawn_unit_lo[ILM_MAX_SPAWNS], spawn_unit_hi[ILM_MAX_SPAWNS];   // segments of the target chunk a record touches
    int32_t cat_stride, _pad1;       // cat_stride: see cat_bounds
    // update pass
    float dt_s; uint32_t bezier_codes, update_bits; int32_t noise_op;
    IlmParticleSystemUniforms sys;
    IlmUpdateParams update;
    // transforms
    StepDerived::Op dop[ILM_MAX_OPS];
    LeanOp op[ILM_MAX_OPS];
    StepDerived::NoiseFast noise;
    // spawners (inline kind only) -- or, in a launch without them, the 5 x 5 noise tables (kNoiseBigClasses)
    const float4* rnd; int32_t rw, rh; float inv_rw, inv_rh;
    // step_lean_clamp_kernel: the category records of the system's chunks (api.hip, System::cat_current), cat_stride = kCategoryRecordStride
    // x 4 bytes per chunk, {lo, hi} first -- or, for a launch without records, g_no_category_record with a stride of 0: a NaN record for
    // every chunk, which no filter contains (every wave loads the category plane up front)
    const float* cat_bounds;
    union {
        IlmSpawnRecord spawns[ILM_MAX_SPAWNS];
        IlmFloat4 noise_big[2 * kNoiseBigClasses * kNoiseBigClasses];
    };
};
static_assert(sizeof(LeanStep) <= 4096, "LeanStep travels in the kernarg segment (4 KB)");

// PS_Gravity with the attractor records and type codes of LeanGravity: apply_gravity's terms (gravity_term), added in its order
// FILTER = false: as for apply_fma.
template <bool FILTER = true>
ILM_DEV void apply_gravity_lean(float4& pos, float4& vel, const LeanGravity& g, float dt_ms, float mv) {
    if (FILTER && ((pos.w <= 0.0f) || !((vel.w >= g.cat_lo) && (vel.w <= g.cat_hi))))
        return;
    f3 acceleration = mk3(0.0f, 0.0f, 0.0f);
    const uint32_t types = g.types;
    int i = 0;
#ifndef ILM_GRAVITY_EXACT
    // Four attractors at a time while none of the four is of the physical type (the one with the IEEE division): their records come
    // in together, every decision is a select on a uniform mask, so the four dependent chains (subtract, dot, rsq, rcp, ...) sit in
    // one basic block and the scheduler interleaves them.  The same operations per attractor, the terms added in index order: the
    // same bits as the loop below.  (A wave alone on its SIMD spent 1.24 us of its 3.4 in the transforms, one attractor after the
    // other behind a scalar load each -- and that latency is what the head and the tail of every launch consist of.)
    for (; i + 4 <= g.count && ((((types >> (2 * i)) | (types >> (2 * i + 1))) & 0x55u) == 0x55u); i += 4) {
        f3 term[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const LeanAttractor A = g.a[i + k];
            const bool squared = ((types >> (2 * (i + k))) & 2u) != 0u;
            term[k] = gravity_term(mk3(A.x, A.y, A.z) - xyz(pos), squared ? 2u : 1u, A.radius, A.strength, dt_ms);
        }
        acceleration = (((acceleration + term[0]) + term[1]) + term[2]) + term[3];
    }
#endif
    for (; i < g.count; i++) {
        const LeanAttractor A = g.a[i];
        acceleration = acceleration + gravity_term(mk3(A.x, A.y, A.z) - xyz(pos), (types >> (2 * i)) & 3u, A.radius, A.strength, dt_ms);
    }
    gravity_finish(vel, acceleration, g.max_accel, mv);
}

typedef const LeanStep __attribute__((address_space(4))) CLeanStep;
static_assert(sizeof(LeanStep) >= 0xc84 && sizeof(LeanStep) <= 0xcc0, "touch_kernarg_lines_lean reads one dword of each 64-byte line of LeanStep");

// Slot (x, y) of a lean unit's lanes, and the unit's first slot, row and first column.  The unit lies in one row (chunk size a
// multiple of 64).
ILM_DEV void lean_unit_slot(const LeanStep& a, int seg, unsigned lane, int& first, int& row, int& x0, float& fx, float& fy) {
    first = seg * 64;
    row = first >> a.cs_shift;
    x0 = first - (row << a.cs_shift);
    fx = (float)(x0 + (int)lane); fy = (float)row;
}

// ---- store elision (internal.hpp, kElideDerived) -------------------------------------------------------------------------------
// A wave stores a plane only when it has to: writing the bits memory already holds changes nothing, and at cfg4's size every plane
// access is HBM traffic.  When it stores, it stores all 64 lanes (an unchanged lane rewrites its own bits; a lane-masked store saves
// no burst).
ILM_DEV bool same_bits(float a, float b) { return __builtin_bit_cast(uint32_t, a) == __builtin_bit_cast(uint32_t, b); }
// Only the STREAM variant elides.  The cache-resident one keeps every store: its planes live in the Infinity Cache from one step to the
// next, its time follows the issue of its instructions rather than its bytes (see step_lean_kernel), and the compares would be added work.
template <bool STREAM>
ILM_DEV void st_plane_changed(const UnitPlanes& u, int c, unsigned lane4, float v, float loaded) {
    if (!STREAM || __ballot(!same_bits(v, loaded)) != 0ull) st_plane<STREAM>(u, c, lane4, v);
}
// A curve of the update pass gives the same value for two inputs whose t (tForScaledBezier) is the same bits and no NaN: the rest of
// evaluateBezier is a function of t and of the curve (part of the render key).  A constant curve reads no t at all.
ILM_DEV bool same_curve_t(const IlmFloat4& rc, float v0, float v1, uint32_t code) {
    if ((code & 3u) == 0u) return true;
    const float t1 = t_for_coded_bezier(rc, v1, code);
    return same_bits(t_for_coded_bezier(rc, v0, code), t1) && (t1 == t1);
}
// The render planes of a render-current chunk (every chunk of the launch; api.hip, System::render_gen) hold what render_data gives for the
// state this wave loaded.  Per lane, a component keeps its bits when
//   - the slot is dead before and after the step: all eight components are 0 and stay 0; or, for a slot alive before and after,
//   - its inputs have the same bits (rd.z: the velocity; rd.w: the category, no NaN), or
//   - a value that decides it is the same bits for the loaded and the new state and no NaN: renderColor by the two colour curves' t, with
//     the attributes not spawned over and colour curves that cannot give a NaN factor (kElideColor, host-checked); rd.x by the size
//     curves' t, rd.x itself no NaN; rd.y, when getVelocityRotation() == 0, by itself (recomputed for the loaded state, no NaN).
// Anything else -- liveness changed, rotation from velocity, a NaN -- stores.  A plane is stored when any lane of the wave needs it;
// the attributes are loaded only by a wave that stores renderColor.  (No life ramp here: build_lean_step.)
template <bool SPAWN, bool STREAM>
ILM_DEV void store_changed_render_planes(const LeanStep& a, const UnitPlanes& up, unsigned lane4, float fx, float fy, const SlotIn& cur,
                                         float4 pos, float4 vel, float4 attr, bool spawned) {
    const float4 zero = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    const IlmUpdateParams& p = a.update;
    const uint32_t codes = a.bezier_codes;
    const bool live0 = !(cur.life <= 0.0f), live1 = !(pos.w <= 0.0f);
    const bool dead = !live0 && !live1, both = live0 && live1;
    float4 rc, rd;
    render_data(fx, fy, pos, vel, zero, a.sys, p, codes, a.update_bits, nullptr, 0, 0, rc, rd);     // (rc: not used)
    // the speed the velocity curves read, for the loaded state, only where a velocity curve is not constant
    float speed0 = 0.0f, speed1 = 0.0f;
    if ((codes & 0x03000300u) != 0u) {
        speed0 = fmaxf(len3_fast(mk3(cur.vx, cur.vy, cur.vz)), 0.0001f);
        speed1 = fmaxf(len3_fast(xyz(vel)), 0.0001f);
    }
    const bool same_v = same_bits(cur.vx, vel.x) && same_bits(cur.vy, vel.y) && same_bits(cur.vz, vel.z);
    const bool rc_same = dead || (both && !spawned && ((a.elide & kElideColor) != 0u) && same_curve_t(p.ColorFromLife.RangeAndCount, cur.life, pos.w, codes & 0xFFu) &&
                                  same_curve_t(p.ColorFromVelocity.RangeAndCount, speed0, speed1, (codes >> 8) & 0xFFu));
    const bool rdx_same = dead || (both && same_curve_t(p.SizeFromLife.RangeAndCount, cur.life, pos.w, (codes >> 16) & 0xFFu) &&
                                   same_curve_t(p.SizeFromVelocity.RangeAndCount, speed0, speed1, codes >> 24) && (rd.x == rd.x));
    bool rdy_same = dead;
    if (a.update_bits & 2u) {
        const float y0 = render_rotation(rotation_unscaled(cur.vx, cur.vy), cur.life, render_index(fx, fy), a.sys, p);
        rdy_same = rdy_same || (both && same_bits(y0, rd.y) && (rd.y == rd.y));
    }
    const bool rdz_same = dead || (both && same_v);
    const bool rdw_same = dead || (both && same_bits(cur.ct, vel.w) && (vel.w == vel.w));
    if (__ballot(!rc_same) != 0ull) {
        const float4 stored = load_attributes<STREAM>(up, lane4);
        if (!SPAWN || !spawned) attr = stored;
        float4 rd_unused;
        render_data(fx, fy, pos, vel, attr, a.sys, p, codes, a.update_bits, nullptr, 0, 0, rc, rd_unused);
        store_render_color<STREAM>(up, lane4, rc);
    }
    if (__ballot(!rdx_same) != 0ull) st_plane<STREAM>(up, 16, lane4, rd.x);
    if (__ballot(!rdy_same) != 0ull) st_plane<STREAM>(up, 17, lane4, rd.y);
    if (__ballot(!rdz_same) != 0ull) st_plane<STREAM>(up, 18, lane4, rd.z);
    if (__ballot(!rdw_same) != 0ull) st_plane<STREAM>(up, 19, lane4, rd.w);
}

// The curve classes of the streaming lean step (launch_lean_step selects, ilm_debug_last_step_kernel reports): compile-time
// instantiations of step_lean_block (step_lean_kernel<..> / step_lean_clamp_kernel).  kCurvesClamp: every
// curve of the update pass is constant or has the clamp range and no shaping (bezier_codes & ~kClampCodes == 0), the velocity rotation
// is zero and there is no life ramp (update_bits == 2), the launch elides (kElideDerived) and has no spawner (the spawning kernel's
// registers are the spawn path's: a class of it would gain little).  The instantiation holds no fmodf, sinf or atan2f code; which curves
// are constant stays a scalar test.
constexpr int kCurvesGeneral = 0, kCurvesClamp = 1;
constexpr uint32_t kClampCodes = 0x13131313u;      // per curve: the count class (bits 0-1) and the sign of the inverse divisor (bit 4)

// One curve's part in the elision proof and in the value: t for the loaded and the new state, formed once.
struct CurveT { float t1; bool same; };
ILM_DEV CurveT clamp_curve_t(const IlmFloat4& rc, float v0, float v1, uint32_t code) {
    CurveT c = { 0.0f, true };      // a constant curve reads no t
    if ((code & 3u) != 0u) {
        c.t1 = t_for_clamp_bezier(rc, v1, code);
        c.same = same_bits(t_for_clamp_bezier(rc, v0, code), c.t1) && (c.t1 == c.t1);
    }
    return c;
}
// store_changed_render_planes for kCurvesClamp: the same stores of the same bits (the rules above, render_data's operations on the same
// operands), with each t and the new state's speed formed once and shared by the proof and the value, and the dead lanes selected at
// the end instead of branched around.  (No spawner: the attributes are the stored ones.)
ILM_DEV void store_changed_render_planes_clamp(const LeanStep& a, const UnitPlanes& up, unsigned lane4, float fx, float fy, const SlotIn& cur,
                                               float4 pos, float4 vel) {
    const IlmUpdateParams& p = a.update;
    const uint32_t codes = a.bezier_codes & kClampCodes;
    const uint32_t c_cl = codes & 0xFFu, c_cv = (codes >> 8) & 0xFFu, c_sl = (codes >> 16) & 0xFFu, c_sv = codes >> 24;
    const bool live0 = !(cur.life <= 0.0f), live1 = !(pos.w <= 0.0f);
    const bool dead = !live0 && !live1, both = live0 && live1;
    const float index = render_index(fx, fy);
    const float speed1 = fmaxf(len3_fast(xyz(vel)), 0.0001f);
    float speed0 = 0.0f;
    if ((codes & 0x03000300u) != 0u)        // the loaded state's speed, only where a velocity curve is not constant
        speed0 = fmaxf(len3_fast(mk3(cur.vx, cur.vy, cur.vz)), 0.0001f);
    const CurveT cl = clamp_curve_t(p.ColorFromLife.RangeAndCount, cur.life, pos.w, c_cl);
    const CurveT cv = clamp_curve_t(p.ColorFromVelocity.RangeAndCount, speed0, speed1, c_cv);
    const CurveT sl = clamp_curve_t(p.SizeFromLife.RangeAndCount, cur.life, pos.w, c_sl);
    const CurveT sv = clamp_curve_t(p.SizeFromVelocity.RangeAndCount, speed0, speed1, c_sv);
    const float size_l = ((c_sl & 3u) == 0u) ? p.SizeFromLife.ABCD.x : bezier1_at(p.SizeFromLife, sl.t1, c_sl & 3u);
    const float size_v = ((c_sv & 3u) == 0u) ? p.SizeFromVelocity.ABCD.x : bezier1_at(p.SizeFromVelocity, sv.t1, c_sv & 3u);
    float4 rd;
    rd.x = live1 ? size_l * size_v : 0.0f;
    rd.y = live1 ? render_rotation(rotation_unscaled(vel.x, vel.y), pos.w, index, a.sys, p) : 0.0f;
    rd.z = live1 ? speed1 : 0.0f;
    rd.w = live1 ? vel.w : 0.0f;
    const float y0 = render_rotation(rotation_unscaled(cur.vx, cur.vy), cur.life, index, a.sys, p);
    const bool same_v = same_bits(cur.vx, vel.x) && same_bits(cur.vy, vel.y) && same_bits(cur.vz, vel.z);
    const bool rc_same = dead || (both && ((a.elide & kElideColor) != 0u) && cl.same && cv.same);
    const bool rdx_same = dead || (both && sl.same && sv.same && (rd.x == rd.x));
    const bool rdy_same = dead || (both && same_bits(y0, rd.y) && (rd.y == rd.y));
    const bool rdz_same = dead || (both && same_v);
    const bool rdw_same = dead || (both && same_bits(cur.ct, vel.w) && (vel.w == vel.w));
    if (__ballot(!rc_same) != 0ull) {
        const float4 attr = load_attributes<true>(up, lane4);
        const float4 color_l = ((c_cl & 3u) == 0u) ? ld4(p.ColorFromLife.A) : bezier4_at(p.ColorFromLife, cl.t1, c_cl & 3u);
        const float4 color_v = ((c_cv & 3u) == 0u) ? ld4(p.ColorFromVelocity.A) : bezier4_at(p.ColorFromVelocity, cv.t1, c_cv & 3u);
        float4 rc = mul4(attr, mul4(color_l, color_v));
        rc.w = sat(rc.w);
        rc.x *= rc.w; rc.y *= rc.w; rc.z *= rc.w;
        st_plane<true>(up, 12, lane4, live1 ? rc.x : 0.0f); st_plane<true>(up, 13, lane4, live1 ? rc.y : 0.0f);
        st_plane<true>(up, 14, lane4, live1 ? rc.z : 0.0f); st_plane<true>(up, 15, lane4, live1 ? rc.w : 0.0f);
    }
    if (__ballot(!rdx_same) != 0ull) st_plane<true>(up, 16, lane4, rd.x);
    if (__ballot(!rdy_same) != 0ull) st_plane<true>(up, 17, lane4, rd.y);
    if (__ballot(!rdz_same) != 0ull) st_plane<true>(up, 18, lane4, rd.z);
    if (__ballot(!rdw_same) != 0ull) st_plane<true>(up, 19, lane4, rd.w);
}

// The lanes of the wave for which p holds, as the scalar mask a compare leaves; testing it is scalar work.  p must BE one compare: the
// ballot of anything else (and __ballot of anything at all) goes through a select and a second vector compare.  Combine masks, not
// predicates.  (Every wave of these kernels is whole: the block is a multiple of 64 threads and no lane has left.)
ILM_DEV uint64_t lane_mask(bool p) { return __builtin_amdgcn_ballot_w64(p); }
constexpr uint64_t kAllLanes = ~0ull;
// which body a wave of the clamp class is in (step_lean_block): the selecting one from the top, or the regular one
constexpr int kBodySelecting = 0, kBodyRegular = 1;

// The lanes that are REGULAR as loaded: alive with a finite life, a category every transform of the list accepts (and so no NaN;
// a.regular_cat_*: build_lean_step) and no NaN in the velocity's x and y.
ILM_DEV uint64_t regular_lanes_loaded(const LeanStep& a, const SlotIn& cur) {
    return lane_mask(cur.life > 0.0f) & lane_mask(cur.life < __builtin_inff()) & lane_mask(cur.ct >= a.regular_cat_lo) & lane_mask(cur.ct <= a.regular_cat_hi) &
           lane_mask(!__builtin_isunordered(cur.vx, cur.vy));
}
// ... in a chunk whose category record lies inside the launch's filter (category_proven): every slot with a finite life > 0 has a
// category the transforms accept, so the two category compares are decided and the category itself is not needed.
ILM_DEV uint64_t regular_lanes_loaded_proven(const SlotIn& cur) {
    return lane_mask(cur.life > 0.0f) & lane_mask(cur.life < __builtin_inff()) & lane_mask(!__builtin_isunordered(cur.vx, cur.vy));
}
// The chunk's category record against the launch's filter: {lo, hi} is one 8-byte scalar load through the constant address space (the
// table is written by category_bounds_kernel ahead of the launch on its stream and never during one: the chunk table's rule).  Float
// compares, so a NaN on either side -- a chunk with a NaN category, a filter with a NaN bound -- proves nothing; no branch between
// them.  Wave-uniform.  (Fetching the record and the chunk's base pointer by one hand-issued pair of loads measured the same:
// docs/experiments.md 7.38.)
typedef const uint64_t __attribute__((address_space(4))) CUint64;
__device__ __attribute__((aligned(8))) float g_no_category_record[2] = { __builtin_nanf(""), __builtin_nanf("") };
ILM_DEV bool category_proven(const LeanStep& a, int chunk) {
    const uint64_t record = *(CUint64*)((const char*)a.cat_bounds + chunk * a.cat_stride);
    const float lo = __builtin_bit_cast(float, (uint32_t)record), hi = __builtin_bit_cast(float, (uint32_t)(record >> 32));
    return ((lo >= a.regular_cat_lo) & (hi <= a.regular_cat_hi)) != 0;
}
// the slot's loads without the category plane (load_slot<false, true> otherwise)
ILM_DEV SlotIn load_slot_uncategorised(const UnitPlanes& u, unsigned lane4) {
    SlotIn s;
    s.life = ld_plane<true>(u, 3, lane4);
    s.px = ld_plane<true>(u, 0, lane4); s.py = ld_plane<true>(u, 1, lane4); s.pz = ld_plane<true>(u, 2, lane4);
    s.vx = ld_plane<true>(u, 4, lane4); s.vy = ld_plane<true>(u, 5, lane4); s.vz = ld_plane<true>(u, 6, lane4); s.ct = 0.0f;
    s.ar = s.ag = s.ab = s.aa = 0.0f;
    return s;
}
// ... and after the update: still alive with a finite life, no NaN in the new velocity's x and y.
ILM_DEV uint64_t regular_lanes_updated(float new_life, float vx, float vy) {
    return lane_mask(new_life > 0.0f) & lane_mask(new_life < __builtin_inff()) & lane_mask(!__builtin_isunordered(vx, vy));
}
// clamp_curve_t for a wave of live lanes: t for the new state, and the lanes where the proof fails (t changed its bits or is a NaN)
ILM_DEV uint64_t clamp_curve_changed(const IlmFloat4& rc, float v0, float v1, uint32_t code, float& t1) {
    t1 = 0.0f;      // a constant curve reads no t
    if ((code & 3u) == 0u) return 0ull;
    t1 = t_for_clamp_bezier(rc, v1, code);
    return lane_mask(!same_bits(t_for_clamp_bezier(rc, v0, code), t1)) | lane_mask(t1 != t1);
}

// store_changed_render_planes_clamp for a wave whose 64 lanes are regular before and after the step (regular_lanes_*): the same stores of
// the same bits, without what those masks decide.  Every lane is `both`, none `dead`, so each *_same is its bare proof and no value is
// selected against zero.  The category keeps its bits and is no NaN: rd.w is never stored.  The velocity's x and y are no NaN, so
// rotation_unscaled is 0 for both states.  With kElideRotation the host has found RotationFromLifeAndIndex[0] == 0: life x (+-0) has the
// same bits for any two finite positive lives, rd.y's operands are the loaded state's and it keeps its bits (and, the index factor
// being finite, is no NaN).
// v_changed: the lanes whose velocity changed a bit (the caller's plane compares).
ILM_DEV void store_changed_render_planes_regular(const LeanStep& a, const UnitPlanes& up, unsigned lane4, float fx, float fy, const SlotIn& cur,
                                                 float4 pos, float4 vel, uint64_t v_changed) {
    const IlmUpdateParams& p = a.update;
    const uint32_t codes = a.bezier_codes & kClampCodes;
    const uint32_t c_cl = codes & 0xFFu, c_cv = (codes >> 8) & 0xFFu, c_sl = (codes >> 16) & 0xFFu, c_sv = codes >> 24;
    const float speed1 = fmaxf(len3_fast(xyz(vel)), 0.0001f);
    float speed0 = 0.0f;
    if ((codes & 0x03000300u) != 0u)        // the loaded state's speed, only where a velocity curve is not constant
        speed0 = fmaxf(len3_fast(mk3(cur.vx, cur.vy, cur.vz)), 0.0001f);
    float t_cl, t_cv, t_sl, t_sv;
    const uint64_t rc_changed = clamp_curve_changed(p.ColorFromLife.RangeAndCount, cur.life, pos.w, c_cl, t_cl) |
                                clamp_curve_changed(p.ColorFromVelocity.RangeAndCount, speed0, speed1, c_cv, t_cv);
    const uint64_t size_changed = clamp_curve_changed(p.SizeFromLife.RangeAndCount, cur.life, pos.w, c_sl, t_sl) |
                                  clamp_curve_changed(p.SizeFromVelocity.RangeAndCount, speed0, speed1, c_sv, t_sv);
    if (((a.elide & kElideColor) == 0u) || rc_changed != 0ull) {
        const float4 attr = load_attributes<true>(up, lane4);
        const float4 color_l = ((c_cl & 3u) == 0u) ? ld4(p.ColorFromLife.A) : bezier4_at(p.ColorFromLife, t_cl, c_cl & 3u);
        const float4 color_v = ((c_cv & 3u) == 0u) ? ld4(p.ColorFromVelocity.A) : bezier4_at(p.ColorFromVelocity, t_cv, c_cv & 3u);
        float4 rc = mul4(attr, mul4(color_l, color_v));
        rc.w = sat(rc.w);
        rc.x *= rc.w; rc.y *= rc.w; rc.z *= rc.w;
        st_plane<true>(up, 12, lane4, rc.x); st_plane<true>(up, 13, lane4, rc.y); st_plane<true>(up, 14, lane4, rc.z); st_plane<true>(up, 15, lane4, rc.w);
    }
    const float size_l = ((c_sl & 3u) == 0u) ? p.SizeFromLife.ABCD.x : bezier1_at(p.SizeFromLife, t_sl, c_sl & 3u);
    const float size_v = ((c_sv & 3u) == 0u) ? p.SizeFromVelocity.ABCD.x : bezier1_at(p.SizeFromVelocity, t_sv, c_sv & 3u);
    const float rdx = size_l * size_v;
    if ((size_changed | lane_mask(rdx != rdx)) != 0ull) st_plane<true>(up, 16, lane4, rdx);
    if ((a.elide & kElideRotation) == 0u) {
        const float index = render_index(fx, fy);
        const float rdy = render_rotation(0.0f, pos.w, index, a.sys, p);
        const float y0 = render_rotation(0.0f, cur.life, index, a.sys, p);
        if ((lane_mask(!same_bits(y0, rdy)) | lane_mask(rdy != rdy)) != 0ull) st_plane<true>(up, 17, lane4, rdy);
    }
    if (v_changed != 0ull) st_plane<true>(up, 18, lane4, speed1);
}


// One block of the lean step, for one curve class (the kernels below).
template <bool SPAWN, bool STREAM, int CURVES>
ILM_DEV void step_lean_block() {
    static_assert(CURVES == kCurvesGeneral || (STREAM && !SPAWN), "the curve classes are instantiations of the streaming variant without spawners");
    __shared__ uint32_t wave_live[kStepThreads / 64];
    const LeanStep& a = *(const LeanStep*)(CLeanStep*)__builtin_amdgcn_kernarg_segment_ptr();
    // (only the launch's first generation of blocks can be the first to read a line; for the others the loads would just load the
    // scalar cache: one lookup per line per wave)
    if (blockIdx.x < kTouchBlocks) touch_kernarg_lines_lean();
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    int v = (int)blockIdx.x * (kStepThreads / 64) + a.unit_rotate;      // first unit of the block (rotation: see step_kernel)
    if (v >= a.total_padded) v -= a.total_padded;
    const int u = v + wave;
    uint32_t n_live = 0;
    if (u < a.total_units) {
        const int chunk_rel = u >> a.upc_shift;
        const int seg = u - (chunk_rel << a.upc_shift);
        const int chunk = a.first_chunk + chunk_rel;
        bool untouched = false;
        if (a.partial_count != 0) {
#pragma unroll
            for (int k = 0; k < kMaxPartialChunks; k++)
                untouched = untouched || ((a.partial_chunk[k] == chunk) && (seg >= a.partial_units[k]));
        }
        if (!untouched) {
            const unsigned lane4 = lane * 4u;
            // the chunk table through the constant address space: a scalar load whatever the optimiser thinks may alias (behind the
            // volatile asm of touch_kernarg_lines it would otherwise fetch the base with a VECTOR load and wrap every plane access in
            // a waterfall loop over a "divergent" buffer resource: +160 vector instructions per wave); the table is written by a copy
            // that precedes the launch on its stream and never during one
            // kCurvesClamp: a wave of a chunk whose category record the filter contains leaves the category plane alone until it needs it
            bool ct_pending = false;
            if constexpr (CURVES == kCurvesClamp) ct_pending = category_proven(a, chunk);
            const UnitPlanes up = unit_planes(((CBase*)a.chunk_bases)[chunk], a.stride, seg * 64);
            // a render-current chunk needs its attributes only where renderColor is recomputed: loaded below, by the waves that do
            const bool elide = STREAM && ((CURVES == kCurvesClamp) || (a.elide & kElideDerived) != 0u);
            SlotIn cur;
            if (CURVES == kCurvesClamp && ct_pending) cur = load_slot_uncategorised(up, lane4);
            else cur = load_slot<false, STREAM>(up, lane4);
            const bool ct_proven = ct_pending;
            if (!elide) {
                const float4 stored = load_attributes<STREAM>(up, lane4);
                cur.ar = stored.x; cur.ag = stored.y; cur.ab = stored.z; cur.aa = stored.w;
            }
            int first, row, x0; float fx, fy;
            lean_unit_slot(a, seg, lane, first, row, x0, fx, fy);
            NoiseDeltas noise;
            noise.valid = false;
            if (a.noise_op >= 0)
                noise = noise_prepare(a.noise, a.noise_big, x0, row);

            float4 pos = mk4(cur.px, cur.py, cur.pz, cur.life);
            float4 vel = mk4(cur.vx, cur.vy, cur.vz, cur.ct);
            float4 attr = mk4(cur.ar, cur.ag, cur.ab, cur.aa);
            bool spawn_here = false, spawned = false;
            if constexpr (SPAWN) {
                for (int s = 0; s < a.spawn_count; s++) {
                    if (a.spawn_chunk[s] == chunk && seg >= a.spawn_unit_lo[s] && seg <= a.spawn_unit_hi[s]) {
                        const IlmSpawnRecord& r = a.spawns[s];
                        const float fi = (float)(first + (int)lane);
                        if (fi >= r.Params.ChunkSizeAndIndices[1] && fi <= r.Params.ChunkSizeAndIndices[2]) {
                            spawn_here = true;
                            if (spawn_slot(pos, vel, attr, fx, fy, a.rnd, a.rw, a.rh, a.inv_rw, a.inv_rh, r.Params))
                                spawned = true;
                        }
                    }
                }
            }
            // `<= 0` as the shaders test it: a NaN life is not dead.  A dead slot nothing writes keeps the cleared target's zeros.
            const bool process = !(cur.life <= 0.0f) || spawn_here;
            const float4 zero = mk4(0.0f, 0.0f, 0.0f, 0.0f);
            float4 rc = zero, rd = zero;
            if constexpr (CURVES == kCurvesClamp) {
                // A wave of 64 regular lanes (regular_lanes_loaded) runs the transforms and the update without the tests and selects that
                // serve dead, filtered and NaN lanes: the same operations on the same operands, so where the wave turns out not to stay
                // regular the selects applied afterwards give the bits of the selecting body.  Only FMA can take a life to <= 0 (Gravity
                // leaves it alone, a lean launch's Noise leaves it or makes it a NaN: noise_may_revive), and only FMA writes the category
                // (its lerp covers the velocity's w; Gravity and Noise pass it through).  A wave where FMA does either -- a life <= 0, or a
                // category with other bits than the loaded one, -0 to +0 and NaN included -- starts again from the loaded state in the
                // selecting body, which filters the later transforms by the new category, skips them for a dead lane and stores the
                // category plane and rd.w.  So in the regular body the category is the loaded one to the end.
                // A wave whose chunk is proven (category_proven) carries no category: it forms the loaded mask without the category compares
                // and, wherever it leaves the regular path -- a mask that is not full, the second mask -- loads the plane there (ct_pending)
                // and goes on with the state a wave that loaded it up front has at that point.  No such wave meets an FMA: launch_step
                // gives a launch with one the NaN record, so every wave of it loads the category up front.
                int body = kBodySelecting;
                if ((ct_proven ? regular_lanes_loaded_proven(cur) : regular_lanes_loaded(a, cur)) == kAllLanes) {
                    body = kBodyRegular;
#pragma unroll
                    for (int o = 0; o < ILM_MAX_OPS; o++) {
                        if (body == kBodyRegular && o < a.op_count) {
                            const int type = a.op_type[o];
                            if (type == ILM_OP_GRAVITY) {
                                apply_gravity_lean<false>(pos, vel, a.op[o].gravity, a.sys.GlobalSettings.x, a.sys.GlobalSettings.z);
                            } else if (type == ILM_OP_NOISE) {
                                apply_noise<false, false>(pos, vel, fx, fy, a.rnd, a.rw, a.rh, a.sys, a.op[o].noise, a.inv_rw, a.inv_rh, a.dop[o],
                                                          (o == a.noise_op) ? noise : NoiseDeltas{ false, zero, zero });
                            } else {
                                apply_fma<false, false>(pos, vel, a.sys, a.op[o].fma, a.dop[o]);
                                if ((lane_mask(pos.w <= 0.0f) | lane_mask(!same_bits(vel.w, cur.ct))) != 0ull) body = kBodySelecting;
                            }
                        }
                    }
                }
                if (body == kBodyRegular) {
                    update_positions_unselected(pos, vel, a.sys, a.dt_s);
                    const bool stays = regular_lanes_updated(pos.w, vel.x, vel.y) == kAllLanes;
                    const int counting = __builtin_amdgcn_readfirstlane(*(CInt32*)&g_step_count_regular_waves);
                    if (counting != 0 && lane == 0u) {
                        if (counting & 1) atomicAdd(&g_step_regular_waves[stays ? 0 : 1], 1ull);
                        if (counting & 2) atomicAdd(&g_step_category_waves[ct_proven ? (stays ? 0 : 1) : 2], 1ull);
                    }
                    if (stays) {
                        const uint64_t vx_changed = lane_mask(!same_bits(vel.x, cur.vx)), vy_changed = lane_mask(!same_bits(vel.y, cur.vy)), vz_changed = lane_mask(!same_bits(vel.z, cur.vz));
                        if (lane_mask(!same_bits(pos.x, cur.px)) != 0ull) st_plane<true>(up, 0, lane4, pos.x);
                        if (lane_mask(!same_bits(pos.y, cur.py)) != 0ull) st_plane<true>(up, 1, lane4, pos.y);
                        if (lane_mask(!same_bits(pos.z, cur.pz)) != 0ull) st_plane<true>(up, 2, lane4, pos.z);
                        if (lane_mask(!same_bits(pos.w, cur.life)) != 0ull) st_plane<true>(up, 3, lane4, pos.w);
                        if (vx_changed != 0ull) st_plane<true>(up, 4, lane4, vel.x);
                        if (vy_changed != 0ull) st_plane<true>(up, 5, lane4, vel.y);
                        if (vz_changed != 0ull) st_plane<true>(up, 6, lane4, vel.z);
                        // (the category keeps its bits: no store)
                        store_changed_render_planes_regular(a, up, lane4, fx, fy, cur, pos, vel, vx_changed | vy_changed | vz_changed);
                        n_live = 64u;
                        goto unit_stored;       // (a flag tested at the stores below moved the general instantiations' registers)
                    }
                    if (ct_pending) {       // the category passed through the transforms and the update: the loaded one
                        cur.ct = ld_plane<true>(up, 7, lane4);
                        vel.w = cur.ct;
                        ct_pending = false;
                    }
                    // every lane was alive after the transforms: update_positions_select's `keep` is the new life's test alone
                    const bool keep = !(pos.w <= 0.0f);
                    pos = mk4(keep ? pos.x : 0.0f, keep ? pos.y : 0.0f, keep ? pos.z : 0.0f, keep ? pos.w : 0.0f);
                    vel = mk4(keep ? vel.x : 0.0f, keep ? vel.y : 0.0f, keep ? vel.z : 0.0f, keep ? vel.w : 0.0f);
                }
                if (body == kBodySelecting) {
                    if (ct_pending) {
                        cur.ct = ld_plane<true>(up, 7, lane4);
                        ct_pending = false;
                    }
                    {
                        const int counting = __builtin_amdgcn_readfirstlane(*(CInt32*)&g_step_count_regular_waves);
                        if ((counting & 2) != 0 && lane == 0u) atomicAdd(&g_step_category_waves[ct_proven ? 1 : 2], 1ull);
                    }
                    pos = mk4(cur.px, cur.py, cur.pz, cur.life);
                    vel = mk4(cur.vx, cur.vy, cur.vz, cur.ct);
                    if (__ballot(process) != 0ull) {
                        // Every lane goes through the transforms and the update, and one select at the end keeps the live ones: a slot the
                        // step does not process comes out as zeros whatever was computed for it.  The transforms are dispatched from
                        // unrolled positions so that position and velocity stay in their registers from one to the next.
#pragma unroll
                        for (int o = 0; o < ILM_MAX_OPS; o++) {
                            if (o < a.op_count) {
                                const int type = a.op_type[o];
                                if (type == ILM_OP_GRAVITY)
                                    apply_gravity_lean(pos, vel, a.op[o].gravity, a.sys.GlobalSettings.x, a.sys.GlobalSettings.z);
                                else if (type == ILM_OP_NOISE)
                                    apply_noise<true, false>(pos, vel, fx, fy, a.rnd, a.rw, a.rh, a.sys, a.op[o].noise, a.inv_rw, a.inv_rh, a.dop[o],
                                                             (o == a.noise_op) ? noise : NoiseDeltas{ false, zero, zero });
                                else
                                    apply_fma<true, false>(pos, vel, a.sys, a.op[o].fma, a.dop[o]);
                            }
                        }
                        update_positions_select(pos, vel, a.sys, a.dt_s, process && !(pos.w <= 0.0f));
                    } else {
                        pos = vel = zero;
                    }
                }
            } else if (__ballot(process) != 0ull) {
                if (process) {
                    for (int o = 0; o < a.op_count; o++) {
                        const int type = a.op_type[o];
                        if (type == ILM_OP_GRAVITY)
                            apply_gravity_lean(pos, vel, a.op[o].gravity, a.sys.GlobalSettings.x, a.sys.GlobalSettings.z);
                        else if (type == ILM_OP_NOISE)
                            apply_noise(pos, vel, fx, fy, a.rnd, a.rw, a.rh, a.sys, a.op[o].noise, a.inv_rw, a.inv_rh, a.dop[o],
                                        (o == a.noise_op) ? noise : NoiseDeltas{ false, zero, zero });
                        else
                            apply_fma(pos, vel, a.sys, a.op[o].fma, a.dop[o]);
                    }
                    if (pos.w <= 0.0f) {
                        pos = vel = zero;  // readStateOrDiscard: discard => cleared target
                    } else {
                        update_positions(pos, vel, a.sys, a.dt_s);
                        if (!elide)
                            render_data(fx, fy, pos, vel, attr, a.sys, a.update, a.bezier_codes, a.update_bits, nullptr, 0, 0, rc, rd);
                    }
                } else {
                    pos = vel = zero;
                }
            } else {
                pos = vel = zero;
            }
            // STREAM: a plane is stored when some lane of the wave changed its bits (integer compares: NaN and -0.0 exactly), at full width
            st_plane_changed<STREAM>(up, 0, lane4, pos.x, cur.px); st_plane_changed<STREAM>(up, 1, lane4, pos.y, cur.py);
            st_plane_changed<STREAM>(up, 2, lane4, pos.z, cur.pz); st_plane_changed<STREAM>(up, 3, lane4, pos.w, cur.life);
            st_plane_changed<STREAM>(up, 4, lane4, vel.x, cur.vx); st_plane_changed<STREAM>(up, 5, lane4, vel.y, cur.vy);
            st_plane_changed<STREAM>(up, 6, lane4, vel.z, cur.vz); st_plane_changed<STREAM>(up, 7, lane4, vel.w, cur.ct);
            if constexpr (SPAWN) {
                if (spawned)
                    store_attributes<STREAM>(up, lane4, attr);
            }
            if (!elide) {
                store_render<STREAM>(up, lane4, rc, rd);
            } else if constexpr (CURVES == kCurvesClamp) {
                store_changed_render_planes_clamp(a, up, lane4, fx, fy, cur, pos, vel);
            } else {
                store_changed_render_planes<SPAWN, STREAM>(a, up, lane4, fx, fy, cur, pos, vel, attr, spawned);
            }
            n_live = (uint32_t)__popcll(__ballot(pos.w > 0.0f));
        // The clamp class's regular body jumps here with its planes stored and n_live set.  Everything between `process` and this label
        // belongs to the selecting bodies alone: whatever a unit must do whichever body ran (the count below is the one such thing
        // today) goes AFTER the label, never above it.
        unit_stored: __attribute__((unused));
        }
    }
    if (a.flags & ILM_STEP_COUNT_LIVE)
        publish_block_count(wave_live, n_live, lane, wave, v < a.total_units, a.first_chunk + (v >> a.upc_shift),
                            (v & ((1 << a.upc_shift) - 1)) / (kStepThreads / 64), (1 << a.upc_shift) / (kStepThreads / 64), a.count_buckets,
                            a.live_counts, a.zero_counts, a.zero_n, a.host_counts, a.count_seq);
}

// The general instantiations keep the kernel names the profiles and bench.py's traffic figures are keyed by; the class is a kernel of
// its own (a class selected inside step_lean_kernel<false, true> by a launch-uniform word took the kernel from 8 waves per SIMD to 7 and
// the headline from 0.78 to 0.89 ms).
template <bool SPAWN, bool STREAM>
__global__ __launch_bounds__(kStepThreads) void step_lean_kernel(const LeanStep a_) { step_lean_block<SPAWN, STREAM, kCurvesGeneral>(); }
__global__ __launch_bounds__(kStepThreads) void step_lean_clamp_kernel(const LeanStep a_) { step_lean_block<false, true, kCurvesClamp>(); }

// ---------------------------------------------------------------------------------------------
// the lean collision step (r06) -- UpdateParticleSystemWithDistanceField.fx:29-147 on the lean descriptor
// ---------------------------------------------------------------------------------------------
// The collision update is two things in one shader.  EVERY live particle samples the field where it is and where it is going (the
// first iteration of the sweep): two dependent lookups, the same for all lanes.  A particle whose first sweep lookup lands inside an
// obstacle (14 % of them on the demo's field) goes on: up to two more sweep lookups, estimateNormal4 (four more), the bounce / redirect
// / escape arithmetic -- about as many vector instructions again as the whole rest of the step, run by a wave for its few such lanes
// (the interpreter's step_kernel<.., DF>: 1 071 instructions per wave at 39.4 of 64 lanes, profiles/r06_collision_step.txt).
// Here a wave walks K consecutive units in three phases.
//   A  per unit: load, spawn, transforms, the common path at full width.  The lanes that collided are PARKED -- their state after the
//      transforms and the two distances already sampled, eleven words, in a ring of 128 entries the wave owns in LDS (no barrier: the
//      ring is private to the wave).  The unit's position and velocity stay in registers; nothing is stored yet.
//   L  whenever 64 are parked, and once more after the last unit: the parked particles, one per lane, through the rest of the reference
//      update (df_long, which the interpreter's update_with_distance_field runs too); the results go back into the same ring
//      entries.
//   B  per unit: the parked lanes take their results from the ring, then computeRenderData and all sixteen stores at FULL width.
// So the long path runs at 64 lanes -- or, for the remainder, at whatever K units leave -- instead of at ~9 lanes once per unit, and
// every plane of a unit is still written by ONE full-width store (a first form of this kernel stored the finished lanes at once and
// the parked ones later, from the long pass: two partial writes per line, and cfg4's share took 507-597 us against the interpreter's
// 394 -- masked and scattered 4-byte stores cost a read-modify-write each once the line has left the L2).
// A ring that would overflow (more than 128 of a wave's K x 64 particles colliding) is not waited for: that unit's parked lanes take the
// long path in place, as the interpreter does.
struct LeanStepDf {
    LeanStep base;
    IlmDistanceFieldUniforms df;
    SdfView sdf;
};
static_assert(sizeof(LeanStepDf) <= 4096, "LeanStepDf travels in the kernarg segment (4 KB)");
static_assert(sizeof(LeanStepDf) > 0xd40 && sizeof(LeanStepDf) <= 0xe00, "touch_kernarg_lines_lean_df reads one dword of each 64-byte line of LeanStepDf");
ILM_DEV void touch_kernarg_lines_lean_df() {       // LeanStepDf: 54 .. 56 lines
    const auto kp = __builtin_amdgcn_kernarg_segment_ptr();
    uint32_t sink;
    asm volatile(ILM_T16(0x0) ILM_T16(0x400) ILM_T16(0x800) ILM_T4(0xc00) ILM_T1(0xd00) ILM_T1(0xd40) "s_waitcnt lgkmcnt(0)"
                 : "=&s"(sink) : "s"(kp));
}
typedef const LeanStepDf __attribute__((address_space(4))) CLeanStepDf;

constexpr int kDfRing = 128;                     // parked particles per wave
struct DfParked { float px[kDfRing], py[kDfRing], pz[kDfRing], life[kDfRing], vx[kDfRing], vy[kDfRing], vz[kDfRing], ct[kDfRing], d0[kDfRing], d1[kDfRing]; uint32_t slot[kDfRing]; };   // slot: bit 31 = d1 is the first iteration's lookup

// The common path of PS_Update (distance field) for a live slot (life > 0 on entry): everything a particle needs that meets no obstacle.
// The reference samples the field at the particle (initial_distance) and then at old + unit * travel with travel = max(0, min(
// initial_distance, |velocity| dt)) -- two DEPENDENT lookups.  Away from obstacles travel IS |velocity| dt, known before any lookup: both
// positions are sampled at once, and when min() did pick |velocity| dt (bit for bit) the second sample is the sweep's first
// step_distance -- same position, same bits.  Returns 0 when the particle is finished (position and velocity final; zeros for one that
// died); 1 when it must go on with the sweep's first iteration still to do (travel is not |velocity| dt: it sits at or inside an
// obstacle); 2 when the first iteration is done and collided (step_distance valid).  For 1 and 2 position and velocity are left as they
// came: the caller parks them for df_long.  Same operations in the same order as update_with_distance_field takes on these paths
// (tests/test_step_kernels_gpu.py holds the kernels bit-equal, sample counts included).
template <int FMT>
ILM_DEV int df_common_path(float4& pos, float4& vel, const IlmParticleSystemUniforms& sys, float dts, const IlmDistanceFieldUniforms& df, const SdfView& sdf, int& samples,
                           float& initial_distance, float& step_distance) {
#pragma clang fp contract(off)
    const float4 zero = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    const float new_life = pos.w - (sys.GlobalSettings.w * dts);
    initial_distance = step_distance = 0.0f;
    if (new_life <= 0.0f) {
        pos = vel = zero;
        return 0;
    }
    const float collision_distance = sys.CollisionSettings.z;
    const f3 old_xyz = xyz(pos);
    const f3 unit_vector = norm3(xyz(vel));
    const f3 velocity = friction_and_maximum(xyz(vel), sys, dts);
    const f3 scaled_velocity = velocity * dts;
    const float reach = len3(scaled_velocity);
    const f3 ahead = old_xyz + (unit_vector * reach);
    initial_distance = sample_distance_field<(FMT & 1), true, (FMT & 2) != 0, (FMT & 4) != 0>(old_xyz, df, sdf);
    step_distance = sample_distance_field<(FMT & 1), true, (FMT & 2) != 0, (FMT & 4) != 0>(ahead, df, sdf);        // (independent of the first: both in flight together)
    samples++;
    const bool was_colliding = initial_distance < collision_distance;
    const float travel_distance = fmaxf(0.0f, fminf(initial_distance, reach));
    if (__builtin_bit_cast(uint32_t, travel_distance) != __builtin_bit_cast(uint32_t, reach))
        return 1;                                                 // the sweep starts somewhere else than `ahead`
    if (was_colliding || !(travel_distance <= 0.001f)) {          // step_count 1 or MAX_STEP_COUNT: the sweep's first iteration runs, at `ahead`
        samples++;
        if (step_distance < collision_distance)
            return 2;
    }
    pos = mk4(ahead.x, ahead.y, ahead.z, new_life);
    vel = mk4(velocity.x, velocity.y, velocity.z, fmaxf(vel.w - 1.0f, 0.0f));
    return 0;
}

template <int FMT, bool SPAWN, bool STREAM, int K>
__global__ __launch_bounds__(kStepThreads) void step_lean_df_kernel(const LeanStepDf a_) {
    static_assert(K == 1 || K == 2 || K == 4, "units per wave");
    __shared__ uint32_t wave_live[kStepThreads / 64];
    __shared__ DfParked parked_all[kStepThreads / 64];
    const LeanStepDf& A = *(const LeanStepDf*)(CLeanStepDf*)__builtin_amdgcn_kernarg_segment_ptr();
    const LeanStep& a = A.base;
    if (blockIdx.x < kTouchBlocks / K) touch_kernarg_lines_lean_df();
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    DfParked& parked = parked_all[wave];
    constexpr int kUnitsPerBlock = (kStepThreads / 64) * K;
    int v = (int)blockIdx.x * kUnitsPerBlock + a.unit_rotate;           // first unit of the block (rotation: see step_kernel; a multiple of kUnitsPerBlock)
    if (v >= a.total_padded) v -= a.total_padded;
    const int u0 = v + wave * K;                                        // this wave's K consecutive units: one chunk (units per chunk is a multiple of kUnitsPerBlock)
    uint32_t n_live = 0;
    int sdf_samples = 0;
    const float4 zero = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    if (u0 < a.total_units) {
        const int chunk_rel = u0 >> a.upc_shift;
        const int seg0 = u0 - (chunk_rel << a.upc_shift);
        const int chunk = a.first_chunk + chunk_rel;
        int seg_end = 1 << a.upc_shift;                                 // units of this chunk that hold particles
        if (a.partial_count != 0) {
#pragma unroll
            for (int k = 0; k < kMaxPartialChunks; k++)
                if (a.partial_chunk[k] == chunk) seg_end = min(seg_end, a.partial_units[k]);
        }
        const int units = max(0, min(K, seg_end - seg0));               // (past seg_end: the never-written tail of a spawn-target chunk, zeros that stay zeros)
        float* const chunk_base = ((CBase*)a.chunk_bases)[chunk];
        const unsigned lane4 = lane * 4u;
        const unsigned long long lanes_below = (1ull << lane) - 1ull;
        // what a unit keeps in registers between phase A and phase B, and where its parked lanes sit in the ring
        float4 hp0 = zero, hp1 = zero, hp2 = zero, hp3 = zero, hv0 = zero, hv1 = zero, hv2 = zero, hv3 = zero;
        unsigned long long pm0 = 0ull, pm1 = 0ull, pm2 = 0ull, pm3 = 0ull;
        uint32_t pb0 = 0, pb1 = 0, pb2 = 0, pb3 = 0;
        uint32_t pending = 0, done = 0;                                 // ring entries [0, pending) hold parked particles, [0, done) their results

        // the parked particles [first, first + count), count <= 64, one per lane: the rest of the reference's update, results in place
        auto long_pass = [&](uint32_t first, uint32_t count) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane < count) {
                const uint32_t e = first + lane;
                float4 pos = mk4(parked.px[e], parked.py[e], parked.pz[e], parked.life[e]);
                float4 vel = mk4(parked.vx[e], parked.vy[e], parked.vz[e], parked.ct[e]);
                const uint32_t tagged = parked.slot[e];
                const int slot = (int)(tagged & 0x7FFFFFFFu);
                const int sy = slot >> a.cs_shift;
                const float fx = (float)(slot - (sy << a.cs_shift)), fy = (float)sy;
                df_long<FMT>(pos, vel, fx, fy, parked.d0[e], parked.d1[e], (tagged >> 31) != 0u, a.sys, a.dt_s, A.df, A.sdf, sdf_samples);
                parked.px[e] = pos.x; parked.py[e] = pos.y; parked.pz[e] = pos.z; parked.life[e] = pos.w;
                parked.vx[e] = vel.x; parked.vy[e] = vel.y; parked.vz[e] = vel.z; parked.ct[e] = vel.w;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        };

        // ---- phase A ----
#pragma nounroll
        for (int j = 0; j < units; j++) {
            const int seg = seg0 + j;
            const UnitPlanes up = unit_planes(chunk_base, a.stride, seg * 64);
            const SlotIn cur = load_slot<true, STREAM>(up, lane4);
            int first, row, x0; float fx, fy;
            lean_unit_slot(a, seg, lane, first, row, x0, fx, fy);
            NoiseDeltas noise;
            noise.valid = false;
            if (a.noise_op >= 0)
                noise = noise_prepare(a.noise, a.noise_big, x0, row);
            float4 pos = mk4(cur.px, cur.py, cur.pz, cur.life);
            float4 vel = mk4(cur.vx, cur.vy, cur.vz, cur.ct);
            float4 attr = mk4(cur.ar, cur.ag, cur.ab, cur.aa);
            bool spawn_here = false, spawned = false;
            if constexpr (SPAWN) {
                for (int s = 0; s < a.spawn_count; s++) {
                    if (a.spawn_chunk[s] == chunk && seg >= a.spawn_unit_lo[s] && seg <= a.spawn_unit_hi[s]) {
                        const IlmSpawnRecord& r = a.spawns[s];
                        const float fi = (float)(first + (int)lane);
                        if (fi >= r.Params.ChunkSizeAndIndices[1] && fi <= r.Params.ChunkSizeAndIndices[2]) {
                            spawn_here = true;
                            if (spawn_slot(pos, vel, attr, fx, fy, a.rnd, a.rw, a.rh, a.inv_rw, a.inv_rh, r.Params))
                                spawned = true;
                        }
                    }
                }
            }
            const bool process = !(cur.life <= 0.0f) || spawn_here;
            int parking = 0;
            float d0 = 0.0f, d1 = 0.0f;
            if (__ballot(process) != 0ull) {
                if (process) {
                    for (int o = 0; o < a.op_count; o++) {
                        const int type = a.op_type[o];
                        if (type == ILM_OP_GRAVITY)
                            apply_gravity_lean(pos, vel, a.op[o].gravity, a.sys.GlobalSettings.x, a.sys.GlobalSettings.z);
                        else if (type == ILM_OP_NOISE)
                            apply_noise(pos, vel, fx, fy, a.rnd, a.rw, a.rh, a.sys, a.op[o].noise, a.inv_rw, a.inv_rh, a.dop[o],
                                        (o == a.noise_op) ? noise : NoiseDeltas{ false, zero, zero });
                        else
                            apply_fma(pos, vel, a.sys, a.op[o].fma, a.dop[o]);
                    }
                    if (pos.w <= 0.0f)
                        pos = vel = zero;  // readStateOrDiscard: discard => cleared target
                    else
                        parking = df_common_path<FMT>(pos, vel, a.sys, a.dt_s, A.df, A.sdf, sdf_samples, d0, d1);
                } else {
                    pos = vel = zero;
                }
            } else {
                pos = vel = zero;
            }
            if constexpr (SPAWN) {
                if (spawned) {      // (phase B reads the attributes back from the planes)
                    st_plane<STREAM>(up, 8, lane4, attr.x); st_plane<STREAM>(up, 9, lane4, attr.y); st_plane<STREAM>(up, 10, lane4, attr.z); st_plane<STREAM>(up, 11, lane4, attr.w);
                }
            }
            const bool park = parking != 0;
            unsigned long long park_mask = __ballot(park);
            const uint32_t n_park = (uint32_t)__popcll(park_mask);
            if (n_park != 0u && pending + n_park > (uint32_t)kDfRing) {
                // no room in the ring: these lanes take the long path here, as the interpreter's kernel does
                if (park) df_long<FMT>(pos, vel, fx, fy, d0, d1, parking == 2, a.sys, a.dt_s, A.df, A.sdf, sdf_samples);
                park_mask = 0ull;
            } else if (n_park != 0u) {
                if (park) {
                    const uint32_t e = pending + (uint32_t)__popcll(park_mask & lanes_below);
                    parked.px[e] = pos.x; parked.py[e] = pos.y; parked.pz[e] = pos.z; parked.life[e] = pos.w;
                    parked.vx[e] = vel.x; parked.vy[e] = vel.y; parked.vz[e] = vel.z; parked.ct[e] = vel.w;
                    parked.d0[e] = d0; parked.d1[e] = d1; parked.slot[e] = (uint32_t)(first + (int)lane) | ((parking == 2) ? 0x80000000u : 0u);
                }
            }
            if (K == 1 || j == 0) { hp0 = pos; hv0 = vel; pm0 = park_mask; pb0 = pending; }
            else if (K == 2 || j == 1) { hp1 = pos; hv1 = vel; pm1 = park_mask; pb1 = pending; }
            else if (j == 2) { hp2 = pos; hv2 = vel; pm2 = park_mask; pb2 = pending; }
            else { hp3 = pos; hv3 = vel; pm3 = park_mask; pb3 = pending; }
            pending += (uint32_t)__popcll(park_mask);
            if (pending - done >= 64u) { long_pass(done, 64u); done += 64u; }
        }
        // ---- phase L: what is still parked ----
        while (done < pending) {
            const uint32_t count = min(64u, pending - done);
            long_pass(done, count);
            done += count;
        }
        // ---- phase B ----
        if constexpr (SPAWN) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the attributes stored for slots spawned in this launch are read back below
#pragma nounroll
        for (int j = 0; j < units; j++) {
            const int seg = seg0 + j;
            const UnitPlanes up = unit_planes(chunk_base, a.stride, seg * 64);
            // (the plane accesses of this kernel stay written out: through the plane-group helpers the spawning cache-resident instantiations
            // come out with other scalar registers and another order of their mask operations)
            const float4 attr = mk4(ld_plane<STREAM>(up, 8, lane4), ld_plane<STREAM>(up, 9, lane4), ld_plane<STREAM>(up, 10, lane4), ld_plane<STREAM>(up, 11, lane4));
            float4 pos, vel; unsigned long long pm; uint32_t pb;
            if (K == 1 || j == 0) { pos = hp0; vel = hv0; pm = pm0; pb = pb0; }
            else if (K == 2 || j == 1) { pos = hp1; vel = hv1; pm = pm1; pb = pb1; }
            else if (j == 2) { pos = hp2; vel = hv2; pm = pm2; pb = pb2; }
            else { pos = hp3; vel = hv3; pm = pm3; pb = pb3; }
            if ((pm >> lane) & 1ull) {
                const uint32_t e = pb + (uint32_t)__popcll(pm & lanes_below);
                pos = mk4(parked.px[e], parked.py[e], parked.pz[e], parked.life[e]);
                vel = mk4(parked.vx[e], parked.vy[e], parked.vz[e], parked.ct[e]);
            }
            const int first = seg * 64;
            const int row = first >> a.cs_shift;
            const float fx = (float)(first - (row << a.cs_shift) + (int)lane), fy = (float)row;
            float4 rc = zero, rd = zero;
            if (__ballot(pos.w > 0.0f) != 0ull)
                render_data(fx, fy, pos, vel, attr, a.sys, a.update, a.bezier_codes, a.update_bits, nullptr, 0, 0, rc, rd);
            st_plane<STREAM>(up, 0, lane4, pos.x); st_plane<STREAM>(up, 1, lane4, pos.y); st_plane<STREAM>(up, 2, lane4, pos.z); st_plane<STREAM>(up, 3, lane4, pos.w);
            st_plane<STREAM>(up, 4, lane4, vel.x); st_plane<STREAM>(up, 5, lane4, vel.y); st_plane<STREAM>(up, 6, lane4, vel.z); st_plane<STREAM>(up, 7, lane4, vel.w);
            st_plane<STREAM>(up, 12, lane4, rc.x); st_plane<STREAM>(up, 13, lane4, rc.y); st_plane<STREAM>(up, 14, lane4, rc.z); st_plane<STREAM>(up, 15, lane4, rc.w);
            st_plane<STREAM>(up, 16, lane4, rd.x); st_plane<STREAM>(up, 17, lane4, rd.y); st_plane<STREAM>(up, 18, lane4, rd.z); st_plane<STREAM>(up, 19, lane4, rd.w);
            n_live += (uint32_t)__popcll(__ballot(pos.w > 0.0f));
        }
    }
    if ((__builtin_amdgcn_readfirstlane(g_step_count_sdf_samples) != 0) && (sdf_samples != 0))
        atomicAdd(&g_step_sdf_samples, (unsigned long long)sdf_samples);
    if (a.flags & ILM_STEP_COUNT_LIVE)
        publish_block_count(wave_live, n_live, lane, wave, v < a.total_units, a.first_chunk + (v >> a.upc_shift),
                            (v & ((1 << a.upc_shift) - 1)) / kUnitsPerBlock, (1 << a.upc_shift) / kUnitsPerBlock, a.count_buckets,
                            a.live_counts, a.zero_counts, a.zero_n, a.host_counts, a.count_seq);
}

// LeanStep from a StepLaunch whose launch_step fields are filled; false when the step is not of the lean shape
static bool build_lean_step(const StepLaunch& a, LeanStep& f) {
    const IlmStepDesc& d = a.desc;
    if (d.UpdateMode != ILM_UPDATE_POSITIONS && d.UpdateMode != ILM_UPDATE_WITH_DISTANCE_FIELD) return false;   // (the collision update: launch_lean_df_step adds the field)
    // power-of-two chunk size >= 64: no stride padding, a unit lies in one row, and units_per_chunk is a power of two >= 64, so every
    // block size of the lean kernels (kStepThreads / 64 x K units, K <= 4) divides it
    if (a.derived.cs_shift < 6 || a.upc_shift < 0) return false;
    if (a.slots != a.span) return false;
    if (a.derived.noise_may_revive != 0) return false;
    if (a.derived.update_bits & 1u) return false;                                   // life ramp
    if (a.op_mask & ~((1u << ILM_OP_GRAVITY) | (1u << ILM_OP_NOISE) | (1u << ILM_OP_FMA))) return false;
    memset(&f, 0, sizeof(f));
    for (int o = 0; o < d.OpCount; o++) {
        const IlmTransformOp& op = d.Ops[o];
        f.op_type[o] = op.Type;
        f.dop[o] = a.derived.op[o];
        if (op.Type == ILM_OP_GRAVITY) {
            const IlmGravityParams& g = op.u.Gravity;
            if (g.AttractorCount > kLeanMaxAttractors) return false;
            LeanGravity& l = f.op[o].gravity;
            l.count = g.AttractorCount < 0 ? 0 : g.AttractorCount;
            l.max_accel = a.derived.op[o].max_accel;
            l.cat_lo = g.CategoryFilter[0]; l.cat_hi = g.CategoryFilter[1];
            l.types = 0;
            for (int i = 0; i < l.count; i++) {
                l.a[i].x = g.AttractorPositions[i][0]; l.a[i].y = g.AttractorPositions[i][1]; l.a[i].z = g.AttractorPositions[i][2];
                l.a[i].radius = g.AttractorRadiusesAndStrengths[i][0];
                l.a[i].strength = g.AttractorRadiusesAndStrengths[i][1];
                const float type = g.AttractorRadiusesAndStrengths[i][2];
                l.types |= ((type >= 1.5f) ? 2u : ((type >= 0.5f) ? 1u : 0u)) << (2 * i);
            }
        } else if (op.Type == ILM_OP_NOISE) {
            // the per-slot form of evaluateByTypeId stays with the interpreter; a second Noise op has no uniform deltas
            if (!a.derived.op[o].area_none || a.derived.noise.op != o) return false;
            f.op[o].noise = op.u.Noise;
        } else {
            if (!a.derived.op[o].area_none) return false;
            f.op[o].fma = op.u.FMA;
        }
    }
    // The regular waves of the clamp class: a category passes every transform's filter exactly when it lies in their intersection (a
    // NaN bound fails every category, like the shader's comparisons); without a transform any category that is no NaN passes.
    float cat_lo = -INFINITY, cat_hi = INFINITY;
    for (int o = 0; o < d.OpCount; o++) {
        const IlmTransformOp& op = d.Ops[o];
        const float* mm = (op.Type == ILM_OP_GRAVITY) ? op.u.Gravity.CategoryFilter : (op.Type == ILM_OP_NOISE) ? op.u.Noise.Area.CategoryFilter : op.u.FMA.Area.CategoryFilter;
        if (std::isnan(mm[0]) || std::isnan(mm[1])) cat_lo = NAN;
        cat_lo = (mm[0] > cat_lo) ? mm[0] : cat_lo;     // (a NaN cat_lo stays)
        cat_hi = (mm[1] < cat_hi) ? mm[1] : cat_hi;
    }
    f.regular_cat_lo = cat_lo; f.regular_cat_hi = cat_hi;
    // rd.y = rotation x getVelocityRotation() + (life x RotationFromLifeAndIndex[0] + index x [1]): with a zero factor, a finite life
    // contributes the same +-0 whatever it is (the shader's own comparison: update_bits bit 1 is `== 0.0f` likewise).  Only with a finite
    // index factor: rd.y is then no NaN (the index is finite), so the bit never rests on what NaN an earlier writer left in the plane --
    // a NaN rd.y keeps both evaluations and the store the selecting tail gives it.
    f.elide = (d.Update.RotationFromLifeAndIndex[0] == 0.0f && std::isfinite(d.Update.RotationFromLifeAndIndex[1]) && (a.derived.update_bits & 2u)) ? kElideRotation : 0u;
    f.op_count = d.OpCount;
    f.noise_op = a.derived.noise.op;
    f.noise = a.derived.noise;
    f.spawn_count = 0;
    for (int s = 0; s < ILM_MAX_SPAWNS; s++) { f.spawn_chunk[s] = -1; f.spawn_unit_lo[s] = 1; f.spawn_unit_hi[s] = 0; }
    for (int s = 0; s < d.SpawnCount; s++) {
        const IlmSpawnRecord& r = d.Spawns[s];
        if (r.Kind != ILM_SPAWN_INLINE) return false;
        f.spawns[s] = r;
        f.spawn_chunk[s] = r.ChunkIndex;
        const float first = r.Params.ChunkSizeAndIndices[1], last = r.Params.ChunkSizeAndIndices[2];
        if (last >= first && last >= 0.0f) {      // (a NaN bound compares false: no lane can pass the per-lane test either)
            const double lo = first < 0.0f ? 0.0 : std::floor((double)first), hi = std::floor((double)last);
            const double max_unit = (double)(a.units_per_chunk - 1);
            f.spawn_unit_lo[s] = (int32_t)std::fmin(lo / 64.0, max_unit + 1.0);
            f.spawn_unit_hi[s] = (int32_t)std::fmin(hi / 64.0, max_unit);
        }
        f.spawn_count = s + 1;
    }
    if (d.SpawnCount == 0 && a.derived.noise.op >= 0 && a.derived.noise.classes == kNoiseBigClasses)
        memcpy(f.noise_big, &d.Spawns[0], sizeof(f.noise_big));       // fill_noise_fast put the 5 x 5 tables there
    f.chunk_bases = a.chunk_bases;
    f.live_counts = a.live_counts; f.zero_counts = a.zero_counts; f.zero_n = a.zero_n; f.host_counts = a.host_counts; f.count_seq = a.count_seq; f.count_buckets = a.count_buckets;
    f.stride = a.stride;
    f.upc_shift = a.upc_shift; f.unit_rotate = a.unit_rotate; f.total_padded = a.total_padded; f.total_units = a.unit_end - a.unit_begin;
    f.first_chunk = a.first_chunk; f.cs_shift = a.derived.cs_shift; f.flags = d.Flags;
    f.partial_count = a.partial_count;
    for (int k = 0; k < kMaxPartialChunks; k++) {
        f.partial_chunk[k] = (k < a.partial_count) ? a.partial_chunk[k] : -1;
        f.partial_units[k] = (k < a.partial_count) ? a.partial_units[k] : 0;
    }
    f.dt_s = a.derived.dt_s; f.bezier_codes = a.derived.bezier_codes; f.update_bits = a.derived.update_bits;
    f.sys = d.System; f.update = d.Update;
    f.rnd = a.rnd; f.rw = a.rw; f.rh = a.rh; f.inv_rw = a.derived.inv_rw; f.inv_rh = a.derived.inv_rh;
    return true;
}

// kElideColor: every point of the two colour curves is finite and at most 2^60 in magnitude, so each curve's value is finite (|t| <= 16
// for every range and shaping mode: < 2^76) and the colour factor renderColor is formed from is never a NaN.  A NaN in renderColor then
// comes from one attribute or is the default NaN of 0 x inf, so equal factors and unchanged attributes give the same bits, NaN payloads
// included.
static bool color_curves_bounded(const IlmUpdateParams& u) {
    for (const IlmClampedBezier4* b : { &u.ColorFromLife, &u.ColorFromVelocity })
        for (const IlmFloat4* q : { &b->A, &b->B, &b->C, &b->D })
            for (const float x : { q->x, q->y, q->z, q->w })
                if (!(std::fabs(x) <= 0x1p60f)) return false;
    return true;
}

// Which kernel the process's latest launch_step ran (ilm_debug_last_step_kernel): a diagnostic, like g_step_interpreter below.
static std::atomic<int> g_last_step_kernel{ILM_STEP_KERNEL_NONE};
int last_step_kernel() { return g_last_step_kernel; }

// kCurvesClamp's rule (see the constants): a streaming launch without spawners that elides, whose curves all have the clamp range and no
// shaping, with no velocity rotation and no life ramp.  Everything else runs the general instantiation.
static bool curves_clamp(const LeanStep& f, bool spawning, bool streaming) {
    return streaming && !spawning && (f.elide & kElideDerived) != 0u && (f.bezier_codes & ~kClampCodes) == 0u && f.update_bits == 2u;
}

// The category record of chunks [first_chunk, first_chunk + gridDim.y): {lo, hi} = the smallest and the largest category (plane 7) among
// the chunk's first `used` slots -- the slots past them were never written and are never stepped -- into floats 0 and 1 of the chunk's
// record; a NaN lo (which contains nobody) when one of them is a NaN.  A thread reads four slots at a time, 64 times; a wave reduces
// by shuffles, thread 0 combines the block's four waves and folds them into words 4..6 of the record -- integer maxima over keys that
// order like the floats (word 4 holds the complement of the smallest key, so the words start from zero) -- and the block that draws
// the last ticket (word 7) turns the keys back into floats and zeroes the words for the next scan.  One scan per chunk at a time
// (launch_step: on the stream that steps the chunk).  Few, long blocks: the records lie side by side, their atomics queue on one memory
// channel at some 20 ns each, and with 4 096 slots per block they were the whole of the kernel's time (32 chunks of 1024^2: 0.69 ms for
// 134 MB).
constexpr int kCategoryScanSlots = 65536;     // per block
ILM_DEV uint32_t float_order_key(float v) {
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
ILM_DEV float float_of_order_key(uint32_t k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__global__ __launch_bounds__(256) void category_bounds_kernel(float* const* __restrict__ bases, int64_t stride, int first_chunk, int used, float* __restrict__ records) {
    __shared__ float wave_lo[4], wave_hi[4];
    __shared__ uint32_t wave_nan[4];
    const int chunk = first_chunk + (int)blockIdx.y;
    const float* cat = bases[chunk] + 7 * stride;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    bool nan = false;
#pragma unroll 4
    for (int k = 0; k < kCategoryScanSlots / 1024; k++) {
        // i0 < used <= stride, i0 and the stride multiples of four: the four slots lie inside the plane; the slots at and past `used` are
        // read and left out below
        const int i0 = (int)blockIdx.x * kCategoryScanSlots + k * 1024 + (int)threadIdx.x * 4;
        if (i0 < used) {
            const float4 c = *reinterpret_cast<const float4*>(cat + i0);
            const float v[4] = { c.x, c.y, c.z, c.w };
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (i0 + j < used) {
                    lo = fminf(lo, v[j]); hi = fmaxf(hi, v[j]);      // (a NaN leaves both alone)
                    nan = nan || (v[j] != v[j]);
                }
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, d));
        hi = fmaxf(hi, __shfl_xor(hi, d));
    }
    const bool wave_has_nan = __ballot(nan) != 0ull;
    if ((threadIdx.x & 63) == 0) { wave_lo[threadIdx.x >> 6] = lo; wave_hi[threadIdx.x >> 6] = hi; wave_nan[threadIdx.x >> 6] = wave_has_nan ? 1u : 0u; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(wave_lo[0], wave_lo[1]), fminf(wave_lo[2], wave_lo[3]));
        hi = fmaxf(fmaxf(wave_hi[0], wave_hi[1]), fmaxf(wave_hi[2], wave_hi[3]));
        float* rec = records + (size_t)chunk * kCategoryRecordStride;
        uint32_t* work = reinterpret_cast<uint32_t*>(rec) + 4;
        atomicMax(&work[0], ~float_order_key(lo));
        atomicMax(&work[1], float_order_key(hi));
        if ((wave_nan[0] | wave_nan[1] | wave_nan[2] | wave_nan[3]) != 0u) atomicOr(&work[2], 1u);
        __threadfence();
        if (atomicAdd(&work[3], 1u) == gridDim.x - 1u) {
            __threadfence();
            const uint32_t k_lo = ~atomicOr(&work[0], 0u), k_hi = atomicOr(&work[1], 0u), any_nan = atomicOr(&work[2], 0u);
            rec[0] = any_nan ? __builtin_nanf("") : float_of_order_key(k_lo);
            rec[1] = float_of_order_key(k_hi);
            work[0] = 0u; work[1] = 0u; work[2] = 0u; work[3] = 0u;
        }
    }
}
static hipError_t launch_category_bounds(float* const* chunk_bases, int64_t stride, int first_chunk, int chunk_count, int used, float* records, hipStream_t stream) {
    const unsigned blocks = (unsigned)std::max(1, (used + kCategoryScanSlots - 1) / kCategoryScanSlots);
    hipLaunchKernelGGL(category_bounds_kernel, dim3(blocks, (unsigned)chunk_count), dim3(256), 0, stream, chunk_bases, stride, first_chunk, used, records);
    return hipGetLastError();
}
// g_no_category_record on the current device (looked up once per device)
static const float* no_category_record() {
    constexpr int kDevices = 64;
    static std::atomic<const float*> found[kDevices];
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess || device < 0 || device >= kDevices) { (void)hipGetLastError(); return nullptr; }
    const float* p = found[device];
    if (p == nullptr) {
        void* address = nullptr;
        if (hipGetSymbolAddress(&address, HIP_SYMBOL(g_no_category_record)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        found[device] = p = static_cast<const float*>(address);
    }
    return p;
}
// The scans a clamp-class launch needs: every chunk of its range whose record is not current, one launch per run of consecutive such
// chunks with the same number of used slots, on the launch's stream ahead of it.
static hipError_t scan_category_records(const StepLaunch& a, CategoryRecords& cat, hipStream_t stream) {
    const int end = a.first_chunk + a.chunk_count;
    for (int ci = a.first_chunk; ci < end;) {
        if (cat.current[ci]) { ci++; continue; }
        int run = 1;
        while (ci + run < end && !cat.current[ci + run] && cat.used[ci + run] == cat.used[ci]) run++;
        const hipError_t e = launch_category_bounds(a.chunk_bases, a.stride, ci, run, std::min(cat.used[ci], a.slots), cat.table, stream);
        if (e != hipSuccess) return e;
        for (int k = 0; k < run; k++) cat.current[ci + k] = 1;
        ci += run;
    }
    return hipSuccess;
}

static hipError_t launch_lean_step(const LeanStep& f, bool spawning, bool streaming, hipStream_t stream) {
    const int units_per_block = kStepThreads / 64;
    const dim3 grid((unsigned)((f.total_units + units_per_block - 1) / units_per_block), 1, 1), block(kStepThreads, 1, 1);
    const bool clamp = curves_clamp(f, spawning, streaming);
    if (spawning) {
        if (streaming) hipLaunchKernelGGL((step_lean_kernel<true, true>), grid, block, 0, stream, f);
        else hipLaunchKernelGGL((step_lean_kernel<true, false>), grid, block, 0, stream, f);
    } else {
        if (clamp) hipLaunchKernelGGL(step_lean_clamp_kernel, grid, block, 0, stream, f);
        else if (streaming) hipLaunchKernelGGL((step_lean_kernel<false, true>), grid, block, 0, stream, f);
        else hipLaunchKernelGGL((step_lean_kernel<false, false>), grid, block, 0, stream, f);
    }
    g_last_step_kernel = clamp ? ILM_STEP_KERNEL_LEAN_CLAMP : ILM_STEP_KERNEL_LEAN;
    return hipGetLastError();
}

// The collision kernels' first template argument: the field's format, plus kFieldSlice0 when the uniforms put every lookup in virtual
// slice 0 with a z weight of 0 (hlsl_math.hpp sample_distance_field<.., SLICE0>) -- what the reference's particle path binds.
constexpr int kFieldSlice0 = 2;
constexpr int kFieldCells0 = 4;      // ... plus the slice-0 cells (SdfView::cells0): one load per lookup (lean collision kernel only)
static_assert((ILM_SDF_UNORM16 | ILM_SDF_FP16) == 1, "the format is bit 0 of the collision kernels' first template argument");
// The slice-0 sampler returns the bilinear fetch of channel r where the general one forms lerp(lo, hi, 0) = fma(0, hi - lo, lo): equal
// for FINITE texels only, so it serves UNORM16 fields (every code is finite); an FP16 atlas uploaded through ilm_sdf_upload may hold
// inf / NaN (hi = inf gives NaN in the general form and in the oracle) and keeps the general sampler.  The uniforms whose fma(0, ., .)
// terms the slice-0 form drops (Packed1.x, .z, TextureSliceAndTexelSize.xy) must be finite for the same reason.
static bool field_is_slice0(const IlmDistanceFieldUniforms& df, int format) {
    return (format == ILM_SDF_UNORM16) && (df.Packed1.y == 0.0f) && std::isfinite(df.Packed1.x) && std::isfinite(df.Packed1.z) &&
           std::isfinite(df.TextureSliceAndTexelSize.x) && std::isfinite(df.TextureSliceAndTexelSize.y);
}
// A launch's field as the collision kernels' first template argument: launch(std::integral_constant<int, FMT>()).  CELLS: the caller
// has kernels for kFieldCells0 (the lean collision kernel; the interpreter has none, and none is instantiated for it).
template <bool CELLS, class Launch>
static hipError_t with_field_format(const StepLaunch& a, Launch launch) {
    int fmt = (int)a.sdf.format | (field_is_slice0(a.desc.DistanceField, (int)a.sdf.format) ? kFieldSlice0 : 0);
    if (CELLS && fmt == (ILM_SDF_UNORM16 | kFieldSlice0) && a.sdf.cells0 != nullptr) fmt |= kFieldCells0;
    switch (fmt) {
        case ILM_SDF_UNORM16: return launch(std::integral_constant<int, ILM_SDF_UNORM16>());
        case ILM_SDF_FP16: return launch(std::integral_constant<int, ILM_SDF_FP16>());
        case ILM_SDF_UNORM16 | kFieldSlice0: return launch(std::integral_constant<int, ILM_SDF_UNORM16 | kFieldSlice0>());
        case ILM_SDF_FP16 | kFieldSlice0: return launch(std::integral_constant<int, ILM_SDF_FP16 | kFieldSlice0>());
        case ILM_SDF_UNORM16 | kFieldSlice0 | kFieldCells0:
            if constexpr (CELLS) return launch(std::integral_constant<int, ILM_SDF_UNORM16 | kFieldSlice0 | kFieldCells0>());
    }
    return hipErrorInvalidValue;      // (no field is created with another format)
}
// The block lay-out of a launch whose blocks hold `upb` units (upb divides units_per_chunk): the padded unit count the rotation wraps
// at, the rotation rounded down to a block, the live-count buckets of a chunk (publish_block_count)
struct BlockLayout { int total_padded, unit_rotate, count_buckets; };
static BlockLayout block_layout(int total_units, int unit_rotate, int units_per_chunk, int upb) {
    BlockLayout l;
    l.total_padded = (total_units + upb - 1) / upb * upb;
    l.unit_rotate = unit_rotate / upb * upb;
    l.count_buckets = 1;
    while (l.count_buckets * 2 <= kCountLines - 1 && (units_per_chunk / upb) % (l.count_buckets * 2) == 0) l.count_buckets *= 2;
    return l;
}
// SdfView::cells0 from the atlas: cell (x0, yr) = channel r of the taps (x0, y0), (x1, y0), (x0, y1), (x1, y1) of a bilinear fetch whose
// upper-left tap is column x0 (already wrapped) of row yi = yr - 1 -- x1 = x0 + 1 with U WRAP, y0 = clamp(yi), y1 = the next row exactly
// when 0 <= yi < height - 1: the integer bookkeeping of sample_distance_field, done once per texel instead of once per lookup.
__global__ __launch_bounds__(256) void build_slice0_cells_kernel(const uint2* __restrict__ texels, int width, int height, uint2* __restrict__ cells) {
    const int x0 = (int)blockIdx.x * 256 + (int)threadIdx.x, yr = (int)blockIdx.y;
    if (x0 >= width) return;
    const int yi = yr - 1;
    const int y0 = min(max(yi, 0), height - 1);
    const int y1 = ((uint32_t)yi < (uint32_t)(height - 1)) ? y0 + 1 : y0;
    const int x1 = (x0 + 1 == width) ? 0 : x0 + 1;
    const uint32_t r00 = texels[(size_t)y0 * width + x0].x & 0xFFFFu, r10 = texels[(size_t)y0 * width + x1].x & 0xFFFFu;
    const uint32_t r01 = texels[(size_t)y1 * width + x0].x & 0xFFFFu, r11 = texels[(size_t)y1 * width + x1].x & 0xFFFFu;
    cells[(size_t)yr * width + x0] = make_uint2(r00 | (r10 << 16), r01 | (r11 << 16));
}
hipError_t launch_build_slice0_cells(const uint2* texels, int width, int height, void* cells, hipStream_t stream) {
    hipLaunchKernelGGL(build_slice0_cells_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)(height + 1)), dim3(256), 0, stream, texels, width, height, static_cast<uint2*>(cells));
    return hipGetLastError();
}
static bool step_interpreter_forced();
bool step_wants_slice0_cells(const IlmStepDesc& d, int format) {
    const char* e = getenv("ILM_DF_CELLS0");            // A/B switch, read per step: 0 = the four-tap form
    if (e && atoi(e) == 0) return false;
    const char* lean = getenv("ILM_DF_LEAN");
    if ((lean && atoi(lean) == 0) || step_interpreter_forced()) return false;
    if (!(d.UpdateMode == ILM_UPDATE_WITH_DISTANCE_FIELD && format == ILM_SDF_UNORM16 && field_is_slice0(d.DistanceField, format))) return false;
    // A cell row is yi + 1 with no clamp (hlsl_math.hpp), and the array has rows 0 .. height: only uniforms that keep every v in [0, 1]
    // may use it.  cy is in [0, Extent.y] and fl(cy * TexelSize.w) is monotone in cy, so v <= fl(Extent.y * TexelSize.w) -- the product
    // the device forms, in fp32 -- and -1 <= yi <= height - 1.  Any other uniforms (V past the atlas, a negative or non-finite texel
    // size) take the four-tap form, which clamps V like the reference's sampler.
    const float ey = d.DistanceField.Extent.y, tw = d.DistanceField.TextureSliceAndTexelSize.w;
    const float v_max = ey * tw;
    return std::isfinite(ey) && std::isfinite(tw) && std::isfinite(v_max) && ey >= 0.0f && tw >= 0.0f && v_max <= 1.0f;
}

// The lean collision step.  K = units per wave: the more units a wave walks, the fuller its long passes run -- and the longer it lives, so
// a launch of few waves (cfg2: 16 384 units) takes the smaller K (tools/ab_collision.sh; ILM_DF_UNITS overrides).
template <int FMT, bool SPAWN>
static hipError_t launch_lean_df_variant(const LeanStepDf& f, int k, bool streaming, const dim3& grid, hipStream_t stream) {
    const dim3 block(kStepThreads, 1, 1);
    if (streaming) hipLaunchKernelGGL((step_lean_df_kernel<FMT, SPAWN, true, 4>), grid, block, 0, stream, f);
    else if (k == 4) hipLaunchKernelGGL((step_lean_df_kernel<FMT, SPAWN, false, 4>), grid, block, 0, stream, f);
    else if (k == 2) hipLaunchKernelGGL((step_lean_df_kernel<FMT, SPAWN, false, 2>), grid, block, 0, stream, f);
    else hipLaunchKernelGGL((step_lean_df_kernel<FMT, SPAWN, false, 1>), grid, block, 0, stream, f);
    return hipGetLastError();
}
static hipError_t launch_lean_df_step(LeanStepDf& f, const StepLaunch& a, bool spawning, hipStream_t stream) {
    const char* forced_env = getenv("ILM_DF_UNITS");                  // (read per launch: an A/B and test switch)
    const int forced_k = forced_env ? atoi(forced_env) : 0;
    const bool streaming = a.streaming != 0;
    int k = (forced_k == 1 || forced_k == 2 || forced_k == 4) ? forced_k : ((f.base.total_units >= 65536) ? 4 : 2);
    if (streaming) k = 4;
    const int upb = (kStepThreads / 64) * k;                            // units per block: divides units_per_chunk (build_lean_step)
    // the grid's bookkeeping for blocks of upb units (launch_step laid it out for blocks of kStepThreads / 64)
    const BlockLayout l = block_layout(f.base.total_units, f.base.unit_rotate, a.units_per_chunk, upb);
    f.base.total_padded = l.total_padded; f.base.unit_rotate = l.unit_rotate; f.base.count_buckets = l.count_buckets;
    const dim3 grid((unsigned)(l.total_padded / upb), 1, 1);
    return with_field_format<true>(a, [&](auto fmt) {
        return spawning ? launch_lean_df_variant<decltype(fmt)::value, true>(f, k, streaming, grid, stream) : launch_lean_df_variant<decltype(fmt)::value, false>(f, k, streaming, grid, stream);
    });
}

// The extended variant carries the rarely used techniques (MatrixMultiply, SpatialNoise, the position-buffer and feedback spawners) so
// that the common variants do not pay their registers; it is always the spawning superset.
static bool needs_extended_variant(const StepLaunch& a) {
    if (a.op_mask & ((1u << ILM_OP_MATRIX_MULTIPLY) | (1u << ILM_OP_SPATIAL_NOISE))) return true;
    for (int s = 0; s < a.desc.SpawnCount; s++)
        if (a.desc.Spawns[s].Kind != ILM_SPAWN_INLINE) return true;
    return false;
}

// Collision variants: six waves per SIMD (79 VGPRs, no scratch) 37.5-38.3 us on bench.py's collision row against 38.6-39.4 for the
// allocator's own 86 VGPRs / five waves; seven (72 VGPRs, 24 B of scratch) 44.4, eight (64 VGPRs, 76 B) 55.2 (tools/ab_collision.sh)
constexpr int kDfMinWaves = 6;
template <bool SPAWN>
static hipError_t launch_step_variant(const StepLaunch& a, hipStream_t stream) {
    const int units = a.unit_end - a.unit_begin;
    if (units <= 0) return hipSuccess;
    const int units_per_block = kStepThreads / 64;
    const dim3 grid((unsigned)((units + units_per_block - 1) / units_per_block), 1, 1), block(kStepThreads, 1, 1);
    const bool df = a.desc.UpdateMode == ILM_UPDATE_WITH_DISTANCE_FIELD;
    if (needs_extended_variant(a)) {
        if (df)
            return with_field_format<false>(a, [&](auto fmt) {
                hipLaunchKernelGGL((step_kernel<decltype(fmt)::value, true, true, 1, true>), grid, block, 0, stream, a);
                return hipGetLastError();
            });
        hipLaunchKernelGGL((step_kernel<ILM_SDF_UNORM16, false, true, 1, true>), grid, block, 0, stream, a);
    } else if (df) {
        // waves per SIMD requested for the collision variants (kDfMinWaves; measured in docs/experiments.md 3.1)
        return with_field_format<false>(a, [&](auto fmt) {
            hipLaunchKernelGGL((step_kernel<decltype(fmt)::value, true, SPAWN, kDfMinWaves>), grid, block, 0, stream, a);
            return hipGetLastError();
        });
    } else if (a.streaming) {
        hipLaunchKernelGGL((step_kernel<ILM_SDF_UNORM16, false, SPAWN, 1, false, true>), grid, block, 0, stream, a);
    } else {
        // (bounding this variant to 7 / 8 waves per SIMD -- 72 / 64 VGPRs with 8 / 24 bytes of scratch in the cold spawn path --
        // measured 3.5 % / 14 % SLOWER on cfg2: the step is VALU-issue-bound, not occupancy-bound; DESIGN.md "experiments")
        hipLaunchKernelGGL((step_kernel<ILM_SDF_UNORM16, false, SPAWN, 1>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

static std::atomic<int> g_step_interpreter{-1};      // (atomic: a process-wide switch read by every stepping thread)  -1: not decided yet (ILM_STEP_LEAN), 0: lean kernel where it applies, 1: interpreter always
static bool step_interpreter_forced() {
    if (g_step_interpreter < 0) {
        const char* e = getenv("ILM_STEP_LEAN");
        g_step_interpreter = (e && atoi(e) == 0) ? 1 : 0;
    }
    return g_step_interpreter != 0;
}
int set_step_interpreter(int on) {
    const int before = step_interpreter_forced() ? 1 : 0;
    g_step_interpreter = on ? 1 : 0;
    return before;
}

// One launch per ParticleSystem.Update: the unit range covers every chunk of the step; when spawn records are
// present the SPAWN variant runs (for every unit) and the grid is rotated to start at the first spawn range.
// The launch's unit range and block lay-out (the StepLaunch fields "filled by launch_step"); true when spawn records apply to the range.
static bool layout_step(StepLaunch& a) {
    a.units_per_chunk = a.span / 64;
    a.upc_shift = -1;
    for (int b = 0; b < 31; b++)
        if ((1 << b) == a.units_per_chunk) a.upc_shift = b;
    a.unit_begin = 0;
    a.unit_end = a.chunk_count * a.units_per_chunk;
    int first_spawn_unit = 0;
    bool spawning = false;
    for (int s = 0; s < a.desc.SpawnCount; s++) {
        const IlmSpawnRecord& r = a.desc.Spawns[s];
        if (r.ChunkIndex < a.first_chunk || r.ChunkIndex >= a.first_chunk + a.chunk_count)
            continue;
        if (r.Params.ChunkSizeAndIndices[2] < r.Params.ChunkSizeAndIndices[1])
            continue;
        if (!spawning)
            first_spawn_unit = (r.ChunkIndex - a.first_chunk) * a.units_per_chunk + (int)r.Params.ChunkSizeAndIndices[1] / 64;
        spawning = true;
    }
    const BlockLayout l = block_layout(a.unit_end, first_spawn_unit, a.units_per_chunk, kStepThreads / 64);
    a.total_padded = l.total_padded; a.unit_rotate = l.unit_rotate; a.count_buckets = l.count_buckets;
    return spawning;
}
// The category records of the launch's range (api.hip, System::cat_current).  A record stays current through a lean step that runs
// neither an FMA nor a spawner: Gravity, Noise and the update pass hand a live slot's category through, and a slot they discard gets
// its zero category together with a zero life.  Every other kernel may write a live slot's category: its range's records are cleared.
// The clamp class is the one reader: a launch of it without an FMA scans what is not current and takes the table along.
static void clear_category_records(const StepLaunch& a, CategoryRecords* cat) {
    for (int ci = a.first_chunk; cat && ci < a.first_chunk + a.chunk_count; ci++) cat->current[ci] = 0;
}
hipError_t launch_step(StepLaunch& a, hipStream_t stream, uint32_t render_elide, bool* refreshed, CategoryRecords* cat) {
    if (refreshed) *refreshed = false;
    const bool spawning = layout_step(a);
    if (spawning || (a.op_mask & (1u << ILM_OP_FMA)) != 0u) { clear_category_records(a, cat); cat = nullptr; }
    if (!step_interpreter_forced() && a.unit_end > a.unit_begin) {
        if (a.desc.UpdateMode == ILM_UPDATE_WITH_DISTANCE_FIELD) {
            const char* lean_env = getenv("ILM_DF_LEAN");                 // A/B switch, read per launch: 0 = the interpreter
            const bool lean_df = !(lean_env && atoi(lean_env) == 0);
            LeanStepDf f;
            if (lean_df && build_lean_step(a, f.base)) {
                f.df = a.desc.DistanceField;
                f.sdf = a.sdf;
                clear_category_records(a, cat);       // (the collision update redirects and parks slots: not checked against the record's rule)
                g_last_step_kernel = ILM_STEP_KERNEL_LEAN_DF;
                return launch_lean_df_step(f, a, spawning, stream);
            }
        } else {
            LeanStep f;
            if (build_lean_step(a, f)) {
                f.elide = ((render_elide & kElideDerived) && a.streaming) ? (kElideDerived | (color_curves_bounded(a.desc.Update) ? kElideColor : 0u) | (f.elide & kElideRotation)) : 0u;
                if (curves_clamp(f, spawning, a.streaming != 0)) {
                    if (cat) {
                        const hipError_t scanned = scan_category_records(a, *cat, stream);
                        if (scanned != hipSuccess) { clear_category_records(a, cat); return scanned; }
                        f.cat_bounds = cat->table; f.cat_stride = kCategoryRecordStride * (int32_t)sizeof(float);
                    } else {
                        f.cat_bounds = no_category_record(); f.cat_stride = 0;
                        if (f.cat_bounds == nullptr) return hipErrorInvalidSymbol;
                    }
                }
                const hipError_t e = launch_lean_step(f, spawning, a.streaming != 0, stream);
                if (refreshed) *refreshed = (e == hipSuccess);
                return e;
            }
        }
    }
    clear_category_records(a, cat);
    g_last_step_kernel = ILM_STEP_KERNEL_INTERPRETER;
    return spawning ? launch_step_variant<true>(a, stream) : launch_step_variant<false>(a, stream);
}

// The batch kernel's variants are launch_step_variant's without the streaming one.  Key: bits 0-1 = 0 plain, 1 spawning, 2 extended;
// bits 2.. = 0 without a field, else 1 + the collision kernels' first template argument (format | kFieldSlice0).
int step_batch_layout(StepLaunch& a, int* blocks) {
    const bool spawning = layout_step(a);
    const int units = a.unit_end - a.unit_begin;
    *blocks = (units + kStepThreads / 64 - 1) / (kStepThreads / 64);
    if (a.streaming || units <= 0) return -1;
    int field = 0;
    if (a.desc.UpdateMode == ILM_UPDATE_WITH_DISTANCE_FIELD) {
        if (with_field_format<false>(a, [&](auto fmt) { field = 1 + decltype(fmt)::value; return hipSuccess; }) != hipSuccess) return -1;
    }
    return (field << 2) | (needs_extended_variant(a) ? 2 : (spawning ? 1 : 0));
}
template <int FMT, bool DF>
static hipError_t launch_step_batch_variant(int kind, const StepBatchItem* table, const int32_t* item_of_block, const dim3& grid, hipStream_t stream) {
    const dim3 block(kStepThreads, 1, 1);
    constexpr int kMinWaves = DF ? kDfMinWaves : 1;
    if (kind == 2) hipLaunchKernelGGL((step_batch_kernel<FMT, DF, true, 1, true>), grid, block, 0, stream, table, item_of_block);
    else if (kind == 1) hipLaunchKernelGGL((step_batch_kernel<FMT, DF, true, kMinWaves>), grid, block, 0, stream, table, item_of_block);
    else hipLaunchKernelGGL((step_batch_kernel<FMT, DF, false, kMinWaves>), grid, block, 0, stream, table, item_of_block);
    return hipGetLastError();
}
hipError_t launch_step_batch(int variant, const StepBatchItem* table, const int32_t* item_of_block, int blocks, hipStream_t stream) {
    if (blocks <= 0) return hipSuccess;
    const dim3 grid((unsigned)blocks, 1, 1);
    const int kind = variant & 3;
    g_last_step_kernel = ILM_STEP_KERNEL_BATCH;
    switch (variant >> 2) {
        case 0: return launch_step_batch_variant<ILM_SDF_UNORM16, false>(kind, table, item_of_block, grid, stream);
        case 1 + ILM_SDF_UNORM16: return launch_step_batch_variant<ILM_SDF_UNORM16, true>(kind, table, item_of_block, grid, stream);
        case 1 + ILM_SDF_FP16: return launch_step_batch_variant<ILM_SDF_FP16, true>(kind, table, item_of_block, grid, stream);
        case 1 + (ILM_SDF_UNORM16 | kFieldSlice0): return launch_step_batch_variant<ILM_SDF_UNORM16 | kFieldSlice0, true>(kind, table, item_of_block, grid, stream);
        case 1 + (ILM_SDF_FP16 | kFieldSlice0): return launch_step_batch_variant<ILM_SDF_FP16 | kFieldSlice0, true>(kind, table, item_of_block, grid, stream);
    }
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
// layout conversion: the reference API speaks AoS float4 (Spawn initializers, AutoReadback)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aos_to_soa_kernel(const float4* __restrict__ src, float* __restrict__ plane0, int64_t stride,
                                                          int first_slot, int count) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= count) return;
    const float4 v = src[i];
    float* p = plane0 + first_slot + i;
    p[0] = v.x; p[stride] = v.y; p[2 * stride] = v.z; p[3 * stride] = v.w;
}
__global__ __launch_bounds__(256) void soa_to_aos_kernel(const float* __restrict__ plane0, int64_t stride, float4* __restrict__ dst,
                                                          int first_slot, int count) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= count) return;
    const float* p = plane0 + first_slot + i;
    dst[i] = mk4(p[0], p[stride], p[2 * stride], p[3 * stride]);
}
hipError_t launch_aos_to_soa(const float4* src, float* plane0, int64_t stride, int32_t first_slot, int32_t count, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(aos_to_soa_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, src, plane0, stride, first_slot, count);
    return hipGetLastError();
}
hipError_t launch_soa_to_aos(const float* plane0, int64_t stride, float4* dst, int32_t first_slot, int32_t count, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(soa_to_aos_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, plane0, stride, dst, first_slot, count);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// liveness: standalone count + ordered live-slot compaction
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void count_live_kernel(float* const* __restrict__ bases, int64_t stride, int slots, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wave_live[4];
    const int chunk = (int)blockIdx.y;
    const float* life = bases[chunk] + 3 * stride;
    const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
    const float4 l = *reinterpret_cast<const float4*>(life + i0);
    // only the chunk's ChunkSize^2 slots are particles: the padding up to the stride is not counted
    const uint32_t n = (uint32_t)__popcll(__ballot((i0 < slots) && (l.x > 0.0f))) + (uint32_t)__popcll(__ballot((i0 + 1 < slots) && (l.y > 0.0f))) +
                       (uint32_t)__popcll(__ballot((i0 + 2 < slots) && (l.z > 0.0f))) + (uint32_t)__popcll(__ballot((i0 + 3 < slots) && (l.w > 0.0f)));
    if ((threadIdx.x & 63) == 0) wave_live[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = wave_live[0] + wave_live[1] + wave_live[2] + wave_live[3];
        if (total != 0) atomicAdd(&counts[chunk * kCountStride], total);
    }
}
hipError_t launch_count_live(float* const* chunk_bases, int64_t stride, int32_t span, int32_t slots, int32_t chunk_count, uint32_t* counts, hipStream_t stream) {
    if (chunk_count <= 0) return hipSuccess;
    hipLaunchKernelGGL(count_live_kernel, dim3((unsigned)(span / 1024), (unsigned)chunk_count), dim3(256), 0, stream, chunk_bases, stride, slots, counts);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// sensors: the particles inside an area (PS_CollectParticles, CollectParticles.fx:10-38; Sensor, Transforms.cs:374-486)
// ---------------------------------------------------------------------------------------------
// The reference would count with an occlusion query: the pixels the shader does not discard.  A slot is kept when
//   checkCategoryFilter(velocity.w, CategoryFilter)                                                   (:22)
//   position.w > 1  -- life against ONE, as the text has it                                           (:32)
//   1 - saturate(evaluateByTypeId(AreaType, position, ...) / AreaFalloff) > 0.01                      (:27-32)
// which is count_live_kernel's reduction with a longer predicate.  One lane holds four consecutive slots, so a wave covers 256 and
// every load is 16 bytes per lane; the life and the category are read first and x, y, z only by a wave in which some slot has a
// life above one (20 bytes per slot at most, no other plane, no store to the state).  Every sensor of the launch is evaluated on
// the loaded slots (the parameters are kernel arguments: scalar loads), per sensor one ballot + popcount per slot column.
// A workgroup walks tiles_per_block consecutive 1 024-slot tiles of one chunk and keeps its waves' counts in LDS; at the end the
// four waves meet in LDS and the workgroup issues ONE atomic add per sensor, none for a sensor it counted nothing for, into a counter
// that has a 128-byte line of its own (kSenseStride).  Measured (tools/sensor_timing.py, docs/experiments.md 7.37): with one add per
// wave and 256 slots into counters packed side by side, the adds alone -- 32 768 per sensor on one line at cfg4's share -- took 128 us
// per sensor, five times the HBM floor of the whole pass.
// AREA = false: the host has seen that no sensor of the launch has an area (AreaType 0).  evaluateByTypeId then returns 0 and
// 1 - saturate(0 / falloff) is 1 for every finite falloff (0 / 0 = NaN, saturate(NaN) = 0, hlsl_math.hpp), so the third condition holds
// for every slot: the instantiation holds no distance code and loads no coordinate.
template <bool AREA>
__global__ __launch_bounds__(256) void sense_kernel(const SenseLaunch a) {
#pragma clang fp contract(off)
    __shared__ uint32_t wave_counts[4][ILM_MAX_SENSORS];
    const int chunk = (int)blockIdx.y;
    const float* base = a.chunk_bases[a.first_chunk + chunk];
    // a wave's counts, per sensor: touched by its first lane only until the workgroup meets (in LDS: the sensor loop stays a loop -- unrolled
    // for counters in registers, the eight sensors' arithmetic interleaves into 155 VGPRs and three waves per SIMD)
    if (threadIdx.x < 4 * ILM_MAX_SENSORS) (&wave_counts[0][0])[threadIdx.x] = 0u;
    __syncthreads();
    const bool lane0 = (threadIdx.x & 63) == 0;
    uint32_t* const counted = wave_counts[threadIdx.x >> 6];
    const int tile_end = min(((int)blockIdx.x + 1) * a.tiles_per_block, a.span / 1024);
    for (int tile = (int)blockIdx.x * a.tiles_per_block; tile < tile_end; tile++) {
        const int i0 = (tile * 256 + (int)threadIdx.x) * 4;      // < span <= stride: the planes are padded to whole tiles
        const float4 l4 = *reinterpret_cast<const float4*>(base + 3 * a.stride + i0);
        const float4 c4 = *reinterpret_cast<const float4*>(base + 7 * a.stride + i0);
        const float life[4] = { l4.x, l4.y, l4.z, l4.w }, cat[4] = { c4.x, c4.y, c4.z, c4.w };
        // only the chunk's ChunkSize^2 slots are particles: the padding up to the stride is not counted
        bool alive[4];
        bool any_alive = false;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            alive[j] = (i0 + j < a.slots) && (life[j] > 1.0f);
            any_alive = any_alive || alive[j];
        }
        if (__ballot(any_alive) == 0ull) continue;
        float x[4] = {}, y[4] = {}, z[4] = {};
        if (AREA) {
            const float4 x4 = *reinterpret_cast<const float4*>(base + i0);
            const float4 y4 = *reinterpret_cast<const float4*>(base + a.stride + i0);
            const float4 z4 = *reinterpret_cast<const float4*>(base + 2 * a.stride + i0);
            x[0] = x4.x; x[1] = x4.y; x[2] = x4.z; x[3] = x4.w;
            y[0] = y4.x; y[1] = y4.y; y[2] = y4.z; y[3] = y4.w;
            z[0] = z4.x; z[1] = z4.y; z[2] = z4.z; z[3] = z4.w;
        }
        for (int k = 0; k < a.sensor_count; k++) {
            const IlmAreaParams& s = a.sensors[k];
            bool pass[4];
            bool any = false;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                pass[j] = alive[j] && category_ok(cat[j], s.CategoryFilter);
                any = any || pass[j];
            }
            // a wave none of whose slots passes the filter and the life test skips the area
            if (__ballot(any) == 0ull) continue;
            if (AREA && s.AreaType != 0) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float distance = evaluate_area(s.AreaType, mk3(x[j], y[j], z[j]), s);
                    const float scaled = 1.0f - sat(distance / s.AreaFalloff);
                    pass[j] = pass[j] && (scaled > 0.01f);
                }
            }
            const uint32_t n = (uint32_t)__popcll(__ballot(pass[0])) + (uint32_t)__popcll(__ballot(pass[1])) +
                               (uint32_t)__popcll(__ballot(pass[2])) + (uint32_t)__popcll(__ballot(pass[3]));
            if (lane0 && n != 0u) counted[k] += n;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < a.sensor_count) {
        const int k = (int)threadIdx.x;
        const uint32_t total = wave_counts[0][k] + wave_counts[1][k] + wave_counts[2][k] + wave_counts[3][k];
        if (total != 0u) atomicAdd(&a.counts[((size_t)k * (size_t)a.chunk_count + (size_t)chunk) * kSenseStride], total);
    }
}
hipError_t launch_sense(SenseLaunch& a, hipStream_t stream) {
    if (a.chunk_count <= 0 || a.sensor_count <= 0) return hipSuccess;
    if (a.chunk_count > 65535 || a.sensor_count > ILM_MAX_SENSORS) return hipErrorInvalidValue;
    bool area = false;
    for (int k = 0; k < a.sensor_count; k++) area = area || (a.sensors[k].AreaType != 0);
    // enough workgroups to fill the device (about 2 048), then up to eight tiles each: fewer, fuller atomic adds
    const int tiles = a.span / 1024;
    const long long total_tiles = (long long)tiles * a.chunk_count;
    a.tiles_per_block = (int)std::min<long long>(8, std::max<long long>(1, total_tiles / 2048));
    const dim3 grid((unsigned)((tiles + a.tiles_per_block - 1) / a.tiles_per_block), (unsigned)a.chunk_count);
    if (area) hipLaunchKernelGGL(sense_kernel<true>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(sense_kernel<false>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

// Single workgroup of 1024 threads walks the chunk in 1024-slot tiles keeping a
// running base, so the output is in ascending slot order (deterministic):
// per-wave ballot -> popcount prefix inside the wave, LDS scan across the 16 waves.
// Two launches over 1024-slot blocks (r04; one workgroup used to walk the whole chunk, 64 rounds of three barriers for a 256^2 chunk:
// 97 us): the blocks' live counts, then every block adds the counts in front of it and writes its slots at that base -- ballot +
// popcount prefix inside the block, so the list is in slot order.
__global__ __launch_bounds__(1024) void live_slots_count_kernel(const float* __restrict__ life, int slots, uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t wave_counts[16];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int i = (int)blockIdx.x * 1024 + (int)threadIdx.x;
    const bool alive = (i < slots) && (life[i] > 0.0f);
    const unsigned long long mask = __ballot(alive);
    if (lane == 0) wave_counts[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < 16; w++) t += wave_counts[w];
        block_counts[blockIdx.x] = t;
    }
}
__global__ __launch_bounds__(1024) void live_slots_emit_kernel(const float* __restrict__ life, int slots, const uint32_t* __restrict__ block_counts,
                                                                uint32_t* __restrict__ out, uint32_t capacity, uint32_t* __restrict__ out_count) {
    __shared__ uint32_t wave_counts[16];
    __shared__ uint32_t partial[16];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    // the live slots in the blocks in front of this one
    uint32_t before = 0;
    for (int b = (int)threadIdx.x; b < (int)blockIdx.x; b += 1024) before += block_counts[b];
    for (int off = 32; off > 0; off >>= 1) before += __shfl_down(before, off);
    if (lane == 0) partial[wave] = before;
    const int i = (int)blockIdx.x * 1024 + (int)threadIdx.x;
    const bool alive = (i < slots) && (life[i] > 0.0f);
    const unsigned long long mask = __ballot(alive);
    const uint32_t prefix = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_counts[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < 16; w++) base += partial[w];
    uint32_t wave_base = base;
    for (int w = 0; w < wave; w++) wave_base += wave_counts[w];
    if (alive) {
        const uint32_t dst = wave_base + prefix;
        if (dst < capacity) out[dst] = (uint32_t)i;
    }
    if ((blockIdx.x == gridDim.x - 1) && (threadIdx.x == 0)) {
        uint32_t t = base;
        for (int w = 0; w < 16; w++) t += wave_counts[w];
        *out_count = t;
    }
}
hipError_t launch_live_slots(const float* life, int32_t slots, uint32_t* out_slots, uint32_t capacity, uint32_t* out_count, uint32_t* block_counts, hipStream_t stream) {
    const unsigned blocks = (unsigned)((slots + 1023) / 1024);
    if (blocks == 0) return hipMemsetAsync(out_count, 0, sizeof(uint32_t), stream);
    hipLaunchKernelGGL(live_slots_count_kernel, dim3(blocks), dim3(1024), 0, stream, life, slots, block_counts);
    hipLaunchKernelGGL(live_slots_emit_kernel, dim3(blocks), dim3(1024), 0, stream, life, slots, block_counts, out_slots, capacity, out_count);
    return hipGetLastError();
}

// ilm_debug_step_sdf_samples: switch the count on / off and fetch-and-clear it (the caller has synchronised the device)
hipError_t step_sdf_sample_counter(int enable, unsigned long long* out) {
    unsigned long long value = 0, zero = 0;
    hipError_t e = hipMemcpyFromSymbol(&value, HIP_SYMBOL(g_step_sdf_samples), sizeof(value));
    if (e != hipSuccess) return e;
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_step_sdf_samples), &zero, sizeof(zero));
    if (e != hipSuccess) return e;
    const int flag = enable ? 1 : 0;
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_step_count_sdf_samples), &flag, sizeof(flag));
    if (out) *out = value;
    return e;
}

// The clamp class's two wave counters share one device flag (g_step_count_regular_waves): `bit` of it follows `enable`
static std::atomic<int> g_step_wave_counting{0};
static hipError_t set_step_wave_counting(int bit, int enable) {
    const int flag = enable ? (g_step_wave_counting |= bit) : (g_step_wave_counting &= ~bit);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_step_count_regular_waves), &flag, sizeof(flag));
}
// ilm_debug_step_regular_waves: the same for the clamp class's two wave counts
hipError_t step_regular_wave_counter(int enable, unsigned long long out[2]) {
    unsigned long long value[2] = { 0, 0 }, zero[2] = { 0, 0 };
    hipError_t e = hipMemcpyFromSymbol(value, HIP_SYMBOL(g_step_regular_waves), sizeof(value));
    if (e != hipSuccess) return e;
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_step_regular_waves), zero, sizeof(zero));
    if (e != hipSuccess) return e;
    e = set_step_wave_counting(1, enable);
    if (out) { out[0] = value[0]; out[1] = value[1]; }
    return e;
}

// ilm_debug_step_category_waves: the same for the three category counts
hipError_t step_category_wave_counter(int enable, unsigned long long out[3]) {
    unsigned long long value[3] = { 0, 0, 0 }, zero[3] = { 0, 0, 0 };
    hipError_t e = hipMemcpyFromSymbol(value, HIP_SYMBOL(g_step_category_waves), sizeof(value));
    if (e != hipSuccess) return e;
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_step_category_waves), zero, sizeof(zero));
    if (e != hipSuccess) return e;
    e = set_step_wave_counting(2, enable);
    if (out) { out[0] = value[0]; out[1] = value[1]; out[2] = value[2]; }
    return e;
}

}  // namespace ilm
