// visualize.hip -- distance-field views for gfx950: techniques ObjectSurfaces / ObjectOutlines of LightingRenderer.VisualizeDistanceField
// (Illuminant/Shaders/VisualizeDistanceField.fx:40-100, VisualizeCommon.fxh:47-133; Illuminant/Lighting/LightingRenderer.cs:1699-1892).
//
// The reference draws ONE quad whose four vertices carry the corners of a view plane (RayStart) and one ray vector, and sphere-traces
// the field per pixel.  Here: one thread per pixel of the quad's rectangle, 256-thread workgroups over 16 x 16 pixel tiles, a wave on
// an 8 x 8 block of them (the rays are parallel: neighbouring lanes tap neighbouring texels and leave the loop after similar trip
// counts).  The field is read through the general sampler (sample_distance_field, the one ilm_sdf_sample runs): no cell array, no
// rebuild bookkeeping, every position defined.
//
// Compiled with -ffp-contract=off, and the trace says so itself: every loop exit is a comparison of these values, and the tests hold
// the drawn mask and the sample counts to the CPU restatement exactly.
#include "internal.hpp"

namespace ilm {

namespace {
// VisualizeDistanceField.fx:8-9 (traceSurface) and the literals of traceOutlines, VisualizeCommon.fxh:105,126
constexpr float kTraceMinStepSize = 2.0f;
constexpr float kTraceFinalMinStepSize = 12.0f;
constexpr float kOutlineMinStepSize = 2.5f;
constexpr float kOutlineFinalMinStepSize = 12.0f;
constexpr float kOutlineFarthest = 99999.0f;
// The loops end on their own: positionAlongRay grows by at least 2 per iteration (fmaxf drops a NaN distance) and the entry point
// admits 1e-3 <= rayLength <= 65536, so `positionAlongRay <= rayLength` fails after at most 32 769 iterations.  The cap can never
// change a result; it is there because a loop that did not end would take the device with it.
constexpr int kMaxTraceIterations = 32800;
}  // namespace

template <int FMT, int MODE, int TARGET, bool COUNT>
__global__ __launch_bounds__(256) void visualize_kernel(const VisualizeLaunch a) {
#pragma clang fp contract(off)
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = a.tile_x0 + ((int)blockIdx.x * 16) + (wave & 1) * 8 + (lane & 7);
    const int y = a.tile_y0 + ((int)blockIdx.y * 16) + (wave >> 1) * 8 + (lane >> 3);
    // the top-left rule of an axis-aligned quad, on pixel centres; [x0, x1) x [y0, y1) is a superset clipped to the target
    const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
    const bool covered = (x >= a.x0) & (x < a.x1) & (y >= a.y0) & (y < a.y1) & (a.px0 <= cx) & (cx < a.px1) & (a.py0 <= cy) & (cy < a.py1);
    uint32_t samples = 0u;
    bool drawn = false;
    if (covered) {
        const float u = (cx - a.px0) / a.span_x, v = (cy - a.py0) / a.span_y;
        const f3 tl = mk3(a.ray_start[0][0], a.ray_start[0][1], a.ray_start[0][2]), tr = mk3(a.ray_start[1][0], a.ray_start[1][1], a.ray_start[1][2]);
        const f3 br = mk3(a.ray_start[2][0], a.ray_start[2][1], a.ray_start[2][2]), bl = mk3(a.ray_start[3][0], a.ray_start[3][1], a.ray_start[3][2]);
        const f3 top = tl + ((tr - tl) * u), bottom = bl + ((br - bl) * u);
        const f3 ray_start = top + ((bottom - top) * v);
        const f3 ray_direction = mk3(a.ray_direction[0], a.ray_direction[1], a.ray_direction[2]);
        const float ray_length = a.ray_length;
        float position_along_ray = 0.0f;
        float4 src = mk4(0.0f, 0.0f, 0.0f, 0.0f);
        if (MODE == ILM_VISUALIZE_SURFACES) {
            // traceSurface, VisualizeCommon.fxh:65-98
            bool hit = false;
            float intersection_distance = 0.0f;
            for (int i = 0; (i < kMaxTraceIterations) && (position_along_ray <= ray_length); i++) {
                const f3 sample_position = ray_start + (ray_direction * position_along_ray);
                const float distance = sample_distance_field<FMT>(sample_position, a.df, a.sdf);
                samples++;
                const float min_step_size = fmaxf(kTraceMinStepSize, (position_along_ray / ray_length) * kTraceFinalMinStepSize);
                if (distance <= min_step_size) {
                    intersection_distance = position_along_ray + distance;
                    hit = true;
                    break;
                }
                const float step_size = fmaxf(min_step_size, fabsf(distance));
                position_along_ray = position_along_ray + step_size;
            }
            if (hit) {
                // ObjectSurfacesPixelShader, VisualizeDistanceField.fx:53-61
                const f3 estimated_intersection = ray_start + (ray_direction * intersection_distance);
                const f3 normal = estimate_normal4<FMT>(estimated_intersection, a.df, a.sdf);
                samples += 4u;
                float normal_dot_light = dot3(normal, mk3(a.light_direction[0], a.light_direction[1], a.light_direction[2]));
                normal_dot_light = fminf(fmaxf((normal_dot_light + 0.05f) * 1.1f, 0.0f), 1.0f);
                src = mk4(a.ambient_color[0] + ((a.light_color[0] * normal_dot_light) * a.color[0]),
                          a.ambient_color[1] + ((a.light_color[1] * normal_dot_light) * a.color[1]),
                          a.ambient_color[2] + ((a.light_color[2] * normal_dot_light) * a.color[2]), 1.0f);
                drawn = true;
            }
        } else {
            // traceOutlines, VisualizeCommon.fxh:100-133; FILL_INTERIOR = FilledInterior (Silhouettes)
            float closest_distance = kOutlineFarthest;
            bool filled = false;
            for (int i = 0; (i < kMaxTraceIterations) && (position_along_ray <= ray_length); i++) {
                const f3 sample_position = ray_start + (ray_direction * position_along_ray);
                const float distance = sample_distance_field<FMT>(sample_position, a.df, a.sdf);
                samples++;
                closest_distance = fminf(distance, closest_distance);
                if (MODE == ILM_VISUALIZE_SILHOUETTES) {
                    if (distance <= 1.0f) { filled = true; break; }
                } else {
                    if (distance < -a.outline_size) break;
                }
                const float min_step_size = fmaxf(kOutlineMinStepSize, (position_along_ray / ray_length) * kOutlineFinalMinStepSize);
                const float step_size = fmaxf(min_step_size, fabsf(distance));
                position_along_ray = position_along_ray + step_size;
            }
            float alpha = 1.0f;
            if (!filled) {
                const float clamped = fminf(fmaxf(closest_distance - 1.0f, -a.outline_size), a.outline_size);
                const float t = 1.0f - fabsf(clamped / a.outline_size);
                alpha = t * t;
            }
            // ObjectOutlinesPixelShader, VisualizeDistanceField.fx:78-83
            src = mk4(alpha * a.color[0], alpha * a.color[1], alpha * a.color[2], alpha * a.color[3]);
            drawn = !(alpha <= 0.0f);
        }
        if (drawn) {
            const size_t o = (size_t)y * (size_t)a.width + (size_t)x;
            const float4 dst = load_target<TARGET>(a.target, o);
            const float keep = (a.blend_mode == ILM_BLEND_ADDITIVE) ? 1.0f : (1.0f - src.w);
            store_target<TARGET>(a.target, o, mk4(src.x + (dst.x * keep), src.y + (dst.y * keep), src.z + (dst.z * keep), src.w + (dst.w * keep)));
        }
    }
    if (COUNT) {
        // per-wave sums, one atomic per wave and counter
        uint32_t n_covered = covered ? 1u : 0u, n_drawn = drawn ? 1u : 0u;
        for (int off = 32; off > 0; off >>= 1) {
            n_covered += __shfl_down(n_covered, off);
            n_drawn += __shfl_down(n_drawn, off);
            samples += __shfl_down(samples, off);
        }
        if (lane == 0) {
            if (n_covered != 0u) atomicAdd(&a.stats[0], (unsigned long long)n_covered);
            if (n_drawn != 0u) atomicAdd(&a.stats[1], (unsigned long long)n_drawn);
            if (samples != 0u) atomicAdd(&a.stats[2], (unsigned long long)samples);
        }
    }
}

template <int FMT, int MODE, int TARGET>
static void launch_counted(const VisualizeLaunch& a, dim3 grid, hipStream_t stream) {
    if (a.stats) hipLaunchKernelGGL((visualize_kernel<FMT, MODE, TARGET, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((visualize_kernel<FMT, MODE, TARGET, false>), grid, dim3(256), 0, stream, a);
}
template <int FMT, int MODE>
static void launch_target(const VisualizeLaunch& a, dim3 grid, hipStream_t stream) {
    if (a.format == ILM_LIGHTMAP_FLOAT4) launch_counted<FMT, MODE, ILM_LIGHTMAP_FLOAT4>(a, grid, stream);
    else if (a.format == ILM_LIGHTMAP_HALF4) launch_counted<FMT, MODE, ILM_LIGHTMAP_HALF4>(a, grid, stream);
    else launch_counted<FMT, MODE, ILM_LIGHTMAP_RGBA8>(a, grid, stream);
}
template <int FMT>
static void launch_mode(const VisualizeLaunch& a, dim3 grid, hipStream_t stream) {
    if (a.mode == ILM_VISUALIZE_SURFACES) launch_target<FMT, ILM_VISUALIZE_SURFACES>(a, grid, stream);
    else if (a.mode == ILM_VISUALIZE_OUTLINES) launch_target<FMT, ILM_VISUALIZE_OUTLINES>(a, grid, stream);
    else launch_target<FMT, ILM_VISUALIZE_SILHOUETTES>(a, grid, stream);
}

// [x0, x1) x [y0, y1) must lie inside the target and be non-empty (api.hip clips; an empty rectangle is never launched)
hipError_t launch_visualize(const VisualizeLaunch& launch, hipStream_t stream) {
    VisualizeLaunch a = launch;
    if (a.x0 < 0 || a.y0 < 0 || a.x1 > a.width || a.y1 > a.height || a.x0 >= a.x1 || a.y0 >= a.y1) return hipErrorInvalidValue;
    a.tile_x0 = a.x0 & ~15; a.tile_y0 = a.y0 & ~15;
    const dim3 grid((unsigned)((a.x1 - a.tile_x0 + 15) / 16), (unsigned)((a.y1 - a.tile_y0 + 15) / 16));
    if (a.sdf.format == ILM_SDF_FP16) launch_mode<ILM_SDF_FP16>(a, grid, stream);
    else launch_mode<ILM_SDF_UNORM16>(a, grid, stream);
    return hipGetLastError();
}

}  // namespace ilm
