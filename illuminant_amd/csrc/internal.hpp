// internal.hpp -- launch descriptors shared between the kernels (particles.hip,
// lighting.hip) and the C-ABI implementation (api.hip).  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/illuminant_hip.h"
#include "hlsl_math.hpp"

namespace ilm {

// Component planes of one chunk, SoA, `stride` floats apart:
//   0..3  x, y, z, life          (PositionAndLife)
//   4..7  vx, vy, vz, category   (Velocity)
//   8..11 attribute rgba         (Chunk.Color)
//  12..15 render color rgba      (Chunk.RenderColor)
//  16..19 render data            (Chunk.RenderData: size, rotation, speed, category)
constexpr int kComponents = 20;
constexpr int kSlotsPerThread = 4;         // widest variant; strides are padded for it
// 128-thread blocks: a block's slot is refilled when its slowest wave ends, and the spawning variant (74 VGPRs, 6 waves per SIMD) fills the
// CU more evenly in pairs of waves than in fours (tools/step_ab.py r02: cfg2 with the spawner 22.1 -> 20.9 us per step, others unchanged)
constexpr int kStepThreads = 128;
constexpr int kSlotsPerBlock = 1024;       // strides are padded to this

// Values every wave would otherwise recompute on the vector ALU from uniform inputs (gfx950 has no scalar float
// unit): filled on the host with the SAME IEEE single-precision operations, in the same order, as the per-slot
// code they replace, so the results are bit-identical (api.hip is compiled with -ffp-contract=off).
struct StepDerived {
    float dt_s;                  // getDeltaTimeSeconds: GlobalSettings.x / 1000            (ParticleCommon.fxh:54-56)
    float inv_rw, inv_rh;        // RandomnessTexel = 1 / (807, 653)                         (RandomCommon.fxh:12-15)
    int32_t cs_shift;            // log2(chunk_size) when it is a power of two, else -1
    int32_t noise_may_revive;    // some Noise op can change the life of a dead slot (see api.hip); 0 => dead slots skip the transforms
    uint32_t bezier_codes;       // the uniform decisions of the update pass's four curves (bezier.hpp): byte 0 ColorFromLife, 1 ColorFromVelocity,
                                 // 2 SizeFromLife, 3 SizeFromVelocity
    uint32_t update_bits;        // bit 0: LifeRampSettings.x != 0 (life ramp on)   bit 1: getVelocityRotation() == 0   bit 2: LifeRampSettings.x < 0
    // Noise.fx:49-52 samples the randomness table at uv = ((xy * RandomnessTexel) + offset) * RandomnessTexel: the slot coordinate is
    // scaled by the texel size TWICE, so the texel column only steps once per 807 slots along x (the row once per 653 along y) and
    // a whole wave of 64 consecutive slots almost always reads ONE texel in each of the four lookups -- positionDelta and
    // velocityDelta (Noise.fx:49-60) are then the same for all 64 slots.  The map coordinate -> texel index is monotone (a chain
    // of monotone float operations), i.e. a step function; the host finds its steps with the same IEEE operations, evaluates the
    // two deltas for every combination of runs (api.hip, fill_noise_fast) and the wave picks its pair with scalar integer code.
    // A wave with a step inside it keeps the per-slot lookups.
    struct NoiseFast {
        int32_t op;              // index of the (first) Noise op this describes; -1: none / not applicable (then nothing else is read)
        int32_t classes;         // classes per axis of the delta tables: 3 (tables below) or 5 (tables in the unused spawn records
                                 // of the descriptor: chunk sizes above the table size, 807 x 653, step more often; see kNoiseBigTable)
        int32_t yb[4];           // rows where a sample's texel row steps (INT32_MAX: no such step): y class = #(yb <= row)
        uint32_t wcode[16];      // per 64-slot column w of a chunk row: bit 6 = usable, bits 0-2 = x class of the (x, y) samples,
                                 // bits 3-5 = x class of the (x + 2, y + 1) samples
        IlmFloat4 position[3][3];   // positionDelta [y class of row][x class]          (classes == 3)
        IlmFloat4 velocity[3][3];   // velocityDelta [y class of row + 1][x class]
    } noise;
    struct Op {
        int32_t area_none;       // AreaType outside 1..5: evaluateByTypeId returns 0 => weight == Strength exactly
        float   t;               // Noise / FMA with area_none: weight * dtMs / TimeDivisor
        float   max_accel;       // Gravity: MaximumAcceleration * dtMs / 1000
        int32_t _pad;
    } op[ILM_MAX_OPS];
};

// With 5 classes per axis the two delta tables are 2 x 25 float4 = 800 bytes: more than the kernarg block has left, but a launch
// without spawn records does not use desc.Spawns (2 x 544 bytes), so they live there: positionDelta[5][5] then velocityDelta[5][5].
constexpr int kNoiseBigClasses = 5;
static_assert(sizeof(IlmSpawnRecord) * ILM_MAX_SPAWNS >= 2 * kNoiseBigClasses * kNoiseBigClasses * sizeof(IlmFloat4), "noise tables fit the spawn records");

constexpr int kMaxPartialChunks = 4;
struct StepLaunch {
    IlmStepDesc desc;
    StepDerived derived;
    float* const* chunk_bases;   // device table, one base pointer per chunk
    int64_t stride;              // floats between component planes: span + the engine's plane padding (api.hip, ilm_engine_create)
    int32_t span;                // slots rounded up to kSlotsPerBlock: the units a launch walks per chunk are span / 64
    int32_t chunk_size;
    int32_t slots;               // chunk_size^2: lanes at or past it are stride padding (the stride is rounded up to 1024) and take no part
    int32_t first_chunk, chunk_count;
    uint32_t op_mask;            // bit t set when an op of type t is present
    int32_t streaming;           // != 0: the chunks of this launch do not fit the Infinity Cache -> non-temporal plane accesses
    const float4* rnd; int32_t rw, rh;
    const uint2* rnd_lp;         // the Rgba64 copy of the randomness table (SpatialNoise; ParticleEngine.cs:508-540)
    const float4* ramp; int32_t ramp_w, ramp_h;
    // extended spawn kinds (per spawn record slot): the Spawner's PositionBuffer and the feedback source chunk
    const float4* spawn_positions[ILM_MAX_SPAWNS]; int32_t spawn_position_count[ILM_MAX_SPAWNS];
    const float* source_base[ILM_MAX_SPAWNS];
    // PatternSpawner texture: mip levels back to back (ilm_system_set_spawn_pattern)
    const float4* spawn_pattern[ILM_MAX_SPAWNS]; int32_t pattern_w[ILM_MAX_SPAWNS], pattern_h[ILM_MAX_SPAWNS], pattern_levels[ILM_MAX_SPAWNS];
    SdfView sdf;
    // chunks whose tail has never been written (api.hip, System::used): units >= partial_units[i] of chunk partial_chunk[i]
    // hold only zeros and are skipped; chunks not listed are processed whole
    int32_t partial_count; int32_t partial_chunk[kMaxPartialChunks]; int32_t partial_units[kMaxPartialChunks];
    // ILM_STEP_COUNT_LIVE: one 64-bit counter per chunk at index chunk * kCountStride (its own 128-byte line), all zero on entry:
    // low word = live particles, high word = blocks of the chunk that have reported.  The block that completes a chunk publishes
    // {count_seq, count} with ONE system-scope store into page-locked host memory, where ilm_system_poll_counts reads it: no copy,
    // no event, no second stream (a record / wait pair on the stepping stream cost two ~7 us bubbles per counting step).
    // A chunk owns kCountLines lines: line 0 collects the chunk, lines 1.. are buckets that the chunk's blocks are dealt over
    // (block b of the chunk -> bucket b mod count_buckets), so that the ~4000 blocks of a 1024^2 chunk, which are resident at the
    // same time, do not queue on one address; the block that completes a bucket carries its sum to line 0.
    unsigned long long* live_counts;
    unsigned long long* zero_counts;     // the other counter region: zeroed by this launch for the next counting step
    unsigned long long* host_counts;     // device address of the page-locked table, one word per chunk: count_seq << 32 | count
    uint32_t count_seq;
    int32_t zero_n;                      // lines of the other region (capacity in chunks x kCountLines)
    int32_t count_buckets;               // power of two <= kCountLines - 1 that divides the blocks per chunk
    // Work is cut into units of one wave (64 consecutive slots); unit = chunk_rel * units_per_chunk + segment.
    // Filled by launch_step.
    int32_t units_per_chunk;     // stride / 64
    int32_t upc_shift;           // log2(units_per_chunk) when it is a power of two, else -1
    int32_t unit_begin, unit_end;        // global unit range [begin, end) of this launch
    int32_t unit_rotate, total_padded;   // block b starts at unit (b * 4 + unit_rotate) mod total_padded
};

static_assert(sizeof(StepLaunch) <= 4096, "StepLaunch travels in the kernarg segment (4 KB)");

// One item of ilm_engine_step_batch as it lies in the engine's device table: the item's StepLaunch, then where its blocks start in
// the grid of its launch (step_batch_kernel).  4 KB each, so a record starts on a line of its own.
struct alignas(4096) StepBatchItem {
    StepLaunch a;
    int32_t first_block;         // of the item in its launch's grid
    int32_t block_count;
};
static_assert(sizeof(StepBatchItem) == 4096 && offsetof(StepBatchItem, a) == 0, "a batch record is its StepLaunch plus the block range, 4 KB");

// per-chunk live counters are kCountStride 64-bit words apart (one 128-byte line each)
constexpr int kCountStride = 16;     // in 64-bit words
constexpr int kCountLines = 17;      // per chunk in the step kernels' counter regions: the chunk's line + 16 bucket lines
// Store elision of step_lean_kernel<.., STREAM = true> (particles.hip; the HBM-resident variant: the cache-resident one stores everything).
// Position and velocity planes are stored by a wave only when some lane changed their bits; that needs no bookkeeping.  The render colour / render data planes of a chunk may also be left alone when the host knows them to
// be RENDER-CURRENT under the step's render key (api.hip, System::render_gen): they hold exactly what the lean step's store path writes
// for the chunk's stored position, velocity and attributes under that key.  `render_elide` of launch_step: kElideDerived when every chunk
// of the launch is render-current.  `refreshed`: set when the lean step with its update pass ran, so that every chunk of the range is
// render-current under the key afterwards; left false by every other kernel (the records of the range must then be cleared).
constexpr uint32_t kElideDerived = 1u;
constexpr uint32_t kElideColor = 2u;     // (set by build_lean_step) the colour curves cannot produce a NaN factor: renderColor may be elided
constexpr uint32_t kElideRotation = 4u;  // (set by build_lean_step) RotationFromLifeAndIndex[0] == 0 and the velocity rotation is 0: rd.y does not read a finite life
// The category records of a system's chunks as launch_step sees them (api.hip, System::cat_current, states the rule): `table` is device
// memory, kCategoryRecordStride floats (one 64-byte line) per chunk -- floats 0 and 1 the {lo, hi} that category_bounds_kernel found, words
// 4..7 that kernel's scratch; `current` and `used` are the system's host arrays, indexed by chunk.  launch_step clears `current` over the
// range of a launch that may write a live slot's category, and has a clamp-class launch scan the chunks that are not current.
constexpr int kCategoryRecordStride = 16;
struct CategoryRecords { float* table; uint8_t* current; const int32_t* used; };
hipError_t launch_step(StepLaunch& a, hipStream_t stream, uint32_t render_elide = 0u, bool* refreshed = nullptr, CategoryRecords* cat = nullptr);
// ilm_engine_step_batch: lay a prepared StepLaunch out like launch_step does and return the batch kernel's variant for it (-1: the batch
// kernel does not cover it -- a streaming range -- and launch_step runs it); *blocks = the blocks it takes in a launch's grid.
// launch_step_batch: ONE launch over `blocks` blocks of items of one variant; item_of_block[b] indexes `table` (device memory, read-only).
int step_batch_layout(StepLaunch& a, int* blocks);
hipError_t launch_step_batch(int variant, const StepBatchItem* table, const int32_t* item_of_block, int blocks, hipStream_t stream);
hipError_t step_sdf_sample_counter(int enable, unsigned long long* out);   // ilm_debug_step_sdf_samples
hipError_t step_regular_wave_counter(int enable, unsigned long long out[2]);   // ilm_debug_step_regular_waves
hipError_t step_category_wave_counter(int enable, unsigned long long out[3]);  // ilm_debug_step_category_waves
// the slice-0 cells of a UNORM16 field (SdfView::cells0): does this step's collision update use them, and their build
bool step_wants_slice0_cells(const IlmStepDesc& d, int format);
hipError_t launch_build_slice0_cells(const uint2* texels, int width, int height, void* cells, hipStream_t stream);
int set_step_interpreter(int on);     // ilm_debug_step_interpreter: returns the previous setting
int last_step_kernel();               // ilm_debug_last_step_kernel: ILM_STEP_KERNEL_* of the process's latest launch_step
int set_step_streams(int n);          // ilm_debug_step_streams: 1 keeps every step on the context stream, 2 (default) lets large steps use two; returns the previous setting
// the context's stream for work that is not a particle step: ordered after everything the context's second stepping stream holds (api.hip)
hipStream_t ctx_stream_joined(IlmHandle ctx);
// Tracing ranges (the reference brackets every transform and light batch with RenderTrace.Marker,
// Illuminant/Particles/ParticleSystem.cs:464-469, Illuminant/Lighting/LightingRenderer.cs:1123-1124).  ILM_TRACE=1: every data-path entry
// point of the C ABI pushes a named roctx range for its duration (host side: what a call queues; the kernels of a range carry its
// correlation in a rocprofv3 --marker-trace --kernel-trace run).  The roctx library is bound at run time like RCCL (dlopen of
// librocprofiler-sdk-roctx.so.1, then libroctx64.so.4); off (the default) an entry point pays one predictable branch.
struct TraceApi { int (*push)(const char*) = nullptr; int (*pop)() = nullptr; bool on = false; };
const TraceApi& trace_api();
struct TraceRange {
    bool on;
    explicit TraceRange(const char* name) : on(trace_api().on) { if (on) (void)trace_api().push(name); }
    ~TraceRange() { if (on) (void)trace_api().pop(); }
    TraceRange(const TraceRange&) = delete;
    TraceRange& operator=(const TraceRange&) = delete;
};
#define ILM_TRACE_RANGE(name) ::ilm::TraceRange ilm_trace_range_(name)
// store-mode exchange of a group lightmap: the light passes into `lightmap` also store at the same offsets of `count` other buffers (0: off)
int32_t lightmap_set_mirrors(IlmHandle lightmap, void* const* buffers, int count);

// AoS float4 (device staging) <-> one SoA plane group (4 consecutive components)
hipError_t launch_aos_to_soa(const float4* src, float* plane0, int64_t stride, int32_t first_slot, int32_t count, hipStream_t stream);
hipError_t launch_soa_to_aos(const float* plane0, int64_t stride, float4* dst, int32_t first_slot, int32_t count, hipStream_t stream);

// standalone liveness count over the life plane of each chunk (CountLiveParticles.fx)
hipError_t launch_count_live(float* const* chunk_bases, int64_t stride, int32_t span, int32_t slots, int32_t chunk_count, uint32_t* counts, hipStream_t stream);
// Sensors (CollectParticles.fx:10-38; Sensor, Transforms.cs:374-486): sensor_count areas over chunks [first_chunk, first_chunk +
// chunk_count) in ONE pass over the position plane and the category.  counts[(k * chunk_count + c) * kSenseStride] += slots of chunk
// first_chunk + c that sensor k counts: every counter on a 128-byte line of its own, the table zero on entry.  Strength is not read.
constexpr int kSenseStride = 32;     // in 32-bit words
struct SenseLaunch {
    float* const* chunk_bases; int64_t stride; int32_t span, slots;
    int32_t first_chunk, chunk_count, sensor_count;
    int32_t tiles_per_block;         // filled by launch_sense: consecutive 1 024-slot tiles of a chunk per workgroup
    uint32_t* counts;
    IlmAreaParams sensors[ILM_MAX_SENSORS];
};
hipError_t launch_sense(SenseLaunch& a, hipStream_t stream);
// ordered live-slot compaction of one chunk (ballot + prefix sum); *out_count is a device counter
hipError_t launch_live_slots(const float* life, int32_t slots, uint32_t* out_slots, uint32_t capacity, uint32_t* out_count, uint32_t* block_counts, hipStream_t stream);

struct GBufferView {
    const void* texels;
    int32_t width, height, format;
};

// RampTexture of the light group being rendered (technique SphereLightWithDistanceRamp, RampCommon.fxh); texels == nullptr => none
struct RampView { const float4* texels; int32_t width, height; };

struct LightLaunch {
    int32_t light_count;
    IlmEnvironment env;
    IlmDistanceFieldUniforms df;
    GBufferView gbuffer;            // texels == nullptr => none
    TraceSdfView sdf;               // texels == nullptr => none
    float ambient[4];
    void* lightmap; int32_t width, height, format;
    int32_t row_begin, row_end;
    unsigned long long* stats;      // device, 3 counters, or nullptr
    const int32_t* light_count_ptr; // device: when non-null the record count is read from here (particle lights are counted on the device)
    int32_t accumulate;             // != 0: start from the lightmap's contents instead of `ambient` (additive blend onto an earlier pass)
    int32_t blend_fp16;             // != 0: the reference's HalfVector4 render target -- round through fp16 after every light (ilm_ctx_set_lightmap_blend)
    RampView ramp;
    int32_t tile_macro;             // edge of the square groups of tiles dealt round-robin to the XCDs (sphere_lights_kernel's tile map)
    // Light split (lighting.hip, "parts"): `split` workgroups serve one tile, each walking kLightParts / split consecutive parts of the
    // tile's light list; their per-part sums meet in `partials` (float4 per pixel, tile-major, part, thread) and the workgroup that
    // draws the tile's last ticket adds them up in part order.  split == 1: one workgroup per tile, nothing leaves the registers / LDS.
    const uint16_t* group_order;    // the groups in the order they are dealt out (heaviest first), or nullptr: row-major
    int32_t split;                  // the largest number of workgroups per tile in this launch (1: no split anywhere)
    // Tapered split: of the `taper_slots` tiles an XCD is dealt (block slots, padding included), the first taper[0] are served by one
    // workgroup each, those up to taper[1] by two, up to taper[2] by four, the rest by eight -- the work that starts last comes in the
    // smallest pieces (guided self-scheduling, laid out in the grid).  No taper: taper[0..2] = taper_slots.
    int32_t taper[3], taper_slots;
    float4* partials;               // device scratch of the context: tile_count * kLightParts * 256 float4 (split > 1)
    uint32_t* tickets;              // device, one per tile, zero between launches (the last arriver resets its tile's)
    // Store-mode exchange of a group lightmap (ILM_GATHER_STORE, group.hip): the lightmap's texel is ALSO stored at the same offset of
    // `mirror_count` other buffers -- the other members' copies of the frame, peer-mapped over xGMI -- so the strips need no gather phase.
    void* const* mirrors;           // device array of mirror_count base pointers (nullptr / 0: an ordinary lightmap)
    int32_t mirror_count;
    // ILM_LIGHT_BLEND_* of the call's rgb and of its alpha (ilm_ctx_set_light_blend_function).  Anything but ADD / ADD runs the BLEND
    // instantiations of the pass's kernel; the additive ones never read the pair.  (Two halves of the word that padded the descriptor
    // to its alignment: no member and no kernel argument moved.)
    int16_t blend_color, blend_alpha;
};
static_assert(sizeof(LightLaunch) == 456, "the blend functions fill the descriptor's tail padding: the kernels' argument offsets stay where they were");
// A tile's light list is summed in kLightParts consecutive parts (entries [p n / 8, (p + 1) n / 8) of a list of n), each part from zero in
// light order, the parts added onto the clear colour in part order: the sum's bits depend on the tile and its list only, not on how
// many workgroups computed the parts.
constexpr int kLightParts = 8;
// Tile edge of the light pass in pixels: four waves per workgroup, one 8 x 8 quadrant each
constexpr int kLightTile = 16;
constexpr int kLightTileThreads = (kLightTile / 8) * (kLightTile / 8) * 64;

constexpr size_t kLightRecBytes = 128;   // sizeof(LightRec) in lighting.hip
// What the in-volume trace loop asks of a light and the field, decided once per light by the prepare kernels (lighting.hip,
// light_flags): the centre inside the table sampler's box (SdfView) with the margin for rounding, and a field whose encoded distance,
// extent and step budget are in range.
struct TraceGate {
    float x0, x1, y0, y1, z0, z1;       // box of SdfView shrunk by the light-side margin; empty when the field has no table
    float field_ok;
};
TraceGate make_trace_gate(const IlmDistanceFieldUniforms& df, const SdfView& sdf);
// per-call preparation of the light records (footprint, cone config, trace flags) into `recs` (device, count * kLightRecBytes)
hipError_t launch_prepare_lights(const IlmLightVertex* lights, int count, const IlmEnvironment& env, const IlmDistanceFieldUniforms& df,
                                 const SdfView& sdf, void* recs, hipStream_t stream);
// sdf_filter: the bound field's ilm_sdf_set_filter state (FIXED8: one workgroup per tile, fp32 model, ADD / ADD -- anything else is an error)
hipError_t launch_sphere_lights_prepared(const LightLaunch& a, const void* recs, hipStream_t stream, int sdf_filter = ILM_SDF_FILTER_FP32);
// Directional lights (DirectionalLight.fx): the records (count * kLightRecBytes) and the full-frame pass over a's rows.  Of the launch
// descriptor the pass reads the frame, the resources, ambient / accumulate / blend_fp16, the ramp, stats and the mirrors; the sphere
// pass's tile map and light split do not apply (a footprint is a rectangle: four compares per pixel and light).
hipError_t launch_prepare_directional_lights(const IlmLightVertex* lights, int count, const IlmEnvironment& env, const IlmDistanceFieldUniforms& df,
                                             void* recs, hipStream_t stream);
hipError_t launch_directional_lights_prepared(const LightLaunch& a, const void* recs, hipStream_t stream);
// Projector lights (ProjectorLight.fx): the records (count * kProjectorRecBytes: one and a half slots of reserve_light_recs each) and the
// pass over a's rows, in the directional pass's frame.  a.ramp is the group's projector texture (ilm_ctx_set_projector_texture), not the
// ramp binding; a launch with lights needs one.
constexpr size_t kProjectorRecBytes = 192;
constexpr int32_t kMaxProjectorLights = 1 << 24;      // per call: 3 GiB of records; the slot arithmetic stays far inside an int
hipError_t launch_prepare_projector_lights(const IlmLightVertex* lights, int count, const IlmEnvironment& env, const IlmDistanceFieldUniforms& df,
                                           void* recs, hipStream_t stream);
hipError_t launch_projector_lights_prepared(const LightLaunch& a, const void* recs, hipStream_t stream);
// ... with a mip chain bound (ilm_ctx_set_projector_texture_mips, levels > 1): the table of the chain's levels, made on the host when the
// texture is bound -- level l is width[l] x height[l] texels from texel offset[l] of a.ramp.texels -- goes to the preparation by value
// (kernel arguments: scalar registers), which resolves each light's LOD against it into the record; the pass then reads records only.
// Records of the one preparation are not for the other pass.
constexpr int kMaxProjectorLevels = 16;
struct ProjectorMips { int32_t levels; int32_t offset[kMaxProjectorLevels], width[kMaxProjectorLevels], height[kMaxProjectorLevels]; };
hipError_t launch_prepare_projector_mip_lights(const IlmLightVertex* lights, int count, const IlmEnvironment& env, const IlmDistanceFieldUniforms& df,
                                               const ProjectorMips& mips, void* recs, hipStream_t stream);
hipError_t launch_projector_mip_lights_prepared(const LightLaunch& a, const void* recs, hipStream_t stream);
// Line lights (LineLight.fx): the records (count * kLightRecBytes) and the full-frame pass over a's rows, in the directional pass's frame.
// The ramp is not read (the reference has no LineLightWithRamp).
hipError_t launch_prepare_line_lights(const IlmLightVertex* lights, int count, const IlmDistanceFieldUniforms& df, void* recs, hipStream_t stream);
hipError_t launch_line_lights_prepared(const LightLaunch& a, const void* recs, hipStream_t stream);
// Volumetric lights (VolumetricLight.fx, ShadowedVolumetricLight.fx): the records (count * kLightRecBytes) and the pass over a's rows, in the
// directional pass's frame with its footprint test.  Neither the ramp nor the field uniforms are read by the preparation.
hipError_t launch_prepare_volumetric_lights(const IlmLightVertex* lights, int count, const IlmEnvironment& env, const IlmDistanceFieldUniforms& df,
                                            void* recs, hipStream_t stream);
hipError_t launch_volumetric_lights_prepared(const LightLaunch& a, const void* recs, hipStream_t stream);
int light_launch_blocks(const LightLaunch& a);    // workgroups of the tile kernel's launch for a (split / taper included)
int light_block_slots(const LightLaunch& a);      // block slots per XCD of the tile kernel's launch over a's rows

// Particle lights (ParticleLight.fx): ordered device-side compaction of the live, visible particles of every chunk into light
// records.  block_counts: one int per 1024-slot block of every chunk (scratch); *out_count receives the record count.
struct ParticleLightLaunch {
    float* const* chunk_bases; int64_t stride; int32_t chunk_count, slots;
    const int32_t* quad_counts;     // device, per chunk; nullptr => every slot
    IlmParticleLightParams params;
    IlmEnvironment env;
    float max_cone_radius;
    TraceGate gate;                 // make_trace_gate of the frame's field
    int32_t* block_counts;          // chunk_count * blocks_per_chunk
    void* recs; int32_t capacity;   // LightRec array
    int32_t* out_count;
};
hipError_t launch_prepare_particle_lights(const ParticleLightLaunch& a, hipStream_t stream);
// The same compaction over the chunks of many systems (ilm_engine_render_particle_lights_batch): one entry per (item, chunk) with a quad
// count above 0, in batch order.  An entry owns the ceil(quads / kParticleLightBatchBlock) workgroups from first_block on; `item` indexes
// the table of the items' parameters.  Records come out in entry / slot order -- item, chunk, slot.
constexpr int kParticleLightBatchBlock = 256;
struct ParticleLightBatchEntry { const float* base; int32_t quads, item, first_block, _pad; };
static_assert(sizeof(ParticleLightBatchEntry) == 24, "the entry table is laid out on the host");
struct ParticleLightBatchLaunch {
    const ParticleLightBatchEntry* entries; int32_t entry_count;     // device
    int32_t block_count;                                             // workgroups of all entries
    const IlmParticleLightParams* params;                            // device, one per item
    int64_t stride;
    IlmEnvironment env;
    float max_cone_radius;
    TraceGate gate;
    int32_t* block_counts;          // block_count ints: the workgroups' counts, then their exclusive bases
    void* recs; int32_t capacity;   // LightRec array
    int32_t* out_count;             // device: the record count, for the tile kernel
    int32_t* out_count_host;        // device-visible host word that receives it too (the diagnostic reads it after the stream)
};
hipError_t launch_prepare_particle_lights_batch(const ParticleLightBatchLaunch& a, hipStream_t stream);
// Light probes: every prepared light record on every probe; values = float4 per probe (device).  directional = false: sphere records
// (launch_prepare_lights; SphereLightProbe.fx, and LineLightProbe.fx through them); true: the directional pass's records
// (launch_prepare_directional_lights; DirectionalLight.fx:163-219), whose footprint is not read and which do not read `env`
hipError_t launch_light_probes(bool directional, const void* recs, int light_count, const float4* probe_positions, const float4* probe_normals,
                               int probe_count, const IlmEnvironment& env, const IlmDistanceFieldUniforms& df, const SdfView& sdf, const RampView& ramp,
                               float4* values, float4* pairs, hipStream_t stream);
// sampleDistanceFieldEx at `count` positions (xyz triples) -- diagnostic entry point ilm_sdf_sample
hipError_t launch_stamp16(void* where, const uint32_t stamp[4], hipStream_t stream);      // 16 bytes stored by a kernel (output.hip)
hipError_t launch_sdf_sample(const SdfView& sdf, const IlmDistanceFieldUniforms& df, const float* positions, int count, float* out, hipStream_t stream,
                             int sdf_filter = ILM_SDF_FILTER_FP32);
// fills the cell array of the table sampler (sdf.table_slices x sdf.slice_h x sdf.slice_w cells of 16 bytes) from the atlas
hipError_t launch_build_sdf_cells(const TraceSdfView& sdf, void* cells, int first_slice, int slice_count, hipStream_t stream);
hipError_t launch_sdf_sample_inside(const TraceSdfView& sdf, const IlmDistanceFieldUniforms& df, const float* positions, int count, float* out, int32_t* used,
                                    hipStream_t stream, int sdf_filter = ILM_SDF_FILTER_FP32);
hipError_t launch_divide_by_constant(float divisor, float reciprocal, unsigned long long* mismatches, hipStream_t stream);
void light_constant_divisors(float out[2][2]);
hipError_t launch_divide_probe(const float* n, const float* d, int count, float* out_fast, float* out_ieee, hipStream_t stream);

// ---- distance-field generation (fields.hip) ---------------------------------------------------------------
// One obstruction as the kernel reads it: the DistanceFunctionVertex (Vertices.cs:105-141) plus its quad in slice
// pixels, computed on the host with the oracle's operations (api.hip is compiled with -ffp-contract=off).
struct FieldObstruction {
    float cx, cy, cz; int32_t type;
    float sx, sy, sz; int32_t _pad;       // flags (api.hip): bit 0 the orientation is the identity quaternion (the rotation is skipped), bit 1 sizes and centre of ordinary magnitude
    float qx, qy, qz, qw;
    float x0, x1, y0, y1;       // raster bounds of DistanceFunctionVertexShader's quad, slice-local pixels
    // Exact culling (fields.hip): with e = |world position - centre|, the distance function is provably >= (e - cull_radius) / cull_inv_scale
    // (api.hip, fill_cull_bound: bounding sphere of the shape, safety margins for the float evaluation folded in).  An obstruction whose
    // bound cannot beat a texel's current maximum is not evaluated; cull_radius = +infinity switches the test off.
    float cull_inv_scale, cull_radius;
    float _pad2[2];
};
static_assert(sizeof(FieldObstruction) == 80, "FieldObstruction is one 80-byte record");
struct FieldVolume {
    int32_t first_vertex, vertex_count;
    float z0, z1;               // zRange = (ZBase, ZBase + Height)
    float x0, x1, y0, y1;       // hv.Bounds.Expand(DistanceLimit) in slice-local pixels
    float cx, cy, radius;       // a circle (world units) that holds the polygon, radius rounded up: the culling bound of fields.hip
    float _pad;
};
struct FieldLaunch {
    uint2* atlas; const uint2* clear_source; int32_t atlas_w;
    const int32_t* first_slices; int32_t triplet_count;     // device
    const FieldObstruction* obstructions; int32_t obstruction_count;
    const FieldVolume* volumes; int32_t volume_count;
    const float2* polygon_xy;
    int32_t slice_w, slice_h, columns, virtual_w, virtual_h;
    float slice_count_f, virtual_depth, z_offset, max_encoded, inv_scale_x, inv_scale_y;
};
hipError_t launch_render_slices(const FieldLaunch& a, int format, hipStream_t stream);

// G-buffer generation (fields.hip): volumes sorted by top height on the host, bounds of each polygon for the early reject
struct GBufferVolume {
    int32_t first_vertex, vertex_count;
    float top; int32_t enable_shadows;
    float x0, x1, y0, y1;
};
struct GBufferLaunch {
    void* texels; int32_t width, height, format;
    IlmGBufferRenderDesc desc;
    const GBufferVolume* volumes; int32_t volume_count;
    const float2* polygon_xy;
};
hipError_t launch_render_gbuffer(const GBufferLaunch& a, hipStream_t stream);

// G-buffer from the host's meshes (gbuffer.hip): one record per triangle in draw order, written by the setup kernel and read
// wave-uniformly by the raster kernel
constexpr int kGBufferAttrs = 11;
// what the setup kernel works on (one triangle in draw order) ...
struct GBufferPrimSetup {
    int32_t x[3], y[3];           // 1/256-pixel positions, clockwise on the y-down screen
    int32_t i0, i1, j0, j1;       // pixels whose centres the bounding box holds (inclusive; empty for a degenerate triangle)
    int32_t kind, texture;        // pixel shader; index into the launch's texture table or -1
    float a[3][kGBufferAttrs];    // per-vertex attributes
    int32_t flat;                 // bit k: attribute k is the same finite number at the three vertices (interpolation returns a[0][k] + 0)
    float enc_x, enc_y;           // the encoded normal of a ground / top / front-face triangle whose normal is flat
};
// ... and what it leaves for the raster kernel's scalar loads: per attribute (a0, a1 - a0, a2 - a0) side by side -- one 16-byte load and
// no subtraction per attribute and covering triangle (the differences are the same IEEE operations, taken once)
struct GBufferPrim {
    float4 attr[kGBufferAttrs];
    int32_t flat; float enc_x, enc_y; int32_t _pad;
};
struct GBufferTex { const void* texels; int32_t width, height, format, _pad; };
struct GBufferMeshLaunch {
    void* texels; int32_t width, height, format;
    IlmGBufferMeshDesc desc;
    const IlmHeightVolumeVertex* top; int32_t top_triangles;
    const IlmHeightVolumeVertex* front; int32_t front_triangles;
    const IlmBillboardVertex* billboards;
    const int4* quads;            // (quad, texture, kind, -) per billboard quad in draw order
    const GBufferTex* textures;   // device copy (read by the raster kernel)
    const GBufferTex* textures_in; int32_t texture_count;   // where the setup kernel copies it from (the pinned slot)
    GBufferPrim* prims; int32_t prim_count;
    int4* bounds;                 // (i0, i1, j0, j1) per record: what the binning passes read
    int4* verts;                  // (x0, y0, x1, y1), (x2, y2, kind, texture) per record: what a wave's coverage test reads
    int32_t block_shift, block_cols, block_rows;   // coarse bins: blocks of (1 << block_shift)^2 pixels, a multiple of the 16 x 16 tile
    int32_t* block_count;         // [block_cols * block_rows]
    int32_t* block_list;          // [block_cols * block_rows][prim_count] record indices in draw order
};
constexpr size_t kGBufferBlockListBudget = (size_t)256 << 20;   // bytes of block lists per frame before the blocks grow
hipError_t launch_gbuffer_meshes(const GBufferMeshLaunch& a, hipStream_t stream);

// ---- output side (output.hip) ---------------------------------------------------------------------------------
struct ReadbackLaunch {
    float* const* chunk_bases; int64_t stride; int32_t chunk_count, slots;
    const int32_t* element_counts;      // device, per chunk; nullptr => every slot
    IlmReadbackParams params;
    // derived on the host exactly as FillReadbackResult does before its loop (ParticleReadback.cs:100-112)
    float region_w, region_h; int32_t frame_count_x, frame_count_y; double max_angle_x, max_angle_y;
    int32_t* block_counts;
    IlmReadbackDrawCall* out; int32_t capacity;
    int32_t* out_count;
};
hipError_t launch_readback(const ReadbackLaunch& a, hipStream_t stream);

struct ResolveLaunch {
    const void* src; int32_t src_format;
    void* dst; int32_t dst_format;
    const void* albedo; int32_t albedo_format;      // the ...WithAlbedo techniques: the albedo texture, texel for texel (NULL: plain resolve)
    int32_t width, row_begin, row_end, mode;
    // uniform reciprocals are taken on the host (one rounding each; the per-pixel divisions they replace cost ~10 VALU instructions)
    float inverse_scale, offset, exposure_minus_one, gamma_minus_one, middle_gray, inv_average_luminance, inv_maximum_luminance_squared, inv_white;
};
hipError_t launch_resolve(const ResolveLaunch& a, hipStream_t stream);

// ilm_resolve_lighting_scaled: the per-pixel arithmetic is ResolveLaunch's (r.width is the DESTINATION's pitch in texels; r.row_begin and
// r.row_end are not read), the fetch is the header's: destination pixels [x0, x1) x [y0, y1), already clamped to the target and the rows.
struct ResolveScaledLaunch {
    ResolveLaunch r;
    int32_t src_w, src_h, albedo_w, albedo_h;
    int32_t x0, x1, y0, y1;
    float quad[4], lightmap_region[4], albedo_region[4], uv_offset[2];
    int32_t lightmap_filter, albedo_filter;
};
hipError_t launch_resolve_scaled(const ResolveScaledLaunch& a, hipStream_t stream);

// ilm_resolve_lighting_lut: the fetch and the coverage are ResolveScaledLaunch's (s.r.albedo is never NULL, s.r.mode is ILM_HDR_NONE: the
// epilogue of resolve_texel's plain branch), the arithmetic between them is the header's.  Every decision that does not depend on the
// pixel is taken on the host and arrives here: band or not, luminance or per-channel weight, which of the two non-band branches.
struct ResolveLutTexture {
    const void* texels; int32_t format;
    int32_t n;                          // Resolution: n slices of n x n texels side by side
    int32_t pitch;                      // texels per texture row: n * n
    int32_t row0;                       // Row * n: the first texel row of the LUT row that is read
};
struct ResolveLutLaunch {
    ResolveScaledLaunch s;
    ResolveLutTexture dark, bright;
    int32_t has_band, normalize, ramp, lut_only;     // ramp: BrightLevel > DarkLevel (else the shader's HACK branch)
    float dark_level;
    float neutral;                      // fminf(NeutralBandSize, bandWidth - 0.01f); read with has_band
    float transition;                   // (bandWidth - neutral) * 0.5f; read with has_band
    float inv_transition;               // 1.0f / transition
    float inv_range;                    // 1.0f / (BrightLevel - DarkLevel); read with ramp
};
hipError_t launch_resolve_lut(const ResolveLutLaunch& a, hipStream_t stream);

// ---- brightness estimation (brightness.hip) ---------------------------------------------------------------------
struct LuminanceLaunch {
    const void* texels; int32_t format, pitch;      // the lightmap, pitch in texels
    int32_t rw, rh, w0, h0;                          // render size and level-0 size (rw / 2, rh / 2)
    int32_t level;                                   // the level to produce: (w0 >> level) x (h0 >> level) floats at `out`
    float* out;
    float* mip[2];                                   // levels past 3: level 3 goes to mip[0], level k to mip[(k + 1) & 1] (each >= level 3's size)
};
hipError_t launch_luminance_level(const LuminanceLaunch& a, hipStream_t stream);
struct HistogramLaunch {
    const float* values; int32_t n;                  // the level
    int32_t bucket_count, ignore_zeroes; float scale;
    float table[256];                                // BucketMaxValues
    uint32_t* work;                                  // histogram_work_bytes() of device scratch
    float* partials; int32_t blocks;                 // bucket_count x histogram_blocks(n) partial sums
    double* sums;                                    // 256: each bucket's sum
    IlmHistogramBucket* out_buckets; float* out_totals;     // device-visible: bucket_count states, then SampleCount (bits), Min, Max, Sum, Median
};
int histogram_blocks(int n);
size_t histogram_work_bytes();
hipError_t launch_histogram(const HistogramLaunch& a, hipStream_t stream);
// One block of grow-on-demand device scratch: grown by api.hip's `reserve`, freed by the destroy entry point of its owner (no destructor:
// those may run while the process is torn down).  `bytes` is what was allocated; a capacity in elements is bytes / sizeof(T).
struct DeviceScratch {
    void* p = nullptr; size_t bytes = 0;
    template <class T> T* as() const { return static_cast<T*>(p); }
};
struct BrightnessScratch {
    DeviceScratch level;         // floats
    DeviceScratch mip;           // floats, both halves
    DeviceScratch work;          // histogram_work_bytes()
    DeviceScratch partials;      // 256 doubles (the buckets' sums), then 256 floats per workgroup
};

// ---- particle rasterisation (raster.hip) ------------------------------------------------------------------------
struct Sprite;
// One item of ilm_engine_render_particles_batch as it lies in the context's device table (items without chunks are left out): what
// RasterLaunch holds per call.  An item owns the blocks [first_block, first_block + ceil(total_slots / 256)) of the setup grid -- its slot
// range is padded to whole blocks, so a block never straddles two items and the item of a block is one search over this column.
struct RasterItem {
    float* const* chunk_bases; const int32_t* quad_counts;         // as RasterLaunch
    const float4* bitmap; int32_t bitmap_w, bitmap_h;
    int32_t first_block, total_slots;
    IlmRasterizeParams params;
};
static_assert(sizeof(RasterItem) % 8 == 0, "the quad counts behind the table stay aligned");
struct RasterLaunch {
    float* const* chunk_bases; int64_t stride; int32_t chunk_count, slots, total_slots;
    const int32_t* quad_counts;         // device, per chunk; nullptr => every slot
    IlmRasterizeParams params;
    void* target; int32_t format, width, height, tiles_x, tiles_y;
    int32_t count_shaded;               // != 0: count the fragments that were blended (statistics)
    const float4* bitmap; int32_t bitmap_w, bitmap_h;      // Appearance.Texture, one level (ilm_system_set_bitmap)
    // scratch, filled by render_particles
    Sprite* sprites; uint32_t* counts; uint32_t* offsets; uint2* rects;
    unsigned long long* keys; unsigned long long* sorted_keys; int64_t pair_count;
    unsigned long long* stats;          // [0] live quads, [2] shaded pixels
    // per tile (tile_count + 1 entries where scanned): first key of the tile's run, number of segments the run is cut into, first
    // work item of the tile, first partial-result slot of the tile (tiles with more than one segment only)
    uint32_t* tile_begin; uint32_t* tile_segments; uint32_t* tile_first_item; uint32_t* tile_multi; uint32_t* tile_first_partial;
    float* partials;                    // per partial slot: 256 x (premultiplied colour sum rgba, transmittance)
    int32_t work_items;                 // upper bound of the work items (grid of the shading kernel)
    // The batch (ilm_engine_render_particles_batch): items != nullptr -- last, so that nothing the single call reads moves.  Then chunk_bases,
    // quad_counts, params and bitmap are unused, total_slots is the padded total (256 x the setup grid) and a sprite's record carries its
    // item's index (raster.hip, Sprite).
    const RasterItem* items; int32_t item_count;
};
// device buffers the rasteriser keeps between calls (owned by the context)
struct RasterScratch {
    void* sprites = nullptr; void* counts = nullptr; void* offsets = nullptr; void* keys = nullptr; void* sorted_keys = nullptr;
    void* temp = nullptr; void* stats = nullptr; void* tiles = nullptr; void* partials = nullptr; void* rects = nullptr;
    size_t sprites_cap = 0, counts_cap = 0, offsets_cap = 0, keys_cap = 0, sorted_cap = 0, temp_cap = 0, tiles_cap = 0, partials_cap = 0, rects_cap = 0;
    unsigned long long* host_words = nullptr;    // pinned, device-visible: [0] the frame's pair count, [1..4] its statistics (written by kernels, read after a stream sync)
};
hipError_t render_particles(RasterLaunch& a, RasterScratch& s, hipStream_t stream, unsigned long long out_stats[3], bool* too_many);
void free_raster_scratch(RasterScratch& s);
hipError_t launch_clear_target(void* texels, int format, size_t n, float4 color, hipStream_t stream);

// ---- distance-field views (visualize.hip) -----------------------------------------------------------------------
struct VisualizeLaunch {
    SdfView sdf;
    IlmDistanceFieldUniforms df;
    void* target; int32_t format, width, height;
    int32_t x0, y0, x1, y1;             // pixels [x0, x1) x [y0, y1): a superset of the covered ones, inside the target (coverage is decided per pixel)
    int32_t tile_x0, tile_y0;           // origin of the grid's first tile (filled by launch_visualize)
    float px0, py0, px1, py1;           // the quad's rectangle in pixels
    float span_x, span_y;               // px1 - px0, py1 - py0
    float ray_start[4][3];              // TL, TR, BR, BL
    float ray_direction[3], ray_length; // RayVector / |RayVector| and |RayVector|, rounded once on the host (api.hip)
    float color[4], ambient_color[3], light_direction[3], light_color[3];
    float outline_size;
    int32_t mode, blend_mode;           // ILM_VISUALIZE_*, ILM_BLEND_ALPHA / ILM_BLEND_ADDITIVE
    unsigned long long* stats;          // device, zeroed: [0] covered pixels, [1] pixels drawn, [2] SDF samples; nullptr => the instantiation without counters
};
hipError_t launch_visualize(const VisualizeLaunch& a, hipStream_t stream);

// ---- shared with group.hip (the multi-device layer sits on the C ABI of api.hip, inside the same library) -------------------------
// thread-local error text + return code, as every entry point reports failures
int32_t api_fail(int32_t code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// the table of live handles (api.hip): objects of other translation units register under their own magic
constexpr uint32_t kMagicGroup = 0x494C4752u, kMagicGroupLightmap = 0x494C474Cu;
IlmHandle handle_register(const void* object, uint32_t magic);
bool handle_is_live(IlmHandle h, uint32_t magic);
void handle_retire(const void* object);
int ctx_child_count(IlmHandle ctx);        // live objects of a context (-1: not a context)
// one chunk of a system for the chunk exchange (api.hip): base of component 0, stride between component planes (floats), chunk size, owning context
int32_t system_chunk_view(IlmHandle system, int chunk, bool written, float** out_base, int64_t* out_stride, int32_t* out_chunk_size, IlmHandle* out_ctx);

}  // namespace ilm
