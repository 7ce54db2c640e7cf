/*
 * illuminant_hip.h -- C ABI of libilluminant_hip.so
 *
 * The drop-in boundary for the two data-parallel hot paths of sq/Illuminant on
 * MI355X (gfx950): the ParticleEngine per-chunk state update and the
 * LightingRenderer sphere-light SDF cone trace.  Everything here is plain C:
 * POD structs whose byte layout is the reference's own uniform / vertex
 * structs (so C# can pass them with `ref` / `fixed`), opaque handles for
 * device memory, int32 return codes (0 = ok).
 *
 * All file:line citations are relative to the reference checkout
 * (sq/Illuminant @ 2025-08-29).  The reference interface each entry point
 * replaces is cited on the entry point.  INTEGRATION.md shows the P/Invoke
 * declarations a maintainer of the reference would add.
 *
 * Threading: a context owns one HIP stream; calls on one context are
 * asynchronous and ordered; callers serialise calls per context (this is what
 * the reference's `lock (_UpdateParameterPool)` / issue-thread ordering gives,
 * Illuminant/Particles/ParticleSystem.cs:681).  Different contexts may be driven
 * from different threads; the ilm_debug_* switches are process-wide (atomic) and
 * change the behaviour of every context.  Host output buffers are valid
 * after the call returns (download / count calls synchronise the stream).
 */
#ifndef ILLUMINANT_HIP_H
#define ILLUMINANT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 11: + ilm_engine_step_batch, ilm_debug_last_step_batch, ILM_STEP_KERNEL_BATCH; later, under the same number (no layout changed, nothing
 * removed): + ilm_visualize_distance_field / IlmVisualizeVertex, IlmVisualizeParams, ILM_VISUALIZE_* (distance-field views);
 * + ilm_render_directional_lights (directional lights; no new struct: the reference packs them into a LightVertex);
 * + ilm_ctx_set_projector_texture, ilm_render_projector_lights (projector lights; a LightVertex again);
 * + ilm_render_line_lights (line lights; a LightVertex again); + ilm_render_volumetric_lights (volumetric lights; likewise);
 * + ilm_ctx_set_projector_texture_mips (a projector texture's mip chain, fetched trilinearly at the light's mip bias);
 * + ilm_ctx_set_light_blend_function, ILM_LIGHT_BLEND_* (subtractive, max and min light groups: LightSource.BlendMode);
 * + ilm_resolve_lighting_scaled, ILM_FILTER_* (the resolve onto a target of another size: RenderScale != 1);
 * + ilm_resolve_lighting_lut / IlmLUTBlending (the LUT-blended resolve over a dark and a bright colour LUT);
 * + ilm_sdf_set_filter, ilm_sdf_get_filter, ILM_SDF_FILTER_* (a fixed-point bilinear filter mode of the distance-field sampler);
 * + ilm_engine_render_particles_batch, ilm_debug_last_render_batch / IlmRasterizeItem (a frame's particle systems rasterised as one draw list);
 * + ilm_system_sense, ilm_system_sense_async, ilm_system_poll_sense, ILM_MAX_SENSORS (particle sensors: Transforms.Sensor counted on the device);
 * + ilm_engine_render_particle_lights_batch, ilm_debug_last_particle_light_batch / IlmParticleLightItem (a frame's particle light sources as one light list).
 * 10: + ilm_lightmap_luminance, ilm_lightmap_histogram, ilm_debug_queue_luminance / IlmHistogramBucket, IlmHistogramParams,
 * IlmHistogramResult (brightness estimation on the device).  Nothing removed or changed in layout.
 * 9 (r06): + ilm_group_gather_chunks (the sharded particle state made whole on every member: Pos+Life for global consumers, Pos+Life
 * and RenderColor for particle lights across ranks).  Nothing removed or changed in layout.
 * 8 (r05): + ilm_group_lightmap_store_mode, ILM_GATHER_STORE, ilm_debug_last_light_launch, ilm_ctx_create_sibling,
 * ILM_GATHER_ASYNC + ilm_group_lightmap_wait.
 * 7 (r04): + ilm_ctx_set_light_split, ilm_sdf_mark_dirty, ilm_sdf_trace_info / IlmSdfTraceInfo; ilm_group_lightmap_set_strips became a
 * collective with one process per GPU.  Nothing was removed or changed in layout since 6. */
#define ILM_ABI_VERSION 11

/* ---- return codes ------------------------------------------------------ */
#define ILM_OK                    0
#define ILM_ERR_INVALID_ARGUMENT  (-1)
#define ILM_ERR_INVALID_HANDLE    (-2)
#define ILM_ERR_OUT_OF_RANGE      (-3)
#define ILM_ERR_TOO_MANY          (-4)   /* e.g. >16 attractors: Transforms.cs:348-349 */
#define ILM_ERR_NO_DEVICE         (-5)
#define ILM_ERR_STATE             (-6)   /* e.g. DF update without a bound field: ParticleSystem.cs:835-836 */
/* positive values are hipError_t values passed through unchanged */

/* Opaque object handles (contexts, engines, systems, textures).  Every entry point looks its handles up in a table of live
 * objects first: a destroyed, foreign or garbage value returns ILM_ERR_INVALID_HANDLE, it is never dereferenced.  0 is never
 * a valid handle.  A create call that fails releases everything it had allocated and leaves *out = 0.  Parents outlive children:
 * destroying a context (engine) that still has live objects (systems) returns ILM_ERR_STATE and destroys nothing. */
typedef uint64_t IlmHandle;

/* ---- POD mirrors of the reference's uniform structs -------------------- */

typedef struct IlmFloat4 { float x, y, z, w; } IlmFloat4;

/* XNA Matrix, row-major M11..M44; shaders use mul(rowVector, M)
 * (Illuminant/Shaders/SpawnerCommon.fxh:166,179). */
typedef struct IlmMatrix { float m[16]; } IlmMatrix;

/* Uniforms.ParticleSystem -- Illuminant/Uniforms.cs:197-236,
 * accessors Illuminant/Shaders/ParticleCommon.fxh:29-92. */
typedef struct IlmParticleSystemUniforms {
    IlmFloat4 GlobalSettings;     /* deltaTimeMilliseconds, friction, maximumVelocity, lifeDecayRate */
    IlmFloat4 CollisionSettings;  /* escapeVelocity, bounceVelocityMultiplier, collisionDistance, collisionLifePenalty */
    IlmFloat4 TexelAndSize;       /* 1/ChunkSize, 1/ChunkSize, Size.X, Size.Y */
    IlmFloat4 AnimationRateAndRotationAndZToY; /* rate_x, rate_y, velocityRotation, zToY */
} IlmParticleSystemUniforms;

/* Uniforms.ClampedBezier1 / ClampedBezier4 -- Illuminant/Bezier.cs:433-441,588-599;
 * shader side Illuminant/Shaders/Bezier.fxh:6-19. */
typedef struct IlmClampedBezier1 { IlmFloat4 RangeAndCount, ABCD; } IlmClampedBezier1;
typedef struct IlmClampedBezier4 { IlmFloat4 RangeAndCount, A, B, C, D; } IlmClampedBezier4;

/* Uniforms.DistanceField -- Illuminant/Uniforms.cs:79-88 -- followed by the
 * separately-bound DistanceFieldPacked1 (Illuminant/Lighting/LightingRenderer.cs:1933-1939,
 * Illuminant/Shaders/DistanceFieldCommon.fxh:189-206). */
typedef struct IlmDistanceFieldUniforms {
    IlmFloat4 ConeAndMisc;              /* MaxConeRadius, DistanceFieldZOffset, OcclusionToOpacityPower, InvScaleFactorX */
    IlmFloat4 TextureSliceAndTexelSize; /* 1/cols, 1/rows, 1/(virtualW*cols), 1/(virtualH*rows) */
    IlmFloat4 StepAndMisc2;             /* StepLimit, MinimumLength, LongStepFactor, InvScaleFactorY */
    IlmFloat4 TextureSliceCount;        /* cols, rows, validZ, sliceCount */
    IlmFloat4 Extent;                   /* virtualW, virtualH, virtualDepth, maximumEncodedDistance */
    IlmFloat4 Packed1;                  /* 1/(3*cols), sliceCount/extentZ, validZ, minStepSize */
} IlmDistanceFieldUniforms;

/* Uniforms.Environment -- Illuminant/Uniforms.cs:14-24 -- plus the G-buffer
 * uniforms bound by SetGBufferParameters (Illuminant/Lighting/LightingRenderer.GBuffer.cs:520-534)
 * and the view-transform values the pixel shader reads through
 * GetViewportPosition()/GetViewportScale() (Illuminant/Shaders/LightCommon.fxh:27-33). */
typedef struct IlmEnvironment {
    IlmFloat4 ZAndScale;          /* GroundZ, MaximumZ, RenderScale.X, RenderScale.Y */
    IlmFloat4 ZToY;               /* ZToYMultiplier, InvZToYMultiplier, LightOcclusion, unused */
    IlmFloat4 GBufferTexelSizeAndMisc; /* 1/gbufW, 1/gbufH, ViewportScaleX, ViewportScaleY; xy==0 => no G-buffer */
    float     ViewportPosition[2];
    float     GBufferViewportRelative;
    float     _pad0;
} IlmEnvironment;

/* LightVertex, 8 x float4, Pack=4 -- Illuminant/Vertices.cs:10-39; filled by
 * RenderSphereLightSource, Illuminant/Lighting/LightingRenderer.cs:1193-1219. */
typedef struct IlmLightVertex {
    IlmFloat4 LightPosition1, LightPosition2, LightPosition3;
    IlmFloat4 LightProperties;         /* radius, rampLength, rampMode, castsShadows */
    IlmFloat4 MoreLightProperties;     /* aoRadius, shadowDistanceFalloff, falloffYFactor, aoOpacity */
    IlmFloat4 EvenMoreLightProperties; /* shadowFilter, 0, rampOffset, rampRate */
    IlmFloat4 Color1;                  /* rgb, a*opacity*intensityScale */
    IlmFloat4 Color2;                  /* specular rgb, specular power */
} IlmLightVertex;

/* ---- particle transform parameters ------------------------------------- */

/* ParticleAreaTransform.SetParameters -- Illuminant/Particles/ParticleTransform.cs:294-318. */
typedef struct IlmAreaParams {
    int32_t AreaType;             /* 0 none, 1 ellipsoid, 2 box, 3 cylinder, 4 spheroid, 5 octagon */
    float   Strength;
    float   AreaFalloff;
    float   AreaRotation;
    float   AreaCenter[3];  float _pad0;
    float   AreaSize[3];    float _pad1;
    float   CategoryFilter[2];    /* default (-9999, 9999) */
    float   _pad2[2];
} IlmAreaParams;

#define ILM_MAX_ATTRACTORS 16     /* Illuminant/Shaders/Gravity.fx:3 */

/* Gravity.SetParameters -- Illuminant/Particles/Transforms.cs:347-365; shader
 * Illuminant/Shaders/Gravity.fx:5-10.  NOTE: Gravity derives from ParticleTransform,
 * not ParticleAreaTransform, so the reference never binds CategoryFilter for it
 * and the effect default (0,0) applies; the field is explicit here. */
typedef struct IlmGravityParams {
    int32_t AttractorCount;
    float   MaximumAcceleration;
    float   CategoryFilter[2];
    float   AttractorPositions[ILM_MAX_ATTRACTORS][3];
    float   AttractorRadiusesAndStrengths[ILM_MAX_ATTRACTORS][3]; /* radius, strength, type */
} IlmGravityParams;

/* FMA.SetParameters -- Illuminant/Particles/Transforms.cs:38-45; shader Illuminant/Shaders/FMA.fx:4-13. */
typedef struct IlmFMAParams {
    IlmAreaParams Area;
    float     TimeDivisor;  float _pad[3];
    IlmFloat4 PositionAdd, PositionMultiply;
    IlmFloat4 VelocityAdd, VelocityMultiply;
} IlmFMAParams;

/* Noise.SetParameters -- Illuminant/Particles/Transforms.cs:243-268; shader Illuminant/Shaders/Noise.fx:5-19. */
typedef struct IlmNoiseParams {
    IlmAreaParams Area;
    float     TimeDivisor;
    float     FrequencyLerp;
    float     ReplaceOldVelocity;
    float     _pad;
    float     RandomnessOffset[2];
    float     NextRandomnessOffset[2];
    IlmFloat4 PositionOffset, PositionMinimum, PositionScale;
    IlmFloat4 VelocityOffset, VelocityMinimum, VelocityScale;
} IlmNoiseParams;

#define ILM_MAX_INLINE_POSITION_CONSTANTS 4   /* Illuminant/Shaders/SpawnerCommon.fxh:1 */

/* SpawnerBase.SetParameters + Spawner.SetParameters --
 * Illuminant/Particles/ParticleSpawner.cs:200-256,376-403; shader uniforms
 * Illuminant/Shaders/SpawnerCommon.fxh:3-15. */
typedef struct IlmSpawnParams {
    float     ChunkSizeAndIndices[4];   /* chunkSize, first, last, positionIndexOffset */
    IlmFloat4 Configuration[9];
    float     FormulaTypes[4];
    IlmMatrix PositionMatrix, VelocityMatrix;
    float     AxisMask[3];
    float     AlignVelocityAndPosition;
    float     RandomnessOffset[2];
    float     AttributeDiscardThreshold;  /* AlphaDiscardThreshold / 255 */
    float     PolygonRate;
    float     PolygonLoop;
    float     PositionConstantCount;
    float     _pad[2];
    IlmFloat4 InlinePositionConstants[ILM_MAX_INLINE_POSITION_CONSTANTS];
} IlmSpawnParams;

/* Everything SetSystemUniforms (Illuminant/Particles/ParticleSystem.cs:547-575) and
 * UpdateHandler._BeforeDraw (Illuminant/Particles/ParticleTransform.cs:84-168) bind
 * for the Update pass. */
typedef struct IlmUpdateParams {
    IlmClampedBezier4 ColorFromLife, ColorFromVelocity;
    IlmClampedBezier1 SizeFromLife, SizeFromVelocity;
    float     RotationFromLifeAndIndex[2];   /* radians */
    float     _pad[2];
    IlmFloat4 LifeRampSettings;              /* strength, min, divisor, indexDivisor; x==0 => off */
} IlmUpdateParams;

/* MatrixMultiply.SetParameters -- Illuminant/Particles/Transforms.cs:61-66; shader
 * Illuminant/Shaders/MatrixMultiply.fx:4-52 (mul3: Illuminant/Shaders/ParticleCommon.fxh:183-196). */
typedef struct IlmMatrixMultiplyParams {
    IlmAreaParams Area;
    float     TimeDivisor;  float _pad[3];     /* 1000 / CyclesPerSecond, or -1 => timeScale 1 */
    IlmMatrix PositionMatrix, VelocityMatrix;
} IlmMatrixMultiplyParams;

/* SpatialNoise.SetParameters -- Illuminant/Particles/Transforms.cs:275-300 on top of Noise's; shader
 * Illuminant/Shaders/Noise.fx:17,74-116 (smoothRandomCustom: bilinear, WRAP, on the Rgba64 copy of the
 * randomness table, Illuminant/Shaders/RandomCommon.fxh:7-15,36-39, Illuminant/Particles/ParticleEngine.cs:508-540). */
typedef struct IlmSpatialNoiseParams {
    IlmNoiseParams Noise;            /* PositionMinimum / VelocityMinimum are not read by this technique */
    float     SpaceScale[2];         /* 1 / SpaceScale.X, 1 / SpaceScale.Y */
    float     _pad[2];
} IlmSpatialNoiseParams;

enum {
    ILM_OP_GRAVITY         = 1,   /* technique Gravity,        Illuminant/Shaders/Gravity.fx:12-61        */
    ILM_OP_NOISE           = 2,   /* technique Noise,          Illuminant/Shaders/Noise.fx:28-72          */
    ILM_OP_FMA             = 3,   /* technique FMA,            Illuminant/Shaders/FMA.fx:15-51            */
    ILM_OP_MATRIX_MULTIPLY = 4,   /* technique MatrixMultiply, Illuminant/Shaders/MatrixMultiply.fx:22-52 */
    ILM_OP_SPATIAL_NOISE   = 5    /* technique SpatialNoise,   Illuminant/Shaders/Noise.fx:74-116         */
};

typedef struct IlmTransformOp {
    int32_t Type;
    int32_t _pad[3];
    union {
        IlmGravityParams        Gravity;
        IlmNoiseParams          Noise;
        IlmFMAParams            FMA;
        IlmMatrixMultiplyParams MatrixMultiply;
        IlmSpatialNoiseParams   SpatialNoise;
    } u;
} IlmTransformOp;

enum {
    ILM_UPDATE_NONE                = 0,  /* transforms only */
    ILM_UPDATE_POSITIONS           = 1,  /* technique UpdatePositions, UpdateParticleSystem.fx:9-38 */
    ILM_UPDATE_WITH_DISTANCE_FIELD = 2,  /* technique UpdateWithDistanceField, UpdateParticleSystemWithDistanceField.fx:29-147 */
    ILM_UPDATE_ERASE               = 3   /* technique Erase, UpdateParticleSystem.fx:40-49 */
};

#define ILM_MAX_OPS    4
#define ILM_MAX_SPAWNS 2

#define ILM_STEP_COUNT_LIVE  1u   /* also produce per-chunk live counts (CountLiveParticles.fx) */

enum {
    ILM_SPAWN_INLINE           = 0,  /* technique SpawnParticles (<= 4 inline positions), SpawnParticles.fx:10-30 */
    ILM_SPAWN_POSITION_BUFFER  = 1,  /* technique SpawnParticlesFromPositionTexture, SpawnParticles.fx:32-52: positions from
                                        the list bound with ilm_system_set_spawn_positions */
    ILM_SPAWN_FEEDBACK         = 2,  /* technique SpawnFeedbackParticles, SpawnParticles.fx:54-118: one source particle of
                                        another system's chunk per InstanceMultiplier new particles */
    ILM_SPAWN_PATTERN          = 3   /* technique SpawnPatternParticles, PatternSpawner.fx:21-97: one particle per Divisor x Divisor
                                        block of the texture bound with ilm_system_set_spawn_pattern */
};

/* FeedbackSpawner.SetParameters (Illuminant/Particles/SpecialSpawners.cs:411-427) + the source chunk bound by
 * UpdateHandler._BeforeDraw (Illuminant/Particles/ParticleTransform.cs:129-141, SourceChunkSizeAndTexel). */
typedef struct IlmFeedbackParams {
    IlmHandle SourceSystem;            /* system that owns the source chunk (same engine chunk size) */
    int32_t   SourceChunkIndex;        /* index in the source system's chunk table */
    float     FeedbackSourceIndex;     /* first source slot */
    float     InstanceMultiplier;
    float     SourceVelocityFactor;
    float     AlignPositionConstant, MultiplyLife, MultiplyAttributeConstant;
    float     SourceLifeRange[2];
    float     _pad;
} IlmFeedbackParams;

/* PatternSpawner.SetParameters (Illuminant/Particles/SpecialSpawners.cs:208-256); uniforms of
 * Illuminant/Shaders/PatternSpawner.fx:6-9. */
typedef struct IlmPatternParams {
    float StepWidthAndSizeScale[4];    /* Divisor, ParticlesPerRow, Divisor / texWidth, Divisor / texHeight */
    float YOffsetsAndCoordScale[4];    /* currentRow, currentRow * Divisor / texHeight, Divisor, Divisor */
    float TexelOffsetAndMipBias[4];    /* -0.5 / texWidth + baseX, -0.5 / texHeight + baseY, 0, log2(Divisor) + MipBiasBase */
    float CenteringOffset[2];          /* DirectTextureSize * -0.5 */
    float MultiplyAttributeConstant;   /* != 0: pattern colour * Configuration[5], else + */
    float _pad;
} IlmPatternParams;

typedef struct IlmSpawnRecord {
    int32_t        ChunkIndex;    /* index in the system's chunk table */
    int32_t        Kind;          /* ILM_SPAWN_* */
    int32_t        _pad[2];
    IlmSpawnParams Params;
    IlmFeedbackParams Feedback;   /* read when Kind == ILM_SPAWN_FEEDBACK */
    IlmPatternParams  Pattern;    /* read when Kind == ILM_SPAWN_PATTERN */
} IlmSpawnRecord;

/* One ParticleSystem.Update's worth of GPU work (Illuminant/Particles/ParticleSystem.cs:725-745):
 * spawns first, then for every chunk in [FirstChunk, FirstChunk+ChunkCount) each
 * transform in order, then the update pass.  Executed as ONE kernel launch with
 * every pass applied in registers; pass-ordering semantics are preserved per slot. */
typedef struct IlmStepDesc {
    int32_t  FirstChunk, ChunkCount;   /* ChunkCount < 0 => all chunks */
    int32_t  OpCount, SpawnCount;
    int32_t  UpdateMode;
    uint32_t Flags;
    int32_t  _pad[2];
    IlmParticleSystemUniforms System;
    IlmUpdateParams           Update;
    IlmDistanceFieldUniforms  DistanceField;  /* used when UpdateMode == ILM_UPDATE_WITH_DISTANCE_FIELD */
    IlmTransformOp            Ops[ILM_MAX_OPS];
    IlmSpawnRecord            Spawns[ILM_MAX_SPAWNS];
} IlmStepDesc;

/* ---- formats ------------------------------------------------------------ */
enum {
    ILM_SDF_UNORM16 = 0,  /* SurfaceFormat.Rgba64, Illuminant/SDF/DistanceField.cs:22 */
    ILM_SDF_FP16    = 1   /* same atlas, channels stored as IEEE half of the encoded value */
};
enum {
    ILM_GBUFFER_FLOAT4 = 0, /* SurfaceFormat.Vector4     (Illuminant/GBuffer.cs:30-38) */
    ILM_GBUFFER_HALF4  = 1  /* SurfaceFormat.HalfVector4 */
};
enum {
    ILM_LIGHTMAP_FLOAT4 = 0, /* fp32 accumulation written unrounded (parity format) */
    ILM_LIGHTMAP_HALF4  = 1, /* HalfVector4 lightmap, Illuminant/Lighting/LightingRenderer.cs:476-479 */
    ILM_LIGHTMAP_RGBA8  = 2  /* SurfaceFormat.Color lightmap (low quality) */
};

/* Which particle attribute planes to move in upload / download. */
enum {
    ILM_PLANE_POSITION     = 0,  /* PositionAndLife  (xyz, life)      ParticleSystem.cs:73-146 */
    ILM_PLANE_VELOCITY     = 1,  /* Velocity         (xyz, category)  */
    ILM_PLANE_ATTRIBUTES   = 2,  /* Chunk.Color      (rgba)           ParticleSystem.cs:159 */
    ILM_PLANE_RENDER_COLOR = 3,  /* Chunk.RenderColor (premultiplied) ParticleSystem.cs:160 */
    ILM_PLANE_RENDER_DATA  = 4   /* Chunk.RenderData (size, rotation, speed, category) ParticleSystem.cs:161 */
};

/* ---- library / context -------------------------------------------------- */

int32_t     ilm_abi_version(void);
/* Last error text for the calling thread ("" if none). */
const char* ilm_last_error(void);
/* Number of visible HIP devices (0 when there is no GPU; never fails). */
int32_t     ilm_device_count(void);

/* The numbers the kernels take from the reference's text, by the reference's own names ("ConeTrace.fxh:FULLY_SHADOWED_THRESHOLD",
 * "SpawnerCommon.fxh:randomOffset1.x modulus", ...; csrc/reference_constants.hpp).  Diagnostic, needs no GPU: tests/test_reference_pin.py
 * compares every entry with the values tools/pin_reference_constants.py extracts from the reference sources. */
int32_t     ilm_debug_reference_constant(const char* key, double* out_value);
int32_t     ilm_debug_reference_constant_count(void);
const char* ilm_debug_reference_constant_key(int32_t index);

/* One context per GPU.  Replaces the GraphicsDevice/RenderCoordinator the
 * reference threads through ParticleEngine (Illuminant/Particles/ParticleEngine.cs:95-141)
 * and LightingRenderer (Illuminant/Lighting/LightingRenderer.cs:486-560). */
int32_t ilm_ctx_create(int32_t device_id, IlmHandle* out_ctx);
/* A second (third, ...) context on the device of `ctx` for FRAMES IN FLIGHT (r05).  The reference keeps a ring of lightmaps
 * (BufferRing, Illuminant/Lighting/LightingRenderer.cs:472-485) because frame N + 1 is built while frame N renders; here a launch on a
 * context's stream starts when the previous launch of that stream has drained, so a host that wants the next frame's first waves to fill
 * the slots the previous frame's tail leaves empty renders alternate frames on sibling contexts: each has its own stream, scratch and
 * lightmaps, and -- unlike unrelated contexts -- the light passes of one (ilm_render_sphere_lights, ilm_render_particle_lights) may READ
 * the distance fields and G-buffers of another.  The library orders those reads against the owner's writes (uploads, ilm_sdf_render_slices,
 * ilm_gbuffer_render*, the field's cell rebuild -- all of which run on the OWNER's stream) with events, nothing blocks the host; writes
 * the library cannot see (ilm_sdf_device_ptr) are the host's to order.  Sibling contexts that share objects are driven from one thread.
 * Destroy like any context. */
int32_t ilm_ctx_create_sibling(IlmHandle ctx, IlmHandle* out_ctx);
int32_t ilm_ctx_destroy(IlmHandle ctx);
/* Block until all work queued on the context has finished. */
int32_t ilm_ctx_sync(IlmHandle ctx);
/* Raw hipStream_t of the context (for interop with RCCL / torch streams). */
int32_t ilm_ctx_stream(IlmHandle ctx, void** out_stream);

/* GPU-side timers around a region of queued work (hipEvent pair on the context
 * stream); elapsed time in milliseconds is returned by ilm_timer_stop after it
 * synchronises on the stop event. */
int32_t ilm_timer_start(IlmHandle ctx);
int32_t ilm_timer_stop(IlmHandle ctx, float* out_ms);

/* ---- particle engine ----------------------------------------------------- */

/* ParticleEngine ctor: chunk size + the 807x653 float4 randomness table
 * (Illuminant/Particles/ParticleEngine.cs:45-46,495-544).  The reference fills
 * it from an unseeded RNG, so it is an explicit input here.  `randomness` is a
 * host pointer to width*height float4 texels, row-major. */
#define ILM_RANDOMNESS_WIDTH  807
#define ILM_RANDOMNESS_HEIGHT 653
int32_t ilm_engine_create(IlmHandle ctx, int32_t chunk_size,
                          const IlmFloat4* randomness, int32_t rand_width, int32_t rand_height,
                          IlmHandle* out_engine);
int32_t ilm_engine_destroy(IlmHandle engine);

/* ParticleSystem: a table of chunks of chunk_size^2 slots each
 * (Illuminant/Particles/ParticleSystem.cs:148-240).  State is stored SoA, one
 * buffer set per chunk, updated in place (the reference's Previous/Current
 * ping-pong exists only to satisfy render-target hazards,
 * ParticleSystem.cs:577-616). */
int32_t ilm_system_create(IlmHandle engine, IlmHandle* out_system);
int32_t ilm_system_destroy(IlmHandle system);
/* CreateChunk (ParticleSystem.cs:349-384): appends a zero-filled chunk, returns its table index. */
int32_t ilm_system_add_chunk(IlmHandle system, int32_t* out_chunk_index);
/* Reap (ParticleLiveness.cs:120-129): removes the chunk at `chunk_index`; later chunks shift down by one. */
int32_t ilm_system_remove_chunk(IlmHandle system, int32_t chunk_index);
int32_t ilm_system_chunk_count(IlmHandle system, int32_t* out_count);

/* ParticleSystem.Spawn(initializers) upload path (ParticleSpawning.cs:13-113) /
 * AutoReadback (ParticleReadback.cs:21-71).  Host buffers are AoS float4,
 * `count` slots starting at slot `first_slot`. */
int32_t ilm_chunk_upload(IlmHandle system, int32_t chunk_index, int32_t plane,
                         const IlmFloat4* src, int32_t first_slot, int32_t count);
int32_t ilm_chunk_download(IlmHandle system, int32_t chunk_index, int32_t plane,
                           IlmFloat4* dst, int32_t first_slot, int32_t count);
/* Device pointer of one SoA component array of a chunk (component 0..19 =
 * x,y,z,life, vx,vy,vz,category, attr rgba, renderColor rgba, renderData xyzw);
 * `out_stride_floats` is the distance between component arrays.  For zero-copy
 * consumers (RCCL all-gather of positions, renderers). */
int32_t ilm_chunk_device_ptr(IlmHandle system, int32_t chunk_index, int32_t component,
                             void** out_ptr, int64_t* out_stride_floats);

/* Bind the distance field particles collide with
 * (ParticleCollision.DistanceField, ParticleConfiguration.cs:20-24); 0 unbinds. */
int32_t ilm_system_set_distance_field(IlmHandle system, IlmHandle sdf);
/* Optional life ramp texture (ParticleSystem.cs:911-941): width*height float4, POINT, U clamp / V wrap. */
int32_t ilm_system_set_life_ramp(IlmHandle system, const IlmFloat4* texels, int32_t width, int32_t height);

/* The Spawner's PositionBuffer texture (Illuminant/Particles/ParticleSpawner.cs:301-353): `count` (xyz, life) position
 * constants for spawn record `spawn_slot` (0 .. ILM_MAX_SPAWNS-1) of this system, used by records of kind
 * ILM_SPAWN_POSITION_BUFFER.  The reference pads the texture width to a multiple of 128 and addresses it with
 * index * (1 / width), POINT / CLAMP; the same arithmetic is applied here.  count == 0 releases the list. */
int32_t ilm_system_set_spawn_positions(IlmHandle system, int32_t spawn_slot, const IlmFloat4* positions, int32_t count);

/* The PatternSpawner's texture (Illuminant/Particles/SpecialSpawners.cs:19-22,255; sampler PatternSampler,
 * Illuminant/Shaders/PatternSpawner.fx:11-19: CLAMP, LINEAR min/mag, POINT mip) for spawn record `spawn_slot`, used by records of
 * kind ILM_SPAWN_PATTERN.  `texels` holds `levels` mip levels back to back, level l being max(1, width >> l) x max(1, height >> l)
 * float4 texels, row-major (the reference's mip chain comes from its texture loader, which is outside the tree: it is an explicit
 * input here; levels == 1 is a texture without mips).  tex2Dlod's explicit LOD picks level clamp(floor(lod + 0.5), 0, levels - 1).
 * levels == 0 releases the texture. */
int32_t ilm_system_set_spawn_pattern(IlmHandle system, int32_t spawn_slot, const IlmFloat4* texels,
                                     int32_t width, int32_t height, int32_t levels);

/* The hot path.  Replaces RunSpawner + the UpdateChunk loop of
 * ParticleSystem.Update (ParticleSystem.cs:725-745, 791-856): every RunTransform
 * draw for every chunk becomes one launch. */
int32_t ilm_system_step(IlmHandle system, const IlmStepDesc* desc);

/* A frame's worth of steps in one call.  The reference's Update only builds batches inside a BatchGroup (ParticleSystem.cs:33-46,682-687)
 * that the render coordinator issues later (UpdateHandler._BeforeDraw runs at issue time, ParticleTransform.cs:84-168), and systems do
 * not interact apart from feedback spawners: the Update loop over the systems of an engine
 * (Scenes/ManySystemsManySpawners.cs:41-50,78-81: 256 systems, each updated every frame) is independent work.  After the call the
 * device memory of every system and everything the host can observe are what ilm_system_step(systems[i], &descs[i]) for
 * i = 0 .. count - 1, in that order, would have left -- the planes bit for bit -- but independent items share launches: one per kernel
 * variant and round, where an item runs one round after the latest earlier item that touches a system it touches (its own, or the
 * source of a feedback record).  The same system may appear more than once; count == 0 does nothing.  All items are validated before
 * anything is queued or changed: a refusal (a handle that is not a system, a system of another engine, or whatever ilm_system_step
 * refuses, with its code) names the item in ilm_last_error() and leaves every system as it was.  Ranges large enough for the streaming
 * kernels, and every item while the context's stream is being captured, are launched one by one as ilm_system_step would. */
int32_t ilm_engine_step_batch(IlmHandle engine, const IlmHandle* systems, const IlmStepDesc* descs, int32_t count);
/* Diagnostic: the engine's latest ilm_engine_step_batch that had items -- launches of the batch kernel, rounds, and items that were
 * launched one by one instead.  Any out pointer may be NULL. */
int32_t ilm_debug_last_step_batch(IlmHandle engine, int32_t* out_launches, int32_t* out_rounds, int32_t* out_fallback_items);

/* Single-pass entry points, one per reference technique (LoadMaterials.cs:387-522);
 * chunk_index < 0 => every chunk.  Thin wrappers over ilm_system_step. */
int32_t ilm_spawn  (IlmHandle system, int32_t chunk_index, const IlmParticleSystemUniforms* sys, const IlmSpawnParams* p);
int32_t ilm_gravity(IlmHandle system, int32_t chunk_index, const IlmParticleSystemUniforms* sys, const IlmGravityParams* p);
int32_t ilm_noise  (IlmHandle system, int32_t chunk_index, const IlmParticleSystemUniforms* sys, const IlmNoiseParams* p);
int32_t ilm_fma    (IlmHandle system, int32_t chunk_index, const IlmParticleSystemUniforms* sys, const IlmFMAParams* p);
int32_t ilm_matrix_multiply(IlmHandle system, int32_t chunk_index, const IlmParticleSystemUniforms* sys, const IlmMatrixMultiplyParams* p);
int32_t ilm_spatial_noise  (IlmHandle system, int32_t chunk_index, const IlmParticleSystemUniforms* sys, const IlmSpatialNoiseParams* p);
int32_t ilm_update (IlmHandle system, int32_t chunk_index, const IlmParticleSystemUniforms* sys, const IlmUpdateParams* p,
                    const IlmDistanceFieldUniforms* df /* NULL => UpdatePositions */);
int32_t ilm_erase  (IlmHandle system, int32_t chunk_index);

/* Liveness (CountLiveParticles.fx:5-40 + ProcessLivenessInfoData, ParticleEngine.cs:224-252):
 * out_counts[i] = #{slots of chunk i with life > 0}; when saturate16 != 0 the
 * value is min(count, 65535) exactly as the reference's 16-bit additive target decodes. */
int32_t ilm_system_live_counts(IlmHandle system, uint32_t* out_counts, int32_t capacity, int32_t saturate16);

/* Counts produced inside the last ilm_system_step that had ILM_STEP_COUNT_LIVE set
 * (the ballot/popcount reduction fused into the update kernel); synchronises. */
int32_t ilm_system_step_counts(IlmHandle system, uint32_t* out_counts, int32_t capacity, int32_t saturate16);

/* Non-blocking form (the reference reads liveness back a frame or more later through
 * LivenessDataReadbackWorkItem, ParticleWorkItems.cs:98-135): *out_ready = 1 and the counts are
 * written when the last counting step has finished on the GPU, else *out_ready = 0. */
int32_t ilm_system_poll_counts(IlmHandle system, uint32_t* out_counts, int32_t capacity, int32_t saturate16, int32_t* out_ready);

/* Sensors (Sensor, Illuminant/Particles/Transforms.cs:374-486; technique CollectParticles, Illuminant/Shaders/CollectParticles.fx:10-46):
 * how many particles are inside an area.  The reference means to count with an occlusion query, i.e. the pixels PS_CollectParticles does
 * not discard; a slot is counted if and only if (CollectParticles.fx:22-37)
 *   checkCategoryFilter(velocity.w, CategoryFilter),
 *   position.w > 1  (the life against ONE, as the text has it), and
 *   1 - saturate(evaluateByTypeId(AreaType, position, AreaCenter, AreaSize, AreaRotation) / AreaFalloff) > 0.01
 * with the scalar AreaRotation promoted to (r, r, r, r) as in FMA and saturate(NaN) = 0: AreaType 0 with the effect default AreaFalloff 0
 * (0 / 0) counts every slot the first two conditions keep.  Strength is no uniform of that shader and is not read.
 * The C# never begins a query (BeforeUpdateChunk / AfterUpdateChunk return at once, Transforms.cs:479-485, ActiveQuery is never
 * assigned), so the reference's Count stays 0, and an analyzer pass would bind chunk.Previous without rotating the buffers
 * (ParticleSystem.cs:454-458); these entries count over THE STATE THE SYSTEM HOLDS WHEN THEY RUN: behind everything queued before. */
#define ILM_MAX_SENSORS 8
/* CollectParticles.fx:10-46, Transforms.cs:374-486.  Blocking: up to ILM_MAX_SENSORS sensors over chunks [first_chunk, first_chunk +
 * chunk_count) (chunk_count < 0: every chunk) in one pass that reads the position plane and the category and writes no state.
 * out_counts (host) is laid out [sensor_count][chunks of the range]; capacity is in entries; counts are not saturated.
 * ILM_ERR_INVALID_ARGUMENT: a NULL pointer, sensor_count outside 1..ILM_MAX_SENSORS, a chunk range outside the system, a capacity below
 * sensor_count x chunks, an AreaType outside 0..5, or an AreaCenter, AreaSize, AreaRotation or AreaFalloff that is not finite.  A refusal
 * leaves counts and state untouched. */
int32_t ilm_system_sense(IlmHandle system, int32_t first_chunk, int32_t chunk_count, const IlmAreaParams* sensors, int32_t sensor_count,
                         uint32_t* out_counts, int32_t capacity);
/* CollectParticles.fx:10-46, Transforms.cs:374-486.  The same count queued behind the system's pending work (a step on either of the
 * context's streams) without waiting for it -- what Sensor.AfterFrame hands to DoUpdateCount (Transforms.cs:424-477).  A second queued
 * count replaces the first.  Refuses what ilm_system_sense refuses. */
int32_t ilm_system_sense_async(IlmHandle system, int32_t first_chunk, int32_t chunk_count, const IlmAreaParams* sensors, int32_t sensor_count);
/* CollectParticles.fx:10-46, Transforms.cs:443-477 (DoUpdateCount).  Non-blocking, like ilm_system_poll_counts: *out_ready = 1 and the
 * queued count's table is written when it has finished on the GPU, else *out_ready = 0.  ILM_ERR_STATE when nothing is queued;
 * ILM_ERR_INVALID_ARGUMENT for a NULL pointer or a capacity below the queued count's entries (it stays queued). */
int32_t ilm_system_poll_sense(IlmHandle system, uint32_t* out_counts, int32_t capacity, int32_t* out_ready);

/* Ordered live-slot list of one chunk (wave64 ballot + prefix sum): writes the
 * ascending slot indices with life > 0 to `out_slots` (host, capacity entries)
 * and their number to out_count.  Consumer: particle lights (ParticleLight.fx). */
int32_t ilm_chunk_live_slots(IlmHandle system, int32_t chunk_index, uint32_t* out_slots, int32_t capacity, int32_t* out_count);

/* ---- lighting ------------------------------------------------------------- */

/* DistanceField atlas (Illuminant/SDF/DistanceField.cs:43-122): width x height
 * texels of 4 x 16 bit, row-major; `texels` is a host pointer (DistanceField.Load
 * layout, DistanceField.cs:178-213). */
int32_t ilm_sdf_create(IlmHandle ctx, int32_t atlas_width, int32_t atlas_height, int32_t format, IlmHandle* out_sdf);
int32_t ilm_sdf_upload(IlmHandle sdf, const uint16_t* texels);
/* sampleDistanceFieldEx (Illuminant/Shaders/DistanceFieldCommon.fxh:313-353) evaluated on the device at `count`
 * world positions (host array of xyz triples); writes `count` distances to out_distances (host) and synchronises.
 * Not on the reference's call path: it exposes the very sampler the particle collision and the cone trace use, so a
 * host (or a test) can query the field the kernels see. */
int32_t ilm_sdf_sample(IlmHandle sdf, const IlmDistanceFieldUniforms* df, const float* positions, int32_t count, float* out_distances);

/* Diagnostic, like ilm_sdf_sample: the cone trace samples positions that lie well inside the field through a second, table-driven form of
 * sampleDistanceFieldEx (csrc/hlsl_math.hpp, sample_inside_table) that reads the field's cell array (built from the atlas on demand and
 * rebuilt when the atlas changes).  This evaluates `count` positions the way the trace loop does:
 * out_used_table[i] = 1 where position i met that form's precondition and went through it, 0 where the general form was used.  A test
 * holds both bit-equal to the CPU restatement. */
int32_t ilm_debug_sdf_sample_inside(IlmHandle sdf, const IlmDistanceFieldUniforms* df, const float* positions, int32_t count,
                                    float* out_distances, int32_t* out_used_table);

/* Diagnostic, like ilm_sdf_sample: the cone trace's in-volume loop divides (distance + HACK_DISTANCE_OFFSET) by the cone radius
 * (ConeTrace.fxh:62) with an instruction sequence that skips the IEEE division's range scaling.  This evaluates that sequence
 * (`out_fast`) and the plain IEEE division (`out_ieee`) for `count` operand pairs on the device, so a test can hold them
 * bit-equal over the operand range the kernel admits (2^-60 <= |d| <= 2^60, |n| <= 2^60 or zero / infinite / NaN). */
int32_t ilm_debug_divide(IlmHandle ctx, const float* numerators, const float* denominators, int32_t count, float* out_fast, float* out_ieee);
/* The light pass divides by two constants -- DOT_RAMP_RANGE (LightCommon.fxh:6) and UNSHADOWED_THRESHOLD - FULLY_SHADOWED_THRESHOLD
 * (ConeTrace.fxh:19-20, :186) -- with the constants' reciprocals folded in at compile time.  This runs, for each of them, ALL 2^32
 * float bit patterns as the numerator through that sequence and through the IEEE division and counts the results that differ:
 * out_mismatches[2 i] for numerators inside the range the sequence is specified for (2^-60 <= |n| <= 2^60, zero, infinite, NaN -- the
 * kernel's numerators are saturates and sums of unit-vector components), out_mismatches[2 i + 1] outside it, for divisor
 * out_divisors[i]; *out_count divisors, out_mismatches holds 2 * capacity entries.  A test requires zero inside. */
int32_t ilm_debug_divide_by_constants(IlmHandle ctx, float* out_divisors, uint64_t* out_mismatches, int32_t capacity, int32_t* out_count);
/* ilm_system_step runs a step of the common shape (power-of-two chunk size >= 64, UpdatePositions, Gravity / area-less Noise and FMA,
 * inline spawners) through a kernel specialised for it and every other step through the kernel that interprets the descriptor; the
 * per-slot arithmetic is the same.  interpreter != 0 forces the interpreting kernel for every later step of this process (0: the
 * default choice) so that a test can hold the two bit-equal; returns the previous setting.  Environment: ILM_STEP_LEAN=0. */
int32_t ilm_debug_step_interpreter(int32_t interpreter);
/* Diagnostic: which kernel the latest ilm_system_step launch of this process ran, so that a test can tell that the case it built
 * reached the instantiation it is meant to hold bit-equal.  LEAN_CLAMP: the streaming specialised kernel's class for update passes
 * whose curves are all constant or clamp-ranged without shaping, with no velocity rotation and no life ramp. */
#define ILM_STEP_KERNEL_NONE         0   /* no step launched yet */
#define ILM_STEP_KERNEL_INTERPRETER  1
#define ILM_STEP_KERNEL_LEAN         2   /* the specialised kernel, general instantiation (cache-resident or streaming) */
#define ILM_STEP_KERNEL_LEAN_CLAMP   3
#define ILM_STEP_KERNEL_LEAN_DF      4   /* the specialised collision step */
#define ILM_STEP_KERNEL_BATCH        5   /* ilm_engine_step_batch: the interpreting kernel over the items of a launch */
int32_t ilm_debug_last_step_kernel(void);
/* A step over at least two chunks and half a million slots puts the second half of its chunk range on a second stream of the context
 * (chunks never interact, ParticleSystem.cs:743-745; every other entry point waits for both streams before it touches anything).
 * streams == 1 keeps every later step of this process on the context stream, 2 restores the default; returns the previous setting.
 * Environment: ILM_STEP_STREAMS=1.  A context whose stream was handed out by ilm_ctx_stream never splits. */
int32_t ilm_debug_step_streams(int32_t streams);
/* Diagnostic: the collision update (UpdateParticleSystemWithDistanceField.fx:29-147) is priced per sampleDistanceFieldEx call -- the
 * field lookup at the particle, one per step of its sweep, four for a bounce / redirect normal (VisualizeCommon.fxh:44-63).  enable != 0
 * makes every later ilm_system_step of this process that runs the collision update count those calls on the device; the call returns
 * the count accumulated since the previous call in *out_samples (may be NULL) and clears it.  Synchronises the context.  The count
 * costs one atomic per particle while it is on: for measurement runs only. */
int32_t ilm_debug_step_sdf_samples(IlmHandle ctx, int32_t enable, uint64_t* out_samples);
/* Diagnostic: ILM_STEP_KERNEL_LEAN_CLAMP has two bodies.  A wave whose 64 slots are all REGULAR as loaded -- alive with a finite life, a
 * category that passes every transform's filter, no NaN in the velocity's x and y -- runs the transforms and the update without the tests
 * and selects that serve other lanes, and finishes there when all 64 are still alive, finite and free of NaN afterwards; every other wave
 * runs the selecting body.  The planes get the same bits either way.  enable != 0 makes every later step of this process that runs that
 * kernel count, on the device, the waves that ran the regular body to its end (*out_regular) and those that ran its transforms but
 * finished through the selects (*out_selected); the call returns the counts accumulated since the previous call (either pointer may be
 * NULL) and clears them.  Synchronises the context.  One atomic per counted wave while it is on; one scalar load per wave while off. */
int32_t ilm_debug_step_regular_waves(IlmHandle ctx, int32_t enable, uint64_t* out_regular, uint64_t* out_selected);
/* Diagnostic: the category record of one chunk as the library holds it.  Ahead of a launch of ILM_STEP_KERNEL_LEAN_CLAMP whose transforms
 * hold no FMA the library scans the category plane of every chunk of the launch that has no current record: *out_lo / *out_hi are the
 * smallest and the largest category among the chunk's used slots (a NaN lo when one of them is a NaN), and *out_current is 1 while the
 * record is known to bound the category of every live slot of the chunk -- uploads, spawners, FMA steps, erase, chunk exchange, a
 * handed-out chunk pointer and graph capture end that.  A wave of that kernel whose chunk's bounds lie inside the step's category
 * filters does not read the category plane.  Before the first scan the bounds read 0.  Any pointer may be NULL.  Synchronises the
 * context. */
int32_t ilm_debug_chunk_category_bounds(IlmHandle system, int32_t chunk, float* out_lo, float* out_hi, int32_t* out_current);
/* Diagnostic, as ilm_debug_step_regular_waves: the waves of ILM_STEP_KERNEL_LEAN_CLAMP counted by what they did about the category
 * plane -- never loaded it (*out_skipped: the chunk's record lies inside the filters and the wave stayed regular), loaded it late
 * (*out_late: such a wave that left the regular body) or loaded it up front with the other planes (*out_upfront).  The three add up to
 * the waves of the kernel that were not skipped as never written.  Any pointer may be NULL.  Synchronises the context. */
int32_t ilm_debug_step_category_waves(IlmHandle ctx, int32_t enable, uint64_t* out_skipped, uint64_t* out_late, uint64_t* out_upfront);
/* The grid of the context's last light-pass launch (sphere or particle lights): workgroups of 256 threads (four waves each; exit-only
 * workgroups of partial tile groups included -- what a profiler's wave count sees), the largest number of workgroups per tile (light
 * split; 1 = none) and the edge of the tile groups dealt to the XCDs (0: another block -> tile map).  Measurement scripts price per-wave
 * counters with it instead of re-deriving the launch (r05). */
int32_t ilm_debug_last_light_launch(IlmHandle ctx, int32_t* out_workgroups, int32_t* out_split, int32_t* out_tile_macro);
int32_t ilm_sdf_destroy(IlmHandle sdf);
/* DistanceField.Save (Illuminant/SDF/DistanceField.cs:178-194): the atlas bytes, 8 per texel, row-major. */
int32_t ilm_sdf_download(IlmHandle sdf, uint16_t* texels);
/* The atlas in device memory, for callers that write it themselves (a torch tensor view, another library's kernel).  The light passes
 * read the field through a cell array derived from the atlas (docs/experiments.md 2): once the pointer has been handed out the library cannot know
 * when the atlas changes and re-derives ALL cells before every light pass (138 MB on a 512 x 512 x 33 field) -- until the caller takes
 * over the bookkeeping with ilm_sdf_mark_dirty. */
int32_t ilm_sdf_device_ptr(IlmHandle sdf, void** out_ptr);
/* "I have written virtual slices [first_virtual_slice, first_virtual_slice + slice_count) of the atlas" (slice_count 0: all of it).  The
 * next light pass re-derives the cells of those slices and their lower neighbour only -- the reference regenerates
 * MaximumFieldUpdatesPerFrame = 1 slice triplet per frame (Illuminant/Lighting/LightingRenderer.Configuration.cs:91,
 * LightingRenderer.DistanceField.cs:415-464) -- and from this call on the field is no longer re-derived before every pass:
 * the caller reports its writes.  ilm_sdf_upload and ilm_sdf_render_slices do this bookkeeping themselves. */
int32_t ilm_sdf_mark_dirty(IlmHandle sdf, int32_t first_virtual_slice, int32_t slice_count);
/* What the light passes do with this field: the bytes of its cell array (0: none was built), how many virtual slices the last light pass
 * re-derived and has a table for (TableSlices 0: the pass used the general sampler -- uniforms that do not tile the atlas, more than 256
 * slices, cells past 2 GiB, or no memory for them: same results, about half the speed), and the running totals. */
typedef struct IlmSdfTraceInfo {
    uint64_t CellBytes;
    uint64_t CellRebuilds;          /* light passes that re-derived at least one slice */
    uint64_t CellSlicesRebuilt;     /* virtual slices re-derived in total */
    int32_t  LastRebuiltSlices;
    int32_t  TableSlices;
    int32_t  RebuiltEveryFrame;     /* 1: the device pointer was handed out and ilm_sdf_mark_dirty has not been called since */
    int32_t  Reserved;
} IlmSdfTraceInfo;
int32_t ilm_sdf_trace_info(IlmHandle sdf, IlmSdfTraceInfo* out);

/* The field's bilinear filter: a per-texture sampler state, like a D3D sampler state -- a property of the texture, not of the context.
 *
 * Why: the reference reads the atlas through a hardware LINEAR sampler (DistanceFieldCommon.fxh:274-281, :335).  A hardware sampler
 * converts the texel-space coordinate to fixed point before it blends; eight fractional bits are the Direct3D 10+ floor, and
 * D3D9-class hardware is no finer.  The library's parity criterion is defined against fp32 weights (oracle/ilm_oracle.h), and the
 * sampled value feeds coneTrace's loop exit (ConeTrace.fxh:162-170), which is discontinuous in it.
 *
 *   ILM_SDF_FILTER_FP32   (default) the two bilinear fractions are fp32 values: sampleDistanceFieldEx as ilm_sdf_sample states it.
 *   ILM_SDF_FILTER_FIXED8 the two bilinear fractions carry 8 fractional bits.
 *
 * MODEL.  FIXED8 changes exactly one thing in sampleDistanceFieldEx as this library states it.  Everything up to and including
 *     fx = x - floor(x),  fy = y - floor(y)          (x, y: the texel-space coordinates, texel centres at +0.5)
 * is the FP32 arithmetic, so the four taps are the same taps.  Then, before the first lerp,
 *     fx = rintf(fx * 256.0f) * (1.0f / 256.0f),     fy likewise.
 * Both products are exact.  rintf rounds half to even (v_rndne_f32): 0.5 / 256 -> 0, 1.5 / 256 -> 2 / 256.  The lerp stays
 * fma(t, b - a, a).  The z blend (slice_position - floor(slice_position)) is shader arithmetic in the reference and is NOT quantised.
 * The clamp to the volume, the distance to the volume, the decode and the NaN rules are unchanged.
 *
 * DEFINED DEVIATION.  A fraction of at least 255.5 / 256 becomes the weight 1.0; the taps do NOT move to the next texel.  A true
 * fixed-point sampler would carry into the next texel, which differs from the weight 1.0 by at most the last ulp of one lerp.  The
 * reference text names no fraction width: FIXED8 is a model of a sampler this library cannot run, not the reference's measured behaviour.
 *
 * ilm_sdf_set_filter: the handle is looked up first (ILM_ERR_INVALID_HANDLE); a value other than 0 or 8 returns
 * ILM_ERR_INVALID_ARGUMENT and the state stays as it was.  The state is read when a kernel is launched: setting it neither synchronises
 * nor touches the atlas or the cell arrays (they hold taps, not weights; IlmSdfTraceInfo.CellRebuilds does not move).
 *
 * Honoured by ilm_sdf_sample, ilm_debug_sdf_sample_inside (both sampler forms) and ilm_render_sphere_lights -- counting and plain, with and
 * without a G-buffer, every atlas and lightmap format.  A FIXED8 sphere launch is served by one workgroup per tile and composes only
 * with ILM_BLEND_FP32_ACCUMULATE and the ADD / ADD blend functions: under the fp16-per-light model or another blend function the
 * call is refused.
 * Not built: every other consumer of a field.  While the field's filter is not 0, ilm_render_particle_lights, ilm_render_light_probes,
 * the directional, line, projector and volumetric passes, ilm_group_render_sphere_lights, ilm_visualize_distance_field,
 * ilm_system_set_distance_field, ilm_system_step with the collision update and ilm_engine_step_batch with such an item return
 * ILM_ERR_INVALID_ARGUMENT with a message that names the filter; the target is untouched and nothing is queued.  The collision update
 * and the other light kinds under the filter, fraction widths other than 8 and the carry into the next texel are follow-ups. */
#define ILM_SDF_FILTER_FP32    0   /* default: fp32 weights */
#define ILM_SDF_FILTER_FIXED8  8   /* the two bilinear fractions carry 8 fractional bits */
int32_t ilm_sdf_set_filter(IlmHandle sdf, int32_t fraction_bits);
int32_t ilm_sdf_get_filter(IlmHandle sdf, int32_t* out_fraction_bits);

/* ---- distance field generation ------------------------------ */

/* LightObstruction (Illuminant/Lighting/LightObstruction.cs:10-140): the DistanceFunctionVertex it packs
 * (Center, Size, Orientation quaternion -- Illuminant/Vertices.cs:105-141) + Type + IsDynamic. */
enum {
    ILM_OBSTRUCTION_ELLIPSOID = 0, ILM_OBSTRUCTION_BOX = 1, ILM_OBSTRUCTION_CYLINDER = 2,
    ILM_OBSTRUCTION_SPHEROID = 3, ILM_OBSTRUCTION_OCTAGON = 4
};
typedef struct IlmObstruction {
    float   Center[3];      int32_t Type;        /* LightObstructionType */
    float   Size[3];        int32_t IsDynamic;
    float   Orientation[4];                      /* quaternion x, y, z, w */
} IlmObstruction;

/* HeightVolumeBase (Illuminant/SDF/HeightVolume.cs:14-80) as RenderDistanceFieldHeightVolumes consumes it
 * (Illuminant/Lighting/LightingRenderer.DistanceField.cs:185-266): a polygon (a vertex range in the shared
 * xy array handed to the call) extruded over [ZBase, ZBase + Height]. */
typedef struct IlmHeightVolume {
    int32_t FirstVertex, VertexCount;
    float   ZBase, Height;
    int32_t IsDynamic;
    int32_t TopFaceEnableShadows;   /* HeightVolumeBase.TopFaceEnableShadows (:18), read by the G-buffer pass only */
    int32_t _pad[2];
} IlmHeightVolume;

#define ILM_DISTANCE_LIMIT 520.0f   /* LightingRenderer.DistanceLimit, Illuminant/Lighting/LightingRenderer.cs:316 */

/* What RenderDistanceFieldSliceTriplet binds for a group of slice triplets
 * (Illuminant/Lighting/LightingRenderer.DistanceField.cs:80-152): the atlas layout of the DistanceField
 * constructor (Illuminant/SDF/DistanceField.cs:43-122) and SliceIndexToZ's inputs (:32-35). */
typedef struct IlmDistanceFieldRenderDesc {
    int32_t VirtualWidth, VirtualHeight;
    float   VirtualDepth, ZOffset;
    int32_t SliceWidth, SliceHeight, SliceCount, ColumnCount;
    int32_t RowCount;
    float   MaximumEncodedDistance;
    float   InvScaleFactorX, InvScaleFactorY;    /* VirtualWidth / SliceWidth, VirtualHeight / SliceHeight (Uniforms.cs:108-109) */
    int32_t DynamicFlagFilter;                   /* -1: every obstruction (plain DistanceField); 0: static only; 1: dynamic only */
    int32_t _pad[3];
} IlmDistanceFieldRenderDesc;

/* RenderDistanceFieldPartition's inner loop (LightingRenderer.DistanceField.cs:415-464) for `triplet_count` slice
 * triplets at once: for each first virtual slice s = first_virtual_slices[i] (a multiple of 3) the physical slice
 * s / 3 is cleared -- to zero, or to the texels of `clear_source` (the DynamicDistanceField's static texture,
 * ClearDistanceField.fx:30-44) -- and every obstruction / height volume passing the dynamic-flag filter is
 * rasterised into it with the analytic distance functions of DistanceFunction.fx:33-115 (quad of half-size
 * max|Size| + MaximumEncodedDistance + 4, :24-25) / DistanceField.fx:75-115, encoded (DistanceFieldCommon.fxh:264-266)
 * and MAX-blended (LoadMaterials.cs:164-176); texel RGBA = virtual slices s .. s+3.
 * `obstructions`, `volumes`, `polygon_xy` (x,y pairs) and `first_virtual_slices` are host arrays.  Asynchronous.
 * InvScaleFactorX, InvScaleFactorY, VirtualDepth and ZOffset of `desc` must be finite: ILM_ERR_INVALID_ARGUMENT otherwise, with
 * nothing queued and the atlas untouched. */
int32_t ilm_sdf_render_slices(IlmHandle sdf, IlmHandle clear_source, const IlmDistanceFieldRenderDesc* desc,
                              const int32_t* first_virtual_slices, int32_t triplet_count,
                              const IlmObstruction* obstructions, int32_t obstruction_count,
                              const IlmHeightVolume* volumes, int32_t volume_count,
                              const float* polygon_xy, int32_t polygon_vertex_count);

/* G-buffer (Illuminant/GBuffer.cs): width x height texels (encNormal.xy, relativeY, encodedZ). */
int32_t ilm_gbuffer_create(IlmHandle ctx, int32_t width, int32_t height, int32_t format, IlmHandle* out_gbuffer);
int32_t ilm_gbuffer_upload(IlmHandle gbuffer, const void* texels);
int32_t ilm_gbuffer_destroy(IlmHandle gbuffer);
int32_t ilm_gbuffer_download(IlmHandle gbuffer, void* texels);

/* What RenderGBuffer binds in its non-2.5D form (Illuminant/Lighting/LightingRenderer.GBuffer.cs:127-203): the view transform
 * (Position = the pending field viewport position, Scale = viewportScale * RenderScale, :131-135) and the ground plane's inputs
 * (RenderGroundPlane, :271-299). */
typedef struct IlmGBufferRenderDesc {
    float   ViewportPosition[2];
    float   ViewportScale[2];
    float   GroundZ;
    int32_t RenderGroundPlane;        /* Configuration.RenderGroundPlane: false lifts the plane by 99999 (:280-286) */
    int32_t EnableGroundShadows;      /* Environment.EnableGroundShadows */
    int32_t _pad;
} IlmGBufferRenderDesc;

/* RenderGBuffer without TwoPointFiveD, billboards or user content: clear to transparent, the ground plane
 * (technique GroundPlane, Illuminant/Shaders/GBuffer.fx:7-19,57-70) and the top face of every height volume drawn with the same
 * material from the lowest to the highest (RenderGBufferVolumes, :205-219), encoded by encodeGBufferSample
 * (Illuminant/Shaders/GBufferShaderCommon.fxh:10-35).  The top-face meshes come from Fracture's Geometry.Triangulate
 * (SDF/HeightVolume.cs:126-133), which is outside the tree; a triangulation covers exactly the polygon's interior, so coverage
 * is decided per pixel centre with an even-odd point-in-polygon test instead.  Host arrays; asynchronous.
 * ViewportScale may be negative (a mirrored view); a zero component is ILM_ERR_INVALID_ARGUMENT.  A NaN scale leaves every pixel
 * centre outside every volume: the ground plane alone. */
int32_t ilm_gbuffer_render(IlmHandle gbuffer, const IlmGBufferRenderDesc* desc,
                           const IlmHeightVolume* volumes, int32_t volume_count,
                           const float* polygon_xy, int32_t polygon_vertex_count);

/* ---- RenderGBuffer with the host's own meshes: 2.5D (top + front faces under a depth test) and billboards ------------------
 * The reference's host builds triangle lists -- HeightVolume.Mesh3D / GetFrontFaceMesh3D (Illuminant/SDF/HeightVolume.cs:106-224)
 * and the billboard quads of RenderGBufferBillboards (Illuminant/Lighting/LightingRenderer.GBuffer.cs:330-478) -- and hands them
 * to the GPU; those builders stay host code, the arrays cross the boundary as they are. */

/* HeightVolumeVertex, Illuminant/Vertices.cs:41-46 (Sequential, Pack = 4: 36 bytes) */
typedef struct IlmHeightVolumeVertex {
    float Position[3];
    float Normal[3];
    float ZRange[2];
    float EnableShadows;
} IlmHeightVolumeVertex;

/* BillboardVertex, Illuminant/Vertices.cs:75-81 (Sequential, Pack = 4: 48 bytes) */
typedef struct IlmBillboardVertex {
    float ScreenPosition[2];
    float TexCoord[2];
    float WorldPosition[3];
    float Normal[3];
    float DataScaleAndDynamicFlag[2];
} IlmBillboardVertex;

enum {
    ILM_BILLBOARD_MASK         = 0,  /* BillboardType.Mask        -> technique MaskBillboard  (GBufferBitmap.fx:29-59,115-122) */
    ILM_BILLBOARD_GBUFFER_DATA = 1   /* BillboardType.GBufferData -> technique GDataBillboard (GBufferBitmap.fx:61-113,124-131) */
};

/* One PrimitiveDrawCall of RenderGBufferBillboards (LightingRenderer.GBuffer.cs:392-409): a run of quads sharing a texture and a
 * type.  Texture = a lightmap-class texture of the same context (ilm_lightmap_create + ilm_lightmap_upload; RGBA8 = SurfaceFormat.Color,
 * float4 / half4 accepted), sampled POINT / CLAMP (_SetTextureForGBufferBillboard, :301-307); 0 = no texture bound, which Direct3D 9
 * samples as (0, 0, 0, 1) -- "the mask is an opaque rectangle" (Billboard.cs:93). */
typedef struct IlmBillboardRun {
    IlmHandle Texture;
    int32_t   FirstQuad, QuadCount;   /* quads [FirstQuad, FirstQuad + QuadCount) of the vertex array, 4 vertices each (TL, TR, BR, BL) */
    int32_t   Type;                   /* ILM_BILLBOARD_* */
    int32_t   _pad;
} IlmBillboardRun;

/* What RenderGBuffer and _SetupGBufferGroundPlane bind (LightingRenderer.GBuffer.cs:102-157): the view transform, the Environment
 * uniforms the three techniques read (Uniforms.cs:15-24: GroundZ, ZToYMultiplier, RenderScale), DistanceFieldExtent.z and the two
 * self-occlusion hacks (ComputeSelfOcclusionHack / ComputeZSelfOcclusionHack, :62-80 -- host arithmetic, passed in). */
typedef struct IlmGBufferMeshDesc {
    float   ViewportPosition[2];
    float   ViewportScale[2];
    float   GroundZ;
    float   ZToYMultiplier;
    float   RenderScale[2];
    float   DistanceFieldExtentZ;
    float   SelfOcclusionHack;
    float   ZSelfOcclusionHack;
    int32_t TwoPointFiveD;            /* Configuration.TwoPointFiveD */
    int32_t RenderGroundPlane;
    int32_t EnableGroundShadows;
    int32_t _pad[2];
} IlmGBufferMeshDesc;

/* RenderGBuffer (LightingRenderer.GBuffer.cs:127-203) in draw order -- clear (colour 0, depth 0); the ground plane; then
 *   TwoPointFiveD = 1: every triangle of `top` with technique HeightVolume, then every triangle of `front` with technique
 *     HeightVolumeFace (GBuffer.fx:21-55,72-103), both under DepthBufferFunction GreaterEqual with depth writes on a 24-bit depth
 *     buffer, depth = z / DistanceFieldExtent.z (LightingRenderer.cs:539-551, GBuffer.cs:30-38; RenderTwoPointFiveDVolumes, :221-269 --
 *     the caller concatenates the volumes' meshes in its OrderByDescending(ZBase + Height) order);
 *   TwoPointFiveD = 0: every triangle of `top` with the ground plane's technique in the caller's OrderBy(ZBase + Height) order
 *     (RenderGBufferVolumes, :205-219); `front` must be empty;
 * then the billboard runs: all Mask runs in array order, then all GBufferData runs (layerIndex, layerIndex + 1, :371-392), no
 * depth test.  Triangles cover a pixel when its centre is inside under the top-left rule on positions snapped to 1/256 pixel
 * (both windings: CullMode.None); vertex attributes are interpolated with the barycentric weights of the snapped triangle;
 * fragments whose depth leaves [0, 1] are clipped.  Host arrays; asynchronous. */
int32_t ilm_gbuffer_render_meshes(IlmHandle gbuffer, const IlmGBufferMeshDesc* desc,
                                  const IlmHeightVolumeVertex* top_vertices, int32_t top_vertex_count,
                                  const IlmHeightVolumeVertex* front_vertices, int32_t front_vertex_count,
                                  const IlmBillboardVertex* billboard_vertices, int32_t billboard_vertex_count,
                                  const IlmBillboardRun* runs, int32_t run_count);

/* Lightmap render target (BufferRing of lightmaps, LightingRenderer.cs:472-485).
 * If external_device_ptr != NULL the lightmap aliases caller-owned device memory
 * of width*height*bytes_per_texel bytes (e.g. a torch tensor that RCCL gathers). */
int32_t ilm_lightmap_create(IlmHandle ctx, int32_t width, int32_t height, int32_t format,
                            void* external_device_ptr, IlmHandle* out_lightmap);
int32_t ilm_lightmap_download(IlmHandle lightmap, void* dst, int32_t first_row, int32_t row_count);
/* Texture2D.SetData on rows [first_row, first_row + row_count) in the lightmap's own texel format (the albedo texture of the with-albedo
 * resolve is such a texture). */
int32_t ilm_lightmap_upload(IlmHandle lightmap, const void* src, int32_t first_row, int32_t row_count);
int32_t ilm_lightmap_device_ptr(IlmHandle lightmap, void** out_ptr);
int32_t ilm_lightmap_destroy(IlmHandle lightmap);

typedef struct IlmRenderStats {
    uint64_t SdfSamples;       /* sampleDistanceFieldEx calls executed (AO + cone-trace steps) */
    uint64_t PixelLightPairs;  /* pixel x light pairs inside a light's raster footprint */
    uint64_t TracedPairs;      /* pairs that ran the cone trace */
} IlmRenderStats;

/* The sphere-light pass of LightingRenderer.RenderLighting
 * (Illuminant/Lighting/LightingRenderer.cs:1004-1169 + technique SphereLight,
 * Illuminant/Shaders/SphereLight.fx:7-46): lightmap[row_begin..row_end) =
 * ambient + sum over lights, in light order.  gbuffer == 0 => ground plane
 * (LightCommon.fxh:130-141); sdf == 0 => no distance field.  `lights` is a host
 * array.  stats may be NULL; when non-NULL the instrumented (counting) kernel
 * variant runs and the call synchronises.
 * ambient == NULL: the lights are ADDED to what the lightmap holds -- a further light group of the same frame (the reference draws
 * one batch group per LightTypeRenderStateKey, e.g. per ramp texture, onto the same target, LightingRenderer.cs:1004-1169).
 * With a ramp texture bound (ilm_ctx_set_light_ramp) the technique is SphereLightWithDistanceRamp (SphereLight.fx:48-86,
 * SphereLightPixelEpilogueWithRamp, SphereLightCore.fxh:99-119). */
int32_t ilm_render_sphere_lights(IlmHandle ctx,
                                 const IlmLightVertex* lights, int32_t light_count,
                                 const IlmEnvironment* env,
                                 const IlmDistanceFieldUniforms* df,
                                 IlmHandle gbuffer, IlmHandle sdf,
                                 const float ambient[4],
                                 IlmHandle lightmap, int32_t row_begin, int32_t row_end,
                                 IlmRenderStats* stats);

/* The directional-light pass of LightingRenderer.RenderLighting: techniques DirectionalLight / DirectionalLightWithRamp
 * (Illuminant/Shaders/DirectionalLight.fx:19-161), one quad per light, added onto the lightmap like every other light type.  The
 * arguments mean what they mean for ilm_render_sphere_lights: gbuffer == 0 => ground plane, sdf == 0 => no distance field, ambient ==
 * NULL => the lights are ADDED to what rows [row_begin, row_end) hold, ambient != NULL => every pixel of the rows is cleared to it first
 * (whatever light_count is, 0 included), stats != NULL => the counting variant runs and the call synchronises.  Any light_count >= 0.
 * ilm_ctx_set_lightmap_blend applies (fp32 registers over this call's lights in list order, the sum added to the base value and rounded
 * once at the store; or the fp16-per-light model), and so does ilm_ctx_set_light_ramp: while a ramp is bound the technique is
 * DirectionalLightWithRamp, opacity = SampleFromRamp(opacity) (RampCommon.fxh:15-17: channel r at v = 0).
 * Vertex layout, as RenderDirectionalLightSource fills it (Illuminant/Lighting/LightingRenderer.cs:1256-1307, LightVertex
 * Illuminant/Lighting/Vertices.cs:22-30):
 *   LightPosition1.xy / LightPosition2.xy   Bounds.TopLeft / BottomRight, or -99999 / +99999 without bounds
 *   Color1                                  Color.rgb, Color.a * Opacity * intensityScale
 *   Color2                                  (Direction, 1), or all 0 for a null direction (an ambient light in an area)
 *   LightProperties                         CastsShadows ? 1 : 0, ShadowTraceLength, ShadowSoftness, ShadowRampRate
 *   MoreLightProperties                     AmbientOcclusionRadius, ShadowDistanceFalloff or -99999, 0, AmbientOcclusionOpacity
 *   EvenMoreLightProperties.x               ShadowFilter
 * (LightPosition3 and the other members are not read.)
 * Coverage -- the reference leaves it to the rasteriser; here: pixel (x, y) lies in a light's footprint iff its centre (x + 0.5,
 * y + 0.5) lies in [x0, x1) x [y0, y1), with x0 = (LightPosition1.x - ViewportPosition.x) * (ViewportScale.x * RenderScale.x), x1 the same
 * from LightPosition2.x, y0 / y1 likewise: fp32, one rounding per operation, the scales multiplied first as
 * DirectionalLightVertexShader writes it (DirectionalLight.fx:32-34; ViewportScale = GBufferTexelSizeAndMisc.zw, RenderScale =
 * ZAndScale.zw).  A light with LightPosition1 > LightPosition2 on an axis, or a NaN in either, is refused: ILM_ERR_INVALID_ARGUMENT.
 * Discards: a pixel outside the footprint, a fullbright pixel, one the shadow filter rejects and one that is not visible (G-buffer x <=
 * -9999, clip(), :91) get nothing from the light -- no rgb and no + 1 on alpha.  There is no opacity discard (unlike SphereLight.fx): a
 * visible pixel whose opacity is 0 still adds alpha 1.
 * Statistics: PixelLightPairs = pairs inside a footprint; TracedPairs = pairs with traceShadows (:73) and a bound field (sdf != 0,
 * Extent.x > 0); SdfSamples = ambient-occlusion + cone-trace samples.
 * The light-probe techniques (DirectionalLightProbe*) are ilm_render_directional_light_probes.  Not built: the group entry point. */
int32_t ilm_render_directional_lights(IlmHandle ctx,
                                      const IlmLightVertex* lights, int32_t light_count,
                                      const IlmEnvironment* env,
                                      const IlmDistanceFieldUniforms* df,
                                      IlmHandle gbuffer, IlmHandle sdf,
                                      const float ambient[4],
                                      IlmHandle lightmap, int32_t row_begin, int32_t row_end,
                                      IlmRenderStats* stats);

/* The line-light pass of LightingRenderer.RenderLighting: technique LineLight (Illuminant/Shaders/LineLight.fx:7-42 over
 * LineLightCore.fxh:17-120), one quad per light, added onto the lightmap like every other light type.  The arguments mean what they mean
 * for ilm_render_directional_lights: gbuffer == 0 => ground plane, sdf == 0 => no distance field, ambient == NULL => the lights are ADDED
 * to what rows [row_begin, row_end) hold, ambient != NULL => every pixel of the rows is cleared to it first (whatever light_count is, 0
 * included), stats != NULL => the counting variant runs and the call synchronises.  Any light_count >= 0.  ilm_ctx_set_lightmap_blend
 * applies (fp32 registers over this call's lights in list order, the sum added to the base value and rounded once at the store; or the
 * fp16-per-light model).  A bound light ramp (ilm_ctx_set_light_ramp) is neither read nor changed: the reference has no LineLightWithRamp.
 * Vertex layout, as RenderLineLightSource fills it (Illuminant/Lighting/LightingRenderer.cs:1309-1337):
 *   LightPosition1.xyz / LightPosition2.xyz StartPosition / EndPosition
 *   Color1 / Color2                         StartColor / EndColor, alpha already multiplied by Opacity * intensityScale
 *   LightProperties                         Radius, ramp length, RampMode, casts ? 1 : 0.  The host writes 0 for the ramp length (:1324);
 *                                           the shader reads it (createTraceConfig), so what is given is honoured.  RampMode is not read.
 *   MoreLightProperties                     AmbientOcclusionRadius, ShadowDistanceFalloff or -99999, FalloffYFactor,
 *                                           AmbientOcclusionOpacity; .y and .z are not read by the pixel shader.
 * (EvenMoreLightProperties and LightPosition3 are not read.)
 * Coverage: every pixel of the rows.  The vertex shader's quad is min(P) - 9999 .. max(P) + 9999 (LineLightCore.fxh:142-152: "how the
 * hell do we compute bounds for this"); that it covers the frame is the definition here -- there is no footprint test.
 * Per pixel (LineLight.fx:7-42, LineLightCore.fxh:70-120), p = the shaded point, n = its normal:
 *   a fullbright pixel is discarded (:25-29); casts *= enableShadows (:31);
 *   distanceOpacity = computeLineLightOpacity (FBPBR.fxh:53-101), which also yields u = saturate(dot(p - start, delta) / dot(delta,
 *   delta)) and the closest point start + u * delta (closestPointOnLineSegment3, DistanceFieldCommon.fxh:151-155);
 *   the pixel is discarded unless distanceOpacity > 0 && p.x > -9999 (clip(), :90-93);
 *   AO as for directional lights: radius * max(0, n.z), sampled only when >= 0.5 and a field is bound;
 *   preTraceOpacity = distanceOpacity * aoOpacity; the pair traces iff casts != 0 && preTraceOpacity >= 0.75 / 255 (:104);
 *   color = lerp(Color1, Color2, u) on all four components; rgb added = (color.rgb * color.a) * (preTraceOpacity * coneOpacity), alpha + 1.
 * Unlike the directional pass, a pixel whose distance opacity is 0 IS discarded: it gets no rgb and no + 1 on alpha.
 * The opacity term is a DEFINED function, fp32 with one rounding per + - * / sqrt in the order the HLSL writes it (dot = (x + y) + z,
 * normalize = three IEEE divisions by the length, cross as written), and acos = acos_defined: sqrt(1 - |x|) * P7(|x|) with Abramowitz &
 * Stegun 4.4.46's coefficients rounded to fp32, Horner form without fma, pi - r for x < 0 -- within 2^-21 of the real acos on [-1, 1],
 * NaN outside it.  The solid angle g0 + g1 + g2 + g3 - 2 pi (FBPBR.fxh:46-50) cancels, so a library acos that differs by an ulp between
 * host and device would move the decisions above, which feed exact statistics; parity with fxc's own acos expansion stays unpinned.
 * Degenerate geometry is defined by that arithmetic and not special-cased: normalize(0) is 0 / 0 = NaN, the NaN reaches the final
 * saturate, and saturate(NaN) = min(max(NaN, 0), 1) = 0.  So each of these gives distance opacity 0 and a discard, with no trace and no
 * sample: Radius == 0 (the reference's default, LightSource.cs:325), a pixel on the segment's axis (up = cross(left, forward) = 0),
 * start == end, a NaN position.  No memory access depends on any of them.
 * The trace (lineConeTrace, LineLightCore.fxh:17-68): three TraceStates share the origin p + 1.5 * n and aim at start + saturate(u - o) *
 * delta, start + u * delta and start + saturate(u + o) * delta, o = max(saturate((Radius + 1) / |delta|), 0.03); each is initialised
 * with lightRadius = Radius (length = max(|target - origin| - Radius, 1), position 0.5, visibility 1); config = createTraceConfig((Radius,
 * ramp length), (1, falloff)): maxRadius = clamp(Radius, 0.33, MaxConeRadius), growth = maxRadius / max(ramp length, 16).  Every
 * iteration advances ALL three rays with coneTraceAdvanceEx (ConeTrace.fxh:84-96: position = min(position + step, length), liveness
 * factor saturate(visibility - 0.075) * saturate((length - position) * 100)), then stepsRemaining-- and liveness = stepsRemaining * (the
 * sum of the three).  A ray that has reached its end keeps sampling at its end point and keeps lowering its own visibility while
 * another ray lives: that is the reference's arithmetic.  visibility = min((va + vb + vc) / 3, stepsRemaining / 2), then the sphere
 * light's threshold and pow; unlike coneTrace there is no stepsRemaining == 0 fix-up.  The sample position origin + direction * position
 * and the cone radius growth * position + 0.33 are fused multiply-adds, as in the other passes.
 * Statistics: PixelLightPairs = pairs that reach the opacity term (every pair of a pixel of the rows that is not fullbright);
 * TracedPairs = pairs that trace with a bound field (sdf != 0, Extent.x > 0); SdfSamples = the AO sample + 3 per loop iteration.
 * LineLightProbe is ilm_render_line_light_probes.  Not built: the group entry point, an in-volume fast loop. */
int32_t ilm_render_line_lights(IlmHandle ctx,
                               const IlmLightVertex* lights, int32_t light_count,
                               const IlmEnvironment* env,
                               const IlmDistanceFieldUniforms* df,
                               IlmHandle gbuffer, IlmHandle sdf,
                               const float ambient[4],
                               IlmHandle lightmap, int32_t row_begin, int32_t row_end,
                               IlmRenderStats* stats);

/* ProjectorLightSource.TextureRef of the light group rendered by the FOLLOWING ilm_render_projector_lights calls (the reference groups
 * projector lights by texture, one LightTypeRenderStateKey each, and binds it as the group's RampTexture; sampler
 * ProjectorTextureSampler, Illuminant/Shaders/ProjectorLightCore.fxh:11-18: LINEAR, WRAP on both axes): width * height float4 texels,
 * row-major, ONE level.  Any size from 1 x 1 up is a texture; width == 0 unbinds.  A binding of its own: ilm_ctx_set_light_ramp's (U
 * CLAMP, a 1 x 1 ramp is none) is neither read nor changed by it, nor by ilm_render_projector_lights.  The texels are copied: the call
 * waits for the context's queued work (an earlier pass may still read the texels it replaces) and copies synchronously, so a host keeps a
 * texture bound over as many calls and frames as it serves and binds only when the group's texture changes. */
int32_t ilm_ctx_set_projector_texture(IlmHandle ctx, const IlmFloat4* texels, int32_t width, int32_t height);

/* The same binding with a mip chain (a Texture2D with LevelCount > 1; the reference's texture loader, which builds the chain, is outside
 * the tree: the levels are an input, as for ilm_system_set_spawn_pattern, whose layout and limits these are).  `texels` holds `levels`
 * levels back to back, level l being max(1, width >> l) x max(1, height >> l) float4 texels, row-major; levels in [0, 16] (else
 * ILM_ERR_OUT_OF_RANGE), sides in [1, 16384] and texels != NULL when levels > 0 (else ILM_ERR_INVALID_ARGUMENT).  levels == 0 or
 * width == 0 (with height == 0) unbinds; levels == 1 IS ilm_ctx_set_projector_texture(ctx, texels, width, height).  There is one projector
 * binding: either setter replaces what the other bound.  Copy and ordering as above (waits for the context's queued work, copies
 * synchronously); a refused call leaves the binding as it was; the ramp binding is neither read nor changed.  How the levels are read:
 * "Texture fetch" under ilm_render_projector_lights. */
int32_t ilm_ctx_set_projector_texture_mips(IlmHandle ctx, const IlmFloat4* texels, int32_t width, int32_t height, int32_t levels);

/* The projector-light pass of LightingRenderer.RenderLighting: technique ProjectorLight (Illuminant/Shaders/ProjectorLight.fx:14-56 over
 * ProjectorLightCore.fxh), one quad per light, added onto the lightmap like every other light type.  The arguments mean what they mean
 * for ilm_render_directional_lights: gbuffer == 0 => ground plane, sdf == 0 => no distance field (which is the technique
 * ProjectorLightWithoutDistanceField), ambient == NULL => the lights are ADDED to what rows [row_begin, row_end) hold, ambient != NULL =>
 * every pixel of the rows is cleared to it first (whatever light_count is, 0 included), stats != NULL => the counting variant runs and
 * the call synchronises.  Any light_count from 0 to 2^24 (more are refused); light_count > 0 with no projector texture bound is refused (ILM_ERR_INVALID_ARGUMENT:
 * the reference skips a light whose texture is null before it packs it).  ilm_ctx_set_lightmap_blend applies (fp32 registers over this
 * call's lights in list order, the sum added to the base value and rounded once at the store; or the fp16-per-light model).
 * Vertex layout, as RenderProjectorLightSource fills it (Illuminant/Lighting/LightingRenderer.cs:1386-1446):
 *   LightPosition1, LightPosition2, Color1, Color2   rows 1-4 of the inverse matrix M (world -> texture space); Color2.w carries the mip
 *                                           bias and the matrix's m44 is 1, as the vertex shader restores it (ProjectorLightCore.fxh:244-245)
 *   LightPosition3                          (Origin, 1), or all 0 without an origin
 *   LightProperties                         Radius, RampLength, RampMode (not read), shadows ? 1 : 0
 *   MoreLightProperties                     AmbientOcclusionRadius, Opacity * intensityScale, clamp (1 = not Wrap), AmbientOcclusionOpacity
 *   EvenMoreLightProperties                 the texture region x1, y1, x2, y2
 * Per pixel, fp32 with one rounding per + - * / sqrt, p = the shaded point, region = EvenMoreLightProperties:
 *   t_c = ((p.x * m1c + p.y * m2c) + p.z * m3c) + 1 * m4c for c = x, y, z, w; t.xyz /= t.w (IEEE divisions); t.xy += region.xy;
 *   t.z = max(0, t.z); clamped = clamp(t.xyz, (region.xy, 0), (region.zw, 1));
 *   distanceToVolume = min(length(clamped - t), 0.001f) * (1.0f / 0.001f);
 *   distanceOpacity = clamp > 0.5 ? max(1 - distanceToVolume, 0) : 1;
 *   visible = distanceOpacity > 0 && p.x > -9999 && MoreLightProperties.y > 0;
 *   t.xy = t.xy + (clamped.xy - t.xy) * clamp;
 *   normalOpacity = 1 + (computeNormalFactor(normalize(p - origin.xyz), normal) - 1) * origin.w -- the sphere pass's DOT_OFFSET,
 *   DOT_RAMP_RANGE, DOT_EXPONENT and its rule for a zero normal (factor 1), IEEE divisions.  DEFINED DEVIATION: when origin.w == 0
 *   exactly the factor is not evaluated and normalOpacity is 1 -- the lerp's value for every finite factor; it removes the reference's
 *   NaN at a shaded point equal to a zero origin.
 *   AO as for directional lights: radius * max(0, normal.z), sampled only when >= 0.5 and a field is bound;
 *   opacity = ((distanceOpacity * normalOpacity) * MoreLightProperties.y) * aoOpacity, times the cone opacity when the pair traces:
 *   LightProperties.w * enableShadows != 0 and that opacity >= 0.75 / 255 -- the sphere light's coneTrace from p + 1.5 * normal towards
 *   origin.xyz with lightRamp = (Radius, RampLength) and cone growth 1;
 *   rgb added = (tex.rgb * tex.a) * opacity, alpha + 1, with tex = the texture at (t.x, t.y).
 * Texture fetch: tex2Dlod(ProjectorTextureSampler, (u, v, 0, lod)) with lod = Color2.w (the mip bias RenderProjectorLightSource packs,
 * LightingRenderer.cs:1417-1428) and MipFilter, MinFilter, MagFilter all LINEAR (ProjectorLightCore.fxh:9-18), over the L levels bound
 * (L = 1 after ilm_ctx_set_projector_texture; mip chains come from ilm_ctx_set_projector_texture_mips).  fp32, one rounding per operation:
 *   c = fminf(fmaxf(lod, 0), L - 1) -- a NaN lod becomes 0 through fmaxf, an infinite one clamps;
 *   l0 = (int)floorf(c); f = c - floorf(c); l1 = min(l0 + 1, L - 1);
 *   c0 = the bilinear fetch below on level l0, with that level's own width and height;
 *   f == 0: tex = c0 and level l1 is NOT read (one level, an integral lod and a clamped lod are exact; no texel of l1 can show);
 *   otherwise c1 = the same fetch on level l1 and tex = c0 + (c1 - c0) * f per component.
 * With L = 1 every lod reads level 0, as a sampler does for a texture without a chain.  DEFINED DEVIATION: a hardware sampler's
 * trilinear (and bilinear) weights are fixed-point; these are the fp32 values above, and parity with a D3D9 sampler's rounding is not
 * pinned.  The bilinear fetch on a level of width x height texels -- LINEAR: s = u * width -
 * 0.5, first tap floor(s), weight s - floor(s), second tap = the integer first tap + 1; WRAP: both taps modulo the size in exact
 * integer arithmetic for every finite coordinate, tap 0 for a non-finite one; the same on v.  Every index lies inside the level.
 * Discards: a pixel outside the footprint, a fullbright pixel and one that is not `visible` get nothing from the light -- no rgb and
 * no + 1 on alpha.  No shadow filter (the shader never calls it) and no opacity discard: a visible pixel whose opacity is 0 adds alpha 1.
 * Coverage -- the reference leaves it to the rasteriser; here, as for directional lights: pixel (x, y) is covered iff its centre lies
 * in the half-open screen rectangle [x0, x1) x [y0, y1) of the light's world rectangle, mapped by (world - ViewportPosition) *
 * (ViewportScale * RenderScale), the scales multiplied first.  With clamp <= 0.5 the world rectangle is (-9999, -9999) .. (9999, 9999).
 * With clamp > 0.5 it is the vertex shader's bounding box (ProjectorLightCore.fxh:251-278), fp32 in the order the shader writes it,
 * once per light: invertMatrix of the four rows; the four corners lerp(0, region.zw - region.xy, corner) projected at z = 0 and z = 1,
 * each divided by its w; min / max (minNum / maxNum) over the eight points from 999999 / -999999; the quad's corners lerp(tl, br, 0 / 1);
 * y padded by -/+ MaximumZ * ZToYMultiplier.  A light whose rectangle comes out NaN or inverted on an axis covers nothing.
 * Statistics: PixelLightPairs = pairs inside a footprint and the image; TracedPairs = pairs that trace with a bound field (sdf != 0,
 * Extent.x > 0); SdfSamples = ambient-occlusion + cone-trace samples.  Texture taps are not counted, with one level or many.
 * Not built: the light-probe technique -- ProjectorLightProbe.fx's pixel shader reads projectorOrigin : TEXCOORD6 (:48), which its vertex
 * shader never writes (:14-34), and the origin drives both the trace target and the normal term: the text does not define the result;
 * ProjectorLightWithoutDistanceField as a technique of its own (sdf == 0 is it); the group entry point. */
int32_t ilm_render_projector_lights(IlmHandle ctx,
                                    const IlmLightVertex* lights, int32_t light_count,
                                    const IlmEnvironment* env,
                                    const IlmDistanceFieldUniforms* df,
                                    IlmHandle gbuffer, IlmHandle sdf,
                                    const float ambient[4],
                                    IlmHandle lightmap, int32_t row_begin, int32_t row_end,
                                    IlmRenderStats* stats);

/* The volumetric-light pass of LightingRenderer.RenderLighting: techniques VolumetricLight and ShadowedVolumetricLight
 * (Illuminant/Shaders/VolumetricLight.fx:7-51, ShadowedVolumetricLight.fx:7-52 over VolumetricLightCore.fxh), one quad per light, added
 * onto the lightmap like every other light type.  The arguments mean what they mean for ilm_render_directional_lights: gbuffer == 0 =>
 * ground plane, sdf == 0 => no distance field, ambient == NULL => the lights are ADDED to what rows [row_begin, row_end) hold, ambient !=
 * NULL => every pixel of the rows is cleared to it first (whatever light_count is, 0 included), stats != NULL => the counting variant runs
 * and the call synchronises.  Any light_count >= 0.  ilm_ctx_set_lightmap_blend applies (both models).  A bound light ramp or projector
 * texture is neither read nor changed.  One entry point serves both techniques: they differ in LightProperties.w alone (VolumetricLight
 * sets it to 0, the render-state key selects by CastsShadows, LightingRenderer.cs:190-193), and the vertex's w already carries that.
 * Vertex layout, as RenderVolumetricLightSource fills it (Illuminant/Lighting/LightingRenderer.cs:1339-1384):
 *   LightPosition1 / LightPosition2         (start, StartRadius) / (end, EndRadius); for Shape 0 and 2 the host has already turned
 *                                           [start, end] into [centre, half-extent]
 *   LightPosition3.xyz                      LightDirection, or 0
 *   Color1                                  Color, alpha already multiplied by Opacity * intensityScale (Color2 is the same; not read)
 *   LightProperties                         Volumetricity, RampLength, RampMode, casts && field ? 1 : 0
 *   MoreLightProperties                     AmbientOcclusionRadius, ShadowDistanceFalloff or -99999, FalloffYFactor,
 *                                           AmbientOcclusionOpacity; .y and .z are not read
 *   EvenMoreLightProperties                 BlowoutFactor, RampPower, DistanceAttenuation, Shape (0 ellipsoid, 1 cone, 2 box)
 * Shape must be exactly 0, 1 or 2 -- the shader's `<=`, `(float) ==` and `(int) ==` tests agree only there; anything else, a NaN included,
 * is ILM_ERR_INVALID_ARGUMENT (the host never packs another value, :1361-1362).  MaxStepCount (StepAndMisc2.x) that is NaN, < 1 or > 4096
 * is ILM_ERR_INVALID_ARGUMENT for this entry point: it divides the column and bounds both loops.
 * Coverage (VolumetricLightVertexShader, VolumetricLightCore.fxh:510-549), once per light, fp32 in the order written: cone p1 = min(start,
 * end) - max(r1, r2), p2 = max(start, end) + max(r1, r2); otherwise p1 = start - end, p2 = start + end; tl = min(p1, p2), br = max(p1, p2)
 * (min / max return the operand that is not a NaN).  Only x and y matter; z is not padded into y ("FIXME: zToY").  The world rectangle is
 * mapped by (world - ViewportPosition) * (ViewportScale * RenderScale), the scales multiplied first, and a pixel is covered iff its centre
 * lies in the half-open rectangle [x0, x1) x [y0, y1): the directional pass's rule.  A rectangle with a NaN bound covers nothing.
 * Per pixel (VolumetricLightPixelCore and volumetricTrace, :315-508), p = the shaded point, n = its normal.  Arithmetic is fp32 with one
 * rounding per + - * / sqrt in the order the HLSL writes it; every division is IEEE (1.0 / l2; hits / steps / Volumetricity as two; p / r per
 * component); dot = (x + y) + z, length = sqrt of that dot, normalize = three divisions by the length, lerp(a, b, t) = a + (b - a) * t
 * unsaturated, saturate(NaN) = 0, sign(0) = sign(NaN) = 0, max / min return the operand that is not a NaN, pow(x, y) = y == 0 ? 1 : exp2(y *
 * log2(x)).  FUSED are only the march's sample position from + along * d (one fma per component) and what the shared sampler fuses.
 *   a fullbright pixel is discarded; a pixel with p.x <= -9999 is not visible, the core returns 0 and it is discarded;
 *   `intersect` (:300-313) returns true on its second line: the early-out never fires, and ellipsoidIntersect, roundConeIntersect,
 *   boxIntersect, coneIntersect, capsuleIntersect, sdCappedCone and sdCapsule are dead code -- not built;
 *   AO as for directional lights: radius * max(0, n.z), sampled only when >= 0.5 and a field is bound (sdf != 0, Extent.x > 0);
 *   traceShadows = (LightProperties.w * enableShadows != 0) && Extent.z > 0 -- .z, the only pass that tests it; samples are taken only with
 *   a bound field: without one occlusion = 1 and nothing is sampled;
 *   the column: steps = MaxStepCount, z2 = max(p.z, GroundZ), z1 = max(MaximumZ, z2); cone: z1 = min(z1, max(start.z, end.z) + max(r1, r2)),
 *   z2 = max(z2, min(start.z, end.z) - max(r1, r2)), md0 = |end - start|; otherwise z1 = min(z1, start.z + end.z), z2 = max(z2, start.z -
 *   end.z), md0 = |end|; step = max(|z2 - z1|, 1) / steps; z = z1 + dither * step; do { body; z -= step; } while (z >= z2).  The body always
 *   runs once, even when the narrowed z1 < z2;
 *   body at pos = (p.x, p.y, z): sd = eval(pos): sdEllipsoid(pos - start, end) = k0 * (k0 - 1) / k1 with k0 = |q / r|, k1 = |q / (r * r)|;
 *   sdRoundCone(pos, start, end, r1, r2) (:31-54) as written, products left to right; sdBox(pos - start, end) = |max(d, 0.0001)| + min(max(
 *   max(d.x, d.y), d.z), 0.0001), d = |q| - b.  occlusion = 1, or the march's; hits += pow(saturate(-sd / RampLength), RampPower) * occlusion;
 *   the march (:359-399), only when traceShadows: d = dither * 0.66; when |LightPosition3.xyz| < 0.01 it runs from start.xyz along pos -
 *   start with md = |pos - start|, otherwise from pos - t along t with t = LightPosition3.xyz * md0 and md = md0; along /= md as written
 *   (t / md0 is not simplified); at most (int)MaxStepCount samples: s = the field at from + along * d; occlusion = saturate(s * 0.5); s <= -0.1
 *   ends the march with occlusion = 0; d += max(|s| * 0.99, MinStepSize); d >= md ends it; occlusion is what the last sample left;
 *   volumetricOpacity = saturate(hits / steps / Volumetricity); preTraceOpacity = aoOpacity * volumetricOpacity;
 *   the contact term: fullLength = md0; c = cone ? max(r1, r2) / 64 : 0; dotRange = lerp(0.15, 0.33, c), dotOffset likewise;
 *   normalOpacity = computeNormalFactorEx(normalize(p - start), n, dotOffset, dotRange) (1 for a zero normal), then lerp(x, x * 2 - 1,
 *   BlowoutFactor); shapeOpacity = eval(p) < 0 ? pow(saturate(-eval(p) / RampLength), RampPower) : 0; distanceOpacity = 1 - saturate(|p -
 *   start| / (fullLength * DistanceAttenuation)); diffuse = (normalOpacity * shapeOpacity) * distanceOpacity.  The RampMode >= 1 squaring
 *   (:495-498) follows the last read of what it changes: it is not computed, RampMode is not read;
 *   opacity = diffuse < 0 ? preTraceOpacity + diffuse : max(preTraceOpacity, diffuse).
 * Discards: a fullbright pixel, an uncovered one, one that is not visible and one with opacity <= 0 get nothing -- no rgb, no + 1 on
 * alpha.  Otherwise rgb += (Color1.rgb * Color1.a) * opacity and alpha += 1.
 * dither = Dither17(vpos, (FrameIndex % 4) + 0.5), a function of Fracture's DitherCommon.fxh outside the reference tree, restated from the
 * one its author published (Jimenez, "Next Generation Post Processing in Call of Duty: Advanced Warfare": frac(dot(float3(pos, frame),
 * float3(2, 7, 23) / 17))) as a DEFINED function, since 1 / 17 is no binary fraction and the order of operations would matter: k = 2 x + 7 y
 * + 23 f with the integer pixel (x, y), exact in fp32; k mod 17 exactly; dither = (k mod 17) / 17, one IEEE division.  FrameIndex is an
 * effect parameter nothing in Illuminant/Lighting sets for the light materials (the only assignment, LightingRenderer.cs:1495, is the
 * resolve pass's): it holds its default 0, f = 0.5, and the entry point takes no frame argument.
 * Termination: z -= step stops making progress once step is below an ulp of z (a huge MaximumZ), so the column loop is also bounded by an
 * integer: at most (int)MaxStepCount + 4 bodies (the arithmetic ends it after at most MaxStepCount + 1 where it makes progress).  A NaN z
 * ends the loop: the comparison is false.  The march is bounded by its counter.
 * Degenerate geometry is defined by that arithmetic and not special-cased; no memory access depends on any of it.  A zero radius component
 * of an ellipsoid: q / 0 is +-inf or NaN, sd = inf * inf / inf = NaN or inf, saturate gives 0 -- no hits; sdEllipsoid at the centre: 0 * -1 /
 * 0 = NaN, no hit from that point; a zero-length cone: l2 = 0, il2 = inf, every product with it NaN or inf, no hits and shapeOpacity 0; md =
 * 0 (the column point at start): along = 0 / 0 = NaN, the NaN sample coordinates are treated as 0 (the test is hoisted out of the march),
 * d >= 0 ends the march after one sample; RampLength = 0: -sd / 0 = +inf inside the shape (ramp 1), -inf outside (0), NaN on the surface
 * (0); Volumetricity = 0: hits / steps / 0 = +inf (1) or NaN (0); NaN positions: a NaN footprint covers nothing, a NaN sd adds no hit, a
 * NaN diffuse compares false and max(preTraceOpacity, NaN) = preTraceOpacity.
 * Statistics: PixelLightPairs = pairs inside a footprint and the image; TracedPairs = pairs with traceShadows and a bound field;
 * SdfSamples = the AO sample + every sample of every march.
 * Not built: VolumetricLightProbe -- Illuminant/LoadMaterials.cs:145-146 loads it, but the reference tree holds no
 * VolumetricLightProbe.fx to define it; the group entry point; the dead intersection code. */
int32_t ilm_render_volumetric_lights(IlmHandle ctx,
                                     const IlmLightVertex* lights, int32_t light_count,
                                     const IlmEnvironment* env,
                                     const IlmDistanceFieldUniforms* df,
                                     IlmHandle gbuffer, IlmHandle sdf,
                                     const float ambient[4],
                                     IlmHandle lightmap, int32_t row_begin, int32_t row_end,
                                     IlmRenderStats* stats);

/* LightSource.TextureRef / Configuration.DefaultRampTexture of the light group rendered by the FOLLOWING ilm_render_sphere_lights,
 * ilm_render_directional_lights (SampleFromRamp(opacity), channel r at v = 0: DirectionalLightWithRamp) and
 * ilm_render_light_probes calls (bound per group by _LightBatchSetup, Illuminant/Lighting/LightingRenderer.cs:764-766; sampler
 * RampTextureSampler, Illuminant/Shaders/RampCommon.fxh:4-21: tex2Dlod level 0, LINEAR, U CLAMP, V WRAP): width * height float4 texels.
 * width == 0 -- or a 1 x 1 texture, which the reference treats as none (:822-827) -- selects the techniques without a ramp. */
int32_t ilm_ctx_set_light_ramp(IlmHandle ctx, const IlmFloat4* texels, int32_t width, int32_t height);

/* How the light passes of this context sum the lights of a pixel.
 *   ILM_BLEND_FP32_ACCUMULATE (default): fp32 registers over all lights in light order, one rounding when the texel is stored.
 *   ILM_BLEND_FP16_PER_LIGHT: the reference's render target.  Its lightmap is a HalfVector4 surface (LightingRenderer.cs:476-479) that
 *     the ROP blends into additively, one light quad after the other: the clear colour and every partial sum are fp16 values.  The
 *     model: dst = half(float(dst) + float(half(src))) per light and channel, round to nearest even (Direct3D converts the shader's
 *     output to the target format, then blends).  Same light order, same shader arithmetic; only the rounding of the sum differs.
 * 1e-4 parity with the HLSL path is defined against the fp32 form; this mode exists to MEASURE how far the frame the
 * reference's hardware path displays lies from it (docs/experiments.md 3.2; tests/test_lighting_gpu.py holds it bit-equal to the oracle's model). */
#define ILM_BLEND_FP32_ACCUMULATE 0
#define ILM_BLEND_FP16_PER_LIGHT 1
int32_t ilm_ctx_set_lightmap_blend(IlmHandle ctx, int32_t mode);

/* Light blend functions: LightSource.BlendMode (Illuminant/Lighting/LightSource.cs:59-65, "Overrides how light is blended into the
 * lightmap"), the BlendState member of LightTypeRenderStateKey (LightingRenderer.cs:51,84,206,806: Key.BlendState ?? BlendState.Additive).
 * Per context, like ilm_ctx_set_lightmap_blend; applies to the FOLLOWING ilm_render_sphere_lights, ilm_render_particle_lights,
 * ilm_render_directional_lights, ilm_render_line_lights, ilm_render_projector_lights and ilm_render_volumetric_lights calls, and to
 * ilm_group_render_sphere_lights through each member context's own setting (the host sets every member alike).  ilm_render_light_probes
 * ignores it: the reference forces RenderStates.AdditiveBlend on the probe target (LightingRenderer.LightProbes.cs:27).
 * color_function acts on r, g and b, alpha_function on a (XNA's ColorBlendFunction / AlphaBlendFunction); both default to ADD.  The
 * factors are One / One -- BlendState.Additive's too: a light shader's output alpha is always 1, so SourceAlpha is One for every technique.
 * Any other value: ILM_ERR_INVALID_ARGUMENT, the state stays as it was (the handle is looked up first: ILM_ERR_INVALID_HANDLE).
 *
 * A (pixel, light) pair contributes exactly when it does under ADD: every discard, footprint test and trace decision is unchanged, and
 * so is IlmRenderStats.  A contributing pair's source value is c = (its rgb contribution, 1).  `base` is the clear colour when
 * ambient != NULL, else the texel, read and converted as under ADD.  Per channel, with f that channel's function:
 *   ILM_BLEND_FP32_ACCUMULATE
 *     ADD:               out = base + S, as ever.
 *     REVERSE_SUBTRACT:  out = base - S, S the very sum ADD forms (sphere and particle lights: the same parts, the same balanced tree;
 *                        the full-frame passes: list order from zero): one subtraction, one rounding.
 *     MAX:               M = -inf; every contributing pair: M = (c > M) ? c : M; out = (M > base) ? M : base.
 *     MIN:               M = +inf; every contributing pair: M = (c < M) ? c : M; out = (M < base) ? M : base.
 *     Comparisons and selects, not fmaxf / fminf: a NaN source is never selected, a NaN base is kept, a pixel without a contributing
 *     pair keeps base bit for bit.  The result of MAX / MIN does not depend on the order of the lights, on parts or on the light split.
 *   ILM_BLEND_FP16_PER_LIGHT: dst = half(base); every contributing pair in list order, s = half(c):
 *     ADD: dst = half(dst + s).  REVERSE_SUBTRACT: dst = half(dst - s).  MAX: dst = (s > dst) ? s : dst.  MIN: dst = (s < dst) ? s : dst.
 * Both models: the store conversion follows the combine and is unchanged -- HALF4 rounds once, RGBA8 saturates (a subtraction ends at
 * byte 0, as on a UNORM target); ambient != NULL with light_count == 0 still clears; store-mode mirrors receive the same texel; the
 * particle lights of a call are one light list (S is the sum ADD forms over it, list batches included).  A sphere-light launch whose functions are not
 * ADD / ADD is served by one workgroup per tile (ilm_ctx_set_light_split does not apply; the bits do not depend on it anyway).
 * Not built: BlendFunction.Subtract (src - dst); destination-colour factors (multiplicative lights); blend factors and write masks. */
#define ILM_LIGHT_BLEND_ADD              0   /* BlendFunction.Add (default) */
#define ILM_LIGHT_BLEND_REVERSE_SUBTRACT 1   /* BlendFunction.ReverseSubtract: dst - src */
#define ILM_LIGHT_BLEND_MAX              2   /* BlendFunction.Max */
#define ILM_LIGHT_BLEND_MIN              3   /* BlendFunction.Min */
int32_t ilm_ctx_set_light_blend_function(IlmHandle ctx, int32_t color_function, int32_t alpha_function);

/* How many workgroups serve one 16 x 16 tile of this context's sphere-light launches ("light split").  The reference cuts a frame's
 * light list into draws of 128 instances and the ROP adds them (Illuminant/Lighting/LightingRenderer.cs:1149-1166,
 * Illuminant/Shaders/SphereLight.fx:42-45): the sum does not care who shaded which light.  Here a tile's list is summed in 8 fixed
 * parts -- each part in light order, the parts onto the clear colour in part order -- and `workgroups` = 1, 2, 4 or 8 says how many
 * workgroups share those parts; the lightmap's bits do not depend on it.  0 (default) = chosen per launch: 1 for launches that fill the
 * device several times over (whole frames); short ones (one rank's strip of a frame split over 8 GPUs, a small target), which would
 * otherwise last two wave lifetimes whatever their share of the work, are TAPERED -- the tiles that start first are served whole, later
 * ones by 2, then 4, the last by 8 workgroups, so that the launch drains in its smallest pieces (docs/experiments.md 3.2).  A non-zero value
 * serves every tile by that many.  Launches in the ILM_BLEND_FP16_PER_LIGHT model, of fewer than 16 or more than 1 024 lights, or of
 * particle lights always use 1. */
int32_t ilm_ctx_set_light_split(IlmHandle ctx, int32_t workgroups);

/* ---- particle lights and light probes --------------------------------------------------------- */

/* What _ParticleLightBatchSetup binds for a ParticleLightSource (Illuminant/Lighting/LightingRenderer.cs:769-790,
 * Illuminant/Lighting/LightSource.cs:466-505) + the StippleFactor ParticleSystem.Render adds
 * (Illuminant/Particles/ParticleSystem.cs:1023). */
typedef struct IlmParticleLightParams {
    IlmFloat4 LightProperties;      /* Template.Radius, RampLength, RampMode, CastsShadows && DistanceField */
    IlmFloat4 MoreLightProperties;  /* aoRadius (0 when aoOpacity <= .001), shadowDistanceFalloff | -99999, falloffYFactor, saturate(aoOpacity) */
    IlmFloat4 LightColor;           /* Template.Color */
    IlmFloat4 LightSpecularColor;   /* Template.SpecularColor, SpecularPower */
    float     StippleFactor;        /* must be >= 1: StippleReject is Fracture code outside the tree (DitherCommon.fxh) */
    float     _pad[3];
} IlmParticleLightParams;

/* technique ParticleLight (Illuminant/Shaders/ParticleLight.fx:16-118): one sphere light per live particle of `system`
 * (position from PositionAndLife, colour = un-premultiplied Chunk.RenderColor x LightColor), additively blended onto what the
 * lightmap already holds -- RenderLighting draws it as one more light-type render state after the clear
 * (LightingRenderer.cs:1126-1141).  quad_counts[i] = min(ChunkMaximumCount, chunk.TotalSpawned + 1) slots of chunk i take part
 * (RenderChunk, ParticleSystem.cs:880); NULL => every slot.  The live particles are compacted on the device in chunk / slot
 * order (wave64 ballot + prefix sum) into the same light records the sphere-light pass uses; nothing is read back. */
int32_t ilm_render_particle_lights(IlmHandle ctx, IlmHandle system, const int32_t* quad_counts, int32_t chunk_count,
                                   const IlmParticleLightParams* params,
                                   const IlmEnvironment* env, const IlmDistanceFieldUniforms* df,
                                   IlmHandle gbuffer, IlmHandle sdf,
                                   IlmHandle lightmap, int32_t row_begin, int32_t row_end,
                                   IlmRenderStats* stats);

/* One ParticleLightSource inside ilm_engine_render_particle_lights_batch: the system arguments of ilm_render_particle_lights. */
typedef struct {
    IlmHandle              System;
    const int32_t*         QuadCounts;  /* ChunkCount entries, or NULL => every slot; as ilm_render_particle_lights */
    int32_t                ChunkCount;  /* the first ChunkCount chunks of System */
    int32_t                _pad;
    IlmParticleLightParams Params;      /* this item's template light */
} IlmParticleLightItem;                 /* 104 bytes */

/* A frame's particle light sources in one call: the loop of one render state per ParticleLightSource (LightingRenderer.cs:1126-1141) over
 * the systems of one engine.  The batch is ONE light list: the items' live, visible particles in item, chunk, slot order, each record
 * built from its OWN item's Params exactly as ilm_render_particle_lights builds it, operation for operation (the emit predicate, the
 * un-premultiply, the quad, the light's flags under the frame's trace gate).  That list goes through ONE launch of the particle-light
 * tile kernel onto what the lightmap holds, under the context's current blend function and blend model, over rows [row_begin, row_end).
 * The context is the engine's.  The same system may appear more than once, with different Params.  Systems, G-buffer, field and
 * lightmap are read and written as in the single call; store-mode mirrors of a group lightmap receive the same texels.  So:
 *  - a batch of one item leaves the bits ilm_render_particle_lights leaves, on every lightmap format;
 *  - items with equal Params whose chunks, concatenated, are the chunks of one system Z leave the bits of one
 *    ilm_render_particle_lights call on Z (the same list, hence the same parts and the same tree);
 *  - ADD under fp32 accumulation, items that differ: the K single calls add K tree roots one after the other, the batch forms one tree --
 *    a DEFINED difference in the order of the sum.  On HALF4 / RGBA8 lightmaps those calls also round after every system, the batch once;
 *  - MAX / MIN under fp32 accumulation: bit for bit the K single calls on a FLOAT4 lightmap (the order does not matter);
 *  - ILM_BLEND_FP16_PER_LIGHT: one chain of roundings in list order -- on a HALF4 lightmap, or a FLOAT4 one whose contents are
 *    half-representable, bit for bit the K single calls in item order;
 *  - stats (may be NULL) are exactly the sums of what the K single calls report: a (pixel, light) pair's shading does not depend on
 *    the rest of the list.
 * count == 0, items without chunks, all-dead systems, quad counts of 0 and a batch in which no particle emits succeed and leave every
 * texel's bits alone.  Three preparation launches however many items there are; asynchronous on the context's stream unless stats is
 * given.
 * Every check runs before anything is queued, uploaded or reserved; a refusal about an item names it in ilm_last_error() ("item 3:
 * ...") and the lightmap is untouched.  Engine and lightmap handles first (ILM_ERR_INVALID_HANDLE); then count < 0, items == NULL with
 * count > 0; per item, a handle that is not a system (ILM_ERR_INVALID_HANDLE), a system of another engine (ILM_ERR_INVALID_ARGUMENT),
 * StippleFactor < 1 (as the single call), ChunkCount outside the system's, a quad count outside [0, slots] (ILM_ERR_OUT_OF_RANGE); over
 * the batch, more than 2^22 quads in sum (ILM_ERR_TOO_MANY, the single call's bound); and whatever the single call refuses about env,
 * df, the G-buffer, the field (a filter other than ILM_SDF_FILTER_FP32 included), the lightmap and the rows, with its code. */
int32_t ilm_engine_render_particle_lights_batch(IlmHandle engine, const IlmParticleLightItem* items, int32_t count,
                                                const IlmEnvironment* env, const IlmDistanceFieldUniforms* df,
                                                IlmHandle gbuffer, IlmHandle sdf, IlmHandle lightmap,
                                                int32_t row_begin, int32_t row_end, IlmRenderStats* stats);
/* Diagnostic: the engine's latest ilm_engine_render_particle_lights_batch that was accepted -- its items (count), the preparation
 * launches and the tile-kernel launches its list took: 3 and 1 for a batch that emitted a record, whatever its items; 0 and 0 for one
 * that had nothing to add.  Without a quad the call queues nothing; with quads of which none emits, what it queued finds an empty list
 * and changes no texel, which only the device knows: this call waits for the context's stream and reads the record count the
 * preparation published.  Any out pointer may be NULL. */
int32_t ilm_debug_last_particle_light_batch(IlmHandle engine, int32_t* out_items, int32_t* out_prepare_launches,
                                            int32_t* out_tile_launches);

/* technique SphereLightProbe (Illuminant/Shaders/SphereLightProbe.fx:19-44) for `probe_count` probes
 * (UpdateLightProbes, Illuminant/Lighting/LightingRenderer.LightProbes.cs:49-110): probe_positions[i] = (position, 1),
 * probe_normals[i] = (normal or 0, enableShadows); out_values[i] = sum over lights of color.rgb * color.a * opacity, alpha =
 * number of contributing lights.  Host arrays; synchronises (the reference reads the values back, :112-150). */
int32_t ilm_render_light_probes(IlmHandle ctx, const IlmLightVertex* lights, int32_t light_count,
                                const IlmFloat4* probe_positions, const IlmFloat4* probe_normals, int32_t probe_count,
                                const IlmEnvironment* env, const IlmDistanceFieldUniforms* df, IlmHandle sdf,
                                IlmFloat4* out_values);

/* techniques DirectionalLightProbe / DirectionalLightProbeWithRamp (Illuminant/Shaders/DirectionalLight.fx:39-50,163-219) over
 * DirectionalLightPixelCore (:52-93), drawn by UpdateLightProbes with the directional render state's probe material
 * (LightingRenderer.LightProbes.cs:63-84).  Arguments and contract of ilm_render_light_probes: host arrays, probe_positions[i] =
 * (position, opacity), probe_normals[i] = (normal or 0, enableShadows), out_values[i] = the sum over the lights in list order, alpha =
 * the number of contributing lights; the call synchronises; light_count == 0 gives zeros; probe_count == 0 returns ILM_OK and touches
 * nothing.  `lights` has the vertex layout of ilm_render_directional_lights.  Per (probe, light):
 *   a probe with positions.w <= 0 receives nothing, no rgb and no alpha (sampleLightProbeBuffer discards, LightCommon.fxh:233-254);
 *   LightProperties.x *= normals.w and MoreLightProperties.x = .w = 0 (:182-183): no ambient-occlusion sample; then the core as in the
 *   frame pass;
 *   the normal factor applies only when Color2.w >= 0.1 (LightCommon.fxh:227); a zero normal gives factor 1 (:154-165);
 *   the trace runs iff the probe is visible, LightProperties.x * normals.w != 0, opacity >= 1 / 256 and the light is directed (:73);
 *   it starts at position + 1.5 * normal (:81);
 *   Bounds (LightPosition1.xy / LightPosition2.xy) are NOT read: the probe vertex shader covers the whole target (:48-49) and the pixel
 *   shader carries "FIXME: Clip to region" (:175) -- a bounded light reaches every probe, and no bounds are refused;
 *   the shadow filter is not consulted (the probe shaders do not take EvenMoreLightProperties, :163-169);
 *   no opacity discard: a visible probe (x > -9999) with w > 0 adds alpha 1 even at opacity 0; an invisible one adds nothing (clip, :91);
 *   value = Color1.rgb * Color1.a * opacity * positions.w (:185-189), one rounding per product, left to right;
 *   while a ramp is bound (ilm_ctx_set_light_ramp, not 1 x 1) the technique is DirectionalLightProbeWithRamp: opacity =
 *   SampleFromRamp(opacity) before the multiply by positions.w (:86-87,214-216).
 * ilm_ctx_set_light_blend_function and ilm_ctx_set_lightmap_blend are ignored, as by ilm_render_light_probes (the probe target is
 * forced to additive blending, LightProbes.cs:27).  A field whose filter is not ILM_SDF_FILTER_FP32 is refused
 * (ILM_ERR_INVALID_ARGUMENT, out_values untouched). */
int32_t ilm_render_directional_light_probes(IlmHandle ctx, const IlmLightVertex* lights, int32_t light_count,
                                            const IlmFloat4* probe_positions, const IlmFloat4* probe_normals, int32_t probe_count,
                                            const IlmEnvironment* env, const IlmDistanceFieldUniforms* df, IlmHandle sdf,
                                            IlmFloat4* out_values);

/* technique LineLightProbe (Illuminant/Shaders/LineLightProbe.fx:9-48), with the arguments and contract of ilm_render_light_probes and
 * the vertex layout of ilm_render_line_lights.  The shader is SphereLightProbe's at the line's start point ("FIXME: Why is this file
 * sphere lights and not line lights", :4): the result is exactly what ilm_render_light_probes computes for sphere lights with centre
 * LightPosition1.xyz, colour Color1, LightProperties and MoreLightProperties taken from the line vertex -- the line vertex is rewritten
 * into that sphere vertex on the host and goes through the sphere preparation and kernels.  LightProperties.y, the ramp length, is 0 as
 * RenderLineLightSource writes it (LightingRenderer.cs:1324) and is honoured as given: the distance falloff (distance - radius) / 0 is
 * IEEE (+inf, -inf or NaN; saturate: 1, 0, 0), so such a light is full inside its radius and absent outside, and the cone growth is
 * maxRadius / 16 (createTraceConfig's max(ramp length, 16)).  LightPosition2, Color2 and EvenMoreLightProperties are not read, and neither is a bound ramp (there is no
 * LineLightProbeWithDistanceRamp).  A field whose filter is not ILM_SDF_FILTER_FP32 is refused as above. */
int32_t ilm_render_line_light_probes(IlmHandle ctx, const IlmLightVertex* lights, int32_t light_count,
                                     const IlmFloat4* probe_positions, const IlmFloat4* probe_normals, int32_t probe_count,
                                     const IlmEnvironment* env, const IlmDistanceFieldUniforms* df, IlmHandle sdf,
                                     IlmFloat4* out_values);

/* ---- output side: particle read-back and lightmap resolve -------------------------------------- */

/* The members of Fracture's BitmapDrawCall that FillReadbackResult writes per live particle
 * (Illuminant/Particles/ParticleReadback.cs:73-167).  BitmapDrawCall itself is outside the reference tree. */
typedef struct IlmReadbackDrawCall {
    float   Position[2];        /* pAndL.X, pAndL.Y */
    float   Scale[2];           /* pSize * renderData.x */
    float   TextureRegion[4];   /* TopLeft.xy, BottomRight.xy (animation frame applied) */
    float   Rotation;           /* RotationFromVelocity ? renderData.y % 2 pi : 0 */
    float   SortOrder;          /* SortedReadback ? pAndL.Y + ZToY : 0 */
    uint8_t MultiplyColor[4];   /* (byte)(renderColor * 255), R G B A */
    int32_t _pad;
} IlmReadbackDrawCall;

/* What FillReadbackResult reads from ParticleSystemConfiguration / ParticleAppearance (:80-115): pSize and the texture region are
 * resolved by the caller (they depend on the texture's size, which lives on the C# side). */
typedef struct IlmReadbackParams {
    float   Size[2];            /* pSize */
    float   TextureRegion[4];   /* region: TopLeft.xy, BottomRight.xy; Bounds.Unit = (0,0,1,1) without a texture */
    float   AnimationRate[2];
    float   ZToY;
    int32_t ColumnFromVelocity, RowFromVelocity, RotationFromVelocity, SortedReadback;
    int32_t _pad;
} IlmReadbackParams;

/* MaybePerformReadback + FillReadbackResult (ParticleReadback.cs:21-167): instead of reading three whole float4 planes per chunk
 * back and filtering on the CPU, the live particles are compacted on the device (chunk / slot order, wave64 ballot + prefix sum)
 * straight into draw-call records and only those cross PCIe.  element_counts[i] = ceil(TotalSpawned / ChunkSize) * ChunkSize slots
 * of chunk i are examined (:57-58); NULL => every slot.  Writes at most `capacity` records and the total to *out_count;
 * synchronises. */
int32_t ilm_system_readback(IlmHandle system, const int32_t* element_counts, int32_t chunk_count, const IlmReadbackParams* params,
                            IlmReadbackDrawCall* out, int32_t capacity, int32_t* out_count);
/* The same read-back without the last copy: the records stay in a page-locked host buffer owned by the system's context (the
 * reference keeps a pooled ReadbackResultBuffer too, ParticleReadback.cs:40-41) and *out_records points at it; valid until the next
 * read-back on that context or its destruction.  Capacity is every examined slot.  NULL when nothing is alive.  Synchronises. */
int32_t ilm_system_readback_view(IlmHandle system, const int32_t* element_counts, int32_t chunk_count, const IlmReadbackParams* params,
                                 const IlmReadbackDrawCall** out_records, int32_t* out_count);

enum { ILM_HDR_NONE = 0, ILM_HDR_GAMMA_COMPRESS = 1, ILM_HDR_TONE_MAP = 2 };   /* HDRMode, LightingRenderer.HDR.cs:254-258 */

/* ---- particle rasterisation (techniques RasterizeParticlesNoTexture / TexturePoint / TextureLinear) -------------- */

enum {
    ILM_BLEND_ALPHA    = 0,  /* BlendState.AlphaBlend on premultiplied colour: dst = src + dst * (1 - src.a) */
    ILM_BLEND_ADDITIVE = 1   /* BlendState.Additive-like (One, One): dst = src + dst */
};
enum {
    ILM_BITMAP_NONE   = 0,   /* technique RasterizeParticlesNoTexture */
    ILM_BITMAP_POINT  = 1,   /* technique RasterizeParticlesTexturePoint  (BitmapPointSampler: POINT, CLAMP) */
    ILM_BITMAP_LINEAR = 2    /* technique RasterizeParticlesTextureLinear (BitmapSampler: LINEAR, CLAMP) */
};

/* What ParticleSystem.Render binds for the rasterise techniques: Uniforms.RasterizeParticleSystem (Illuminant/Uniforms.cs:238-290),
 * RoundingPowerFromLife, RenderingOptions, StippleFactor (Illuminant/Particles/ParticleSystem.cs:943-1041, :254-271) and the bits of
 * Uniforms.ParticleSystem the vertex shader reads (TexelAndSize.zw, ZToY).  The view transform -- Fracture's ViewTransformCommon.fxh,
 * outside the tree -- is reduced to the default one of a render target: pixel = (display - ViewportPosition) * ViewportScale,
 * pixel centres at +0.5; the depth formula is carried but unused (no depth buffer). */
typedef struct IlmRasterizeParams {
    IlmFloat4 GlobalColor;             /* Color.Global, premultiplied (Uniforms.cs:279-283) */
    IlmFloat4 BitmapTextureRegion;     /* (offset, offset + size) / texture size; (0, 0, 1, 1) without a texture */
    IlmFloat4 SizeFactorAndPosition;   /* (SizePx / 2 when RelativeSize and a texture is bound, else (1, 1); origin.xy) */
    IlmFloat4 Scale;                   /* (scale.xy, 0, 0) */
    IlmFloat4 ZFormula;
    IlmFloat4 ZConfiguration;          /* (SizeFromZ, 0, 0, 0) */
    IlmClampedBezier1 RoundingPowerFromLife;
    float     RenderingOptions[4];     /* Rounded, DitheredOpacity (premultipliedToDithered, RasterizeParticleSystem.fx:158-175, over Dither64 -- Fracture code outside the
                                      * tree, restated from the function it publishes: Jimenez, SIGGRAPH 2014), column / row (of the frame sheet) from velocity */
    float     SystemSize[2];           /* System.TexelAndSize.zw = Configuration.Size */
    float     ZToY;
    float     StippleFactor;           /* must be >= 1 (StippleReject is Fracture code) */
    float     ViewportScale[2], ViewportPosition[2];
    int32_t   BlendMode;               /* ILM_BLEND_* */
    int32_t   BitmapFilter;            /* ILM_BITMAP_*: which technique; the bitmap is the one bound with ilm_system_set_bitmap */
    float     AnimationRate[2];        /* System.AnimationRateAndRotationAndZToY.xy = 1 / Appearance.AnimationRate (0 when that is 0) */
} IlmRasterizeParams;

/* ParticleSystem.Render with technique RasterizeParticlesNoTexture (Illuminant/Shaders/RasterizeParticleSystem.fx:61-260,
 * Illuminant/Particles/ParticleSystem.cs:876-1041): every live particle of the first chunk_count chunks becomes a rotated quad
 * (VS_PosVelAttr) shaded by PS_NoTexture (colour x GlobalColor x computeCircularAlpha, discard at alpha <= 0 -- the shader's
 * `1 / 512` is an integer division) and blended onto `target` (a lightmap object used as the render target) IN CHUNK / SLOT ORDER,
 * as the instanced draws of RenderChunk do.  quad_counts[i] = min(ChunkMaximumCount, TotalSpawned + 1) slots of chunk i take part
 * (NULL => every slot).  A pixel belongs to a quad when its centre maps to unit coordinates in [-1, 1) x [-1, 1) (the top-left rule
 * of an axis-aligned quad, carried along with the rotation).  Sorted on the device by (16 x 16 tile, slot); nothing is read back.
 * out_stats (may be NULL): [0] live quads, [1] (quad, tile) pairs, [2] shaded pixels (fragments not discarded). */
int32_t ilm_render_particles(IlmHandle system, const int32_t* quad_counts, int32_t chunk_count, const IlmRasterizeParams* params,
                             IlmHandle target, uint64_t* out_stats);

/* One system's draw inside ilm_engine_render_particles_batch: the arguments of ilm_render_particles. */
typedef struct {
    IlmHandle          System;
    const int32_t*     QuadCounts;   /* ChunkCount entries, or NULL => every slot; as ilm_render_particles */
    int32_t            ChunkCount;   /* the first ChunkCount chunks of System */
    int32_t            _pad;
    IlmRasterizeParams Params;       /* this item's technique, blend mode, colours, view transform */
} IlmRasterizeItem;

/* A frame's worth of ParticleSystem.Render in one call: the Render half of the loop ilm_engine_step_batch takes the Update half of
 * (Scenes/ManySystemsManySpawners.cs:78-81, `s.Render(group, j++)` for 256 systems).  The batch is ONE draw list: the items' sprites
 * concatenated in item, chunk, slot order.  A pixel's value: the target texel converted to fp32 once; every fragment of every item that
 * is not discarded blended onto it in that order, in fp32, with its OWN item's state (BlendMode, RenderingOptions, BitmapFilter,
 * BitmapTextureRegion, GlobalColor, its system's bitmap); one store conversion.  Setup, coverage, shading and discards are those of
 * ilm_render_particles, operation for operation.  So:
 *  - FLOAT4 target, no tile's run in the batch longer than one segment (2 048 (quad, tile) pairs): the texels are bit for bit what
 *    ilm_render_particles(items[i] ...) for i = 0 .. count - 1 would leave.
 *  - HALF4 / RGBA8 target: those calls round to the target format after every system, the batch rounds once -- a DEFINED difference
 *    (the reference's ROP rounds after every quad: neither form is its bits).
 *  - A tile whose run in the batch exceeds one segment is composed from partial results as in ilm_render_particles, the run cut every
 *    2 048 pairs wherever item boundaries fall (additive is the partial with transmittance 1, so blend modes mix within a run).
 *  - out_stats (may be NULL): [0..2] as ilm_render_particles, summed over the items -- exactly the sum of what those calls report.
 * The same system may appear more than once (it is only read).  count == 0, and a batch without a live on-screen quad, succeed and
 * leave every texel's bits alone.  One host synchronisation (the pair count) and one sort however many items there are; afterwards
 * asynchronous on the context's stream unless out_stats is given.
 * All items are validated before anything is queued, uploaded or changed; a refusal about an item names it in ilm_last_error() ("item 3:
 * ...") and the target is untouched.  Engine and target handles are checked first (ILM_ERR_INVALID_HANDLE); then count < 0, items ==
 * NULL with count > 0, a target of another context or beyond the single call's size bound; per item, a handle that is not a system
 * (ILM_ERR_INVALID_HANDLE), a system of another engine (ILM_ERR_INVALID_ARGUMENT) and whatever ilm_render_particles refuses, with its
 * code; over the batch, more than INT32_MAX slots -- each item's slots counted in whole blocks of 256 -- or more than 2^28 pairs
 * (ILM_ERR_TOO_MANY). */
int32_t ilm_engine_render_particles_batch(IlmHandle engine, const IlmRasterizeItem* items, int32_t count,
                                          IlmHandle target, uint64_t* out_stats);
/* Diagnostic: the engine's latest ilm_engine_render_particles_batch that was accepted -- its items (count), the radix sorts it ran and
 * the tile-kernel launches it made: 1 and 1 for a batch that drew something, 0 and 0 for one with nothing to draw (count == 0, no
 * chunks, nothing alive or on screen).  Any out pointer may be NULL. */
int32_t ilm_debug_last_render_batch(IlmHandle engine, int32_t* out_items, int32_t* out_sorts, int32_t* out_tile_launches);

/* Appearance.Texture for the textured techniques (PS_Texture / PS_TexturePoint, RasterizeParticleSystem.fx:191-226; frame selection
 * of VS_PosVelAttr, :112-139): width * height float4 texels, row-major, ONE level -- the reference samples with a mip filter whose
 * level comes from screen-space derivatives (hardware-defined) over a chain its texture loader builds; a bitmap without mips is
 * the case that is defined by the shader text alone.  The fragment is colour x texel x GlobalColor x computeCircularAlpha.
 * width == 0 releases the bitmap. */
int32_t ilm_system_set_bitmap(IlmHandle system, const IlmFloat4* texels, int32_t width, int32_t height);
/* Fill a lightmap / render target with one colour (the Clear before ParticleSystem.Render). */
int32_t ilm_lightmap_clear(IlmHandle lightmap, const float rgba[4]);

/* HDRConfiguration (Illuminant/Lighting/LightingRenderer.HDR.cs:198-252) as LightingResolveHandler._Before binds it
 * (Illuminant/Lighting/LightingRenderer.cs:1463-1520; clamps of IlluminantMaterials.cs:81-137 are applied by the library). */
typedef struct IlmHDRConfiguration {
    int32_t Mode;
    float   InverseScaleFactor;     /* 0 => 1 */
    float   Offset, Exposure, Gamma;
    float   MiddleGray, AverageLuminance, MaximumLuminance;   /* GammaCompression */
    float   WhitePoint;                                       /* ToneMapping */
    int32_t ResolveToSRGB;          /* must be 0: pLinearToPSRGB is Fracture code (sRGBCommon.fxh, outside the tree) */
    int32_t DitheringStrength;      /* must be 0: ApplyDither is Fracture code (DitherCommon.fxh) */
    int32_t AlbedoIsSRGB;           /* with-albedo resolve only; must be 0: pSRGBToPLinear is Fracture code (sRGBCommon.fxh) */
} IlmHDRConfiguration;

/* RenderedLighting.Resolve without albedo, 1:1 (techniques ScreenSpaceLightingResolve / GammaCompressedLightingResolve /
 * ToneMappedLightingResolve, Illuminant/Shaders/Resolve.fx:25-139 + HDR.fxh): dst[row_begin..row_end) = tone-mapped src, alpha 1.
 * src and dst are lightmap handles of the same width (any formats; dst RGBA8 is the back-buffer case).  Heights may differ -- a group
 * member's lightmap (ilm_group_lightmap_member) carries padding rows below the frame, a back buffer does not -- as long as the rows
 * resolved exist in every texture involved.
 * Non-finite results (defined behaviour, both entry points): the shader's arithmetic is kept, so a black pixel is NaN (0 / 0) in the
 * GammaCompress mode, and inf or NaN texels give what IEEE arithmetic gives.  What the destination then holds: a FLOAT4 destination
 * the value itself; a HALF4 destination NaN for NaN and infinity for whatever lies beyond the largest half; an RGBA8 destination
 * byte 0 for NaN (saturate(NaN) = 0, as Direct3D's), 0 for -inf and 255 for +inf.  A finite texel whose square stays finite never resolves
 * to NaN in the plain and ToneMap modes. */
int32_t ilm_resolve_lighting(IlmHandle src_lightmap, IlmHandle dst_lightmap, const IlmHDRConfiguration* hdr,
                             int32_t row_begin, int32_t row_end);
/* RenderedLighting.Resolve WITH albedo (LightingRenderer.ResolveLighting with `albedo != null`, Illuminant/Lighting/LightingRenderer.cs:1537-1580;
 * techniques ScreenSpaceLightingResolveWithAlbedo / GammaCompressed... / ToneMapped..., Illuminant/Shaders/Resolve.fx:43-60,141-233), 1:1:
 * light = src * (InverseScaleFactor * 2); rgb = lerp(albedo.rgb, albedo.rgb * light.rgb, saturate(light.a)); alpha = albedo.a; then the
 * HDR mode as above.  `albedo` is a texture the size of the lightmap held in a lightmap object (RGBA8 = SurfaceFormat.Color is the
 * usual case; upload with ilm_lightmap_upload); albedo == 0 is ilm_resolve_lighting.  Not bound: AlbedoIsSRGB.  The LUT-blended technique is ilm_resolve_lighting_lut. */
int32_t ilm_resolve_lighting_with_albedo(IlmHandle src_lightmap, IlmHandle albedo, IlmHandle dst_lightmap, const IlmHDRConfiguration* hdr,
                                         int32_t row_begin, int32_t row_end);

/* The scaled, filtered resolve: RenderedLighting.Resolve(container, layer, width, height, ...) and Resolve(container, layer, position,
 * scale, ...) (Illuminant/Lighting/LightingRenderer.HDR.cs:99-151) through LightingRenderer.ResolveLighting
 * (Illuminant/Lighting/LightingRenderer.cs:1537-1645) -- the lightmap, rendered at Configuration.RenderScale
 * (LightingRenderer.Configuration.cs:58-60,203-214), drawn as a quad of any size (Scale = scale / Configuration.RenderScale, :1638) through
 * `lightmapSamplerState ?? SamplerState.LinearClamp` (:1621-1622), over an albedo texture when there is one (TextureRegion2 =
 * lightmapBounds, :1626-1633).  The two entry points above are the case source size == destination size and stay as they are.
 *
 * DEFINED DEVIATION.  The reference leaves the quad to Fracture's BitmapDrawCall, its vertex shader and BitmapCommon.fxh, and the fetch
 * to the hardware sampler; none of these is in the tree.  What replaces them is stated here in full, as the rasteriser's view
 * transform is:
 *   Coverage.  Destination pixel (px, py) is written when its centre (px + 0.5, py + 0.5) lies in [x, x + width) x [y, y + height)
 *     (quad = x, y, width, height in DESTINATION pixels), row_begin <= py < row_end, and it is inside `dst`.  The pixel ranges are
 *     computed in double from the float arguments and clamped to the target before any conversion to int.  Every other texel of `dst`
 *     keeps its bits; a quad that misses the target, or has width or height 0, succeeds and writes nothing.
 *   Coordinate.  Per axis, in TEXELS of the texture read (not UV: at scale 1 the coordinate is exactly px + 0.5), in fp32 with every
 *     operation rounded, in this order -- r0, r1 the region's bounds on the axis, a multiply, then an IEEE divide:
 *         u = r0 + (((float)px + 0.5f) - x) * (r1 - r0) / width
 *     the lightmap only:  u += uv_offset        (LightmapUVOffset, in SOURCE texels; NULL = (0, 0))
 *         u = fminf(fmaxf(u, r0), r1)           (clamp2(texCoord + LightmapUVOffset, texRgn.xy, texRgn.zw), Resolve.fx:34,49-50)
 *     so a NaN coordinate becomes r0 and an infinite one a bound of the region: any uv_offset is valid input.
 *   ILM_FILTER_LINEAR (CLAMP addressing).  s = u - 0.5f, f = s - floorf(s); taps clamp((int)floorf(s), 0, size - 1) and
 *     clamp((int)floorf(s) + 1, 0, size - 1); the value is lerp4(lerp4(t00, t10, fx), lerp4(t01, t11, fx), fy), lerp(a, b, t) =
 *     a + (b - a) * t: the taps and weights of the projector texture's fetch with clamped instead of wrapped indices.  Every index is
 *     inside the texture by integer arithmetic, whatever the floats are.  The region clamps the COORDINATE, not the taps: a region
 *     smaller than its texture (the reference's lightmap is MaximumRenderSize, its region GetRenderSize) bleeds the neighbouring column
 *     or row at its far edge when magnified, as the hardware fetch does.
 *   ILM_FILTER_POINT.  The texel clamp((int)floorf(u), 0, size - 1).
 *   The light texel sampled so over lightmap_region with lightmap_filter, and the albedo texel sampled the same way over albedo_region
 *     with albedo_filter (no offset), go through the arithmetic of ilm_resolve_lighting[_with_albedo] unchanged: every HDR mode, every
 *     source / albedo / destination format and the non-finite behaviour documented there carry over.
 * Regions are x0, y0, x1, y1 in texels of their texture; albedo_region is ignored (may be NULL) when albedo == 0.  The three textures
 * may have any sizes and formats.
 * Refused, leaving `dst` untouched: a bad handle (ILM_ERR_INVALID_HANDLE, before anything else); textures of different contexts; hdr,
 * quad or a needed region NULL; a quad that is not finite or has a negative size; a region that is not finite or not
 * 0 <= x0 <= x1 <= the texture's width (likewise in y); a filter other than the two; rows outside [0, dst height] (ILM_ERR_OUT_OF_RANGE);
 * ResolveToSRGB, dithering and AlbedoIsSRGB as above.  Asynchronous on the context's main stream, like the 1:1 resolve.
 * Not built: the world-space techniques (they need the view transform), the `blendState` override, LUT blending, and mip filtering
 * of the albedo. */
#define ILM_FILTER_POINT  0   /* SamplerState.PointClamp */
#define ILM_FILTER_LINEAR 1   /* SamplerState.LinearClamp: the default of ResolveLighting, LightingRenderer.cs:1621-1622 */
int32_t ilm_resolve_lighting_scaled(IlmHandle src_lightmap, IlmHandle albedo /* 0 = none */, IlmHandle dst,
                                    const IlmHDRConfiguration* hdr,
                                    const float quad[4],             /* x, y, width, height in DESTINATION pixels */
                                    const float lightmap_region[4],  /* x0, y0, x1, y1 in SOURCE texels */
                                    const float albedo_region[4],    /* x0, y0, x1, y1 in ALBEDO texels; ignored (may be NULL) when albedo == 0 */
                                    const float uv_offset[2],        /* LightmapUVOffset in SOURCE texels; NULL = (0, 0) */
                                    int32_t lightmap_filter, int32_t albedo_filter,
                                    int32_t row_begin, int32_t row_end);   /* destination rows; the strip of a group member */

/* The LUT-blended resolve: RenderedLighting.Resolve with a LUTBlendingConfiguration (Illuminant/Lighting/LightingRenderer.HDR.cs:260-273)
 * and an albedo -- technique ScreenSpaceLUTBlendedLightingResolveWithAlbedo (Illuminant/Shaders/LUTResolve.fx:61-144), selected at
 * Illuminant/Lighting/LightingRenderer.cs:1574-1577, its uniforms bound by SetLUTBlending (Illuminant/Lighting/IlluminantMaterials.cs:139-147).
 * The albedo is looked up in a dark and a bright colour LUT and the two are blended by the light's luminance (or per channel).
 *
 * Fetch and coverage are ilm_resolve_lighting_scaled's, word for word: quad, regions, uv_offset, filters and rows mean what they mean
 * there, and the light texel `tap` and the albedo texel `albedo` are the ones that contract defines.  The 1:1 case is the quad of the
 * albedo's size.
 *
 * Per pixel (LUTBlendedResolveWithAlbedoCommon, LUTResolve.fx:61-115), in fp32, one rounding per operation, no contraction, in this order:
 *     light = tap * (InverseScaleFactor * 2)                                              (:75; InverseScaleFactor 0 => 1)
 *     a = saturate(albedo.rgb)            (:87; a NaN becomes 0, as saturate does everywhere in this header); the alpha written is albedo.a
 *   Launch-uniform, computed once on the host in fp32 in the shader's order (:78-81):
 *     bandWidth = saturate(BrightLevel - DarkLevel);  neutral = fminf(NeutralBandSize, bandWidth - 0.01f)
 *     hasNeutralBand = neutral > 0;  normalize = !PerChannel || hasNeutralBand
 *   Weight (:77,82-85): under `normalize` every channel of w is (light.r * 0.299f + light.g * 0.587f) + light.b * 0.144f (0.144 is
 *     LUTResolve.fx:16's constant, as in ilm_lightmap_luminance); otherwise w = light.rgb.
 *   dark = ReadLUT(DarkLUT, a), bright = ReadLUT(BrightLUT, a): below.  lerp(x, y, t) = x + (y - x) * t.
 *   With a neutral band (:93-98): t = (bandWidth - neutral) * 0.5f (0.005 less a rounding at the least: never a zero divisor), v = w.x - DarkLevel,
 *     v3 = (v - t) - neutral;  val1 = lerp(dark, a, saturate(v * (1 / t)));  blended = lerp(val1, bright, saturate(v3 * (1 / t))).
 *   Without one (:100-110): when BrightLevel > DarkLevel, w = saturate(fmaxf(0, w - DarkLevel) * (1 / (BrightLevel - DarkLevel))), else
 *     (the shader's HACK branch) w = saturate(w - DarkLevel);  blended = lerp(dark, bright, w), channel by channel.
 *   The two uniform divisors are host-side reciprocals: 1.0f / t and 1.0f / (BrightLevel - DarkLevel) are each rounded once on the host and
 *     the pixel multiplies by them, as the resolve's other uniform divisors are taken.
 *   rgb = LUTOnly ? blended : blended * light.rgb (:113), then the ILM_HDR_NONE epilogue of the other resolves unchanged (:129-131):
 *     pow(max(0, rgb + Offset) * Exposure, Gamma) with their clamps of Exposure and Gamma.  Destination formats and non-finite results are
 *     those of ilm_resolve_lighting; a non-finite light texel gives what IEEE arithmetic gives and never an index outside a LUT.
 *
 * DEFINED DEVIATION: ReadLUT and the texture layout.  The reference leaves both to Fracture's LUTCommon.fxh and ColorLUT, which are
 * outside the tree.  What replaces them, in full:
 *   Layout.  A LUT of resolution N with R rows is a texture of width N * N and height N * R: R rows of N slices of N x N texels, the
 *     slices side by side.  Lattice point (ri, gi, bi) of row `Row` is the texel at column bi * N + ri, texel row Row * N + gi.  Only its
 *     rgb is read.  The texture may have any format (RGBA8 is the usual one).
 *   Per channel c of a:  s = c * (float)(N - 1), i0 = min((int)floorf(s), N - 1), i1 = min(i0 + 1, N - 1), f = s - floorf(s).
 *   The value is the trilinear blend of the eight lattice points T[ri][gi][bi] round a:
 *     lerp3(lerp3(lerp3(T000, T100, fr), lerp3(T010, T110, fr), fg), lerp3(lerp3(T001, T101, fr), lerp3(T011, T111, fr), fg), fb)
 *   Indices are clamped inside the slice and the row by integer arithmetic: no tap ever comes from a neighbouring slice or row, whatever
 *     the floats are.  This is the lattice fetch that a bilinear sampler with a half-texel inset plus a manual blue lerp approximates.
 *   DarkRow / BrightRow choose the row; the reference never sets LUTOffsets (SetLUTBlending's "FIXME: RowIndex"), which is row 0.
 *
 * Refused, leaving `dst` untouched: a bad handle -- src, dst, albedo, and DarkLUT / BrightLUT once `lut` can be read
 * (ILM_ERR_INVALID_HANDLE; src and dst before anything else); albedo == 0 (the reference has no LUT technique without albedo); hdr, lut,
 * quad or a region NULL; hdr->Mode other than ILM_HDR_NONE (the reference throws "LUT blending is not compatible with this type of
 * lighting resolve", LightingRenderer.cs:1589-1590); a Resolution < 2 or a RowCount < 1; a LUT texture whose size is not N * N x N * R; a
 * row outside [0, R); a DarkLevel, NeutralBandSize or BrightLevel that is not finite; textures of different contexts; and everything
 * ilm_resolve_lighting_scaled refuses (ResolveToSRGB, dithering, AlbedoIsSRGB, a bad filter, rows, quad or region).
 * Asynchronous on the context's main stream. */
typedef struct {
    IlmHandle DarkLUT, BrightLUT;                 /* lightmap objects holding the LUT textures (any format; RGBA8 is the usual one) */
    int32_t   DarkResolution, BrightResolution;   /* LUTResolutionsAndRowCounts.xy */
    int32_t   DarkRowCount,  BrightRowCount;      /* LUTResolutionsAndRowCounts.zw */
    int32_t   DarkRow, BrightRow;                 /* which row of the texture is read; the reference never sets LUTOffsets: 0 */
    float     DarkLevel, NeutralBandSize, BrightLevel;   /* LUTLevels.xyz */
    int32_t   PerChannel, LUTOnly;
} IlmLUTBlending;
int32_t ilm_resolve_lighting_lut(IlmHandle src_lightmap, IlmHandle albedo /* required */, IlmHandle dst,
                                 const IlmHDRConfiguration* hdr, const IlmLUTBlending* lut,
                                 const float quad[4], const float lightmap_region[4], const float albedo_region[4],
                                 const float uv_offset[2], int32_t lightmap_filter, int32_t albedo_filter,
                                 int32_t row_begin, int32_t row_end);

/* ---- brightness estimation: the inputs of the resolve's AverageLuminance / MaximumLuminance / Exposure / WhitePoint -------
 *
 * Configuration.EnableBrightnessEstimation makes RenderLighting draw the lightmap into a half-size Single target with technique
 * CalculateLuminance (Illuminant/Shaders/Resolve.fx:15,212-227,337-343; Illuminant/Lighting/LightingRenderer.cs:527-537,839-898,989-1001);
 * RenderedLighting.TryComputeHistogram reads one mip level of it back and feeds it to Histogram.Add
 * (Illuminant/Lighting/LightingRenderer.HDR.cs:21-55,154-183; Illuminant/Histogram.cs:17-246).  Both run on the device here.
 *
 * The level: level 0 is (render_width / 2) x (render_height / 2); its texel (x, y) is the lightmap's texel
 * (min(rw - 1, ((2x + 1) rw) / (2 w0)), min(rh - 1, ((2y + 1) rh) / (2 h0))) -- the destination pixel centre through the draw of
 * LightingRenderer.cs:888-893, in integer arithmetic -- turned into (r * 0.299f + g * 0.587f) + b * 0.144f (0.144 is Resolve.fx:15's
 * constant).  Level k is ((a + b) + (c + d)) * 0.25f over the 2 x 2 texels of level k - 1, an odd last row / column dropped.  The level
 * used is min(accuracy_factor, LevelCount - 1) with LevelCount = floor(log2(max(W / 2, H / 2))) + 1 of the lightmap's own size
 * (HDR.cs:164) and holds (w0 >> level) x (h0 >> level) texels (HDR.cs:176-177); a level without texels is ILM_ERR_OUT_OF_RANGE.
 * Refused with ILM_ERR_INVALID_ARGUMENT, nothing written: a render size below 2 or beyond the lightmap's, a negative accuracy factor,
 * BucketCount outside [2, 256], a NaN or non-increasing bucket table.
 *
 * (The three structs below are untagged typedefs; tests/test_brightness_kat.py holds their layout to the ctypes mirrors.) */
typedef struct { int32_t Count; float Min, Max, Sum; } IlmHistogramBucket;     /* BucketState, Histogram.cs:32-35 */
typedef struct {
    int32_t RenderWidth, RenderHeight;      /* Configuration.GetRenderSize of the frame in the lightmap */
    int32_t AccuracyFactor;                 /* TryComputeHistogram's accuracyFactor (3 in the reference) */
    int32_t BucketCount, IgnoreZeroes;
    float   ScaleFactor;                    /* RenderedLighting.InverseScaleFactor */
} IlmHistogramParams;
typedef struct {
    int32_t SampleCount, LevelIndex, Width, Height;
    float   Min, Max, Mean, Median, Sum;    /* Histogram.cs:50-54,60 after Clear + Add */
} IlmHistogramResult;
/* Texture.GetDataFast(LevelIndex, ...) of HistogramUpdateTask.Execute (HDR.cs:38-41): the level's texels, row-major.
 * out_values == NULL only reports level and size.  Synchronous. */
int32_t ilm_lightmap_luminance(IlmHandle lightmap, int32_t render_width, int32_t render_height, int32_t accuracy_factor,
                               float* out_values, int32_t capacity, int32_t* out_level, int32_t* out_width, int32_t* out_height);
/* Histogram.Clear + Histogram.Add(buffer, count, ScaleFactor) over that level (HDR.cs:43-49, Histogram.cs:94-112,165-219) with the
 * caller's BucketMaxValues (Histogram.cs:69-75): out_buckets[BucketCount] are the BucketStates, *out the totals and the median.
 * Counts, minima, maxima and the median are exact; sums are added in a fixed order (the same call returns the same bits) and differ
 * from the reference's sequential sum by rounding only.  The median's last-zero search sees exactly the level's values (the reference
 * searches its whole, possibly longer, scratch array).  Synchronous, like ilm_render_light_probes. */
int32_t ilm_lightmap_histogram(IlmHandle lightmap, const IlmHistogramParams* params, const float* bucket_max_values,
                               IlmHistogramBucket* out_buckets, IlmHistogramResult* out);

/* Measurement hook (tools/brightness_time.py): queues the luminance pass of the two calls above on the context's stream and returns --
 * nothing is read back, nothing synchronises.  Same refusals. */
int32_t ilm_debug_queue_luminance(IlmHandle lightmap, int32_t render_width, int32_t render_height, int32_t accuracy_factor);

/* ---- distance-field views (the reference's debug view of a field) ----------------------------------------------------------
 *
 * LightingRenderer.VisualizeDistanceField (Illuminant/Lighting/LightingRenderer.cs:1699-1892) draws one quad and sphere-traces the field
 * per pixel: techniques ObjectSurfaces / ObjectOutlines (Illuminant/Shaders/VisualizeDistanceField.fx:40-100, traceSurface / traceOutlines /
 * estimateNormal4 of VisualizeCommon.fxh:47-133).  One launch here, onto a lightmap object used as the render target (any format), blended
 * like ilm_render_particles; the field is read where it lies -- a host no longer downloads the atlas to look at it.
 *
 * The quad: four vertices in the order TL, TR, BR, BL (:1808-1833) whose Positions are an axis-aligned rectangle; RayVector and Color
 * are the same in all four (the reference gives them the same); Position.z is ignored (VisualizeVertexShader writes z = 0).  What the
 * reference leaves to the rasteriser is defined here, in fp32 with one rounding per operation in the order written:
 *     px0 = (quad[0].Position.x - ViewportPosition.x) * ViewportScale.x, px1 the same from quad[1]; py0 from quad[0].Position.y, py1 from
 *     quad[3].Position.y; pixel (i, j) is covered iff px0 <= i + 0.5 < px1 and py0 <= j + 0.5 < py1 (the top-left rule), pixels outside
 *     the target are clipped;  u = ((i + 0.5) - px0) / (px1 - px0), v likewise;
 *     top = TL + (TR - TL) * u, bottom = BL + (BR - BL) * u, rayStart = top + (bottom - top) * v on the RayStart components
 * (for the reference's parallelogram, :1801-1804, this is barycentric interpolation up to rounding).  An empty rectangle draws nothing.
 * rayLength = sqrt((x x + y y) + z z) of RayVector and rayDirection = RayVector / rayLength are computed once by the call, on the host.
 *
 * The pixel: ILM_VISUALIZE_SURFACES is ObjectSurfacesPixelShader (TRACE_MIN_STEP_SIZE 2, TRACE_FINAL_MIN_STEP_SIZE 12; a hit is
 * AmbientColor + LightColor * clamp((dot(estimateNormal4, LightDirection) + 0.05) * 1.1, 0, 1) * Color.rgb with alpha 1, a miss is
 * discarded), ILM_VISUALIZE_OUTLINES is ObjectOutlinesPixelShader with FilledInterior = 0, ILM_VISUALIZE_SILHOUETTES with FilledInterior = 1
 * (:1878; a ray that never meets distance <= 1 still gets the outline alpha of its closest distance); alpha <= 0 is discarded.  HLSL's
 * min / max are fminf / fmaxf.  Discarded and uncovered pixels keep their bits; the others are blended, ILM_BLEND_ALPHA (the reference's
 * default, :1851) dst = src + dst * (1 - src.a) or ILM_BLEND_ADDITIVE dst = src + dst.
 * The trace loops end: every iteration adds at least 2 to the position along the ray and rayLength is at most 65536 -- at most 32 769
 * iterations, whatever the field holds (the kernel carries an iteration cap just above that, which can never change a result).
 *
 * Refused with ILM_ERR_INVALID_ARGUMENT, nothing queued or written: Positions that are not an axis-aligned rectangle in TL, TR, BR, BL
 * order; a RayVector or Color that differs between vertices; a vertex or parameter value that is not finite; |RayVector| outside
 * [1e-3, 65536]; an unknown Mode or BlendMode; OutlineSize below 1 (or NaN) in the outline modes (the reference binds
 * Math.Max(outlineSize, 1), :1877); distance-field uniforms ilm_render_sphere_lights would refuse.  The vertex and parameter values are
 * judged before any handle is looked up (they need no object), so a host can learn them without a device.  Then: ctx, sdf != 0 and target
 * must be live handles (ILM_ERR_INVALID_HANDLE); sdf == 0 is ILM_ERR_STATE (the reference returns Failed without a field, :1713); the
 * target must belong to ctx (ILM_ERR_INVALID_ARGUMENT, as ilm_render_particles); the field may be ctx's or a sibling context's, ordered
 * against its owner's writes as ilm_render_sphere_lights orders it.  Asynchronous on ctx's stream unless out_stats is given.
 * out_stats (may be NULL): [0] covered pixels, [1] pixels drawn (not discarded), [2] sampleDistanceFieldEx calls (the trace's, plus the
 * normal's four per surface hit).
 *
 * Not built: the single-object techniques FunctionSurface / FunctionOutline (VisualizeDistanceFunction.fx).  The reference binds a float
 * angle (singleObject.Rotation ?? 0, :1874) to FunctionRotation and hands it to evaluateByTypeId, whose rotation parameter is a
 * quaternion float4 (DistanceFunctionCommon.fxh:167-169): what that computes is not defined by the text.  Refused rather than guessed.
 *
 * (The two structs below are untagged typedefs; tests/test_visualize_kat.py holds their layout to the ctypes mirrors.) */
/* VisualizeDistanceFieldVertex, Vertices.cs:143-148 (Sequential, Pack = 4: 52 bytes) */
typedef struct { float Position[3], RayStart[3], RayVector[3], Color[4]; } IlmVisualizeVertex;
enum { ILM_VISUALIZE_SURFACES = 0, ILM_VISUALIZE_OUTLINES = 1, ILM_VISUALIZE_SILHOUETTES = 2 };  /* VisualizationMode, LightingRenderer.cs:2055-2059 */
typedef struct {
    int32_t Mode, BlendMode;            /* ILM_VISUALIZE_*, ILM_BLEND_ALPHA (the reference's default) / ILM_BLEND_ADDITIVE */
    float   OutlineSize, _pad0;         /* Math.Max(outlineSize, 1), LightingRenderer.cs:1877; read in the outline modes only */
    float   AmbientColor[3], _pad1, LightDirection[3], _pad2, LightColor[3], _pad3;   /* :1860-1868; the host normalises the direction */
    float   ViewportScale[2], ViewportPosition[2];   /* as IlmRasterizeParams: pixel = (Position.xy - ViewportPosition) * ViewportScale */
} IlmVisualizeParams;
int32_t ilm_visualize_distance_field(IlmHandle ctx, IlmHandle sdf, const IlmDistanceFieldUniforms* df,
                                     const IlmVisualizeVertex quad[4] /* TL, TR, BR, BL */, const IlmVisualizeParams* params,
                                     IlmHandle target, uint64_t* out_stats /* may be NULL: [0] covered pixels, [1] pixels drawn, [2] SDF samples */);

/* ---- multi-device groups (SURVEY 8e / 8b "ilm_ctx_create(device_ids, n)") --------------------------------------------------------
 *
 * The reference renders on one GraphicsDevice.  A group is the MI355X-native extension that keeps its call sites unchanged while
 * the work spreads over the GPUs of a node: the caller of LightingRenderer.RenderLighting (Illuminant/Lighting/LightingRenderer.cs:917-923)
 * still gets ONE composited lightmap per frame (:1004-1010), the caller of ParticleSystem.Update (Illuminant/Particles/ParticleSystem.cs:630-761)
 * still sees one liveness table.  Two shapes, same entry points afterwards:
 *   - in-process: one host process drives n devices (ilm_group_create) -- the shape of a C# host;
 *   - one process per GPU: every process creates its member with the same 128-byte id (ilm_group_unique_id on rank 0, handed to the
 *     others by the launcher) -- the shape of `torchrun` / MPI jobs.
 * Each member owns a context (ilm_group_ctx): replicated inputs -- the distance-field atlas, G-buffers, light ramps, randomness tables --
 * are ordinary per-context objects the host creates in a loop over the members (the atlas is 25 MB; generating it per device is
 * cheaper than broadcasting it).  Ranks number the members of the whole group: rank = first_rank + local index.
 *
 * Lighting: the frame is cut into `world` strips of whole 16-row tile bands, equal slots of R rows (world * R >= height); every member
 * renders its strip into its own full-frame buffer and the strips are all-gathered IN PLACE, so every device ends with the composited
 * frame.  Particles: chunks never interact (ParticleSystem.cs:743-745), chunk c lives on rank c % world as that member's chunk
 * c / world; the per-step data path has no collective, only the per-chunk live counts are gathered (ilm_group_live_counts). */

enum {
    ILM_GATHER_NONE = 0,  /* strips stay where they were rendered (a host that reads every strip back itself) */
    ILM_GATHER_PEER = 1,  /* in-process groups: every member pushes its strip to the n - 1 others with hipMemcpyPeerAsync -- one
                             transfer per xGMI link, all links of the full mesh busy at once */
    ILM_GATHER_RCCL = 2,  /* ncclAllGather on the members' context streams (RCCL over xGMI; the only exchange between processes) */
    ILM_GATHER_ASYNC = 0x100, /* flag, OR'ed onto ILM_GATHER_PEER / ILM_GATHER_RCCL (r05): the exchange runs on a second stream of every member,
                             behind the strip just queued, and the member's context stream goes on -- with the next frame's strip into ANOTHER
                             group lightmap (a ring of two, the reference's BufferRing).  ilm_group_lightmap_wait orders later work behind it. */
    ILM_GATHER_STORE = 3  /* (r05; in-process groups through peer access, groups that span processes through IPC-mapped buffers): no copy phase at all -- the light kernel's final store writes every texel of a member's
                             strip at the same offset of EVERY member's copy of the frame (the others' buffers peer-mapped over xGMI:
                             n stores of 8 B per pixel), so the exchange overlaps the strip; what remains of the gather is a fence */
};

/* In-process group over `n` devices (ids may repeat: several members on one device, which is how the exchange paths are tested on a
 * one-GPU box; RCCL itself refuses duplicate devices).  Creates one context per member. */
int32_t ilm_group_create(const int32_t* device_ids, int32_t n, IlmHandle* out_group);
/* One-process-per-GPU group: rank 0 obtains `id` (128 bytes) from ilm_group_unique_id and the launcher hands it to every rank; all
 * `world` processes then call ilm_group_create_rank collectively (it creates the RCCL communicator). */
int32_t ilm_group_unique_id(void* out_id128);
int32_t ilm_group_create_rank(int32_t device_id, int32_t rank, int32_t world, const void* id128, IlmHandle* out_group);
/* Destroys the member contexts too; ILM_ERR_STATE while group lightmaps or objects of the member contexts are alive. */
int32_t ilm_group_destroy(IlmHandle group);
/* out_local = members in this process, out_world = members of the whole group, out_first_rank = rank of local member 0,
 * out_comm_ranks = the rank count the RCCL communicator itself reports (ncclCommCount; 0 while no communicator exists). */
int32_t ilm_group_info(IlmHandle group, int32_t* out_local, int32_t* out_world, int32_t* out_first_rank, int32_t* out_comm_ranks);
int32_t ilm_group_ctx(IlmHandle group, int32_t local_index, IlmHandle* out_ctx);
int32_t ilm_group_sync(IlmHandle group);

/* In-place all-gather of device buffers: buffers[i] (on local member i's device) holds world * bytes_per_rank bytes and rank r's
 * slot starts at r * bytes_per_rank; on return (stream-ordered on each member's context stream) every buffer holds every slot.
 * This is the primitive under ilm_group_lightmap_gather; a host uses it directly for the optional Pos+Life all-gather of SURVEY 8e
 * (planes from ilm_chunk_device_ptr) when a global consumer exists. */
int32_t ilm_group_all_gather(IlmHandle group, void* const* buffers, uint64_t bytes_per_rank, int32_t gather);

/* Small HOST payloads across the group (timings, counters; <= 1 MiB per rank): local = n_local * bytes_per_rank bytes, one slot per
 * local member in member order; out_all receives world * bytes_per_rank bytes, rank r's slot at r * bytes_per_rank, identical on every
 * process.  Waits for the members' queued work first, so it is also the barrier a host brackets a timed region with. */
int32_t ilm_group_host_all_gather(IlmHandle group, const void* local, void* out_all, uint32_t bytes_per_rank);

/* The composited lightmap of a group: one buffer of world * R rows per local member (the frame is its first `height` rows). */
int32_t ilm_group_lightmap_create(IlmHandle group, int32_t width, int32_t height, int32_t format, IlmHandle* out_group_lightmap);
/* The plain lightmap object (aliasing the member's buffer) that per-context calls -- particle lights, resolve, download -- take. */
int32_t ilm_group_lightmap_member(IlmHandle group_lightmap, int32_t local_index, IlmHandle* out_lightmap);
/* Rows [*out_row_begin, *out_row_end) of the frame that rank `rank` renders, and the slot height R. */
int32_t ilm_group_lightmap_strip(IlmHandle group_lightmap, int32_t rank, int32_t* out_row_begin, int32_t* out_row_end, int32_t* out_slot_rows);
/* Replaces the equal slots by other strips: row_begins[r], row_ends[r] for every rank r of the group (world entries each), contiguous in
 * rank order, whole 16-row tile bands, covering [0, height) -- cost-balanced strips when the lights are unevenly spread (SURVEY 8e;
 * the reference has one device and no such notion).  Every process of the group must install the same table: with one process per GPU
 * the call is ALWAYS a COLLECTIVE (r05) -- every rank, also one that was handed a malformed table and one that resets to the equal slots
 * with NULL, NULL, enters the same 8-byte host all-gather with a hash of its argument, and all ranks succeed or fail together: they return
 * ILM_ERR_STATE (ILM_ERR_INVALID_ARGUMENT on the rank whose own table is malformed) and keep the table they had when the arguments differ
 * or any of them is malformed (each rank sizes its sends and receives from its own copy).  Unequal strips are
 * exchanged range by range at their true rows (ILM_GATHER_PEER: peer copies; ILM_GATHER_RCCL: one group of ncclSend / ncclRecv, one
 * transfer per xGMI link and direction) instead of by the single in-place all-gather.  NULL, NULL restores the equal slots. */
int32_t ilm_group_lightmap_set_strips(IlmHandle group_lightmap, const int32_t* row_begins, const int32_t* row_ends);
int32_t ilm_group_lightmap_gather(IlmHandle group_lightmap, int32_t gather);
/* After ilm_group_lightmap_gather(..., mode | ILM_GATHER_ASYNC): every member's context stream waits for that exchange (stream-ordered,
 * nothing blocks the host).  Call it before anything reads the composited frame and before the lightmap is rendered into again
 * (ilm_group_render_sphere_lights does it itself); a no-op when no asynchronous exchange is pending.  A host keeps two group lightmaps
 * and alternates: strip N + 1 is rendered while strip N travels.  ilm_group_sync / ilm_group_host_all_gather drain the exchange streams too. */
int32_t ilm_group_lightmap_wait(IlmHandle group_lightmap);
/* Arms (enable != 0) or disarms the store-mode exchange: while armed, EVERY light pass into a member's lightmap (ilm_render_sphere_lights,
 * ilm_render_particle_lights through ilm_group_lightmap_member's handle) also stores its texels into the other members' copies of the frame, and
 * ilm_group_lightmap_gather(ILM_GATHER_STORE) is the fence that orders each member's later readers behind the other members' passes --
 * call it after the strips of a frame, and again in front of the next frame's strips when readers of the old frame may still be queued
 * (a pass overwrites the other members' copies as it runs).  ilm_group_render_sphere_lights(..., ILM_GATHER_STORE) does all of this
 * itself for one call.  In-process groups need peer access between their devices (ILM_ERR_STATE otherwise).  For a group that spans
 * processes the call is a COLLECTIVE (arming and disarming alike; destroying an armed lightmap disarms it): every rank exports its buffer
 * as an IPC handle (hipIpcGetMemHandle), the handles are all-gathered, every rank maps the others' (hipIpcOpenMemHandle) -- and either
 * every rank arms or none does (ILM_ERR_STATE on all); the fence of ILM_GATHER_STORE is then an 8-byte collective on the context streams.
 * The mappings are made once per group lightmap, PROVEN before anybody arms (every rank writes a stamp through each of its mappings
 * and finds every other rank's stamp in its own buffer; the bytes underneath are restored) and kept until the GROUP is destroyed --
 * disarming, re-arming and destroying the lightmap unmap nothing (unmapping and re-exporting inside one process was measured to
 * resolve handles to the wrong buffer on ROCm 7.2: DESIGN.md section 5).
 * The table follows the BUFFER: a lightmap object the host made around a member's texels on the member's context (ilm_lightmap_create
 * with external_device_ptr = ilm_lightmap_device_ptr(member)) is mirrored exactly like the member handle itself; such an object on ANOTHER
 * context (a sibling's) is refused by the light passes with ILM_ERR_STATE while the mode is armed (its stream is outside the fence).
 * ONLY the light passes are mirrored: ilm_lightmap_clear, ilm_lightmap_upload, ilm_render_particles and ilm_resolve_lighting into an armed
 * member (or an alias of its texels) write THAT member's copy alone -- the members' frames stay equal only if every member makes the same
 * call (a host that clears or uploads per frame does it on every member, as it creates the replicated inputs).
 * Synchronises the members' streams.  The reference has one device and one lightmap
 * (Illuminant/Lighting/LightingRenderer.cs:1004-1010): every member still ends with that one composited frame. */
int32_t ilm_group_lightmap_store_mode(IlmHandle group_lightmap, int32_t enable);
int32_t ilm_group_lightmap_destroy(IlmHandle group_lightmap);

/* ilm_render_sphere_lights for the whole group: every local member renders its strip (same lights, environment and uniforms;
 * gbuffers / sdfs = one handle per local member, objects of that member's context, NULL / 0 as in the single-device call), then the
 * strips are gathered.  stats (may be NULL) = sums over the local members. */
int32_t ilm_group_render_sphere_lights(IlmHandle group, const IlmLightVertex* lights, int32_t light_count,
                                       const IlmEnvironment* env, const IlmDistanceFieldUniforms* df,
                                       const IlmHandle* gbuffers, const IlmHandle* sdfs, const float ambient[4],
                                       IlmHandle group_lightmap, int32_t gather, IlmRenderStats* stats);

/* Liveness table of a sharded particle system: systems[i] = local member i's system (chunk c of the table = chunk c / world of rank
 * c % world); out_counts[c] = live count of chunk c from each member's last counting step, identical on every process (integers,
 * bit-exact).  One small RCCL all-gather when the group spans processes, none otherwise.  Synchronises. */
int32_t ilm_group_live_counts(IlmHandle group, const IlmHandle* systems, int32_t total_chunks, uint32_t* out_counts, int32_t capacity,
                              int32_t saturate16);

/* The sharded particle state made whole ("optional all-gather of Pos+Life, 16 B/slot, only when a global consumer
 * exists -- particle lights, host readback").  sources[i] = local member i's system (chunk c of the table = chunk c / world of rank
 * c % world, as for ilm_group_live_counts); gathered[i] = an ordinary system on the SAME member's context whose engine has the same
 * chunk size and which holds total_chunks chunks (ilm_system_add_chunk).  After the call (stream-ordered on the members' context
 * streams, nothing blocks the host) components [first_component, first_component + component_count) of chunk c of every gathered
 * system are those of chunk c of the table: 0..3 = Pos+Life (ParticleSystem.cs:73-146 PositionAndLife), 12..15 = RenderColor (what
 * ParticleLight.fx:16-83 reads beside the position).  The planes of a chunk are contiguous, so a chunk travels as one range from the
 * owner's planes into the destination's planes, no packing: ILM_GATHER_PEER (in-process groups) = hipMemcpyPeerAsync to each other
 * member; ILM_GATHER_RCCL = one group of ncclSend / ncclRecv per call; ILM_GATHER_NONE = only each member's own chunks are copied over.
 * Every other component of the gathered system is left as it is.  Any consumer that takes a system handle then sees the whole table in
 * chunk order: ilm_render_particle_lights(ctx, gathered, ...) lights a member's strip with EVERY rank's particles, in the order -- and
 * therefore with the bits -- of the one-context frame.  A collective when the group spans processes: every rank calls it with the same
 * total_chunks, components and mode. */
int32_t ilm_group_gather_chunks(IlmHandle group, const IlmHandle* sources, const IlmHandle* gathered, int32_t total_chunks,
                                int32_t first_component, int32_t component_count, int32_t gather);


#ifdef __cplusplus
}
#endif
#endif /* ILLUMINANT_HIP_H */
