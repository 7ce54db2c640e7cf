"""A/B of LIGHTING a frame from MANY particle systems: A = one ilm_render_particle_lights per system (the loop of one render state per
ParticleLightSource, LightingRenderer.cs:1126-1141), B = one ilm_engine_render_particle_lights_batch for the frame.

Workload: the 4 096 particle lights of bench.py's 1080p particle-light row (cfg3's field and ground-plane G-buffer, radius 4, ramp 60, the
renderer's HALF4 lightmap), the SAME particles in the same order split evenly over K = 1, 16, 64, 256 systems of one engine (chunk size 64;
a system's quad count is its share + 1, as RenderChunk passes it).  A frame is ilm_lightmap_clear and the light calls.

Method: before anything is timed, each K's batch frame is held to the loop's frame on FLOAT4 lightmaps -- no texel outside 1e-4 x |loop| +
1e-5 x the component's largest value, the statistics equal -- or the script stops.  Then A and B run in the same process over the same
systems onto HALF4 lightmaps of their own, both warmed at every K; blocks of --frames frames alternate A, B, A, B ...; each block is timed
with the host clock up to the end of an ilm_ctx_sync, the context's HIP events beside it.  The K = 1 loop's blocks give the noise floor
(max - min of its block times).  Criteria: B at K = 1 within that spread of A at K = 1; B at every K >= 16 not slower than A beyond it.

  python tools/particle_light_batch_ab.py [--frames 20] [--blocks 5] [--sizes 1,16,64,256] [--out FILE]           (on the GPU box)
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/particle_light_batch_ab.py --only A --sizes 256 --frames 50   (a trace of its own)
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from illuminant_amd import abi, native, scenes  # noqa: E402

LIGHTS, CS, W, H = 4096, 64, 1920, 1080
AMBIENT = (0.05, 0.05, 0.05, 1.0)


def build(Host, hctx, k, particles):
    """k systems of one engine holding the LIGHTS particles in order, one step each so that RenderColor is populated"""
    pos, vel, attr = particles
    engine = Host.ParticleEngine(hctx, Host.ParticleEngineConfiguration(CS), scenes.randomness_table(7))
    pcfg = Host.ParticleSystemConfiguration()
    pcfg.LifeDecayPerSecond = 0.01
    share = LIGHTS // k
    systems = []
    for i in range(k):
        s = Host.ParticleSystem(engine, pcfg)
        a, b = i * share, (i + 1) * share
        s.Spawn(share, pos[a:b], vel[a:b], attr[a:b])
        s.Update(0)
        systems.append(s)
    return engine, systems, share


def run(Host, hctx, ctx, L, k, particles, args, emit):
    lib = native.lib()
    r = L["renderer"]
    engine, systems, share = build(Host, hctx, k, particles)
    pls = Host.ParticleLightSource()
    tmpl = Host.SphereLightSource()
    tmpl.Radius = 4.0; tmpl.RampLength = 60.0; tmpl.Color = [1.0, 0.9, 0.8, 1.0]
    pls.Template = tmpl
    params = abi.ParticleLightParams.from_buffer_copy(Host.LightingRenderer.PackParticleLightBytes(pls, True))
    env = abi.Environment.from_buffer_copy(r.GetEnvironmentUniformsBytes())
    dfu = abi.DistanceFieldUniforms.from_buffer_copy(r.GetDistanceFieldUniformsBytes())
    env_p, dfu_p, params_p = (C.cast(C.byref(x), C.c_void_p) for x in (env, dfu, params))
    gb, sdf = abi.Handle(r.GBufferHandle), abi.Handle(L["field"].TextureHandle)
    quads = (C.c_int32 * 1)(min(CS * CS, share + 1))
    quads_p = C.cast(quads, C.c_void_p)
    items = (abi.ParticleLightItem * k)()
    for i, s in enumerate(systems):
        items[i].System, items[i].QuadCounts, items[i].ChunkCount, items[i].Params = s.Handle, C.addressof(quads), 1, params
    items_p = C.cast(items, C.c_void_p)
    handles = [abi.Handle(s.Handle) for s in systems]
    engine_h = abi.Handle(engine.Handle)
    clear = (C.c_float * 4)(*AMBIENT)

    def frame_a(lm, stats=None):
        native.check(lib.ilm_lightmap_clear(lm.handle, clear))
        total = [0, 0, 0]
        st = abi.RenderStats()
        for h in handles:
            rc = lib.ilm_render_particle_lights(ctx.handle, h, quads_p, 1, params_p, env_p, dfu_p, gb, sdf, lm.handle, 0, H,
                                                C.cast(C.byref(st), C.c_void_p) if stats else None)
            if rc != 0:
                native.check(rc)
            if stats:
                total = [x + int(y) for x, y in zip(total, (st.SdfSamples, st.PixelLightPairs, st.TracedPairs))]
        return tuple(total)

    def frame_b(lm, stats=None):
        native.check(lib.ilm_lightmap_clear(lm.handle, clear))
        st = abi.RenderStats()
        native.check(lib.ilm_engine_render_particle_lights_batch(engine_h, items_p, k, env_p, dfu_p, gb, sdf, lm.handle, 0, H,
                                                                 C.cast(C.byref(st), C.c_void_p) if stats else None))
        return (int(st.SdfSamples), int(st.PixelLightPairs), int(st.TracedPairs))

    row = {"k": k}
    # ---- the frames agree, or nothing is timed --------------------------------------------------------------------------------------
    fa, fb = native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4), native.Lightmap(ctx, W, H, abi.LIGHTMAP_FLOAT4)
    stats_a, stats_b = frame_a(fa, True), frame_b(fb, True)
    pa, pb = fa.download().astype(np.float64), fb.download().astype(np.float64)
    fa.close(); fb.close()
    scale = np.abs(pa).reshape(-1, 4).max(axis=0)
    beyond = int((np.abs(pb - pa) > 1e-4 * np.abs(pa) + 1e-5 * scale).any(axis=-1).sum())
    di, dp, dt = C.c_int32(), C.c_int32(), C.c_int32()
    native.check(lib.ilm_debug_last_particle_light_batch(engine_h, C.byref(di), C.byref(dp), C.byref(dt)))
    diag = (di.value, dp.value, dt.value)
    emit("K=%4d    check on FLOAT4: %d of %d texels beyond 1e-4 |loop| + 1e-5 scale; largest |B - A| %.3g of %.3g; statistics A %s B %s %s" % (
        k, beyond, W * H, float(np.abs(pb - pa).max()), float(np.abs(pa).max()), stats_a, stats_b, "equal" if stats_a == stats_b else "DIFFERENT"))
    row["agree"] = beyond == 0 and stats_a == stats_b
    if not row["agree"]:
        return row
    # ---- timing ------------------------------------------------------------------------------------------------------------------------
    targets = {"A": native.Lightmap(ctx, W, H, abi.LIGHTMAP_HALF4), "B": native.Lightmap(ctx, W, H, abi.LIGHTMAP_HALF4)}
    frames = {"A": frame_a, "B": frame_b}
    names = [n for n in ("A", "B") if args.only in (None, n)]
    for _ in range(args.warm):
        for n in names:
            frames[n](targets[n])
    ctx.sync()
    times = {n: [] for n in names}
    events = {n: [] for n in names}
    for _ in range(args.blocks):
        for n in names:
            ctx.sync()
            ctx.timer_start()
            t0 = time.perf_counter()
            for _ in range(args.frames):
                frames[n](targets[n])
            ctx.sync()
            times[n].append((time.perf_counter() - t0) / args.frames * 1e3)
            events[n].append(ctx.timer_stop() / args.frames)
    med = lambda v: sorted(v)[len(v) // 2]
    for n in names:
        row[n] = (med(times[n]), min(times[n]), max(times[n]), med(events[n]))
        emit("K=%4d %s: host clock median %8.4f min %8.4f max %8.4f ms/frame   HIP events median %8.4f ms/frame   (%d blocks of %d frames)" % (
            k, n, row[n][0], row[n][1], row[n][2], row[n][3], args.blocks, args.frames))
    emit("K=%4d    launches per frame besides the clear: A %d (two preparation launches and the tile kernel per system); B %d preparation + %d tile "
         "(%d items)" % (k, 3 * k, diag[1], diag[2], diag[0]))
    for t in targets.values():
        t.close()
    del systems, engine
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--sizes", default="1,16,64,256")
    ap.add_argument("--only", choices=("A", "B"), default=None, help="time one variant alone (a profiler run of its own)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    from illuminant_amd import _host as Host
    hctx = Host.DeviceContext(0)
    ctx = native.Context(0, borrowed_handle=hctx.Handle)
    L = bench.build_lighting(Host, hctx, scenes, abi, W, H, 0, 0.25, 2048, abi.SDF_UNORM16)
    particles = scenes.make_particles(91, LIGHTS, pos_lo=(0, 0, 4), pos_hi=(W, H, 48), life=(50.0, 90.0))
    emit("# tools/particle_light_batch_ab.py: A = ilm_render_particle_lights per system, B = one ilm_engine_render_particle_lights_batch per frame; "
         "%d particle lights over K systems, %d x %d HALF4 lightmap, cfg3's field and G-buffer" % (LIGHTS, W, H))
    rows = [run(Host, hctx, ctx, L, int(k), particles, args, emit) for k in args.sizes.split(",")]
    ok = all(r["agree"] for r in rows)
    emit("# frames and statistics: %s" % ("B agrees with A at every K" if ok else "B does NOT agree with A: nothing below counts"))
    base = [r for r in rows if r["k"] == 1 and "A" in r]
    if ok and base and args.only is None:
        spread = base[0]["A"][2] - base[0]["A"][1]
        emit("# noise floor: the K = 1 loop's %d blocks span %.4f ms/frame (min %.4f, max %.4f)" % (args.blocks, spread, base[0]["A"][1], base[0]["A"][2]))
        for r in rows:
            if r["k"] == 1:
                verdict = "within" if abs(r["B"][0] - r["A"][0]) <= spread else "NOT within"
                emit("# K =    1: B - A = %+.4f ms/frame (medians): %s the spread" % (r["B"][0] - r["A"][0], verdict))
            else:
                verdict = "not slower beyond the spread" if r["B"][0] <= r["A"][0] + spread else "SLOWER beyond the spread"
                emit("# K = %4d: A / B = %.2f (medians %.4f / %.4f ms/frame): B is %s" % (r["k"], r["A"][0] / r["B"][0], r["A"][0], r["B"][0], verdict))
        emit("# B from K = 1 to K = %d: %.4f -> %.4f ms/frame" % (rows[-1]["k"], base[0]["B"][0], rows[-1]["B"][0]))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
