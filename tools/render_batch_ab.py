"""A/B of RENDERING a frame of MANY small particle systems (the reference's Scenes/ManySystemsManySpawners.cs:78-81: 256 systems on an
engine of ChunkSize 128, each rendered every frame): A = one ilm_render_particles per system, B = one
ilm_engine_render_particles_batch for the frame.

Workload: N systems (16, 64, 256, 1024) of one chunk each with 2 048 spawned slots (the quad count Render passes), nearly all alive,
scattered over a 1920 x 1080 HALF4 target, sprites of a few pixels, rounded, alpha-blended (every fourth system additive).  A frame
is a clear of the target and the N draws.

Method: A and B run in the same process over the SAME systems (rendering only reads them) onto targets of their own, both warmed; blocks
of --frames frames alternate A, B, A, B ...; each block is timed with the host clock up to the end of an ilm_ctx_sync and with the
context's HIP events beside it.  Reported per N: median / minimum / maximum block time per frame for A and B, the sorts and tile launches
of B's frame (ilm_debug_last_render_batch), the statistics of one frame on either side (they must be equal) and the largest difference
between the two HALF4 pictures (A rounds to fp16 after every system, B once: a defined difference, reported, not judged).
The criterion is B's median below A's by more than A's own spread (max - min) at N = 256; the script states whether it holds.

  python tools/render_batch_ab.py [--frames 20] [--blocks 5] [--sizes 16,64,256,1024] [--out FILE]        (on the GPU box)
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from illuminant_amd import abi, native, scenes   # noqa: E402

CS = 128
SLOTS = CS * CS
QUADS = 2048
W, H = 1920, 1080
VARIANTS = 16                    # distinct chunk contents, shared round robin


def chunk_planes(seed):
    pos = np.zeros((SLOTS, 4), np.float32)
    pos[:QUADS, 0] = scenes.uniform(seed, (QUADS,), 0.0, float(W))
    pos[:QUADS, 1] = scenes.uniform(seed + 1, (QUADS,), 0.0, float(H))
    pos[:QUADS, 3] = np.where(scenes.uniform(seed + 2, (QUADS,)) < 0.05, 0.0, 1.0)
    a = scenes.uniform(seed + 3, (QUADS,), 0.1, 0.6)
    col = np.zeros((SLOTS, 4), np.float32)
    col[:QUADS, :3] = scenes.uniform(seed + 4, (QUADS, 3), 0.0, 1.0) * a[:, None]
    col[:QUADS, 3] = a
    rd = np.zeros((SLOTS, 4), np.float32)
    rd[:QUADS, 0] = scenes.uniform(seed + 5, (QUADS,), 1.0, 3.0)           # half extent in pixels
    rd[:QUADS, 1] = scenes.uniform(seed + 6, (QUADS,), 0.0, 6.0)
    return pos, col, rd


def run(ctx, variants, n, frames, blocks, warm, emit):
    lib = native.lib()
    engine = native.Engine(ctx, CS, scenes.randomness_table(7))
    systems = []
    for i in range(n):
        s = native.System(engine)
        s.add_chunk()
        pos, col, rd = variants[i % VARIANTS]
        s.upload(0, abi.PLANE_POSITION, pos); s.upload(0, abi.PLANE_RENDER_COLOR, col); s.upload(0, abi.PLANE_RENDER_DATA, rd)
        systems.append(s)
    quads = (C.c_int32 * 1)(QUADS)
    items = (abi.RasterizeItem * n)()
    params = []
    for i, s in enumerate(systems):
        p = scenes.rasterize_params(rounded=True, blend=abi.BLEND_ADDITIVE if i % 4 == 3 else abi.BLEND_ALPHA,
                                    global_color=(1.0, 0.9, 0.8, 0.9), origin=(float(i % 13), float(i % 7)))
        params.append(p)
        items[i].System, items[i].QuadCounts, items[i].ChunkCount = s.handle.value, C.addressof(quads), 1
        C.memmove(C.byref(items[i], abi.RasterizeItem.Params.offset), C.byref(p), C.sizeof(p))
    calls = [(abi.Handle(s.handle.value), C.cast(C.byref(p), C.c_void_p)) for s, p in zip(systems, params)]
    targets = {"A": native.Lightmap(ctx, W, H, abi.LIGHTMAP_HALF4), "B": native.Lightmap(ctx, W, H, abi.LIGHTMAP_HALF4)}
    black = (C.c_float * 4)(0.02, 0.03, 0.04, 1.0)
    quads_p, items_p = C.cast(quads, C.c_void_p), C.cast(items, C.c_void_p)

    def frame_a(stats=None):
        t = targets["A"]
        native.check(lib.ilm_lightmap_clear(t.handle, black))
        total = [0, 0, 0]
        out = (C.c_uint64 * 3)()
        for h, p in calls:
            rc = lib.ilm_render_particles(h, quads_p, 1, p, t.handle, C.cast(out, C.c_void_p) if stats else None)
            if rc != 0:
                native.check(rc)
            if stats:
                total = [x + int(y) for x, y in zip(total, out)]
        return tuple(total)

    def frame_b(stats=None):
        t = targets["B"]
        native.check(lib.ilm_lightmap_clear(t.handle, black))
        out = (C.c_uint64 * 3)()
        native.check(lib.ilm_engine_render_particles_batch(engine.handle, items_p, n, t.handle, C.cast(out, C.c_void_p) if stats else None))
        return tuple(int(x) for x in out)

    for _ in range(warm):
        frame_a(); frame_b()
    ctx.sync()
    times = {"A": [], "B": []}
    events = {"A": [], "B": []}
    for block in range(blocks):
        for name, frame in (("A", frame_a), ("B", frame_b)):
            ctx.sync()
            ctx.timer_start()
            t0 = time.perf_counter()
            for _ in range(frames):
                frame()
            ctx.sync()
            times[name].append((time.perf_counter() - t0) / frames * 1e6)
            events[name].append(ctx.timer_stop() / frames * 1e3)
    diag = engine.last_render_batch()
    stats_a, stats_b = frame_a(True), frame_b(True)
    pa = targets["A"].download().astype(np.float32)
    pb = targets["B"].download().astype(np.float32)
    med = lambda v: sorted(v)[len(v) // 2]
    row = {"n": n}
    for name in ("A", "B"):
        row[name] = (med(times[name]), min(times[name]), max(times[name]), med(events[name]))
        emit("N=%4d %s: host clock median %9.1f min %9.1f max %9.1f us/frame   HIP events median %9.1f us/frame   (%d blocks of %d frames)" % (
            n, name, row[name][0], row[name][1], row[name][2], row[name][3], blocks, frames))
    emit("N=%4d    per frame: A %d calls (a host synchronisation and a sort each); B %d item(s), %d sort(s), %d tile launch(es)" % (n, n, diag[0], diag[1], diag[2]))
    emit("N=%4d    (live quads, pairs, shaded pixels) of a frame: A %s  B %s  %s" % (n, stats_a, stats_b, "equal" if stats_a == stats_b else "DIFFERENT"))
    emit("N=%4d    largest |A - B| over the HALF4 pictures: %.4g (A rounds after every system, B once); largest value %.4g" % (
        n, float(np.abs(pa - pb).max()), float(np.abs(pb).max())))
    spread = row["A"][2] - row["A"][1]
    emit("N=%4d    A / B = %.2f (medians); A's block-to-block spread %.1f us/frame; B's median is %s A's by more than that" % (
        n, row["A"][0] / row["B"][0], spread, "below" if row["A"][0] - row["B"][0] > spread else "NOT below"))
    row["stats_equal"] = stats_a == stats_b
    row["wins"] = row["A"][0] - row["B"][0] > spread
    for t in targets.values():
        t.close()
    for s in systems:
        s.close()
    engine.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--sizes", default="16,64,256,1024")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    ctx = native.Context(0)
    variants = [chunk_planes(3000 + 10 * k) for k in range(VARIANTS)]
    emit("# tools/render_batch_ab.py: A = ilm_render_particles per system, B = one ilm_engine_render_particles_batch per frame; chunk size %d, "
         "%d quads per system, %d x %d HALF4 target" % (CS, QUADS, W, H))
    rows = [run(ctx, variants, int(n), args.frames, args.blocks, args.warm, emit) for n in args.sizes.split(",")]
    ok = all(r["stats_equal"] for r in rows)
    at256 = [r for r in rows if r["n"] == 256]
    if at256:
        emit("# criterion at N = 256: %s" % ("B wins by more than A's spread" if at256[0]["wins"] else "B does NOT win by more than A's spread"))
    emit("# statistics: %s" % ("all equal" if ok else "NOT all equal"))
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
