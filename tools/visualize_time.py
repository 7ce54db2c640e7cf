#!/usr/bin/env python3
"""What a distance-field view costs on the device (docs/experiments.md, "Distance-field views").

On cfg3's field (2048 x 2048 x 128 units at 1/4 texel per unit, 33 slices in a 3 x 4 unorm16 atlas, 256 random obstructions generated
by ilm_sdf_render_slices) a 1920 x 1080 HalfVector4 target is viewed in the three modes, top-down and obliquely:
  ms            one ilm_visualize_distance_field launch, HIP events around `block` queued launches (median over `--blocks` blocks after a
                warm-up block; ilm_timer_*)
  samples       the call's own sampleDistanceFieldEx count, from the counting instantiation, run separately from the timed launches
  download_ms   ilm_sdf_download of that field: what a host pays today before it can look at anything
and, in the same run, cfg3's sphere-light frame (64 lights, no G-buffer) with its SDF sample count, so the divergent march's sample
rate stands beside the cone trace's from the same machine.
Prints one JSON line; --out FILE also writes it there.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from illuminant_amd import abi, native, scenes  # noqa: E402

MODES = (("surfaces", abi.VISUALIZE_SURFACES), ("outlines", abi.VISUALIZE_OUTLINES), ("silhouettes", abi.VISUALIZE_SILHOUETTES))
VIEWS = (("top-down", (0.0, 0.0, -1.0)), ("oblique", (0.3, 0.5, -0.8)))


def median_ms(ctx, blocks, block, body):
    times = []
    for b in range(blocks + 1):
        ctx.sync()
        ctx.timer_start()
        for _ in range(block):
            body()
        ms = ctx.timer_stop() / block
        if b > 0:                   # the first block warms up (allocations, code objects)
            times.append(ms)
    return statistics.median(times), min(times)


def camera_quad(extent, direction, width, height):
    """A view plane in front of the field's centre, against the view direction, a little larger than the field's footprint; rays of
    twice the field's diagonal (LightingRenderer.cs:1763)."""
    extent = np.asarray(extent, np.float64)
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    right = np.cross(d, (0.0, 1.0, 0.0))
    right = right / np.linalg.norm(right)
    down = -np.cross(d, right)
    diagonal = float(np.linalg.norm(extent))
    origin = extent / 2 - d * (0.6 * diagonal)
    half = (0.55 * extent[0], 0.55 * extent[0] * height / width)
    quad = (abi.VisualizeVertex * 4)()
    for i, (x, y, sr, sd) in enumerate(((0, 0, -1, -1), (width, 0, 1, -1), (width, height, 1, 1), (0, height, -1, 1))):
        start = origin + right * (sr * half[0]) + down * (sd * half[1])
        for k in range(3):
            quad[i].Position[k] = float((x, y, 0)[k])
            quad[i].RayStart[k] = float(start[k])
            quad[i].RayVector[k] = float(np.float32(d[k] * 2 * diagonal))
        for k in range(4):
            quad[i].Color[k] = 1.0
    return quad


def view_params(mode):
    p = abi.VisualizeParams()
    p.Mode, p.BlendMode, p.OutlineSize = mode, abi.BLEND_ALPHA, 1.8
    ld = np.array([0.0, -0.5, -1.0]) / np.linalg.norm([0.0, -0.5, -1.0])
    for k in range(3):
        p.AmbientColor[k], p.LightDirection[k], p.LightColor[k] = (0.1, 0.15, 0.15)[k], float(ld[k]), 0.75
    p.ViewportScale[0] = p.ViewportScale[1] = 1.0
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert native.device_count() > 0, "needs a GPU: there is no CPU path"
    ctx = native.Context(args.device)
    lib = native.lib()
    width, height, world = 1920, 1080, 2048
    layout = scenes.DistanceFieldLayout(world, world, 128.0, 32, 0.25, 128)
    obstacles = [(typ - 1, center, size) for (typ, center, size) in scenes.random_obstacles(11, 256, (world, world))]
    field = native.DistanceFieldTexture(ctx, None, abi.SDF_UNORM16, size=(layout.atlas_width, layout.atlas_height))
    field.render_slices(scenes.render_desc(layout), list(range(0, layout.slice_count, 3)), scenes.obstruction_array(obstacles))
    dfu = layout.uniforms(power=0.7, min_step_size=1.0, long_step_factor=0.5)
    target = native.Lightmap(ctx, width, height, abi.LIGHTMAP_HALF4)
    rows = []
    for view_name, direction in VIEWS:
        quad = camera_quad((world, world, 128.0), direction, width, height)
        for mode_name, mode in MODES:
            p = view_params(mode)
            target.clear((0.0, 0.0, 0.0, 1.0))
            stats = native.visualize_distance_field(ctx, field, dfu, quad, p, target, want_stats=True)
            ms = median_ms(ctx, args.blocks, args.block, lambda: native.visualize_distance_field(ctx, field, dfu, quad, p, target))
            rows.append({"view": view_name, "mode": mode_name, "ms": ms[0], "ms_min": ms[1], "covered_pixels": stats[0], "pixels_drawn": stats[1],
                         "sdf_samples": stats[2], "samples_per_pixel": stats[2] / max(stats[0], 1), "gsamples_per_s": stats[2] / (ms[0] * 1e-3) / 1e9})
    host = np.empty((layout.atlas_height, layout.atlas_width, 4), np.uint16)
    download = median_ms(ctx, args.blocks, 2, lambda: native.check(lib.ilm_sdf_download(field.handle, host.ctypes.data_as(C.c_void_p))))
    # cfg3's sphere lights over the same field (no G-buffer): the cone trace's sample rate on this machine, in this run
    lights = scenes.random_lights(12, 64, width, height, z=(8.0, 64.0), radius=24.0, ramp=(200.0, 550.0))
    lights = (abi.LightVertex * len(lights))(*lights)
    env = scenes.environment()
    ambient = (0.05, 0.05, 0.05, 1.0)
    light_stats = native.render_sphere_lights(ctx, lights, env, dfu, None, field, ambient, target, want_stats=True)
    light_ms = median_ms(ctx, args.blocks, args.block, lambda: native.render_sphere_lights(ctx, lights, env, dfu, None, field, ambient, target))
    record = {"tool": "visualize_time", "blocks": args.blocks, "block": args.block, "target": [width, height], "target_format": "half4",
              "field": {"virtual": [world, world, 128], "atlas": [layout.atlas_width, layout.atlas_height], "format": "unorm16",
                        "bytes": int(host.nbytes), "obstructions": len(obstacles)},
              "rows": rows, "sdf_download_ms": download[0], "sdf_download_ms_min": download[1],
              "sphere_lights_cfg3": {"lights": len(lights), "ms": light_ms[0], "ms_min": light_ms[1], "sdf_samples": int(light_stats.SdfSamples),
                                     "gsamples_per_s": int(light_stats.SdfSamples) / (light_ms[0] * 1e-3) / 1e9}}
    target.close(); field.close(); ctx.close()
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
