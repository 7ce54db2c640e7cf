#!/usr/bin/env python3
"""What a frame of projector lights costs on the device (docs/experiments.md, "Projector lights").

Two frames, no G-buffer, HalfVector4 target, cfg3's quality settings (MinStepSize 1, LongStepFactor 0.5, MaxStepCount 64, MaxConeRadius
24, OcclusionToOpacityPower 0.7), the frames of tools/directional_time.py:
  cfg3   1920 x 1080 over cfg3's field (2048 x 2048 x 128 units at 1/4 texel per unit, unorm16, 256 random obstructions)
  cfg5   3840 x 2160 over cfg5's field (4096 x 4096 x 128 units at 1/8 texel per unit, fp16, the same obstructions' generator)
each lit by four shadowed projector lights through one 256 x 256 texture -- two clamped ones that cover a half of the frame each and
two wrapping ones that tile it, every one with an origin above the frame -- and, in the same run, by the configuration's own sphere
lights (64 / 256, bench.py's seeds) as the yardstick:
  ms            one call (record preparation + the pass), HIP events around a block of queued calls: median over `--blocks` blocks after a
                warm-up block, each block at least `--block` calls and enough of them to fill ~0.1 s of device time;
                projector_clear_only is the same call with zero lights
  samples       the call's own sampleDistanceFieldEx count, from the counting instantiation, run separately from the timed launches
  gsamples_per_s, and the projector pass's sample rate over the sphere pass's of the same field
Prints one JSON line; --out FILE also writes it there.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from illuminant_amd import abi, native, scenes  # noqa: E402


def light_array(lights):
    return (abi.LightVertex * len(lights))(*lights)


def forward(scale, translation):
    m = np.diag([scale[0], scale[1], scale[2], 1.0])
    m[3, :3] = translation
    return m


def projector_lights(width, height):
    """two clamped lights over the left and the right half of the frame (with a margin), two wrapping ones tiling it at different
    periods; origins above the frame's quarters, so that every trace is oblique and of a different length"""
    w, h = float(width), float(height)
    common = dict(radius=8.0, ramp_length=200.0, opacity=0.8)
    return [scenes.projector_light(forward((w * 0.46, h * 0.9, 128.0), (w * 0.02, h * 0.05, 0.0)), origin=(w * 0.25, h * 0.4, 120.0), **common),
            scenes.projector_light(forward((w * 0.46, h * 0.9, 128.0), (w * 0.52, h * 0.05, 0.0)), origin=(w * 0.75, h * 0.6, 110.0), **common),
            scenes.projector_light(forward((w * 0.31, h * 0.37, 128.0), (3.0, 5.0, 0.0)), origin=(w * 0.4, h * 0.8, 100.0), wrap=True, **common),
            scenes.projector_light(forward((w * 0.17, h * 0.23, 128.0), (7.0, 2.0, 0.0)), origin=(w * 0.6, h * 0.2, 90.0), wrap=True, **common)]


def median_ms(ctx, blocks, block, body, window_ms=100.0):
    """Median and minimum ms per launch over `blocks` timed blocks; the warm-up block also sizes the timed ones (tools/directional_time.py)"""
    times = []
    for b in range(blocks + 1):
        ctx.sync()
        ctx.timer_start()
        for _ in range(block):
            body()
        ms = ctx.timer_stop() / block
        if b > 0:
            times.append(ms)
        else:
            block = int(min(max(block, math.ceil(window_ms / max(ms, 1e-3))), 4000))
    return statistics.median(times), min(times), block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert native.device_count() > 0, "needs a GPU: there is no CPU path"
    assert args.blocks * args.block >= 20, "at least 20 timed launches"
    ctx = native.Context(args.device)
    env = scenes.environment()
    ambient = (0.05, 0.05, 0.05, 1.0)
    texture = scenes.uniform(5, (256, 256, 4), 0.2, 1.0)
    native.set_projector_texture(ctx, texture)
    frames = []
    for name, width, height, world, resolution, fmt, n_sphere, seed in (("cfg3", 1920, 1080, 2048, 0.25, abi.SDF_UNORM16, 64, 12),
                                                                         ("cfg5", 3840, 2160, 4096, 0.125, abi.SDF_FP16, 256, 13)):
        layout = scenes.DistanceFieldLayout(world, world, 128.0, 32, resolution, 128)
        obstacles = [(typ - 1, center, size) for (typ, center, size) in scenes.random_obstacles(11, 256, (world, world))]
        field = native.DistanceFieldTexture(ctx, None, fmt, size=(layout.atlas_width, layout.atlas_height))
        field.render_slices(scenes.render_desc(layout), list(range(0, layout.slice_count, 3)), scenes.obstruction_array(obstacles))
        dfu = layout.uniforms(power=0.7, min_step_size=1.0, long_step_factor=0.5)
        target = native.Lightmap(ctx, width, height, abi.LIGHTMAP_HALF4)
        sc = width / 1920.0
        spheres = scenes.random_lights(seed, n_sphere, width, height, z=(8.0, 64.0), radius=24.0, ramp=(200.0 * sc, 550.0 * sc))
        spheres = (abi.LightVertex * len(spheres))(*spheres)
        st = native.render_sphere_lights(ctx, spheres, env, dfu, None, field, ambient, target, want_stats=True)
        ms = median_ms(ctx, args.blocks, args.block, lambda: native.render_sphere_lights(ctx, spheres, env, dfu, None, field, ambient, target))
        sphere = {"lights": len(spheres), "ms": ms[0], "ms_min": ms[1], "launches_per_block": ms[2], "sdf_samples": int(st.SdfSamples), "pairs": int(st.PixelLightPairs),
                  "traced_pairs": int(st.TracedPairs), "gsamples_per_s": int(st.SdfSamples) / (ms[0] * 1e-3) / 1e9}
        ms = median_ms(ctx, args.blocks, args.block, lambda: native.render_projector_lights(ctx, None, env, dfu, None, field, ambient, target))
        clear = {"ms": ms[0], "ms_min": ms[1], "launches_per_block": ms[2]}
        lights = light_array(projector_lights(width, height))
        st = native.render_projector_lights(ctx, lights, env, dfu, None, field, ambient, target, want_stats=True)
        ms = median_ms(ctx, args.blocks, args.block, lambda: native.render_projector_lights(ctx, lights, env, dfu, None, field, ambient, target))
        rate = int(st.SdfSamples) / (ms[0] * 1e-3) / 1e9
        row = {"lights": len(lights), "ms": ms[0], "ms_min": ms[1], "launches_per_block": ms[2], "sdf_samples": int(st.SdfSamples), "pairs": int(st.PixelLightPairs),
               "traced_pairs": int(st.TracedPairs), "samples_per_traced_pair": int(st.SdfSamples) / max(int(st.TracedPairs), 1),
               "gsamples_per_s": rate, "rate_over_sphere_pass": rate / sphere["gsamples_per_s"]}
        frames.append({"frame": name, "target": [width, height], "field": {"virtual": [world, world, 128], "atlas": [layout.atlas_width, layout.atlas_height],
                                                                             "format": "unorm16" if fmt == abi.SDF_UNORM16 else "fp16"},
                       "sphere_lights": sphere, "projector_clear_only": clear, "projector_lights": row})
        target.close(); field.close()
    native.set_projector_texture(ctx, None)
    ctx.close()
    record = {"tool": "projector_time", "blocks": args.blocks, "block": args.block, "target_format": "half4", "texture": [256, 256], "frames": frames}
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
