#!/usr/bin/env python3
"""What a frame of line lights costs on the device (docs/experiments.md, "Line lights").

The two frames of tools/directional_time.py -- no G-buffer, HalfVector4 target, cfg3's quality settings (MinStepSize 1, LongStepFactor 0.5,
MaxStepCount 64, MaxConeRadius 24, OcclusionToOpacityPower 0.7):
  cfg3   1920 x 1080 over cfg3's field (2048 x 2048 x 128 units at 1/4 texel per unit, unorm16, 256 random obstructions)
  cfg5   3840 x 2160 over cfg5's field (4096 x 4096 x 128 units at 1/8 texel per unit, fp16, the same obstructions' generator)
each lit by four shadow-casting line lights (segments of a third to a half of the frame's width at z = 48 .. 96, radius 6), by the same
four without shadows (the opacity term alone), and, in the same run, by four directional lights (directional_time.py's) as the yardstick:
  ms            one call (record preparation + the pass), HIP events around a block of queued calls: median and minimum over `--blocks`
                blocks after a warm-up block, each block at least `--block` calls and enough of them to fill ~0.1 s of device time
  samples       the call's own sampleDistanceFieldEx count, from the counting instantiation, run separately from the timed launches
  gsamples_per_s, and the line pass's sample rate over the directional pass's of the same field: the comparison to report
Prints one JSON line; --out FILE also writes it there.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from illuminant_amd import abi, native, scenes  # noqa: E402
from directional_time import DIRECTIONS, light_array, median_ms  # noqa: E402

# (start, end) as fractions of the frame's width / height, z
SEGMENTS = (((0.10, 0.20, 64.0), (0.55, 0.30, 48.0)), ((0.60, 0.15, 96.0), (0.90, 0.70, 64.0)), ((0.20, 0.80, 48.0), (0.70, 0.90, 80.0)),
            ((0.45, 0.40, 72.0), (0.45, 0.75, 72.0)))


def line_lights(width, height, casts_shadows):
    return light_array([scenes.line_light((a[0] * width, a[1] * height, a[2]), (b[0] * width, b[1] * height, b[2]), 6.0, start_color=(1.0, 0.9, 0.8, 1.0),
                                          end_color=(0.6, 0.8, 1.0, 1.0), casts_shadows=casts_shadows) for a, b in SEGMENTS])


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
    frames = []

    def timed(call, lights):
        st = call(ctx, lights, env, dfu, None, field, ambient, target, want_stats=True)
        ms = median_ms(ctx, args.blocks, args.block, lambda: call(ctx, lights, env, dfu, None, field, ambient, target))
        return {"lights": len(lights), "ms": ms[0], "ms_min": ms[1], "launches_per_block": ms[2], "sdf_samples": int(st.SdfSamples),
                "pairs": int(st.PixelLightPairs), "traced_pairs": int(st.TracedPairs),
                "samples_per_traced_pair": int(st.SdfSamples) / max(int(st.TracedPairs), 1), "gsamples_per_s": int(st.SdfSamples) / (ms[0] * 1e-3) / 1e9}

    for name, width, height, world, resolution, fmt in (("cfg3", 1920, 1080, 2048, 0.25, abi.SDF_UNORM16), ("cfg5", 3840, 2160, 4096, 0.125, abi.SDF_FP16)):
        layout = scenes.DistanceFieldLayout(world, world, 128.0, 32, resolution, 128)
        obstacles = [(typ - 1, center, size) for (typ, center, size) in scenes.random_obstacles(11, 256, (world, world))]
        field = native.DistanceFieldTexture(ctx, None, fmt, size=(layout.atlas_width, layout.atlas_height))
        field.render_slices(scenes.render_desc(layout), list(range(0, layout.slice_count, 3)), scenes.obstruction_array(obstacles))
        dfu = layout.uniforms(power=0.7, min_step_size=1.0, long_step_factor=0.5)
        target = native.Lightmap(ctx, width, height, abi.LIGHTMAP_HALF4)
        directional = timed(native.render_directional_lights,
                            light_array([scenes.directional_light(direction=DIRECTIONS[i], color=(1.0, 0.9, 0.8, 1.0)) for i in range(4)]))
        shadowed = timed(native.render_line_lights, line_lights(width, height, True))
        shadowed["rate_over_directional_pass"] = shadowed["gsamples_per_s"] / directional["gsamples_per_s"]
        unshadowed = timed(native.render_line_lights, line_lights(width, height, False))
        frames.append({"frame": name, "target": [width, height], "field": {"virtual": [world, world, 128], "atlas": [layout.atlas_width, layout.atlas_height],
                                                                             "format": "unorm16" if fmt == abi.SDF_UNORM16 else "fp16"},
                       "directional_lights": directional, "line_lights": shadowed, "line_lights_without_shadows": unshadowed})
        target.close(); field.close()
    ctx.close()
    record = {"tool": "line_time", "blocks": args.blocks, "block": args.block, "target_format": "half4", "frames": frames}
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
