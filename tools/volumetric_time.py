#!/usr/bin/env python3
"""What a frame of volumetric lights costs on the device (docs/experiments.md, "Volumetric lights").

The two frames of tools/directional_time.py -- no G-buffer, HalfVector4 target, cfg3's quality settings but for the step budget
(MinStepSize 1, LongStepFactor 0.5, MaxConeRadius 24, OcclusionToOpacityPower 0.7):
  cfg3   1920 x 1080 over cfg3's field (2048 x 2048 x 128 units at 1/4 texel per unit, unorm16, 256 random obstructions)
  cfg5   3840 x 2160 over cfg5's field (4096 x 4096 x 128 units at 1/8 texel per unit, fp16, the same obstructions' generator)
each lit by three shadow-casting volumetric lights -- a cone that projects from its start, an ellipsoid lit along a direction and a box,
each over about a ninth of the frame -- at MaxStepCount 16 and 64 (a pair walks MaxStepCount + 1 column points of up to MaxStepCount
samples each), by the same three without shadows (the column and the contact term alone), and, in the same run, by four directional
lights at MaxStepCount 64 (directional_time.py's) as the yardstick:
  ms            one call (record preparation + the pass), HIP events around a block of queued calls: median and minimum over `--blocks`
                blocks after a warm-up block, each block at least `--block` calls and enough of them to fill ~0.1 s of device time
  samples       the call's own sampleDistanceFieldEx count, from the counting instantiation, run separately from the timed launches
  gsamples_per_s, and the volumetric pass's sample rate over the directional pass's of the same field: the comparison to report
  ns_per_column_point for the lights without shadows: what one evaluation of the shape with its pow costs
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


def volumetric_lights(width, height, casts_shadows):
    w, h = float(width), float(height)
    common = dict(casts_shadows=casts_shadows, ramp_length=24.0, volumetricity=0.5, color=(1.0, 0.9, 0.8, 1.0))
    return light_array([
        scenes.volumetric_light(shape=scenes.VOLUMETRIC_CONE, start=(0.12 * w, 0.15 * h, 110.0), end=(0.30 * w, 0.40 * h, 8.0), start_radius=0.02 * w,
                                end_radius=0.08 * w, **common),
        scenes.volumetric_light(shape=scenes.VOLUMETRIC_ELLIPSOID, start=(0.45 * w, 0.10 * h, -20.0), end=(0.78 * w, 0.43 * h, 100.0),
                                direction=(0.3, 0.2, -0.9), **common),
        scenes.volumetric_light(shape=scenes.VOLUMETRIC_BOX, start=(0.20 * w, 0.55 * h, 0.0), end=(0.53 * w, 0.88 * h, 90.0), **common)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frames", default="cfg3,cfg5")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert native.device_count() > 0, "needs a GPU: there is no CPU path"
    assert args.blocks * args.block >= 20, "at least 20 timed launches"
    ctx = native.Context(args.device)
    env = scenes.environment()
    ambient = (0.05, 0.05, 0.05, 1.0)
    frames = []

    def timed(call, lights, dfu):
        st = call(ctx, lights, env, dfu, None, field, ambient, target, want_stats=True)
        ms = median_ms(ctx, args.blocks, args.block, lambda: call(ctx, lights, env, dfu, None, field, ambient, target))
        return {"lights": len(lights), "max_step_count": float(dfu.StepAndMisc2.x), "ms": ms[0], "ms_min": ms[1], "launches_per_block": ms[2],
                "sdf_samples": int(st.SdfSamples), "pairs": int(st.PixelLightPairs), "traced_pairs": int(st.TracedPairs),
                "samples_per_traced_pair": int(st.SdfSamples) / max(int(st.TracedPairs), 1), "gsamples_per_s": int(st.SdfSamples) / (ms[0] * 1e-3) / 1e9}

    for name, width, height, world, resolution, fmt in (("cfg3", 1920, 1080, 2048, 0.25, abi.SDF_UNORM16), ("cfg5", 3840, 2160, 4096, 0.125, abi.SDF_FP16)):
        if name not in args.frames.split(","):
            continue
        layout = scenes.DistanceFieldLayout(world, world, 128.0, 32, resolution, 128)
        obstacles = [(typ - 1, center, size) for (typ, center, size) in scenes.random_obstacles(11, 256, (world, world))]
        field = native.DistanceFieldTexture(ctx, None, fmt, size=(layout.atlas_width, layout.atlas_height))
        field.render_slices(scenes.render_desc(layout), list(range(0, layout.slice_count, 3)), scenes.obstruction_array(obstacles))
        target = native.Lightmap(ctx, width, height, abi.LIGHTMAP_HALF4)
        record = {"frame": name, "target": [width, height], "field": {"virtual": [world, world, 128], "atlas": [layout.atlas_width, layout.atlas_height],
                                                                       "format": "unorm16" if fmt == abi.SDF_UNORM16 else "fp16"}}
        dfu64 = layout.uniforms(power=0.7, min_step_size=1.0, long_step_factor=0.5)
        directional = timed(native.render_directional_lights,
                            light_array([scenes.directional_light(direction=DIRECTIONS[i], color=(1.0, 0.9, 0.8, 1.0)) for i in range(4)]), dfu64)
        record["directional_lights"] = directional
        for steps in (16, 64):
            dfu = layout.uniforms(power=0.7, min_step_size=1.0, long_step_factor=0.5, step_limit=steps)
            shadowed = timed(native.render_volumetric_lights, volumetric_lights(width, height, True), dfu)
            shadowed["rate_over_directional_pass"] = shadowed["gsamples_per_s"] / directional["gsamples_per_s"]
            unshadowed = timed(native.render_volumetric_lights, volumetric_lights(width, height, False), dfu)
            unshadowed["ns_per_column_point"] = unshadowed["ms"] * 1e6 / (unshadowed["pairs"] * (steps + 1))
            record["volumetric_lights_%d" % steps] = shadowed
            record["volumetric_lights_without_shadows_%d" % steps] = unshadowed
        frames.append(record)
        target.close(); field.close()
    ctx.close()
    record = {"tool": "volumetric_time", "blocks": args.blocks, "block": args.block, "target_format": "half4", "frames": frames}
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
