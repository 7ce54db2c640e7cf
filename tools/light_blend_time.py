#!/usr/bin/env python3
"""What a non-additive light group costs beside the additive one (docs/experiments.md, "Light blend functions").

The frames of tools/directional_time.py -- no G-buffer, HalfVector4 target, cfg3's quality settings:
  cfg3   1920 x 1080 over cfg3's field (unorm16), 64 sphere lights (bench.py's seed)
  cfg5   3840 x 2160 over cfg5's field (fp16), 256 sphere lights
each lit by its sphere lights, by directional_time.py's four directional lights and by line_time.py's four shadowed line lights, every
group ACCUMULATED onto a frame the sphere lights rendered before (ambient NULL: the base is the texel, the form a darkening group
takes), under each blend function in turn: ADD, REVERSE_SUBTRACT, MAX, MIN for colour and alpha alike (ilm_ctx_set_light_blend_function).
Per row: ms per call (median and minimum over `--blocks` blocks, as the other tools time), the ratio to the ADD row of the same group,
and the launch's workgroups (ilm_debug_last_light_launch) -- a non-additive sphere launch is served by one workgroup per tile, the
full-frame passes launch what ADD launches.  ADD is timed first and again last (add_again): the distance between the two is the run's
own spread.  Prints one JSON line; --out FILE also writes it there.
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
from line_time import line_lights  # noqa: E402

FUNCTIONS = (("add", abi.LIGHT_BLEND_ADD), ("reverse_subtract", abi.LIGHT_BLEND_REVERSE_SUBTRACT), ("max", abi.LIGHT_BLEND_MAX),
             ("min", abi.LIGHT_BLEND_MIN), ("add_again", abi.LIGHT_BLEND_ADD))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=5)
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
    for name, width, height, world, resolution, fmt, n_sphere, seed in (("cfg3", 1920, 1080, 2048, 0.25, abi.SDF_UNORM16, 64, 12),
                                                                         ("cfg5", 3840, 2160, 4096, 0.125, abi.SDF_FP16, 256, 13)):
        if name not in args.frames.split(","):
            continue
        layout = scenes.DistanceFieldLayout(world, world, 128.0, 32, resolution, 128)
        obstacles = [(typ - 1, center, size) for (typ, center, size) in scenes.random_obstacles(11, 256, (world, world))]
        field = native.DistanceFieldTexture(ctx, None, fmt, size=(layout.atlas_width, layout.atlas_height))
        field.render_slices(scenes.render_desc(layout), list(range(0, layout.slice_count, 3)), scenes.obstruction_array(obstacles))
        dfu = layout.uniforms(power=0.7, min_step_size=1.0, long_step_factor=0.5)
        target = native.Lightmap(ctx, width, height, abi.LIGHTMAP_HALF4)
        sc = width / 1920.0
        spheres = scenes.random_lights(seed, n_sphere, width, height, z=(8.0, 64.0), radius=24.0, ramp=(200.0 * sc, 550.0 * sc))
        spheres = (abi.LightVertex * len(spheres))(*spheres)
        groups = (("sphere_lights", native.render_sphere_lights, spheres),
                  ("directional_lights", native.render_directional_lights,
                   light_array([scenes.directional_light(direction=DIRECTIONS[i], color=(1.0, 0.9, 0.8, 1.0)) for i in range(4)])),
                  ("line_lights", native.render_line_lights, line_lights(width, height, True)))
        record = {"frame": name, "target": [width, height], "field_format": "unorm16" if fmt == abi.SDF_UNORM16 else "fp16"}
        for group, call, lights in groups:
            rows = {}
            for label, function in FUNCTIONS:
                # the base every row starts from: the frame's sphere lights, additively (a subtraction onto a growing or shrinking
                # texel would time other values, not another function)
                ctx.set_light_blend_function()
                native.render_sphere_lights(ctx, spheres, env, dfu, None, field, ambient, target)
                ctx.set_light_blend_function(function, function)
                ms = median_ms(ctx, args.blocks, args.block, lambda: call(ctx, lights, env, dfu, None, field, None, target))
                rows[label] = {"ms": ms[0], "ms_min": ms[1], "launches_per_block": ms[2], "workgroups": ctx.last_light_launch()[0],
                               "split": ctx.last_light_launch()[1]}
            ctx.set_light_blend_function()
            for label in rows:
                rows[label]["over_add"] = rows[label]["ms"] / rows["add"]["ms"]
            record[group] = {"lights": len(lights), "functions": rows}
        frames.append(record)
        target.close(); field.close()
    ctx.close()
    line = json.dumps({"tool": "light_blend_time", "blocks": args.blocks, "block": args.block, "target_format": "half4", "accumulate": True,
                       "frames": frames})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
