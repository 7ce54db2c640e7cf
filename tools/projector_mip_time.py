#!/usr/bin/env python3
"""What the mip chain costs the projector pass (docs/experiments.md, "Projector lights: mip chains").

tools/projector_time.py's two frames and four shadowed lights (cfg3: 1920 x 1080 over the unorm16 field; cfg5: 3840 x 2160 over the fp16
field; HalfVector4 target, no G-buffer), timed in ONE run as
  one_level       the 256 x 256 texture bound with ilm_ctx_set_projector_texture: projector_lights_kernel, the kernel the pass had
                  before there were chains (timed first and again last: the two medians bracket the run's own drift)
  chain_lod_0     the same lights over the texture's 9-level box-filter chain (ilm_ctx_set_projector_texture_mips) at LOD 0: the MIPS
                  kernel with one level read (weight 0: the scalar branch skips level 1)
  chain_lod_067   the same chain at LOD 0.67, a light drawn at half size: two levels, eight taps, one more lerp
each as tools/projector_time.py measures a call (record preparation + the pass, HIP events around blocks of queued calls, median and
minimum over `--blocks` blocks after a warm-up block), with the ratios to one_level.  The images of one_level and chain_lod_0 must be
the same bits (level 0 is the same texture); the tool asserts it.
Prints one JSON line; --out FILE also writes it there.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from illuminant_amd import abi, native, scenes  # noqa: E402
from projector_time import light_array, median_ms, projector_lights  # noqa: E402


def with_lod(lights, lod):
    out = []
    for l in lights:
        v = abi.LightVertex.from_buffer_copy(bytes(l))
        v.Color2.w = lod
        out.append(v)
    return light_array(out)


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
    chain = scenes.projector_mip_chain(texture)
    assert len(chain) == 9
    frames = []
    for name, width, height, world, resolution, fmt in (("cfg3", 1920, 1080, 2048, 0.25, abi.SDF_UNORM16), ("cfg5", 3840, 2160, 4096, 0.125, abi.SDF_FP16)):
        layout = scenes.DistanceFieldLayout(world, world, 128.0, 32, resolution, 128)
        obstacles = [(typ - 1, center, size) for (typ, center, size) in scenes.random_obstacles(11, 256, (world, world))]
        field = native.DistanceFieldTexture(ctx, None, fmt, size=(layout.atlas_width, layout.atlas_height))
        field.render_slices(scenes.render_desc(layout), list(range(0, layout.slice_count, 3)), scenes.obstruction_array(obstacles))
        dfu = layout.uniforms(power=0.7, min_step_size=1.0, long_step_factor=0.5)
        target = native.Lightmap(ctx, width, height, abi.LIGHTMAP_HALF4)
        base = projector_lights(width, height)
        rows, images = {}, {}
        for row, bound, lod in (("one_level", texture, 0.0), ("chain_lod_0", chain, 0.0), ("chain_lod_067", chain, 0.67), ("one_level_again", texture, 0.0)):
            native.set_projector_texture(ctx, bound)
            lights = with_lod(base, lod)
            st = native.render_projector_lights(ctx, lights, env, dfu, None, field, ambient, target, want_stats=True)
            images[row] = target.download()
            ms = median_ms(ctx, args.blocks, args.block, lambda: native.render_projector_lights(ctx, lights, env, dfu, None, field, ambient, target))
            rows[row] = {"levels": len(bound) if isinstance(bound, list) else 1, "lod": lod, "ms": ms[0], "ms_min": ms[1], "launches_per_block": ms[2],
                         "sdf_samples": int(st.SdfSamples), "pairs": int(st.PixelLightPairs), "traced_pairs": int(st.TracedPairs)}
        assert np.array_equal(images["one_level"].view(np.uint16), images["chain_lod_0"].view(np.uint16)), "LOD 0 of the chain is the one-level texture"
        assert np.array_equal(images["one_level"].view(np.uint16), images["one_level_again"].view(np.uint16))
        assert not np.array_equal(images["one_level"].view(np.uint16), images["chain_lod_067"].view(np.uint16))
        a = rows["one_level"]["ms"]
        for row in ("chain_lod_0", "chain_lod_067", "one_level_again"):
            rows[row]["ms_over_one_level"] = rows[row]["ms"] / a
        frames.append({"frame": name, "target": [width, height], "field": {"virtual": [world, world, 128], "atlas": [layout.atlas_width, layout.atlas_height],
                                                                             "format": "unorm16" if fmt == abi.SDF_UNORM16 else "fp16"}, **rows})
        target.close(); field.close()
    native.set_projector_texture(ctx, None)
    ctx.close()
    record = {"tool": "projector_mip_time", "blocks": args.blocks, "block": args.block, "target_format": "half4", "texture": [256, 256], "levels": len(chain),
              "frames": frames}
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
