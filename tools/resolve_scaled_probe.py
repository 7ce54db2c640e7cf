#!/usr/bin/env python3
"""What the scaled resolve costs beside the 1:1 resolve of the same back buffer (docs/experiments.md, "Scaled resolve").

Three calls, all writing a 3840 x 2160 RGBA8 target in the tone-mapping mode:
  scaled          ilm_resolve_lighting_scaled, 1920 x 1080 HALF4 lightmap, LINEAR, whole-target quad (RenderScale 0.5)
  scaled_albedo   the same over a 3840 x 2160 RGBA8 albedo, LINEAR
  one_to_one      ilm_resolve_lighting, 3840 x 2160 HALF4 lightmap: the kernel this work leaves untouched, the yardstick
Each call is timed in blocks of `--block` launches between two events on the context's stream (ilm_timer_*), the three calls alternating
block by block, `--blocks` blocks each: median and minimum ms per call.  Every variant rotates over `--sets` sets of textures so that the
bytes touched between two uses of a texture exceed the 256 MiB Infinity Cache (sets = 1: the cache-resident figure, reported beside it).
bytes = the unique bytes the call must move (source + albedo read once, destination written once), computed from the shapes; rate =
bytes / median time; hbm_fraction = rate / --hbm-peak (8 TB/s by specification).  A block's time is the stream's: where the host
enqueues more slowly than the device runs, it is the enqueue rate -- the kernel's own time is rocprofv3 --kernel-trace's, in a run of its
own.  Prints one JSON line; --out FILE also writes it there."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from illuminant_amd import abi, native  # noqa: E402

BYTES = {abi.LIGHTMAP_FLOAT4: 16, abi.LIGHTMAP_HALF4: 8, abi.LIGHTMAP_RGBA8: 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--block", type=int, default=32)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--no-resident", action="store_true", help="skip the sets = 1 pass (a kernel trace of the rotating pass alone)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--target", default="3840x2160")
    ap.add_argument("--hbm-peak", type=float, default=8.0e12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert native.device_count() > 0, "needs a GPU: there is no CPU path"
    tw, th = [int(v) for v in args.target.split("x")]
    sw, sh = tw // 2, th // 2
    ctx = native.Context(args.device)
    rng = np.random.default_rng(5)
    small = rng.uniform(0.0, 3.0, (sh, sw, 4)).astype(np.float16)
    big = np.tile(small, (2, 2, 1))[:th, :tw]
    color = rng.integers(0, 256, (th, tw, 4), dtype=np.uint8)
    hdr = abi.HDRConfiguration()
    hdr.Mode, hdr.InverseScaleFactor, hdr.Offset, hdr.Exposure, hdr.Gamma, hdr.WhitePoint = abi.HDR_TONE_MAP, 0.75, 0.02, 1.3, 0.9, 2.5

    def make(width, height, fmt, texels, count):
        out = []
        for _ in range(count):
            t = native.Lightmap(ctx, width, height, fmt)
            if texels is not None:
                t.upload(texels)
            out.append(t)
        return out

    records = {}
    for sets in sorted({args.sets} if args.no_resident else {args.sets, 1}, reverse=True):
        lightmaps, frames = make(sw, sh, abi.LIGHTMAP_HALF4, small, sets), make(tw, th, abi.LIGHTMAP_HALF4, big, sets)
        albedos, targets = make(tw, th, abi.LIGHTMAP_RGBA8, color, sets), make(tw, th, abi.LIGHTMAP_RGBA8, None, sets)
        quad = (0.0, 0.0, float(tw), float(th))
        calls = {
            "scaled": (lambda k: native.resolve_lighting_scaled(lightmaps[k], targets[k], hdr, quad),
                       sw * sh * BYTES[abi.LIGHTMAP_HALF4] + tw * th * BYTES[abi.LIGHTMAP_RGBA8]),
            "scaled_albedo": (lambda k: native.resolve_lighting_scaled(lightmaps[k], targets[k], hdr, quad, albedo=albedos[k]),
                              sw * sh * BYTES[abi.LIGHTMAP_HALF4] + 2 * tw * th * BYTES[abi.LIGHTMAP_RGBA8]),
            "one_to_one": (lambda k: native.resolve_lighting(frames[k], targets[k], hdr),
                           tw * th * (BYTES[abi.LIGHTMAP_HALF4] + BYTES[abi.LIGHTMAP_RGBA8])),
        }
        times = {name: [] for name in calls}
        for name, (call, _) in calls.items():            # warm-up: every shape and every texture once
            for k in range(sets):
                call(k)
        ctx.sync()
        n = 0
        for _ in range(args.blocks):
            for name, (call, _) in calls.items():
                ctx.timer_start()
                for _ in range(args.block):
                    call(n % sets)
                    n += 1
                times[name].append(ctx.timer_stop() / args.block)
        rows = {}
        for name, (_, moved) in calls.items():
            ms = statistics.median(times[name])
            rows[name] = {"ms": ms, "ms_min": min(times[name]), "bytes": moved, "bytes_per_s": moved / (ms * 1e-3),
                          "hbm_fraction": moved / (ms * 1e-3) / args.hbm_peak}
        for name in rows:
            rows[name]["over_one_to_one"] = rows[name]["ms"] / rows["one_to_one"]["ms"]
        records["sets_%d" % sets] = rows
        for t in lightmaps + frames + albedos + targets:
            t.close()
    ctx.close()
    line = json.dumps({"tool": "resolve_scaled_probe", "target": [tw, th], "lightmap": [sw, sh], "mode": "tone_map", "filter": "linear",
                       "blocks": args.blocks, "block": args.block, "hbm_peak": args.hbm_peak, "results": records})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
