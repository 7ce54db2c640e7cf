#!/usr/bin/env python3
"""What the LUT-blended resolve costs beside the with-albedo scaled resolve of the same textures (docs/experiments.md, "LUT-blended resolve").

Two calls, both resolving a 1920 x 1080 HALF4 lightmap onto a 3840 x 2160 RGBA8 target over a 3840 x 2160 RGBA8 albedo, LINEAR, HDR mode
None (the only mode the LUT technique has), whole-target quad:
  lut             ilm_resolve_lighting_lut with two 17^3 RGBA8 LUTs (289 x 17 texels each), a neutral band, LUTOnly off
  scaled_albedo   ilm_resolve_lighting_scaled: the kernel this work leaves untouched, the yardstick
`--tone-map` adds scaled_albedo_tone_map, the call tools/resolve_scaled_probe.py times (the mode the earlier record was taken in).
Each call is timed in blocks of `--block` launches between two events on the context's stream (ilm_timer_*), the calls alternating block by
block, `--blocks` blocks each: median and minimum ms per call.  Every call rotates over `--sets` sets of lightmap, albedo and target so that
the bytes touched between two uses of a texture exceed the 256 MiB Infinity Cache (sets = 1: the cache-resident figure, reported beside
it); the two LUTs are one pair throughout, as in a frame.  bytes = the unique bytes the call must move.  A block's time is the stream's:
where the host enqueues more slowly than the device runs it is the enqueue rate -- the kernel's own time is rocprofv3 --kernel-trace's, in a
run of its own.  Prints one JSON line; --out FILE also writes it there."""
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
N = 17


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--block", type=int, default=32)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--no-resident", action="store_true", help="skip the sets = 1 pass (a kernel trace of the rotating pass alone)")
    ap.add_argument("--tone-map", action="store_true", help="also time the scaled resolve in the tone-mapping mode")
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
    small = rng.uniform(0.0, 1.5, (sh, sw, 4)).astype(np.float16)
    color = rng.integers(0, 256, (th, tw, 4), dtype=np.uint8)
    hdr = abi.HDRConfiguration()
    hdr.Mode, hdr.InverseScaleFactor, hdr.Offset, hdr.Exposure, hdr.Gamma, hdr.WhitePoint = abi.HDR_NONE, 0.75, 0.02, 1.3, 0.9, 2.5
    tone = abi.HDRConfiguration()
    tone.Mode, tone.InverseScaleFactor, tone.Offset, tone.Exposure, tone.Gamma, tone.WhitePoint = abi.HDR_TONE_MAP, 0.75, 0.02, 1.3, 0.9, 2.5
    luts = []
    for _ in range(2):
        t = native.Lightmap(ctx, N * N, N, abi.LIGHTMAP_RGBA8)
        t.upload(rng.integers(0, 256, (N, N * N, 4), dtype=np.uint8))
        luts.append(t)
    blending = native.lut_blending(luts[0], luts[1], 0.25, 0.75, 0.25)

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
        lightmaps = make(sw, sh, abi.LIGHTMAP_HALF4, small, sets)
        albedos, targets = make(tw, th, abi.LIGHTMAP_RGBA8, color, sets), make(tw, th, abi.LIGHTMAP_RGBA8, None, sets)
        quad = (0.0, 0.0, float(tw), float(th))
        moved = sw * sh * BYTES[abi.LIGHTMAP_HALF4] + 2 * tw * th * BYTES[abi.LIGHTMAP_RGBA8]
        calls = {
            "lut": (lambda k: native.resolve_lighting_lut(lightmaps[k], targets[k], hdr, blending, quad, albedos[k]), moved + 2 * N * N * N * 4),
            "scaled_albedo": (lambda k: native.resolve_lighting_scaled(lightmaps[k], targets[k], hdr, quad, albedo=albedos[k]), moved),
        }
        if args.tone_map:
            calls["scaled_albedo_tone_map"] = (lambda k: native.resolve_lighting_scaled(lightmaps[k], targets[k], tone, quad, albedo=albedos[k]), moved)
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
        for name, (_, nbytes) in calls.items():
            ms = statistics.median(times[name])
            rows[name] = {"ms": ms, "ms_min": min(times[name]), "ms_max": max(times[name]), "bytes": nbytes, "bytes_per_s": nbytes / (ms * 1e-3),
                          "hbm_fraction": nbytes / (ms * 1e-3) / args.hbm_peak}
        for name in rows:
            rows[name]["over_scaled_albedo"] = rows[name]["ms"] / rows["scaled_albedo"]["ms"]
        records["sets_%d" % sets] = rows
        for t in lightmaps + albedos + targets:
            t.close()
    for t in luts:
        t.close()
    ctx.close()
    line = json.dumps({"tool": "resolve_lut_probe", "library": os.path.basename(native.LIB_PATH), "target": [tw, th], "lightmap": [sw, sh],
                       "lut": [N, "rgba8"], "mode": "none", "filter": "linear", "blocks": args.blocks, "block": args.block,
                       "hbm_peak": args.hbm_peak, "results": records})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
