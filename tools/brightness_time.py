#!/usr/bin/env python3
"""What brightness estimation costs on the device (docs/experiments.md, "Brightness estimation").

For a 3840 x 2160 and a 1920 x 1080 HalfVector4 lit frame, at level 3 (the reference's default accuracyFactor) and level 0:
  luminance   the luminance pass alone (ilm_debug_queue_luminance), HIP events around `block` queued passes
  histogram   the whole ilm_lightmap_histogram call -- luminance pass, statistics, select, the pinned block's hand-over and the call's
              synchronisation -- HIP events around `block` calls
  download    ilm_lightmap_download of the same lightmap: what a caller without these entry points does before it can reduce anything
and the luminance pass's bytes touched (the odd rows: half of the lightmap) over its time beside the copy rate csrc/calib.hip reaches in
the same run.  Times are the median over `--blocks` blocks after a warm-up block; HIP events through ilm_timer_*.
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


def histogram_table(max_value=4.0, power=2.0, count=64):
    """Histogram's ctor table (Illuminant/Histogram.cs:69-75)."""
    import math
    log = math.log(float(np.float32(1) + np.float32(max_value))) / math.log(power)
    return np.array([np.float32(math.pow(power, (log / count) * (i + 1))) - np.float32(1) for i in range(count)], np.float32)


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


def copy_rate_gb_per_s(device):
    path = os.path.join(ROOT, "illuminant_amd", "lib", "libilluminant_calib.so")
    cl = C.CDLL(path)
    cl.ilm_calib_copy_rates.argtypes = [C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    cl.ilm_calib_copy_rates.restype = C.c_int
    rates = (C.c_double * 3)()
    rc = cl.ilm_calib_copy_rates(device, C.c_size_t(1 << 30), 6, rates)
    if rc != 0:
        raise RuntimeError("ilm_calib_copy_rates failed: hipError %d" % rc)
    return max(rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert native.device_count() > 0, "needs a GPU: there is no CPU path"
    ctx = native.Context(args.device)
    lib = native.lib()
    table = histogram_table()
    rows = []
    for width, height in ((3840, 2160), (1920, 1080)):
        lm = native.Lightmap(ctx, width, height, abi.LIGHTMAP_HALF4)
        lights = scenes.random_lights(width + height, 64, width, height, z=(8.0, 64.0), radius=height / 20.0, ramp=(height / 8.0, height / 2.0))
        lights = (abi.LightVertex * len(lights))(*lights)
        dfu = scenes.DistanceFieldLayout(64, 64, 32.0, 3, 1.0, 64).uniforms()
        native.render_sphere_lights(ctx, lights, scenes.environment(), dfu, None, None, (0.03, 0.05, 0.04, 1.0), lm)
        host = np.empty((height, width, 4), np.float16)
        download = median_ms(ctx, args.blocks, max(args.block // 4, 1), lambda: native.check(lib.ilm_lightmap_download(lm.handle, host.ctypes.data_as(C.c_void_p), 0, height)))
        for level in (3, 0):
            lum = median_ms(ctx, args.blocks, args.block, lambda: native.check(lib.ilm_debug_queue_luminance(lm.handle, width, height, level)))
            result = [None]

            def whole():
                result[0] = lm.histogram(table, level, 1.0, False)
            hist = median_ms(ctx, args.blocks, args.block, whole)
            touched = (height // 2) * width * 8
            rows.append({"width": width, "height": height, "level": level, "values": result[0][0].Width * result[0][0].Height,
                         "luminance_ms": lum[0], "luminance_ms_min": lum[1], "histogram_call_ms": hist[0], "histogram_call_ms_min": hist[1],
                         "download_ms": download[0], "download_ms_min": download[1],
                         "luminance_bytes_touched": touched, "luminance_gb_per_s": touched / (lum[0] * 1e-3) / 1e9,
                         "median": result[0][0].Median, "mean": result[0][0].Mean, "sample_count": result[0][0].SampleCount})
        lm.close()
    ctx.sync()
    record = {"tool": "brightness_time", "blocks": args.blocks, "block": args.block, "copy_rate_gb_per_s": copy_rate_gb_per_s(args.device), "rows": rows}
    ctx.close()
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
