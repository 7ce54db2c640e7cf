"""Run ON THE GPU BOX: what the distance field's fixed-point filter (ilm_sdf_set_filter, ILM_SDF_FILTER_FIXED8) does to a frame.
    python tools/sdf_filter_report.py [--frames 7] [--scenes cfg3,cfg5]

For cfg3 and cfg5 (tools/strip_probe.build: the bench's lit frames) the frame is rendered once with the filter at 0 and once at 8, both
into a float4 lightmap with the counting variant, and compared: over the rgb of all pixels the maximum and the 99.9th percentile of
|on - off| / |off|, the share of pixels beyond the suite's criterion (tests.util.assert_close: 1e-4 relative + 1e-5 of the component's
scale), SdfSamples and TracedPairs of both modes and their differences, and the median frame time of each mode over a handful of plain
launches.  FIXED8 is a MODEL of a hardware sampler nobody here can run (the header states it and its defined deviation), not the
reference's measured behaviour: these are findings, not thresholds.  Not run by any test; the output is committed under profiles/."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from illuminant_amd import abi, native, scenes  # noqa: E402
from tools.strip_probe import build  # noqa: E402

RTOL, ATOL = 1e-4, 1e-5       # tests/util.py: the suite's criterion for a lightmap


def median_ms(ctx, fn, frames):
    fn(); fn()
    ctx.sync()
    times = []
    for _ in range(frames):
        ctx.timer_start()
        fn()
        times.append(ctx.timer_stop())
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--scenes", default="cfg3,cfg5")
    args = ap.parse_args()
    ctx = native.Context(0)
    env = scenes.environment()
    ambient = (0.05, 0.05, 0.05, 1.0)
    print("# ilm_sdf_set_filter: ILM_SDF_FILTER_FIXED8 (on) against ILM_SDF_FILTER_FP32 (off), ilm_render_sphere_lights, float4 lightmap, counting variant")
    print("# FIXED8 is a model of a hardware sampler (8 fraction bits, round half to even, no carry into the next texel), not the reference's measured behaviour")
    for name in args.scenes.split(","):
        w, h, dfu, lights, sdf = build(ctx, name)
        lm = native.Lightmap(ctx, w, h, abi.LIGHTMAP_FLOAT4)
        frames, stats = {}, {}
        for bits in (abi.SDF_FILTER_FP32, abi.SDF_FILTER_FIXED8):
            sdf.set_filter(bits)
            s = native.render_sphere_lights(ctx, lights, env, dfu, None, sdf, ambient, lm, want_stats=True)
            frames[bits], stats[bits] = lm.download(), (s.SdfSamples, s.PixelLightPairs, s.TracedPairs)
        off, on = frames[0][..., :3].astype(np.float64), frames[8][..., :3].astype(np.float64)
        rel = np.abs(on - off) / np.maximum(np.abs(off), 1e-30)
        scale = np.abs(off).reshape(-1, 3).max(axis=0)
        beyond = (np.abs(on - off) > RTOL * np.abs(off) + ATOL * scale).any(axis=-1)
        print("%s: %d x %d, %d lights, field format %s" % (name, w, h, len(lights), "fp16" if sdf.format == abi.SDF_FP16 else "unorm16"))
        print("  rgb |on - off| / |off|: max %.4g, 99.9th percentile %.4g, median %.4g" % (rel.max(), np.percentile(rel, 99.9), np.median(rel)))
        print("  pixels beyond the suite's criterion (1e-4 relative + 1e-5 of the component's scale): %d of %d = %.3f %%" % (
            int(beyond.sum()), beyond.size, 100.0 * beyond.mean()))
        print("  alpha (contributing lights per pixel) equal: %s" % bool(np.array_equal(frames[0][..., 3], frames[8][..., 3])))
        print("  SdfSamples off %d, on %d, on - off %+d (%+.4f %%)" % (stats[0][0], stats[8][0], stats[8][0] - stats[0][0],
                                                                   100.0 * (stats[8][0] - stats[0][0]) / max(stats[0][0], 1)))
        print("  TracedPairs off %d, on %d, on - off %+d;  PixelLightPairs off %d, on %d" % (stats[0][2], stats[8][2], stats[8][2] - stats[0][2],
                                                                                          stats[0][1], stats[8][1]))
        # plain launches: the default path as planned (light split chosen per launch), the default path with one workgroup per tile --
        # what a FIXED8 launch is served by -- and FIXED8
        plain = lambda: native.render_sphere_lights(ctx, lights, env, dfu, None, sdf, ambient, lm)
        sdf.set_filter(abi.SDF_FILTER_FP32)
        ctx.set_light_split(0)
        t_off = median_ms(ctx, plain, args.frames)
        ctx.set_light_split(1)
        t_off1 = median_ms(ctx, plain, args.frames)
        ctx.set_light_split(0)
        sdf.set_filter(abi.SDF_FILTER_FIXED8)
        t_on = median_ms(ctx, plain, args.frames)
        print("  median ms per frame over %d plain launches: off %.4f (split chosen per launch), off %.4f (one workgroup per tile), on %.4f (%+.1f %% on the latter)" % (
            args.frames, t_off, t_off1, t_on, 100.0 * (t_on - t_off1) / t_off1))
        info = sdf.trace_info()
        print("  cell array: %d bytes, rebuilt %d time(s) over all of the above" % (info.CellBytes, info.CellRebuilds))
        sdf.set_filter(abi.SDF_FILTER_FP32)
        lm.close(); sdf.close()
    ctx.close()


if __name__ == "__main__":
    main()
