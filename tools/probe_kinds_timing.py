"""Run ON THE GPU BOX.  What one probe call of each light kind costs end to end (the calls are synchronous: a host clock around each), in one
process, against ilm_render_light_probes with the same counts as the yardstick:

    ilm_render_directional_light_probes   256 probes x 4 shadowed lights on cfg3's field     vs the sphere entry, 256 x 4
    ilm_render_line_light_probes          256 probes x 64 lights on cfg3's field             vs the sphere entry, 256 x 64

The median of `reps` calls after warm-up, the entries alternating call by call so that what else the host is doing falls on both.

    python tools/probe_kinds_timing.py [reps] [output file]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from illuminant_amd import abi, native, scenes  # noqa: E402
from tools.strip_probe import build  # noqa: E402

PROBES = 256


def light_array(lights):
    arr = (abi.LightVertex * len(lights))()
    for i, l in enumerate(lights):
        arr[i] = l
    return arr


def medians(calls, reps):
    """{name: (median, min, max) in us} of calls = {name: function}, alternating"""
    for fn in calls.values():
        for _ in range(5):
            fn()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e6)
    return {name: (float(np.median(t)), float(np.min(t)), float(np.max(t))) for name, t in times.items()}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    ctx = native.Context(0)
    w, h, dfu, spheres, sdf = build(ctx, "cfg3")
    env = scenes.environment()
    pp = np.zeros((PROBES, 4), np.float32)
    pp[:, 3] = 1.0
    pp[:, 0] = scenes.uniform(5, (PROBES,), 0.0, w); pp[:, 1] = scenes.uniform(6, (PROBES,), 0.0, h); pp[:, 2] = scenes.uniform(7, (PROBES,), 0.0, 32.0)
    pn = np.zeros((PROBES, 4), np.float32)
    pn[:, 2] = 1.0; pn[:, 3] = 1.0                      # up, shadows enabled
    directions = ((0.55, 0.3, -0.6), (0.0, 0.0, -1.0), (-0.4, 0.5, -0.7), (0.3, -0.6, -0.5))
    directional = light_array([scenes.directional_light(direction=d, shadow_trace_length=256.0, shadow_softness=12.0) for d in directions])
    lines = light_array([scenes.line_light((spheres[i].LightPosition1.x, spheres[i].LightPosition1.y, spheres[i].LightPosition1.z),
                                           (spheres[(i + 1) % 64].LightPosition1.x, spheres[(i + 1) % 64].LightPosition1.y, 16.0),
                                           spheres[i].LightProperties.x, ramp_length=spheres[i].LightProperties.y) for i in range(64)])
    four = light_array([spheres[i] for i in range(4)])
    results = medians({
        "directional 256 x 4": lambda: native.render_directional_light_probes(ctx, directional, pp, pn, env, dfu, sdf),
        "sphere      256 x 4": lambda: native.render_light_probes(ctx, four, pp, pn, env, dfu, sdf),
        "line        256 x 64": lambda: native.render_line_light_probes(ctx, lines, pp, pn, env, dfu, sdf),
        "sphere      256 x 64": lambda: native.render_light_probes(ctx, spheres, pp, pn, env, dfu, sdf),
    }, reps)
    lit = native.render_directional_light_probes(ctx, directional, pp, pn, env, dfu, sdf)
    text = ["probe calls on cfg3's field (2048 x 2048 x 128, 32 slices), %d probes, median of %d calls each, alternating; us per call (min .. max)" % (PROBES, reps)]
    for name, (med, lo, hi) in results.items():
        text.append("  %-22s %8.1f   (%.1f .. %.1f)" % (name, med, lo, hi))
    flat = pn.copy()
    flat[:, 3] = 0.0                                   # enableShadows off: the same probes without the trace
    unshadowed = native.render_directional_light_probes(ctx, directional, pp, flat, env, dfu, sdf)
    text.append("  (directional probes: mean alpha %.2f, mean r %.4f; with enableShadows = 0 mean r %.4f: the timed call traces)"
                % (float(lit[:, 3].mean()), float(lit[:, 0].mean()), float(unshadowed[:, 0].mean())))
    print("\n".join(text))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
