#!/usr/bin/env python3
"""GPU box: what the waves of step_lean_clamp_kernel do about the category plane on bench.py's headline (cfg4 whole: 64 chunks of 1024^2,
Gravity x4 + Noise + UpdatePositions), read from ilm_debug_step_category_waves, and the chunks' category records afterwards
(ilm_debug_chunk_category_bounds).

    python tools/step_category_share.py [steps]

The system is built by bench.build_particle_system as the headline's row builds it.  Two untimed steps first (the first step of a system
stores everything through the general instantiation; the second is the class's first and scans every chunk), then `steps` (default 10)
counted ones."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from illuminant_amd import abi, native, scenes  # noqa: E402
from illuminant_amd import _host as H  # noqa: E402


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    ctx = H.DeviceContext(0)
    F = bench.build_particle_system(H, ctx, scenes, abi, 1024, 64, 0, with_spawner=False, replicate_cfg4_images=True)
    ps, tp = F["ps"], F["tp"]
    lib, handle = native.lib(), C.c_uint64(ctx.Handle)
    skipped, late, upfront = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    try:
        for frame in range(2 + steps):
            if frame == 2:
                native.check(lib.ilm_debug_step_category_waves(handle, 1, None, None, None))
            tp.Advance(1.0 / 60.0); ps.Update(frame)
        ctx.Sync()
    finally:
        native.check(lib.ilm_debug_step_category_waves(handle, 0, C.byref(skipped), C.byref(late), C.byref(upfront)))
    waves = steps * F["live"] // 64
    print("steps 3..%d of the headline: %d waves; category plane never loaded %d (%.4f %%), loaded late %d, loaded up front %d; last kernel %d"
          % (2 + steps, waves, skipped.value, 100.0 * skipped.value / waves, late.value, upfront.value, lib.ilm_debug_last_step_kernel()))
    records = set()
    for chunk in range(64):
        lo, hi, current = C.c_float(0), C.c_float(0), C.c_int32(0)
        native.check(lib.ilm_debug_chunk_category_bounds(C.c_uint64(ps.Handle), chunk, C.byref(lo), C.byref(hi), C.byref(current)))
        records.add((lo.value, hi.value, current.value))
    print("category records of the 64 chunks (lo, hi, current):", sorted(records))


if __name__ == "__main__":
    main()
