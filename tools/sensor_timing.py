"""Run ON THE GPU BOX.  ilm_system_sense (particle sensors, CollectParticles.fx) at cfg4's per-GPU share (8 chunks of 1024^2 = 8.4 M slots,
HBM-resident) and at cfg2's size (16 chunks of 256^2 = 1 M slots, cache-resident), with 1 and 8 box sensors, beside two yardsticks on the
same system and box: ilm_system_live_counts (the 4 B/slot reduction the sensor kernel grew from) and the floor 20 B x slots over the box's
calibrated copy rate (csrc/calib.hip, the figure bench.py --full prints as hbm_calibration).

    python tools/sensor_timing.py [--out FILE] [--reps N]

Three clocks per row, after warm-up:
  queued   ilm_timer_* (device events) around `reps` ilm_system_sense_async calls back to back: memset + sense_kernel + the copy of the
           table, no host in between -- the figure to hold against the floor
  blocking ilm_timer_* around `reps` blocking calls (each synchronises: the device idles while the host returns), for sense and live counts
  host     the host's clock around the same blocking calls, per call
The floor counts 20 B per slot although a wave none of whose slots has life > 1 loads 8 B per slot (half the particles here are that
alive: nearly every wave loads everything)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from illuminant_amd import abi, native, scenes  # noqa: E402

SIZES = (("cfg4 share", 1024, 8), ("cfg2", 256, 16))


def box_sensor(k):
    a = abi.AreaParams()
    a.AreaType = 2
    a.Strength = 1.0
    a.AreaFalloff = 120.0
    a.AreaRotation = 0.5          # the unit quaternion (0.5, 0.5, 0.5, 0.5): a pure rotation
    a.AreaCenter[0], a.AreaCenter[1], a.AreaCenter[2] = 400.0 + 150.0 * k, 300.0 + 60.0 * k, 16.0
    a.AreaSize[0], a.AreaSize[1], a.AreaSize[2] = 300.0, 200.0, 250.0
    a.CategoryFilter[0], a.CategoryFilter[1] = 0.0, 1.0 + (k % 2)
    return a


def calibrated_copy_rate(device):
    """GB/s of the best of calib.hip's three copy kernels (read + written bytes), or None without the calibration library."""
    path = os.path.join(ROOT, "illuminant_amd", "lib", "libilluminant_calib.so")
    if not os.path.exists(path):
        return None
    cl = C.CDLL(path)
    cl.ilm_calib_copy_rates.argtypes = [C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    out = (C.c_double * 3)()
    if cl.ilm_calib_copy_rates(int(device), C.c_size_t(1 << 30), 6, out) != 0:
        return None
    return max(float(out[i]) for i in range(3))


def build(ctx, cs, n_chunks):
    eng = native.Engine(ctx, cs, scenes.randomness_table(7))
    sysm = native.System(eng)
    for c in range(n_chunks):
        sysm.add_chunk()
        pos, vel, _ = scenes.make_particles(100 + c, cs * cs, pos_lo=(0, 0, 0), pos_hi=(1920, 1080, 32), life=(0.0, 2.0), categories=(0.0, 1.0, 2.0, 3.0))
        sysm.upload(c, abi.PLANE_POSITION, pos)
        sysm.upload(c, abi.PLANE_VELOCITY, vel)
    return eng, sysm


def device_ms(ctx, fn, reps):
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def host_ms(ctx, fn, reps):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    assert native.device_count() > 0, "needs a GPU"
    ctx = native.Context(0)
    rate = calibrated_copy_rate(0)
    lines = ["ilm_system_sense: box sensors (rotated, falloff 120, a category filter), %d calls per figure after warm-up" % args.reps,
             "calibrated copy rate of this box (csrc/calib.hip, read + written): %s GB/s" % ("%.0f" % rate if rate else "not measured"), "",
             "%-11s %9s %8s | %10s %10s %10s | %10s %10s | %9s %9s" % ("size", "slots", "sensors", "queued us", "blocking", "host us", "live cnt", "host us",
                                                                     "floor us", "queued/fl")]
    for name, cs, n_chunks in SIZES:
        eng, sysm = build(ctx, cs, n_chunks)
        slots = cs * cs * n_chunks
        floor_us = 20.0 * slots / (rate * 1e9) * 1e6 if rate else None
        live = lambda: sysm.live_counts()
        for _ in range(5):
            live()
        live_dev, live_host = device_ms(ctx, live, args.reps), host_ms(ctx, live, args.reps)
        for n in (1, 8):
            sensors = [box_sensor(k) for k in range(n)]
            counts = sysm.sense(sensors)
            assert counts.shape == (n, n_chunks) and counts.all() and (counts < cs * cs).all()
            blocking, queued = (lambda: sysm.sense(sensors)), (lambda: sysm.sense_async(sensors))
            for _ in range(5):
                blocking(); queued()
            q = device_ms(ctx, queued, args.reps)
            assert (sysm.poll_sense() == counts).all()
            b, h = device_ms(ctx, blocking, args.reps), host_ms(ctx, blocking, args.reps)
            lines.append("%-11s %9d %8d | %10.1f %10.1f %10.1f | %10.1f %10.1f | %9s %9s"
                         % (name, slots, n, q * 1e3, b * 1e3, h * 1e3, live_dev * 1e3, live_host * 1e3,
                            "%.1f" % floor_us if floor_us else "-", "%.2f" % (q * 1e3 / floor_us) if floor_us else "-"))
        sysm.close(); eng.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
