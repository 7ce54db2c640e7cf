"""A/B of a frame of MANY small particle systems (the reference's Scenes/ManySystemsManySpawners.cs: 256 systems on an engine of
ChunkSize 128, each updated every frame): A = one ilm_system_step per system, B = one ilm_engine_step_batch for the frame.

Workload: N systems (16, 64, 256, 1024) of one uploaded full chunk each (16 384 particles), cfg2's transform list without its spawner
(Gravity with 4 attractors, Noise, UpdatePositions), liveness counting every 5th frame; systems 0, 2, 5 and 9 also own a spawn-target
chunk and two inline spawners at the scene's rates (10..50 particles / s each: one slot per frame between them).

Method: A and B run in the same process on twin sets of systems with the same content, both warmed; blocks of --frames frames alternate
A, B, A, B ...; each block is timed with the host clock up to the end of an ilm_ctx_sync and with the context's HIP events beside it.
Reported per N: median / minimum / maximum block time per frame for A and B, the launches per frame B needed (ilm_debug_last_step_batch),
and the CRC of every plane of every system after the last block of A and of B (the twins took the same frames: the CRCs must be equal).
The criterion is B's median below A's by more than A's own spread (max - min) at N = 256; the script states whether it holds.

  python tools/step_batch_ab.py [--frames 200] [--blocks 5] [--sizes 16,64,256,1024] [--out FILE]        (on the GPU box)
"""
import argparse
import ctypes as C
import os
import sys
import time
import zlib


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from illuminant_amd import abi, native, scenes   # noqa: E402

CS = 128
SLOTS = CS * CS
SPAWNING = (0, 2, 5, 9)
PLANES = (abi.PLANE_POSITION, abi.PLANE_VELOCITY, abi.PLANE_ATTRIBUTES, abi.PLANE_RENDER_COLOR, abi.PLANE_RENDER_DATA)
ATTRACTORS = [((400., 300., 0.), 70., 600., 0), ((1500., 300., 0.), 150., 900., 0), ((400., 800., 0.), 200., 1200., 0), ((1500., 800., 0.), 100., 1500., 0)]


def step_desc(counting):
    d = abi.StepDesc()
    d.FirstChunk, d.ChunkCount = 0, -1
    d.System = scenes.system_uniforms(CS, friction=0.02, max_velocity=2048.0, life_decay=0.01)
    d.Update = abi.UpdateParams.default()
    d.OpCount = 2
    d.Ops[0].Type = abi.OP_GRAVITY
    d.Ops[0].u.Gravity = scenes.gravity_params(ATTRACTORS, maximum_acceleration=1024.0)
    d.Ops[1].Type = abi.OP_NOISE
    d.Ops[1].u.Noise = scenes.noise_params(scenes.area_none(), (0.37 * 253, 0.81 * 127), (0.12 * 253, 0.55 * 127), 0.35)
    d.UpdateMode = abi.UPDATE_POSITIONS
    d.Flags = abi.STEP_COUNT_LIVE if counting else 0
    return d


class Side:
    """One of the twin sets: N systems on an engine of its own, their descriptors for a plain and for a counting frame."""

    def __init__(self, ctx, rnd, n, particles):
        self.ctx, self.n = ctx, n
        self.engine = native.Engine(ctx, CS, rnd)
        self.systems = []
        pos, vel, attr = particles
        for i in range(n):
            s = native.System(self.engine)
            s.add_chunk()
            at = (i % 16) * SLOTS
            s.upload(0, PLANES[0], pos[at:at + SLOTS]); s.upload(0, PLANES[1], vel[at:at + SLOTS]); s.upload(0, PLANES[2], attr[at:at + SLOTS])
            if i in SPAWNING:
                s.add_chunk()
            self.systems.append(s)
        self.descs = [(abi.StepDesc * n)(), (abi.StepDesc * n)()]        # [plain, counting]
        for counting in (0, 1):
            template = step_desc(bool(counting))
            for i in range(n):
                C.memmove(C.byref(self.descs[counting], i * C.sizeof(abi.StepDesc)), C.byref(template), C.sizeof(abi.StepDesc))
        self.spawners = {i: [scenes.spawn_params(CS, 0, 0, 0, (0.3 * 253, 0.6 * 127), position=((100.0 + 37.0 * i + 500.0 * k, 200.0 + 11.0 * i, 0), (16, 16, 0), (0, 0, 0), scenes.FORMULA_SPHERICAL),
                                                 velocity=((0, 0, 0), (60, 60, 10), (0, 0, 0), scenes.FORMULA_SPHERICAL), life=(60.0, 5.0, 0.0)) for k in (0, 1)]
                         for i in SPAWNING if i < n}
        self.handles = (abi.Handle * n)(*[s.handle.value for s in self.systems])
        size = C.sizeof(abi.StepDesc)
        self.item_args = [[(abi.Handle(s.handle.value), C.c_void_p(C.addressof(arr) + i * size)) for i, s in enumerate(self.systems)] for arr in self.descs]
        self.frame_index = 0

    def next_frame(self):
        """The frame's descriptor array: counting every 5th frame, the spawners' one slot of the frame."""
        f = self.frame_index
        self.frame_index += 1
        counting = 1 if f % 5 == 0 else 0
        arr = self.descs[counting]
        for i, pair in self.spawners.items():
            p = pair[f % 2]
            p.ChunkSizeAndIndices[1] = p.ChunkSizeAndIndices[2] = float(f)       # slot f of the spawn-target chunk
            arr[i].SpawnCount = 1
            arr[i].Spawns[0].ChunkIndex = 1
            arr[i].Spawns[0].Kind = abi.SPAWN_INLINE
            arr[i].Spawns[0].Params = p
        return counting

    def frame_a(self, step):
        for h, p in self.item_args[self.next_frame()]:
            rc = step(h, p)
            if rc != 0:
                native.check(rc)

    def frame_b(self, step_batch):
        arr = self.descs[self.next_frame()]
        native.check(step_batch(self.engine.handle, C.cast(self.handles, C.c_void_p), C.cast(arr, C.c_void_p), self.n))

    def crc(self, stride=1):
        crc = 0
        for s in self.systems[::stride]:
            for c in range(s.chunk_count()):
                for plane in PLANES:
                    crc = zlib.crc32(s.download(c, plane).tobytes(), crc)
        return crc

    def close(self):
        for s in self.systems:
            s.close()
        self.engine.close()


def run(ctx, rnd, particles, n, frames, blocks, warm, emit):
    lib = native.lib()
    a, b = Side(ctx, rnd, n, particles), Side(ctx, rnd, n, particles)
    assert warm + blocks * frames < SLOTS, "the spawners take one slot of their chunk per frame"
    for _ in range(warm):
        a.frame_a(lib.ilm_system_step)
        b.frame_b(lib.ilm_engine_step_batch)
    ctx.sync()
    times = {"A": [], "B": []}
    events = {"A": [], "B": []}
    launches = []
    for block in range(blocks):
        for name, side in (("A", a), ("B", b)):
            ctx.sync()
            ctx.timer_start()
            t0 = time.perf_counter()
            if name == "A":
                for _ in range(frames):
                    side.frame_a(lib.ilm_system_step)
            else:
                for _ in range(frames):
                    side.frame_b(lib.ilm_engine_step_batch)
            ctx.sync()
            times[name].append((time.perf_counter() - t0) / frames * 1e6)
            events[name].append(ctx.timer_stop() / frames * 1e3)
        launches.append(b.engine.last_step_batch())
    stride = 1 if n <= 256 else 8
    crc_a, crc_b = a.crc(stride), b.crc(stride)
    med = lambda v: sorted(v)[len(v) // 2]
    row = {"n": n}
    for name in ("A", "B"):
        row[name] = (med(times[name]), min(times[name]), max(times[name]), med(events[name]))
        emit("N=%4d %s: host clock median %9.1f min %9.1f max %9.1f us/frame   HIP events median %9.1f us/frame   (%d blocks of %d frames)" % (
            n, name, row[name][0], row[name][1], row[name][2], row[name][3], blocks, frames))
    emit("N=%4d    launches per frame: A %d (one per system), B %d in %d round(s), %d item(s) one by one" % (n, n, launches[-1][0], launches[-1][1], launches[-1][2]))
    emit("N=%4d    CRC of the planes%s after the last block: A %08x  B %08x  %s" % (n, "" if stride == 1 else " (every %dth system)" % stride, crc_a, crc_b,
                                                                                 "equal" if crc_a == crc_b else "DIFFERENT"))
    spread = row["A"][2] - row["A"][1]
    emit("N=%4d    A / B = %.2f (medians); A's block-to-block spread %.1f us/frame; B's median is %s A's by more than that" % (
        n, row["A"][0] / row["B"][0], spread, "below" if row["A"][0] - row["B"][0] > spread else "NOT below"))
    row["crc_equal"] = crc_a == crc_b
    row["wins"] = row["A"][0] - row["B"][0] > spread
    a.close(); b.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--sizes", default="16,64,256,1024")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    ctx = native.Context(0)
    rnd = scenes.randomness_table(7)
    particles = scenes.make_particles(1000, 16 * SLOTS, pos_lo=(0, 0, 0), pos_hi=(1920, 1080, 32), life=(50.0, 90.0))
    emit("# tools/step_batch_ab.py: A = ilm_system_step per system, B = one ilm_engine_step_batch per frame; chunk size %d, one full chunk per system" % CS)
    rows = [run(ctx, rnd, particles, int(n), args.frames, args.blocks, args.warm, emit) for n in args.sizes.split(",")]
    ok = all(r["crc_equal"] for r in rows)
    at256 = [r for r in rows if r["n"] == 256]
    if at256:
        emit("# criterion at N = 256: %s" % ("B wins by more than A's spread" if at256[0]["wins"] else "B does NOT win by more than A's spread"))
    emit("# CRCs: %s" % ("all equal" if ok else "NOT all equal"))
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
