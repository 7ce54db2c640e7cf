"""ilm_engine_render_particle_lights_batch without a GPU: IlmParticleLightItem's layout against the header (an untagged typedef, so
tests/test_abi_layout.py does not see it), the two names in the header and the C# binding, both entry points looking their handles up
first, and the invariants of the chained-oracle scenes the GPU tests rely on -- held on the oracle alone, so that no GPU test passes
vacuously."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from illuminant_amd import abi, native
from tests import particle_light_batch_common as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "illuminant_hip.h")
CSHARP = os.path.join(ROOT, "integration", "IlluminantHip.cs")
NAMES = ("ilm_engine_render_particle_lights_batch", "ilm_debug_last_particle_light_batch")


def test_struct_layout_matches_the_c_header(tmp_path):
    mirror = abi.ParticleLightItem
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(IlmParticleLightItem));']
    for fname, _ in mirror._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(IlmParticleLightItem, %s));' % (fname, fname))
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == C.sizeof(mirror) == abi.EXPECTED_SIZES["IlmParticleLightItem"][1] == 104
    assert {f: int(v) for f, v in out.items()} == dict(System=0, QuadCounts=8, ChunkCount=16, _pad=20, Params=24)
    for fname, value in out.items():
        assert getattr(mirror, fname).offset == int(value), fname
    # the params are the single call's, member for member
    assert mirror.Params.size == C.sizeof(abi.ParticleLightParams) == 80


def test_both_names_are_in_the_header_and_the_csharp_binding():
    header, csharp = open(HEADER).read(), open(CSHARP).read()
    for name in NAMES:
        assert re.search(r"^int32_t %s\(" % name, header, re.M), name
        assert re.search(r"public static extern int %s \(" % name, csharp), name
        assert hasattr(native.lib(), name)
    assert "} IlmParticleLightItem;" in header and "public struct IlmParticleLightItem" in csharp


def test_entry_points_refuse_bad_handles_without_a_device():
    lib = native.lib()
    items = (abi.ParticleLightItem * 2)()
    stats = abi.RenderStats(7, 7, 7)
    for handle in (0, 12345):
        rc = lib.ilm_engine_render_particle_lights_batch(abi.Handle(handle), C.cast(items, C.c_void_p), 2, None, None, abi.Handle(0), abi.Handle(0),
                                                         abi.Handle(handle), 0, 1, C.cast(C.byref(stats), C.c_void_p))
        assert rc == abi.ERR_INVALID_HANDLE and b"engine" in lib.ilm_last_error()
        assert (stats.SdfSamples, stats.PixelLightPairs, stats.TracedPairs) == (7, 7, 7)
        n = C.c_int32(-7)
        assert lib.ilm_debug_last_particle_light_batch(abi.Handle(handle), C.byref(n), C.byref(n), C.byref(n)) == abi.ERR_INVALID_HANDLE
        assert b"engine" in lib.ilm_last_error() and n.value == -7
    # the handle comes first: a NULL item list or a negative count behind a bad handle is still a handle error
    for count in (3, -1):
        assert lib.ilm_engine_render_particle_lights_batch(abi.Handle(0), None, count, None, None, abi.Handle(0), abi.Handle(0), abi.Handle(0), 0, 0,
                                                           None) == abi.ERR_INVALID_HANDLE
    assert lib.ilm_debug_last_particle_light_batch(abi.Handle(0), None, None, None) == abi.ERR_INVALID_HANDLE


def test_the_crowded_scene_emits_more_than_one_wide_list_batch():
    sc = bc.crowded_scene()
    counts = [sc.emitting(it) for it in sc.items]
    assert sum(counts) >= 4097 and all(c > 0 for c in counts)
    assert sc.slots == 1600 and [it.chunk_count for it in sc.items] == [1, 2, 1]
    # the three items' chunks, concatenated, are system 3's
    joined = [planes for it in sc.items for planes in sc.systems[it.system][:it.chunk_count]]
    assert len(joined) == len(sc.systems[3]) == 4 and all(a is b for a, b in zip(joined, sc.systems[3]))


def test_the_mixed_scene_is_what_the_gpu_tests_assume(oracle):
    sc = bc.mixed_scene()
    assert (sc.width, sc.height, sc.slots) == (70, 45, 144)
    assert [it.chunk_count for it in sc.items] == [0, 1, 3, 2, 6, 1]
    assert sc.items[4].chunk_count < len(sc.systems[sc.items[4].system]), "one item passes fewer chunks than its system has"
    assert sc.items[1].system == sc.items[5].system and bytes(sc.items[1].params) != bytes(sc.items[5].params)
    assert len({bytes(it.params) for it in sc.items}) == len(sc.items), "every item has its own template"
    assert all(it.quads[-1] == 100 for it in sc.items if it.chunk_count)
    want, stats = bc.chained_oracle(oracle, sc)
    assert (want[..., 3] > 3.5).any(), "several lights overlap somewhere"
    assert stats[2] > 1000, "shadowed items trace"
    # item 3 is all dead: it emits nothing and contributes nothing; every other item with chunks contributes
    assert sc.emitting(sc.items[3]) == 0
    alone, dead_stats = bc.chained_oracle(oracle, sc, items=[3])
    assert alone.tobytes() == bc.ambient_frame(sc).tobytes() and dead_stats == (0, 0, 0)
    for i in (1, 2, 4, 5):
        assert sc.emitting(sc.items[i]) > 0
        assert (bc.chained_oracle(oracle, sc, items=[i])[0] != bc.ambient_frame(sc)).any(), i
    # the half tests start from an ambient that a half holds exactly
    assert np.array_equal(np.asarray(bc.HALF_AMBIENT, np.float32), np.asarray(bc.HALF_AMBIENT, np.float32).astype(np.float16).astype(np.float32))
