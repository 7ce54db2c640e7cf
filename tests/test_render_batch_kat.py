"""ilm_engine_render_particles_batch without a GPU: IlmRasterizeItem's layout against the header (an untagged typedef, so
tests/test_abi_layout.py does not see it), and both entry points looking their handles up before anything else."""
import ctypes as C
import os
import subprocess

from illuminant_amd import abi, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "illuminant_hip.h")


def test_struct_layout_matches_the_c_header(tmp_path):
    mirror = abi.RasterizeItem
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(IlmRasterizeItem));']
    for fname, _ in mirror._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(IlmRasterizeItem, %s));' % (fname, fname))
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == C.sizeof(mirror) == abi.EXPECTED_SIZES["IlmRasterizeItem"][1] == 216
    assert sorted(out) == sorted(f for f, _ in mirror._fields_) and len(out) == 5
    for fname, value in out.items():
        assert getattr(mirror, fname).offset == int(value), fname
    # the params are the single call's, member for member
    assert mirror.Params.offset == 24 and mirror.Params.size == C.sizeof(abi.RasterizeParams) == 192


def test_entry_points_refuse_bad_handles_without_a_device():
    lib = native.lib()
    items = (abi.RasterizeItem * 2)()
    stats = (C.c_uint64 * 3)(7, 7, 7)
    for handle in (0, 12345):
        rc = lib.ilm_engine_render_particles_batch(abi.Handle(handle), C.cast(items, C.c_void_p), 2, abi.Handle(handle), C.cast(stats, C.c_void_p))
        assert rc == abi.ERR_INVALID_HANDLE and b"engine" in lib.ilm_last_error()
        assert list(stats) == [7, 7, 7]
        n = C.c_int32(-7)
        assert lib.ilm_debug_last_render_batch(abi.Handle(handle), C.byref(n), C.byref(n), C.byref(n)) == abi.ERR_INVALID_HANDLE
        assert b"engine" in lib.ilm_last_error() and n.value == -7
    # the handle comes first: a NULL item list or a negative count behind a bad handle is still a handle error
    assert lib.ilm_engine_render_particles_batch(abi.Handle(0), None, 3, abi.Handle(0), None) == abi.ERR_INVALID_HANDLE
    assert lib.ilm_engine_render_particles_batch(abi.Handle(0), None, -1, abi.Handle(0), None) == abi.ERR_INVALID_HANDLE
    assert lib.ilm_debug_last_render_batch(abi.Handle(0), None, None, None) == abi.ERR_INVALID_HANDLE
