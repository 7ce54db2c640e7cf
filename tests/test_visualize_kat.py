"""The distance-field view without a GPU: the ABI's two structs against the C header, the symbol in header, library and bindings, the
entry point's refusals (its vertex and parameter values are judged before any handle is looked up), the restatement
(tests/visualize_common.py) against facts known by construction, and the host mirror's quad against the line-by-line transliteration.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from illuminant_amd import abi, native
from tests import visualize_common as vc

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "illuminant_hip.h")


def test_struct_layouts_match_the_c_header(tmp_path):
    structs = {"IlmVisualizeVertex": abi.VisualizeVertex, "IlmVisualizeParams": abi.VisualizeParams}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void) {"]
    for cname, mirror in structs.items():
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in mirror._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.splitlines():
        cname, what, value = line.split()
        if what == "sizeof":
            assert C.sizeof(structs[cname]) == int(value) == abi.EXPECTED_SIZES[cname][1], cname
        else:
            assert getattr(structs[cname], what).offset == int(value), (cname, what)
        seen += 1
    assert seen == 2 + 4 + 12
    assert C.sizeof(abi.VisualizeVertex) == 52 and C.sizeof(abi.VisualizeParams) == 80


def test_header_library_and_bindings_agree_on_the_symbol():
    text = open(HEADER).read()
    assert re.search(r"^int32_t ilm_visualize_distance_field\(IlmHandle ctx, IlmHandle sdf,", text, flags=re.M)
    assert "ilm_visualize_distance_field" in native.SYMBOLS and len(native.SYMBOLS["ilm_visualize_distance_field"][1]) == 7
    assert native.lib().ilm_visualize_distance_field is not None
    assert int(re.search(r"#define ILM_ABI_VERSION (\d+)", text).group(1)) == abi.ABI_VERSION == native.lib().ilm_abi_version() == 11
    # untagged typedefs: the tagged form must not appear for them anywhere in the header, comments included
    assert "typedef struct IlmVisualize" not in text
    cs = open(os.path.join(ROOT, "integration", "IlluminantHip.cs")).read()
    assert "ilm_visualize_distance_field (ulong ctx, ulong sdf, IlmDistanceFieldUniforms* df, IlmVisualizeVertex* quad" in cs
    assert "VISUALIZE_SILHOUETTES = 2" in cs and "struct IlmVisualizeParams" in cs
    assert (abi.VISUALIZE_SURFACES, abi.VISUALIZE_OUTLINES, abi.VISUALIZE_SILHOUETTES) == (0, 1, 2)


# ---- refusals ---------------------------------------------------------------------------------------------------------------

REFUSALS = vc.refusal_cases()


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_without_a_device(case):
    """Each refusal gives ILM_ERR_INVALID_ARGUMENT and names its reason; the stats are not touched (no object exists to touch)."""
    _, quad, params, word = case
    lib = native.lib()
    dfu = vc.field_layout().uniforms()
    stats = (C.c_uint64 * 3)(7, 8, 9)
    vertices = vc.quad_array(quad)
    rc = lib.ilm_visualize_distance_field(abi.Handle(0), abi.Handle(0), C.cast(C.byref(dfu), C.c_void_p), C.cast(vertices, C.c_void_p),
                                          C.cast(C.byref(params), C.c_void_p), abi.Handle(0), C.cast(stats, C.c_void_p))
    assert rc == abi.ERR_INVALID_ARGUMENT
    assert word.lower() in lib.ilm_last_error().decode().lower(), lib.ilm_last_error()
    assert list(stats) == [7, 8, 9]


def test_bad_handles_without_a_device():
    lib = native.lib()
    dfu = vc.field_layout().uniforms()
    quad = vc.quad_array(vc.camera_quad(vc.OBLIQUE))
    stats = (C.c_uint64 * 3)(7, 8, 9)
    for mode in (vc.SURFACES, vc.OUTLINES, vc.SILHOUETTES):
        params = vc.make_params(mode)
        for handle in (0, 12345):
            rc = lib.ilm_visualize_distance_field(abi.Handle(handle), abi.Handle(handle), C.cast(C.byref(dfu), C.c_void_p), C.cast(quad, C.c_void_p),
                                                  C.cast(C.byref(params), C.c_void_p), abi.Handle(handle), C.cast(stats, C.c_void_p))
            assert rc == abi.ERR_INVALID_HANDLE and b"context" in lib.ilm_last_error()
            assert list(stats) == [7, 8, 9]
    # an empty rectangle is not a refusal: it gets as far as the handles
    params = vc.make_params(0)
    empty = vc.quad_array(vc.camera_quad(vc.TOP_DOWN, size=(0, 0)))
    rc = lib.ilm_visualize_distance_field(abi.Handle(0), abi.Handle(0), C.cast(C.byref(dfu), C.c_void_p), C.cast(empty, C.c_void_p),
                                          C.cast(C.byref(params), C.c_void_p), abi.Handle(0), None)
    assert rc == abi.ERR_INVALID_HANDLE, lib.ilm_last_error()
    assert lib.ilm_visualize_distance_field(abi.Handle(0), abi.Handle(0), C.cast(C.byref(dfu), C.c_void_p), None, C.cast(C.byref(params), C.c_void_p),
                                            abi.Handle(0), None) == abi.ERR_INVALID_ARGUMENT
    assert lib.ilm_visualize_distance_field(abi.Handle(0), abi.Handle(0), None, C.cast(quad, C.c_void_p), C.cast(C.byref(params), C.c_void_p),
                                            abi.Handle(0), None) == abi.ERR_INVALID_ARGUMENT


# ---- the restatement against facts known by construction ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def box_field(oracle):
    atlas = np.ascontiguousarray(vc.field_atlas(abi.SDF_UNORM16, (vc.BOX,)))
    return vc.field_layout().uniforms(), oracle.make_texture(atlas, abi.SDF_UNORM16)


def _pixel_xy(quad, i, j, size=vc.VIEW_SIZE):
    """World (x, y) of pixel (i, j) of a top-down camera quad whose rectangle starts at the origin."""
    u, v = (i + 0.5) / size[0], (j + 0.5) / size[1]
    tl, tr, bl = quad[0, 3:6].astype(np.float64), quad[1, 3:6].astype(np.float64), quad[3, 3:6].astype(np.float64)
    p = tl + (tr - tl) * u + (bl - tl) * v
    return p[0], p[1]


def test_top_down_surface_view_of_the_box(oracle, box_field):
    """Rays straight down onto the box alone: a pixel is drawn exactly when the march found a sample at or below its step threshold; every
    ray over the box's footprint must find one (sphere tracing converges onto the top face), and no ray farther than 12 units from the
    footprint can -- the threshold never exceeds TRACE_FINAL_MIN_STEP_SIZE = 12 and the sampled field is at least the distance to the box
    (interpolating a convex distance function over-estimates it)."""
    dfu, texture = box_field
    quad = vc.camera_quad(vc.TOP_DOWN)
    r = vc.render(oracle, dfu, texture, quad, vc.make_params(vc.SURFACES), np.zeros((24, 32, 4), np.float32))
    assert r.covered.all() and r.stats[0] == 768 and 0 < r.stats[1] < 768
    _, center, size = vc.BOX
    inside = outside = 0
    for j in range(24):
        for i in range(32):
            d = r.detail[(i, j)]
            assert r.drawn[j, i] == d["hit"]
            if d["hit"]:
                assert d["last"] <= d["threshold"] <= F(12) and r.samples[j, i] >= 5
            x, y = _pixel_xy(quad, i, j)
            dx, dy = abs(x - center[0]) - size[0], abs(y - center[1]) - size[1]
            if dx < -1.0 and dy < -1.0:
                assert r.drawn[j, i], (i, j)
                inside += 1
            if max(dx, dy) > 12.0:
                assert not r.drawn[j, i], (i, j)
                outside += 1
    assert inside >= 20 and outside >= 300
    # a drawn pixel is opaque: ambient + light, alpha 1, over whatever was there
    assert np.all(r.image[r.drawn][:, 3] == 1.0) and np.all(r.image[~r.drawn] == 0.0)
    assert np.all(r.image[r.drawn][:, :3] >= np.array(vc.DEFAULT_AMBIENT, np.float32))
    assert r.stats[2] == int(r.samples.sum()) and r.stats[2] > 4 * r.stats[1]


def test_silhouette_alpha_is_one_wherever_the_ray_meets_the_surface(oracle, box_field):
    dfu, texture = box_field
    for view in (vc.TOP_DOWN, vc.OBLIQUE):
        quad = vc.camera_quad(view)
        r = vc.render(oracle, dfu, texture, quad, vc.make_params(vc.SILHOUETTES), np.zeros((24, 32, 4), np.float32))
        met = np.zeros((24, 32), bool)
        for (i, j), d in r.detail.items():
            met[j, i] = d["closest"] <= F(1)
            assert (d["alpha"] == F(1)) == bool(met[j, i]) or (d["alpha"] == F(1) and d["closest"] == F(1))
        assert met.any() and not met.all()
        assert np.all(r.image[met] == 1.0)                            # colour (1, 1, 1, 1) x alpha 1 over black
        # the outline mode draws the rim only: the interior's closest distance lies more than OutlineSize below 1
        o = vc.render(oracle, dfu, texture, quad, vc.make_params(vc.OUTLINES), np.zeros((24, 32, 4), np.float32))
        assert 0 < o.stats[1] < r.stats[1] and np.all(o.image[..., 3] <= 1.0)
        assert (met & ~o.drawn).any()


def test_blends_by_hand():
    src, dst = np.array([0.25, 0.5, 0.125, 0.5], np.float32), np.array([0.5, 0.25, 1.0, 0.75], np.float32)
    assert list(vc.blend(src, dst, abi.BLEND_ALPHA)) == [0.5, 0.625, 0.625, 0.875]
    assert list(vc.blend(src, dst, abi.BLEND_ADDITIVE)) == [0.75, 0.75, 1.125, 1.25]


# ---- the host mirror's quad ---------------------------------------------------------------------------------------------------

VIEWS = [(0.0, 0.0, -1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), vc.OBLIQUE, (-0.4, 0.2, 0.9)]


@pytest.mark.parametrize("view", VIEWS)
def test_host_mirror_quad_matches_the_transliteration(view):
    from illuminant_amd import _host as H
    rectangle = (4.25, 1.5, 36.25, 25.5)
    color = (0.5, 0.25, 1.0, 0.75)
    for world_min, world_max in (((0, 0, 0), (64, 48, 32)), ((-3.0, 2.0, 1.0), (61.0, 50.0, 33.0))):
        info, raw = H.LightingRenderer.BuildVisualizationQuad(list(rectangle), list(view), list(world_min), list(world_max), list(color))
        want_info, want = vc.reference_quad(rectangle, view, world_min, world_max, color)
        assert info.Failed == want_info["Failed"]
        for name in ("Up", "Right", "ViewDirection") + (() if info.Failed else ("ViewCenter",)):
            assert np.array(getattr(info, name), np.float32).tobytes() == want_info[name].astype(np.float32).tobytes(), name
        if info.Failed:
            continue
        got = np.frombuffer(raw, np.float32).reshape(4, 13)
        assert got.tobytes() == want.tobytes(), (got, want)
        # TL, TR, BR, BL of an axis-aligned rectangle moved by half a texel of the view (LightingRenderer.cs:1760)
        assert got[0, 0] == got[3, 0] == F(F(4.25) + F(-0.5) * F(F(1) / F(32))) and got[0, 1] == got[1, 1] and got[1, 0] == got[2, 0]
        # the entry point accepts what the mirror builds
        assert np.all(got[:, 6:13] == got[0, 6:13])


def test_host_mirror_reports_failed_when_no_plane_is_met():
    """FindBoxIntersection's first three planes all use boxMin.X (as written): with boxMin.X = -50 the plane `z = 50` lies behind a ray
    that starts at z = 10 and runs towards -z, the far plane z = 30 lies behind it too, and the x / y planes are parallel to it."""
    from illuminant_amd import _host as H
    args = ((0.0, 0.0, 32.0, 24.0), (0.0, 0.0, 1.0), (-50.0, 0.0, 10.0), (50.0, 40.0, 30.0))
    info, _ = H.LightingRenderer.BuildVisualizationQuad(*[list(a) for a in args], [1, 1, 1, 1])
    want_info, want = vc.reference_quad(*args)
    assert info.Failed and want_info["Failed"] and want is None
    assert info.Up == [0.0, -1.0, 0.0] and info.Right == [1.0, 0.0, 0.0] and info.ViewDirection == [0.0, 0.0, 1.0]
    assert vc.find_box_intersection(vc._v(0, 20, 10), vc._v(0, 0, -1), vc._v(-50, 0, 10), vc._v(50, 40, 30)) is None
    assert vc.ray_intersects_plane(vc._v(0, 0, 0), vc._v(0, 0, 1), vc._v(0, 0, 1), F(5e-6)) == F(0)       # -5e-6: clamped to 0
    assert vc.ray_intersects_plane(vc._v(0, 0, 0), vc._v(0, 0, 1), vc._v(0, 0, 1), F(1.0)) is None          # t = -1
    assert vc.ray_intersects_plane(vc._v(0, 0, 0), vc._v(1, 0, 0), vc._v(0, 0, 1), F(1.0)) is None          # parallel
