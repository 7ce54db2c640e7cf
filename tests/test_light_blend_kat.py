"""ilm_ctx_set_light_blend_function without a GPU: the symbol in the header, the library, the ctypes table and the C# layer; the refusal
that needs no device; the numpy statement of the combine rules (tests/light_blend_common.py) on cases worked out by hand; the words of the
header's contract."""
import os
import re
import subprocess
import sys

import numpy as np

from illuminant_amd import abi, native
from tests import light_blend_common as lb

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADD, RSUB, MAX, MIN = lb.ADD, lb.REVERSE_SUBTRACT, lb.MAX, lb.MIN


def header():
    return open(os.path.join(ROOT, "include", "illuminant_hip.h")).read()


def image(*pixels):
    """a 1 x n image of the given (r, g, b, a) pixels"""
    return np.asarray([list(pixels)], np.float32)


def test_the_symbol_is_exported_bound_and_declared():
    text = header()
    decl = re.search(r"^int32_t ilm_ctx_set_light_blend_function\(([^)]*)\);", text, flags=re.M).group(1)
    assert [p.strip().rsplit(" ", 1) for p in decl.split(",")] == [["IlmHandle", "ctx"], ["int32_t", "color_function"], ["int32_t", "alpha_function"]]
    for name, value in (("ADD", 0), ("REVERSE_SUBTRACT", 1), ("MAX", 2), ("MIN", 3)):
        assert re.search(r"^#define ILM_LIGHT_BLEND_%s\s+%d\b" % (name, value), text, flags=re.M), name
        assert getattr(abi, "LIGHT_BLEND_" + name) == value == getattr(lb, name)
    result, args = native.SYMBOLS["ilm_ctx_set_lightmap_blend"]
    assert native.SYMBOLS["ilm_ctx_set_light_blend_function"] == (result, args + [args[-1]])      # one more int32 than the model's setter
    assert hasattr(native.lib(), "ilm_ctx_set_light_blend_function")
    cs = open(os.path.join(ROOT, "integration", "IlluminantHip.cs")).read()
    assert "ilm_ctx_set_light_blend_function (ulong ctx, int colorFunction, int alphaFunction)" in cs
    assert "LIGHT_BLEND_REVERSE_SUBTRACT = 1" in cs
    assert "#define ILM_ABI_VERSION 11" in text and "+ ilm_ctx_set_light_blend_function" in text[:text.index("#define ILM_ABI_VERSION")]
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_csharp_binding.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr


def test_handle_zero_is_refused_before_the_functions_are_looked_at():
    lib = native.lib()
    assert lib.ilm_ctx_set_light_blend_function(abi.Handle(0), abi.LIGHT_BLEND_MAX, abi.LIGHT_BLEND_ADD) == abi.ERR_INVALID_HANDLE
    assert lib.ilm_ctx_set_light_blend_function(abi.Handle(0), 99, -5) == abi.ERR_INVALID_HANDLE
    assert b"context" in lib.ilm_last_error()


def test_the_contract_names_what_is_not_built():
    text = header()
    contract = text[text.index("/* Light blend functions"):text.index("int32_t ilm_ctx_set_light_blend_function")]
    for word in ("Not built", "BlendFunction.Subtract (src - dst)", "destination-colour factors", "multiplicative", "blend factors and write masks",
                 "ilm_render_light_probes\n * ignores it", "(c > M) ? c : M", "(M < base) ? M : base", "not fmaxf / fminf", "half(dst - s)",
                 "ilm_group_render_sphere_lights", "ILM_ERR_INVALID_ARGUMENT", "ILM_ERR_INVALID_HANDLE"):
        assert word in contract, word
    for call in ("sphere", "particle", "directional", "line", "projector", "volumetric"):
        assert "ilm_render_%s_lights" % call in contract, call


def test_a_pixel_no_light_contributes_to_keeps_its_base_under_every_function():
    base = image((0.25, -3.0, np.inf, 7.0), (np.nan, -np.inf, -0.0, 0.0))
    nothing = [np.zeros_like(base), np.zeros_like(base)]                       # alpha 0: the pairs do not contribute
    for f in lb.FUNCTIONS:
        for g in lb.FUNCTIONS:
            out = lb.combine_fp32(base, nothing, f, g)
            assert np.array_equal(out, base, equal_nan=True), (f, g)
            # MAX / MIN select: the very bits (base + 0 and base - 0 turn a -0 base into +0, as the addition always did)
            for ch, fn in enumerate(lb.channel_functions(f, g)):
                if fn in (MAX, MIN):
                    assert np.array_equal(out[..., ch].view(np.uint32), base[..., ch].view(np.uint32)), (f, g, ch)
    halves = image((0.25, -3.0, 2.0, 7.0))
    for f in lb.FUNCTIONS:
        assert np.array_equal(lb.combine_fp16(halves, [np.zeros_like(halves)] * 2, f, f), halves)


def test_min_takes_a_contributing_zero_and_not_a_pair_that_does_not_contribute():
    base = image((0.5, 0.5, 0.5, 4.0), (0.5, 0.5, 0.5, 4.0))
    # pixel 0: light A contributes (0, 0.75, 0.25); pixel 1: it does not -- its zeros are no source value
    a = image((0.0, 0.75, 0.25, 1.0), (0.0, 0.0, 0.0, 0.0))
    b = image((0.125, 0.125, 0.125, 1.0), (0.125, 0.875, 0.125, 1.0))
    out = lb.combine_fp32(base, [a, b], MIN, MIN)
    assert out[0, 0].tolist() == [0.0, 0.125, 0.125, 1.0]
    assert out[0, 1].tolist() == [0.125, 0.5, 0.125, 1.0]
    out = lb.combine_fp32(base, [a, b], MAX, lb.ADD)
    assert out[0, 0].tolist() == [0.5, 0.75, 0.5, 6.0] and out[0, 1].tolist() == [0.5, 0.875, 0.5, 5.0]
    # the order of the lights does not matter to MAX / MIN
    for f in (MAX, MIN):
        assert np.array_equal(lb.combine_fp32(base, [a, b], f, f), lb.combine_fp32(base, [b, a], f, f))


def test_a_nan_source_is_ignored_and_a_nan_base_is_kept():
    base = image((0.5, np.nan, 0.5, 1.0))
    a = image((np.nan, 0.25, 0.75, 1.0))
    b = image((0.25, 0.25, np.nan, 1.0))
    mx = lb.combine_fp32(base, [a, b], MAX, MAX)
    mn = lb.combine_fp32(base, [a, b], MIN, MIN)
    assert mx[0, 0, 0] == 0.5 and np.isnan(mx[0, 0, 1]) and mx[0, 0, 2] == 0.75 and mx[0, 0, 3] == 1.0
    assert mn[0, 0, 0] == 0.25 and np.isnan(mn[0, 0, 1]) and mn[0, 0, 2] == 0.5 and mn[0, 0, 3] == 1.0
    h = lb.combine_fp16(image((0.5, 0.5, 0.5, 1.0)), [a, b], MAX, MAX)
    assert h[0, 0].tolist() == [0.5, 0.5, 0.75, 1.0]


def test_reverse_subtract_is_one_subtraction_and_ends_at_byte_zero():
    base = image((0.75, 0.25, 1.0, 3.0))
    a = image((0.5, 0.5, 0.1, 1.0))
    b = image((0.125, 0.25, 0.2, 1.0))
    out = lb.combine_fp32(base, [a, b], RSUB, RSUB)
    s = F(F(0.1) + F(0.2))
    assert out[0, 0].tolist() == [0.125, -0.5, float(F(F(1.0) - s)), 1.0]
    assert lb.to_stored(out, abi.LIGHTMAP_RGBA8)[0, 0].tolist() == [32, 0, int(np.rint(F(F(1.0) - s) * F(255))), 255]
    assert lb.to_stored(out, abi.LIGHTMAP_HALF4)[0, 0, 1] == np.float16(-0.5)
    # S handed in (the device's own sum) is used as it is
    out = lb.combine_fp32(base, [a, b], RSUB, lb.ADD, total=image((0.25, 0.25, 0.25, 2.0)))
    assert out[0, 0].tolist() == [0.5, 0.0, 0.75, 5.0]


def test_the_fp16_chain_runs_in_list_order():
    base = image((2048.0, 1.0, 0.1, 1.0))
    one = image((1.0, 0.0004, 0.3, 1.0))
    big = image((-2048.0, 1.0, 0.3, 1.0))
    # 2048 + 1 is not an fp16 value (the spacing there is 2): half(2049) = 2048, then - 2048 = 0; the other order gives 0 + 1 = 1
    assert lb.combine_fp16(base, [one, big], ADD, ADD)[0, 0, 0] == 0.0
    assert lb.combine_fp16(base, [big, one], ADD, ADD)[0, 0, 0] == 1.0
    assert lb.combine_fp16(base, [one, big], RSUB, ADD)[0, 0, 0] == 4096.0        # half(2048 - 1) = 2047 (exact), + 2048 = 4095 -> 4096
    assert lb.combine_fp16(base, [one], RSUB, ADD)[0, 0, 0] == 2047.0
    # dst starts at half(base), every source passes through half: 0.1 and 0.3 are not fp16 values
    out = lb.combine_fp16(base, [one], MAX, MIN)
    assert out[0, 0, 2] == np.float32(np.float16(0.3)) and out[0, 0, 3] == 1.0
    out = lb.combine_fp16(base, [one], MIN, MAX)
    assert out[0, 0, 2] == np.float32(np.float16(0.1)) and out[0, 0, 1] == np.float32(np.float16(0.0004))
    # alpha counts in the chain under ADD and follows its own function otherwise
    assert lb.combine_fp16(base, [one, big], MAX, ADD)[0, 0, 3] == 3.0
    assert lb.combine_fp16(base, [one, big], ADD, RSUB)[0, 0, 3] == -1.0
