"""The streaming lean step comes in curve classes (csrc/particles.hip, kCurvesClamp; launch_lean_step selects per launch from
bezier_codes / update_bits).  Every instantiation must leave the bits the interpreting kernel leaves: each case runs the same script on a
system stepped by the default choice and on a twin stepped by the interpreter (ilm_debug_step_interpreter), several steps so that the
store elision is active, and compares all five planes of every chunk bit for bit and the live counts.  ilm_debug_last_step_kernel says
which kernel the default choice was, so each case also pins the side of the selector's boundary it was built for.
These systems are small, so ILM_STEP_STREAMING=1 selects the HBM-resident variant the classes belong to.
"""
import numpy as np
import pytest

from illuminant_amd import abi, native
from tests.test_step_store_elision_gpu import Twins, particles, step_desc, update_params, P, V, A

pytestmark = pytest.mark.gpu

# ILM_STEP_KERNEL_* of include/illuminant_hip.h
INTERPRETER, LEAN, LEAN_CLAMP = 1, 2, 3
REPEAT, MIRROR, SINE, SQUARE = 256, 512, 1, 2
CS = 64


@pytest.fixture(autouse=True)
def streaming_variant(monkeypatch):
    monkeypatch.setenv("ILM_STEP_STREAMING", "1")


def test_the_header_names_the_kernels():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "illuminant_hip.h")).read()
    defines = dict(re.findall(r"#define (ILM_STEP_KERNEL_\w+)\s+(\d+)", text))
    assert (int(defines["ILM_STEP_KERNEL_INTERPRETER"]), int(defines["ILM_STEP_KERNEL_LEAN"]), int(defines["ILM_STEP_KERNEL_LEAN_CLAMP"])) == \
        (INTERPRETER, LEAN, LEAN_CLAMP)


class KernelTwins(Twins):
    """Twins that also records which kernel each step of the first (default choice) system ran."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.kernels = []

    def step(self, d, n=1, lean_uses_interpreter=False):
        for _ in range(n):
            for i, s in enumerate(self.systems):
                native.lib().ilm_debug_step_interpreter(1 if (i == 1 or lean_uses_interpreter) else 0)
                s.step(d)
                if i == 0:
                    self.kernels.append(native.lib().ilm_debug_last_step_kernel())
                if d.Flags & abi.STEP_COUNT_LIVE:
                    self.counts[i].append(s.step_counts().copy())
        native.lib().ilm_debug_step_interpreter(0)


def run(ctx, d, what, expect, steps=5, life=(50.0, 90.0), ramp=None, n_chunks=3):
    """`steps` steps of `d` on both twins; the first step of a system stores everything through the general instantiation (no chunk is
    render-current yet), every later one must have run `expect`."""
    t = KernelTwins(ctx, CS, n_chunks, life=life)
    try:
        if ramp is not None:
            t.both(lambda s: s.set_life_ramp(ramp))
        t.step(d, steps)
        t.check(what)
        assert t.kernels[0] == (INTERPRETER if expect == INTERPRETER else LEAN), (what, t.kernels)
        assert t.kernels[1:] == [expect] * (steps - 1), (what, t.kernels)
    finally:
        t.close()


def curve4(count, mode=0, lo=0.0, inverse=1.0 / 80.0):
    return abi.ClampedBezier4(abi.f4(lo, inverse, count, mode), abi.f4(1.0, 0.2, 0.1, 1.0), abi.f4(0.4, 0.9, 0.3, 0.8),
                              abi.f4(0.1, 0.5, 1.0, 0.5), abi.f4(0.9, 0.1, 0.6, 0.2))


def curve1(count, mode=0, lo=0.0, inverse=1.0 / 80.0):
    return abi.ClampedBezier1(abi.f4(lo, inverse, count, mode), abi.f4(0.5, 2.0, 1.25, 3.0))


# ---- inside the class ----------------------------------------------------------------------------------------------------------

CLAMP_CASES = {
    "bench curves": dict(),
    "every curve constant": dict(ColorFromLife=abi.UpdateParams.default().ColorFromLife),
    "four clamp curves, counts 2 3 4 2": dict(ColorFromLife=curve4(2), ColorFromVelocity=curve4(3, lo=5.0, inverse=1.0 / 60.0),
                                              SizeFromLife=curve1(4), SizeFromVelocity=curve1(2, inverse=1.0 / 120.0)),
    "negative inverse divisors": dict(ColorFromLife=curve4(4, inverse=-1.0 / 80.0), ColorFromVelocity=curve4(2, inverse=-1.0 / 90.0),
                                      SizeFromLife=curve1(3, inverse=-1.0 / 70.0), SizeFromVelocity=curve1(4, lo=3.0, inverse=-1.0 / 100.0)),
    # a constant curve reads neither its range nor its other points, whatever they hold
    "constant curves with negative divisors and infinite points": dict(
        SizeFromLife=abi.ClampedBezier1(abi.f4(0.0, -1.0 / 70.0, 1, 0), abi.f4(0.5, float("inf"), float("nan"), -float("inf"))),
        SizeFromVelocity=abi.ClampedBezier1(abi.f4(2.0, -1.0 / 9.0, 1, 0), abi.f4(1.5, float("-inf"), 2.0, float("nan"))),
        ColorFromVelocity=abi.ClampedBezier4(abi.f4(1.0, -1.0 / 50.0, 1, 0), abi.f4(1.0, 0.5, 0.25, 1.0), abi.f4(*[float("inf")] * 4),
                                             abi.f4(*[float("nan")] * 4), abi.f4(0.9, 0.1, 0.6, 0.2))),
    "rotation from life and index": dict(rotation_from_life=0.25, rotation_from_index=0.001, SizeFromVelocity=curve1(2)),
}


@pytest.mark.parametrize("name", list(CLAMP_CASES))
def test_clamp_class_matches_the_interpreter(ctx, name):
    run(ctx, step_desc(CS, update=update_params(**CLAMP_CASES[name])), name, LEAN_CLAMP, steps=6)


@pytest.mark.parametrize("ops", [("gravity", "noise"), ("fma", "gravity"), ("noise", "fma", "gravity", "gravity"), ()],
                         ids=["gravity noise", "fma gravity", "four transforms", "no transform"])
def test_clamp_class_with_every_transform_position(ctx, ops):
    """The class dispatches its transforms from unrolled positions: every count from none to ILM_MAX_OPS, each kind in more than one place."""
    run(ctx, step_desc(CS, ops=ops, update=update_params(SizeFromLife=curve1(2))), "ops %s" % (ops,), LEAN_CLAMP)


def test_a_spawning_step_takes_the_general_instantiation(ctx):
    """The class has no spawning instantiation: a launch with spawn records runs the general one, whatever its curves are."""
    d = step_desc(CS, life_decay=2.0, spawns=((2, 100, 1500), (0, 4000, 4095)), update=update_params(ColorFromVelocity=curve4(2)))
    run(ctx, d, "spawning", LEAN, steps=6, life=(0.01, 3.0))


def test_clamp_class_dying_reviving_and_nan_lanes(ctx):
    """Lives that cross OpacityFromLife and zero inside a wave next to NaN / infinite lives, velocities and categories (the particles of
    tests/test_step_store_elision_gpu.py), a reviving Noise in between (an interpreter step), then spawns over the dead slots (steps of
    the general instantiation) with class steps after them."""
    t = KernelTwins(ctx, CS, 3, life=(0.01, 3.0))
    try:
        curves = update_params(SizeFromLife=curve1(4, inverse=1.0 / 2.5), ColorFromVelocity=curve4(3, inverse=1.0 / 120.0), rotation_from_life=0.7)
        dying = step_desc(CS, life_decay=30.0, update=curves)
        t.step(dying, 4)
        t.check("dying")
        assert t.kernels[1:] == [LEAN_CLAMP] * 3, t.kernels
        t.step(step_desc(CS, life_decay=30.0, revive=True, update=curves), 1)
        assert t.kernels[-1] == INTERPRETER, t.kernels
        t.step(dying, 3)
        t.check("after a reviving Noise")
        assert t.kernels[-2:] == [LEAN_CLAMP] * 2, t.kernels
        t.step(step_desc(CS, life_decay=2.0, spawns=((1, 0, 4095), (0, 700, 900)), update=curves), 3)
        t.check("spawned over")
        assert t.kernels[-3:] == [LEAN] * 3, t.kernels
        t.step(dying, 3)
        t.check("dying again after the spawns")
        assert t.kernels[-3:] == [LEAN_CLAMP] * 3, t.kernels
        # a whole wave of NaN lives and one of NaN velocities, written into render-current chunks
        pos, vel, attr = particles(7, t.n, life=(1.0, 60.0), specials=False)
        pos[128:192, 3] = np.nan
        vel[256:320, :3] = np.nan
        vel[320:330, 0] = np.inf
        t.both(lambda s: (s.upload(2, P, pos), s.upload(2, V, vel), s.upload(2, A, attr)))
        t.step(dying, 4)
        t.check("NaN waves")
        assert t.kernels[-3:] == [LEAN_CLAMP] * 3, t.kernels
    finally:
        t.close()


# ---- on the other side of each boundary: the general instantiation (or the interpreter) ----------------------------------------------

def _on_curve(name, mode):
    make = curve4 if name.startswith("Color") else curve1
    return {name: make(3 if name.endswith("Life") else 2, mode)}


GENERAL_CASES = {}
for _curve in ("ColorFromLife", "ColorFromVelocity", "SizeFromLife", "SizeFromVelocity"):
    GENERAL_CASES["repeat range on %s" % _curve] = _on_curve(_curve, REPEAT)
    GENERAL_CASES["mirror range on %s" % _curve] = _on_curve(_curve, MIRROR)
GENERAL_CASES["sine shaping"] = dict(ColorFromLife=curve4(2, SINE), SizeFromVelocity=curve1(4, SINE))
GENERAL_CASES["square shaping"] = dict(SizeFromLife=curve1(2, SQUARE), ColorFromVelocity=curve4(4, SQUARE))
GENERAL_CASES["mirror range with sine shaping, negative divisor"] = dict(SizeFromLife=curve1(4, MIRROR + SINE, inverse=-1.0 / 30.0))


@pytest.mark.parametrize("name", list(GENERAL_CASES))
def test_curves_outside_the_class_take_the_general_instantiation(ctx, name):
    run(ctx, step_desc(CS, update=update_params(**GENERAL_CASES[name])), name, LEAN)


def test_velocity_rotation_takes_the_general_instantiation(ctx):
    run(ctx, step_desc(CS, rotation=True, update=update_params(SizeFromLife=curve1(2))), "rotation from velocity", LEAN)


def test_cache_resident_steps_take_the_general_instantiation(ctx, monkeypatch):
    monkeypatch.setenv("ILM_STEP_STREAMING", "0")
    run(ctx, step_desc(CS), "cache-resident", LEAN)


def test_a_life_ramp_stays_with_the_interpreter(ctx):
    """build_lean_step sends a life ramp to the interpreting kernel; the default choice and the forced interpreter agree."""
    rng = np.random.default_rng(3)
    ramp = rng.uniform(0.0, 1.0, (4, 16, 4)).astype(np.float32)
    u = update_params()
    u.LifeRampSettings = abi.f4(-0.7, 0.5, 80.0, 8.0)
    run(ctx, step_desc(CS, update=u), "life ramp", INTERPRETER, ramp=ramp)
