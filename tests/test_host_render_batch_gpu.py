"""Host mirror: ParticleEngine.RenderSystems -- the Render loop of Scenes/ManySystemsManySpawners.cs:78-81 as one
ilm_engine_render_particles_batch -- against calling each system's Render in order."""
import numpy as np
import pytest

from illuminant_amd import abi, scenes

pytestmark = pytest.mark.gpu


def make_system(H, engine, index, sheet):
    cfg = H.ParticleSystemConfiguration()
    cfg.LifeDecayPerSecond = 0.5
    cfg.Size = [4.0 + index, 3.0] if sheet is None else [1.0, 0.8]      # (RelativeSize: a textured sprite is Size x SizePx / 2)
    cfg.RotationFromLife = 90.0
    cfg.ZToY = 0.5
    col = H.ParticleColor(); col.Global = [0.9, 0.6 + 0.1 * index, 1.0, 0.7]
    cfg.Color = col
    ap = H.ParticleAppearance(); ap.Rounded = bool(index & 1)
    if sheet is not None:
        ap.TextureSize = [32.0, 16.0]; ap.SizePx = [8.0, 8.0]; ap.Bilinear = True; ap.AnimationRate = [0.5, 0.0]
    cfg.Appearance = ap
    ps = H.ParticleSystem(engine, cfg)
    if sheet is not None:
        ps.SetBitmap(sheet)
    sp = H.Spawner(11 + index)
    sp.MinRate = sp.MaxRate = 900.0
    f = H.Formula3(); f.Constant = [40 + 8 * index, 30, 2]; f.RandomScale = [45, 28, 2]; f.Type = H.FormulaType.Spherical
    sp.Position = f
    g = H.Formula3(); g.RandomScale = [30, 30, 0]; g.Type = H.FormulaType.Spherical
    sp.Velocity = g
    life = H.Formula1(); life.Constant = 2.0; life.RandomScale = 2.0
    sp.Life = life
    c4 = H.Formula4(); c4.Constant = [0.6, 0.5, 0.4, 0.5]; c4.RandomScale = [0.4, 0.5, 0.6, 0.5]
    sp.Color = c4
    ps.AddTransform(sp)
    return ps


def test_render_systems_equals_the_render_loop():
    from illuminant_amd import _host as H
    ctx = H.DeviceContext(0)
    tp = H.ManualTimeProvider()
    ecfg = H.ParticleEngineConfiguration(32)
    ecfg.TimeProvider = tp
    engine = H.ParticleEngine(ctx, ecfg, scenes.randomness_table(7))
    sheet = scenes.uniform(77, (16, 32, 4), 0.0, 1.0)
    systems = [make_system(H, engine, i, sheet if i == 2 else None) for i in range(4)]
    for frame in range(6):
        tp.Advance(1.0 / 60.0)
        engine.UpdateSystems(systems, frame)
    w, h = 120, 72
    clear = [0.02, 0.03, 0.04, 1.0]
    origin, scale, vscale, vpos = [4.0, -3.0], [1.0, 1.0], [1.0, 1.0], [2.0, 1.0]
    for blend in (abi.BLEND_ALPHA, abi.BLEND_ADDITIVE):
        loop, one = H.RenderTarget(ctx, w, h), H.RenderTarget(ctx, w, h)
        loop.Clear(clear); one.Clear(clear)
        total = [0, 0, 0]
        for ps in systems:
            total = [a + b for a, b in zip(total, ps.Render(loop, blend, origin, scale, vscale, vpos, True))]
        stats = engine.RenderSystems(systems, one, blend, origin, scale, vscale, vpos, True)
        assert tuple(stats) == tuple(total)
        assert stats[0] > 200 and 0 < stats[1] <= 2048          # no tile's run can exceed a segment: the bit-equal case
        got, want = np.asarray(one.Download()), np.asarray(loop.Download())
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
        assert (np.abs(got - np.asarray(clear, np.float32)).max(axis=-1) > 1e-3).mean() > 0.2
        # without stats the call is the same draw
        again = H.RenderTarget(ctx, w, h)
        again.Clear(clear)
        assert tuple(engine.RenderSystems(systems, again, blend, origin, scale, vscale, vpos)) == (0, 0, 0)
        assert np.asarray(again.Download()).tobytes() == want.tobytes()
    # an empty list draws nothing
    assert tuple(engine.RenderSystems([], one)) == (0, 0, 0)
