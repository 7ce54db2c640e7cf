"""ilm_resolve_lighting_lut on the device against its numpy statement (tests/resolve_lut_common.py, itself checked by hand in
tests/test_resolve_lut_kat.py) under the project's float criterion (tests/util.assert_close's defaults; +-1 byte and the exact band for an
RGBA8 destination, tests/output_common.check_destination).  Shapes are a few dozen pixels: every branch of the kernel is launch-uniform,
so what a shape can change is the span loop (1061 pixels: one full span of 1024 and a ragged one) and the fetch."""
import numpy as np
import pytest

from illuminant_amd import abi, native
from tests import output_common as oc
from tests import resolve_lut_common as rl
from tests import resolve_scaled_common as rs
from tests.util import assert_close

pytestmark = pytest.mark.gpu

F = np.float32
F4, H4, C8 = abi.LIGHTMAP_FLOAT4, abi.LIGHTMAP_HALF4, abi.LIGHTMAP_RGBA8
_DTYPE = {F4: np.float32, H4: np.float16, C8: np.uint8}


def _encode(values, fmt):
    """float32 texels in [0, 1] as a texture of the format holds them"""
    if fmt == C8:
        return np.rint(np.clip(values, 0.0, 1.0) * 255.0).astype(np.uint8)
    return np.asarray(values).astype(_DTYPE[fmt])


def _texture(ctx, texels, fmt):
    t = native.Lightmap(ctx, texels.shape[1], texels.shape[0], fmt)
    t.upload(np.ascontiguousarray(texels))
    return t


def _sentinel(fmt, size):
    return np.full((size[1], size[0], 4), oc.SENTINEL[fmt])


def _close(*textures):
    for t in textures:
        if t is not None:
            t.close()


def _random_lut(n, rows, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n * rows, n * n, 4)).astype(np.float32)


def _constant_lut(n, value, rows=1):
    return np.full((n * rows, n * n, 4), value, np.float32)


class Case:
    """The textures of one call on the device beside their decoded arrays; run() resolves and returns (device, statement, covered)."""

    def __init__(self, ctx, light, albedo, dark, bright, light_fmt=F4, albedo_fmt=F4, lut_fmt=F4, dark_n=None, bright_n=None):
        self.ctx = ctx
        self.light_t, self.albedo_t = _encode(light, light_fmt), _encode(albedo, albedo_fmt)
        dark_t, bright_t = _encode(dark, lut_fmt), _encode(bright, lut_fmt)
        self.light, self.albedo = oc.decode(self.light_t, light_fmt), oc.decode(self.albedo_t, albedo_fmt)
        self.dark, self.bright = oc.decode(dark_t, lut_fmt), oc.decode(bright_t, lut_fmt)
        self.src, self.tex = _texture(ctx, self.light_t, light_fmt), _texture(ctx, self.albedo_t, albedo_fmt)
        self.dark_tex, self.bright_tex = _texture(ctx, dark_t, lut_fmt), _texture(ctx, bright_t, lut_fmt)
        self.dark_n, self.bright_n = dark_n, bright_n

    def blending(self, dark_level, bright_level, neutral_band_size=0.0, per_channel=False, lut_only=False, dark_row=0, bright_row=0):
        device = native.lut_blending(self.dark_tex, self.bright_tex, dark_level, bright_level, neutral_band_size, per_channel, lut_only, dark_row,
                                     bright_row, self.dark_n, self.bright_n)
        statement = rl.Blending(self.dark, self.bright, dark_level, bright_level, neutral_band_size, per_channel, lut_only, self.dark_n,
                                self.bright_n, dark_row, bright_row)
        return device, statement

    def run(self, dst, blending, hdr, quad, lightmap_region=None, albedo_region=None, uv_offset=None, lightmap_filter=rs.LINEAR,
            albedo_filter=rs.LINEAR, row_begin=0, row_end=None):
        device, statement = blending
        native.resolve_lighting_lut(self.src, dst, hdr, device, quad, self.tex, lightmap_region, albedo_region, uv_offset, lightmap_filter,
                                    albedo_filter, row_begin, row_end)
        size = (dst.width, dst.height)
        want = rl.resolve(self.light, self.albedo, size, quad, statement, hdr, lightmap_region, albedo_region, uv_offset, lightmap_filter, albedo_filter)
        return dst.download(), want, rs.coverage(size, quad, row_begin, row_end)

    def target(self, size, fmt=F4):
        dst = native.Lightmap(self.ctx, size[0], size[1], fmt)
        dst.upload(_sentinel(fmt, size))
        return dst

    def close(self):
        _close(self.src, self.tex, self.dark_tex, self.bright_tex)


HDR = oc.hdr_configuration(abi.HDR_NONE, 0.75, 0.02, 1.3, 0.9)
PLAIN = oc.hdr_configuration(abi.HDR_NONE, 0.5)             # light = the tap itself, no offset, exposure and gamma 1


# ---- the weight: constant LUTs ------------------------------------------------------------------------------------------------------------
LEVELS = (0.0, 0.1, 0.2, 0.25, 0.3, 0.34, 0.375, 0.45, 0.5, 0.55, 0.625, 0.66, 0.7, 0.75, 0.8, 1.0, 2.5)
WEIGHT_PATHS = {                                             # dark level, bright level, neutral band size, per channel
    "band": (0.25, 0.75, 0.25, False),
    "band_overrides_per_channel": (0.25, 0.75, 0.25, True),
    "ramp_luminance": (0.25, 0.75, 0.0, False),
    "ramp_per_channel": (0.25, 0.75, 0.0, True),
    "hack_luminance": (0.5, 0.5, 0.0, False),
    "hack_per_channel": (0.5, 0.25, 0.0, True),
}


@pytest.fixture(scope="module")
def weight_case(ctx):
    """17 x 17 texels: red runs through LEVELS along x, green along y, blue through them at another pace; grey on the diagonal."""
    n = len(LEVELS)
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    light = np.ones((n, n, 4), np.float32)
    v = np.array(LEVELS, np.float32)
    light[..., 0], light[..., 1], light[..., 2] = v[i], v[j], v[(2 * i + 3 * j) % n]
    albedo = np.random.default_rng(3).uniform(0.0, 1.0, (n, n, 4)).astype(np.float32)
    case = Case(ctx, light, albedo, _constant_lut(2, 0.25), _constant_lut(2, 0.75))
    yield case
    case.close()


@pytest.mark.parametrize("lut_only", (True, False), ids=("lut_only", "times_light"))
@pytest.mark.parametrize("path", sorted(WEIGHT_PATHS))
def test_constant_luts_show_the_weight_of_every_path_and_zone(weight_case, path, lut_only):
    """Dark LUT 0.25, bright LUT 0.75: the result reads the weight directly.  The lightmap lands below, inside and above every zone."""
    dark_level, bright_level, neutral, per_channel = WEIGHT_PATHS[path]
    n = len(LEVELS)
    u = rl.uniforms(dark_level, neutral, bright_level, per_channel)
    w = rl.weight(weight_case.light[..., :3], u["normalize"])
    if u["has_band"]:                                      # the five zones of the band: dark, rising, albedo, rising, bright
        v = w[..., 0] - F(dark_level)
        edges = np.cumsum([0.0, u["transition"], u["neutral"], u["transition"]])
        zones = np.searchsorted(edges, v, side="right")
        assert set(zones.ravel()) == {0, 1, 2, 3, 4}
    else:                                                  # below, inside and above the ramp, in every channel that has a weight of its own
        top = F(bright_level) if u["ramp"] else F(dark_level) + F(1.0)
        for k in range(3):
            assert (w[..., k] < dark_level).any() and ((w[..., k] > dark_level) & (w[..., k] < top)).any() and (w[..., k] > top).any()
    assert u["normalize"] or not np.array_equal(w[..., 0], w[..., 1])
    dst = weight_case.target((n, n))
    blending = weight_case.blending(dark_level, bright_level, neutral, per_channel, lut_only)
    for hdr in (PLAIN, HDR):
        got, want, covered = weight_case.run(dst, blending, hdr, (0, 0, n, n))
        assert covered.all()
        oc.check_destination(got, want, F4, "%s %s" % (path, "lut only" if lut_only else "times light"))
    if lut_only and not u["has_band"]:                     # read directly: 0.25 + 0.5 w, all of [0.25, 0.75] and nothing else
        got, want, _ = weight_case.run(dst, blending, PLAIN, (0, 0, n, n))
        assert abs(got[..., :3].min() - 0.25) <= 1e-5 and abs(got[..., :3].max() - 0.75) <= 1e-5
    assert np.array_equal(got[..., 3], weight_case.albedo[..., 3])
    dst.close()


# ---- tap selection ----------------------------------------------------------------------------------------------------------------------
def _code_lut(n, rows=1):
    """Texel (ri, gi, bi) of every row holds (ri, gi, bi) / 8 + row / 64 in rgb: its own address"""
    lut = np.zeros((n * rows, n * n, 4), np.float32)
    for row in range(rows):
        for g in range(n):
            for b in range(n):
                for r in range(n):
                    lut[row * n + g, b * n + r, :3] = (r / 8.0 + row / 64.0, g / 8.0 + row / 64.0, b / 8.0 + row / 64.0)
    return lut


def test_lattice_points_midpoints_zero_and_one_pick_the_texels_the_definition_names(ctx):
    """N = 5 LUTs whose texels hold their own (ri, gi, bi); a 27 x 27 albedo of every combination of the five lattice points (0 and 1 among
    them) and the four midpoints.  DarkLevel beyond every light: the result is the dark LUT's value alone."""
    values = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 0.125, 0.375, 0.625, 0.875], np.float32)
    idx = np.arange(729).reshape(27, 27)
    albedo = np.ones((27, 27, 4), np.float32)
    albedo[..., 0], albedo[..., 1], albedo[..., 2] = values[idx % 9], values[(idx // 9) % 9], values[idx // 81]
    light = np.random.default_rng(5).uniform(0.0, 2.0, (27, 27, 4)).astype(np.float32)
    case = Case(ctx, light, albedo, _code_lut(5), _constant_lut(5, 1.0))
    dst = case.target((27, 27))
    got, want, _ = case.run(dst, case.blending(100.0, 101.0, lut_only=True), PLAIN, (0, 0, 27, 27), lightmap_filter=rs.POINT, albedo_filter=rs.POINT)
    oc.check_destination(got, want, F4, "tap selection")
    # read directly: the value is the albedo's position in the lattice, a / 0.25 / 8 = a / 2 -- at lattice points the texel itself
    assert_close(got[..., :3], albedo[..., :3] * F(0.5), "the lattice address")
    on_lattice = (idx % 9 < 5) & ((idx // 9) % 9 < 5) & (idx // 81 < 5)
    assert np.array_equal(np.rint(got[on_lattice][:, :3] * 8.0), np.rint(albedo[on_lattice][:, :3] * 4.0))
    _close(dst)
    case.close()


def test_slices_and_rows_do_not_bleed(ctx):
    """Two rows of N = 5.  Row 0 is read at the far edge of slice and row (albedo r = g = 1): only texels with ri = gi = 4 hold 1, so the
    first column of the next slice and the first texel row of row 1 hold 0 -- a tap from either would pull the result below 1.  Row 1 at the
    near edge (r = g = 0): only ri = gi = 0 hold 1, the last column of the previous slice and the last texel row of row 0 hold 0."""
    n = 5
    far, near = np.zeros((2 * n, n * n, 4), np.float32), np.zeros((2 * n, n * n, 4), np.float32)
    far[n - 1, n - 1::n, :3] = 1.0                        # row 0, gi = 4, ri = 4 of every slice
    near[n, 0::n, :3] = 1.0                               # row 1, gi = 0, ri = 0 of every slice
    blues = np.array([0.0, 0.1, 0.25, 0.6, 0.75, 0.99, 1.0], np.float32)
    albedo_far, albedo_near = np.ones((1, 7, 4), np.float32), np.zeros((1, 7, 4), np.float32)
    albedo_far[0, :, 2], albedo_near[0, :, 2] = blues, blues
    light = np.full((1, 7, 4), 0.5, np.float32)
    for lut, albedo, row in ((far, albedo_far, 0), (near, albedo_near, 1)):
        case = Case(ctx, light, albedo, lut, lut, dark_n=n, bright_n=n)
        dst = case.target((7, 1))
        got, want, _ = case.run(dst, case.blending(0.25, 0.75, 0.0, lut_only=True, dark_row=row, bright_row=row), PLAIN, (0, 0, 7, 1))
        rows, cols = rl.lut_taps(n, row, case.albedo[..., :3])
        assert (rows // n == row).all() and (cols % n == (n - 1 if row == 0 else 0))[..., 0::2].all()       # the definition's taps stay in the row
        assert row == 1 or (lut[rows, cols, 0] == 1.0).all()                  # at the far edge both taps of an axis are the last texel
        oc.check_destination(got, want, F4, "row %d" % row)
        assert np.abs(got[..., :3] - 1.0).max() <= 1e-6, got[..., :3]
        _close(dst)
        case.close()


# ---- resolutions, rows, formats -----------------------------------------------------------------------------------------------------------
LUT_SHAPES = {                                              # dark (n, rows, row), bright (n, rows, row)
    "2_and_2": ((2, 1, 0), (2, 1, 0)),
    "5_and_17": ((5, 1, 0), (17, 1, 0)),
    "rows_1_of_2_and_0_of_2": ((5, 2, 1), (5, 2, 0)),
    "17_row_2_of_3_and_2": ((17, 3, 2), (2, 1, 0)),
}


@pytest.mark.parametrize("lut_fmt", (C8, H4, F4), ids=lambda f: "lut_" + oc.FORMAT_NAME[f])
@pytest.mark.parametrize("shape", sorted(LUT_SHAPES))
def test_resolutions_rows_and_formats(ctx, shape, lut_fmt):
    """Random LUTs of unequal resolutions and row counts in every format, a HALF4 lightmap (19 x 13) and an RGBA8 albedo (23 x 17) onto a
    37 x 29 target, float and Color; band and LUTOnly off -- the usual call."""
    (dn, drows, drow), (bn, brows, brow) = LUT_SHAPES[shape]
    rng = np.random.default_rng(17)
    light = rng.uniform(0.0, 1.2, (13, 19, 4)).astype(np.float32)
    albedo = rng.uniform(0.0, 1.0, (17, 23, 4)).astype(np.float32)
    case = Case(ctx, light, albedo, _random_lut(dn, drows, 1), _random_lut(bn, brows, 2), H4, C8, lut_fmt, dn, bn)
    blending = case.blending(0.2, 0.9, 0.3, dark_row=drow, bright_row=brow)
    for dst_fmt in (F4, C8):
        dst = case.target((37, 29), dst_fmt)
        got, want, covered = case.run(dst, blending, HDR, (0, 0, 37, 29))
        assert covered.all()
        oc.check_destination(got, want, dst_fmt, "%s %s -> %s" % (shape, oc.FORMAT_NAME[lut_fmt], oc.FORMAT_NAME[dst_fmt]))
        _close(dst)
    case.close()


def test_identity_luts_give_the_with_albedo_resolve(ctx):
    """Dark and bright LUT both the identity (N = 17, float): the blend is the albedo, whatever the weight, and blended * light is what
    ilm_resolve_lighting_scaled computes from the same textures when saturate(light.a) = 1 and the albedo lies in [0, 1]."""
    n = 17
    identity = np.zeros((n, n * n, 4), np.float32)
    g, bi, r = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    identity[g, bi * n + r, 0], identity[g, bi * n + r, 1], identity[g, bi * n + r, 2] = r / F(16.0), g / F(16.0), bi / F(16.0)
    rng = np.random.default_rng(23)
    light = rng.uniform(0.0, 2.0, (13, 19, 4)).astype(np.float32)
    light[..., 3] = 1.0                                   # * (0.75 * 2) saturates to 1
    albedo = rng.uniform(0.0, 1.0, (17, 23, 4)).astype(np.float32)
    case = Case(ctx, light, albedo, identity, identity, H4, F4, F4)
    dst, ref = case.target((37, 29)), case.target((37, 29))
    for blending in (case.blending(0.2, 0.9, 0.3), case.blending(0.3, 0.6, 0.0, per_channel=True)):
        got, want, _ = case.run(dst, blending, HDR, (0, 0, 37, 29))
        oc.check_destination(got, want, F4, "identity against the statement")
        native.resolve_lighting_scaled(case.src, ref, HDR, (0, 0, 37, 29), albedo=case.tex)
        assert_close(got, ref.download(), "identity against ilm_resolve_lighting_scaled")
    _close(dst, ref)
    case.close()


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------
GEOMETRY = {      # target size, quad, lightmap filter, albedo filter, uv offset
    "37x5_linear": ((37, 5), (0, 0, 37, 5), rs.LINEAR, rs.LINEAR, None),
    "37x5_point": ((37, 5), (0, 0, 37, 5), rs.POINT, rs.POINT, None),
    "1061x3_a_full_span_and_a_ragged_one": ((1061, 3), (0, 0, 1061, 3), rs.LINEAR, rs.POINT, None),
    "partial_quad": ((37, 5), (-3.5, 1.25, 30.0, 3.0), rs.LINEAR, rs.LINEAR, None),
    "uv_offset": ((37, 5), (0, 0, 37, 5), rs.LINEAR, rs.LINEAR, (0.5, -0.25)),
    "uv_offset_nan_inf": ((37, 5), (0, 0, 37, 5), rs.POINT, rs.LINEAR, (float("nan"), float("inf"))),
}


@pytest.fixture(scope="module")
def geometry_case(ctx):
    rng = np.random.default_rng(29)
    light = rng.uniform(0.0, 1.2, (4, 8, 4)).astype(np.float32)
    albedo = rng.uniform(0.0, 1.0, (3, 11, 4)).astype(np.float32)
    case = Case(ctx, light, albedo, _random_lut(5, 1, 3), _random_lut(5, 1, 4), H4, C8, C8)
    yield case
    case.close()


@pytest.mark.parametrize("dst_fmt", (F4, C8), ids=lambda f: "to_" + oc.FORMAT_NAME[f])
@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_fetch_coverage_and_strips_are_the_scaled_resolves(geometry_case, name, dst_fmt):
    """An 8 x 4 lightmap and an 11 x 3 albedo onto the target: covered pixels match the statement, every other texel keeps its bits, and a
    call split into two row strips leaves the bits of the whole call."""
    size, quad, lf, af, offset = GEOMETRY[name]
    case = geometry_case
    blending = case.blending(0.2, 0.9, 0.3)
    fill = _sentinel(dst_fmt, size)
    dst = case.target(size, dst_fmt)
    got, want, covered = case.run(dst, blending, HDR, quad, uv_offset=offset, lightmap_filter=lf, albedo_filter=af)
    assert covered.any() and (covered.all() or name == "partial_quad")
    assert np.array_equal(got[~covered], fill[~covered]), "a texel outside the quad was written"
    oc.check_destination(got[covered], want[covered], dst_fmt, name)
    strips = case.target(size, dst_fmt)
    split = size[1] // 2 + 1
    case.run(strips, blending, HDR, quad, uv_offset=offset, lightmap_filter=lf, albedo_filter=af, row_begin=0, row_end=split)
    half = strips.download()
    assert np.array_equal(half[split:], fill[split:]) and half[:split].tobytes() == got[:split].tobytes()
    case.run(strips, blending, HDR, quad, uv_offset=offset, lightmap_filter=lf, albedo_filter=af, row_begin=split, row_end=size[1])
    assert strips.download().tobytes() == got.tobytes()
    _close(dst, strips)


def test_regions_smaller_than_their_textures(geometry_case):
    case = geometry_case
    dst = case.target((37, 5))
    got, want, covered = case.run(dst, case.blending(0.2, 0.9, 0.3), HDR, (0, 0, 37, 5), lightmap_region=(1, 1, 7, 3.5), albedo_region=(2.5, 0, 9, 2))
    oc.check_destination(got[covered], want[covered], F4, "regions")
    _close(dst)


# ---- non-finite input ---------------------------------------------------------------------------------------------------------------------
def test_non_finite_albedo_and_light_stay_inside_the_luts(ctx):
    """A float albedo holding NaN, -1, 2 and +-inf is saturated before it becomes an index (NaN -> 0); an infinite light saturates the
    weight.  Nothing faults, and the device matches the statement wherever that is finite."""
    nan, inf = float("nan"), float("inf")
    odd = np.array([nan, -1.0, 2.0, inf, -inf, 0.5, 0.0, 1.0], np.float32)
    idx = np.arange(64).reshape(8, 8)
    albedo = np.ones((8, 8, 4), np.float32)
    albedo[..., 0], albedo[..., 1], albedo[..., 2] = odd[idx % 8], odd[idx // 8], odd[(idx + idx // 8) % 8]
    light = np.random.default_rng(31).uniform(0.0, 1.2, (8, 8, 4)).astype(np.float32)
    light[idx % 5 == 0, 0] = inf
    light[idx % 7 == 0, :3] = inf
    case = Case(ctx, light, albedo, _random_lut(5, 1, 5), _random_lut(17, 1, 6))
    dst = case.target((8, 8))
    for blending in (case.blending(0.2, 0.9, 0.3), case.blending(0.2, 0.9, 0.0, per_channel=True), case.blending(0.2, 0.9, 0.3, lut_only=True)):
        got, want, _ = case.run(dst, blending, HDR, (0, 0, 8, 8), lightmap_filter=rs.POINT, albedo_filter=rs.POINT)
        finite = np.isfinite(want[..., :3])
        assert finite.mean() > 0.5
        assert_close(np.where(finite, got[..., :3], 0.0), np.where(finite, want[..., :3], 0.0), "where the statement is finite")
    # with LUTOnly an infinite light never reaches the colour: everything is finite
    assert np.isfinite(got[..., :3]).all()
    _close(dst)
    case.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_destination_untouched(ctx):
    size = (12, 9)
    rng = np.random.default_rng(37)
    case = Case(ctx, rng.uniform(0, 1, (6, 8, 4)).astype(np.float32), rng.uniform(0, 1, (7, 10, 4)).astype(np.float32),
                _random_lut(5, 2, 7), _random_lut(2, 1, 8), H4, C8, C8, 5, 2)
    dst = case.target(size)
    fill = _sentinel(F4, size)
    bad, nan, inf = abi.ERR_INVALID_ARGUMENT, float("nan"), float("inf")

    def refused(code, words=None, lut=None, **changes):
        a = dict(quad=(0, 0, 12, 9), hdr=oc.hdr_configuration(), albedo=case.tex, src=case.src, dst=dst)
        a.update(changes)
        device = native.lut_blending(case.dark_tex, case.bright_tex, 0.25, 0.75, 0.1, dark_resolution=5, bright_resolution=2)
        for k, v in (lut or {}).items():
            setattr(device, k, v)
        with pytest.raises(native.IlluminantError) as e:
            native.resolve_lighting_lut(a.pop("src"), a.pop("dst"), a.pop("hdr"), device, a.pop("quad"), a.pop("albedo"), **a)
        assert e.value.code == code, (changes, lut, str(e.value))
        assert words is None or words in str(e.value), str(e.value)
        assert np.array_equal(dst.download(), fill), (changes, lut)

    # the call these refusals vary is accepted
    native.resolve_lighting_lut(case.src, dst, oc.hdr_configuration(), native.lut_blending(case.dark_tex, case.bright_tex, 0.25, 0.75, 0.1), (0, 0, 12, 9), case.tex)
    assert (dst.download() != fill).any()
    dst.upload(fill)
    refused(bad, "albedo", albedo=None)
    for mode in (abi.HDR_GAMMA_COMPRESS, abi.HDR_TONE_MAP):
        refused(bad, "LUT blending is not compatible with this type of lighting resolve", hdr=oc.matrix_hdr(mode))
    refused(abi.ERR_INVALID_HANDLE, lut=dict(DarkLUT=0))
    refused(abi.ERR_INVALID_HANDLE, lut=dict(BrightLUT=123456789))
    refused(bad, "resolution", lut=dict(BrightResolution=1, BrightRowCount=4))
    refused(bad, "resolution", lut=dict(DarkResolution=0))
    refused(bad, "row count", lut=dict(DarkRowCount=0))
    refused(bad, "texture", lut=dict(DarkResolution=4))                            # 25 x 10 is not 16 x 8
    refused(bad, "texture", lut=dict(DarkRowCount=3))
    refused(bad, "texture", lut=dict(BrightResolution=5, BrightRowCount=2))        # the bright texture is 4 x 2
    refused(bad, "row", lut=dict(DarkRow=2))
    refused(bad, "row", lut=dict(DarkRow=-1))
    refused(bad, "row", lut=dict(BrightRow=1))
    for field in ("DarkLevel", "NeutralBandSize", "BrightLevel"):
        for value in (nan, inf, -inf):
            refused(bad, "finite", lut={field: value})
    # everything the scaled entry point refuses
    for quad in ((0, 0, -1, 9), (0, 0, nan, 9), (nan, 0, 12, 9), (0, inf, 12, 9)):
        refused(bad, quad=quad)
    for region in ((0, 0, 9, 6), (-1, 0, 8, 6), (5, 0, 4, 6), (0, 0, nan, 6)):
        refused(bad, lightmap_region=region)
    for region in ((0, 0, 11, 7), (0, -0.5, 10, 7), (0, 0, 10, nan)):
        refused(bad, albedo_region=region)
    refused(bad, lightmap_filter=2)
    refused(bad, albedo_filter=-1)
    refused(abi.ERR_OUT_OF_RANGE, row_end=10)
    refused(abi.ERR_OUT_OF_RANGE, row_begin=-1)
    refused(abi.ERR_OUT_OF_RANGE, row_begin=5, row_end=4)
    hdr = oc.hdr_configuration(); hdr.ResolveToSRGB = 1
    refused(bad, "pLinearToPSRGB", hdr=hdr)
    hdr = oc.hdr_configuration(); hdr.DitheringStrength = 1
    refused(bad, "ApplyDither", hdr=hdr)
    hdr = oc.hdr_configuration(); hdr.AlbedoIsSRGB = 1
    refused(bad, "pSRGBToPLinear", hdr=hdr)
    # NULL hdr, lut, quad, regions: through the raw entry point
    import ctypes as C
    lib = native.lib()
    device = native.lut_blending(case.dark_tex, case.bright_tex, 0.25, 0.75, 0.1)
    hdr = oc.hdr_configuration()
    quad = (C.c_float * 4)(0, 0, 12, 9)
    lr, ar = (C.c_float * 4)(0, 0, 8, 6), (C.c_float * 4)(0, 0, 10, 7)
    p = lambda x: C.cast(x, C.c_void_p) if not isinstance(x, C.Structure) else C.cast(C.byref(x), C.c_void_p)      # noqa: E731
    full = [p(hdr), p(device), p(quad), p(lr), p(ar)]
    for missing in range(5):
        args = list(full)
        args[missing] = None
        assert lib.ilm_resolve_lighting_lut(case.src.handle, case.tex.handle, dst.handle, *args, None, 1, 1, 0, 9) == bad, missing
        assert np.array_equal(dst.download(), fill), missing
    # a zero-sized quad is valid and writes nothing
    native.resolve_lighting_lut(case.src, dst, oc.hdr_configuration(), device, (3, 3, 0, 5), case.tex)
    assert np.array_equal(dst.download(), fill)
    # textures of another context
    other = native.Context(0)
    foreign = dict(src=native.Lightmap(other, 8, 6, H4), albedo=native.Lightmap(other, 10, 7, C8), lut=native.Lightmap(other, 25, 10, C8),
                   dst=native.Lightmap(other, 12, 9, F4))
    foreign["dst"].upload(fill)
    refused(bad, "context", src=foreign["src"])
    refused(bad, "context", albedo=foreign["albedo"])
    refused(bad, "context", lut=dict(DarkLUT=foreign["lut"].handle))
    with pytest.raises(native.IlluminantError) as e:
        native.resolve_lighting_lut(case.src, foreign["dst"], oc.hdr_configuration(), device, (0, 0, 12, 9), case.tex)
    assert e.value.code == bad and np.array_equal(foreign["dst"].download(), fill)
    _close(*foreign.values())
    other.close()
    _close(dst)
    case.close()
