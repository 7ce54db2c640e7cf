"""Pins the oracle's FillReadbackResult / lightmap resolve restatement (oracle/ilm_oracle_output.c) on the hand-evaluated
cases of tests/golden/output_ext.json and, for the resolve, at the edges of its domain: black, dim, negative and non-finite texels, the
parameter clamps, a second reading of the shaders in numpy.  No GPU."""
import numpy as np
import pytest

from illuminant_amd import abi
from tests import output_common as oc
from tests.util import assert_bits_equal, assert_close


@pytest.mark.parametrize("index", range(len(oc.load_cases())))
def test_closed_form_case(oracle, index):
    oc.check_case(oc.load_cases()[index], oc.OracleBackend(oracle))


# ---- the resolve at black, dim and non-finite texels (tests/output_common.py) ----------------------------------------------------------
@pytest.mark.parametrize("index", range(len(oc.EDGE_CASES)), ids=[c["name"] for c in oc.EDGE_CASES])
def test_edge_closed_form_case(oracle, index):
    oc.check_edge_case(oc.EDGE_CASES[index], oc.OracleBackend(oracle))


def test_black_tone_mapped_texel_is_one_ulp_of_the_curves_floor(oracle):
    """Uncharted2Tonemap(0) in float32 is 2^-27, not 0: what every dim pixel's parity hangs on (the quotient must be correctly rounded)."""
    lm = np.zeros((1, 2, 4), np.float32)
    out = oracle.resolve_lighting(lm, oc.hdr_configuration(abi.HDR_TONE_MAP, white_point=4.0))
    white = oc._uncharted2(np.float32(4.0))
    assert_bits_equal(out[0, 0, :3], np.full(3, np.float32(2.0 ** -27) / white, np.float32), "tone-mapped black")


@pytest.mark.parametrize("with_albedo", [False, True], ids=["plain", "albedo"])
@pytest.mark.parametrize("mode", oc.MODES, ids=[oc.MODE_NAME[m] for m in oc.MODES])
@pytest.mark.parametrize("fmt", oc.FORMATS, ids=[oc.FORMAT_NAME[f] for f in oc.FORMATS])
def test_second_reading_matches_oracle_on_the_edge_frame(oracle, fmt, mode, with_albedo):
    """The numpy restatement against the oracle at black, dim, negative and non-finite texels: the same NaN and infinities, GammaCompress
    (no pow) bit for bit, the two pow modes to 1e-6 relative (powf against a rounded double pow)."""
    light = oc.decode(oc.edge_source(fmt), fmt)
    af = oc.edge_albedo_format(fmt)
    albedo = oc.decode(oc.edge_albedo(af), af) if with_albedo else None
    for gamma in oc.EDGE_GAMMAS if mode != abi.HDR_GAMMA_COMPRESS else (1.0,):
        for offset in oc.EDGE_OFFSETS:
            hdr = oc.edge_hdr(mode, gamma, offset)
            what = "edge frame %s %s gamma %g offset %g" % (oc.FORMAT_NAME[fmt], oc.MODE_NAME[mode], gamma, offset)
            want = oracle.resolve_lighting(light, hdr, albedo=albedo)
            mine = oc.resolve_reference(light, hdr, albedo)
            if mode == abi.HDR_GAMMA_COMPRESS:
                assert_bits_equal(mine, want, what)
            else:
                m, w = oc.assert_same_where_not_finite(mine, want, what)
                assert_close(m, w, what, rtol=1e-6, atol=0.0)
            finite = np.isfinite(light).all(axis=-1) & (albedo is None or np.isfinite(albedo).all(axis=-1))
            if mode != abi.HDR_GAMMA_COMPRESS:
                assert not np.isnan(want[finite]).any(), what + ": a finite texel resolves to NaN"
            elif albedo is None and offset == 0.0:
                black = (light[..., :3] == 0).all(axis=-1)
                assert black.any() and np.isnan(want[black][:, :3]).all()            # 0 / 0, in the shader as here


@pytest.mark.parametrize("mode", oc.MODES, ids=[oc.MODE_NAME[m] for m in oc.MODES])
def test_exact_byte_set_is_most_of_the_random_frame(oracle, mode):
    """The RGBA8 criterion of the format matrix demands the exact byte wherever the tolerance band holds one byte; with independent
    uniform content that must be (and is asserted on the GPU to be) at least 90 % of the colour bytes, for every source and albedo."""
    for fmt in oc.FORMATS:
        for af in (None,) + oc.FORMATS:
            light = oc.decode(oc.random_source(fmt), fmt)
            albedo = oc.decode(oc.random_albedo(af), af) if af is not None else None
            want = oracle.resolve_lighting(light, oc.matrix_hdr(mode), albedo=albedo)
            _, exact = oc.byte_band(want)
            assert exact[..., :3].mean() >= 0.9, (oc.FORMAT_NAME[fmt], oc.FORMAT_NAME[af], exact[..., :3].mean())
            mine = oc.resolve_reference(light, oc.matrix_hdr(mode), albedo)
            assert_close(mine, want, "random frame", rtol=1e-6, atol=0.0)
