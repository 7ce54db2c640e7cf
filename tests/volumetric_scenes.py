"""The light lists of the volumetric-light tests with what each must contain.  tests/test_volumetric_gpu.py renders them on the device and
asserts these conditions on the restatement it compares with; tests/test_volumetric_kat.py asserts them without a GPU, so a scene that
does not contain what it claims fails there too.

The frame is directional_common's: 44 x 27 pixels over a field with a tall box (x 10 .. 20, y 8 .. 16, z 0 .. 24) and an ellipsoid
(centre (33, 18, 6), radii (6, 5, 6)); the G-buffer's relief lies at z = 0.5 .. 5.5, the ground plane at z = 0; MaximumZ = 128.
"""
from illuminant_amd import abi
from tests import volumetric_common as vc

W, H = vc.WIDTH, vc.HEIGHT
AMBIENT = (0.0213, 0.0377, 0.0591, 1.0)
FORMAT_PAIRS = [(abi.SDF_UNORM16, None), (abi.SDF_FP16, None), (abi.SDF_UNORM16, abi.GBUFFER_FLOAT4), (abi.SDF_FP16, abi.GBUFFER_HALF4),
                (None, abi.GBUFFER_FLOAT4), (None, None)]
NAN = float("nan")


def cone(**kw):
    """a round cone that widens towards the ground behind the field's box; no light direction: the march projects from its start"""
    args = dict(shape=vc.CONE, start=(8.0, 6.0, 26.0), end=(26.0, 18.0, 2.0), start_radius=2.0, end_radius=7.0, color=(1.0, 0.8, 0.6, 0.9),
                opacity=0.6, volumetricity=0.5, ramp_length=4.0, ramp_power=1.5, ao_radius=5.0, ao_opacity=0.6)
    args.update(kw)
    return vc.volumetric_light(**args)


def ellipsoid(**kw):
    """an ellipsoid around the field's ellipsoid, lit along a direction"""
    args = dict(shape=vc.ELLIPSOID, start=(24.0, 4.0, -6.0), end=(42.0, 22.0, 14.0), direction=(0.3, 0.2, -0.9), color=(0.3, 0.5, 1.0, 0.7),
                ramp_length=3.0, ramp_power=0.8, distance_attenuation=2.0)
    args.update(kw)
    return vc.volumetric_light(**args)


def box(**kw):
    """a box standing on the ground that casts no shadow: technique VolumetricLight"""
    args = dict(shape=vc.BOX, start=(2.0, 14.0, 0.0), end=(16.0, 26.0, 10.0), color=(0.2, 0.9, 0.4, 1.0), ramp_length=2.0, casts_shadows=False,
                volumetricity=2.0)
    args.update(kw)
    return vc.volumetric_light(**args)


def three_shapes():
    return [cone(), ellipsoid(), box()]


def lit(want):
    return [f for f in want.detail.values() if not f.get("discarded")]


def discarded(want):
    return [f for f in want.detail.values() if f.get("discarded")]


def assert_three_shapes(want, have_field, have_gbuffer):
    samples, pairs, traced = want.stats
    shapes = {f["shape"] for f in lit(want)}
    assert shapes == {vc.ELLIPSOID, vc.CONE, vc.BOX}, shapes
    assert len(lit(want)) > 300 and len(discarded(want)) > 50, (len(lit(want)), len(discarded(want)))
    assert {b for f in want.detail.values() for b in f["column_branches"]} == {0, 1, 2}, "the three returns of sdRoundCone"
    assert all(f["iterations"] == vc.MAX_STEP_COUNT + 1 for f in want.detail.values())
    assert all(not f["march_samples"] for f in want.detail.values() if f["shape"] == vc.BOX), "the box casts no shadow"
    if have_field:
        ends = {e for f in want.detail.values() for e in f["march_ends"]}
        assert ends == {"hit", "end", "count"}, ends
        assert traced > 300 and samples > 20 * traced
        assert any(f["ao"] < 1 for f in want.detail.values()), "an AO sample shows"
        shadowed = [f for f in lit(want) if f["march_ends"] and f["hits"] == 0]
        assert len(shadowed) > 5, "some lit pairs have every column point in shadow"
    else:
        assert samples == 0 and traced == 0
        assert all(not f["march_samples"] for f in want.detail.values())
    if have_gbuffer:
        assert any(f["trace_shadows"] is False and f["shape"] != vc.BOX for f in want.detail.values()), "texels with shadows disabled"
        assert pairs > len(want.detail), "fullbright texels form pairs and are discarded before the core"
    else:
        assert pairs == len(want.detail)


def _below_the_ground(want):
    assert want.detail and all(f["iterations"] == 1 and f["z1"] < f["z2"] for f in want.detail.values()), "the body runs once"
    assert not lit(want)


def _thin(want):
    counts = {f["iterations"] for f in want.detail.values()}
    assert len(counts) >= 3 and min(counts) >= 1 and max(counts) < vc.MAX_STEP_COUNT + 1, counts
    assert all(f["step"] == vc.F(1) / vc.F(vc.MAX_STEP_COUNT) for f in want.detail.values()), "step = max(|z2 - z1|, 1) / steps"
    assert len(lit(want)) > 20


def _partly_outside(want):
    assert 0 < want.stats[1] < 200 and len(lit(want)) > 20


def _wholly_outside(want):
    assert want.stats == (0, 0, 0) and not want.detail


def _blowout(want):
    returned = {f["returned"] for f in want.detail.values()}
    assert returned == {"sum", "max"}, returned
    sums = [f for f in want.detail.values() if f["returned"] == "sum"]
    assert any(f.get("discarded") for f in sums) and any(not f.get("discarded") for f in sums), "blowout darkens some pixels to nothing"
    assert all(f["diffuse"] < 0 for f in sums)


def _capsule(want):
    assert len(lit(want)) > 100
    assert {b for f in want.detail.values() for b in f["column_branches"]} == {0, 1, 2}
    assert any(f["contact"] < 0 and f["diffuse"] > f["pre_trace"] for f in lit(want)), "the contact term wins somewhere"


SPECIAL = {
    "below the ground": (lambda: [ellipsoid(start=(10.0, 5.0, -30.0), end=(30.0, 20.0, -10.0))], _below_the_ground),
    "thin": (lambda: [box(start=(4.0, 3.0, 4.8), end=(30.0, 20.0, 5.2), casts_shadows=True, ramp_length=0.5, volumetricity=0.2)], _thin),
    "partly outside the frame": (lambda: [cone(start=(-12.0, -9.0, 20.0), end=(6.0, 5.0, 3.0))], _partly_outside),
    "wholly outside the frame": (lambda: [box(start=(60.0, -30.0, 0.0), end=(90.0, -10.0, 25.0), color=(4.0, 3.0, 2.0, 1.0))], _wholly_outside),
    "blowout under surfaces that face away": (lambda: [ellipsoid(start=(6.0, 2.0, -13.0), end=(30.0, 24.0, 7.0), blowout=0.3, volumetricity=0.2,
                                                                   casts_shadows=False)], _blowout),
    "a capsule along a direction": (lambda: [cone(start=(8.0, 20.0, 3.0), end=(36.0, 8.0, 3.0), start_radius=40.0 / 8, end_radius=40.0 / 8,
                                                  direction=(-0.5, 0.3, -0.8), ao_radius=0.0, volumetricity=1.0)], _capsule),
}


def special(which):
    return SPECIAL[which][0]()


STEP_COUNTS = (1.0, 2.5, 4096.0)


def step_count_lights(steps):
    if steps > 64:      # four pixels, no march: 4 097 column points each
        return [box(start=(20.0, 10.0, 0.0), end=(22.0, 12.0, 10.0))]
    return three_shapes()


def assert_step_counts(want, steps):
    assert want.detail
    counts = {f["iterations"] for f in want.detail.values()}
    assert max(counts) <= int(steps) + 2 and all(f["guard_left"] > 0 for f in want.detail.values()), "the arithmetic ends the column, not the guard"
    if steps > 64:
        assert want.stats[1] == 4 and counts == {4097}
    else:
        assert max(max(f["march_samples"], default=0) for f in want.detail.values()) == int(steps)
        assert len(lit(want)) > 100


def five_lights():
    return [special("partly outside the frame")[0], special("wholly outside the frame")[0], ellipsoid(), box(start=(10.0, 4.0, 0.0), end=(34.0, 22.0, 8.0)), cone()]


def assert_five_lights(want):
    assert want.image[..., 3].max() >= 4 and want.stats[2] > 300


def invisible_lights():
    return [box(start=(-10030.0, -5.0, 0.0), end=(-9970.0, 35.0, 20.0), casts_shadows=True)]


STUCK_ENVIRONMENT = (("ground_z", 2.0 ** 40), ("maximum_z", 2.0 ** 40))


def stuck_lights():
    return [box(start=(5.0, 4.0, 0.0), end=(30.0, 20.0, 2.0 ** 41), casts_shadows=True)]


def assert_stuck(want):
    bodies = int(vc.MAX_STEP_COUNT) + vc.LOOP_GUARD
    assert len(want.detail) > 100
    assert all(f["iterations"] == bodies and f["guard_left"] == 0 for f in want.detail.values())
    assert want.stats[2] == len(want.detail) and want.stats[0] >= bodies * want.stats[2]


def exact_lights():
    """RampPower 0 and shapes that hover above the ground: no pow in what they add"""
    return [cone(end=(26.0, 18.0, 12.0), end_radius=5.0, ramp_power=0.0, volumetricity=2.5),
            ellipsoid(start=(24.0, 4.0, 6.0), end=(42.0, 22.0, 18.0), ramp_power=0.0, volumetricity=1.7, ao_radius=4.0, ao_opacity=0.5),
            box(start=(2.0, 14.0, 4.0), end=(16.0, 26.0, 20.0), ramp_power=0.0, volumetricity=3.0)]


def assert_exact_lights(want):
    assert all(f["shape_opacity"] == 0 and f["diffuse"] == 0 for f in want.detail.values())
    assert want.stats[2] > 300
    values = {float(f["opacity"]) for f in lit(want)}
    assert len(values) > 50 and any(0 < v < 1 for v in values)


def degenerate_lights():
    return [ellipsoid(start=(10.0, 5.0, 0.0), end=(10.0, 15.0, 8.0)),                                  # a zero radius component
            cone(start=(20.0, 10.0, 5.0), end=(20.0, 10.0, 5.0), start_radius=3.0, end_radius=3.0),    # a zero-length cone
            box(ramp_length=0.0),
            ellipsoid(volumetricity=0.0),
            ellipsoid(start=(14.0, 4.0, -6.0), end=(26.0, 16.0, 6.0), direction=None),                 # centred on the ground plane's point (20, 10, 0)
            cone(start=(NAN, 6.0, 26.0)),
            box(end=(16.0, 26.0, NAN)),
            cone(start=(NAN, NAN, NAN), end=(NAN, NAN, NAN), start_radius=NAN, end_radius=NAN)]


def dark_degenerate_lights():
    d = degenerate_lights()
    return [d[1], d[5], d[7]]


def assert_dark(want):
    assert not lit(want) and want.stats[1] > 0
