"""CPU: the host side of the wide view of the dichromats -- FovSpec, fov= on the species, the `video` command's
--fov options and their refusals, the routing, the library's declaration, and the warp tables against the oracle's maps."""
import math
import subprocess

import numpy as np
import pytest

import _wide_ref as WR


def _parse(*argv):
    from animal_vision_amd import video

    return video.parse_args(["in.y4m", "out.y4m", *argv])


def _refused(capsys, *argv):
    with pytest.raises(SystemExit) as e:
        _parse(*argv)
    assert e.value.code == 2
    return capsys.readouterr().err


# ---------------------------------------------------------------- FovSpec ------------------------------------------------------------
def test_fov_spec_defaults_are_cats_constants_and_it_is_frozen_and_hashable():
    from animal_vision_amd.animals import Cat
    from animal_vision_amd.dichromat import FovSpec

    f = FovSpec(Cat.CAT_PER_EYE_HALF_FOV_DEG, Cat.CAT_OVERLAP_DEG)
    assert (f.camera_hfov_deg, f.to_human_ratio) == (Cat.CAMERA_HFOV_DEG, Cat.CAT_TO_HUMAN_RATIO) == (100.0, 1.30)
    assert f == FovSpec(105, 40) and hash(f) == hash(FovSpec(105.0, 40.0, 100.0, 1.3)) and len({f, FovSpec(105, 40), FovSpec(50, 80)}) == 2
    with pytest.raises(Exception):
        f.overlap_deg = 10.0
    assert f.shown_deg == 4 * 105 - 40 and FovSpec(50, 200).shown_deg == 100.0  # alpha is clamped at 0


@pytest.mark.parametrize("kw,field", [
    (dict(per_eye_half_fov_deg=0.0), "per_eye_half_fov_deg"), (dict(per_eye_half_fov_deg=-5.0), "per_eye_half_fov_deg"),
    (dict(per_eye_half_fov_deg=180.5), "per_eye_half_fov_deg"), (dict(per_eye_half_fov_deg=math.nan), "per_eye_half_fov_deg"),
    (dict(per_eye_half_fov_deg="105"), "per_eye_half_fov_deg"), (dict(per_eye_half_fov_deg=True), "per_eye_half_fov_deg"),
    (dict(overlap_deg=-1.0), "overlap_deg"), (dict(overlap_deg=360.5), "overlap_deg"), (dict(overlap_deg=math.inf), "overlap_deg"),
    (dict(camera_hfov_deg=0.0), "camera_hfov_deg"), (dict(camera_hfov_deg=180.0), "camera_hfov_deg"), (dict(camera_hfov_deg=math.nan), "camera_hfov_deg"),
    (dict(to_human_ratio=0.99), "to_human_ratio"), (dict(to_human_ratio=math.inf), "to_human_ratio"), (dict(to_human_ratio=None), "to_human_ratio"),
])
def test_fov_spec_refuses_by_field(kw, field):
    from animal_vision_amd.dichromat import FovSpec

    base = dict(per_eye_half_fov_deg=105.0, overlap_deg=40.0)
    base.update(kw)
    with pytest.raises(ValueError, match=f"FovSpec.{field}"):
        FovSpec(**base)


def test_fov_spec_accepts_the_edges():
    from animal_vision_amd.dichromat import FovSpec

    FovSpec(180.0, 0.0, 179.9, 1.0)
    FovSpec(0.001, 360.0, 0.001, 1e6)
    FovSpec(np.float32(105), np.int64(40))


# ---------------------------------------------------------------- the species ---------------------------------------------------------
def test_fov_on_the_species():
    from animal_vision_amd import animals
    from animal_vision_amd.dichromat import FovSpec, NightSpec

    spec = FovSpec(100, 20, 60)
    dog = animals.Dog(fov=spec)
    assert dog.fov is spec and dog.night is None and animals.Dog().fov is None
    assert animals.Horse(fov=(100, 20, 60)).fov == spec  # the arguments as a tuple
    assert animals.Rat(night=True, fov=spec).night == NightSpec()
    with pytest.raises(TypeError, match="fov"):
        animals.Dog(fov=105)
    with pytest.raises(ValueError, match="FovSpec.overlap_deg"):
        animals.Dog(fov=(105, -1))
    with pytest.raises(NotImplementedError, match="Dog: fov is implemented for uint8 frames, got float32"):
        dog.visualize(np.zeros((8, 8, 3), np.float32))


def test_cat_follows_its_fov():
    from animal_vision_amd.animals import Cat
    from animal_vision_amd.animals._dichromats import CatStreamOp, WideStreamOp
    from animal_vision_amd.dichromat import FovSpec

    cat = Cat(fov=FovSpec(50, 80, 90, 1.5))
    assert (cat.CAMERA_HFOV_DEG, cat.CAT_PER_EYE_HALF_FOV_DEG, cat.CAT_OVERLAP_DEG, cat.CAT_TO_HUMAN_RATIO) == (90.0, 50.0, 80.0, 1.5)
    assert (Cat.CAMERA_HFOV_DEG, Cat.CAT_PER_EYE_HALF_FOV_DEG, Cat.CAT_OVERLAP_DEG, Cat.CAT_TO_HUMAN_RATIO) == (100.0, 105.0, 40.0, 1.30)
    plain = Cat()
    assert plain.fov is None and "CAMERA_HFOV_DEG" not in plain.__dict__
    assert WideStreamOp.crop_rect(Cat(fov=FovSpec(105, 40)), 270, 480) == WideStreamOp.crop_rect(plain, 270, 480)
    assert issubclass(CatStreamOp, WideStreamOp)


# ---------------------------------------------------------------- the command ---------------------------------------------------------
def test_video_fov_options_and_make_animal():
    from animal_vision_amd import video
    from animal_vision_amd.dichromat import AutoNight, FovSpec

    args = _parse("--species", "Horse", "--fov", "105:40")
    assert args.fov == (105.0, 40.0) and args.camera_hfov is None and args.fov_ratio is None
    horse = video.make_animal(args)
    assert type(horse).__name__ == "Horse" and horse.fov == FovSpec(105.0, 40.0, 100.0, 1.30)
    args = _parse("--species", "Dog", "--fov", "50.5:80", "--camera-hfov", "60", "--fov-ratio", "2", "--night-auto", "--bloom", "0.12")
    dog = video.make_animal(args)
    assert dog.fov == FovSpec(50.5, 80.0, 60.0, 2.0) and isinstance(dog.night, AutoNight) and dog.night.night.bloom == 0.12
    cat = video.make_animal(_parse("--species", "Cat", "--fov", "50:80"))
    assert cat.CAT_PER_EYE_HALF_FOV_DEG == 50.0 and cat.CAT_OVERLAP_DEG == 80.0
    assert video.make_animal(_parse("--species", "Dog")).fov is None


def test_build_parser_stays_the_recorded_option_list():
    from animal_vision_amd import video

    flags = {s for a in video.build_parser()._actions for s in a.option_strings}
    assert not flags & {"--fov", "--camera-hfov", "--fov-ratio"}


@pytest.mark.parametrize("argv,words", [
    (["--species", "HoneyBee", "--fov", "105:40"], "--fov: --species HoneyBee is not one of the 20 dichromats"),
    (["--species", "Mantis Shrimp", "--fov", "105:40"], "--fov: --species Mantis Shrimp is not one of the 20 dichromats"),
    (["--species", "Dog", "--camera-hfov", "90"], "--camera-hfov needs --fov"),
    (["--species", "Dog", "--fov-ratio", "1.5"], "--fov-ratio needs --fov"),
    (["--species", "Dog", "--fov", "105"], "--fov takes PHI:OVERLAP"),
    (["--species", "Dog", "--fov", "a:b"], "--fov takes PHI:OVERLAP"),
    (["--species", "Dog", "--fov", "1:2:3"], "--fov takes PHI:OVERLAP"),
    (["--species", "Dog", "--fov", "0:40"], "--fov: PHI must be above 0 and at most 180"),
    (["--species", "Dog", "--fov", "181:40"], "--fov: PHI must be above 0 and at most 180"),
    (["--species", "Dog", "--fov", "nan:40"], "--fov: PHI must be above 0 and at most 180"),
    (["--species", "Dog", "--fov", "105:-1"], "--fov: OVERLAP must be at least 0 and at most 360"),
    (["--species", "Dog", "--fov", "105:361"], "--fov: OVERLAP must be at least 0 and at most 360"),
    (["--species", "Dog", "--fov", "105:40", "--camera-hfov", "180"], "--camera-hfov must be above 0 and below 180"),
    (["--species", "Dog", "--fov", "105:40", "--camera-hfov", "0"], "--camera-hfov must be above 0 and below 180"),
    (["--species", "Dog", "--fov", "105:40", "--camera-hfov", "wide"], "--camera-hfov takes a number"),
    (["--species", "Dog", "--fov", "105:40", "--fov-ratio", "0.9"], "--fov-ratio must be finite and at least 1"),
    (["--species", "Dog", "--fov", "105:40", "--fov-ratio", "inf"], "--fov-ratio must be finite and at least 1"),
    (["--species", "Dog", "--fov", "105:40", "--fov-ratio", "x"], "--fov-ratio takes a number"),
])
def test_video_fov_refusals(capsys, argv, words):
    assert words in _refused(capsys, *argv)


# ---------------------------------------------------------------- routing -------------------------------------------------------------
def test_routing():
    from animal_vision_amd import animals, video
    from animal_vision_amd.dichromat import FovSpec

    fov = FovSpec(105, 40)
    assert video.route(animals.Dog()) == "dichromat" and video.route(animals.Dog(fov=fov)) == "dichromat"  # route() keeps its value
    assert video.route(animals.Cat()) == "frame" and video.route(animals.Cat(fov=fov)) == "frame"
    for cls in (animals.Dog, animals.Horse, animals.Rat, animals.Rabbit, animals.Cat):
        assert video.has_stream_op(cls(fov=fov)) and video.has_stream_op(cls())
    assert not video.has_stream_op(animals.MantisShrimp())


def test_the_library_declares_the_entry():
    from animal_vision_amd import _lib

    res, args = _lib._SIGS["avx_dichromat_wide_u8"]
    fn = _lib.lib.avx_dichromat_wide_u8
    assert res is _lib._i and len(args) == 13 and fn.argtypes == args == _lib._SIGS["avx_cat_wide_u8"][1]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {"avx_dichromat_wide_u8", "avx_cat_wide_u8"} <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert fn(None, None, None, 1, 4, 4, None, None, None, None, None, None, None) == _lib.AVX_ERR_INVALID  # no context: refused, no GPU touched


# ---------------------------------------------------------------- the tables ----------------------------------------------------------
@pytest.mark.parametrize("geometry", WR.GEOMETRIES)
@pytest.mark.parametrize("H,W", [(5, 6), (53, 37), (131, 96)])
def test_warp_tables_equal_the_oracles_maps(oracle, geometry, H, W):
    from animal_vision_amd import geometry as G

    phi, overlap, camera = geometry
    xL, xR, ymap, wL, wR = G.binocular_warp_tables(H, W, W, H, camera, phi, overlap)
    oxL, oxR, oymap, owL, owR = oracle.binocular_warp_maps(H, W, W, H, camera, phi, overlap)
    for got, want in ((xL, oxL[0]), (xR, oxR[0]), (wL, owL[0]), (wR, owR[0]), (ymap, oymap[:, 0])):
        assert got.dtype == np.float32 and np.array_equal(got, want)
    assert (oxL == oxL[0]).all() and (owR == owR[0]).all() and (oymap == oymap[:, :1]).all()  # the grids are what the vectors say


def test_the_three_geometries_are_what_the_tests_take_them_for():
    """Cat's leaves the middle third of the columns black, the narrow camera about 60 %, the third none -- and most columns to both eyes."""
    W = 480
    lit = [WR.lit_columns(W, g) for g in WR.GEOMETRIES]
    assert abs(lit[0].mean() - 2 / 3) < 0.01 and not lit[0][W // 3 + 1 : 2 * W // 3 - 1].any() and lit[0][: W // 3 - 1].all()
    assert 0.35 < lit[1].mean() < 0.45 and lit[2].all()
    from oracle import cpu_ref

    phi, overlap, camera = WR.TWO_EYES
    _, _, _, wL, wR = cpu_ref.binocular_warp_maps(4, W, W, 4, camera, phi, overlap)
    assert 0.65 < ((wL[0] > 0) & (wR[0] > 0)).mean() < 0.85
    assert not WR.wide_ref(cpu_ref.DICHROMATS["dog"], np.full((6, 5, 3), 255, np.uint8), WR.NARROW_CAMERA).any()  # 6 x 5 is all black: never test it alone
