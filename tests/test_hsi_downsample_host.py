"""HoneyBee on MST++ at reduced network resolution, the host side: the `video` command's --hsi-model / --hsi-scale flags,
how a configured HoneyBee is routed, and the rule that sizes the reduced frame (with the refusal of one too small to reflect-pad).
No device work: no predictor is built and no operator is run."""
import argparse

import pytest


def _args(*extra, species="HoneyBee"):
    from animal_vision_amd.video import parse_args

    return parse_args(["synthetic:96x64:5", "out.npy", "--species", species, *extra])


@pytest.mark.parametrize("flag", [("--hsi-model", "seeded"), ("--hsi-scale", "0.5")])
def test_the_flags_are_honeybees_alone(flag, capsys):
    with pytest.raises(SystemExit):
        _args(*flag, species="Dog")
    err = capsys.readouterr().err
    assert flag[0] in err and "Dog" in err


@pytest.mark.parametrize("bad", ["1.0", "0.01", "half", "nan", "-0.5"])
def test_hsi_scale_outside_the_class_range_is_refused(bad, capsys):
    with pytest.raises(SystemExit):
        _args("--hsi-scale", bad)
    assert "--hsi-scale" in capsys.readouterr().err


def test_a_missing_checkpoint_is_a_parser_error(tmp_path, capsys):
    with pytest.raises(SystemExit):
        _args("--hsi-model", str(tmp_path / "absent.pth"))
    assert "absent.pth" in capsys.readouterr().err


def test_defaults_and_help_text():
    from animal_vision_amd.video import build_parser

    a = _args()
    assert a.hsi_model is None and a.hsi_scale is None
    a = _args("--hsi-model", "seeded", "--hsi-scale", "0.25", "--batch", "2")
    assert a.hsi_model == "seeded" and a.hsi_scale == 0.25 and a.batch == 2
    text = " ".join(build_parser().format_help().split())
    assert "no checkpoint ships" in text and "for testing" in text


def test_make_animal_sets_the_downsample_switch():
    from animal_vision_amd.animals import Dog, HoneyBee
    from animal_vision_amd.video import make_animal, route

    bee = make_animal(_args())
    assert type(bee) is HoneyBee and not bee.hsi_downsample and bee.hsi_model is None and route(bee) == "honeybee"
    bee = make_animal(_args("--hsi-scale", "0.5"))
    assert bee.hsi_downsample and bee.hsi_scale == 0.5 and bee.hsi_model is None and route(bee) == "frame"
    assert type(make_animal(_args(species="Dog"))) is Dog
    # what make_animal reads, without the parser (and without building a predictor: hsi_model stays None)
    bee = make_animal(argparse.Namespace(species="HoneyBee", hsi_scale=0.1, hsi_model=None))
    assert bee.hsi_downsample and bee.hsi_scale == 0.1


def test_route_of_a_configured_honeybee():
    from animal_vision_amd.animals import HoneyBee
    from animal_vision_amd.video import route

    assert route(HoneyBee(hsi_model=object())) == "honeybee_mst"
    assert route(HoneyBee(hsi_model=object(), hsi_downsample=True, hsi_scale=0.5)) == "honeybee_mst"
    assert route(HoneyBee()) == "honeybee"
    assert route(HoneyBee(hsi_downsample=True)) == "frame"


def test_per_frame_species_still_refuse_a_batch():
    from animal_vision_amd.animals import HoneyBee
    from animal_vision_amd.video import stream_op

    assert stream_op(HoneyBee(hsi_downsample=True), 64, 96, 3) is None
    with pytest.raises(ValueError):
        stream_op(HoneyBee(hsi_downsample=True), 64, 96, 3, 2)


def test_reduced_size_rule_against_pad_amounts():
    """h = max(1, round(H s)), w = max(1, round(W s)); refused when a reflect pad to the stride would reach past the reduced frame."""
    from animal_vision_amd.ml.predict import pad_amounts, reduced_size

    # 37 x 45 at 0.1 -> 4 x 4: 12 rows of padding, 6 on either side of 4 rows
    assert (max(1, round(37 * 0.1)), max(1, round(45 * 0.1))) == (4, 4)
    t, b, l, r = pad_amounts(4, 4, 16)
    assert (t, b, l, r) == (6, 6, 6, 6) and max(t, b) >= 4 and max(l, r) >= 4
    with pytest.raises(ValueError) as e:
        reduced_size(37, 45, 0.1, 16)
    msg = str(e.value)
    assert "37x45" in msg and "4x4" in msg and "hsi_scale" in msg and "0.1" in msg
    # 72 x 88 at 0.1 -> 7 x 9: pads (4, 5) and (3, 4) stay inside the frame
    t, b, l, r = pad_amounts(7, 9, 16)
    assert (t, b, l, r) == (4, 5, 3, 4) and max(t, b) < 7 and max(l, r) < 9
    assert reduced_size(72, 88, 0.1, 16) == (7, 9)
    # the rule itself, its floor of one sample, and the cases that are the full-size route
    assert reduced_size(2160, 3840, 0.5, 16) == (1080, 1920)
    assert reduced_size(97, 131, 0.25, 16) == (24, 33)
    assert reduced_size(72, 88, None, 16) is None
    assert reduced_size(1, 1, 0.6, 16) is None  # round(0.6) = 1: nothing is reduced
    for h, w in ((2, 40), (40, 2)):  # one reduced extent of 1 sample cannot be reflected at all
        with pytest.raises(ValueError):
            reduced_size(h * 10, w * 10, 0.05, 16)
    for bad in (1.0, 0.01, 0.0, 2.0):
        with pytest.raises(ValueError):
            reduced_size(72, 88, bad, 16)
