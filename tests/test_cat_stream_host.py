"""CPU: Cat's stream route as far as it can be checked without a GPU -- the two entry points of csrc/cat_wide.hip exist and are
declared to ctypes, `video.has_stream_op` says which species stream, the command's early --batch refusal lets Cat past and still
stops the species of the per-frame loop, and the crop CatStreamOp hands avx_center_zoom_u8 is the reference's."""
import subprocess

import numpy as np
import pytest

SIZES = [(5, 6), (53, 37), (131, 70), (96, 160), (97, 161), (270, 480), (1080, 1920), (2160, 3840), (1, 1), (2, 3), (1, 7)]  # (H, W)


def test_entry_points_are_declared_and_exported():
    from animal_vision_amd import _lib

    for name, nargs in (("avx_cat_wide_u8", 13), ("avx_center_zoom_u8", 11)):
        res, args = _lib._SIGS[name]
        assert res is _lib._i and len(args) == nargs, name
        assert getattr(_lib.lib, name).argtypes == args
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"avx_cat_wide_u8", "avx_center_zoom_u8", "avx_binocular_warp_u8", "avx_dichromat_u8"} <= syms
    assert _lib.lib.avx_abi_version() == 1
    # a NULL context is refused before anything is touched
    assert _lib.lib.avx_cat_wide_u8(None, None, None, 1, 4, 4, None, None, None, None, None, None, None) == _lib.AVX_ERR_INVALID
    assert _lib.lib.avx_center_zoom_u8(None, None, None, 1, 4, 4, 0, 0, 1, 1, None) == _lib.AVX_ERR_INVALID


def test_has_stream_op_and_route():
    from animal_vision_amd.animals import Cat, Dog, HoneyBee, MantisShrimp, RatUV, Reindeer
    from animal_vision_amd.video import has_stream_op, route

    for sp in (Cat(), Dog(), Reindeer(), HoneyBee()):
        assert has_stream_op(sp) is True, type(sp).__name__
    for sp in (MantisShrimp(), RatUV(), HoneyBee(hsi_downsample=True)):
        assert has_stream_op(sp) is False, type(sp).__name__
    assert route(Cat()) == "frame"  # the kind of its operator; the command streams it all the same

    class Tabby(Cat):
        pass

    assert has_stream_op(Tabby()) and route(Tabby()) == "frame"


def test_early_batch_refusal_lets_cat_past_and_stops_the_per_frame_species(tmp_path, monkeypatch):
    from animal_vision_amd import video

    a = video.parse_args(["in.y4m", "out.y4m", "--species", "Cat", "--batch", "2", "--split-compare"])
    assert (a.species, a.batch) == ("Cat", 2)
    assert video.parse_args(["in.y4m", "out.y4m", "--species", "Cat", "--batch", "16"]).batch == 16

    class Reached(Exception):
        pass

    def stop(animal, H, W, depth, batch=1):  # the op itself needs the device
        raise Reached(type(animal).__name__, H, W, depth, batch)

    monkeypatch.setattr(video, "stream_op", stop)
    with pytest.raises(Reached) as e:
        video.main(["synthetic:48x32:3", str(tmp_path / "cat.npy"), "--species", "Cat", "--batch", "2"])
    assert e.value.args == ("Cat", 32, 48, 3, 2)
    with pytest.raises(SystemExit) as e:
        video.main(["synthetic:48x32:3", str(tmp_path / "mantis.npy"), "--species", "Mantis Shrimp", "--batch", "2"])
    assert str(e.value) == "video: --batch 2: Mantis Shrimp runs visualize() per frame and has no batched form"
    with pytest.raises(SystemExit) as e:
        video.main(["synthetic:48x32:3", str(tmp_path / "rat.npy"), "--species", "RatUV", "--batch", "3"])
    assert str(e.value) == "video: --batch 3: RatUV runs visualize() per frame and has no batched form"


@pytest.mark.parametrize("H,W", SIZES)
def test_crop_rectangle_is_the_references(oracle, monkeypatch, H, W):
    """The rectangle the stream op passes to avx_center_zoom_u8 is the one oracle.center_zoom crops: an index image shows which
    source pixels the oracle hands its resize."""
    from animal_vision_amd import geometry as G
    from animal_vision_amd.animals import Cat

    scale = G.zoom_scale_from_cat_ratio(camera_hfov_deg=Cat.CAMERA_HFOV_DEG, cat_per_eye_half_fov_deg=Cat.CAT_PER_EYE_HALF_FOV_DEG,
                                        cat_to_human_ratio=Cat.CAT_TO_HUMAN_RATIO)
    assert scale == oracle.zoom_scale_from_cat_ratio(camera_hfov_deg=100.0, cat_per_eye_half_fov_deg=105.0, cat_to_human_ratio=1.30) and scale > 1.0
    seen = {}

    def record(crop, dsize, interp):
        seen["crop"], seen["dsize"], seen["interp"] = np.array(crop), dsize, interp
        return np.zeros((dsize[1], dsize[0]) + crop.shape[2:], crop.dtype)

    monkeypatch.setattr(oracle, "cv_resize", record)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32), indexing="ij")
    oracle.center_zoom(np.stack([yy, xx], axis=-1), scale)
    crop = seen["crop"]
    want = (int(crop[0, 0, 1]), int(crop[0, 0, 0]), crop.shape[1], crop.shape[0])
    assert seen["dsize"] == (W, H) and seen["interp"] == oracle.INTER_LINEAR
    from animal_vision_amd.animals._dichromats import CatStreamOp

    x0, y0, cw, ch = CatStreamOp.crop_rect(Cat(), H, W)
    assert (x0, y0, cw, ch) == want == G.center_zoom_rect(H, W, scale)
    assert cw >= 1 and ch >= 1 and x0 >= 0 and y0 >= 0 and x0 + cw <= W and y0 + ch <= H
    assert G.center_zoom_rect(H, W, 1.0) is None and G.center_zoom_rect(H, W, 0.5) is None
