"""CPU-only: the species wall's host side -- the sheet's arithmetic, the `wall` command's parser, FramePipeline's
refusal of split_compare for an operator with a size of its own, the renderer's sink size, and the `video` parser, which shares
its option blocks with `wall` now, against a snapshot of it taken before they were factored out (tests/golden/video_parser.json)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN


def test_layout_arithmetic_and_even_rounding():
    from animal_vision_amd.gallery_grid import STRIP_H, GridLayout, grid_shape, keep_ar_size
    from animal_vision_amd.wall import WallLayout

    names = ["Original", "Dog", "Cat", "HoneyBee", "ReinDeer"]
    lay = WallLayout(names, 54, 96, 32, 8)
    assert (lay.h, lay.w) == keep_ar_size(54, 96, 32) == (32, 57)
    assert (lay.cols, lay.rows) == grid_shape(5) == (3, 2) and lay.strip_h == STRIP_H == 40
    assert (lay.cell_h, lay.cell_w) == (32 + 40 + 8, 57 + 8)
    assert lay.grid_shape == (2 * 80 + 8, 3 * 65 + 8) == (168, 203)   # the gallery's canvas: GridLayout's
    assert lay.grid_shape == GridLayout(names, [(54, 96)] * 5, 32, 8).canvas_shape[:2]
    assert lay.canvas_shape == (168, 204)                             # the odd width rounded up
    assert lay.segments.shape[1] == 6 and len(lay.seg_offsets) == len(lay.seg_counts) == 5
    assert lay.seg_offsets[0] == 0 and sum(lay.seg_counts) == len(lay.segments) and all(c > 0 for c in lay.seg_counts)
    # no labels: no strip, no segments; both dimensions odd -> both rounded
    bare = WallLayout(["a", "b"], 37, 51, 16, 7, with_labels=False)
    assert bare.strip_h == 0 and len(bare.segments) == 0 and bare.seg_counts == [0, 0]
    assert (bare.h, bare.w) == (16, 22) and bare.grid_shape == (16 + 7 + 7, 2 * (22 + 7) + 7) == (30, 65) and bare.canvas_shape == (30, 66)
    odd = WallLayout(["a"], 37, 51, 16, 8, with_labels=False)
    assert odd.grid_shape == (32, 38) and odd.canvas_shape == (32, 38)  # already even: unchanged
    both = WallLayout(["a"], 48, 64, 15, 8, with_labels=False)
    assert both.grid_shape == (31, 36) and both.canvas_shape == (32, 36)
    same = WallLayout(["a"] * 20, 1080, 1920, 256, 8)
    assert same.grid_shape == (1224, 2323) and same.canvas_shape == (1224, 2324)  # the README's 20-tile sheet
    assert WallLayout(["a"], 256, 300, 256, 8).w == 300                # tile height = frame height: no resize
    with pytest.raises(ValueError):
        WallLayout([], 48, 64)


def test_per_frame_species_are_named_without_a_device():
    from animal_vision_amd.animals import HoneyBee
    from animal_vision_amd.gallery import _CLASS_NAMES
    from animal_vision_amd.wall import WallStreamOp, per_frame_names

    assert per_frame_names(list(_CLASS_NAMES)) == ["RatUV", "Mantis Shrimp"]
    assert per_frame_names(["Dog", "Cat", "HoneyBee", "ReinDeer"]) == []
    # the operator refuses them before it touches a device (this test has none)
    from animal_vision_amd.gallery import species_class

    with pytest.raises(ValueError, match="rat.*RatUV"):
        WallStreamOp([("Dog", species_class("Dog")()), ("rat", species_class("RatUV")())], 48, 64)
    with pytest.raises(ValueError, match="HoneyBee"):
        WallStreamOp([("bee", HoneyBee(hsi_downsample=True, hsi_scale=0.5))], 48, 64)
    with pytest.raises(ValueError, match="tile_height"):
        WallStreamOp([("Dog", species_class("Dog")())], 48, 64, tile_height=0)
    with pytest.raises(ValueError, match="at least one tile"):
        WallStreamOp([], 48, 64, original=False)


def _error(capsys, argv):
    from animal_vision_amd.wall import parse_args

    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_parser_errors(capsys):
    io = ["synthetic:64x48:2", "out.npy"]
    assert "unknown species 'Dgo'" in _error(capsys, io + ["--species", "Dog,Dgo"])
    err = _error(capsys, io + ["--species", "Dog,Mantis Shrimp,RatUV"])
    assert "Mantis Shrimp" in err and "RatUV" in err and "per frame" in err
    assert "exactly one of --species" in _error(capsys, io)
    assert "exactly one of --species" in _error(capsys, io + ["--species", "Dog", "--category", "UV"])
    assert "--batch must be 1..16" in _error(capsys, io + ["--species", "Dog", "--batch", "17"])  # above every member's cap
    assert "names no species" in _error(capsys, io + ["--species", ","])
    assert "invalid choice" in _error(capsys, io + ["--category", "Fish"])
    assert "--tile-height" in _error(capsys, io + ["--species", "Dog", "--tile-height", "0"])
    # the `video` command's dependency checks, through the shared functions
    assert "--transfer needs --pix-fmt" in _error(capsys, io + ["--species", "Dog", "--transfer", "pq"])
    assert "--tonemap needs --transfer" in _error(capsys, io + ["--species", "Dog", "--tonemap", "clip"])
    assert "--matrix bt2020 needs --transfer" in _error(capsys, io + ["--species", "Dog", "--matrix", "bt2020"])
    assert "only reduces" in _error(capsys, io + ["--species", "Dog", "--scale", "128x96"])
    assert "--pix-fmt and --size go together" in _error(capsys, io + ["--species", "Dog", "--pix-fmt", "nv12"])
    # --hsi-model and --hsi-scale are not offered
    assert "unrecognized arguments" in _error(capsys, io + ["--species", "HoneyBee", "--hsi-scale", "0.5"])
    assert "unrecognized arguments" in _error(capsys, io + ["--species", "HoneyBee", "--hsi-model", "seeded"])


def test_parser_resolves_species_and_categories(capsys):
    from animal_vision_amd.gallery import CATEGORIES
    from animal_vision_amd.wall import parse_args

    a = parse_args(["in.y4m", "out.y4m", "--species", "Dog, Cat,HoneyBee,ReinDeer"])
    assert a.names == ["Dog", "Cat", "HoneyBee", "ReinDeer"] and (a.tile_height, a.pad, a.no_labels, a.no_original) == (256, 8, False, False)
    assert (a.depth, a.batch, a.matrix, a.tonemap, a.peak_nits, a.sdr_white) == (3, 1, "bt601", "mobius", 1000.0, 203.0)  # video's defaults
    assert capsys.readouterr().err == ""
    a = parse_args(["in.y4m", "out.y4m", "--category", "UV", "--no-labels", "--no-original", "--tile-height", "128", "--pad", "0"])
    assert a.names == [n for n in CATEGORIES["UV"] if n not in ("RatUV", "Mantis Shrimp")] and len(a.names) == 14
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "dropped RatUV, Mantis Shrimp" in err  # one line on stderr
    assert parse_args(["in.y4m", "out.y4m", "--category", "Non-UV"]).names == CATEGORIES["Non-UV"]
    assert capsys.readouterr().err == ""


class _SizedOp:
    """An operator with an output size of its own, as FramePipeline sees one."""

    ctx = None

    def out_shape(self, H, W):
        return H + 10, 2 * W

    def run_device(self, *a, **k):
        raise AssertionError("never reached")


def test_split_compare_is_refused_for_an_op_with_its_own_size():
    from animal_vision_amd.pipeline import FramePipeline

    with pytest.raises(ValueError, match="split_compare.*_SizedOp.*out_shape"):
        FramePipeline(_SizedOp(), 48, 64, split_compare=True)


def test_sinks_take_the_size_they_are_told(tmp_path):
    """A .y4m source into a .y4m sink, payloads of another size than the source's: the header and the frames carry the size
    set_output_size names, also when no frame arrives at all."""
    import _yuv_ref as R
    from animal_vision_amd.renderers import VideoRenderer
    from animal_vision_amd.renderers.y4m import Y4MReader

    H, W, Hc, Wc = 48, 64, 20, 36
    rgb = np.random.default_rng(0).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    src = str(tmp_path / "in.y4m")
    with open(src, "wb") as f:
        f.write(R.y4m_bytes(list(R.encode(rgb)), H, W, header="F25:1 Ip A1:1 C420jpeg"))
    sheets = R.encode(np.random.default_rng(1).integers(0, 256, (2, Hc, Wc, 3), dtype=np.uint8))
    for n_rendered in (2, 0):
        dst = str(tmp_path / f"out{n_rendered}.y4m")
        vr = VideoRenderer(read_path=src, write_path=dst)
        vr.open()
        assert vr.yuv_hw == (H, W) and vr.sink_hw == vr.out_hw == (H, W)
        vr.set_output_size(Hc, Wc)
        assert vr.out_hw == (H, W) and vr.sink_hw == (Hc, Wc)
        for k in range(n_rendered):
            vr.render(sheets[k])
        vr.close()
        rd = Y4MReader(dst)
        assert (rd.header.height, rd.header.width) == (Hc, Wc) and rd.total_frames == n_rendered
        for k in range(n_rendered):
            assert np.array_equal(rd.read(), sheets[k])
        rd.close()
    # raw video: the frame size of the sink is the told one
    raw_in, raw_out = str(tmp_path / "in.yuv"), str(tmp_path / "out.yuv")
    R.encode(rgb).tofile(raw_in)
    vr = VideoRenderer(read_path=raw_in, write_path=raw_out, pix_fmt="yuv420p", size=(W, H))
    vr.open()
    vr.set_output_size(Hc, Wc)
    vr.render(sheets[0])
    vr.close()
    assert os.path.getsize(raw_out) == sheets[0].size


def test_video_parser_is_what_it_was(monkeypatch):
    """video.build_parser()'s options and help text against the snapshot taken from the commit before its option blocks were
    factored out for the `wall` command."""
    monkeypatch.setenv("COLUMNS", "100")
    from animal_vision_amd import video

    snap = json.load(open(os.path.join(GOLDEN, "video_parser.json")))
    assert snap["columns"] == 100
    ap = video.build_parser()
    acts = []
    for a in ap._actions:
        acts.append({"flags": list(a.option_strings), "dest": a.dest, "nargs": a.nargs, "default": a.default, "required": bool(a.required),
                     "choices": None if a.choices is None else list(a.choices), "metavar": a.metavar, "help": a.help,
                     "type": getattr(a.type, "__name__", None) if a.type is not None else None, "kind": type(a).__name__})
    assert [a["flags"] or a["dest"] for a in acts] == [a["flags"] or a["dest"] for a in snap["actions"]]
    assert acts == snap["actions"]
    assert ap.format_help() == snap["help"]


def test_wall_parser_offers_the_video_io_options():
    from animal_vision_amd import video, wall

    flags = lambda ap: {s for a in ap._actions for s in a.option_strings}  # noqa: E731
    v, w = flags(video.build_parser()), flags(wall.build_parser())
    assert v - w == {"--split-compare", "--hsi-model", "--hsi-scale"}
    assert w - v == {"--category", "--tile-height", "--pad", "--no-original"}
    shared = {a.dest: a for a in video.build_parser()._actions}
    for a in wall.build_parser()._actions:
        if a.dest in shared and a.dest not in ("help", "species", "no_labels"):
            b = shared[a.dest]
            assert (a.option_strings, a.default, a.choices, a.help, a.metavar) == (b.option_strings, b.default, b.choices, b.help, b.metavar), a.dest
