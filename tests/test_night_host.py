"""CPU: the night form of the dichromats as far as it can be checked without a GPU -- NightSpec's validation, the tap
tables handed to the library, the `video` command's --night / --bloom, the entry point's declaration and export, that nothing changed
by day, and two properties of the oracle composition the GPU tests compare against (tests/_night_ref.py)."""
import ctypes
import subprocess

import numpy as np
import pytest

import _night_ref as N


def test_night_spec_defaults_and_validation():
    from animal_vision_amd.dichromat import NightSpec

    d = NightSpec()
    assert (d.chroma_scale, d.luminance_boost, d.gamma, d.bloom) == (0.07, 1.8, 0.7, 0.0)  # the reference's commented call; bloom is opt-in
    assert NightSpec(0.0, 1e-3, 2.0, 1.0).bloom == 1.0 and NightSpec(chroma_scale=1.0).chroma_scale == 1.0
    for bad in (dict(chroma_scale=-0.01), dict(chroma_scale=1.01), dict(luminance_boost=0.0), dict(luminance_boost=-1.0), dict(gamma=0.0),
                dict(gamma=-0.5), dict(bloom=-0.1), dict(bloom=1.5), dict(gamma=float("nan")), dict(bloom=float("inf")), dict(chroma_scale="0.1"),
                dict(bloom=True)):
        with pytest.raises(ValueError) as e:
            NightSpec(**bad)
        assert next(iter(bad)) in str(e.value), bad


def test_descriptor_taps_are_the_oracles(oracle):
    from animal_vision_amd import _lib
    from animal_vision_amd.dichromat import DichromatOp, NightSpec
    from animal_vision_amd.animals import Dog

    op = DichromatOp(Dog.SPEC, night=NightSpec(bloom=0.12))
    nd = op.night_desc
    assert nd.struct_size == ctypes.sizeof(_lib.NightDesc) and (nd.rod_ksize, nd.bloom_ksize) == (11, 25)
    assert (nd.chroma_scale, nd.luminance_boost, nd.gamma, nd.bloom_strength) == (0.07, 1.8, 0.7, 0.12)
    rod = np.ctypeslib.as_array(nd.rod_taps_host, (11,))
    bloom = np.ctypeslib.as_array(nd.bloom_taps_host, (25,))
    # the library rounds the double taps to float32, as cv::getGaussianKernel's caller does
    assert np.array_equal(rod.astype(np.float32), oracle.gaussian_kernel(11, 1.2)) and np.array_equal(rod, oracle.gaussian_kernel(11, 1.2, np.float64))
    assert np.array_equal(bloom.astype(np.float32), oracle.gaussian_kernel(25, 3.0)) and np.array_equal(bloom, oracle.gaussian_kernel(25, 3.0, np.float64))
    assert oracle.cv_auto_ksize(1.2) == 11 and oracle.cv_auto_ksize(3.0) == 25  # what cv2.GaussianBlur((0, 0), sigma) resolves to
    with pytest.raises(TypeError):
        DichromatOp(Dog.SPEC, night=True)  # the op takes a NightSpec; True is the species constructors' shorthand


def test_video_parser_night_and_bloom(capsys):
    from animal_vision_amd.video import parse_args

    base = ["in.y4m", "out.y4m", "--species"]
    a = parse_args(base + ["Dog"])
    assert a.night is False and a.bloom is None
    a = parse_args(base + ["Dog", "--night"])
    assert a.night is True and a.bloom is None
    a = parse_args(base + ["Cat", "--night", "--bloom", "0.12", "--batch", "4", "--split-compare"])
    assert a.night is True and a.bloom == 0.12 and a.batch == 4
    assert parse_args(base + ["Rat", "--night", "--bloom", "1"]).bloom == 1.0

    def refused(argv, *words):
        with pytest.raises(SystemExit) as e:
            parse_args(argv)
        assert e.value.code == 2
        err = capsys.readouterr().err
        for w in words:
            assert w in err, (argv, err)

    refused(base + ["Dog", "--bloom", "0.12"], "--bloom needs --night")
    refused(base + ["HoneyBee", "--night"], "--night", "HoneyBee", "not one of the 20 dichromats")
    refused(base + ["Mantis Shrimp", "--night", "--bloom", "0.3"], "Mantis Shrimp", "not one of the 20 dichromats")
    refused(base + ["Dog", "--night", "--bloom", "0"], "--bloom must be above 0 and at most 1")
    refused(base + ["Dog", "--night", "--bloom", "1.5"], "--bloom must be above 0 and at most 1")
    refused(base + ["Dog", "--night", "--bloom", "lots"], "--bloom takes a number")


def test_all_twenty_dichromats_take_night():
    from animal_vision_amd.animals._dichromats import _Dichromat
    from animal_vision_amd.dichromat import NightSpec
    from animal_vision_amd.video import SPECIES_NAMES, is_dichromat, species_class

    names = [n for n in SPECIES_NAMES if is_dichromat(n)]
    assert len(names) == 20 and len(SPECIES_NAMES) == 36
    for n in names:
        sp = species_class(n)(night=True)
        assert isinstance(sp, _Dichromat) and sp.night == NightSpec()
        assert sp._operator().night == NightSpec() and sp._operator().night_desc.bloom_strength == 0.0


def test_make_animal_builds_the_night_species():
    from animal_vision_amd.animals import Cat, Dog
    from animal_vision_amd.dichromat import NightSpec
    from animal_vision_amd.video import has_stream_op, make_animal, parse_args, route

    dog = make_animal(parse_args(["in.y4m", "out.y4m", "--species", "Dog", "--night", "--bloom", "0.12"]))
    assert type(dog) is Dog and dog.night == NightSpec(bloom=0.12) and route(dog) == "dichromat"
    cat = make_animal(parse_args(["in.y4m", "out.y4m", "--species", "Cat", "--night"]))
    assert type(cat) is Cat and cat.night == NightSpec() and has_stream_op(cat)
    day = make_animal(parse_args(["in.y4m", "out.y4m", "--species", "Dog"]))
    assert type(day) is Dog and day.night is None


def test_entry_point_is_declared_and_exported():
    from animal_vision_amd import _lib

    res, args = _lib._SIGS["avx_dichromat_night_u8"]
    assert res is _lib._i and len(args) == 9
    assert args[6] == ctypes.POINTER(_lib.DichromatDesc) and args[7] == ctypes.POINTER(_lib.NightDesc)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"avx_dichromat_night_u8", "avx_dichromat_u8"} <= syms
    assert _lib.lib.avx_abi_version() == 1
    assert _lib.lib.avx_dichromat_night_u8(None, None, None, 1, 16, 16, None, None, None) == _lib.AVX_ERR_INVALID
    # the struct as the header lays it out on LP64: uint32 + pad, 3 doubles, int32 + pad, pointer, double, int32 + pad, pointer
    assert ctypes.sizeof(_lib.NightDesc) == 72 and _lib.NightDesc.rod_taps_host.offset == 40 and _lib.NightDesc.bloom_taps_host.offset == 64


def test_day_constructors_are_unchanged():
    from animal_vision_amd.animals import Cat, Dog
    from animal_vision_amd.dichromat import DichromatOp

    dog = Dog()
    assert dog.night is None and dog._op is None and callable(dog.visualize)
    op = DichromatOp(Dog.SPEC)
    assert op.night is None and op.night_desc is None and op.max_batch == 16 and op.desc.in_f32 == 0
    assert dog._operator().night is None
    assert Cat().night is None and Dog(night=False).night is None
    with pytest.raises(TypeError):
        Dog(night=0.12)  # a strength is NightSpec(bloom=...)'s to carry
    with pytest.raises(TypeError):
        Dog(True)  # keyword only: the positional surface of the reference's constructors is unchanged


@pytest.mark.parametrize("name", ["dog", "sheep", "rat", "rabbit", "cat"])
def test_reference_black_stays_black(oracle, name):
    sp = oracle.DICHROMATS[name]
    black = N.frames("black", 13, 17)
    for bloom in (0.0, 0.3):
        assert not N.night_ref(sp, black, bloom=bloom).any(), (name, bloom)


@pytest.mark.parametrize("name", ["dog", "sheep", "rat", "rabbit", "cat"])
def test_reference_bloom_is_gated_by_the_mask(oracle, name):
    """Where L709 never exceeds 0.4 behind the post stage the mask is exactly 0, and the bloom changes nothing."""
    sp = oracle.DICHROMATS[name]
    dark = N.frames("dark", 37, 70)
    lin = np.clip(N.night_lin(sp, dark).astype(np.float32), 0.0, 1.0)
    L = 0.2126 * lin[..., 0] + 0.7152 * lin[..., 1] + 0.0722 * lin[..., 2]
    assert L.max() <= 0.4, float(L.max())
    base = N.night_ref(sp, dark)
    assert base.max() > 40  # the rod stage lifts a dim scene: this is not a black frame
    for bloom in (0.12, 0.3):
        assert np.array_equal(N.night_ref(sp, dark, bloom=bloom), base), (name, bloom)
    lamps = N.frames("lamps", 37, 70)
    d = np.abs(N.night_ref(sp, lamps, bloom=0.3).astype(int) - N.night_ref(sp, lamps).astype(int))
    assert d.max() >= 4, (name, int(d.max()))  # and where the mask opens, the bloom is visible in the codes
