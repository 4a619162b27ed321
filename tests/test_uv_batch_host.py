"""CPU: the batched plane-program interface as far as it can be checked without a GPU -- the four new C entry points exist,
are declared to ctypes and refuse a NULL context before touching anything; the kernel generator still emits one kernel per
recorded program under the same hash keys; the `video` command parses --batch."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["avx_ew_run_batch", "avx_uv_front_u8_batch", "avx_band_stack_batch", "avx_planes_gaussian_blur_batch"]


def test_new_entry_points_exported_declared_and_null_safe():
    from animal_vision_amd import _lib

    for name in NEW:
        fn = getattr(_lib.lib, name)  # AttributeError: the built library does not export it
        assert name in _lib._SIGS, name
        assert fn.argtypes is not None and len(fn.argtypes) == len(_lib._SIGS[name][1]) and fn.restype is ctypes.c_int, name
        # a NULL context is refused before any argument is looked at (no GPU is needed for this call)
        args = [None if t in (ctypes.c_void_p,) or hasattr(t, "contents") else 3 for t in fn.argtypes]
        assert fn(*args) == _lib.AVX_ERR_INVALID, name
    assert _lib.AVX_EW_MAX_FRAMES == 16
    hdr = open(os.path.join(ROOT, "include", "avx.h")).read()
    assert re.search(r"AVX_EW_MAX_FRAMES\s*=\s*16\b", hdr)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name


def _hash(ins, kinds, acc):
    """The structure hash of csrc/ew.hip::avx_ew_run_batch, restated: two FNV-1a style 64-bit hashes over the structure bytes."""
    M = (1 << 64) - 1
    h1, h2 = 0xcbf29ce484222325, 0x84222325cbf29ce4

    def mix(b):
        nonlocal h1, h2
        h1 = ((h1 ^ b) * 0x100000001b3) & M
        h2 = ((h2 ^ ((b + 0x9e) & 0xffffffff)) * 0x100000001b3) & M
        h2 ^= h2 >> 29

    for t in ins:
        for v in (t[0], t[1], t[2], t[3], t[4] & 0xff):
            mix(v)
    mix(0xff)
    for k in kinds:
        mix(k)
    mix(0xfe)
    for r, k in acc:
        mix(r)
        mix(k)
    return h1, h2


def test_generator_emits_one_kernel_per_recorded_program_same_keys(tmp_path):
    src = os.path.join(ROOT, "animal-vision_amd", "csrc", "ew_programs.txt")
    want = []
    for line in sorted({l.strip() for l in open(src) if l.strip() and not l.startswith("#")}):
        head, insn, planes, accs = [s.strip() for s in line.split(":")]
        ins = [tuple(int(v) for v in t.split(",")) for t in insn.split()]
        kinds = [int(v) for v in planes.split()]
        acc = [tuple(int(v) for v in t.split(",")) for t in accs.split()]
        assert [len(ins), len(kinds), len(acc)] == [int(v) for v in head.split()]
        want.append(_hash(ins, kinds, acc))
    want.sort()
    n_prog = len(want)
    assert n_prog >= 131 and len(set(want)) == n_prog  # the 131 structures of the species, plus what the test suite itself records
    # run the generator on a copy of the tree's two inputs: the committed tree is not written to
    work = tmp_path / "tree"
    (work / "tools").mkdir(parents=True)
    (work / "animal-vision_amd" / "csrc").mkdir(parents=True)
    for rel in (("tools", "gen_ew_kernels.py"), ("animal-vision_amd", "csrc", "ew_programs.txt")):
        (work.joinpath(*rel)).write_bytes(open(os.path.join(ROOT, *rel), "rb").read())
    subprocess.check_call([sys.executable, str(work / "tools" / "gen_ew_kernels.py")], stdout=subprocess.DEVNULL)
    gen = (work / "animal-vision_amd" / "csrc" / "ew_gen.hip").read_text()
    kernels = re.findall(r"^__global__ __launch_bounds__\(kET\) void (k_ews_\d+)\(const EwArgs a\)", gen, re.M)
    assert len(kernels) == n_prog and len(set(kernels)) == n_prog
    table = re.findall(r"\{0x([0-9a-f]{16})ull, 0x([0-9a-f]{16})ull, (k_ews_\d+)<4>, \3<8>\},", gen)
    assert [(int(a, 16), int(b, 16)) for a, b, _ in table] == want  # same keys, in the order the binary search needs
    assert sorted(k for _, _, k in table) == sorted(kernels)
    assert f"kEwSpecCount = {n_prog};" in gen
    # every kernel takes its frame from the grid and offsets planes, scalars and the reduction by it
    assert gen.count("const unsigned f = blockIdx.y;") == n_prog
    assert "a.planes[" not in gen and "ew_plane_of(a, 0, f)" in gen


def test_video_parser_batch_flag():
    from animal_vision_amd.video import build_parser

    ap = build_parser()
    base = ["in.y4m", "out.y4m", "--species", "HummingBird"]
    assert ap.parse_args(base).batch == 1
    assert ap.parse_args(base + ["--batch", "8"]).batch == 8
    assert ap.parse_args(base + ["--batch", "16"]).batch == 16
    for bad in ("0", "17", "-1", "x"):
        with pytest.raises(SystemExit):
            ap.parse_args(base + ["--batch", bad])


def test_batch_parameters_are_part_of_the_python_interface():
    """Signatures only (constructing any of these needs a device)."""
    import inspect

    from animal_vision_amd.animals._uv_species import SpeciesStreamOp, UVSpecies
    from animal_vision_amd.pipeline import FramePipeline, run_video
    from animal_vision_amd.planevm import DeviceBackend
    from animal_vision_amd.video import stream_op

    assert inspect.signature(DeviceBackend.__init__).parameters["frames"].default == 1
    assert inspect.signature(DeviceBackend.run_device).parameters["n_frames"].default is None
    assert inspect.signature(SpeciesStreamOp.__init__).parameters["batch"].default == 1
    assert inspect.signature(FramePipeline.__init__).parameters["batch"].default == 1
    assert inspect.signature(run_video).parameters["batch"].default == 1
    assert inspect.signature(stream_op).parameters["batch"].default == 1
    assert callable(UVSpecies.visualize_batch)
