"""CPU: planevm._Compiled, the lowering of expression DAGs to register programs, against tests/_ew_ref.py.

No device: the compiler is built against a stub backend (it only needs H, W, N_SCALARS, scalars.ptr, frame_stride() and const()),
its output is executed by the NumPy emulator of the ISA and compared with a direct evaluation of the DAG, bit for bit.  The
register allocator (operand-register reuse, immediates without a register, accumulators above the temporaries, the 16- or
32-register choice) is what stands between the two."""
import numpy as np
import pytest

import _ew_ref as R

H, W = 4, 16
N = H * W
SEEDS = 2000


class _Buf:
    """Stand-in for a DeviceBuffer: an address nobody dereferences."""
    _next = 1 << 20

    def __init__(self, nbytes):
        self.ptr, self.nbytes = _Buf._next, nbytes
        _Buf._next += (nbytes + 255) // 256 * 256


class StubBackend:
    N_SCALARS = 256
    name = "stub"

    def __init__(self, H, W):
        from animal_vision_amd import planevm

        self._vm = planevm
        self.H, self.W, self.n = H, W, H * W
        self.scalars = _Buf(8 * self.N_SCALARS)
        self._slot = 0

    def const(self, v):
        return self._vm.Val(self, "const", (), float(v))

    def load(self, ref):
        return self._vm.Val(self, "load", (), ref)

    def scalar(self, slot):
        return self._vm.Val(self, "scalar", (), int(slot))

    def new_planes(self, k=1):
        b = _Buf(4 * self.n * k)
        return [self._vm.PlaneRef(b, 4 * self.n * i) for i in range(k)]

    def new_slot(self):
        self._slot += 1
        assert self._slot <= self.N_SCALARS
        return self._slot - 1

    def frame_stride(self, ref):
        return 0

    def compile(self, outputs):
        return self._vm._Compiled(self, outputs)


def _case(seed):
    """Seed -> (backend, DAG, compiled program or None when the allocator refuses it)."""
    rng = np.random.default_rng(seed)
    be = StubBackend(H, W)
    tail = seed % 2 == 1  # half of the seeds
    dag = R.random_dag(rng, be, R.FULL_VOCABULARY, int(rng.integers(4, 90)), int(rng.integers(8, 57)) if tail else 0)
    try:
        comp = be.compile(dag["outputs"])
    except ValueError as e:
        assert "live registers" in str(e), e
        comp = None
    return rng, be, dag, comp


def _check_structure(seed, comp, insn, refs, acc):
    acc_regs = [r for r, _, _ in acc]
    is_acc = lambda t: R.NAME[t[0] & R.OPCODE_MASK] in ("ACCMIN", "ACCMAX", "ACCSUM")  # noqa: E731
    temps = set()
    written = set()
    loads, scalars = [], []
    for pc, t in enumerate(insn):
        op, d, a, b, imm = t
        name = R.NAME[op & R.OPCODE_MASK]
        ia, ib = bool(op & R.IMM_A), bool(op & R.IMM_B)
        assert not (ia and ib), (seed, pc, "both immediate flags")
        assert not (ia or ib) or name in R.BINARY_FN, (seed, pc, name, "immediate flag on a non-binary opcode")
        reads = []
        if name in R.BINARY_FN:
            reads = ([] if ia else [a]) + ([] if ib else [b])
        elif name in R.UNARY_FN or name == "STORE" or is_acc(t):
            reads = [a]
        elif name == "SELECT":
            reads = [a, b, imm & 0xFF]
        for r in reads:
            assert r in written, (seed, pc, name, f"reads r{r} before anything wrote it")
            assert r not in acc_regs, (seed, pc, name, f"reads accumulator r{r}")
        if is_acc(t):
            assert d in acc_regs, (seed, pc)
        elif name != "STORE":
            assert d not in acc_regs, (seed, pc, name, f"temporary in accumulator register r{d}")
            written.add(d)
            temps.add(d)
        temps.update(reads)
        if name == "LOAD":
            loads.append(imm)
        if name == "SCALAR":
            scalars.append(imm)
    top = max(temps) + 1 if temps else 1
    assert acc_regs == list(range(top, top + len(acc))), (seed, "accumulators sit directly above the temporaries", top, acc_regs)
    assert comp.n_regs == top + len(acc) <= 32, (seed, comp.n_regs)
    assert len(set(loads)) == len(loads) and len({(refs[i].uid, refs[i].kind) for i in loads}) == len(loads), (seed, "one LOAD per distinct plane")
    assert len(set(scalars)) == len(scalars), (seed, "one SCALAR per slot")
    return top


@pytest.fixture(scope="module")
def corpus():
    """All seeds compiled, emulated and evaluated once; the tests below read the records."""
    rec = []
    for seed in range(SEEDS):
        rng, be, dag, comp = _case(seed)
        if comp is None:
            rec.append({"seed": seed, "refused": True})
            continue
        values = {r.uid: R.special_mix(rng, N) for r in dag["planes"]}
        table = rng.standard_normal(be.N_SCALARS) * 3.0
        insn, refs, acc = R.program_of(comp)
        planes = [{"kind": r.kind, "stride": r.stride, "data": values.get(r.uid)} for r in refs]
        stored, streams = R.emulate(insn, planes, acc, table, H, W)
        memo, diffs = {}, []
        k_acc = 0
        for o in dag["outputs"]:
            want = R.eval_dag(o[1], values, table, N, memo)
            if o[0] == "store":
                idx = [i for i, r in enumerate(refs) if r.uid == o[2].uid]
                got = stored[idx[0]]
            else:
                assert acc[k_acc][1:] == (o[2], o[3]), (seed, "accumulator order / kind / slot", acc[k_acc], o[2:])
                got = streams[k_acc]
                k_acc += 1
            diffs.append(int(R.same_bits(got, want).sum()))
        assert k_acc == len(acc)
        rec.append({"seed": seed, "refused": False, "comp": comp, "insn": insn, "refs": refs, "acc": acc, "diffs": diffs, "n_out": len(dag["outputs"])})
    return rec


def test_lowering_preserves_meaning(corpus):
    """emulate(compiled) == eval_dag for every stored plane and, pixel by pixel, for every reduced stream: same NaN positions, same
    bits elsewhere.  The counts keep the corpus honest: a change to the fuzzer cannot quietly take the hard programs out."""
    bad = [(r["seed"], r["diffs"]) for r in corpus if not r["refused"] and any(r["diffs"])]
    assert not bad, f"{len(bad)} programs compute something else than their DAG; (seed, differing pixels per output): {bad[:8]}"
    ok = [r for r in corpus if not r["refused"]]
    wide = sum(r["comp"].n_regs > 16 for r in ok)
    refused = len(corpus) - len(ok)
    assert len(corpus) >= 2000 and wide > 200 and refused >= 1, (len(corpus), wide, refused)
    assert max(r["comp"].n_insn for r in ok) >= 100
    seen = {}
    for r in ok:
        for t in r["insn"]:
            seen.setdefault(R.NAME[t[0] & R.OPCODE_MASK], set()).add(t[0] & (R.IMM_A | R.IMM_B))
    assert set(seen) == set(R.OPS), sorted(set(R.OPS) - set(seen))
    for name in R.BINARY_FN:
        assert seen[name] == {0, R.IMM_A, R.IMM_B}, (name, "not seen in every operand form", seen[name])


def test_structural_invariants(corpus):
    """No read of a temporary nobody wrote, accumulators disjoint from and directly above the temporaries, n_regs <= 32, immediate
    flags on binary opcodes only and never both, one LOAD per plane and one SCALAR per slot; and a program whose temporaries and
    accumulators fit 16 registers names none above 15 in any field, so avx_ew_run gives it the 16-register kernel."""
    fits = 0
    for r in corpus:
        if r["refused"]:
            continue
        top = _check_structure(r["seed"], r["comp"], r["insn"], r["refs"], r["acc"])
        assert top + len(r["acc"]) == r["comp"].n_regs
        if r["comp"].n_regs <= 16:
            fits += 1
            hi = max(max(t[1], t[2], t[3], (t[4] & 0xFF) if R.NAME[t[0] & R.OPCODE_MASK] == "SELECT" else 0) for t in r["insn"])
            assert hi <= 15, (r["seed"], "a program that fits 16 registers must get the 16-register kernel", hi)
    assert fits > 500, fits


def test_programs_are_compact(corpus):
    """`top` is not just some bound: every temporary register below it is really needed at the moment it is first used -- when an
    instruction writes register r for the first time, all of r0..r(r-1) hold a value that is read later (or is an operand of this
    very instruction).  So a program whose peak of live values, plus its accumulators, fits 16 registers uses none above 15."""
    for r in corpus:
        if r["refused"]:
            continue
        insn = r["insn"]
        reads_at = []
        for t in insn:
            name = R.NAME[t[0] & R.OPCODE_MASK]
            if name in R.BINARY_FN:
                reads_at.append(([] if t[0] & R.IMM_A else [t[2]]) + ([] if t[0] & R.IMM_B else [t[3]]))
            elif name in R.UNARY_FN or name in ("STORE", "ACCMIN", "ACCMAX", "ACCSUM"):
                reads_at.append([t[2]])
            elif name == "SELECT":
                reads_at.append([t[2], t[3], t[4] & 0xFF])
            else:
                reads_at.append([])
        first_seen = set()
        for pc, t in enumerate(insn):
            name = R.NAME[t[0] & R.OPCODE_MASK]
            if name in ("STORE", "ACCMIN", "ACCMAX", "ACCSUM") or t[1] in first_seen:
                continue
            first_seen.add(t[1])
            for lower in range(t[1]):
                # `lower` must be busy: read by this instruction or by a later one before it is written again
                busy = lower in reads_at[pc]
                for q in range(pc + 1, len(insn)):
                    if busy or lower in reads_at[q]:
                        busy = True
                        break
                    qn = R.NAME[insn[q][0] & R.OPCODE_MASK]
                    if qn not in ("STORE", "ACCMIN", "ACCMAX", "ACCSUM") and insn[q][1] == lower:
                        break
                assert busy, (r["seed"], pc, f"r{t[1]} opened while r{lower} was free")


def _single(build):
    """Compile one expression of a plane x (and the scalar s) -> instruction tuples without the LOAD / STORE around it."""
    be = StubBackend(H, W)
    ref, out = be.new_planes(2)
    x = be.load(ref)
    comp = be.compile([("store", build(be, x), out)])
    insn, _, _ = R.program_of(comp)
    return [(R.NAME[t[0] & R.OPCODE_MASK], t[0] & (R.IMM_A | R.IMM_B), t) for t in insn]


def test_val_operator_surface():
    body = lambda build: [(n, f, t) for n, f, t in _single(build) if n not in ("LOAD", "STORE")]  # noqa: E731
    imm = lambda t: float(R.bits_to_f32(t[4]))  # noqa: E731

    (n, f, t), = body(lambda be, x: x ** 2)
    assert (n, f) == ("MUL", 0) and t[2] == t[3]
    (n, f, t), = body(lambda be, x: x ** 0.5)
    assert (n, f) == ("SQRT", 0)
    (n, f, t), = body(lambda be, x: x ** -1)
    assert (n, f) == ("DIV", R.IMM_A) and imm(t) == 1.0
    # ** 1 is the value itself: the program is LOAD, STORE of the same register
    prog = _single(lambda be, x: x ** 1)
    assert [n for n, _, _ in prog] == ["LOAD", "STORE"] and prog[1][2][2] == prog[0][2][1]
    for p in (2.4, 3, -0.5, 1 / 2.4):
        (n, f, t), = body(lambda be, x, p=p: x ** p)
        assert (n, f) == ("POW", R.IMM_B) and imm(t) == float(np.float32(p)), p
    # reflected operators: the constant stays on the side it was written on
    for build, name, flag, c in ((lambda be, x: 2 - x, "SUB", R.IMM_A, 2.0), (lambda be, x: x - 2, "SUB", R.IMM_B, 2.0),
                                 (lambda be, x: 2 / x, "DIV", R.IMM_A, 2.0), (lambda be, x: x / 2, "DIV", R.IMM_B, 2.0),
                                 (lambda be, x: 2 + x, "ADD", R.IMM_A, 2.0), (lambda be, x: 3 * x, "MUL", R.IMM_A, 3.0),
                                 (lambda be, x: x < 2, "LT", R.IMM_B, 2.0), (lambda be, x: x >= 2, "GE", R.IMM_B, 2.0),
                                 # Python swaps the comparison: 2 < x is x.__gt__(2), 2 >= x is x.__le__(2)
                                 (lambda be, x: 2 < x, "GT", R.IMM_B, 2.0), (lambda be, x: 2 >= x, "LE", R.IMM_B, 2.0),
                                 (lambda be, x: np.float32(0.1) - x, "SUB", R.IMM_A, float(np.float32(0.1))),
                                 (lambda be, x: np.float64(0.1) / x, "DIV", R.IMM_A, float(np.float32(0.1)))):
        (n, f, t), = body(build)
        assert (n, f, imm(t)) == (name, flag, c), (name, flag, c, n, f, imm(t))
    # and they mean it: 2 - x and 2 / x on numbers
    be = StubBackend(H, W)
    ref, o1, o2, o3 = be.new_planes(4)
    x = be.load(ref)
    comp = be.compile([("store", 2 - x, o1), ("store", 2 / x, o2), ("store", (2 < x) & ~(x >= 3), o3)])
    insn, refs, acc = R.program_of(comp)
    xv = np.linspace(-4, 4, N).astype(np.float32)
    stored, _ = R.emulate(insn, [{"kind": r.kind, "stride": r.stride, "data": xv} for r in refs], acc, np.zeros(4), H, W)
    by_uid = {refs[i].uid: v for i, v in stored.items()}
    with np.errstate(all="ignore"):
        assert np.array_equal(by_uid[o1.uid], np.float32(2) - xv) and np.array_equal(by_uid[o2.uid], np.float32(2) / xv)
        assert np.array_equal(by_uid[o3.uid], ((xv > 2) & ~(xv >= 3)).astype(np.float32))
    with pytest.raises(TypeError):
        bool(x)
    with pytest.raises(TypeError):
        if x > 1:  # the idiom that must not silently pick a branch
            pass
    with pytest.raises(TypeError):
        x + "1"


def test_emulator_opcode_numbers_are_the_librarys():
    from animal_vision_amd import _lib

    assert R.OP == _lib.EW and {k: i for i, k in enumerate(R.KINDS)} == _lib.EW_PLANE and {k: i for i, k in enumerate(R.ACC_KINDS)} == _lib.EW_ACC
    assert R.N_REGS == _lib.AVX_EW_MAX_REGS


def test_emulator_special_value_rules():
    """The NaN and zero rules of the ISA as the emulator states them (the device is held to the emulator in test_ew_isa_gpu.py)."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    x = np.array([nan, 1.0, nan, -0.0, 0.0, 2.0], np.float32)
    y = np.array([1.0, nan, nan, 0.0, -0.0, 2.0], np.float32)
    run = lambda name: R.emulate([(R.OP["LOAD"], 0, 0, 0, 0), (R.OP["LOAD"], 1, 0, 0, 1), (R.OP[name], 2, 0, 1, 0), (R.OP["STORE"], 0, 2, 0, 2)],  # noqa: E731
                                 [{"kind": "f32", "stride": 1, "data": x}, {"kind": "f32", "stride": 1, "data": y}, {"kind": "f32", "stride": 1}],
                                 [], np.zeros(1), 1, 6)[0][2]
    assert np.array_equal(run("MIN")[[0, 1, 5]], [1.0, 1.0, 2.0]) and np.isnan(run("MIN")[2]) and np.all(run("MIN")[3:5] == 0)
    assert np.array_equal(run("MAX")[[0, 1, 5]], [1.0, 1.0, 2.0]) and np.isnan(run("MAX")[2])
    for name in ("LT", "LE", "GT", "GE", "EQ"):
        assert np.array_equal(run(name)[:3], [0, 0, 0]), name
    assert np.array_equal(run("EQ")[3:], [1, 1, 1]) and np.array_equal(run("LE")[3:], [1, 1, 1]) and np.array_equal(run("LT")[3:], [0, 0, 0])
    assert np.array_equal(run("AND"), [1, 1, 1, 0, 0, 1]) and np.array_equal(run("OR"), [1, 1, 1, 0, 0, 1])
    assert np.array_equal(run("NOT"), [0, 0, 0, 1, 1, 0])  # of x
    c = run("CLIP01")
    assert np.isnan(c[0]) and np.signbit(c[3]) and c[5] == 1.0
    sel = R.emulate([(R.OP["LOAD"], 0, 0, 0, 0), (R.OP["CONST"], 1, 0, 0, R.f32_bits(7.0)), (R.OP["CONST"], 2, 0, 0, R.f32_bits(9.0)),
                     (R.OP["SELECT"], 3, 0, 1, 2), (R.OP["STORE"], 0, 3, 0, 1)],
                    [{"kind": "f32", "stride": 1, "data": x}, {"kind": "f32", "stride": 1}], [], np.zeros(1), 1, 6)[0][1]
    assert np.array_equal(sel, [7, 7, 7, 9, 9, 7])  # a NaN condition is "not zero": operand b
    # registers start at 0, accumulators at their identity; a scalar is rounded from float64
    st, streams = R.emulate([(R.OP["ADD"] | R.IMM_B, 1, 5, 0, R.f32_bits(1.5)), (R.OP["STORE"], 0, 1, 0, 0), (R.OP["SCALAR"], 2, 0, 0, 1),
                             (R.OP["STORE"], 0, 2, 0, 1), (R.OP["ACCMIN"], 9, 1, 0, 0), (R.OP["STORE"], 0, 9, 0, 2)],
                            [{"kind": "f32", "stride": 1}] * 3, [(9, "min", 0)], np.array([0.0, 0.1]), 1, 2)
    assert np.array_equal(st[0], [1.5, 1.5]) and np.array_equal(st[1], np.full(2, np.float32(0.1))) and np.array_equal(st[2], [1.5, 1.5])
    assert np.array_equal(streams[0], [1.5, 1.5]) and inf > 0
