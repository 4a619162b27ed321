"""A NumPy model of the plane-program ISA (include/avx.h, csrc/ew.hip), a fuzzer of expression DAGs and the small program builder
the GPU tests share.  Test infrastructure: nothing here touches the device, and the module imports nothing from the package (the
builder at the bottom binds the ctypes structures when it is called).

The ISA, as read off csrc/ew.hip::k_ew (DESIGN.md "plane-program ISA" says the same in prose):

* 32 float32 registers per pixel, all 0 at the start; an accumulator register starts at +inf (min), -inf (max) or 0 (sum, mean).
* `op | IMM_A` / `op | IMM_B` (binary opcodes only, never both): operand a / b is float32(imm bits) instead of a register.
* Every instruction is ONE float32 operation.  MIN / MAX are C fminf / fmaxf: a NaN operand is ignored (np.fmin / np.fmax, not
  np.minimum), and the sign of min(-0, +0) is unspecified.  Comparisons with a NaN give 0.  NOT(NaN) = 0, AND / OR take NaN as true,
  SELECT with a NaN condition takes operand b (NaN != 0), CLIP01(NaN) = NaN and CLIP01(-0) = -0.
* SELECT: dst = a != 0 ? b : reg[imm & 0xff].  SCALAR: float32(table[slot]) of a float64 table.  CONST: the imm bits.
* LOAD: f32 `ptr[i * stride]`, u8 `float(byte)`, u8_lut `table0[byte]`, col `ptr[i % W]`, row `ptr[i // W]`.
* STORE: f32 with stride; u8_enc = #{k : table1[k] <= clip(x, 0, 1)} = searchsorted(table1, clip(x), "right"), NaN -> 0.
* ACCMIN / ACCMAX / ACCSUM fold operand a of every valid pixel into the accumulator register."""
import numpy as np

OPS = ("CONST SCALAR LOAD STORE ADD SUB MUL DIV MIN MAX POW ATAN2 NEG ABS SQRT EXP LOG SIN COS FLOOR CEIL CLIP01 TANH "
       "LT LE GT GE EQ AND OR NOT SELECT ACCMIN ACCMAX ACCSUM").split()
OP = {name: i + 1 for i, name in enumerate(OPS)}
NAME = {v: k for k, v in OP.items()}
IMM_A, IMM_B, OPCODE_MASK = 0x40, 0x80, 0x3F
KINDS = ("f32", "u8", "u8_lut", "col", "row", "u8_enc")
ACC_KINDS = ("min", "max", "sum", "mean")
N_REGS = 32

f32 = np.float32


def _mask(m):
    return m.astype(np.float32)


def _clip01(x):
    return np.where(x < 0, f32(0), np.where(x > 1, f32(1), x)).astype(np.float32)


UNARY_FN = {
    "NEG": np.negative, "ABS": np.abs, "SQRT": np.sqrt, "EXP": np.exp, "LOG": np.log, "SIN": np.sin, "COS": np.cos, "FLOOR": np.floor,
    "CEIL": np.ceil, "CLIP01": _clip01, "TANH": np.tanh, "NOT": lambda x: _mask(~(x != 0)),
}
BINARY_FN = {
    "ADD": np.add, "SUB": np.subtract, "MUL": np.multiply, "DIV": np.divide, "MIN": np.fmin, "MAX": np.fmax, "POW": np.power,
    "ATAN2": np.arctan2, "LT": lambda x, y: _mask(x < y), "LE": lambda x, y: _mask(x <= y), "GT": lambda x, y: _mask(x > y),
    "GE": lambda x, y: _mask(x >= y), "EQ": lambda x, y: _mask(x == y), "AND": lambda x, y: _mask((x != 0) & (y != 0)),
    "OR": lambda x, y: _mask((x != 0) | (y != 0)),
}
# planevm's node names
UNARY_NODE = {"neg": "NEG", "abs": "ABS", "sqrt": "SQRT", "exp": "EXP", "log": "LOG", "sin": "SIN", "cos": "COS", "floor": "FLOOR", "ceil": "CEIL",
              "clip01": "CLIP01", "tanh": "TANH", "not": "NOT"}
BINARY_NODE = {"add": "ADD", "sub": "SUB", "mul": "MUL", "div": "DIV", "min": "MIN", "max": "MAX", "pow": "POW", "atan2": "ATAN2", "lt": "LT",
               "le": "LE", "gt": "GT", "ge": "GE", "eq": "EQ", "and": "AND", "or": "OR"}
FULL_VOCABULARY = tuple(UNARY_NODE) + tuple(BINARY_NODE) + ("select",)
# the nodes whose result is exact in float32 on any IEEE machine (the device tests compare these bit for bit)
EXACT_VOCABULARY = ("neg", "abs", "sqrt", "floor", "ceil", "clip01", "not", "add", "sub", "mul", "div", "min", "max", "lt", "le", "gt", "ge", "eq",
                    "and", "or", "select")


def _op1(name, x):
    with np.errstate(all="ignore"):
        r = UNARY_FN[name](np.ascontiguousarray(x, np.float32))
    assert r.dtype == np.float32, name
    return r


def _op2(name, x, y):
    with np.errstate(all="ignore"):
        r = BINARY_FN[name](np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32))
    assert r.dtype == np.float32, name
    return r


def _select(c, x, y):
    return np.where(c != 0, x, y).astype(np.float32)


def bits_to_f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def f32_bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def special_values():
    """The operand table of the exactness tests: zeros, ones, infinities, NaN, the ends of the denormal and normal ranges, the
    neighbours of 1, and a few ordinary numbers (2^24 + 2: the first even integer above the contiguous range)."""
    tiny, big_den = bits_to_f32(1), bits_to_f32(0x007FFFFF)
    fmin, fmax = np.finfo(np.float32).tiny, np.finfo(np.float32).max
    v = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, tiny, -tiny, big_den, -big_den, fmin, -fmin, fmax, -fmax,
         np.nextafter(f32(1), f32(2)), np.nextafter(f32(1), f32(0)), 0.1, 3.0, -2.5, 2.0 ** 24 + 2]
    return np.array(v, np.float32)


def special_mix(rng, n, scale=4.0):
    """n float32 values: random normals with entries of the special table scattered through them (special_pairs gives the full
    cross product of the table instead)."""
    s = special_values()
    x = (rng.standard_normal(n) * scale).astype(np.float32)
    k = min(n, 4 * len(s))
    x[rng.choice(n, k, replace=False)] = s[rng.integers(0, len(s), k)]
    return x


def special_pairs(rng, n):
    """Two planes of n values: the cross product of the special table first, random normals behind it."""
    s = special_values()
    a, b = np.repeat(s, len(s)), np.tile(s, len(s))
    assert n >= len(a) + 200, "room for the cross product and a few hundred random pairs"
    x = np.concatenate([a, (rng.standard_normal(n - len(a)) * 3).astype(np.float32)])
    y = np.concatenate([b, (rng.standard_normal(n - len(b)) * 3).astype(np.float32)])
    return x.astype(np.float32), y.astype(np.float32)


def same_bits(got, want):
    """NaN in the same places, every other value bit for bit (so -0 != +0, and a flushed denormal is a difference) -> bool mask of
    the DIFFERING positions."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    gn, wn = np.isnan(got), np.isnan(want)
    return (gn != wn) | (~gn & ~wn & (got.view(u) != want.view(u)))


def assert_same_bits(got, want, what, operands=()):
    bad = same_bits(got, want)
    if bad.any():
        idx = np.flatnonzero(bad.ravel())[:6]
        rows = [(int(i), [repr(float(np.ravel(o)[i])) for o in operands], repr(float(np.ravel(got)[i])), repr(float(np.ravel(want)[i]))) for i in idx]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ; (index, operands, got, want): {rows}")


# ---------------------------------------------------------------------------------------------------------------- emulator --------
def emulate(insn, planes, acc, scalars, H, W, tables=None):
    """Execute a program on all H*W pixels at once.

    insn: (op, dst, a, b, imm) tuples as in avx_ew_insn.  planes: one dict per plane with `kind` (a name of KINDS), `stride` and
    `data`: the 1-D array that begins at the plane's pointer (float32, or uint8 for u8 / u8_lut; absent for a plane that is only
    stored).  acc: (register, kind name, slot) triples.  scalars: the float64 table.  tables: {0: decode LUT, 1: float32 encode
    thresholds}, passed in by the caller (runtime.get_table).
    -> (stored, streams): stored[plane index] = the n values written (float32, or uint8 codes for u8_enc); streams[k] = the values,
    pixel by pixel, that accumulator k folded (the caller reduces them as it sees fit)."""
    n = H * W
    i = np.arange(n)
    R = np.zeros((N_REGS, n), np.float32)
    init = {"min": np.inf, "max": -np.inf, "sum": 0.0, "mean": 0.0}
    acc_of = {}
    for k, (reg, kind, _slot) in enumerate(acc):
        R[reg] = f32(init[kind])
        acc_of[reg] = k
    stored, streams = {}, [[] for _ in acc]
    for op, dst, a, b, imm in insn:
        o, name = op & OPCODE_MASK, NAME[op & OPCODE_MASK]
        ia, ib = bool(op & IMM_A), bool(op & IMM_B)
        assert not (ia and ib) and (not (ia or ib) or name in BINARY_FN), ("immediate flag", name)
        immf = np.full(n, bits_to_f32(imm), np.float32)
        x = immf if ia else R[a]
        y = immf if ib else R[b]
        if name == "CONST":
            r = immf
        elif name == "SCALAR":
            with np.errstate(all="ignore"):
                r = np.full(n, np.float64(scalars[imm]).astype(np.float32), np.float32)
        elif name == "LOAD":
            p = planes[imm]
            kind, st = p["kind"], p["stride"]
            if kind == "f32":
                r = stored[imm].copy() if imm in stored else np.asarray(p["data"], np.float32)[: (n - 1) * st + 1: st].copy()
            elif kind == "u8":
                r = np.asarray(p["data"], np.uint8)[: (n - 1) * st + 1: st].astype(np.float32)
            elif kind == "u8_lut":
                r = np.asarray(tables[0], np.float32)[np.asarray(p["data"], np.uint8)[: (n - 1) * st + 1: st]]
            elif kind == "col":
                r = np.asarray(p["data"], np.float32)[i % W]
            elif kind == "row":
                r = np.asarray(p["data"], np.float32)[i // W]
            else:
                raise ValueError(f"LOAD from a {kind} plane")
            assert r.shape == (n,)
        elif name == "STORE":
            kind = planes[imm]["kind"]
            if kind == "f32":
                stored[imm] = x.copy()
            elif kind == "u8_enc":
                v = np.where(np.isnan(x), f32(0), _clip01(x))
                stored[imm] = np.searchsorted(np.asarray(tables[1], np.float32), v, side="right").astype(np.uint8)
            else:
                raise ValueError(f"STORE to a {kind} plane")
            continue
        elif name in BINARY_FN:
            r = _op2(name, x, y)
        elif name in UNARY_FN:
            r = _op1(name, x)
        elif name == "SELECT":
            r = _select(x, y, R[imm & 0xFF])
        else:  # ACCMIN / ACCMAX / ACCSUM
            k = acc_of[dst]
            streams[k].append(x.copy())
            r = _op2({"ACCMIN": "MIN", "ACCMAX": "MAX", "ACCSUM": "ADD"}[name], R[dst], x)
        R[dst] = r
    return stored, [np.concatenate(s) if s else np.zeros(0, np.float32) for s in streams]


def program_of(comp):
    """(insn tuples, plane refs, accumulator triples with kind NAMES) of a planevm._Compiled."""
    insn = [(int(t.op), int(t.dst), int(t.a), int(t.b), int(t.imm)) for t in comp.insn[: comp.n_insn]]
    n_acc = int(comp.program.n_acc)
    acc = [(int(comp.acc[3 * k]), ACC_KINDS[int(comp.acc[3 * k + 1])], int(comp.acc[3 * k + 2])) for k in range(n_acc)]
    return insn, list(comp._keep), acc


# ---------------------------------------------------------------------------------------------------------------- DAG fuzzer ------
CONSTANTS = (0.0, -0.0, 1.0, -1.0, 0.5, 2.0, -2.5, 0.1, 3.0, 1e-3, 255.0, 1.7)


def random_dag(rng, be, vocabulary, n_nodes, live_tail=0):
    """A random expression DAG of planevm.Val nodes on backend `be` (a DeviceBackend, or a stub with const / load / scalar /
    new_planes / new_slot).

    Leaves: 1-5 loaded planes, one scalar slot, float32 constants.  Interior: `n_nodes` nodes drawn from `vocabulary` (node names of
    planevm: the unary and binary tables and "select"), operands picked from everything built so far -- half of the time from the
    last few values, so chains form, otherwise from anywhere, so old values stay live and sub-expressions are shared.  A binary
    node takes a constant on either side now and then (the immediate forms), rarely on both (a CONST register).  Every min / max
    is wrapped as `node + 0.0`: the sign of min(-0, +0) is unspecified, and -0 + 0 = +0 either way.  live_tail > 0 appends
    ((v[-1] + v[-2]) + ...) + v[-live_tail] over the last values of the pool: all of them are live until the sum reaches them.
    Outputs: 1-5 values (the tail sum among them), each stored to a plane of its own or reduced (min / max / sum / mean).
    -> dict(planes=[PlaneRef], slot=int, outputs=[("store", Val, PlaneRef) | ("acc", Val, kind, slot)])"""
    refs = be.new_planes(int(rng.integers(1, 6)))
    slot = be.new_slot()
    pool = [be.load(r) for r in refs] + [be.scalar(slot)]
    Val = type(pool[0])
    n_leaves = len(pool)

    def const():
        return be.const(float(np.float32(CONSTANTS[int(rng.integers(len(CONSTANTS)))])))

    def pick():
        if rng.random() < 0.5:
            return pool[-1 - int(rng.integers(min(len(pool), 5)))]
        return pool[int(rng.integers(len(pool)))]

    for _ in range(n_nodes):
        op = vocabulary[int(rng.integers(len(vocabulary)))]
        if op in UNARY_NODE:
            v = Val(be, op, (const() if rng.random() < 0.03 else pick(),))
        elif op in BINARY_NODE:
            a, b, u = pick(), pick(), rng.random()
            if u < 0.2:
                a = const()
            elif u < 0.4:
                b = const()
            elif u < 0.43:
                a, b = const(), const()
            v = Val(be, op, (a, b))
        else:
            v = Val(be, "select", tuple(const() if rng.random() < 0.15 else pick() for _ in range(3)))
        if op in ("min", "max"):
            v = Val(be, "add", (v, be.const(0.0)))
        pool.append(v)
    picks = []
    if live_tail > 0:
        tail = pool[-live_tail:]
        s = tail[-1]
        for v in reversed(tail[:-1]):
            s = Val(be, "add", (s, v))
        pool.append(s)
        picks.append(s)
    n_out = int(rng.integers(1, 6))
    while len(picks) < n_out:
        picks.append(pool[int(rng.integers(n_leaves if len(pool) > n_leaves else 0, len(pool)))])
    outputs = []
    for v in picks:
        if rng.random() < 0.5:
            outputs.append(("store", v, be.new_planes(1)[0]))
        else:
            outputs.append(("acc", v, ACC_KINDS[int(rng.integers(4))], be.new_slot()))
    return {"planes": refs, "slot": slot, "outputs": outputs}


def eval_dag(val, plane_values, scalars, n, memo=None):
    """The value of a Val graph, node by node, with the emulator's own NumPy functions.  plane_values: {PlaneRef.uid: n float32
    values}; scalars: the float64 table; memo: {id(Val): array}, shared between the outputs of one DAG."""
    memo = {} if memo is None else memo
    stack = [val]
    while stack:
        v = stack[-1]
        if id(v) in memo:
            stack.pop()
            continue
        todo = [a for a in v.args if id(a) not in memo]
        if todo:
            stack.extend(todo)
            continue
        stack.pop()
        args = [memo[id(a)] for a in v.args]
        if v.op == "const":
            r = np.full(n, np.float32(v.imm), np.float32)
        elif v.op == "scalar":
            with np.errstate(all="ignore"):
                r = np.full(n, np.float64(scalars[v.imm]).astype(np.float32), np.float32)
        elif v.op == "load":
            r = np.ascontiguousarray(plane_values[v.imm.uid], np.float32)
        elif v.op in UNARY_NODE:
            r = _op1(UNARY_NODE[v.op], args[0])
        elif v.op in BINARY_NODE:
            r = _op2(BINARY_NODE[v.op], args[0], args[1])
        elif v.op == "select":
            r = _select(*args)
        else:
            raise ValueError(v.op)
        memo[id(v)] = r
    return memo[id(val)]


# ---------------------------------------------------------------------------------------------------------------- program builder -
def assemble(H, W, ins, planes, acc, scalars_ptr, n_scalars):
    """An avx_ew_program from (op, dst, a, b, imm) tuples, (device pointer, stride, kind code) planes and a flat accumulator list
    [register, kind code, slot, ...] -> (program, the ctypes arrays it points into: keep them alive)."""
    import ctypes

    from animal_vision_amd._lib import EwInsn, EwPlane, EwProgram

    a_ins = (EwInsn * max(1, len(ins)))(*[EwInsn(*t) for t in ins])
    a_pl = (EwPlane * max(1, len(planes)))(*[EwPlane(*t) for t in planes])
    a_acc = (ctypes.c_int32 * max(1, len(acc)))(*acc)
    p = EwProgram()
    p.struct_size = ctypes.sizeof(EwProgram)
    p.H, p.W = H, W
    p.n_insn, p.insn_host = len(ins), ctypes.cast(a_ins, ctypes.POINTER(EwInsn))
    p.n_planes, p.planes_host = len(planes), ctypes.cast(a_pl, ctypes.POINTER(EwPlane))
    p.n_acc, p.acc_host = len(acc) // 3, ctypes.cast(a_acc, ctypes.POINTER(ctypes.c_int32))
    p.scalars_dev, p.n_scalars = scalars_ptr, n_scalars
    return p, (a_ins, a_pl, a_acc)


def reduction_program(H, W, planes, scalars_ptr, n_scalars):
    """x * col + row, times a per-frame scalar (slot 8); stored, and min / max / sum of it plus the mean of x accumulated into
    slots 0..3.  Its structure is recorded in csrc/ew_programs.txt, so it has a generated kernel."""
    from animal_vision_amd._lib import EW, EW_ACC

    ins = [(EW["LOAD"], 0, 0, 0, 0), (EW["LOAD"], 1, 0, 0, 1), (EW["LOAD"], 2, 0, 0, 2), (EW["MUL"], 3, 0, 1, 0), (EW["ADD"], 3, 3, 2, 0),
           (EW["SCALAR"], 4, 0, 0, 8), (EW["MUL"], 3, 3, 4, 0), (EW["STORE"], 0, 3, 0, 3),
           (EW["ACCMIN"], 5, 3, 0, 0), (EW["ACCMAX"], 6, 3, 0, 0), (EW["ACCSUM"], 7, 3, 0, 0), (EW["ACCSUM"], 8, 0, 0, 0)]
    acc = [5, EW_ACC["min"], 0, 6, EW_ACC["max"], 1, 7, EW_ACC["sum"], 2, 8, EW_ACC["mean"], 3]
    return assemble(H, W, ins, planes, acc, scalars_ptr, n_scalars)


def spec_stats():
    """(hits, misses) of the generated-kernel lookup so far."""
    import ctypes

    from animal_vision_amd._lib import lib

    h, m = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    lib.avx_ew_spec_stats(ctypes.byref(h), ctypes.byref(m))
    return h.value, m.value


def parse_recorded(line):
    """One line of csrc/ew_programs.txt, as tools/gen_ew_kernels.py::parse reads it -> (insn tuples with the structural imm, plane
    kind codes, (register, kind code) accumulators)."""
    head, insn, planes, accs = [s.strip() for s in line.split(":")]
    ins = [tuple(int(v) for v in t.split(",")) for t in insn.split()]
    kinds = [int(v) for v in planes.split()]
    acc = [tuple(int(v) for v in t.split(",")) for t in accs.split()]
    assert [len(ins), len(kinds), len(acc)] == [int(v) for v in head.split()], line[:80]
    return ins, kinds, acc
