"""Every expression operator at its edge operands (tests/math_lattice.py), on the CPU: the oracle against an independent numpy
reference, and the product's copy of the arithmetic (hnb_vm.h + hnb_math.h compiled for the host, CpuVmRunner) against the oracle,
bit for bit, through the streaming and the generic interpreter.

The pattern is tests/test_gpu_scale.py's math probe: one effect whose update evaluates the operators on per-particle input planes
(tests/helpers.py *_probe_asset); the test writes the planes, runs one frame and reads the output planes back. CASES binds each probe
to its operands and to the checks of its outputs; tests/test_gpu_math_lattice.py runs the same CASES on the GPU.

What is asserted against the reference:
  * transcendental functions: the NaN / inf / finite class at EVERY point, the sign of every zero, every finite point within the
    function's ulp bound (hanabi-math v3: sin cos asin atan atan2 2, tan 4, the others 1; pow 8, and 2 where |y log2 x| <= 32);
  * + - * / % sqrt 1/sqrt floor ceil round fract min max step sign saturate abs clamp mix smoothstep, conversions, integer
    operators, pack / unpack, dot / length / distance / normalize / cross: equal BITS (NaN compared as a class);
  * no point is left out: where the project's definition is not libm's, math_lattice.PINNED holds the value it is pinned to.
"""
import functools

import numpy as np
import pytest

import helpers
import math_lattice as ml
import oracle
from helpers import A, CpuVmRunner, Frame, OracleRunner

f32, u32 = np.float32, np.uint32


def _pad(plane, n):
    """a plane of n rows: the operands, then copies of the first row"""
    plane = np.asarray(plane)
    out = np.empty((n,) + plane.shape[1:], plane.dtype)
    out[:len(plane)] = plane
    out[len(plane):] = plane[0]
    return out


class Case:
    """asset(capacity): the probe; inputs: {attribute: operand plane}; checks: [(label, attribute, column or None, kind, reference, operands)],
    kind "libm" (class, zero sign, ulp bound, pins) or "bits" (float planes) or "words" (integer planes)."""

    def __init__(self, name, asset, inputs, checks):
        self.name, self.asset_fn, self.checks = name, asset, checks
        self.n = max(len(p) for p in inputs.values())
        self.inputs = {a: _pad(p, self.n) for a, p in inputs.items()}
        self.outputs = sorted({c[1] for c in checks}, key=lambda a: a.id)

    def asset(self):
        return self.asset_fn(self.n)

    def cut(self, rows):
        """the same case over a subset of its operand rows (a small effect: the shared launches of small programs)"""
        c = Case.__new__(Case)
        c.name, c.asset_fn, c.outputs, c.n = self.name, self.asset_fn, self.outputs, len(rows)
        c.inputs = {a: p[rows] for a, p in self.inputs.items()}
        c.checks = None   # (compared with the oracle only)
        return c


def _libm1(fn, attr, col, x):
    want, pinned = ml.apply_pins(fn, ml.ref_unary(fn, x), x)
    return (fn, attr, col, "libm", (want, pinned, None), (x,))


@functools.lru_cache(None)
def cases():
    out = {}
    # -- the transcendental builtins: helpers.math_probe_asset ------------------------------------------------------------------------------------
    trig, unit = np.concatenate([ml.trig_args(), ml.atan_args()]), ml.unit_args()
    expo, posi = np.concatenate([ml.exp_args(), ml.exp2_args()]), ml.log_args()
    ya, xa = ml.cross(ml.ATAN2_SET, ml.ATAN2_SET)
    yl, xl = ml.landmark_pairs()
    y2, x2 = np.concatenate([ya, yl]), np.concatenate([xa, xl])
    want, pinned = ml.apply_pins("atan2", ml.ref_atan2(y2, x2), y2, x2)
    checks = [_libm1("sin", A.F32X4_0, 0, trig), _libm1("cos", A.F32X4_0, 1, trig), _libm1("tan", A.F32X4_0, 2, trig), _libm1("atan", A.F32X4_0, 3, trig),
              _libm1("asin", A.F32X4_1, 0, unit), _libm1("acos", A.F32X4_1, 1, unit), _libm1("exp", A.F32X4_1, 2, expo), _libm1("exp2", A.F32X4_1, 3, expo),
              _libm1("log", A.F32X4_2, 0, posi), _libm1("log2", A.F32X4_2, 1, posi),
              ("sqrt", A.F32X4_2, 2, "bits", ml.ref_ieee("sqrt", posi), (posi,)), ("inverseSqrt", A.F32X4_2, 3, "bits", ml.ref_ieee("inverseSqrt", posi), (posi,)),
              ("atan2", A.F32X2_1, 0, "libm", (want, pinned, None), (y2, x2))]
    out["transcendental"] = Case("transcendental", helpers.math_probe_asset,
                                 {A.F32_0: trig, A.F32_1: unit, A.F32_2: expo, A.F32_3: posi, A.F32X2_0: np.stack([y2, x2], axis=1)}, checks)
    # -- IEEE arithmetic and the selects -------------------------------------------------------------------------------------------------------------
    a, b = ml.landmark_pairs()
    x = ml.rounding_args()
    checks = [(op, A.F32X4_0, i, "bits", ml.ref_ieee(op, a, b), (a, b)) for i, op in enumerate(("add", "sub", "mul", "div"))]
    checks += [(op, A.F32X4_1, i, "bits", ml.ref_ieee(op, a, b), (a, b)) for i, op in enumerate(("rem", "min", "max", "step"))]
    checks += [(op, A.F32X4_2, i, "bits", ml.ref_ieee(op, x), (x,)) for i, op in enumerate(("floor", "ceil", "round", "fract"))]
    checks += [(op, A.F32X4_3, i, "bits", ml.ref_ieee(op, x), (x,)) for i, op in enumerate(("sign", "saturate", "abs"))]
    out["ieee"] = Case("ieee", helpers.ieee_probe_asset, {A.F32X2_0: np.stack([a, b], axis=1), A.F32_0: x}, checks)
    a, b, c = ml.landmark_triples()
    checks = [(op, A.F32X3_1, i, "bits", ml.ref_ieee(op, a, b, c), (a, b, c)) for i, op in enumerate(("clamp", "mix", "smoothstep"))]
    out["ternary"] = Case("ternary", helpers.ternary_probe_asset, {A.F32X3_0: np.stack([a, b, c], axis=1)}, checks)
    # -- conversions ---------------------------------------------------------------------------------------------------------------------------------------
    checks = [("f32->i32", A.U32_0, 0, "words", ml.ref_f2i(ml.F2I), (ml.F2I.view(u32),)), ("f32->u32", A.U32_1, 0, "words", ml.ref_f2u(ml.F2I), (ml.F2I.view(u32),)),
              ("u32->f32", A.F32_1, 0, "bits", ml.ref_u2f(ml.I2F), (ml.I2F,)), ("i32->f32", A.F32_2, 0, "bits", ml.ref_i2f(ml.I2F), (ml.I2F,))]
    out["convert"] = Case("convert", helpers.convert_probe_asset, {A.F32_0: ml.F2I, A.U32_2: ml.I2F}, checks)
    # -- integer operators ----------------------------------------------------------------------------------------------------------------------------------
    ia, ib, ic = ml.int_triples()
    for which, (signed, ops) in helpers.INT_PROBES.items():
        checks = [(f"{which}.{op}", attr, 0, "words", ml.ref_int(op, ia, ib, ic, signed=signed), (ia, ib, ic)) for attr, op in zip(helpers.INT_PROBE_OUTPUTS, ops)]
        out[which] = Case(which, functools.partial(helpers.int_probe_asset, which=which), {A.U32_0: ia, A.U32_1: ib, A.U32_2: ic}, checks)
    # -- pack / unpack -----------------------------------------------------------------------------------------------------------------------------------------
    v, words = ml.pack_vectors(), ml.unpack_words()
    checks = [("pack4x8unorm", A.U32_0, 0, "words", ml.ref_pack(v, False), (v.view(u32)[:, 0],)), ("pack4x8snorm", A.U32_1, 0, "words", ml.ref_pack(v, True), (v.view(u32)[:, 0],)),
              ("unpack4x8unorm", A.F32X4_1, None, "bits", ml.ref_unpack(words, False), (words,)), ("unpack4x8snorm", A.F32X4_2, None, "bits", ml.ref_unpack(words, True), (words,))]
    out["pack"] = Case("pack", helpers.pack_probe_asset, {A.F32X4_0: v, A.U32_2: words}, checks)
    # -- vectors -----------------------------------------------------------------------------------------------------------------------------------------------
    va, vb = ml.vec3_pairs()
    checks = [("dot", A.F32X4_0, 0, "bits", ml.ref_vec3("dot", va, vb), (va, vb)), ("length", A.F32X4_0, 1, "bits", ml.ref_vec3("length", va), (va,)),
              ("distance", A.F32X4_0, 2, "bits", ml.ref_vec3("distance", va, vb), (va, vb)), ("normalize", A.F32X3_2, None, "bits", ml.ref_vec3("normalize", va), (va,)),
              ("cross", A.F32X3_3, None, "bits", ml.ref_vec3("cross", va, vb), (va, vb))]
    out["vector"] = Case("vector", helpers.vector_probe_asset, {A.F32X3_0: va, A.F32X3_1: vb}, checks)
    return out


CASE_NAMES = ["transcendental", "ieee", "ternary", "convert", "i32_div", "i32_min", "i32_sign", "u32_div", "u32_max", "pack", "vector"]


def run_probe(runner, case):
    """spawn every particle, write the operand planes, one update frame: {attribute name: uint32 plane} of the case's outputs"""
    runner.step(Frame(1 / 60, case.n, 1))
    write = runner.write_attr if hasattr(runner, "write_attr") else runner.fx.write_attr
    for attr, plane in case.inputs.items():
        write(attr.id, plane)
    runner.step(Frame(1 / 60, 0, 2))
    st = runner.state()
    assert st["counters"]["alive_count"] == case.n
    return {a.name: np.array(st["attrs"][a.name], u32) for a in case.outputs}


def assert_same_planes(ref, got, case, what):
    """bit-equal as uint32; where both sides are NaN the payload is not compared (helpers.assert_same_state)"""
    for attr in case.outputs:
        r, g = ref[attr.name], got[attr.name]
        differs = r != g
        if helpers._is_float_attr(attr.name):
            differs &= ~helpers._both_nan(r, g)
        if differs.any():
            row, col = (int(v) for v in np.argwhere(differs)[0])
            operands = {a.name: np.asarray(p)[row] for a, p in case.inputs.items()}
            raise AssertionError(f"{what}: {attr.name}[{row}, {col}] differs at {int(differs.sum())} places; first: oracle {r[row, col]:#x} ({r[row].view(f32)}) "
                                 f"got {g[row, col]:#x} ({g[row].view(f32)}) at operands {operands}")


@functools.lru_cache(None)
def oracle_planes(name):
    """the oracle's outputs of a case: computed once, shared by the tests of this module"""
    case = cases()[name]
    out = run_probe(OracleRunner(case.asset()), case)
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_against_the_reference(name):
    case = cases()[name]
    out = oracle_planes(name)
    report = []
    for label, attr, col, kind, want, operands in case.checks:
        plane = out[attr.name]
        got = (plane if col is None else plane[:, col])[:len(operands[0])]
        if kind == "words":
            ml.check_words(label, got, want, *operands)
        elif kind == "bits":
            ml.check_bits(label, got.view(f32), want, *operands)
        else:
            ref, pinned, moderate = want
            worst = ml.check_against_libm(label, got.view(f32), ref, pinned, operands, moderate=moderate)
            report.append(f"{label} {worst} ulp over {len(ref)} points ({int(pinned.sum())} pinned)")
    if report:
        print("oracle vs binary64 libm on the lattice: " + "; ".join(report))


@pytest.mark.parametrize("force_generic", [False, True], ids=["as-lowered", "force-generic"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_build_of_the_product_against_the_oracle(name, force_generic):
    """hnb_vm.h + hnb_math.h (the product's copy) compiled for the host give the oracle's bits over the same lattices."""
    case = cases()[name]
    got = run_probe(CpuVmRunner(case.asset(), force_generic=force_generic), case)
    assert_same_planes(oracle_planes(name), got, case, f"{name} cpu_vm force_generic={force_generic}")


def test_pow_on_the_lattice():
    """pow(x, y) has no authoring entry point with a free exponent (HNB_OP_FPOW is reachable through a program blob only; the shape modifiers
    evaluate pow(frand, 1/3), which the GPU parity tests and goldens cover): checked here through oracle.math2 on the CPU only."""
    x, y = ml.pow_args()
    got = np.array([oracle.math2(0, float(a), float(b)) for a, b in zip(x, y)], f32)
    want, pinned = ml.apply_pins("pow", ml.ref_pow(x, y), x, y)
    worst = ml.check_against_libm("pow", got, want, pinned, (x, y), moderate=ml.pow_is_moderate(x, y) & ~pinned)
    print(f"oracle vs binary64 libm on the lattice: pow {worst} ulp over {len(x)} points ({int(pinned.sum())} pinned)")


def test_the_pinned_table_is_exercised():
    """every row of math_lattice.PINNED claims at least one operand of its function's lattice"""
    c = cases()["transcendental"]
    operands = {"pow": ml.pow_args()}
    for label, _, _, kind, _, ops in c.checks:
        if kind == "libm":
            operands[label] = ops
    for fn, what, mask, _ in ml.PINNED:
        with np.errstate(all="ignore"):
            assert mask(*operands[fn]).any(), (fn, what)


def test_uniform_stream_on_the_host():
    """The same operators with every operand an effect property: lowering hoists them into the uniform stream, which the host evaluates once per
    frame (uniform_run in the product, hor_effect_set_property / step in the oracle). One frame per operand pair, the particle spawned in that
    frame keeps the results: product (host build) against the oracle by bits, the oracle's IEEE columns against the numpy reference."""
    a, b = ml.cross(ml.UNIFORM_SET, ml.UNIFORM_SET)
    n = len(a)
    ops = helpers.program_mnemonics(helpers.bh.lower(helpers.uniform_probe_asset(n)))
    assert set(ops["init"]) <= {"M_PIN_SET", "STA", "M_ADD_XLATE"} and not ops["update"] and {"FDIV", "FSIN", "FATAN2", "FSMOOTH"} <= set(ops["uniform"]), ops
    o, v = OracleRunner(helpers.uniform_probe_asset(n)), CpuVmRunner(helpers.uniform_probe_asset(n))
    for f in range(n):
        fr = Frame(1 / 60, 1, f + 1, time=f / 60, props={"a": float(a[f]), "b": float(b[f])})
        o.step(fr)
        v.step(fr)
    ref = o.state()
    helpers.assert_same_state(ref, v.state(), f"uniform stream over {n} operand pairs")
    slot = ref["alive"]                                   # frame f's particle
    assert len(slot) == n
    for attr, names in ((A.F32X4_0, ("add", "sub", "mul", "div")), (A.F32X4_1, ("rem", "min", "max", "step"))):
        plane = ref["attrs"][attr.name].view(f32)[slot]
        for col, op in enumerate(names):
            ml.check_bits(f"uniform {op}", plane[:, col], ml.ref_ieee(op, a, b), a, b)


def test_the_bounds_are_the_documented_ones():
    """math_lattice.MAX_ULP (numpy only, no test imports) restates tests/test_math.py MAX_ULP for the functions both name; atan2 2 and pow 8 / 2 are the
    figures of the header and of test_pow_and_atan2_within_their_ulp_bounds."""
    from test_math import MAX_ULP
    for fn in ml.UNARY64:
        assert ml.MAX_ULP.get(fn, 1) == MAX_ULP.get(fn, 1), fn
    assert ml.MAX_ULP["atan2"] == 2 and ml.MAX_ULP["pow"] == 8 and ml.POW_MODERATE_ULP == 2
