"""Every expression operator at its edge operands (tests/math_lattice.py) ON THE GPU, bit for bit against the oracle, on every path that
evaluates an expression:

  * the byte-code interpreter (HNB_JIT=0) and the per-program specialised kernel (HNB_JIT=1, a hiprtc compile of hnb_math.h): the probes of
    tests/test_math_lattice.py over their whole lattices, one spawn frame and one update frame each;
  * the shared launches that small programs of one context take (k_update_jobs): all the probes in ONE context, each over a few hundred
    points cut from the front (the landmarks) and the body of its lattice;
  * the uniform stream, which the HOST evaluates (hnb_math.h compiled into the runtime library): the operators with every operand an effect
    property, one frame per operand pair of a landmark cross product, the results stored by the init of the one particle that frame spawns.

The output planes must equal the oracle's as uint32; where both sides are NaN the payload is not compared (helpers.assert_same_state).
Every case asserts from Program.kernel_info() - for the uniform stream from the lowered program - that the path it names is the one that
ran. That the oracle itself is right at these operands is tests/test_math_lattice.py's half (no GPU)."""
import numpy as np
import pytest

import bevy_hanabi_amd as bh
import math_lattice as ml
from helpers import Frame, GpuRunner, OracleRunner, assert_same_state, program_mnemonics, uniform_probe_asset
from test_math_lattice import CASE_NAMES, assert_same_planes, cases, oracle_planes, run_probe

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("jit", ["0", "1"], ids=["interp", "jit"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_lattice_on_the_gpu(name, jit, monkeypatch):
    monkeypatch.setenv("HNB_JIT", jit)
    case = cases()[name]
    ctx = bh.Context(0)
    try:
        g = GpuRunner(case.asset(), ctx=ctx)
        got = run_probe(g, case)
        kernels = g.prog.kernel_info().split("\n")[0]
        print(f"{name} ({case.n} particles): {kernels}")
        assert ("update=jit-" in kernels) if jit == "1" else ("update=interp-" in kernels and "jit" not in kernels), g.prog.kernel_info()
        assert "merged launch" not in g.prog.kernel_info()
        assert_same_planes(oracle_planes(name), got, case, f"{name} HNB_JIT={jit} [{kernels}]")
    finally:
        ctx.close()


def _cut(case, points=384):
    """the front of every operand plane (each lattice starts with its landmarks) and an even walk through the rest"""
    front = np.arange(min(case.n, points // 2))
    rest = np.linspace(len(front), case.n - 1, points - len(front)).astype(np.int64) if case.n > len(front) else np.zeros(0, np.int64)
    return case.cut(np.unique(np.concatenate([front, rest])))


def test_lattice_through_the_shared_launches_of_small_programs():
    """Small independent programs of one context share the frame's job-table launches (hnb_plan.h plan_merged_launches): interpreter
    instantiations of their own, behind another kernel entry than the per-program launches."""
    small = [_cut(cases()[name]) for name in CASE_NAMES]
    ctx = bh.Context(0)
    ctx.set_option("scene_merge", 1)
    try:
        gpus = [GpuRunner(c.asset(), ctx=ctx) for c in small]
        orcs = [OracleRunner(c.asset()) for c in small]
        for f, spawn in enumerate((True, False)):
            ctx.frame_begin(1 / 60, f / 60)
            for c, g, o in zip(small, gpus, orcs):
                g.fx.set_frame(c.n if spawn else 0, f + 1, None)
                o.step(Frame(1 / 60, c.n if spawn else 0, f + 1, time=f / 60))
            ctx.simulate()
            if spawn:
                for c, g, o in zip(small, gpus, orcs):
                    for attr, plane in c.inputs.items():
                        g.fx.write_attr(attr.id, plane)
                        o.fx.write_attr(attr.id, plane)
        for c, g, o in zip(small, gpus, orcs):
            info = g.prog.kernel_info()
            line = [l for l in info.split("\n") if l.startswith("update served by a merged launch")]
            assert line and line[0].endswith(": 2 frames"), (c.name, info)
            ref, got = o.state(), g.state()
            assert_same_planes({a.name: ref["attrs"][a.name] for a in c.outputs}, {a.name: got["attrs"][a.name] for a in c.outputs}, c, f"{c.name} in the shared launch")
        print("shared launches: " + ", ".join(f"{c.name} ({c.n})" for c in small) + ": update served by a merged launch in both frames")
    finally:
        ctx.close()


def test_operators_in_the_uniform_stream():
    a, b = ml.cross(ml.UNIFORM_SET, ml.UNIFORM_SET)
    n = len(a)
    asset = uniform_probe_asset(n)
    ops = program_mnemonics(bh.lower(asset))
    assert set(ops["init"]) <= {"M_PIN_SET", "STA", "M_ADD_XLATE"} and not ops["update"], ops          # the device only stores what the host evaluated
    assert {"FADD", "FDIV", "FREM", "FSIN", "FTAN", "FATAN2", "FASIN", "FEXP", "FEXP2", "FLOG2", "FSQRT", "FRSQ", "FROUND", "FSMOOTH"} <= set(ops["uniform"]), ops
    ctx = bh.Context(0)
    try:
        g, o = GpuRunner(asset, ctx=ctx), OracleRunner(uniform_probe_asset(n))
        for f in range(n):
            fr = Frame(1 / 60, 1, f + 1, time=f / 60, props={"a": float(a[f]), "b": float(b[f])})
            g.step(fr)
            o.step(fr)
        assert_same_state(o.state(), g.state(), f"uniform stream over {n} operand pairs")
        print(f"uniform stream: {n} frames of a one-spawn effect, every operator evaluated by the host: equal to the oracle")
    finally:
        ctx.close()
