"""The neighbour sums across two effects (hnb_effect_neighbours_from, include/hanabi_amd_neighbours_from.h) without a GPU: header, ctypes and
INTEGRATION.md agree on the prototype, and the call fails loudly; the plain C++ of csrc/hnb_neighbours_from.h - the per-query body the kernel calls,
the check of a description against two layouts, the scratch layout and the launch plan - compiled as a stand-alone host program under the address and
undefined-behaviour sanitizers gives what the restatements in numpy / Python give, bit for bit; the kernel lives in a code object of its own with no
scratch and no spills. The restatement here (np_neighbours_from) is what tests/test_gpu_neighbours_from.py expects."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import build as hb
from bevy_hanabi_amd import runtime
from test_export_binned_abi import np_cells
from test_export_filtered_abi import CSRC, INSTANCE, _rows, sort_layout
from test_export_sorted_abi import A, LLVM, ROOT
from test_neighbours_abi import ADD, DIFF, ONE, SET, W_ONE, W_U1, W_U2, W_U3, np_contribution, np_d2, np_store, np_weight, one_source

FROM_KERNELS = ["k_neighbours_from_gather"]
F32, U32 = np.float32, np.uint32


# ---- the semantics, restated in numpy ---------------------------------------------------------------------------------------------------------------
def np_neighbours_from(pos_q, alive_q, pos_s, alive_s, src, own, grid, radius, weight, channels, limit):
    """pos_q: [q slots, 3], pos_s: [s slots, 3] binary32; alive_q, alive_s: the alive slots of fx and of the source; src: per channel the
    [s slots] stored words of its source in the SOURCE (one_source for HNB_SPLAT_ATTR_ONE); own: per channel the [q slots] stored words of the same
    attribute in FX (read for DIFF channels only; None otherwise); grid: (dims, origin, inv_cell); channels: per channel (src_attr, src_comp, flags,
    frac_bits, dst_attr, dst_comp, op). Brute force over ALL (query, source) pairs, the cell restriction and the radius tested per pair; no pair is
    left out for its slot numbers. -> dict over fx's slots: inside, crowded, gathered [q slots] bool; cand, nnb [q slots] int64; S [q slots, k]
    int64 (modulo 2^64); cells [q slots]; rejected: int; offsets: the set of cell offsets (source - query) over all neighbour pairs; s_inside,
    s_alive: the inside and the alive sources"""
    pos_q, pos_s = np.asarray(pos_q, F32).reshape(-1, 3), np.asarray(pos_s, F32).reshape(-1, 3)
    aq, as_ = np.asarray(alive_q, np.int64), np.asarray(alive_s, np.int64)
    dims, origin, inv_cell = grid
    dims = [int(d) for d in dims]
    n_cells, nq, K = dims[0] * dims[1] * dims[2], len(pos_q), len(channels)
    cells_q = np.full(nq, n_cells, np.int64)
    if len(aq):
        cells_q[aq] = np_cells(pos_q[aq], dims, origin, inv_cell).astype(np.int64)
    cells_s = np_cells(pos_s[as_], dims, origin, inv_cell).astype(np.int64) if len(as_) else np.zeros(0, np.int64)
    js = as_[cells_s != n_cells]                                          # the inside sources: outside ones contribute to nobody
    cj = cells_s[cells_s != n_cells]
    out = dict(inside=np.zeros(nq, bool), crowded=np.zeros(nq, bool), gathered=np.zeros(nq, bool), cand=np.zeros(nq, np.int64), nnb=np.zeros(nq, np.int64),
               S=np.zeros((nq, K), np.int64), cells=cells_q, rejected=0, offsets=set(), s_inside=len(js), s_alive=len(as_))
    qs = aq[cells_q[aq] != n_cells]
    out["inside"][qs] = True
    if not len(qs):
        return out
    xyz = lambda c: (c % dims[0], (c // dims[0]) % dims[1], c // (dims[0] * dims[1]))
    qx, qy, qz = xyz(cells_q[qs])
    jx, jy, jz = xyz(cj)
    r2 = F32(radius) * F32(radius)
    inv_r2 = F32(1.0) / r2
    S = np.zeros((len(qs), K), np.uint64)
    cand, nnb = np.zeros(len(qs), np.int64), np.zeros(len(qs), np.int64)
    for b in range(0, len(qs), 512):
        q = np.arange(b, min(b + 512, len(qs)))
        near = (np.abs(qx[q, None] - jx[None, :]) <= 1) & (np.abs(qy[q, None] - jy[None, :]) <= 1) & (np.abs(qz[q, None] - jz[None, :]) <= 1)
        cand[q] = near.sum(axis=1)                                         # the inside sources of the at most 27 cells: the query is not among them
        near &= (cand[q] <= int(limit))[:, None]                           # a crowded query is not gathered
        qi, ji = np.nonzero(near)
        qi = q[qi]
        d2 = np_d2(pos_q[qs[qi]], pos_s[js[ji]])
        nb = d2 < r2
        qi, ji, d2 = qi[nb], ji[nb], d2[nb]
        W = np_weight(weight, d2, inv_r2)
        np.add.at(nnb, qi, 1)
        out["offsets"] |= set(zip((jx[ji] - qx[qi]).tolist(), (jy[ji] - qy[qi]).tolist(), (jz[ji] - qz[qi]).tolist()))
        for k, ch in enumerate(channels):
            diff = bool(ch[2] & DIFF)
            vj = np.asarray(src[k], U32)[js[ji]]
            vi = np.asarray(own[k], U32)[qs[qi]] if diff else np.zeros(len(qi), U32)
            ok, qq = np_contribution(vj, vi, diff, weight, W, ch[3])
            np.add.at(S[:, k], qi[ok], qq[ok].view(np.uint64))             # unsigned adds wrap: the two's-complement sum modulo 2^64
            out["rejected"] += int((~ok).sum())
    crowded = cand > int(limit)
    out["cand"][qs] = cand
    out["crowded"][qs] = crowded
    out["gathered"][qs] = ~crowded
    out["S"][qs] = S.view(np.int64)
    out["nnb"][qs] = nnb
    return out


def from_stats(ref, n_alive_q):
    """out_stats of a call whose restatement is ref"""
    return np.array([n_alive_q, ref["gathered"].sum(), n_alive_q - ref["inside"].sum(), ref["crowded"].sum(), ref["rejected"], ref["s_inside"], ref["s_alive"], 0], np.uint64).astype(U32)


def from_plan(cap_q, cap_s, n_cells):
    """neighbours_from_launch_plan restated -> (source sort [(kernel, grid x)], its memset index or None, query sort, its memset index, pack, gather)"""
    def sort(cap, table):
        T = -(-cap // 4096)
        L, memset = [], None
        if T <= 1:
            L.append(("bin_tile", 1))
        else:
            memset = 0
            L.append(("bin_keys", T))
            for p in range(4):
                if p:
                    L.append(("sort_hist", T))
                L.append(("sort_scatter", T))
        if table:
            L.append(("bin_starts", -(-(n_cells + 2) // 256)))
        return L, memset
    return sort(cap_s, True) + sort(cap_q, False) + (max(1, -(-cap_s // 256)), max(1, -(-cap_q // 256)))


def from_layout(cap_q, cap_s, n_channels, n_cells):
    """neighbours_from_scratch_layout restated -> (q_sort_off, snap_off, snap_bytes, src_off, src_bytes, cells_off, cells_bytes, total)"""
    up = lambda x: (x + 255) & ~255
    ss, sq = sort_layout(1, cap_s, INSTANCE), sort_layout(1, cap_q, INSTANCE)
    q_sort_off = up(ss[10])
    snap_off = up(q_sort_off + sq[10])
    src_off = up(snap_off + ss[2] * 16)
    cells_off = up(src_off + ss[2] * 4 * n_channels)
    return (q_sort_off, snap_off, ss[2] * 16, src_off, ss[2] * 4 * n_channels, cells_off, (n_cells + 2) * 4, up(cells_off + (n_cells + 2) * 4))


COUNT = [(ONE, 0, 0, 0, A.LIFETIME.id, 0, SET)]


def test_the_restatement_itself_on_cases_worked_by_hand():
    grid = ((4, 1, 1), (0, 0, 0), (1, 1, 1))
    count = lambda pq, aq, ps, as_, radius=1.0, limit=100, g=grid: np_neighbours_from(pq, aq, ps, as_, [one_source(len(ps))], [None], g, radius, W_ONE, COUNT, limit)
    # a coincident source counts, and equal slot numbers are not excluded: query slot 0 and source slot 0 on one point
    pq = np.array([(0.5, 0.5, 0.5), (2.25, 0.5, 0.5)], F32)
    ps = np.array([(0.5, 0.5, 0.5), (1.4, 0.5, 0.5)], F32)
    r = count(pq, [0, 1], ps, [0, 1])
    assert r["S"][:, 0].tolist() == [2, 1] and r["nnb"].tolist() == [2, 1] and r["cand"].tolist() == [2, 1] and (r["s_inside"], r["s_alive"]) == (2, 2)
    assert r["offsets"] == {(0, 0, 0), (1, 0, 0), (-1, 0, 0)} and from_stats(r, 2).tolist() == [2, 2, 0, 0, 0, 2, 2, 0]
    # a source exactly at d2 == r2 is out; one ulp nearer it is in
    pq = np.array([(0.25, 0.5, 0.5)], F32)
    ps = np.array([(1.25, 0.5, 0.5), (np.nextafter(F32(1.25), F32(0)), 0.5, 0.5)], F32)
    assert count(pq, [0], ps, [0])["nnb"].tolist() == [0] and count(pq, [0], ps, [1])["nnb"].tolist() == [1] and count(pq, [0], ps, [0])["cand"].tolist() == [1]
    # a pair two cells apart is out even when d2 < r2 by rounding: cells of 1/11, the radius the largest binary32 the coverage rule takes there. The
    # query's t rounds into cell 127 and the source's into cell 129, yet the rounded d2 is below the rounded r2
    eleven = ((130, 1, 1), (0, 0, 0), (11, 1, 1))
    radius = F32(0.09090908616781235)
    assert float(radius) * 11.0 <= 1.0 < float(np.nextafter(radius, F32(1))) * 11.0
    pq, ps = np.array([(11.63636302947998, 0.5, 0.5)], F32), np.array([(11.727272033691406, 0.5, 0.5), (11.7, 0.5, 0.5)], F32)
    assert np_cells(pq, *eleven).tolist() == [127] and np_cells(ps, *eleven).tolist() == [129, 128] and np_d2(pq, ps[:1])[0] < radius * radius
    r = count(pq, [0], ps, [0], radius=radius, g=eleven)
    assert r["nnb"].tolist() == [0] and r["cand"].tolist() == [0] and r["gathered"].tolist() == [True]
    r = count(pq, [0], ps, [0, 1], radius=radius, g=eleven)                # ... while the source one cell away counts
    assert r["nnb"].tolist() == [1] and r["cand"].tolist() == [1] and r["offsets"] == {(1, 0, 0)}
    # an outside source contributes to nobody and is no candidate; a NaN source neither; a dead source neither
    pq = np.array([(3.5, 0.5, 0.5)], F32)
    ps = np.array([(4.25, 0.5, 0.5), (np.nan, 0.5, 0.5), (3.75, 0.5, 0.5), (3.25, 0.5, 0.5)], F32)
    r = count(pq, [0], ps, [0, 1, 2])
    assert r["nnb"].tolist() == [1] and r["cand"].tolist() == [1] and (r["s_inside"], r["s_alive"]) == (1, 3)
    # an outside query is counted and nothing else; a dead query is not even visited
    pq = np.array([(-0.25, 0.5, 0.5), (0.25, 0.5, 0.5), (0.3, 0.5, 0.5)], F32)
    ps = np.array([(0.1, 0.5, 0.5)], F32)
    r = count(pq, [1, 0], ps, [0])
    assert r["inside"].tolist() == [False, True, False] and r["gathered"].tolist() == [False, True, False] and r["S"][:, 0].tolist() == [0, 1, 0]
    assert from_stats(r, 2).tolist() == [2, 1, 1, 0, 0, 1, 1, 0]
    # crowding is decided by the sources alone: three queries in a cell with two sources and a limit of 2 are gathered; a third source crowds them
    pq = np.array([(0.2, 0.5, 0.5), (0.4, 0.5, 0.5), (0.6, 0.5, 0.5), (3.5, 0.5, 0.5)], F32)
    ps = np.array([(0.3, 0.5, 0.5), (1.5, 0.5, 0.5), (0.7, 0.5, 0.5)], F32)
    r = count(pq, [0, 1, 2, 3], ps, [0, 1], limit=2)
    assert r["cand"].tolist() == [2, 2, 2, 0] and not r["crowded"].any() and r["S"][:, 0].tolist() == [1, 1, 2, 0]
    r = count(pq, [0, 1, 2, 3], ps, [0, 1, 2], limit=2)
    assert r["cand"].tolist() == [3, 3, 3, 0] and r["crowded"].tolist() == [True, True, True, False] and r["gathered"].tolist() == [False, False, False, True]
    assert r["S"].sum() == 0 and from_stats(r, 4).tolist() == [4, 1, 0, 3, 0, 3, 3, 0]
    # DIFF: v_j from the source, v_i the query's own
    ch = [(A.POSITION.id, 0, DIFF, 10, A.VELOCITY.id, 0, ADD)]
    pq, ps = np.array([(0.5, 0.5, 0.5)], F32), np.array([(0.75, 0.5, 0.5), (0.25, 0.5, 0.5), (1.0, 0.5, 0.5)], F32)
    r = np_neighbours_from(pq, [0], ps, [0, 1, 2], [ps[:, 0].copy().view(U32)], [pq[:, 0].copy().view(U32)], grid, 1.0, W_ONE, ch, 100)
    assert r["S"][:, 0].tolist() == [256 - 256 + 512] and r["rejected"] == 0
    # the restatement speaks the library's own words
    text = open(os.path.join(CSRC, "hnb_neighbours_from.h")).read()
    assert all(f'"{k}"' in text for k in FROM_KERNELS) and "constexpr uint32_t kNeighboursFromBlock = 256;" in text
    assert from_plan(4096, 4097, 62) == ([("bin_keys", 2)] + [(n, 2) for n in ("sort_scatter", "sort_hist", "sort_scatter", "sort_hist", "sort_scatter", "sort_hist", "sort_scatter")]
                                         + [("bin_starts", 1)], 0, [("bin_tile", 1)], None, 17, 16)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------------
def test_ctypes_header_and_integration_agree_on_the_prototype(tmp_path):
    src = r'''
    #include <stdio.h>
    #include "hanabi_amd_neighbours_from.h"
    int main(void) {
        int (*fe)(HnbEffect*, HnbEffect*, const HnbNeighbourDesc*) = hnb_effect_neighbours_from;
        int (*fn)(HnbEffect*, const HnbNeighbourDesc*) = hnb_effect_neighbours;
        printf("%zu\n", sizeof(HnbNeighbourDesc));
        return fe == 0 || fn == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    assert subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split() == ["200"]      # the descriptor is HnbNeighbourDesc unchanged
    assert C.sizeof(runtime.NeighbourDesc) == 200
    lib = runtime.load_library()
    assert runtime.ABI_NEIGHBOURS_FROM_SYMBOLS == ["hnb_effect_neighbours_from"]
    full = open(os.path.join(ROOT, "include", "hanabi_amd_neighbours_from.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(lib, "hnb_effect_neighbours_from") and lib.hnb_effect_neighbours_from.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(runtime.NeighbourDesc)]
    m = re.search(r"int\s+hnb_effect_neighbours_from\s*\(([^)]*)\)\s*;", header)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["HnbEffect* fx", "HnbEffect* source", "const HnbNeighbourDesc* desc"]
    m = re.search(r"\bfn hnb_effect_neighbours_from\(([^)]*)\) -> c_int;", txt)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["fx: *mut HnbEffect", "source: *mut HnbEffect", "desc: *const HnbNeighbourDesc"]
    assert "pub unsafe fn effect_neighbours_from(" in txt and "pub mod neighbours_from {" in txt
    assert list(inspect.signature(runtime.Effect.neighbours_from).parameters) == ["self", "source", "dims", "origin", "inv_cell", "radius", "channels", "weight", "candidate_limit", "scale",
                                                                                  "stats_ptr"]
    assert not hasattr(runtime.Program, "neighbours_from")                 # (no program form: out of scope, the header says so)
    # every header declares exactly its own symbols: hanabi_amd.h and its 61 are as they were, and the companion lists do not overlap
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", header)) == set(runtime.ABI_NEIGHBOURS_FROM_SYMBOLS)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", main)) == set(runtime.ABI_SYMBOLS) and len(runtime.ABI_SYMBOLS) == 61
    for name, syms in (("hanabi_amd_neighbours.h", runtime.ABI_NEIGHBOUR_SYMBOLS), ("hanabi_amd_pairs.h", runtime.ABI_PAIRS_SYMBOLS)):
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", other)) == set(syms)
    for other in (runtime.ABI_SYMBOLS, runtime.ABI_BINNED_SYMBOLS, runtime.ABI_IMPORT_SYMBOLS, runtime.ABI_DEPOSIT_SYMBOLS, runtime.ABI_SAMPLE_SYMBOLS, runtime.ABI_SPLAT_SYMBOLS,
                  runtime.ABI_SAMPLE_PROGRAM_SYMBOLS, runtime.ABI_NEIGHBOUR_SYMBOLS, runtime.ABI_PAIRS_SYMBOLS):
        assert not set(runtime.ABI_NEIGHBOURS_FROM_SYMBOLS) & set(other)
    for inc in ('#include "hanabi_amd.h"', '#include "hanabi_amd_neighbours.h"'):
        assert inc in full
    assert "struct" not in header                                          # there is no new struct
    bound = set(re.findall(r"pub fn (hnb_[a-z0-9_]+)\(", txt))
    assert not set(runtime.ABI_NEIGHBOURS_FROM_SYMBOLS) & bound            # (the `pub fn` set mirrors hanabi_amd.h and the host header: the call sits in a module of its own)
    for word in ("no self-exclusion", "a coincident source is a neighbour", "same context", "source is untouched", "source is only ever", "OUTSIDE BIN", "CROWDED",
                 "the query is not among them", "d2 = s + zz", "lifts that item for the sums", "fx == source", "a DIFF attribute missing from fx's layout", "0xFFFFFF00 slots",
                 "[5] = inside sources", "Out of scope: a program form", "a pair list across effects", "more than one source effect per call", "different grids for the two sides",
                 "a transform", "effects of different contexts", "HnbNeighbourDesc unchanged"):
        assert word in " ".join(full.replace(" * ", " ").split()), word


def test_call_fails_loudly_on_null_arguments_and_without_a_device():
    """Up to the device check: the NULL refusals come before anything is dereferenced, loaded or enqueued. The other refusals need two effects, and
    an effect a device: the stand-alone program below holds them, and tests/test_gpu_neighbours_from.py on live effects."""
    lib = runtime.load_library()
    d = runtime.neighbour_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 1.0, COUNT)
    fake, fake2 = C.c_void_p(0x1000), C.c_void_p(0x2000)   # never dereferenced: the NULL argument is refused first
    for args in ((None, fake2, C.byref(d)), (fake, None, C.byref(d)), (fake, fake2, None), (None, None, None)):
        assert lib.hnb_effect_neighbours_from(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no effect to gather into, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the code object --------------------------------------------------------------------------------------------------------------------------------
def test_code_object_is_built_carried_and_has_its_kernel_without_scratch_or_spills():
    co = hb.neighbours_from_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_neighbours_from.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(FROM_KERNELS), sorted(rows)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert design.index("## Neighbours") < design.index("## Neighbour pairs") < design.index("## Neighbours across effects (`hnb_effect_neighbours_from`)") < design.index("## Measurement (row d)")
    section = design[design.index("## Neighbours across effects"): design.index("## Measurement (row d)")]
    for name, r in rows.items():
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["kernarg_segment_size"] == 264, (name, r)                # one NeighboursFromArgs by value
        assert r["vgpr_count"] <= 64, (name, r)                           # eight waves per SIMD stay possible
        assert r["group_segment_fixed_size"] <= 32, (name, r)             # the stats' five words: the candidates are not staged in LDS
        row = f"| `{name}` | {r['vgpr_count']} | {r['sgpr_count']} | {r['group_segment_fixed_size']} |"
        assert row in section, f"DESIGN.md \"Neighbours across effects\" resource table: {row}"      # (a recorded value, not a preset bound)
    assert "slot-major" in section and "Measured" in section
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_neighbours_from_code)
    for h in ("hnb_neighbours_from.h", "hnb_neighbours.h", "hnb_deposit.h", "hnb_bin_cell.h", "hnb_export_bin.h"):
        assert f'"{h}"' in inspect.getsource(hb.build_neighbours_from_code)
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_neighbours_from.hip")).read()
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_neighbours_from.h")).read()
    assert hb.NEIGHBOURS_FROM_CODE_OBJECTS == (hb.build_neighbours_from_code,)
    assert hb.PAIRS_CODE_OBJECTS == (hb.build_pairs_code,) and hb.NEIGHBOURS_CODE_OBJECTS == (hb.build_neighbours_code,)
    assert "NEIGHBOURS_FROM_CODE_OBJECTS" in inspect.getsource(hb.build_runtime) and "hanabi_amd_neighbours_from.h" in inspect.getsource(hb.build_runtime)
    assert "hanabi_amd_neighbours_from.h" in inspect.getsource(hb._build_code_object)
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "bevy_hanabi_amd/csrc/hnb_neighbours_from_code.inc" in ignored and "*.hsaco" in ignored
    for other in (hb.neighbours_code_path(), hb.pairs_code_path(), hb.export_bin_code_path(), hb.sample_code_path(), hb.deposit_code_path(), hb.export_sort_code_path(),
                  hb.export_filter_code_path()):
        assert not set(_rows(other)) & set(FROM_KERNELS)
    assert sorted(_rows(hb.neighbours_code_path())) == ["k_neighbours_gather", "k_neighbours_pack"]     # the unit whose snapshot kernel the call borrows is as it was


# ---- csrc/hnb_neighbours_from.h as a stand-alone host program under the sanitizers ------------------------------------------------------------------
ERRORS = ["Ok", "ErrSameEffect", "ErrContexts", "ErrStructSize", "ErrFlags", "ErrDims", "ErrOrigin", "ErrInvCell", "ErrRadius", "ErrCoverage", "ErrRadiusSquared", "ErrWeight",
          "ErrCandidateLimit", "ErrChannelCount", "ErrSrcAttr", "ErrSrcComp", "ErrChannelFlags", "ErrDiffOne", "ErrDiffAttr", "ErrFracBits", "ErrDstAttr", "ErrDstComp", "ErrOp",
          "ErrChannelReserved", "ErrDuplicate", "ErrUnusedChannel", "ErrScale", "ErrStats", "ErrNoPosition", "ErrSourceNoPosition", "ErrCapacity", "ErrSourceCapacity"]
E = {n: i for i, n in enumerate(ERRORS)}
# what the check is given: (attr, ncomp, is_f32) of fx and of the source; from entry 1 on neither has a POSITION. The source has HDR_COLOR and SIZE2,
# which fx lacks; fx has F32X4_0, which the source lacks; AGE and LIFETIME lie at different indices.
LAYOUT_Q = [(A.POSITION.id, 3, 1), (A.VELOCITY.id, 3, 1), (A.LIFETIME.id, 1, 1), (A.AGE.id, 1, 1), (A.COLOR.id, 1, 0), (A.F32X4_0.id, 4, 1)]
LAYOUT_S = [(A.POSITION.id, 3, 1), (A.VELOCITY.id, 3, 1), (A.AGE.id, 1, 1), (A.LIFETIME.id, 1, 1), (A.COLOR.id, 1, 0), (A.HDR_COLOR.id, 4, 1), (A.SIZE2.id, 2, 1)]
CH_MEMBERS = ["src_attr", "src_comp", "flags", "frac_bits", "dst_attr", "dst_comp", "op", "reserved"]

HOST_SRC = r"""
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>
#include "hnb_neighbours_from.h"
using namespace hnb;
""" + "\n".join(f"static_assert(kNbFrom{n} == {i}, \"NeighboursFromDescError\");" for i, n in enumerate(ERRORS)) + r"""
static_assert(kNbFromDescErrorCount == """ + str(len(ERRORS)) + r""", "NeighboursFromDescError");
static_assert(sizeof(HnbNeighbourDesc) == 200 && sizeof(NeighboursFromArgs) == 264 && sizeof(NeighbourArgs) == 248 && kNbFromKGather == 0 && kNeighboursFromKernelCount == 1, "hnb_neighbours_from.h");
static_assert(kNeighboursFromBlock == 256 && kNeighboursFromStatsWords == 8 && sizeof(NeighboursFromSnap) == 16, "hnb_neighbours_from.h");
static const NeighbourLayoutAttr kLayoutQ[] = {""" + ", ".join("{%d, %d, %d}" % l for l in LAYOUT_Q) + r"""};
static const NeighbourLayoutAttr kLayoutS[] = {""" + ", ".join("{%d, %d, %d}" % l for l in LAYOUT_S) + r"""};
static float f_of(unsigned b) { float f; std::memcpy(&f, &b, 4); return f; }
static unsigned b_of(float f) { unsigned b; std::memcpy(&b, &f, 4); return b; }
static const char* launch_name(uint32_t k) {
    return k == kExportBinKernelBase + kBinKTile ? "bin_tile" : k == kExportBinKernelBase + kBinKKeys ? "bin_keys" : k == kExportBinKernelBase + kBinKStarts ? "bin_starts" :
           k == kExpSortHist ? "sort_hist" : k == kExpSortScatter ? "sort_scatter" : "?";
}
static int print_sort(const ExportPlan& s, uint32_t cap) {
    if (s.n > kExportPlanMax) return 5;
    std::printf(" %d %u", s.memset_before == kExportNoMemset ? -1 : (int)s.memset_before, s.n);
    for (uint32_t i = 0; i < s.n; ++i) {
        const ExportLaunch& l = s.launch[i];
        if (l.grid_y != 1u || l.args != (l.kernel >= kExportBinKernelBase ? kExportArgsBin : kExportArgsSortPass)) return 5;
        std::printf(" %s:%u:%u", launch_name(l.kernel), l.grid_x, l.pass);
    }
    if (s.memset_before != kExportNoMemset) {                             // relative to the base of the sort's own section
        const ExportSortScratch l = export_sort_scratch_layout(1u, cap, HNB_SORT_SCOPE_INSTANCE);
        if (s.zero_off != l.state_off || s.zero_bytes != l.zero_bytes) return 5;
    }
    return 0;
}
int main() {
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "names")) {
            for (uint32_t i = 0; i < kNeighboursFromKernelCount; ++i) std::printf("%u:%s ", kNeighboursFromKernelNames[i].kernel, kNeighboursFromKernelNames[i].name);
            std::printf("\n");
        } else if (!std::strcmp(what, "texts")) {
            for (uint32_t e = 0; e < kNbFromDescErrorCount; ++e) std::printf("%s|", neighbours_from_error_text(e));
            std::printf("\n");
        } else if (!std::strcmp(what, "plan")) {
            unsigned cq, cs, n_cells;
            if (std::scanf("%u %u %u", &cq, &cs, &n_cells) != 3) return 1;
            const NeighboursFromPlan pl = neighbours_from_launch_plan(cq, cs, n_cells);
            std::printf("%u %u %llu", pl.pack_grid, pl.gather_grid, (unsigned long long)pl.clear_stats_bytes);
            if (print_sort(pl.source_sort, cs)) return 5;
            if (print_sort(pl.query_sort, cq)) return 5;
            std::printf("\n");
        } else if (!std::strcmp(what, "layout")) {
            unsigned cq, cs, nch, n_cells;
            if (std::scanf("%u %u %u %u", &cq, &cs, &nch, &n_cells) != 4) return 1;
            const NeighboursFromScratch l = neighbours_from_scratch_layout(cq, cs, nch, n_cells);
            std::printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %u %u %u %u\n", (unsigned long long)l.q_sort_off, (unsigned long long)l.snap_off, (unsigned long long)l.snap_bytes,
                        (unsigned long long)l.src_off, (unsigned long long)l.src_bytes, (unsigned long long)l.cells_off, (unsigned long long)l.cells_bytes, (unsigned long long)l.total,
                        (unsigned long long)l.s_sort.total, (unsigned long long)l.q_sort.total, l.s_sort.pitch, l.q_sort.pitch, l.s_sort.rows, l.q_sort.rows);
        } else if (!std::strcmp(what, "run")) {   // a whole state through the header: the source's cells, stable sort, table, snapshot; every query through neighbours_from_row; the store
            BinGrid g = {};
            unsigned ob[3], ib[3], rb, sb, weight, limit, nch, nq, ns;
            if (std::scanf("%u %u %u %x %x %x %x %x %x %x %x %u %u %u %u %u", &g.dims[0], &g.dims[1], &g.dims[2], &ob[0], &ob[1], &ob[2], &ib[0], &ib[1], &ib[2], &rb, &sb, &weight, &limit,
                           &nch, &nq, &ns) != 16) return 1;
            for (int c = 0; c < 3; ++c) { g.origin[c] = f_of(ob[c]); g.inv_cell[c] = f_of(ib[c]); }
            g.n_cells = bin_cell_count(g.dims);
            if (nch > 4u) return 1;
            unsigned one[4], diff[4], frac[4], op[4];
            NeighbourChannelArg ch[4] = {};
            for (unsigned k = 0; k < nch; ++k) {
                if (std::scanf("%u %u %u %u", &one[k], &diff[k], &frac[k], &op[k]) != 4) return 1;
                ch[k].src_packed = neighbour_pack_src(1u, 0u, one[k] != 0, diff[k] != 0, frac[k]);
            }
            std::vector<uint32_t> spos(3 * (size_t)ns), ssrc(nch * (size_t)ns);   // the alive sources in list order
            for (size_t i = 0; i < ns; ++i) {
                if (std::scanf("%x %x %x", &spos[3 * i], &spos[3 * i + 1], &spos[3 * i + 2]) != 3) return 1;
                for (unsigned k = 0; k < nch; ++k)
                    if (std::scanf("%x", &ssrc[k * (size_t)ns + i]) != 1) return 1;
            }
            std::vector<uint32_t> qpos(3 * (size_t)nq), own(nch * (size_t)nq), dstv(nch * (size_t)nq);   // the alive queries
            for (size_t i = 0; i < nq; ++i) {
                if (std::scanf("%x %x %x", &qpos[3 * i], &qpos[3 * i + 1], &qpos[3 * i + 2]) != 3) return 1;
                for (unsigned k = 0; k < nch; ++k)
                    if (std::scanf("%x %x", &own[k * (size_t)nq + i], &dstv[k * (size_t)nq + i]) != 2) return 1;
            }
            const float radius = f_of(rb), r2 = radius * radius, inv_r2 = 1.0f / r2;
            std::vector<uint32_t> cell(ns), order(ns);
            for (size_t i = 0; i < ns; ++i) cell[i] = bin_cell_of(g, f_of(spos[3 * i]), f_of(spos[3 * i + 1]), f_of(spos[3 * i + 2]));
            std::iota(order.begin(), order.end(), 0u);
            std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cell[x] < cell[y]; });
            std::vector<uint32_t> start(export_bin_entries(g.n_cells));     // exactly n_cells + 2 entries on the heap: a read past them is an error the sanitizer reports
            for (uint32_t c = 0; c < start.size(); ++c)
                start[c] = (uint32_t)(std::lower_bound(order.begin(), order.end(), c, [&](uint32_t row, uint32_t key) { return cell[row] < key; }) - order.begin());
            const uint32_t n_inside = start[g.n_cells];
            std::vector<NeighboursFromSnap> snap(n_inside);                 // exactly the inside rows: no walk may read an outside one
            std::vector<uint32_t> srcv(nch * (size_t)n_inside);             // ... and their stored sources, pitch n_inside
            for (uint32_t r = 0; r < n_inside; ++r) {
                snap[r] = {spos[3 * order[r]], spos[3 * order[r] + 1], spos[3 * order[r] + 2], order[r]};
                for (unsigned k = 0; k < nch; ++k) srcv[k * (size_t)n_inside + r] = ssrc[k * (size_t)ns + order[r]];
            }
            unsigned long long rejected = 0;
            std::printf("%u", n_inside);
            std::vector<long long> line;
            for (uint32_t i = 0; i < nq; ++i) {
                line.clear();
                const float xi = f_of(qpos[3 * i]), yi = f_of(qpos[3 * i + 1]), zi = f_of(qpos[3 * i + 2]);
                const uint32_t qc = bin_cell_of(g, xi, yi, zi);
                if (qc >= g.n_cells) line = {0};
                else {
                    const uint32_t cand = neighbour_candidates(start.data(), g.dims, neighbour_cell_xyz(g.dims, qc));
                    uint32_t vi[4] = {0u, 0u, 0u, 0u};
                    for (unsigned k = 0; k < nch; ++k) vi[k] = diff[k] ? own[k * (size_t)nq + i] : 0xDEADBEEFu;     // (not read without the flag)
                    const NeighboursFromRow row = neighbours_from_row(snap.data(), srcv.data(), n_inside, start.data(), g.dims, qc, xi, yi, zi, vi, ch, nch, weight, limit, r2, inv_r2);
                    if (row.crowded != (cand > limit ? 1u : 0u)) return 6;
                    if (row.crowded) {
                        for (unsigned k = 0; k < 4u; ++k) if (row.S[k] != 0) return 6;
                        if (row.rejected) return 6;
                        line = {1, (long long)cand};
                    } else {
                        rejected += row.rejected;
                        line = {2, (long long)cand};
                        for (unsigned k = 0; k < nch; ++k) {
                            line.push_back((long long)row.S[k]);
                            line.push_back((long long)b_of(neighbour_store(op[k], f_of(dstv[k * (size_t)nq + i]), row.S[k], frac[k], f_of(sb))));
                        }
                    }
                }
                std::printf(" |");
                for (long long v : line) std::printf(" %lld", v);
            }
            std::printf(" | %llu\n", rejected);
        } else if (!std::strcmp(what, "desc")) {
            HnbNeighbourDesc d;
            std::memset(&d, 0, sizeof d);
            unsigned long long stats; unsigned same_fx, same_ctx, q_first, s_first, cq, cs, ob[3], ib[3], rb, sb;
            if (std::scanf("%u %u %u %u %u %u %u %u %u %u %u %u %x %x %x %x %x %x %x %x %u %u %llx", &same_fx, &same_ctx, &q_first, &s_first, &cq, &cs, &d.struct_size, &d.flags, &d.dims[0],
                           &d.dims[1], &d.dims[2], &d.n_channels, &ob[0], &ob[1], &ob[2], &ib[0], &ib[1], &ib[2], &rb, &sb, &d.weight, &d.candidate_limit, &stats) != 23) return 1;
            std::memcpy(d.origin, ob, 12); std::memcpy(d.inv_cell, ib, 12); d.radius = f_of(rb); d.scale = f_of(sb);
            d.out_stats = (uint32_t*)(uintptr_t)stats;
            for (unsigned k = 0; k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) {
                HnbNeighbourChannel& ch = d.channels[k];
                if (std::scanf("%u %u %u %u %u %u %u %u", &ch.src_attr, &ch.src_comp, &ch.flags, &ch.frac_bits, &ch.dst_attr, &ch.dst_comp, &ch.op, &ch.reserved) != 8) return 1;
            }
            if (q_first > 1 || s_first > 1) return 1;
            const NeighboursFromSide fx = {kLayoutQ + q_first, (uint32_t)(sizeof kLayoutQ / sizeof *kLayoutQ) - q_first, cq};
            const NeighboursFromSide src = {kLayoutS + s_first, (uint32_t)(sizeof kLayoutS / sizeof *kLayoutS) - s_first, cs};
            const NeighboursFromCheck c = neighbours_from_check_desc(d, fx, src, same_fx != 0, same_ctx != 0);
            if (c.error >= kNbFromDescErrorCount || !neighbours_from_error_text(c.error)[1]) return 3;
            std::printf("%u %u %u %u %u %x %x %d %d", c.error, c.channel, c.n_cells, c.q_position_index, c.s_position_index, b_of(c.r2), b_of(c.inv_r2), c.source_age ? 1 : 0, c.own_age ? 1 : 0);
            for (uint32_t k = 0; k < d.n_channels && k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) std::printf(" %u %u %u", c.src_index[k], c.own_index[k], c.dst_index[k]);
            std::printf("\n");
        } else return 4;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """g++ alone, with the address and undefined-behaviour sanitizers and no contraction: the header is plain C++ on the host. The program has its
    own main and is run directly; nothing is loaded into Python under a sanitizer."""
    tmp = tmp_path_factory.mktemp("neighbours_from_host")
    (tmp / "nbf.cpp").write_text(HOST_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), str(tmp / "nbf.cpp"), "-o", str(tmp / "nbf")])
    return str(tmp / "nbf")


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()      # (a sanitizer report ends the program with an error)
    assert len(out) == len(lines)
    return out


def _f32(x):
    return int(np.array([x], F32).view(U32)[0])


# channel 1: a DIFF of VELOCITY.y (in both layouts) added into fx's F32X4_0.w
GOOD_CH = ((ONE, 0, 0, 30, A.LIFETIME.id, 0, SET, 0), (A.VELOCITY.id, 1, DIFF, 12, A.F32X4_0.id, 3, ADD, 0))


def _desc_line(same_fx=0, same_ctx=1, q_first=0, s_first=0, cap_q=10_000, cap_s=20_000, struct_size=200, flags=0, dims=(4, 4, 4), n_channels=2, origin=(0.0, 0.0, 0.0),
               inv_cell=(1.0, 1.0, 1.0), radius=0.75, scale=1.0, weight=3, limit=4096, stats=0x3000, channels=GOOD_CH):
    ch = list(channels) + [(0,) * 8] * (4 - len(channels))
    return ("desc %d %d %d %d %d %d %d %d %d %d %d %d " % (same_fx, same_ctx, q_first, s_first, cap_q, cap_s, struct_size, flags, *dims, n_channels)
            + " ".join("%x" % _f32(x) for x in tuple(origin) + tuple(inv_cell) + (radius, scale)) + " %d %d %x " % (weight, limit, stats)
            + " ".join("%d %d %d %d %d %d %d %d" % tuple(c) for c in ch))


def test_description_check_refuses_what_the_header_lists_every_error_class_in_its_order(host_exe):
    raw = lambda **kw: _ask(host_exe, [_desc_line(**kw)])[0].split()
    ask = lambda **kw: [int(x) for x in raw(**kw)[:5]]
    hit = []

    def refused(name, channel=None, **kw):
        got = ask(**kw)
        assert got[0] == E[name] and (channel is None or got[1] == channel), (name, kw, got)
        if name not in hit:
            hit.append(name)

    w = raw()
    assert [int(x) for x in w[:5]] == [E["Ok"], 0, 64, 0, 0] and [int(w[5], 16), int(w[6], 16)] == [_f32(F32(0.75) * F32(0.75)), _f32(F32(1) / (F32(0.75) * F32(0.75)))]
    # no AGE; ATTR_ONE has no entry on either side, LIFETIME is fx's entry 2; VELOCITY is entry 1 of both, F32X4_0 fx's entry 5
    assert [int(x) for x in w[7:]] == [0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 2, 1, 1, 5]
    age = lambda flags: raw(channels=((A.AGE.id, 0, flags, 0, A.POSITION.id, 2, ADD, 0),), n_channels=1)
    assert age(0)[7:] == ["1", "0", "2", str(0xFFFFFFFF), "0"] and age(DIFF)[7:] == ["1", "1", "2", "3", "0"]     # AGE: the source's entry 2, fx's entry 3; materialised on fx for DIFF only
    # a source attribute fx lacks is fine without DIFF; a destination the source lacks is fine
    assert ask(channels=((A.HDR_COLOR.id, 3, 0, 8, A.F32X4_0.id, 0, SET, 0), (A.SIZE2.id, 1, 0, 8, A.POSITION.id, 0, ADD, 0)))[0] == E["Ok"]
    assert ask(radius=1.0, weight=0, limit=1, stats=0, scale=-0.0)[0] == E["Ok"] and ask(limit=65536, cap_q=0xFFFFFF00, cap_s=0xFFFFFF00)[0] == E["Ok"]
    refused("ErrSameEffect", same_fx=1)
    refused("ErrSameEffect", same_fx=1, same_ctx=0, struct_size=0)          # in front of everything else
    refused("ErrContexts", same_ctx=0)
    refused("ErrContexts", same_ctx=0, struct_size=0)
    for size in (0, 196, 204):
        refused("ErrStructSize", struct_size=size)
    for flags in (1, 0x80000000):
        refused("ErrFlags", flags=flags)
    for dims in ((0, 4, 4), (4, 4, 0), ((1 << 24) + 1, 1, 1), (4096, 4096, 2)):
        refused("ErrDims", dims=dims)
    for axis in range(3):
        for bad in (np.nan, np.inf):
            o = [0.0] * 3; o[axis] = bad
            refused("ErrOrigin", axis, origin=o)
        for bad in (np.nan, np.inf, 0.0, -1.0):
            i = [1.0] * 3; i[axis] = bad
            refused("ErrInvCell", axis, inv_cell=i)
    for bad in (np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0):
        refused("ErrRadius", radius=bad)
    for axis in range(3):
        i = [1.0] * 3; i[axis] = float(np.nextafter(F32(4 / 3), F32(2)))    # 0.75 * 4/3 rounded up: past 1 in double
        refused("ErrCoverage", axis, inv_cell=i)
    refused("ErrCoverage", 0, radius=float(np.nextafter(F32(1.0), F32(2))))
    tiny = (1e-30,) * 3
    refused("ErrRadiusSquared", radius=1e-20, inv_cell=tiny)               # r2 = 1e-40: a denormal
    refused("ErrRadiusSquared", radius=1e-30, inv_cell=tiny)               # r2 = 0, inv_r2 = inf
    refused("ErrRadiusSquared", radius=1e20, inv_cell=tiny)                # r2 = inf
    assert ask(radius=1.1e-19, inv_cell=tiny)[0] == E["Ok"]
    for weight in (4, 0xFFFFFFFF):
        refused("ErrWeight", weight=weight)
    for limit in (0, 65537, 0xFFFFFFFF):
        refused("ErrCandidateLimit", limit=limit)
    refused("ErrChannelCount", n_channels=5)
    refused("ErrChannelCount", n_channels=0, channels=())
    good = GOOD_CH[0]
    ch = lambda **kw: (good, tuple(kw.get(m, v) for m, v in zip(CH_MEMBERS, GOOD_CH[1])))
    # packed u32; not stored; no attribute; and F32X4_0, which is fx's but not the SOURCE's
    for attr in (A.COLOR.id, A.SIZE3.id, A.ID.id, A.PARTICLE_COUNTER.id, 9999, A.F32X4_0.id):
        refused("ErrSrcAttr", 1, channels=ch(src_attr=attr, src_comp=0, flags=0))
    for attr, comp in ((A.LIFETIME.id, 1), (A.POSITION.id, 3), (ONE, 1), (A.SIZE2.id, 2), (A.HDR_COLOR.id, 0xFFFFFFFF)):
        refused("ErrSrcComp", 1, channels=ch(src_attr=attr, src_comp=comp, flags=0))
    for flags in (2, 3, 0x80000000):
        refused("ErrChannelFlags", 1, channels=ch(flags=flags))
    refused("ErrDiffOne", 1, channels=ch(src_attr=ONE, src_comp=0))
    for attr, comp in ((A.HDR_COLOR.id, 0), (A.SIZE2.id, 1)):               # the source's, but missing from fx's layout: there is no v_i
        assert ask(channels=ch(src_attr=attr, src_comp=comp, flags=0))[0] == E["Ok"]
        refused("ErrDiffAttr", 1, channels=ch(src_attr=attr, src_comp=comp))
    for frac in (33, 0xFFFFFFFF):
        refused("ErrFracBits", 1, channels=ch(frac_bits=frac))
    # AGE; packed u32; not in fx's layout - HDR_COLOR and SIZE2 are the SOURCE's alone
    for attr in (A.AGE.id, A.COLOR.id, A.SIZE3.id, A.ID.id, ONE, 9999, A.HDR_COLOR.id, A.SIZE2.id):
        refused("ErrDstAttr", 1, channels=ch(dst_attr=attr, dst_comp=0))
    for attr, comp in ((A.LIFETIME.id, 1), (A.POSITION.id, 3), (A.F32X4_0.id, 4)):
        refused("ErrDstComp", 1, channels=ch(dst_attr=attr, dst_comp=comp))
    for op in (2, 0xFFFFFFFF):
        refused("ErrOp", 1, channels=ch(op=op))
    refused("ErrChannelReserved", 1, channels=ch(reserved=1))
    refused("ErrDuplicate", 1, channels=ch(dst_attr=A.LIFETIME.id, dst_comp=0))
    for k, m in ((2, "src_attr"), (3, "src_comp"), (2, "flags"), (3, "frac_bits"), (2, "dst_attr"), (3, "dst_comp"), (2, "op"), (3, "reserved")):
        entries = list(GOOD_CH) + [(0,) * 8, (0,) * 8]
        entries[k] = tuple(1 if x == m else 0 for x in CH_MEMBERS)
        refused("ErrUnusedChannel", k, channels=entries)
    refused("ErrUnusedChannel", 1, n_channels=1)
    for bad in (np.nan, np.inf, -np.inf):
        refused("ErrScale", scale=bad)
    for stats in (0x3004, 0x3008):
        refused("ErrStats", stats=stats)
    lone = dict(channels=((ONE, 0, 0, 0, A.LIFETIME.id, 0, SET, 0),), n_channels=1)
    refused("ErrNoPosition", q_first=1, **lone)
    refused("ErrNoPosition", q_first=1, s_first=1, **lone)                  # fx's is named first
    refused("ErrSourceNoPosition", s_first=1, **lone)
    for cap in (0xFFFFFF01, 0xFFFFFFFF):
        refused("ErrCapacity", cap_q=cap)
        refused("ErrCapacity", cap_q=cap, cap_s=cap)
    for cap in (0xFFFFFF01, 0xFFFFFFFF):
        refused("ErrSourceCapacity", cap_s=cap)
    assert hit == ERRORS[1:], (hit, ERRORS[1:])                            # every error class, first met in the header's order
    texts = _ask(host_exe, ["texts"])[0].split("|")[:-1]
    assert len(texts) == len(ERRORS) and len(set(texts)) == len(texts) and texts[0] == "ok"
    for name, word in (("ErrSameEffect", "hnb_effect_neighbours'"), ("ErrContexts", "different contexts"), ("ErrSrcAttr", "source's particle layout"), ("ErrDiffAttr", "fx's particle layout"),
                       ("ErrDstAttr", "fx's particle layout"), ("ErrNoPosition", "fx's particle layout has no POSITION"), ("ErrSourceNoPosition", "the source's particle layout has no POSITION"),
                       ("ErrCapacity", "fx has more than 0xFFFFFF00"), ("ErrSourceCapacity", "the source has more than 0xFFFFFF00"), ("ErrCoverage", "radius * inv_cell is above 1")):
        assert word in texts[E[name]], (name, texts[E[name]])


def test_scratch_layout_and_launch_plan_are_their_restatements_at_each_side_s_capacities(host_exe):
    assert _ask(host_exe, ["names"])[0].split() == [f"{i}:{n}" for i, n in enumerate(FROM_KERNELS)]
    caps = [1, 4096, 4097]
    for cap_q in caps + [16_777_216]:
        for cap_s in caps + [10_000]:
            for n_cells, nch in ((1, 1), (512, 3), (1 << 24, 4)):
                lay, plan = _ask(host_exe, ["layout %d %d %d %d" % (cap_q, cap_s, nch, n_cells), "plan %d %d %d" % (cap_q, cap_s, n_cells)])
                lay = [int(x) for x in lay.split()]
                want = from_layout(cap_q, cap_s, nch, n_cells)
                ss, sq = sort_layout(1, cap_s, INSTANCE), sort_layout(1, cap_q, INSTANCE)
                assert tuple(lay[:8]) == want and lay[8:] == [ss[10], sq[10], ss[2], sq[2], cap_s, cap_q], (cap_q, cap_s, nch, n_cells, lay, want)
                q_sort_off, snap_off, snap_b, src_off, src_b, cells_off, cells_b, total = lay[:8]
                assert all(o % 256 == 0 for o in (q_sort_off, snap_off, src_off, cells_off, total))
                assert ss[10] <= q_sort_off and q_sort_off + sq[10] <= snap_off and snap_off + snap_b <= src_off and src_off + src_b <= cells_off and cells_off + cells_b <= total
                assert snap_b >= 16 * cap_s and src_b >= 4 * nch * cap_s and cells_b == 4 * (n_cells + 2)      # the snapshot and the sources are the SOURCE's rows
                w = plan.split()
                Ls, ms, Lq, mq, pack, gather = from_plan(cap_q, cap_s, n_cells)
                assert [int(x) for x in w[:3]] == [pack, gather, 32], (cap_q, cap_s, w)
                assert (pack - 1) * 256 < cap_s <= pack * 256 and (gather - 1) * 256 < cap_q <= gather * 256       # every source row and every query row has a lane
                rest = w[3:]
                for L, memset in ((Ls, ms), (Lq, mq)):
                    assert [int(rest[0]), int(rest[1])] == [-1 if memset is None else memset, len(L)], (cap_q, cap_s, rest)
                    got = [(x.split(":")[0], int(x.split(":")[1])) for x in rest[2: 2 + len(L)]]
                    assert got == L, (cap_q, cap_s, n_cells, got, L)
                    rest = rest[2 + len(L):]
                assert not rest and Ls[-1][0] == "bin_starts" and all(k != "bin_starts" for k, _ in Lq)      # one table: the sources'
                assert len(Ls) + len(Lq) + 2 <= (5 if max(cap_q, cap_s) <= 4096 else 19)
    row = [int(x) for x in _ask(host_exe, ["layout %d 1 1 64" % (0xFFFFFF00 + 1), "layout 1 %d 1 64" % (0xFFFFFF00 + 1)])[0].split()]
    assert row[13] == 0 and row[12] == 1                                   # one above: no sort fits that side (rows == 0), and the check refuses it (above)


# ---- whole states: the header's row body against the brute-force restatement -------------------------------------------------------------------------
def _run_line(pos_q, alive_q, own, dstv, pos_s, alive_s, src, grid, radius, scale, weight, limit, channels):
    dims, origin, inv_cell = grid
    head = "run %d %d %d " % tuple(dims) + " ".join("%x" % _f32(x) for x in tuple(origin) + tuple(inv_cell) + (radius, scale))
    head += " %d %d %d %d %d " % (weight, limit, len(channels), len(alive_q), len(alive_s))
    head += " ".join("%d %d %d %d" % (int(c[0] == ONE), c[2] & DIFF, c[3], c[6]) for c in channels)
    s_rows = np.concatenate([np.asarray(pos_s, F32).view(U32).reshape(-1, 3)] + [np.asarray(s, U32)[:, None] for s in src], axis=1)[alive_s]
    q_rows = np.concatenate([np.asarray(pos_q, F32).view(U32).reshape(-1, 3)] + [np.stack([o, d], axis=1) for o, d in zip(own, dstv)], axis=1)[alive_q]
    return head + " " + " ".join("%x" % w for w in s_rows.reshape(-1)) + " " + " ".join("%x" % w for w in q_rows.reshape(-1))


# (dims, radius, n_q, n_s, limit)
STATES = [((3, 3, 3), 0.3, 300, 400, 4096), ((5, 4, 3), 0.25, 500, 300, 4096), ((1, 1, 1), 1.0, 40, 60, 4096), ((2, 1, 7), 0.14, 200, 300, 90), ((4, 4, 4), 0.25, 300, 500, 30),
          ((3, 3, 3), 0.3, 50, 0, 4096), ((3, 3, 3), 0.3, 0, 50, 4096)]


@pytest.mark.parametrize("dims,radius,n_q,n_s,limit", STATES, ids=["x".join(map(str, s[0])) + f"-q{s[2]}-s{s[3]}-limit{s[4]}" for s in STATES])
def test_whole_states_through_the_row_body_are_the_brute_force_restatement_bit_for_bit(host_exe, dims, radius, n_q, n_s, limit):
    """two clouds uniform in and a little around the unit cube - part of each outside -, a source cluster in one cell (crowding under the small
    limits), queries coincident with sources at equal slot numbers, a NaN and an infinite position on each side, dead slots on each side; sources
    with denormals, zeros and values that are rejected at frac_bits 32"""
    rng = np.random.default_rng(1000 * n_q + n_s)
    def cloud(n):
        pos = rng.uniform(-0.05, 1.05, (n, 3)).astype(F32)
        if n >= 10:
            pos[-1] = (np.nan, 0.5, 0.5); pos[-2] = (0.5, np.inf, 0.5)
        alive = np.union1d(rng.permutation(n)[: n - n // 10], [n - 1, n - 2]) if n >= 10 else np.arange(n)
        return pos, alive[rng.permutation(len(alive))].astype(np.int64)
    pos_q, alive_q = cloud(n_q)
    pos_s, alive_s = cloud(n_s)
    if n_s >= 10:
        pos_s[: n_s // 6] = (F32(0.4) + rng.uniform(0, 0.05, (n_s // 6, 3))).astype(F32)
    m = min(n_q, n_s) // 8
    pos_q[m: 2 * m] = pos_s[m: 2 * m]                                       # coincident, at equal slot numbers: not excluded
    grid = (dims, (0.0, 0.0, 0.0), tuple(float(d) for d in dims))
    vel_s = rng.normal(0, 3, n_s).astype(F32)
    vel_s[::9] = F32(1e-41); vel_s[4::13] = F32(-0.0); vel_s[5::37] = F32(1e30); vel_s[7::41] = F32(np.nan)
    channels = [(ONE, 0, 0, 0, A.LIFETIME.id, 0, SET), (ONE, 0, 0, 30, A.VELOCITY.id, 0, ADD), (A.POSITION.id, 0, DIFF, 20, A.POSITION.id, 0, ADD), (A.VELOCITY.id, 1, 0, 32, A.VELOCITY.id, 2, SET)]
    src = [one_source(n_s), one_source(n_s), pos_s[:, 0].copy().view(U32), vel_s.view(U32)]
    own = [np.zeros(n_q, U32), np.zeros(n_q, U32), pos_q[:, 0].copy().view(U32), np.zeros(n_q, U32)]
    dstv = [rng.normal(0, 1, n_q).astype(F32).view(U32), rng.normal(0, 1, n_q).astype(F32).view(U32), own[2], rng.normal(0, 1, n_q).astype(F32).view(U32)]
    total = dict(gathered=0, crowded=0, outside=0, rejected=0, nb=0, coincident=0)
    for weight, scale in ((W_ONE, 1.0), (W_U1, -0.5), (W_U2, 2.0), (W_U3, 2.0 ** -100)):
        want = np_neighbours_from(pos_q, alive_q, pos_s, alive_s, src, own, grid, radius, weight, channels, limit)
        out = _ask(host_exe, [_run_line(pos_q, alive_q, own, dstv, pos_s, alive_s, src, grid, radius, scale, weight, limit, channels)])[0].split(" |")
        assert int(out[0]) == want["s_inside"] and int(out[-1]) == want["rejected"] and len(out) == len(alive_q) + 2
        for i, item in zip(alive_q, out[1:-1]):
            w = [int(x) for x in item.split()]
            state = 2 if want["gathered"][i] else 1 if want["crowded"][i] else 0
            assert w[0] == state and (state == 0 or w[1] == want["cand"][i]), (i, w, state, want["cand"][i])
            if state == 2:
                for k, ch in enumerate(channels):
                    stored = np_store(ch[6], dstv[k][i: i + 1].view(F32), want["S"][i: i + 1, k], ch[3], scale).view(U32)[0]
                    assert w[2 + 2 * k] == want["S"][i, k], (i, k, w, want["S"][i])
                    assert w[3 + 2 * k] == stored or (np.isnan(np.array([stored], U32).view(F32)[0]) and np.isnan(np.array([w[3 + 2 * k]], U32).view(F32)[0])), (i, k, w)
        total["gathered"] += int(want["gathered"].sum()); total["crowded"] += int(want["crowded"].sum()); total["outside"] += len(alive_q) - int(want["inside"].sum())
        total["rejected"] += want["rejected"]; total["nb"] += int(want["nnb"].sum())
        both = np.intersect1d(np.intersect1d(np.arange(m, 2 * m), alive_q), alive_s)
        total["coincident"] += int((want["gathered"][both] & (want["nnb"][both] >= 1)).sum())
    if n_q == 0:
        assert total == dict(gathered=0, crowded=0, outside=0, rejected=0, nb=0, coincident=0) and want["s_inside"] > 0
    elif n_s == 0:
        assert total["gathered"] > 0 and total["nb"] == 0 and total["crowded"] == 0 and (want["S"] == 0).all() and want["s_alive"] == 0      # S = 0, and the store's formula is followed
    else:
        assert total["gathered"] > 0 and total["outside"] > 0 and total["rejected"] > 0 and total["nb"] > total["gathered"], total
        assert want["s_inside"] < want["s_alive"], "there are outside sources"
        assert (total["crowded"] > 0) == (limit < 4096), total
        assert limit < 4096 or total["coincident"] > 0, "a query coincident with the source of its own slot number counts it"
    if dims == (3, 3, 3) and n_q and n_s:
        assert len(want["offsets"]) == 27                                  # every one of the 26 directions, and the own cell
