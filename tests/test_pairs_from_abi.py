"""The neighbour list across two effects (hnb_effect_pairs_from, include/hanabi_amd_pairs_from.h) without a GPU: header, ctypes and INTEGRATION.md agree
on the prototype, and the call fails loudly; the plain C++ of csrc/hnb_pairs_from.h - the two per-query bodies both kernels call, the check of a
description against two effects, the scratch layout and the launch plan - compiled as a stand-alone host program under the address and
undefined-behaviour sanitizers gives what the restatements in numpy / Python give, bit for bit; the two kernels live in a code object of their own with
no scratch and no spills. The restatement here (np_pairs_from, pairs_from_buffers) is what tests/test_gpu_pairs_from.py expects."""
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
from test_neighbours_from_abi import from_plan
from test_pairs_abi import MEMBERS, NO_ROW, truncations

PAIRS_FROM_KERNELS = ["k_pairs_from_count", "k_pairs_from_fill"]
F32, U32 = np.float32, np.uint32
SENT = 0xDEADBEEF


# ---- the semantics, restated in numpy ---------------------------------------------------------------------------------------------------------------
def np_d2_from(pq, ps):
    """pq: the queries' and ps: the sources' [n, 3] binary32 positions -> d2, the header's eight statements, the query as i and the source as j"""
    with np.errstate(all="ignore"):
        dx = ps[..., 0] - pq[..., 0]
        dy = ps[..., 1] - pq[..., 1]
        dz = ps[..., 2] - pq[..., 2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        s = xx + yy
        d2 = s + zz
    assert d2.dtype == F32
    return d2


def np_pairs_from(pos_q, alive_q, pos_s, alive_s, grid, radius, candidate_limit):
    """pos_q: [q slots, 3], pos_s: [s slots, 3] binary32; alive_q, alive_s: the alive slots of fx and of the source in list order; grid: (dims,
    origin, inv_cell). Brute force over ALL (inside query, inside source) pairs: the 27-cell rule - the cell indices differ by at most 1 on every
    axis - and d2 < r2 are tested per pair; no pair is left out for its slot numbers. -> dict: rows [n_inside] fx's slots in the stable order by
    cell; cells, cand [n_inside]; crowded [n_inside] bool; counts [n_inside] run lengths; T [n_inside + 1] uint64 exclusive sums; pairs [total]
    SOURCE slots and d2 [total] binary32 in CSR order; qrow [total] the pair's query row, jrow [total] its row in the source's stable order by cell
    (ascending within a run); offsets: the set of cell offsets (source - query) over all pairs; n_alive, n_outside of fx; s_inside"""
    pos_q, pos_s = np.asarray(pos_q, F32).reshape(-1, 3), np.asarray(pos_s, F32).reshape(-1, 3)
    aq, as_ = np.asarray(alive_q, np.int64), np.asarray(alive_s, np.int64)
    dims, origin, inv_cell = grid
    dims = [int(d) for d in dims]
    n_cells = dims[0] * dims[1] * dims[2]

    def sort(pos, alive):
        cells = np_cells(pos[alive], dims, origin, inv_cell).astype(np.int64) if len(alive) else np.zeros(0, np.int64)
        order = np.argsort(cells, kind="stable")
        n = int((cells != n_cells).sum())
        return alive[order][:n], cells[order][:n]

    rows, cq = sort(pos_q, aq)
    srows, cs = sort(pos_s, as_)
    xyz = lambda c: (c % dims[0], (c // dims[0]) % dims[1], c // (dims[0] * dims[1]))
    qx, qy, qz = xyz(cq)
    jx, jy, jz = xyz(cs)
    r2 = F32(radius) * F32(radius)
    n_inside = len(rows)
    cand = np.zeros(n_inside, np.int64)
    Q, J, D = [], [], []
    for b in range(0, n_inside, 512):
        q = np.arange(b, min(b + 512, n_inside))
        near = (np.abs(qx[q, None] - jx[None, :]) <= 1) & (np.abs(qy[q, None] - jy[None, :]) <= 1) & (np.abs(qz[q, None] - jz[None, :]) <= 1)
        cand[q] = near.sum(axis=1)                                         # the inside sources of the at most 27 cells: the query is not among them
        near &= (cand[q] <= int(candidate_limit))[:, None]                 # a crowded query lists nothing
        qi, ji = np.nonzero(near)                                          # row-major: by query, then by ascending source row
        qi = q[qi]
        d2 = np_d2_from(pos_q[rows[qi]], pos_s[srows[ji]])
        nb = d2 < r2
        Q.append(qi[nb]); J.append(ji[nb]); D.append(d2[nb])
    qrow = np.concatenate(Q) if Q else np.zeros(0, np.int64)
    jrow = np.concatenate(J) if J else np.zeros(0, np.int64)
    d2 = np.concatenate(D).astype(F32) if D else np.zeros(0, F32)
    assert (np.diff(qrow) >= 0).all() and ((np.diff(jrow) > 0) | (np.diff(qrow) > 0)).all(), "CSR order: by query row, then by ascending source row"
    counts = np.bincount(qrow, minlength=n_inside).astype(np.int64)
    T = np.zeros(n_inside + 1, np.uint64)
    T[1:] = np.cumsum(counts).astype(np.uint64)
    offsets = set(zip((jx[jrow] - qx[qrow]).tolist(), (jy[jrow] - qy[qrow]).tolist(), (jz[jrow] - qz[qrow]).tolist()))
    return dict(rows=rows, cells=cq, cand=cand, crowded=cand > int(candidate_limit), counts=counts, T=T, pairs=srows[jrow].astype(np.int64), d2=d2, qrow=qrow, jrow=jrow,
                offsets=offsets, n_alive=len(aq), n_outside=len(aq) - n_inside, s_inside=len(srows), srows=srows)


def pairs_from_buffers(ref, capacity, pair_capacity):
    """what a call leaves behind; capacity is FX's -> (out_rows [capacity], out_start [capacity + 1], written, out_pairs[:written],
    out_d2[:written] as words, stats [8])"""
    n = len(ref["rows"])
    total = int(ref["T"][n])
    out_rows = np.full(capacity, NO_ROW, U32)
    out_rows[:n] = ref["rows"]
    start = np.empty(capacity + 1, np.uint64)
    start[: n + 1] = np.minimum(ref["T"], np.uint64(pair_capacity))
    start[n + 1:] = start[n]
    written = min(total, pair_capacity)
    stats = np.array([ref["n_alive"], n, ref["n_outside"], int(ref["crowded"].sum()), total & 0xFFFFFFFF, total >> 32, written, ref["s_inside"]], np.uint64).astype(U32)
    return out_rows, start.astype(U32), written, ref["pairs"][:written].astype(U32), ref["d2"][:written].view(U32), stats


def pairs_from_plan(cap_q, cap_s, n_cells):
    """pairs_from_launch_plan restated -> (source sort [(kernel, grid x)], its memset index or None, query sort, its memset index, pack, count, scan,
    fill grids): the sorts are neighbours_from's"""
    return from_plan(cap_q, cap_s, n_cells)[:4] + (max(1, -(-cap_s // 256)), max(1, -(-cap_q // 256)), 1, -(-(cap_q + 1) // 256))


def pairs_from_layout(cap_q, cap_s, n_cells):
    """pairs_from_scratch_layout restated -> (tiles, q_sort_off, snap_off, snap_bytes, count_off, count_bytes, tile_off, tile_bytes, cells_off,
    cells_bytes, total)"""
    up = lambda x: (x + 255) & ~255
    ss, sq = sort_layout(1, cap_s, INSTANCE), sort_layout(1, cap_q, INSTANCE)
    tiles = max(1, -(-cap_q // 256))
    q_sort_off = up(ss[10])
    snap_off = up(q_sort_off + sq[10])
    count_off = up(snap_off + ss[2] * 16)
    tile_off = up(count_off + sq[2] * 4)
    cells_off = up(tile_off + (tiles + 1) * 8)
    return (tiles, q_sort_off, snap_off, ss[2] * 16, count_off, sq[2] * 4, tile_off, (tiles + 1) * 8, cells_off, (n_cells + 2) * 4, up(cells_off + (n_cells + 2) * 4))


LINE_GRID = ((4, 1, 1), (0, 0, 0), (1, 1, 1))


def test_the_restatement_itself_on_cases_worked_by_hand():
    run = lambda pq, aq, ps, as_, radius=1.0, limit=100, g=LINE_GRID: np_pairs_from(pq, aq, ps, as_, g, radius, limit)
    # a coincident source is a neighbour, and equal slot numbers are not excluded: query slot 0 and source slot 0 on one point. Sources: slot 1
    # in cell 1, slot 0 in cell 0 -> the source's rows are slots 0, 1; query slot 1 (cell 2) sees source slot 1 only
    pq = np.array([(0.5, 0.5, 0.5), (2.25, 0.5, 0.5)], F32)
    ps = np.array([(0.5, 0.5, 0.5), (1.4, 0.5, 0.5)], F32)
    r = run(pq, [1, 0], ps, [1, 0])
    assert r["rows"].tolist() == [0, 1] and r["cand"].tolist() == [2, 1] and r["counts"].tolist() == [2, 1] and r["T"].tolist() == [0, 2, 3]
    assert r["pairs"].tolist() == [0, 1, 1] and r["d2"].tolist()[0] == 0.0 and r["offsets"] == {(0, 0, 0), (1, 0, 0), (-1, 0, 0)} and r["s_inside"] == 2
    rows, start, written, pairs, d2, stats = pairs_from_buffers(r, 3, 100)
    assert rows.tolist() == [0, 1, NO_ROW] and start.tolist() == [0, 2, 3, 3] and stats.tolist() == [2, 2, 0, 0, 3, 0, 3, 2]
    rows, start, written, pairs, d2, stats = pairs_from_buffers(r, 3, 1)   # truncated inside the first run: a prefix, the table clamped
    assert start.tolist() == [0, 1, 1, 1] and pairs.tolist() == [0] and stats.tolist() == [2, 2, 0, 0, 3, 0, 1, 2]
    # a run holds source slots in the SOURCE's sorted row order - by cell, then list order -, not in slot order: the sources of cell 0 in list order 2, 0
    ps = np.array([(0.4, 0.5, 0.5), (1.2, 0.5, 0.5), (0.6, 0.5, 0.5)], F32)
    r = run(np.array([(0.5, 0.5, 0.5)], F32), [0], ps, [2, 1, 0])
    assert r["srows"].tolist() == [2, 0, 1] and r["pairs"].tolist() == [2, 0, 1] and r["jrow"].tolist() == [0, 1, 2]
    # a source exactly at d2 == r2 is out; one ulp nearer it is in
    pq = np.array([(0.25, 0.5, 0.5)], F32)
    ps = np.array([(1.25, 0.5, 0.5), (np.nextafter(F32(1.25), F32(0)), 0.5, 0.5)], F32)
    assert np_d2_from(pq, ps[:1])[0] == F32(1.0)
    assert run(pq, [0], ps, [0])["counts"].tolist() == [0] and run(pq, [0], ps, [1])["counts"].tolist() == [1] and run(pq, [0], ps, [0])["cand"].tolist() == [1]
    # a pair two cells apart is out even when d2 < r2 by rounding: cells of 1/11, the radius the largest binary32 the coverage rule takes there. The
    # query's t rounds into cell 127 and the source's into cell 129, yet the rounded d2 is below the rounded r2
    eleven = ((130, 1, 1), (0, 0, 0), (11, 1, 1))
    radius = F32(0.09090908616781235)
    assert float(radius) * 11.0 <= 1.0 < float(np.nextafter(radius, F32(1))) * 11.0
    pq, ps = np.array([(11.63636302947998, 0.5, 0.5)], F32), np.array([(11.727272033691406, 0.5, 0.5), (11.7, 0.5, 0.5)], F32)
    assert np_cells(pq, *eleven).tolist() == [127] and np_cells(ps, *eleven).tolist() == [129, 128] and np_d2_from(pq, ps[:1])[0] < radius * radius
    r = run(pq, [0], ps, [0], radius=radius, g=eleven)
    assert r["counts"].tolist() == [0] and r["cand"].tolist() == [0] and not r["crowded"].any()
    r = run(pq, [0], ps, [0, 1], radius=radius, g=eleven)                  # ... while the source one cell away is listed
    assert r["pairs"].tolist() == [1] and r["cand"].tolist() == [1] and r["offsets"] == {(1, 0, 0)}
    # an outside source is in no run and is no candidate; a NaN source neither; a dead source neither
    pq = np.array([(3.5, 0.5, 0.5)], F32)
    ps = np.array([(4.25, 0.5, 0.5), (np.nan, 0.5, 0.5), (3.75, 0.5, 0.5), (3.25, 0.5, 0.5)], F32)
    r = run(pq, [0], ps, [0, 1, 2])
    assert r["pairs"].tolist() == [2] and r["cand"].tolist() == [1] and r["s_inside"] == 1
    # an outside query has no row and is counted; a dead query is not even visited
    pq = np.array([(-0.25, 0.5, 0.5), (0.25, 0.5, 0.5), (0.3, 0.5, 0.5), (np.inf, 0.5, 0.5)], F32)
    ps = np.array([(0.1, 0.5, 0.5)], F32)
    r = run(pq, [1, 0, 3], ps, [0])
    assert r["rows"].tolist() == [1] and r["pairs"].tolist() == [0] and (r["n_alive"], r["n_outside"]) == (3, 2)
    assert pairs_from_buffers(r, 4, 9)[5].tolist() == [3, 1, 2, 0, 1, 0, 1, 1] and pairs_from_buffers(r, 4, 9)[0].tolist() == [1, NO_ROW, NO_ROW, NO_ROW]
    # crowding is decided by the sources alone: three queries in a cell with two sources and a limit of 2 list them; a third source crowds them
    pq = np.array([(0.2, 0.5, 0.5), (0.4, 0.5, 0.5), (0.6, 0.5, 0.5), (3.5, 0.5, 0.5)], F32)
    ps = np.array([(0.3, 0.5, 0.5), (1.5, 0.5, 0.5), (0.7, 0.5, 0.5)], F32)
    r = run(pq, [0, 1, 2, 3], ps, [0, 1], limit=2)
    assert r["cand"].tolist() == [2, 2, 2, 0] and not r["crowded"].any() and r["counts"].tolist() == [1, 1, 2, 0] and r["pairs"].tolist() == [0, 0, 0, 1]
    r = run(pq, [0, 1, 2, 3], ps, [0, 1, 2], limit=2)
    assert r["cand"].tolist() == [3, 3, 3, 0] and r["crowded"].tolist() == [True, True, True, False] and not r["counts"].any()
    assert pairs_from_buffers(r, 4, 9)[5].tolist() == [4, 4, 0, 3, 0, 0, 0, 3] and not pairs_from_buffers(r, 4, 9)[1].any()
    # a query in an empty neighbourhood: an empty run between two others
    pq = np.array([(0.5, 0.5, 0.5), (2.5, 0.5, 0.5), (3.5, 0.5, 0.5)], F32)
    ps = np.array([(0.6, 0.5, 0.5), (3.6, 0.5, 0.5)], F32)
    r = run(pq, [0, 1, 2], ps, [0, 1], radius=0.5)
    assert r["cand"].tolist() == [1, 1, 1] and r["counts"].tolist() == [1, 0, 1] and pairs_from_buffers(r, 3, 9)[1].tolist() == [0, 1, 1, 2]
    # the restatement speaks the library's own words: the sentinel of the binding, and the kernels and the tile of hnb_pairs_from.h
    assert NO_ROW == runtime.PAIRS_NO_ROW
    text = open(os.path.join(CSRC, "hnb_pairs_from.h")).read()
    assert all(f'"{k}"' in text for k in PAIRS_FROM_KERNELS) and "constexpr uint32_t kPairsFromBlock = 256;" in text
    assert pairs_from_plan(4096, 4097, 62) == ([("bin_keys", 2)] + [(n, 2) for n in ("sort_scatter", "sort_hist", "sort_scatter", "sort_hist", "sort_scatter", "sort_hist", "sort_scatter")]
                                               + [("bin_starts", 1)], 0, [("bin_tile", 1)], None, 17, 16, 1, 17)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------------
def test_ctypes_header_and_integration_agree_on_the_prototype(tmp_path):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd_pairs_from.h"
    int main(void) {
        int (*fe)(HnbEffect*, HnbEffect*, const HnbPairsDesc*) = hnb_effect_pairs_from;
        int (*fp)(HnbEffect*, const HnbPairsDesc*) = hnb_effect_pairs;
        printf("%zu", sizeof(HnbPairsDesc));
    ''' + "\n".join(f'        printf(" %zu", offsetof(HnbPairsDesc, {m}));' for m in MEMBERS) + r'''
        printf("\n");
        return fe == 0 || fp == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()]
    D = runtime.PairsDesc
    assert got == [96, 0, 4, 8, 20, 24, 36, 48, 52, 56, 64, 72, 80, 88]    # the descriptor is HnbPairsDesc unchanged
    assert C.sizeof(D) == 96 and [C.sizeof(D)] + [getattr(D, m).offset for m in MEMBERS] == got
    lib = runtime.load_library()
    assert runtime.ABI_PAIRS_FROM_SYMBOLS == ["hnb_effect_pairs_from"]
    full = open(os.path.join(ROOT, "include", "hanabi_amd_pairs_from.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(lib, "hnb_effect_pairs_from") and lib.hnb_effect_pairs_from.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(runtime.PairsDesc)]
    exported = subprocess.run([f"{LLVM}/llvm-readelf", "--dyn-syms", hb.runtime_lib_path()], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bFUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+hnb_effect_pairs_from$", exported, flags=re.M), "the library exports the symbol"
    m = re.search(r"int\s+hnb_effect_pairs_from\s*\(([^)]*)\)\s*;", header)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["HnbEffect* fx", "HnbEffect* source", "const HnbPairsDesc* desc"]
    m = re.search(r"\bfn hnb_effect_pairs_from\(([^)]*)\) -> c_int;", txt)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["fx: *mut HnbEffect", "source: *mut HnbEffect", "desc: *const HnbPairsDesc"]
    assert "pub unsafe fn effect_pairs_from(" in txt and "pub mod pairs_from {" in txt
    section = txt[txt.index("### Neighbour pairs across effects"):]
    assert "pair_capacity = 0" in section and "stats[4]" in section, "a count-then-allocate example"
    assert list(inspect.signature(runtime.Effect.pairs_from).parameters) == ["self", "source", "dims", "origin", "inv_cell", "radius", "rows_ptr", "start_ptr", "pairs_ptr", "pair_capacity",
                                                                             "d2_ptr", "stats_ptr", "candidate_limit"]
    assert not hasattr(runtime.Program, "pairs_from")                      # (no program form: out of scope, the header says so)
    # every header declares exactly its own symbols: hanabi_amd.h and its 61 are as they were, and the companion lists do not overlap
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", header)) == set(runtime.ABI_PAIRS_FROM_SYMBOLS)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", main)) == set(runtime.ABI_SYMBOLS) and len(runtime.ABI_SYMBOLS) == 61
    for name, syms in (("hanabi_amd_neighbours.h", runtime.ABI_NEIGHBOUR_SYMBOLS), ("hanabi_amd_pairs.h", runtime.ABI_PAIRS_SYMBOLS),
                       ("hanabi_amd_neighbours_from.h", runtime.ABI_NEIGHBOURS_FROM_SYMBOLS)):
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", other)) == set(syms)
    lists = [n for n in dir(runtime) if re.fullmatch(r"ABI_[A-Z_]*SYMBOLS", n)]
    assert len(lists) >= 11 and "ABI_PAIRS_FROM_SYMBOLS" in lists and "ABI_SYMBOLS" in lists and "ABI_NEIGHBOURS_FROM_SYMBOLS" in lists
    for n in lists:
        if n != "ABI_PAIRS_FROM_SYMBOLS":
            assert not set(runtime.ABI_PAIRS_FROM_SYMBOLS) & set(getattr(runtime, n)), n
    for inc in ('#include "hanabi_amd.h"', '#include "hanabi_amd_binned.h"', '#include "hanabi_amd_neighbours.h"', '#include "hanabi_amd_pairs.h"'):
        assert inc in full
    assert "struct" not in header                                          # there is no new struct
    bound = set(re.findall(r"pub fn (hnb_[a-z0-9_]+)\(", txt))
    assert not set(runtime.ABI_PAIRS_FROM_SYMBOLS) & bound                 # (the `pub fn` set mirrors hanabi_amd.h and the host header: the call sits in a module of its own)
    flat = " ".join(full.replace(" * ", " ").split())
    for word in ("no self-exclusion", "a coincident source is a neighbour", "equal slot numbers mean nothing", "same context", "OUTSIDE BIN", "CROWDED", "the query is not among them",
                 "d2 = s + zz", "this call lifts that item", "fx == source", "hnb_effect_pairs'", "HnbPairsDesc unchanged", "One grid serves both sides", "capacity is FX's slot count",
                 "SOURCE slots", "ascending sorted-row order of the source", "flags must be 0", "HNB_PAIRS_HALF is refused", "a slot order across two effects means nothing",
                 "min(T[r], pair_capacity)", "keep every bit", "the call counts only", "[7] = the inside sources", "writes nothing of either effect", "Frozen instances are accepted on both sides",
                 "0xFFFFFF00 slots", "Out of scope: a program form", "more than one source effect per call", "different grids for the two sides", "a transform between the effects' spaces",
                 "ELL (fixed-stride) output", "a HALF form", "that overlap"):
        assert word in flat, word
    # the two headers whose out-of-scope item this one lifts are as they were
    assert "pairs across effects" in open(os.path.join(ROOT, "include", "hanabi_amd_pairs.h")).read()
    assert "a pair list across effects" in open(os.path.join(ROOT, "include", "hanabi_amd_neighbours_from.h")).read()
    assert "hnb_effect_pairs_from" in open(os.path.join(ROOT, "README.md")).read()


def test_call_fails_loudly_on_null_arguments_and_without_a_device():
    """Up to the device check: the NULL refusals come before anything is dereferenced, loaded or enqueued. The other refusals need two effects, and
    an effect a device: the stand-alone program below holds them, and tests/test_gpu_pairs_from.py on live effects."""
    lib = runtime.load_library()
    d = runtime.pairs_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 1.0, 0x1000, 0x2000)
    fake, fake2 = C.c_void_p(0x1000), C.c_void_p(0x2000)   # never dereferenced: the NULL argument is refused first
    for args in ((None, fake2, C.byref(d)), (fake, None, C.byref(d)), (fake, fake2, None), (None, None, None)):
        assert lib.hnb_effect_pairs_from(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no effect to list, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the code object --------------------------------------------------------------------------------------------------------------------------------
def test_code_object_is_built_carried_and_has_its_two_kernels_without_scratch_or_spills():
    co = hb.pairs_from_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_pairs_from.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(PAIRS_FROM_KERNELS), sorted(rows)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert design.index("## Neighbours across effects") < design.index("## Neighbour pairs across effects (`hnb_effect_pairs_from`)") < design.index("## Measurement (row d)")
    section = design[design.index("## Neighbour pairs across effects"): design.index("## Measurement (row d)")]
    for name, r in rows.items():
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["kernarg_segment_size"] == 184, (name, r)                # one PairsFromArgs by value
        assert r["vgpr_count"] <= 64, (name, r)                           # eight waves per SIMD stay possible
        assert r["group_segment_fixed_size"] <= 32, (name, r)             # the stats' and the waves' four words each: the candidates are not staged in LDS
        row = f"| `{name}` | {r['vgpr_count']} | {r['sgpr_count']} | {r['group_segment_fixed_size']} |"
        assert row in section, f"DESIGN.md \"Neighbour pairs across effects\" resource table: {row}"      # (a recorded value, not a preset bound)
    assert "query snapshot" in section and "Measured" in section
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_pairs_from_code)
    for h in ("hnb_pairs_from.h", "hnb_pairs.h", "hnb_neighbours_from.h", "hnb_neighbours.h", "hnb_deposit.h", "hnb_bin_cell.h", "hnb_export_bin.h"):
        assert f'"{h}"' in inspect.getsource(hb.build_pairs_from_code)
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_pairs_from.hip")).read()
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_pairs_from.h")).read()
    assert hb.PAIRS_FROM_CODE_OBJECTS == (hb.build_pairs_from_code,)
    assert hb.PAIRS_CODE_OBJECTS == (hb.build_pairs_code,) and hb.NEIGHBOURS_FROM_CODE_OBJECTS == (hb.build_neighbours_from_code,)
    assert "PAIRS_FROM_CODE_OBJECTS" in inspect.getsource(hb.build_runtime) and "hanabi_amd_pairs_from.h" in inspect.getsource(hb.build_runtime)
    assert "hanabi_amd_pairs_from.h" in inspect.getsource(hb._build_code_object)
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "bevy_hanabi_amd/csrc/hnb_pairs_from_code.inc" in ignored and "*.hsaco" in ignored
    for other in (hb.neighbours_code_path(), hb.pairs_code_path(), hb.neighbours_from_code_path(), hb.export_bin_code_path(), hb.sample_code_path(), hb.deposit_code_path(),
                  hb.export_sort_code_path(), hb.export_filter_code_path()):
        assert not set(_rows(other)) & set(PAIRS_FROM_KERNELS)
    # the units whose kernels the call borrows are as they were: the snapshot and the scan
    assert sorted(_rows(hb.neighbours_code_path())) == ["k_neighbours_gather", "k_neighbours_pack"]
    assert sorted(_rows(hb.pairs_code_path())) == ["k_pairs_count", "k_pairs_fill", "k_pairs_scan"] and _rows(hb.pairs_code_path())["k_pairs_scan"]["kernarg_segment_size"] == 168


# ---- csrc/hnb_pairs_from.h as a stand-alone host program under the sanitizers -------------------------------------------------------------------------
ERRORS = ["Ok", "ErrSameEffect", "ErrContexts", "ErrStructSize", "ErrHalf", "ErrFlags", "ErrDims", "ErrOrigin", "ErrInvCell", "ErrRadius", "ErrCoverage", "ErrRadiusSquared",
          "ErrCandidateLimit", "ErrNoPosition", "ErrSourceNoPosition", "ErrCapacity", "ErrSourceCapacity", "ErrNullRows", "ErrNullStart", "ErrNullPairs", "ErrAlign", "ErrStats",
          "ErrOverlap"]
E = {n: i for i, n in enumerate(ERRORS)}
# what the check is given: (attr, ncomp, is_f32) of fx and of the source, POSITION at different indices; from entry 1 on fx has no POSITION, and the
# source's at entry 1 has two components: no POSITION of 3 f32 from entry 1 on either
LAYOUT_Q = [(A.POSITION.id, 3, 1), (A.VELOCITY.id, 3, 1), (A.AGE.id, 1, 1), (A.LIFETIME.id, 1, 1)]
LAYOUT_S = [(A.POSITION.id, 3, 1), (A.POSITION.id, 2, 1), (A.AGE.id, 1, 1), (A.COLOR.id, 1, 0)]

HOST_SRC = r"""
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>
#include "hnb_pairs_from.h"
using namespace hnb;
""" + "\n".join(f"static_assert(kPairsFrom{n} == {i}, \"PairsFromDescError\");" for i, n in enumerate(ERRORS)) + r"""
static_assert(kPairsFromDescErrorCount == """ + str(len(ERRORS)) + r""", "PairsFromDescError");
static_assert(sizeof(HnbPairsDesc) == 96 && sizeof(PairsFromArgs) == 184 && sizeof(PairsArgs) == 168 && sizeof(NeighbourArgs) == 248, "hnb_pairs_from.h");
static_assert(kPairsFromKCount == 0 && kPairsFromKFill == 1 && kPairsFromKernelCount == 2 && kPairsKScan == 1, "hnb_pairs_from.h");
static_assert(kPairsFromBlock == 256 && kPairsFromStatsWords == 8 && sizeof(PairsSnap) == 16, "hnb_pairs_from.h");
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
// one side of a state: the alive particles in list order -> their cells and the stable order by cell
struct Side { std::vector<uint32_t> slot, pos, cell, order; };
static int read_side(Side& s, unsigned n, const BinGrid& g) {
    s.slot.resize(n); s.pos.resize(3 * (size_t)n); s.cell.resize(n); s.order.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (std::scanf("%u %x %x %x", &s.slot[i], &s.pos[3 * i], &s.pos[3 * i + 1], &s.pos[3 * i + 2]) != 4) return 1;
    for (size_t i = 0; i < n; ++i) s.cell[i] = bin_cell_of(g, f_of(s.pos[3 * i]), f_of(s.pos[3 * i + 1]), f_of(s.pos[3 * i + 2]));
    std::iota(s.order.begin(), s.order.end(), 0u);
    std::stable_sort(s.order.begin(), s.order.end(), [&](uint32_t x, uint32_t y) { return s.cell[x] < s.cell[y]; });
    return 0;
}
int main() {
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "names")) {
            for (uint32_t i = 0; i < kPairsFromKernelCount; ++i) std::printf("%u:%s ", kPairsFromKernelNames[i].kernel, kPairsFromKernelNames[i].name);
            std::printf("\n");
        } else if (!std::strcmp(what, "texts")) {
            for (uint32_t e = 0; e < kPairsFromDescErrorCount; ++e) std::printf("%s|", pairs_from_error_text(e));
            std::printf("\n");
        } else if (!std::strcmp(what, "plan")) {
            unsigned cq, cs, n_cells;
            if (std::scanf("%u %u %u", &cq, &cs, &n_cells) != 3) return 1;
            const PairsFromPlan pl = pairs_from_launch_plan(cq, cs, n_cells);
            std::printf("%u %u %u %u %llu", pl.pack_grid, pl.count_grid, pl.scan_grid, pl.fill_grid, (unsigned long long)pl.clear_stats_bytes);
            if (print_sort(pl.source_sort, cs)) return 5;
            if (print_sort(pl.query_sort, cq)) return 5;
            std::printf("\n");
        } else if (!std::strcmp(what, "layout")) {
            unsigned cq, cs, n_cells;
            if (std::scanf("%u %u %u", &cq, &cs, &n_cells) != 3) return 1;
            const PairsFromScratch l = pairs_from_scratch_layout(cq, cs, n_cells);
            std::printf("%u %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %u %u %u %u\n", l.tiles, (unsigned long long)l.q_sort_off, (unsigned long long)l.snap_off,
                        (unsigned long long)l.snap_bytes, (unsigned long long)l.count_off, (unsigned long long)l.count_bytes, (unsigned long long)l.tile_off,
                        (unsigned long long)l.tile_bytes, (unsigned long long)l.cells_off, (unsigned long long)l.cells_bytes, (unsigned long long)l.total,
                        (unsigned long long)l.s_sort.total, (unsigned long long)l.q_sort.total, l.s_sort.pitch, l.q_sort.pitch, l.s_sort.rows, l.q_sort.rows);
        } else if (!std::strcmp(what, "run")) {   // a whole state through the header: the source's cells, stable sort, table, snapshot; the queries' stable sort; the count of every query row, a host scan, the fill
            BinGrid g = {};
            unsigned ob[3], ib[3], rb, limit, pc, want_d2, nq, ns;
            if (std::scanf("%u %u %u %x %x %x %x %x %x %x %u %u %u %u %u", &g.dims[0], &g.dims[1], &g.dims[2], &ob[0], &ob[1], &ob[2], &ib[0], &ib[1], &ib[2], &rb, &limit, &pc, &want_d2,
                           &nq, &ns) != 15) return 1;
            for (int c = 0; c < 3; ++c) { g.origin[c] = f_of(ob[c]); g.inv_cell[c] = f_of(ib[c]); }
            g.n_cells = bin_cell_count(g.dims);
            Side q, s;
            if (read_side(q, nq, g) || read_side(s, ns, g)) return 1;
            const float radius = f_of(rb), r2 = radius * radius;
            std::vector<uint32_t> start(export_bin_entries(g.n_cells));     // exactly n_cells + 2 entries on the heap: a read past them is an error the sanitizer reports
            for (uint32_t c = 0; c < start.size(); ++c)
                start[c] = (uint32_t)(std::lower_bound(s.order.begin(), s.order.end(), c, [&](uint32_t row, uint32_t key) { return s.cell[row] < key; }) - s.order.begin());
            const uint32_t s_inside = start[g.n_cells];
            std::vector<PairsSnap> snap(s_inside);                          // exactly the inside source rows: no walk may read an outside one
            for (uint32_t r = 0; r < s_inside; ++r) snap[r] = {s.pos[3 * s.order[r]], s.pos[3 * s.order[r] + 1], s.pos[3 * s.order[r] + 2], s.slot[s.order[r]]};
            uint32_t n_inside = 0;
            while (n_inside < nq && q.cell[q.order[n_inside]] < g.n_cells) ++n_inside;      // the outside rows form the tail: the sort is ascending
            std::vector<uint32_t> count(n_inside), crowded(n_inside);
            std::vector<uint64_t> T(n_inside + 1u, 0u);
            const auto at = [&](uint32_t r, int c) { return f_of(q.pos[3 * q.order[r] + c]); };
            for (uint32_t r = 0; r < n_inside; ++r) {
                const PairsFromRowCount rc = pairs_from_row_count(snap.data(), start.data(), g.dims, q.cell[q.order[r]], at(r, 0), at(r, 1), at(r, 2), limit, r2);
                count[r] = rc.count; crowded[r] = rc.crowded;
                if (rc.crowded && rc.count) return 6;
                T[r + 1u] = T[r] + rc.count;
            }
            std::vector<uint32_t> out_pairs(pc, 0xDEADBEEFu);               // exactly pair_capacity entries: a store past them is an error the sanitizer reports
            std::vector<float> out_d2(want_d2 ? pc : 0u, f_of(0xDEADBEEFu));
            for (uint32_t r = 0; r < n_inside; ++r) {
                if (crowded[r]) continue;
                const uint32_t k = pairs_from_row_fill(snap.data(), start.data(), g.dims, q.cell[q.order[r]], at(r, 0), at(r, 1), at(r, 2), r2, T[r], pc, pc ? out_pairs.data() : nullptr,
                                                       want_d2 && pc ? out_d2.data() : nullptr);
                if (k != count[r]) return 7;
            }
            std::printf("%u %llu %u |", n_inside, (unsigned long long)T[n_inside], s_inside);
            for (uint32_t r = 0; r < n_inside; ++r) std::printf(" %u", q.slot[q.order[r]]);
            std::printf(" |");
            for (uint32_t r = 0; r < n_inside; ++r) std::printf(" %u", crowded[r]);
            std::printf(" |");
            for (uint32_t r = 0; r <= n_inside; ++r) std::printf(" %u", pairs_clamp(T[r], pc));
            std::printf(" |");
            for (uint32_t v : out_pairs) std::printf(" %u", v);
            std::printf(" |");
            for (float v : out_d2) std::printf(" %x", b_of(v));
            std::printf("\n");
        } else if (!std::strcmp(what, "desc")) {
            HnbPairsDesc d;
            std::memset(&d, 0, sizeof d);
            unsigned long long ptr[5]; unsigned same_fx, same_ctx, q_first, s_first, cq, cs, ob[3], ib[3], rb;
            if (std::scanf("%u %u %u %u %u %u %u %u %u %u %u %u %x %x %x %x %x %x %x %u %llx %llx %llx %llx %llx", &same_fx, &same_ctx, &q_first, &s_first, &cq, &cs, &d.struct_size, &d.flags,
                           &d.dims[0], &d.dims[1], &d.dims[2], &d.candidate_limit, &ob[0], &ob[1], &ob[2], &ib[0], &ib[1], &ib[2], &rb, &d.pair_capacity, &ptr[0], &ptr[1], &ptr[2], &ptr[3],
                           &ptr[4]) != 25) return 1;
            std::memcpy(d.origin, ob, 12); std::memcpy(d.inv_cell, ib, 12); d.radius = f_of(rb);
            d.out_rows = (uint32_t*)(uintptr_t)ptr[0]; d.out_start = (uint32_t*)(uintptr_t)ptr[1]; d.out_pairs = (uint32_t*)(uintptr_t)ptr[2];
            d.out_d2 = (float*)(uintptr_t)ptr[3]; d.out_stats = (uint32_t*)(uintptr_t)ptr[4];
            if (q_first > 1 || s_first > 1) return 1;
            const NeighboursFromSide fx = {kLayoutQ + q_first, (uint32_t)(sizeof kLayoutQ / sizeof *kLayoutQ) - q_first, cq};
            const NeighboursFromSide source = {kLayoutS + s_first, (uint32_t)(sizeof kLayoutS / sizeof *kLayoutS) - s_first, cs};
            const PairsFromCheck c = pairs_from_check_desc(d, fx, source, same_fx != 0, same_ctx != 0);
            if (c.error >= kPairsFromDescErrorCount || !pairs_from_error_text(c.error)[1]) return 3;
            std::printf("%u %u %u %u %u %x\n", c.error, c.index, c.n_cells, c.q_position_index, c.s_position_index, b_of(c.r2));
        } else return 4;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """g++ alone, with the address and undefined-behaviour sanitizers and no contraction: the header is plain C++ on the host. The program has its
    own main and is run directly."""
    tmp = tmp_path_factory.mktemp("pairs_from_host")
    (tmp / "pairs_from.cpp").write_text(HOST_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), str(tmp / "pairs_from.cpp"), "-o", str(tmp / "pairs_from")])
    return str(tmp / "pairs_from")


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()      # (a sanitizer report ends the program with an error)
    assert len(out) == len(lines)
    return out


def _f32(x):
    return int(np.array([x], F32).view(U32)[0])


def _desc_line(same_fx=0, same_ctx=1, q_first=0, s_first=0, cap_q=10_000, cap_s=7000, struct_size=96, flags=0, dims=(4, 4, 4), limit=4096, origin=(0.0, 0.0, 0.0),
               inv_cell=(1.0, 1.0, 1.0), radius=0.75, pc=5000, rows=0x100000, start=0x200000, pairs=0x300000, d2=0x400000, stats=0x500000):
    return ("desc %d %d %d %d %d %d %d %d %d %d %d %d " % (same_fx, same_ctx, q_first, s_first, cap_q, cap_s, struct_size, flags, *dims, limit)
            + " ".join("%x" % _f32(x) for x in tuple(origin) + tuple(inv_cell) + (radius,)) + " %d %x %x %x %x %x" % (pc, rows, start, pairs, d2, stats))


FAR = dict(rows=0x1000_0000_0000, start=0x2000_0000_0000)                  # destinations far apart: room for the largest capacity


def test_description_check_refuses_what_the_header_lists_every_error_class_in_its_order(host_exe):
    raw = lambda **kw: _ask(host_exe, [_desc_line(**kw)])[0].split()
    ask = lambda **kw: [int(x) for x in raw(**kw)[:5]]
    hit = []

    def refused(name, index=None, **kw):
        got = ask(**kw)
        assert got[0] == E[name] and (index is None or got[1] == index), (name, kw, got)
        if name not in hit:
            hit.append(name)

    w = raw()
    assert [int(x) for x in w[:5]] == [E["Ok"], 0, 64, 0, 0] and int(w[5], 16) == _f32(F32(0.75) * F32(0.75))
    assert ask(radius=1.0, limit=1, stats=0, d2=0)[0] == E["Ok"] and ask(limit=65536, cap_q=0xFFFFFF00, cap_s=0xFFFFFF00, **FAR)[0] == E["Ok"]
    assert ask(pc=0, pairs=0, d2=0)[0] == E["Ok"] and ask(pc=0, pairs=0, d2=0x400000)[0] == E["Ok"]    # count only: out_pairs may be NULL
    # the two effects come first: before the struct size, and before each other in this order
    refused("ErrSameEffect", same_fx=1)
    refused("ErrSameEffect", same_fx=1, same_ctx=0, struct_size=0, flags=1)
    refused("ErrContexts", same_ctx=0)
    refused("ErrContexts", same_ctx=0, struct_size=0, flags=1, rows=0)
    for size in (0, 92, 100, 200):
        refused("ErrStructSize", struct_size=size)
    refused("ErrStructSize", struct_size=92, flags=1)
    for flags in (1, 3, 0x80000001):                                       # HALF, alone or among other bits: the text of its own
        refused("ErrHalf", flags=flags)
    for flags in (2, 4, 0x80000000):
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
    refused("ErrRadiusSquared", radius=1e-30, inv_cell=tiny)               # r2 = 0
    refused("ErrRadiusSquared", radius=1e20, inv_cell=tiny)                # r2 = inf
    assert ask(radius=1.1e-19, inv_cell=tiny)[0] == E["Ok"]
    for limit in (0, 65537, 0xFFFFFFFF):
        refused("ErrCandidateLimit", limit=limit)
    refused("ErrCandidateLimit", limit=0, q_first=1, s_first=1, rows=0)    # ... in front of everything behind it
    refused("ErrNoPosition", q_first=1)
    refused("ErrNoPosition", q_first=1, s_first=1, cap_q=0xFFFFFF01)       # fx's comes before the source's and before the capacities
    refused("ErrSourceNoPosition", s_first=1)
    refused("ErrSourceNoPosition", s_first=1, cap_q=0xFFFFFF01, cap_s=0xFFFFFF01)
    for cap in (0xFFFFFF01, 0xFFFFFFFF):
        refused("ErrCapacity", cap_q=cap, **FAR)
    refused("ErrCapacity", cap_q=0xFFFFFF01, cap_s=0xFFFFFF01, rows=0)
    for cap in (0xFFFFFF01, 0xFFFFFFFF):
        refused("ErrSourceCapacity", cap_s=cap)
    refused("ErrSourceCapacity", cap_s=0xFFFFFF01, rows=0)
    refused("ErrNullRows", rows=0)
    refused("ErrNullStart", start=0)
    refused("ErrNullPairs", pairs=0)
    refused("ErrNullPairs", pairs=0, pc=1)
    for index, name in enumerate(("rows", "start", "pairs", "d2")):
        for off in (1, 2, 3):
            refused("ErrAlign", index, **{name: 0x700000 + off})
    for off in (4, 8, 12):
        refused("ErrStats", 4, stats=0x500000 + off)
    cap, pc = 10_000, 5000
    # any two destination ranges: the later of the two is named. rows [cap], start [cap + 1], pairs / d2 [pc], stats [8] words - cap is FX's
    refused("ErrOverlap", 1, start=0x100000)                               # the same address
    refused("ErrOverlap", 1, start=0x100000 + 4 * (cap - 1))               # the last word of out_rows
    assert ask(start=0x100000 + 4 * cap)[0] == E["Ok"]                     # right behind it
    refused("ErrOverlap", 1, start=0x100000 - 4 * cap)                     # out_start's last word, entry `capacity`, is out_rows' first
    assert ask(start=0x100000 - 4 * (cap + 1))[0] == E["Ok"]
    # ... sized from fx's capacity, not from the source's: with a larger source the same addresses are fine, with a larger fx they are not
    assert ask(start=0x100000 + 4 * cap, cap_s=20_000)[0] == E["Ok"] and ask(start=0x100000 + 4 * 7000, cap_q=7000, cap_s=10_000)[0] == E["Ok"]
    refused("ErrOverlap", 1, start=0x100000 + 4 * cap, cap_q=cap + 1, cap_s=7000)
    refused("ErrOverlap", 2, pairs=0x200000 + 4 * cap)                     # into out_start's last entry
    assert ask(pairs=0x200000 + 4 * (cap + 1))[0] == E["Ok"]
    refused("ErrOverlap", 3, d2=0x300000 + 4 * (pc - 1))
    assert ask(d2=0x300000 + 4 * pc)[0] == E["Ok"]
    refused("ErrOverlap", 3, d2=0x300000)                                  # out_d2 == out_pairs
    refused("ErrOverlap", 4, stats=0x100000 + 16)                          # inside out_rows
    refused("ErrOverlap", 4, stats=0x400000 - 16)                          # its last 16 bytes reach into out_d2
    assert ask(stats=0x400000 - 32)[0] == E["Ok"]
    refused("ErrOverlap", 4, stats=0x300000 + 4 * pc - 16)                 # the tail of out_pairs
    assert ask(pc=0, pairs=0x100000, d2=0x100000)[0] == E["Ok"]            # nothing is written through a destination of no entries
    assert ask(d2=0, pairs=0x400000)[0] == E["Ok"]
    assert hit == ERRORS[1:], (hit, ERRORS[1:])                            # every error class, first met in the header's order
    got = raw(q_first=0, s_first=0)
    assert (int(got[3]), int(got[4])) == (0, 0)
    texts = _ask(host_exe, ["texts"])[0].split("|")[:-1]
    assert len(texts) == len(ERRORS) and len(set(texts)) == len(texts) and texts[0] == "ok"
    for name, word in (("ErrSameEffect", "hnb_effect_pairs'"), ("ErrContexts", "different contexts"), ("ErrHalf", "a slot order across two effects means nothing"),
                       ("ErrHalf", "HNB_PAIRS_HALF"), ("ErrFlags", "flags must be 0"), ("ErrDims", "HNB_BIN_MAX_CELLS"), ("ErrCoverage", "radius * inv_cell is above 1"),
                       ("ErrCandidateLimit", "candidate_limit is not 1.."), ("ErrNoPosition", "fx's particle layout has no POSITION"),
                       ("ErrSourceNoPosition", "the source's particle layout has no POSITION"), ("ErrCapacity", "fx has more than 0xFFFFFF00"),
                       ("ErrSourceCapacity", "the source has more than 0xFFFFFF00"), ("ErrNullRows", "out_rows is NULL"), ("ErrNullStart", "out_start is NULL"),
                       ("ErrNullPairs", "out_pairs is NULL"), ("ErrAlign", "4-byte aligned"), ("ErrStats", "16-byte aligned"), ("ErrOverlap", "overlap")):
        assert word in texts[E[name]], (name, texts[E[name]])
    assert "HNB_PAIRS_HALF" not in texts[E["ErrFlags"]]


CAPS = [1, 4096, 4097]


def test_scratch_layout_and_launch_plan_are_their_restatements_on_each_side_independently(host_exe):
    assert _ask(host_exe, ["names"])[0].split() == [f"{i}:{n}" for i, n in enumerate(PAIRS_FROM_KERNELS)]
    for cq in CAPS + [65_537]:
        for cs in CAPS + [65_537]:
            for n_cells in (1, 512, 68_921):
                lay, plan = _ask(host_exe, ["layout %d %d %d" % (cq, cs, n_cells), "plan %d %d %d" % (cq, cs, n_cells)])
                lay = [int(x) for x in lay.split()]
                want = pairs_from_layout(cq, cs, n_cells)
                ss, sq = sort_layout(1, cs, INSTANCE), sort_layout(1, cq, INSTANCE)
                assert tuple(lay[:11]) == want and lay[11:] == [ss[10], sq[10], ss[2], sq[2], cs, cq], (cq, cs, n_cells, lay, want)
                tiles, q_sort_off, snap_off, snap_b, count_off, count_b, tile_off, tile_b, cells_off, cells_b, total = lay[:11]
                assert all(o % 256 == 0 for o in (q_sort_off, snap_off, count_off, tile_off, cells_off, total))
                # the six sections in the header's order, none overlapping: the source's sort, fx's sort, the snapshot, the run lengths, the tile sums, the table
                assert ss[10] <= q_sort_off and q_sort_off + sq[10] <= snap_off and snap_off + snap_b <= count_off and count_off + count_b <= tile_off
                assert tile_off + tile_b <= cells_off and cells_off + cells_b <= total
                assert snap_b == 16 * ss[2] >= 16 * cs and count_b == 4 * sq[2] >= 4 * cq and tile_b == 8 * (tiles + 1) and cells_b == 4 * (n_cells + 2)
                assert (tiles - 1) * 256 < cq <= tiles * 256
                w = plan.split()
                Ls, ms, Lq, mq, pack, count, scan, fill = pairs_from_plan(cq, cs, n_cells)
                assert [int(x) for x in w[:5]] == [pack, count, scan, fill, 32], (cq, cs, w)
                k = 5
                for L, memset in ((Ls, ms), (Lq, mq)):
                    assert int(w[k]) == (-1 if memset is None else memset) and int(w[k + 1]) == len(L), (cq, cs, w)
                    got = [(x.split(":")[0], int(x.split(":")[1])) for x in w[k + 2: k + 2 + len(L)]]
                    assert got == L, (cq, cs, n_cells, got, L)
                    k += 2 + len(L)
                assert k == len(w)
                assert Ls[-1][0] == "bin_starts" and all(n != "bin_starts" for n, _ in Lq)       # the source plan ends in the table; the query plan has none
                assert (pack - 1) * 256 < cs <= pack * 256 and count == tiles and scan == 1
                assert (fill - 1) * 256 < cq + 1 <= fill * 256 and fill <= tiles + 1             # every query row and the entry behind them has a lane; a fill workgroup reads tile[t], t <= tiles
    l = [int(x) for x in _ask(host_exe, ["layout %d 64 64" % (0xFFFFFF00 + 1)])[0].split()]
    assert l[16] == 0 and l[15] == 64                                      # one above: no sort fits (q_sort.rows == 0) ...
    l = [int(x) for x in _ask(host_exe, ["layout 64 %d 64" % (0xFFFFFF00 + 1)])[0].split()]
    assert l[15] == 0 and l[16] == 64


# ---- whole states: the header's row bodies against the brute-force restatement -----------------------------------------------------------------------
def _run_line(pos_q, alive_q, pos_s, alive_s, grid, radius, limit, pc, want_d2):
    dims, origin, inv_cell = grid
    head = "run %d %d %d " % tuple(dims) + " ".join("%x" % _f32(x) for x in tuple(origin) + tuple(inv_cell) + (radius,)) + " %d %d %d %d %d " % (limit, pc, int(want_d2), len(alive_q),
                                                                                                                                                len(alive_s))
    wq, ws = np.asarray(pos_q, F32).view(U32).reshape(-1, 3), np.asarray(pos_s, F32).view(U32).reshape(-1, 3)
    return head + " ".join("%d %x %x %x" % (s, *wq[s]) for s in alive_q) + " " + " ".join("%d %x %x %x" % (s, *ws[s]) for s in alive_s)


def _assert_run(out, ref, n_slots, pc, want_d2):
    head, rows, crowded, start, pairs, d2 = [s.split() for s in out.split("|")]
    w_rows, w_start, written, w_pairs, w_d2, stats = pairs_from_buffers(ref, n_slots, pc)
    n_inside, total = len(ref["rows"]), int(ref["T"][-1])
    assert [int(x) for x in head] == [n_inside, total, ref["s_inside"]] and [int(x) for x in rows] == ref["rows"].tolist()
    assert [int(x) for x in crowded] == ref["crowded"].astype(int).tolist()
    assert [int(x) for x in start] == w_start[: n_inside + 1].tolist(), pc
    assert [int(x) for x in pairs] == w_pairs.tolist() + [SENT] * (pc - written), pc           # a prefix in CSR order; entries past it keep every bit
    assert [int(x, 16) for x in d2] == (w_d2.tolist() + [SENT] * (pc - written) if want_d2 else []), pc


def _cloud(rng, n, dims):
    """positions uniform in and a little around the unit cube - part of them outside -, a cluster in one cell, a NaN and an infinite position; a
    shuffled alive list with dead slots"""
    pos = rng.uniform(-0.05, 1.05, (n, 3)).astype(F32)
    pos[: n // 6] = (F32(0.4) + rng.uniform(0, 0.05, (n // 6, 3))).astype(F32)
    pos[-1] = (np.nan, 0.5, 0.5); pos[-2] = (0.5, np.inf, 0.5)
    alive = np.union1d(rng.permutation(n)[: n - n // 10], [n - 1, n - 2])   # a tenth of the slots is dead; the non-finite ones are alive
    return pos, alive[rng.permutation(len(alive))]


STATES = [((3, 3, 3), 0.3, 400, 300, 4096), ((5, 4, 3), 0.25, 300, 700, 4096), ((1, 1, 1), 1.0, 60, 40, 4096), ((2, 1, 7), 0.14, 300, 300, 110), ((4, 4, 4), 0.25, 200, 300, 60)]


@pytest.mark.parametrize("dims,radius,nq,ns,limit", STATES, ids=["x".join(map(str, s[0])) + f"-limit{s[4]}" for s in STATES])
def test_whole_states_through_the_row_bodies_are_the_brute_force_restatement_bit_for_bit(host_exe, dims, radius, nq, ns, limit):
    """two clouds with clusters in one cell (crowding under the small limits), coincident (query, source) pairs at equal and at other slot numbers,
    non-finite positions and dead slots on both sides; with and without d2; every truncation into destinations of exactly pair_capacity entries"""
    rng = np.random.default_rng(nq + ns)
    pos_q, alive_q = _cloud(rng, nq, dims)
    pos_s, alive_s = _cloud(rng, ns, dims)
    both = np.intersect1d(alive_q, alive_s)[:10]
    both = both[both < min(nq, ns) - 2]
    pos_s[both[:5]] = pos_q[both[:5]]                                      # coincident at equal slot numbers
    pos_s[both[5:]] = pos_q[both[:len(both[5:])]]                          # ... and at other ones
    grid = (dims, (0.0, 0.0, 0.0), tuple(float(d) for d in dims))
    ref = np_pairs_from(pos_q, alive_q, pos_s, alive_s, grid, radius, limit)
    total = int(ref["T"][-1])
    assert ref["n_outside"] >= 2 and ref["s_inside"] <= len(alive_s) - 2 and total > 0 and (ref["crowded"].any() == (limit < 4096))
    if limit == 4096:
        hit = (ref["d2"] == 0)
        assert (ref["pairs"][hit] == ref["rows"][ref["qrow"][hit]]).any() and (ref["pairs"][hit] != ref["rows"][ref["qrow"][hit]]).any(), "coincident pairs at equal and other slots"
    caps = [(pc, want_d2) for pc in truncations(ref) for want_d2 in ((True, False) if pc in (0, total) else (True,))]
    lines = [_run_line(pos_q, alive_q, pos_s, alive_s, grid, radius, limit, pc, want_d2) for pc, want_d2 in caps]
    for (pc, want_d2), out in zip(caps, _ask(host_exe, lines)):
        _assert_run(out, ref, nq, pc, want_d2)
    if dims == (3, 3, 3):
        assert len(ref["offsets"]) == 27                                   # every one of the 26 directions, and the own cell
    # the roles swapped list the transposed relation among those not crowded on either side
    back = np_pairs_from(pos_s, alive_s, pos_q, alive_q, grid, radius, limit)
    fwd = {(q, j) for q, j in zip(ref["rows"][ref["qrow"]].tolist(), ref["pairs"].tolist())}
    bwd = {(j, q) for q, j in zip(back["rows"][back["qrow"]].tolist(), back["pairs"].tolist())}
    ok_q, ok_s = set(ref["rows"][~ref["crowded"]].tolist()), set(back["rows"][~back["crowded"]].tolist())
    assert {p for p in fwd if p[1] in ok_s} == {p for p in bwd if p[0] in ok_q}


def test_edge_states_one_cell_no_sources_no_queries_everybody_crowded(host_exe):
    rng = np.random.default_rng(9)
    one = ((1, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    pos_q, pos_s = rng.uniform(0, 1, (50, 3)).astype(F32), rng.uniform(0, 1, (30, 3)).astype(F32)
    aq, as_ = rng.permutation(50), rng.permutation(30)
    cases = []
    ref = np_pairs_from(pos_q, aq, pos_s, as_, one, 1.0, 30)               # a 1 x 1 x 1 grid: every source is a candidate of every query
    assert (ref["cand"] == 30).all() and not ref["crowded"].any() and 0 < int(ref["T"][-1]) < 50 * 30
    cases.append((pos_q, aq, pos_s, as_, one, 1.0, 30, ref))
    ref = np_pairs_from(pos_q, aq, pos_s, as_, one, 1.0, 29)               # the limit one below their number: everybody is crowded
    assert ref["crowded"].all() and int(ref["T"][-1]) == 0 and pairs_from_buffers(ref, 50, 9)[5].tolist() == [50, 50, 0, 50, 0, 0, 0, 30]
    cases.append((pos_q, aq, pos_s, as_, one, 1.0, 29, ref))
    grid = ((3, 2, 2), (0.0, 0.0, 0.0), (3.0, 2.0, 2.0))
    none = np.zeros(0, np.int64)
    ref = np_pairs_from(pos_q, aq, pos_s, none, grid, 0.3, 100)            # no sources: every run is empty, the rows are fx's all the same
    assert len(ref["rows"]) == 50 and int(ref["T"][-1]) == 0 and ref["s_inside"] == 0
    cases.append((pos_q, aq, pos_s, none, grid, 0.3, 100, ref))
    ref = np_pairs_from(pos_q, none, pos_s, as_, grid, 0.3, 100)           # no queries: no rows
    assert len(ref["rows"]) == 0 and ref["T"].tolist() == [0] and pairs_from_buffers(ref, 50, 9)[5].tolist() == [0, 0, 0, 0, 0, 0, 0, 30]
    cases.append((pos_q, none, pos_s, as_, grid, 0.3, 100, ref))
    ref = np_pairs_from(pos_q, none, pos_s, none, grid, 0.3, 100)
    cases.append((pos_q, none, pos_s, none, grid, 0.3, 100, ref))
    lines, asked = [], []
    for pq, a, ps, b, g, radius, limit, ref in cases:
        for pc in (0, 7, int(ref["T"][-1]), int(ref["T"][-1]) + 3):
            lines.append(_run_line(pq, a, ps, b, g, radius, limit, pc, True))
            asked.append((ref, pc))
    for (ref, pc), out in zip(asked, _ask(host_exe, lines)):
        _assert_run(out, ref, 50, pc, True)
