"""The neighbour list (hnb_effect_pairs, include/hanabi_amd_pairs.h) without a GPU: header, ctypes mirror and INTEGRATION.md agree on the structure and
the prototype, and the call fails loudly; the plain C++ of csrc/hnb_pairs.h - the two per-row bodies both kernels call, the clamp, the check of a
description, the scratch layout and the launch plan - compiled as a stand-alone host program under the address and undefined-behaviour sanitizers
gives what the restatements in numpy / Python give, bit for bit; the three kernels live in a code object of their own with no scratch and no spills.
The restatement here (np_pairs, pairs_buffers) is what tests/test_gpu_pairs.py expects."""
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
from test_neighbours_abi import np_d2

PAIRS_KERNELS = ["k_pairs_count", "k_pairs_scan", "k_pairs_fill"]
F32, U32 = np.float32, np.uint32
NO_ROW = 0xFFFFFFFF


# ---- the semantics, restated in numpy ---------------------------------------------------------------------------------------------------------------
def np_pairs(pos, alive_order, grid, radius, candidate_limit, half=False):
    """pos: [slots, 3] binary32; alive_order: the alive slots in list order; grid: (dims, origin, inv_cell). Brute force: the rows are the inside
    particles in the stable order by cell; for the rows of one (y, z) strip of cells every row of the up to nine strips around it is tested for the
    cell restriction and the radius (which only leaves out pairs the cell restriction refuses). -> dict: rows [n_inside] slots; cells, cand
    [n_inside]; crowded [n_inside] bool; counts [n_inside] run lengths; T [n_inside + 1] uint64 exclusive sums; pairs [total] neighbour slots and
    d2 [total] binary32 in CSR order; qrow, jrow [total] the pair's query and neighbour rows; offsets: the set of cell offsets over all pairs;
    n_alive, n_outside"""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    alive = np.asarray(alive_order, np.int64)
    dims, origin, inv_cell = grid
    dims = [int(d) for d in dims]
    n_cells = dims[0] * dims[1] * dims[2]
    cells = np_cells(pos[alive], dims, origin, inv_cell).astype(np.int64) if len(alive) else np.zeros(0, np.int64)
    order = np.argsort(cells, kind="stable")
    n_inside = int((cells != n_cells).sum())
    rows = alive[order][:n_inside]
    c = cells[order][:n_inside]
    cx, cy, cz = c % dims[0], (c // dims[0]) % dims[1], c // (dims[0] * dims[1])
    box = np.zeros((dims[2] + 2, dims[1] + 2, dims[0] + 2), np.int64)
    np.add.at(box, (cz + 1, cy + 1, cx + 1), 1)
    tot = np.zeros((dims[2], dims[1], dims[0]), np.int64)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                tot += box[dz: dz + dims[2], dy: dy + dims[1], dx: dx + dims[0]]
    cand = tot[cz, cy, cx]
    crowded = cand > int(candidate_limit)
    r2 = F32(radius) * F32(radius)
    p = pos[rows]
    strip = cz * dims[1] + cy                                              # ascending with the row
    first = np.searchsorted(strip, np.arange(dims[1] * dims[2] + 1))       # the rows of strip s: [first[s], first[s + 1])
    Q, J, D = [], [], []
    for s in np.unique(strip):
        y, z = int(s % dims[1]), int(s // dims[1])
        around = [np.arange(first[zz * dims[1] + yy], first[zz * dims[1] + yy + 1]) for zz in range(max(z - 1, 0), min(z + 2, dims[2])) for yy in range(max(y - 1, 0), min(y + 2, dims[1]))]
        j = np.concatenate(around)                                         # ascending rows
        q_all = np.arange(first[s], first[s + 1])
        q_all = q_all[~crowded[q_all]]
        for b in range(0, len(q_all), 512):
            q = q_all[b: b + 512]
            near = (np.abs(cx[q, None] - cx[None, j]) <= 1) & (q[:, None] != j[None, :])
            if half:
                near &= rows[None, j] > rows[q, None]
            qi, ji = np.nonzero(near)                                      # row-major: by query, then by ascending neighbour row
            qi, ji = q[qi], j[ji]
            d2 = np_d2(p[qi], p[ji])
            nb = d2 < r2
            Q.append(qi[nb]); J.append(ji[nb]); D.append(d2[nb])
    qrow = np.concatenate(Q) if Q else np.zeros(0, np.int64)
    jrow = np.concatenate(J) if J else np.zeros(0, np.int64)
    d2 = np.concatenate(D).astype(F32) if D else np.zeros(0, F32)
    assert (np.diff(qrow) >= 0).all() and ((np.diff(jrow) > 0) | (np.diff(qrow) > 0)).all(), "CSR order: by row, then by ascending neighbour row"
    counts = np.bincount(qrow, minlength=n_inside).astype(np.int64)
    T = np.zeros(n_inside + 1, np.uint64)
    T[1:] = np.cumsum(counts).astype(np.uint64)
    offsets = set(zip((cx[jrow] - cx[qrow]).tolist(), (cy[jrow] - cy[qrow]).tolist(), (cz[jrow] - cz[qrow]).tolist()))
    return dict(rows=rows, cells=c, cand=cand, crowded=crowded, counts=counts, T=T, pairs=rows[jrow].astype(np.int64), d2=d2, qrow=qrow, jrow=jrow, offsets=offsets,
                n_alive=len(alive), n_outside=len(alive) - n_inside)


def pairs_buffers(ref, capacity, pair_capacity):
    """what a call leaves behind -> (out_rows [capacity], out_start [capacity + 1], written, out_pairs[:written], out_d2[:written] as words, stats [8])"""
    n = len(ref["rows"])
    total = int(ref["T"][n])
    out_rows = np.full(capacity, NO_ROW, U32)
    out_rows[:n] = ref["rows"]
    start = np.empty(capacity + 1, np.uint64)
    start[: n + 1] = np.minimum(ref["T"], np.uint64(pair_capacity))
    start[n + 1:] = start[n]
    written = min(total, pair_capacity)
    stats = np.array([ref["n_alive"], n, ref["n_outside"], int(ref["crowded"].sum()), total & 0xFFFFFFFF, total >> 32, written, 0], np.uint64).astype(U32)
    return out_rows, start.astype(U32), written, ref["pairs"][:written].astype(U32), ref["d2"][:written].view(U32), stats


def pairs_plan(cap, n_cells):
    """pairs_launch_plan restated -> ([(kernel, grid x)] of the sort's part, index of the launch behind the memset or None, pack, count, scan, fill grids)"""
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
    L.append(("bin_starts", -(-(n_cells + 2) // 256)))
    G = max(1, -(-cap // 256))
    return L, memset, G, G, 1, -(-(cap + 1) // 256)


def pairs_layout(cap, n_cells):
    """pairs_scratch_layout restated -> (tiles, snap_off, snap_bytes, count_off, count_bytes, tile_off, tile_bytes, cells_off, cells_bytes, total)"""
    up = lambda x: (x + 255) & ~255
    sl = sort_layout(1, cap, INSTANCE)
    tiles = max(1, -(-cap // 256))
    snap_off = up(sl[10])
    count_off = up(snap_off + sl[2] * 16)
    tile_off = up(count_off + sl[2] * 4)
    cells_off = up(tile_off + (tiles + 1) * 8)
    return (tiles, snap_off, sl[2] * 16, count_off, sl[2] * 4, tile_off, (tiles + 1) * 8, cells_off, (n_cells + 2) * 4, up(cells_off + (n_cells + 2) * 4))


LINE = np.array([(0.25, 0.5, 0.5), (0.75, 0.5, 0.5), (1.5, 0.5, 0.5), (3.5, 0.5, 0.5), (5.0, 0.5, 0.5), (0.5, 0.5, 0.5)], F32)
LINE_GRID = ((4, 1, 1), (0, 0, 0), (1, 1, 1))


def test_the_restatement_itself_on_cases_worked_by_hand():
    # five particles on a line in a 4 x 1 x 1 grid of unit cells, radius 1: x = 0.25, 0.75, 1.5, 3.5, and one at 5 (outside); slot 5 is dead.
    # list order 3, 1, 0, 2, 4 -> rows by cell, list order within a cell: cell 0: slots 1, 0; cell 1: slot 2; cell 3: slot 3
    r = np_pairs(LINE, [3, 1, 0, 2, 4], LINE_GRID, 1.0, 100)
    assert r["rows"].tolist() == [1, 0, 2, 3] and r["cand"].tolist() == [3, 3, 3, 1] and (r["n_alive"], r["n_outside"]) == (5, 1)
    assert r["counts"].tolist() == [2, 1, 1, 0] and r["T"].tolist() == [0, 2, 3, 4, 4]      # 0.25 and 1.5 are 1.25 apart: no pair
    assert r["pairs"].tolist() == [0, 2, 1, 1] and r["d2"].tolist() == [0.25, 0.5625, 0.25, 0.5625]       # slot 1's run: rows 1 (slot 0), 2 (slot 2) - ascending ROWS, not slots
    assert r["offsets"] == {(0, 0, 0), (1, 0, 0), (-1, 0, 0)}
    rows, start, written, pairs, d2, stats = pairs_buffers(r, 6, 100)
    assert rows.tolist() == [1, 0, 2, 3, NO_ROW, NO_ROW] and start.tolist() == [0, 2, 3, 4, 4, 4, 4] and stats.tolist() == [5, 4, 1, 0, 4, 0, 4, 0]
    rows, start, written, pairs, d2, stats = pairs_buffers(r, 6, 3)        # truncated: a prefix, the table clamped
    assert start.tolist() == [0, 2, 3, 3, 3, 3, 3] and pairs.tolist() == [0, 2, 1] and stats.tolist() == [5, 4, 1, 0, 4, 0, 3, 0]
    h = np_pairs(LINE, [3, 1, 0, 2, 4], LINE_GRID, 1.0, 100, half=True)     # each pair once, under the lower slot: {0, 1} under 0, {1, 2} under 1
    assert h["counts"].tolist() == [1, 1, 0, 0] and h["pairs"].tolist() == [2, 1]
    # a coincident pair: two slots on one point are neighbours of each other at d2 = 0; the particle itself is not
    pos = np.array([(0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)], F32)
    r = np_pairs(pos, [2, 0], ((1, 1, 1), (0, 0, 0), (1, 1, 1)), 0.5, 100)
    assert r["rows"].tolist() == [2, 0] and r["pairs"].tolist() == [0, 2] and r["d2"].tolist() == [0.0, 0.0] and r["offsets"] == {(0, 0, 0)}
    # a crowded cell: three candidates around cells 0 and 1 with a limit of 2 - they list nothing, and nobody is left who could list them
    r = np_pairs(LINE, [3, 1, 0, 2, 4], LINE_GRID, 1.0, 2)
    assert r["crowded"].tolist() == [True, True, True, False] and r["counts"].tolist() == [0, 0, 0, 0] and pairs_buffers(r, 6, 9)[5].tolist() == [5, 4, 1, 3, 0, 0, 0, 0]
    # ... and one where a crowded query still appears in another's run: 0.3, 0.6 in cell 0 and 1.2 in cell 1 | 2.1 in cell 2 sees 1.2 only
    pos = np.array([(0.3, 0.5, 0.5), (0.6, 0.5, 0.5), (1.2, 0.5, 0.5), (2.1, 0.5, 0.5)], F32)
    r = np_pairs(pos, [0, 1, 2, 3], LINE_GRID, 1.0, 2)
    assert r["cand"].tolist() == [3, 3, 4, 2] and r["crowded"].tolist() == [True, True, True, False] and r["pairs"].tolist() == [2] and r["counts"].tolist() == [0, 0, 0, 1]
    h = np_pairs(pos, [0, 1, 2, 3], LINE_GRID, 1.0, 2, half=True)          # the half list loses {2, 3}: its lower slot is crowded
    assert h["pairs"].tolist() == [] and h["crowded"].sum() == 3
    # the restatement speaks the library's own words: the sentinel of the binding, and the kernels and the tile of hnb_pairs.h
    assert NO_ROW == runtime.PAIRS_NO_ROW and runtime.PAIRS_HALF == 1
    text = open(os.path.join(CSRC, "hnb_pairs.h")).read()
    assert all(f'"{k}"' in text for k in PAIRS_KERNELS) and "constexpr uint32_t kPairsBlock = 256;" in text
    assert pairs_plan(4096, 62)[:2] == ([("bin_tile", 1), ("bin_starts", 1)], None) and pairs_plan(4096, 62)[2:] == (16, 16, 1, 17) and pairs_plan(4097, 510)[2:] == (17, 17, 1, 17)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------------
MEMBERS = ["struct_size", "flags", "dims", "candidate_limit", "origin", "inv_cell", "radius", "pair_capacity", "out_rows", "out_start", "out_pairs", "out_d2", "out_stats"]


def test_ctypes_mirror_header_and_integration_agree_on_the_struct_and_the_prototype(tmp_path):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd_pairs.h"
    int main(void) {
        int (*fe)(HnbEffect*, const HnbPairsDesc*) = hnb_effect_pairs;
        printf("%zu", sizeof(HnbPairsDesc));
    ''' + "\n".join(f'        printf(" %zu", offsetof(HnbPairsDesc, {m}));' for m in MEMBERS) + r'''
        printf(" %u %u\n", HNB_PAIRS_HALF, HNB_PAIRS_NO_ROW);
        return fe == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()]
    D = runtime.PairsDesc
    assert got == [96, 0, 4, 8, 20, 24, 36, 48, 52, 56, 64, 72, 80, 88, 1, 0xFFFFFFFF]
    assert [C.sizeof(D)] + [getattr(D, m).offset for m in MEMBERS] == got[:14]
    assert (runtime.PAIRS_HALF, runtime.PAIRS_NO_ROW) == tuple(got[14:])
    d = runtime.pairs_desc((4, 5, 6), (1, 2, 3), (0.5, 0.25, 2), 0.5, 0x1000, 0x2000, 0x3000, 77, 0x4000, 0x5000, 99, True)
    assert (d.struct_size, d.flags, list(d.dims), d.candidate_limit, list(d.origin), list(d.inv_cell), d.radius, d.pair_capacity, d.out_rows, d.out_start, d.out_pairs, d.out_d2,
            d.out_stats) == (96, 1, [4, 5, 6], 99, [1, 2, 3], [0.5, 0.25, 2], 0.5, 77, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000)
    d = runtime.pairs_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 1.0, 0x1000, 0x2000)
    assert (d.flags, d.candidate_limit, d.pair_capacity, d.out_pairs, d.out_d2, d.out_stats) == (0, 4096, 0, None, None, None)
    lib = runtime.load_library()
    assert runtime.ABI_PAIRS_SYMBOLS == ["hnb_effect_pairs"]
    full = open(os.path.join(ROOT, "include", "hanabi_amd_pairs.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(lib, "hnb_effect_pairs") and lib.hnb_effect_pairs.argtypes == [C.c_void_p, C.POINTER(runtime.PairsDesc)]
    m = re.search(r"int\s+hnb_effect_pairs\s*\(([^)]*)\)\s*;", header)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["HnbEffect* fx", "const HnbPairsDesc* desc"]
    m = re.search(r"\bfn hnb_effect_pairs\(([^)]*)\) -> c_int;", txt)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["fx: *mut HnbEffect", "desc: *const HnbPairsDesc"]
    assert "pub unsafe fn effect_pairs(" in txt and "pub mod pairs {" in txt
    assert list(inspect.signature(runtime.Effect.pairs).parameters) == ["self", "dims", "origin", "inv_cell", "radius", "rows_ptr", "start_ptr", "pairs_ptr", "pair_capacity", "d2_ptr",
                                                                        "stats_ptr", "candidate_limit", "half"]
    assert not hasattr(runtime.Program, "pairs")                           # (no program form: out of scope, the header says so)
    # every header declares exactly its own symbols: hanabi_amd.h and its 61 are as they were, and the companion lists do not overlap
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", header)) == set(runtime.ABI_PAIRS_SYMBOLS)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", main)) == set(runtime.ABI_SYMBOLS) and len(runtime.ABI_SYMBOLS) == 61
    nb = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd_neighbours.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", nb)) == set(runtime.ABI_NEIGHBOUR_SYMBOLS)
    for other in (runtime.ABI_SYMBOLS, runtime.ABI_BINNED_SYMBOLS, runtime.ABI_IMPORT_SYMBOLS, runtime.ABI_DEPOSIT_SYMBOLS, runtime.ABI_SAMPLE_SYMBOLS, runtime.ABI_SPLAT_SYMBOLS,
                  runtime.ABI_SAMPLE_PROGRAM_SYMBOLS, runtime.ABI_NEIGHBOUR_SYMBOLS):
        assert not set(runtime.ABI_PAIRS_SYMBOLS) & set(other)
    for inc in ('#include "hanabi_amd.h"', '#include "hanabi_amd_binned.h"', '#include "hanabi_amd_neighbours.h"'):
        assert inc in full
    bound = set(re.findall(r"pub fn (hnb_[a-z0-9_]+)\(", txt))
    assert not set(runtime.ABI_PAIRS_SYMBOLS) & bound                      # (the `pub fn` set mirrors hanabi_amd.h and the host header: the call sits in a module of its own)
    rust = [" ".join(line.split("//")[0].split()).rstrip(",") for line in
            re.search(r"#\[repr\(C\)\]\s*pub struct HnbPairsDesc \{(.*?)\}", txt, flags=re.S).group(1).splitlines() if line.split("//")[0].strip()]
    assert rust == ["pub struct_size: u32", "pub flags: u32", "pub dims: [u32; 3]", "pub candidate_limit: u32", "pub origin: [f32; 3]", "pub inv_cell: [f32; 3]", "pub radius: f32",
                    "pub pair_capacity: u32", "pub out_rows: *mut u32", "pub out_start: *mut u32", "pub out_pairs: *mut u32", "pub out_d2: *mut f32", "pub out_stats: *mut u32"]
    assert "hnb_effect_device_view" in txt[txt.index("### Neighbour pairs"):] and "out_start[r + 1]" in txt[txt.index("### Neighbour pairs"):]       # the consumer kernel that walks the CSR
    for word in ("OUTSIDE BIN", "d2 = s + zz", "CROWDED", "symmetric bit for bit", "ascending sorted-row order", "already ascending in rows", "complete iff stats[3] == 0",
                 "j is in i's run iff i is in j's", "min(T[r], pair_capacity)", "keep every bit", "count only", "Out of scope: a program form", "pairs across effects", "ELL (fixed-stride) output",
                 "row indices instead of slots", "a per-query cap other than the", "0xFFFFFF00 slots", "radius * inv_cell[c] <= 1", "HNB_PAIRS_NO_ROW", "that overlap"):
        assert word in full, word


def test_call_fails_loudly_on_null_arguments_and_without_a_device():
    """Up to the device check: the NULL refusals come before anything is dereferenced, loaded or enqueued. The refusals of a description's members
    need an effect, and an effect a device: the stand-alone program below holds them, and tests/test_gpu_pairs.py on a live effect."""
    lib = runtime.load_library()
    d = runtime.pairs_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 1.0, 0x1000, 0x2000)
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for args in ((None, C.byref(d)), (fake, None), (None, None)):
        assert lib.hnb_effect_pairs(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no effect to list, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the code object --------------------------------------------------------------------------------------------------------------------------------
def test_code_object_is_built_carried_and_has_its_three_kernels_without_scratch_or_spills():
    co = hb.pairs_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_pairs.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(PAIRS_KERNELS), sorted(rows)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert design.index("## Neighbours") < design.index("## Neighbour pairs") < design.index("## Measurement (row d)")
    section = design[design.index("## Neighbour pairs"): design.index("## Measurement (row d)")]
    for name, r in rows.items():
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["kernarg_segment_size"] == 168, (name, r)                # one PairsArgs by value
        row = f"| `{name}` | {r['vgpr_count']} | {r['sgpr_count']} | {r['group_segment_fixed_size']} |"
        assert row in section, f"DESIGN.md \"Neighbour pairs\" resource table: {row}"      # (a recorded value, not a preset bound)
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_pairs_code)
    for h in ("hnb_pairs.h", "hnb_neighbours.h", "hnb_bin_cell.h", "hnb_export_bin.h"):
        assert f'"{h}"' in inspect.getsource(hb.build_pairs_code)
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_pairs.hip")).read()
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_pairs.h")).read()
    assert hb.PAIRS_CODE_OBJECTS == (hb.build_pairs_code,) and hb.NEIGHBOURS_CODE_OBJECTS == (hb.build_neighbours_code,)
    assert "PAIRS_CODE_OBJECTS" in inspect.getsource(hb.build_runtime) and "hanabi_amd_pairs.h" in inspect.getsource(hb.build_runtime)
    assert "hanabi_amd_pairs.h" in inspect.getsource(hb._build_code_object)
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "bevy_hanabi_amd/csrc/hnb_pairs_code.inc" in ignored and "*.hsaco" in ignored
    for other in (hb.neighbours_code_path(), hb.export_bin_code_path(), hb.sample_code_path(), hb.deposit_code_path(), hb.export_sort_code_path(), hb.export_filter_code_path()):
        assert not set(_rows(other)) & set(PAIRS_KERNELS)
    assert sorted(_rows(hb.neighbours_code_path())) == ["k_neighbours_gather", "k_neighbours_pack"]     # the unit whose snapshot kernel the call borrows is as it was


# ---- csrc/hnb_pairs.h as a stand-alone host program under the sanitizers ----------------------------------------------------------------------------
ERRORS = ["Ok", "ErrStructSize", "ErrFlags", "ErrDims", "ErrOrigin", "ErrInvCell", "ErrRadius", "ErrCoverage", "ErrRadiusSquared", "ErrCandidateLimit", "ErrNoPosition", "ErrCapacity",
          "ErrNullRows", "ErrNullStart", "ErrNullPairs", "ErrAlign", "ErrStats", "ErrOverlap"]
E = {n: i for i, n in enumerate(ERRORS)}
# what the check is given: (attr, ncomp, is_f32); layout 1 has no POSITION
LAYOUT = [(A.POSITION.id, 3, 1), (A.VELOCITY.id, 3, 1), (A.AGE.id, 1, 1), (A.LIFETIME.id, 1, 1)]
SENT = 0xDEADBEEF

HOST_SRC = r"""
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>
#include "hnb_pairs.h"
using namespace hnb;
""" + "\n".join(f"static_assert(kPairs{n} == {i}, \"PairsDescError\");" for i, n in enumerate(ERRORS)) + r"""
static_assert(kPairsDescErrorCount == """ + str(len(ERRORS)) + r""", "PairsDescError");
static_assert(sizeof(HnbPairsDesc) == 96 && sizeof(PairsArgs) == 168 && kPairsKCount == 0 && kPairsKScan == 1 && kPairsKFill == 2 && kPairsKernelCount == 3, "hnb_pairs.h");
static_assert(kPairsBlock == 256 && kPairsStatsWords == 8 && sizeof(PairsSnap) == 16 && sizeof(NeighbourArgs) == 248, "hnb_pairs.h");
static const NeighbourLayoutAttr kLayout[] = {""" + ", ".join("{%d, %d, %d}" % l for l in LAYOUT) + r"""};
static float f_of(unsigned b) { float f; std::memcpy(&f, &b, 4); return f; }
static unsigned b_of(float f) { unsigned b; std::memcpy(&b, &f, 4); return b; }
static const char* launch_name(uint32_t k) {
    return k == kExportBinKernelBase + kBinKTile ? "bin_tile" : k == kExportBinKernelBase + kBinKKeys ? "bin_keys" : k == kExportBinKernelBase + kBinKStarts ? "bin_starts" :
           k == kExpSortHist ? "sort_hist" : k == kExpSortScatter ? "sort_scatter" : "?";
}
int main() {
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "names")) {
            for (uint32_t i = 0; i < kPairsKernelCount; ++i) std::printf("%u:%s ", kPairsKernelNames[i].kernel, kPairsKernelNames[i].name);
            std::printf("\n");
        } else if (!std::strcmp(what, "texts")) {
            for (uint32_t e = 0; e < kPairsDescErrorCount; ++e) std::printf("%s|", pairs_error_text(e));
            std::printf("\n");
        } else if (!std::strcmp(what, "clamp")) {
            unsigned long long T; unsigned pc;
            if (std::scanf("%llu %u", &T, &pc) != 2) return 1;
            std::printf("%u\n", pairs_clamp((uint64_t)T, pc));
        } else if (!std::strcmp(what, "plan")) {
            unsigned cap, n_cells;
            if (std::scanf("%u %u", &cap, &n_cells) != 2) return 1;
            const PairsPlan pl = pairs_launch_plan(cap, n_cells);
            if (pl.sort.n > kExportPlanMax) return 5;
            std::printf("%d %u %u %u %u %llu", pl.sort.memset_before == kExportNoMemset ? -1 : (int)pl.sort.memset_before, pl.pack_grid, pl.count_grid, pl.scan_grid, pl.fill_grid,
                        (unsigned long long)pl.clear_stats_bytes);
            for (uint32_t i = 0; i < pl.sort.n; ++i) {
                const ExportLaunch& l = pl.sort.launch[i];
                if (l.grid_y != 1u || l.args != (l.kernel >= kExportBinKernelBase ? kExportArgsBin : kExportArgsSortPass)) return 5;
                std::printf(" %s:%u:%u", launch_name(l.kernel), l.grid_x, l.pass);
            }
            std::printf("\n");
        } else if (!std::strcmp(what, "layout")) {
            unsigned cap, n_cells;
            if (std::scanf("%u %u", &cap, &n_cells) != 2) return 1;
            const PairsScratch l = pairs_scratch_layout(cap, n_cells);
            std::printf("%u %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %u %u\n", l.tiles, (unsigned long long)l.snap_off, (unsigned long long)l.snap_bytes, (unsigned long long)l.count_off,
                        (unsigned long long)l.count_bytes, (unsigned long long)l.tile_off, (unsigned long long)l.tile_bytes, (unsigned long long)l.cells_off,
                        (unsigned long long)l.cells_bytes, (unsigned long long)l.total, (unsigned long long)l.sort.total, l.sort.pitch, l.sort.rows);
        } else if (!std::strcmp(what, "run")) {   // a whole state through the header: cells, a stable sort, the table, the count of every row, a host scan, the fill
            BinGrid g = {};
            unsigned ob[3], ib[3], rb, limit, half, pc, want_d2, n;
            if (std::scanf("%u %u %u %x %x %x %x %x %x %x %u %u %u %u %u", &g.dims[0], &g.dims[1], &g.dims[2], &ob[0], &ob[1], &ob[2], &ib[0], &ib[1], &ib[2], &rb, &limit, &half, &pc,
                           &want_d2, &n) != 15) return 1;
            for (int c = 0; c < 3; ++c) { g.origin[c] = f_of(ob[c]); g.inv_cell[c] = f_of(ib[c]); }
            g.n_cells = bin_cell_count(g.dims);
            std::vector<uint32_t> slot(n), pos(3 * (size_t)n);              // in list order
            for (size_t i = 0; i < n; ++i)
                if (std::scanf("%u %x %x %x", &slot[i], &pos[3 * i], &pos[3 * i + 1], &pos[3 * i + 2]) != 4) return 1;
            const float radius = f_of(rb), r2 = radius * radius;
            std::vector<uint32_t> cell(n), order(n);
            for (size_t i = 0; i < n; ++i) cell[i] = bin_cell_of(g, f_of(pos[3 * i]), f_of(pos[3 * i + 1]), f_of(pos[3 * i + 2]));
            std::iota(order.begin(), order.end(), 0u);
            std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cell[x] < cell[y]; });
            std::vector<uint32_t> start(export_bin_entries(g.n_cells));     // exactly n_cells + 2 entries on the heap: a read past them is an error the sanitizer reports
            for (uint32_t c = 0; c < start.size(); ++c)
                start[c] = (uint32_t)(std::lower_bound(order.begin(), order.end(), c, [&](uint32_t row, uint32_t key) { return cell[row] < key; }) - order.begin());
            const uint32_t n_inside = start[g.n_cells];
            std::vector<PairsSnap> snap(n_inside);                          // exactly the inside rows: no walk may read an outside one
            for (uint32_t r = 0; r < n_inside; ++r) snap[r] = {pos[3 * order[r]], pos[3 * order[r] + 1], pos[3 * order[r] + 2], slot[order[r]]};
            std::vector<uint32_t> count(n_inside), crowded(n_inside);
            std::vector<uint64_t> T(n_inside + 1u, 0u);
            for (uint32_t r = 0; r < n_inside; ++r) {
                const PairsRowCount rc = pairs_row_count(snap.data(), start.data(), g.dims, r, cell[order[r]], limit, r2, half != 0);
                count[r] = rc.count; crowded[r] = rc.crowded;
                if (rc.crowded && rc.count) return 6;
                T[r + 1u] = T[r] + rc.count;
            }
            std::vector<uint32_t> out_pairs(pc, 0xDEADBEEFu);               // exactly pair_capacity entries: a store past them is an error the sanitizer reports
            std::vector<float> out_d2(want_d2 ? pc : 0u, f_of(0xDEADBEEFu));
            for (uint32_t r = 0; r < n_inside; ++r) {
                if (crowded[r]) continue;
                const uint32_t k = pairs_row_fill(snap.data(), start.data(), g.dims, r, cell[order[r]], r2, half != 0, T[r], pc, pc ? out_pairs.data() : nullptr,
                                                  want_d2 && pc ? out_d2.data() : nullptr);
                if (k != count[r]) return 7;
            }
            std::printf("%u %llu |", n_inside, (unsigned long long)T[n_inside]);
            for (uint32_t r = 0; r < n_inside; ++r) std::printf(" %u", snap[r].slot);
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
            unsigned long long ptr[5]; unsigned layout_first, cap, ob[3], ib[3], rb;
            if (std::scanf("%u %u %u %u %u %u %u %u %x %x %x %x %x %x %x %u %llx %llx %llx %llx %llx", &layout_first, &cap, &d.struct_size, &d.flags, &d.dims[0], &d.dims[1], &d.dims[2],
                           &d.candidate_limit, &ob[0], &ob[1], &ob[2], &ib[0], &ib[1], &ib[2], &rb, &d.pair_capacity, &ptr[0], &ptr[1], &ptr[2], &ptr[3], &ptr[4]) != 21) return 1;
            std::memcpy(d.origin, ob, 12); std::memcpy(d.inv_cell, ib, 12); d.radius = f_of(rb);
            d.out_rows = (uint32_t*)(uintptr_t)ptr[0]; d.out_start = (uint32_t*)(uintptr_t)ptr[1]; d.out_pairs = (uint32_t*)(uintptr_t)ptr[2];
            d.out_d2 = (float*)(uintptr_t)ptr[3]; d.out_stats = (uint32_t*)(uintptr_t)ptr[4];
            if (layout_first > 1) return 1;
            const PairsCheck c = pairs_check_desc(d, kLayout + layout_first, (uint32_t)(sizeof kLayout / sizeof *kLayout) - layout_first, cap);
            if (c.error >= kPairsDescErrorCount || !pairs_error_text(c.error)[1]) return 3;
            std::printf("%u %u %u %u %x\n", c.error, c.index, c.n_cells, c.position_index, b_of(c.r2));
        } else return 4;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """g++ alone, with the address and undefined-behaviour sanitizers and no contraction: the header is plain C++ on the host. The program has its
    own main and is run directly."""
    tmp = tmp_path_factory.mktemp("pairs_host")
    (tmp / "pairs.cpp").write_text(HOST_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), str(tmp / "pairs.cpp"), "-o", str(tmp / "pairs")])
    return str(tmp / "pairs")


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()      # (a sanitizer report ends the program with an error)
    assert len(out) == len(lines)
    return out


def _f32(x):
    return int(np.array([x], F32).view(U32)[0])


def _desc_line(layout_first=0, cap=10_000, struct_size=96, flags=0, dims=(4, 4, 4), limit=4096, origin=(0.0, 0.0, 0.0), inv_cell=(1.0, 1.0, 1.0), radius=0.75, pc=5000,
               rows=0x100000, start=0x200000, pairs=0x300000, d2=0x400000, stats=0x500000):
    return ("desc %d %d %d %d %d %d %d %d " % (layout_first, cap, struct_size, flags, *dims, limit) + " ".join("%x" % _f32(x) for x in tuple(origin) + tuple(inv_cell) + (radius,))
            + " %d %x %x %x %x %x" % (pc, rows, start, pairs, d2, stats))


def test_description_check_refuses_what_the_header_lists_every_error_class_in_its_order(host_exe):
    raw = lambda **kw: _ask(host_exe, [_desc_line(**kw)])[0].split()
    ask = lambda **kw: [int(x) for x in raw(**kw)[:4]]
    hit = []

    def refused(name, index=None, **kw):
        got = ask(**kw)
        assert got[0] == E[name] and (index is None or got[1] == index), (name, kw, got)
        if name not in hit:
            hit.append(name)

    w = raw()
    assert [int(x) for x in w[:4]] == [E["Ok"], 0, 64, 0] and int(w[4], 16) == _f32(F32(0.75) * F32(0.75))
    assert ask(flags=1, radius=1.0, limit=1, stats=0, d2=0)[0] == E["Ok"] and ask(limit=65536, cap=0xFFFFFF00, rows=0x1000_0000_0000, start=0x2000_0000_0000)[0] == E["Ok"]
    assert ask(pc=0, pairs=0, d2=0)[0] == E["Ok"] and ask(pc=0, pairs=0, d2=0x400000)[0] == E["Ok"]    # count only: out_pairs may be NULL
    for size in (0, 92, 100, 200):
        refused("ErrStructSize", struct_size=size)
    for flags in (2, 3, 0x80000000):
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
    refused("ErrNoPosition", layout_first=1)
    for cap in (0xFFFFFF01, 0xFFFFFFFF):
        refused("ErrCapacity", cap=cap, rows=0x1000_0000_0000, start=0x2000_0000_0000)
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
    # any two destination ranges: the later of the two is named. rows [cap], start [cap + 1], pairs / d2 [pc], stats [8] words
    refused("ErrOverlap", 1, start=0x100000)                               # the same address
    refused("ErrOverlap", 1, start=0x100000 + 4 * (cap - 1))               # the last word of out_rows
    assert ask(start=0x100000 + 4 * cap)[0] == E["Ok"]                     # right behind it
    refused("ErrOverlap", 1, start=0x100000 - 4 * cap)                     # out_start's last word, entry `capacity`, is out_rows' first
    assert ask(start=0x100000 - 4 * (cap + 1))[0] == E["Ok"]
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
    texts = _ask(host_exe, ["texts"])[0].split("|")[:-1]
    assert len(texts) == len(ERRORS) and len(set(texts)) == len(texts) and texts[0] == "ok"
    for name, word in (("ErrFlags", "HNB_PAIRS_HALF"), ("ErrDims", "HNB_BIN_MAX_CELLS"), ("ErrCoverage", "radius * inv_cell is above 1"), ("ErrCandidateLimit", "candidate_limit is not 1.."),
                       ("ErrNullRows", "out_rows is NULL"), ("ErrNullStart", "out_start is NULL"), ("ErrNullPairs", "out_pairs is NULL"), ("ErrAlign", "4-byte aligned"),
                       ("ErrStats", "16-byte aligned"), ("ErrOverlap", "overlap"), ("ErrCapacity", "0xFFFFFF00"), ("ErrNoPosition", "POSITION")):
        assert word in texts[E[name]], (name, texts[E[name]])


CAPS = [1, 255, 256, 257, 4096, 4097, 65_536, 65_537, 0xFFFFFF00]


def test_scratch_layout_launch_plan_and_clamp_are_their_restatements(host_exe):
    assert _ask(host_exe, ["names"])[0].split() == [f"{i}:{n}" for i, n in enumerate(PAIRS_KERNELS)]
    for cap in CAPS:
        for n_cells in (1, 512, 68_921, 1 << 24):
            lay, plan = _ask(host_exe, ["layout %d %d" % (cap, n_cells), "plan %d %d" % (cap, n_cells)])
            lay = [int(x) for x in lay.split()]
            want = pairs_layout(cap, n_cells)
            sl = sort_layout(1, cap, INSTANCE)
            assert tuple(lay[:10]) == want and lay[10] == sl[10] and lay[11] == sl[2] and lay[12] == cap, (cap, n_cells, lay, want)
            tiles, snap_off, snap_b, count_off, count_b, tile_off, tile_b, cells_off, cells_b, total = lay[:10]
            assert all(o % 256 == 0 for o in (snap_off, count_off, tile_off, cells_off, total))
            assert lay[10] <= snap_off and snap_off + snap_b <= count_off and count_off + count_b <= tile_off and tile_off + tile_b <= cells_off and cells_off + cells_b <= total
            assert snap_b >= 16 * cap and count_b >= 4 * cap and tile_b == 8 * (tiles + 1) and cells_b == 4 * (n_cells + 2) and (tiles - 1) * 256 < cap <= tiles * 256
            w = plan.split()
            L, memset, pack, count, scan, fill = pairs_plan(cap, n_cells)
            assert [int(x) for x in w[:6]] == [-1 if memset is None else memset, pack, count, scan, fill, 32], (cap, w)
            got = [(x.split(":")[0], int(x.split(":")[1])) for x in w[6:]]
            assert got == L, (cap, n_cells, got, L)
            assert count == tiles and (fill - 1) * 256 < cap + 1 <= fill * 256 and fill <= tiles + 1      # every row and the entry behind them has a lane; a fill workgroup reads tile[t], t <= tiles
    assert int(_ask(host_exe, ["layout %d 64" % (0xFFFFFF00 + 1)])[0].split()[12]) == 0    # one above: no sort fits (sort.rows == 0) ...
    assert int(_ask(host_exe, [_desc_line(cap=0xFFFFFF00 + 1, rows=0x1000_0000_0000, start=0x2000_0000_0000)])[0].split()[0]) == E["ErrCapacity"]        # ... and the check refuses it
    cases = [(0, 0), (5, 0), (0, 7), (6, 7), (7, 7), (8, 7), (1 << 32, 0xFFFFFFFF), ((1 << 32) - 2, 0xFFFFFFFF), (1 << 40, 1), ((1 << 64) - 1, 0xFFFFFFFF)]
    assert [int(x) for x in _ask(host_exe, ["clamp %d %d" % c for c in cases])] == [min(T, pc) for T, pc in cases]


# ---- whole states: the header's row bodies against the brute-force restatement -----------------------------------------------------------------------
def _run_line(pos, alive, grid, radius, limit, half, pc, want_d2):
    dims, origin, inv_cell = grid
    head = "run %d %d %d " % tuple(dims) + " ".join("%x" % _f32(x) for x in tuple(origin) + tuple(inv_cell) + (radius,)) + " %d %d %d %d %d " % (limit, int(half), pc, int(want_d2), len(alive))
    words = np.asarray(pos, F32).view(U32).reshape(-1, 3)
    return head + " ".join("%d %x %x %x" % (s, *words[s]) for s in alive)


def truncations(ref):
    """the capacities of the issue: 0, 1, inside a run, at a run's boundary, total - 1, total, total + 1"""
    total = int(ref["T"][-1])
    long_run = int(np.flatnonzero(ref["counts"] >= 3)[len(np.flatnonzero(ref["counts"] >= 3)) // 2])
    mid, boundary = int(ref["T"][long_run]) + 1, int(ref["T"][long_run])
    assert total > 8 and 1 < boundary < mid < total - 1
    return [0, 1, mid, boundary, total - 1, total, total + 1]


STATES = [((3, 3, 3), 0.3, 400, 4096), ((5, 4, 3), 0.25, 700, 4096), ((1, 1, 1), 1.0, 60, 4096), ((2, 1, 7), 0.14, 300, 110), ((4, 4, 4), 0.25, 300, 60)]


@pytest.mark.parametrize("dims,radius,n,limit", STATES, ids=["x".join(map(str, s[0])) + f"-limit{s[3]}" for s in STATES])
def test_whole_states_through_the_row_bodies_are_the_brute_force_restatement_bit_for_bit(host_exe, dims, radius, n, limit):
    """positions uniform in and a little around the unit cube - part of them outside -, a cluster in one cell (crowding under the small limits),
    coincident pairs, a NaN and an infinite position; a shuffled alive list with dead slots; full and HALF; with and without d2; every truncation"""
    rng = np.random.default_rng(n)
    pos = rng.uniform(-0.05, 1.05, (n, 3)).astype(F32)
    pos[: n // 6] = (F32(0.4) + rng.uniform(0, 0.05, (n // 6, 3))).astype(F32)
    pos[n // 6: n // 6 + 5] = pos[n // 6 + 5: n // 6 + 10]                  # coincident pairs
    pos[-1] = (np.nan, 0.5, 0.5); pos[-2] = (0.5, np.inf, 0.5)
    alive = np.union1d(rng.permutation(n)[: n - n // 10], [n - 1, n - 2])   # a tenth of the slots is dead; the non-finite ones are alive
    alive = alive[rng.permutation(len(alive))]
    grid = (dims, (0.0, 0.0, 0.0), tuple(float(d) for d in dims))
    for half in (False, True):
        ref = np_pairs(pos, alive, grid, radius, limit, half)
        total = int(ref["T"][-1])
        assert ref["n_outside"] >= 2 and total > 0 and (ref["crowded"].any() == (limit < 4096))
        assert limit < 4096 or (ref["d2"] == 0).any(), "a coincident pair is listed, at d2 = 0"
        lines = [_run_line(pos, alive, grid, radius, limit, half, pc, want_d2) for pc in truncations(ref) for want_d2 in ((True, False) if pc in (0, total) else (True,))]
        caps = [(pc, want_d2) for pc in truncations(ref) for want_d2 in ((True, False) if pc in (0, total) else (True,))]
        for (pc, want_d2), out in zip(caps, _ask(host_exe, lines)):
            head, rows, crowded, start, pairs, d2 = [s.split() for s in out.split("|")]
            w_rows, w_start, written, w_pairs, w_d2, stats = pairs_buffers(ref, len(pos), pc)
            n_inside = len(ref["rows"])
            assert [int(x) for x in head] == [n_inside, total] and [int(x) for x in rows] == ref["rows"].tolist() and [int(x) for x in crowded] == ref["crowded"].astype(int).tolist()
            assert [int(x) for x in start] == w_start[: n_inside + 1].tolist(), (pc, half)
            assert [int(x) for x in pairs] == w_pairs.tolist() + [SENT] * (pc - written), (pc, half)       # a prefix in CSR order; entries past it keep every bit
            assert [int(x, 16) for x in d2] == (w_d2.tolist() + [SENT] * (pc - written) if want_d2 else []), (pc, half)
        if not half:                                                        # symmetric among the uncrowded
            unc = ~ref["crowded"][ref["jrow"]]
            fwd = set(zip(ref["qrow"][unc].tolist(), ref["jrow"][unc].tolist()))
            assert fwd == {(j, q) for q, j in fwd}
            full = ref
        else:
            keep = full["pairs"] > full["rows"][full["qrow"]]
            np.testing.assert_array_equal(ref["pairs"], full["pairs"][keep])
            np.testing.assert_array_equal(ref["d2"].view(U32), full["d2"][keep].view(U32))
            if not ref["crowded"].any():
                assert 2 * total == int(full["T"][-1])
    if dims == (3, 3, 3):
        assert len(full["offsets"]) == 27                                  # every one of the 26 directions, and the own cell
