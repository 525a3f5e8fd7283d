"""The neighbour sums (hnb_effect_neighbours, include/hanabi_amd_neighbours.h) without a GPU: header, ctypes mirrors and INTEGRATION.md agree on the
structures and the prototype, and the call fails loudly; the plain C++ of csrc/hnb_neighbours.h - the pair rule, the store, the walk over a
cell_start table, the check of a description, the scratch layout and the launch plan - compiled as a stand-alone host program under the address and
undefined-behaviour sanitizers gives what the restatements in numpy / Python give, bit for bit; the two kernels live in a code object of their own
with no scratch and no spills. The restatements here (np_neighbours, np_store) are what tests/test_gpu_neighbours.py expects."""
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
from test_deposit_abi import np_quantise
from test_export_binned_abi import np_cells
from test_export_filtered_abi import CSRC, INSTANCE, _rows, sort_layout
from test_export_sorted_abi import A, LLVM, ROOT

NEIGHBOUR_KERNELS = ["k_neighbours_pack", "k_neighbours_gather"]
W_ONE, W_U1, W_U2, W_U3 = 0, 1, 2, 3
SET, ADD, DIFF = 0, 1, 1
ONE = 0xFFFFFFFF                                 # HNB_SPLAT_ATTR_ONE
F32, U32 = np.float32, np.uint32


# ---- the semantics, restated in numpy: binary32 arrays, one operation per statement ---------------------------------------------------------------
def np_d2(pi, pj):
    """pi, pj: [..., 3] binary32 -> d2, the header's eight statements"""
    with np.errstate(all="ignore"):
        dx = pj[..., 0] - pi[..., 0]
        dy = pj[..., 1] - pi[..., 1]
        dz = pj[..., 2] - pi[..., 2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        s = xx + yy
        d2 = s + zz
    assert d2.dtype == F32
    return d2


def np_weight(weight, d2, inv_r2):
    """-> W [n] binary32; under W_ONE 1.0 (q and u are not formed)"""
    if weight == W_ONE:
        return np.ones(d2.shape, F32)
    with np.errstate(all="ignore"):
        q = d2 * F32(inv_r2)
        u = F32(1.0) - q
        u2 = u * u
        u3 = u2 * u
    assert u3.dtype == F32
    return (u, u2, u3)[weight - 1]


def np_contribution(vj_bits, vi_bits, diff, weight, W, frac_bits):
    """-> (ok [n] bool, q [n] int64): v = vj or vj - vi; cv = v * W (v itself under W_ONE); the deposit's quantisation"""
    vj, vi = np.asarray(vj_bits, U32).view(F32), np.asarray(vi_bits, U32).view(F32)
    with np.errstate(all="ignore"):
        v = vj - vi if diff else vj
        cv = v if weight == W_ONE else v * W
    assert cv.dtype == F32
    return np_quantise(np.ascontiguousarray(cv).view(U32), frac_bits)


def np_store(op, v, S, frac_bits, scale):
    """v: binary32 stored values, S: int64 sums -> v' = ((float)S * 2^-frac_bits) * scale (SET) or v + that (ADD), each operation rounded"""
    with np.errstate(all="ignore"):
        r = np.asarray(S, np.int64).astype(F32)                            # to nearest, ties to even
        r = r * F32(2.0 ** -int(frac_bits))
        r = r * F32(scale)
        out = np.asarray(v, F32) + r if op == ADD else r
    assert out.dtype == F32
    return out


def one_source(n):
    """the source of a channel of HNB_SPLAT_ATTR_ONE over n slots: 1.0f everywhere"""
    return np.full(n, 0x3F800000, U32)


def np_neighbours(pos, alive_order, src, grid, radius, weight, channels, candidate_limit):
    """pos: [slots, 3] binary32; alive_order: the alive slots; src: per channel the [slots] stored words of its source (one_source for
    HNB_SPLAT_ATTR_ONE); grid: (dims, origin, inv_cell); channels: per channel (src_attr, src_comp, flags, frac_bits, dst_attr, dst_comp, op).
    Brute force over all pairs of inside particles (taken slab by slab of the query's z cell, which only leaves out pairs the cell restriction
    refuses), the cell restriction and the radius tested per pair. -> dict over slots: inside, crowded, gathered [slots] bool; cand, nnb [slots]
    int64 (candidates; neighbours of a gathered particle); S [slots, k] int64 (modulo 2^64); rejected: int; offsets: the set of cell offsets
    (dx, dy, dz) over all neighbour pairs; crowded_nb [slots] int64: neighbours of a gathered particle that are crowded; cells [slots]"""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    slots = np.asarray(alive_order, np.int64)
    dims, origin, inv_cell = grid
    dims = [int(d) for d in dims]
    n_cells, n, K = dims[0] * dims[1] * dims[2], len(pos), len(channels)
    cells_all = np.full(n, n_cells, np.int64)
    cells_all[slots] = np_cells(pos[slots], dims, origin, inv_cell).astype(np.int64)
    out = dict(inside=np.zeros(n, bool), crowded=np.zeros(n, bool), gathered=np.zeros(n, bool), cand=np.zeros(n, np.int64), nnb=np.zeros(n, np.int64),
               S=np.zeros((n, K), np.int64), rejected=0, offsets=set(), crowded_nb=np.zeros(n, np.int64), cells=cells_all)
    ins = slots[cells_all[slots] != n_cells]
    out["inside"][ins] = True
    if not len(ins):
        return out
    c = cells_all[ins]
    cx, cy, cz = c % dims[0], (c // dims[0]) % dims[1], c // (dims[0] * dims[1])
    # candidates: the inside particles of the up to 27 cells around the particle's own
    box = np.zeros((dims[2] + 2, dims[1] + 2, dims[0] + 2), np.int64)
    np.add.at(box, (cz + 1, cy + 1, cx + 1), 1)
    tot = np.zeros((dims[2], dims[1], dims[0]), np.int64)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                tot += box[dz: dz + dims[2], dy: dy + dims[1], dx: dx + dims[0]]
    cand = tot[cz, cy, cx]
    out["cand"][ins] = cand
    crowded = cand > int(candidate_limit)
    out["crowded"][ins] = crowded
    out["gathered"][ins] = ~crowded
    r2 = F32(radius) * F32(radius)
    inv_r2 = F32(1.0) / r2
    p = pos[ins]
    S = np.zeros((len(ins), K), np.uint64)
    nnb = np.zeros(len(ins), np.int64)
    cnb = np.zeros(len(ins), np.int64)
    for z in np.unique(cz):
        Q = np.flatnonzero((cz == z) & ~crowded)
        J = np.flatnonzero(np.abs(cz - z) <= 1)
        for b in range(0, len(Q), 512):
            q = Q[b: b + 512]
            near = (np.abs(cx[q, None] - cx[None, J]) <= 1) & (np.abs(cy[q, None] - cy[None, J]) <= 1) & (q[:, None] != J[None, :])
            qi, ji = np.nonzero(near)
            qi, ji = q[qi], J[ji]
            d2 = np_d2(p[qi], p[ji])
            nb = d2 < r2
            qi, ji, d2 = qi[nb], ji[nb], d2[nb]
            W = np_weight(weight, d2, inv_r2)
            np.add.at(nnb, qi, 1)
            np.add.at(cnb, qi, crowded[ji].astype(np.int64))
            out["offsets"] |= set(zip((cx[ji] - cx[qi]).tolist(), (cy[ji] - cy[qi]).tolist(), (cz[ji] - cz[qi]).tolist()))
            for k, ch in enumerate(channels):
                words = np.asarray(src[k], U32)[ins]
                ok, qq = np_contribution(words[ji], words[qi], bool(ch[2] & DIFF), weight, W, ch[3])
                np.add.at(S[:, k], qi[ok], qq[ok].view(np.uint64))         # unsigned adds wrap: the two's-complement sum modulo 2^64
                out["rejected"] += int((~ok).sum())
    out["S"][ins] = S.view(np.int64)
    out["nnb"][ins] = nnb
    out["crowded_nb"][ins] = cnb
    return out


def neighbour_plan(cap, n_cells):
    """neighbour_launch_plan restated -> ([(kernel, grid x)] of the sort's part, index of the launch behind the memset or None, pack grid, gather grid)"""
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
    return L, memset, G, G


def neighbour_layout(cap, n_channels, n_cells):
    """neighbour_scratch_layout restated -> (snap_off, snap_bytes, src_off, src_bytes, cells_off, cells_bytes, total)"""
    up = lambda x: (x + 255) & ~255
    sl = sort_layout(1, cap, INSTANCE)
    snap_off = up(sl[10])
    src_off = up(snap_off + sl[2] * 16)
    cells_off = up(src_off + sl[2] * 4 * n_channels)
    return (snap_off, sl[2] * 16, src_off, sl[2] * 4 * n_channels, cells_off, (n_cells + 2) * 4, up(cells_off + (n_cells + 2) * 4))


def test_the_restatement_itself_on_cases_worked_by_hand():
    # five particles on a line in a 4 x 1 x 1 grid of unit cells, radius 1: x = 0.25, 0.75, 1.5, 3.5, and one at 5 (outside); slot 5 is dead
    pos = np.array([(0.25, 0.5, 0.5), (0.75, 0.5, 0.5), (1.5, 0.5, 0.5), (3.5, 0.5, 0.5), (5.0, 0.5, 0.5), (0.5, 0.5, 0.5)], F32)
    grid = ((4, 1, 1), (0, 0, 0), (1, 1, 1))
    ch = [(ONE, 0, 0, 0, A.LIFETIME.id, 0, SET), (A.POSITION.id, 0, DIFF, 10, A.VELOCITY.id, 0, ADD)]
    src = [one_source(6), pos[:, 0].copy().view(U32)]
    r = np_neighbours(pos, [3, 1, 0, 2, 4], src, grid, 1.0, W_ONE, ch, 100)
    assert r["inside"].tolist() == [True] * 4 + [False, False] and r["gathered"].tolist() == r["inside"].tolist() and r["cand"].tolist() == [3, 3, 3, 1, 0, 0]
    assert r["S"][:, 0].tolist() == [1, 2, 1, 0, 0, 0] and r["nnb"].tolist() == [1, 2, 1, 0, 0, 0]   # 0.25 and 1.5 are 1.25 apart: no neighbours
    assert r["S"][:, 1].tolist() == [512, 768 - 512, -768, 0, 0, 0]         # (0.5) | (0.75, -0.5) | (-0.75): 0.25 - 1.5 is past the radius
    assert r["offsets"] == {(0, 0, 0), (1, 0, 0), (-1, 0, 0)} and r["rejected"] == 0
    r = np_neighbours(pos, [3, 1, 0, 2, 4], src, grid, 1.0, W_ONE, ch, 2)  # three candidates around cells 0 and 1: crowded, but still sources
    assert r["crowded"].tolist() == [True, True, True, False, False, False] and r["gathered"].tolist() == [False, False, False, True, False, False]
    r = np_neighbours(pos, [3, 1, 0, 2, 4], src, grid, 1.0, W_U2, ch[:1], 100)
    u = F32(1.0) - F32(0.25) * F32(1.0)                                     # 0.25 <-> 0.75: d2 = 0.25
    assert r["S"][0, 0] == 1 and np_quantise(np.array([u * u], F32).view(U32), 0)[1][0] == 1          # 0.5625 rounds to 1 at frac_bits 0
    assert np_store(SET, [F32(7)], [3], 1, -2.0)[0] == F32(-3.0) and np_store(ADD, [F32(7)], [3], 1, -2.0)[0] == F32(4.0)
    assert np_store(SET, [F32(0)], [(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1], 0, 1.0).tolist() == [float(1 << 24), float((1 << 24) + 4), -float(1 << 24)]
    assert neighbour_plan(4096, 62)[:2] == ([("bin_tile", 1), ("bin_starts", 1)], None) and neighbour_plan(4097, 510)[0][-1] == ("bin_starts", 2)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------------
MEMBERS = ["struct_size", "flags", "dims", "n_channels", "origin", "inv_cell", "radius", "scale", "weight", "candidate_limit", "channels", "out_stats"]
CH_MEMBERS = ["src_attr", "src_comp", "flags", "frac_bits", "dst_attr", "dst_comp", "op", "reserved"]


def test_ctypes_mirrors_header_and_integration_agree_on_the_structs_and_the_prototype(tmp_path):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd_neighbours.h"
    int main(void) {
        int (*fe)(HnbEffect*, const HnbNeighbourDesc*) = hnb_effect_neighbours;
        printf("%zu", sizeof(HnbNeighbourDesc));
    ''' + "\n".join(f'        printf(" %zu", offsetof(HnbNeighbourDesc, {m}));' for m in MEMBERS) + r'''
        printf(" %zu", sizeof(HnbNeighbourChannel));
    ''' + "\n".join(f'        printf(" %zu", offsetof(HnbNeighbourChannel, {m}));' for m in CH_MEMBERS) + r'''
        printf(" %u %u %u %u %u %u %u\n", HNB_NEIGHBOUR_MAX_CHANNELS, HNB_NEIGHBOUR_MAX_CANDIDATES, HNB_NEIGHBOUR_W_ONE, HNB_NEIGHBOUR_W_U1, HNB_NEIGHBOUR_W_U2, HNB_NEIGHBOUR_W_U3,
               HNB_NEIGHBOUR_DIFF);
        return fe == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()]
    D, Ch = runtime.NeighbourDesc, runtime.NeighbourChannel
    assert got == [200, 0, 4, 8, 20, 24, 36, 48, 52, 56, 60, 64, 192, 32, 0, 4, 8, 12, 16, 20, 24, 28, 4, 65536, 0, 1, 2, 3, 1]
    assert [C.sizeof(D)] + [getattr(D, m).offset for m in MEMBERS] == got[:13]
    assert [C.sizeof(Ch)] + [getattr(Ch, m).offset for m in CH_MEMBERS] == got[13:22]
    assert (runtime.NEIGHBOUR_MAX_CHANNELS, runtime.NEIGHBOUR_MAX_CANDIDATES, runtime.NEIGHBOUR_W_ONE, runtime.NEIGHBOUR_W_U1, runtime.NEIGHBOUR_W_U2, runtime.NEIGHBOUR_W_U3,
            runtime.NEIGHBOUR_DIFF) == tuple(got[22:])
    d = runtime.neighbour_desc((4, 5, 6), (1, 2, 3), (0.5, 0.25, 2), 0.5, [(ONE, 0, 0, 30, A.LIFETIME.id, 0, SET), (A.VELOCITY.id, 2, DIFF, 12, A.VELOCITY.id, 1, ADD)], W_U3, 77, -0.25, 0x3000)
    assert (d.struct_size, d.flags, list(d.dims), d.n_channels, list(d.origin), list(d.inv_cell), d.radius, d.scale, d.weight, d.candidate_limit, d.out_stats) == (
        200, 0, [4, 5, 6], 2, [1, 2, 3], [0.5, 0.25, 2], 0.5, -0.25, 3, 77, 0x3000)
    assert [tuple(getattr(c, m) for m in CH_MEMBERS) for c in d.channels] == [(ONE, 0, 0, 30, A.LIFETIME.id, 0, 0, 0), (A.VELOCITY.id, 2, 1, 12, A.VELOCITY.id, 1, 1, 0), (0,) * 8, (0,) * 8]
    d = runtime.neighbour_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 1.0, [(ONE, 0, 0, 0, A.LIFETIME.id, 0, SET)])
    assert (d.weight, d.candidate_limit, d.scale, d.n_channels, d.out_stats) == (0, 4096, 1.0, 1, None)
    lib = runtime.load_library()
    assert runtime.ABI_NEIGHBOUR_SYMBOLS == ["hnb_effect_neighbours"]
    full = open(os.path.join(ROOT, "include", "hanabi_amd_neighbours.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(lib, "hnb_effect_neighbours") and lib.hnb_effect_neighbours.argtypes == [C.c_void_p, C.POINTER(runtime.NeighbourDesc)]
    m = re.search(r"int\s+hnb_effect_neighbours\s*\(([^)]*)\)\s*;", header)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["HnbEffect* fx", "const HnbNeighbourDesc* desc"]
    m = re.search(r"\bfn hnb_effect_neighbours\(([^)]*)\) -> c_int;", txt)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["fx: *mut HnbEffect", "desc: *const HnbNeighbourDesc"]
    assert "pub unsafe fn effect_neighbours(" in txt
    assert list(inspect.signature(runtime.Effect.neighbours).parameters) == ["self", "dims", "origin", "inv_cell", "radius", "channels", "weight", "candidate_limit", "scale", "stats_ptr"]
    assert not hasattr(runtime.Program, "neighbours")                     # (no program form: out of scope, the header says so)
    # every header declares exactly its own symbols: hanabi_amd.h and its 61 are as they were, and the companion lists do not overlap
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", header)) == set(runtime.ABI_NEIGHBOUR_SYMBOLS)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", main)) == set(runtime.ABI_SYMBOLS) and len(runtime.ABI_SYMBOLS) == 61
    for other in (runtime.ABI_SYMBOLS, runtime.ABI_BINNED_SYMBOLS, runtime.ABI_IMPORT_SYMBOLS, runtime.ABI_DEPOSIT_SYMBOLS, runtime.ABI_SAMPLE_SYMBOLS, runtime.ABI_SPLAT_SYMBOLS,
                  runtime.ABI_SAMPLE_PROGRAM_SYMBOLS):
        assert not set(runtime.ABI_NEIGHBOUR_SYMBOLS) & set(other)
    assert '#include "hanabi_amd.h"' in full and '#include "hanabi_amd_binned.h"' in full
    bound = set(re.findall(r"pub fn (hnb_[a-z0-9_]+)\(", txt))
    assert not set(runtime.ABI_NEIGHBOUR_SYMBOLS) & bound                 # (the `pub fn` set mirrors hanabi_amd.h and the host header: the call sits in a module of its own)
    rust_of = lambda name: [" ".join(line.split("//")[0].split()).rstrip(",") for line in
                            re.search(r"#\[repr\(C\)\]\s*pub struct " + name + r" \{(.*?)\}", txt, flags=re.S).group(1).splitlines() if line.split("//")[0].strip()]
    assert rust_of("HnbNeighbourDesc") == ["pub struct_size: u32", "pub flags: u32", "pub dims: [u32; 3]", "pub n_channels: u32", "pub origin: [f32; 3]", "pub inv_cell: [f32; 3]",
                                           "pub radius: f32", "pub scale: f32", "pub weight: u32", "pub candidate_limit: u32", "pub channels: [HnbNeighbourChannel; 4]",
                                           "pub out_stats: *mut u32"]
    assert rust_of("HnbNeighbourChannel") == [f"pub {n}: u32" for n in CH_MEMBERS]
    for word in ("OUTSIDE BIN", "d2 = s + zz", "CROWDED", "symmetric bit for bit", "W = (u * u) * u", "modulo 2^64", "ties to even", "Out of scope: a program form",
                 "a neighbour list as output", "per-channel scales", "0xFFFFFF00 slots", "radius * inv_cell[c] <= 1"):
        assert word in full, word


def test_call_fails_loudly_on_null_arguments_and_without_a_device():
    """Up to the device check: the NULL refusals come before anything is dereferenced, loaded or enqueued. The refusals of a description's members
    need an effect, and an effect a device: the stand-alone program below holds them, and tests/test_gpu_neighbours.py on a live effect."""
    lib = runtime.load_library()
    d = runtime.neighbour_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 1.0, [(ONE, 0, 0, 0, A.LIFETIME.id, 0, SET)])
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for args in ((None, C.byref(d)), (fake, None), (None, None)):
        assert lib.hnb_effect_neighbours(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no effect to gather into, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the code object --------------------------------------------------------------------------------------------------------------------------------
def test_code_object_is_built_carried_and_has_its_two_kernels_without_scratch_or_spills():
    co = hb.neighbours_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_neighbours.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(NEIGHBOUR_KERNELS), sorted(rows)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## Neighbours" in design and design.index("## Sample") < design.index("## Neighbours") < design.index("## Measurement (row d)")
    for name, r in rows.items():
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["kernarg_segment_size"] == 248, (name, r)                # one NeighbourArgs by value
        assert r["vgpr_count"] <= 64, (name, r)                           # eight waves per SIMD stay possible
        assert r["group_segment_fixed_size"] <= 32, (name, r)             # the stats' five words: the candidates are not staged in LDS
        row = f"| `{name}` | {r['vgpr_count']} | {r['sgpr_count']} | {r['group_segment_fixed_size']} |"
        assert row in design, f"DESIGN.md \"Neighbours\" resource table: {row}"
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_neighbours_code)
    for h in ("hnb_neighbours.h", "hnb_deposit.h", "hnb_bin_cell.h", "hnb_export_bin.h"):
        assert f'"{h}"' in inspect.getsource(hb.build_neighbours_code)
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_neighbours.hip")).read()
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_neighbours.h")).read()
    assert hb.NEIGHBOURS_CODE_OBJECTS == (hb.build_neighbours_code,)
    assert (hb.BINNED_CODE_OBJECTS, hb.SAMPLE_CODE_OBJECTS, hb.DEPOSIT_CODE_OBJECTS) == ((hb.build_export_bin_code,), (hb.build_sample_code,), (hb.build_deposit_code,))
    assert "NEIGHBOURS_CODE_OBJECTS" in inspect.getsource(hb.build_runtime) and "hanabi_amd_neighbours.h" in inspect.getsource(hb.build_runtime)
    assert "hanabi_amd_neighbours.h" in inspect.getsource(hb._build_code_object)
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "bevy_hanabi_amd/csrc/hnb_neighbours_code.inc" in ignored and "*.hsaco" in ignored
    for other in (hb.export_bin_code_path(), hb.sample_code_path(), hb.deposit_code_path(), hb.export_sort_code_path()):
        assert not set(_rows(other)) & set(NEIGHBOUR_KERNELS)


# ---- csrc/hnb_neighbours.h as a stand-alone host program under the sanitizers ---------------------------------------------------------------------
ERRORS = ["Ok", "ErrStructSize", "ErrFlags", "ErrDims", "ErrOrigin", "ErrInvCell", "ErrRadius", "ErrCoverage", "ErrRadiusSquared", "ErrWeight", "ErrCandidateLimit", "ErrChannelCount",
          "ErrSrcAttr", "ErrSrcComp", "ErrChannelFlags", "ErrDiffOne", "ErrFracBits", "ErrDstAttr", "ErrDstComp", "ErrOp", "ErrChannelReserved", "ErrDuplicate", "ErrUnusedChannel",
          "ErrScale", "ErrStats", "ErrNoPosition", "ErrCapacity"]
E = {n: i for i, n in enumerate(ERRORS)}
# what the check is given: (attr, ncomp, is_f32); layout 1 has no POSITION
LAYOUT = [(A.POSITION.id, 3, 1), (A.VELOCITY.id, 3, 1), (A.AGE.id, 1, 1), (A.LIFETIME.id, 1, 1), (A.COLOR.id, 1, 0), (A.HDR_COLOR.id, 4, 1), (A.SIZE2.id, 2, 1)]

HOST_SRC = r"""
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>
#include "hnb_neighbours.h"
using namespace hnb;
""" + "\n".join(f"static_assert(kNeighbour{n} == {i}, \"NeighbourDescError\");" for i, n in enumerate(ERRORS)) + r"""
static_assert(kNeighbourDescErrorCount == """ + str(len(ERRORS)) + r""", "NeighbourDescError");
static_assert(sizeof(HnbNeighbourDesc) == 200 && sizeof(NeighbourArgs) == 248 && kNeighbourKPack == 0 && kNeighbourKGather == 1 && kNeighbourKernelCount == 2, "hnb_neighbours.h");
static_assert(kNeighbourBlock == 256 && kNeighbourOneBits == 0x3F800000u, "hnb_neighbours.h");
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
            for (uint32_t i = 0; i < kNeighbourKernelCount; ++i) std::printf("%u:%s ", kNeighbourKernelNames[i].kernel, kNeighbourKernelNames[i].name);
            std::printf("\n");
        } else if (!std::strcmp(what, "plan")) {
            unsigned cap, n_cells;
            if (std::scanf("%u %u", &cap, &n_cells) != 2) return 1;
            const NeighbourPlan pl = neighbour_launch_plan(cap, n_cells);
            if (pl.sort.n > kExportPlanMax) return 5;
            std::printf("%d %u %u %llu", pl.sort.memset_before == kExportNoMemset ? -1 : (int)pl.sort.memset_before, pl.pack_grid, pl.gather_grid, (unsigned long long)pl.clear_stats_bytes);
            for (uint32_t i = 0; i < pl.sort.n; ++i) {
                const ExportLaunch& l = pl.sort.launch[i];
                if (l.grid_y != 1u || l.args != (l.kernel >= kExportBinKernelBase ? kExportArgsBin : kExportArgsSortPass)) return 5;
                std::printf(" %s:%u:%u", launch_name(l.kernel), l.grid_x, l.pass);
            }
            if (pl.sort.memset_before != kExportNoMemset) {
                const ExportSortScratch s = export_sort_scratch_layout(1u, cap, HNB_SORT_SCOPE_INSTANCE);
                if (pl.sort.zero_off != s.state_off || pl.sort.zero_bytes != s.zero_bytes) return 5;
            }
            std::printf("\n");
        } else if (!std::strcmp(what, "layout")) {
            unsigned cap, nch, n_cells;
            if (std::scanf("%u %u %u", &cap, &nch, &n_cells) != 3) return 1;
            const NeighbourScratch l = neighbour_scratch_layout(cap, nch, n_cells);
            std::printf("%llu %llu %llu %llu %llu %llu %llu %llu %u\n", (unsigned long long)l.snap_off, (unsigned long long)l.snap_bytes, (unsigned long long)l.src_off,
                        (unsigned long long)l.src_bytes, (unsigned long long)l.cells_off, (unsigned long long)l.cells_bytes, (unsigned long long)l.total, (unsigned long long)l.sort.total,
                        l.sort.pitch);
        } else if (!std::strcmp(what, "pair")) {  // one pair through the kernels' own functions: neighbour? d2, W, ok, q
            unsigned w, diff, frac, b[10];
            if (std::scanf("%u %u %u %x %x %x %x %x %x %x %x %x %x", &w, &diff, &frac, &b[0], &b[1], &b[2], &b[3], &b[4], &b[5], &b[6], &b[7], &b[8], &b[9]) != 13) return 1;
            const float d2 = neighbour_d2(f_of(b[0]), f_of(b[1]), f_of(b[2]), f_of(b[3]), f_of(b[4]), f_of(b[5]));
            const float W = neighbour_weight(w, d2, f_of(b[9]));
            const DepositQuant q = neighbour_contribution(b[7], b[6], diff != 0, w, W, frac);
            std::printf("%d %x %x %d %lld\n", d2 < f_of(b[8]) ? 1 : 0, b_of(d2), b_of(W), q.ok ? 1 : 0, (long long)q.q);
        } else if (!std::strcmp(what, "store")) {
            unsigned op, frac, sb, vb; long long S;
            if (std::scanf("%u %lld %u %x %x", &op, &S, &frac, &sb, &vb) != 5) return 1;
            std::printf("%x\n", b_of(neighbour_store(op, f_of(vb), (int64_t)S, frac, f_of(sb))));
        } else if (!std::strcmp(what, "run")) {   // a whole state through the header: cells, a stable sort, the table, the guard, the walk, the store
            BinGrid g = {};
            unsigned ob[3], ib[3], rb, sb, weight, limit, nch, n;
            if (std::scanf("%u %u %u %x %x %x %x %x %x %x %x %u %u %u %u", &g.dims[0], &g.dims[1], &g.dims[2], &ob[0], &ob[1], &ob[2], &ib[0], &ib[1], &ib[2], &rb, &sb, &weight, &limit,
                           &nch, &n) != 15) return 1;
            for (int c = 0; c < 3; ++c) { g.origin[c] = f_of(ob[c]); g.inv_cell[c] = f_of(ib[c]); }
            g.n_cells = bin_cell_count(g.dims);
            if (nch > 4u) return 1;
            unsigned one[4], diff[4], frac[4], op[4];
            for (unsigned k = 0; k < nch; ++k)
                if (std::scanf("%u %u %u %u", &one[k], &diff[k], &frac[k], &op[k]) != 4) return 1;
            std::vector<uint32_t> pos(3 * (size_t)n), src(nch * (size_t)n), dstv(nch * (size_t)n);
            for (size_t i = 0; i < n; ++i) {
                if (std::scanf("%x %x %x", &pos[3 * i], &pos[3 * i + 1], &pos[3 * i + 2]) != 3) return 1;
                for (unsigned k = 0; k < nch; ++k)
                    if (std::scanf("%x %x", &src[k * (size_t)n + i], &dstv[k * (size_t)n + i]) != 2) return 1;
            }
            const float radius = f_of(rb), r2 = radius * radius, inv_r2 = 1.0f / r2;
            std::vector<uint32_t> cell(n), order(n);
            for (size_t i = 0; i < n; ++i) cell[i] = bin_cell_of(g, f_of(pos[3 * i]), f_of(pos[3 * i + 1]), f_of(pos[3 * i + 2]));
            std::iota(order.begin(), order.end(), 0u);
            std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cell[x] < cell[y]; });
            std::vector<uint32_t> start(export_bin_entries(g.n_cells));     // exactly n_cells + 2 entries on the heap: a read past them is an error the sanitizer reports
            for (uint32_t c = 0; c < start.size(); ++c)
                start[c] = (uint32_t)(std::lower_bound(order.begin(), order.end(), c, [&](uint32_t row, uint32_t key) { return cell[row] < key; }) - order.begin());
            std::vector<std::vector<long long>> line(n);
            unsigned long long rejected = 0;
            for (uint32_t r = 0; r < n; ++r) {
                const uint32_t i = order[r];
                if (r >= start[g.n_cells]) { line[i] = {0}; continue; }
                const NeighbourCell c = neighbour_cell_xyz(g.dims, cell[i]);
                const uint32_t cand = neighbour_candidates(start.data(), g.dims, c);
                if (cand > limit) { line[i] = {1, (long long)cand}; continue; }
                int64_t S[4] = {0, 0, 0, 0};
                uint32_t walked = 0;
                for (uint32_t w = 0; w < 9u; ++w) {
                    const NeighbourRange rg = neighbour_range(start.data(), g.dims, c, w);
                    for (uint32_t jr = rg.lo; jr < rg.hi; ++jr) {
                        ++walked;
                        if (jr == r) continue;
                        const uint32_t j = order.at(jr);
                        const float d2 = neighbour_d2(f_of(pos[3 * i]), f_of(pos[3 * i + 1]), f_of(pos[3 * i + 2]), f_of(pos[3 * j]), f_of(pos[3 * j + 1]), f_of(pos[3 * j + 2]));
                        if (!(d2 < r2)) continue;
                        const float W = neighbour_weight(weight, d2, inv_r2);
                        for (unsigned k = 0; k < nch; ++k) {
                            const DepositQuant q = neighbour_contribution(one[k] ? kNeighbourOneBits : src[k * (size_t)n + j], src[k * (size_t)n + i], diff[k] != 0, weight, W, frac[k]);
                            S[k] = (int64_t)((uint64_t)S[k] + (uint64_t)q.q);
                            rejected += q.ok ? 0u : 1u;
                        }
                    }
                }
                if (walked != cand) return 6;
                line[i] = {2, (long long)cand};
                for (unsigned k = 0; k < nch; ++k) {
                    line[i].push_back((long long)S[k]);
                    line[i].push_back((long long)b_of(neighbour_store(op[k], f_of(dstv[k * (size_t)n + i]), S[k], frac[k], f_of(sb))));
                }
            }
            std::printf("%llu", rejected);
            for (uint32_t i = 0; i < n; ++i) {
                std::printf(" |");
                for (long long v : line[i]) std::printf(" %lld", v);
            }
            std::printf("\n");
        } else if (!std::strcmp(what, "desc")) {
            HnbNeighbourDesc d;
            std::memset(&d, 0, sizeof d);
            unsigned long long stats; unsigned layout_first, cap, ob[3], ib[3], rb, sb;
            if (std::scanf("%u %u %u %u %u %u %u %u %x %x %x %x %x %x %x %x %u %u %llx", &layout_first, &cap, &d.struct_size, &d.flags, &d.dims[0], &d.dims[1], &d.dims[2], &d.n_channels,
                           &ob[0], &ob[1], &ob[2], &ib[0], &ib[1], &ib[2], &rb, &sb, &d.weight, &d.candidate_limit, &stats) != 19) return 1;
            std::memcpy(d.origin, ob, 12); std::memcpy(d.inv_cell, ib, 12); d.radius = f_of(rb); d.scale = f_of(sb);
            d.out_stats = (uint32_t*)(uintptr_t)stats;
            for (unsigned k = 0; k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) {
                HnbNeighbourChannel& ch = d.channels[k];
                if (std::scanf("%u %u %u %u %u %u %u %u", &ch.src_attr, &ch.src_comp, &ch.flags, &ch.frac_bits, &ch.dst_attr, &ch.dst_comp, &ch.op, &ch.reserved) != 8) return 1;
            }
            if (layout_first > 1) return 1;
            const NeighbourCheck c = neighbour_check_desc(d, kLayout + layout_first, (uint32_t)(sizeof kLayout / sizeof *kLayout) - layout_first, cap);
            if (c.error >= kNeighbourDescErrorCount || !neighbour_error_text(c.error)[1]) return 3;
            std::printf("%u %u %u %u %x %x %d", c.error, c.channel, c.n_cells, c.position_index, b_of(c.r2), b_of(c.inv_r2), c.has_age ? 1 : 0);
            for (uint32_t k = 0; k < d.n_channels && k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) std::printf(" %u %u", c.src_index[k], c.dst_index[k]);
            std::printf("\n");
        } else return 4;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """g++ alone, with the address and undefined-behaviour sanitizers and no contraction: the header is plain C++ on the host. The program has its
    own main and is run directly."""
    tmp = tmp_path_factory.mktemp("neighbours_host")
    (tmp / "nb.cpp").write_text(HOST_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), str(tmp / "nb.cpp"), "-o", str(tmp / "nb")])
    return str(tmp / "nb")


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()      # (a sanitizer report ends the program with an error)
    assert len(out) == len(lines)
    return out


def _f32(x):
    return int(np.array([x], F32).view(U32)[0])


GOOD_CH = ((ONE, 0, 0, 30, A.LIFETIME.id, 0, SET, 0), (A.VELOCITY.id, 1, DIFF, 12, A.HDR_COLOR.id, 3, ADD, 0))


def _desc_line(layout_first=0, cap=10_000, struct_size=200, flags=0, dims=(4, 4, 4), n_channels=2, origin=(0.0, 0.0, 0.0), inv_cell=(1.0, 1.0, 1.0), radius=0.75, scale=1.0, weight=3,
               limit=4096, stats=0x3000, channels=GOOD_CH):
    ch = list(channels) + [(0,) * 8] * (4 - len(channels))
    return ("desc %d %d %d %d %d %d %d %d " % (layout_first, cap, struct_size, flags, *dims, n_channels) + " ".join("%x" % _f32(x) for x in tuple(origin) + tuple(inv_cell) + (radius, scale))
            + " %d %d %x " % (weight, limit, stats) + " ".join("%d %d %d %d %d %d %d %d" % tuple(c) for c in ch))


def test_description_check_refuses_what_the_header_lists_every_error_class(host_exe):
    raw = lambda **kw: _ask(host_exe, [_desc_line(**kw)])[0].split()
    ask = lambda **kw: [int(x) for x in raw(**kw)[:4]]
    hit = set()

    def refused(name, channel=None, **kw):
        got = ask(**kw)
        assert got[0] == E[name] and (channel is None or got[1] == channel), (name, kw, got)
        hit.add(name)

    w = raw()
    assert [int(x) for x in w[:4]] == [E["Ok"], 0, 64, 0] and [int(w[4], 16), int(w[5], 16)] == [_f32(F32(0.75) * F32(0.75)), _f32(F32(1) / (F32(0.75) * F32(0.75)))]
    assert [int(x) for x in w[6:]] == [0, 0xFFFFFFFF, 3, 1, 5]           # no AGE; ATTR_ONE has no entry; LIFETIME; VELOCITY; HDR_COLOR
    assert raw(channels=((A.AGE.id, 0, 0, 0, A.POSITION.id, 2, ADD, 0),), n_channels=1)[6] == "1"      # AGE as a source: to be materialised
    assert ask(radius=1.0, weight=0, limit=1, stats=0, scale=-0.0)[0] == E["Ok"] and ask(limit=65536, cap=0xFFFFFF00)[0] == E["Ok"]
    assert ask(n_channels=4, channels=((A.POSITION.id, 0, DIFF, 32, A.POSITION.id, 0, ADD, 0), (A.VELOCITY.id, 0, 0, 0, A.VELOCITY.id, 0, SET, 0), (ONE, 0, 0, 0, A.SIZE2.id, 1, SET, 0),
                                       (A.SIZE2.id, 1, 0, 5, A.POSITION.id, 1, SET, 0)))[0] == E["Ok"]    # a destination may be a source, POSITION included
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
        i = [1.0] * 3; i[axis] = float(np.nextafter(F32(4 / 3), F32(2)))    # 0.75 * 4/3 rounded up: past 1 in double
        refused("ErrCoverage", axis, inv_cell=i)
    for bad in (np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0):
        refused("ErrRadius", radius=bad)
    refused("ErrCoverage", 0, radius=float(np.nextafter(F32(1.0), F32(2))))
    tiny = (1e-30,) * 3
    refused("ErrRadiusSquared", radius=1e-20, inv_cell=tiny)               # r2 = 1e-40: a denormal
    refused("ErrRadiusSquared", radius=1e-30, inv_cell=tiny)               # r2 = 0, inv_r2 = inf
    refused("ErrRadiusSquared", radius=1e20, inv_cell=tiny)                # r2 = inf
    assert ask(radius=1.1e-19, inv_cell=tiny)[0] == E["Ok"]                # r2 = 1.21e-38: normal, inv_r2 finite
    for weight in (4, 0xFFFFFFFF):
        refused("ErrWeight", weight=weight)
    for limit in (0, 65537, 0xFFFFFFFF):
        refused("ErrCandidateLimit", limit=limit)
    refused("ErrChannelCount", n_channels=5)
    refused("ErrChannelCount", n_channels=0, channels=())
    good = GOOD_CH[0]
    ch = lambda **kw: (good, tuple(kw.get(m, v) for m, v in zip(CH_MEMBERS, GOOD_CH[1])))
    for attr in (A.COLOR.id, A.SIZE3.id, A.ID.id, A.PARTICLE_COUNTER.id, 39, 9999):          # packed u32; not in the layout; not stored; no attribute
        refused("ErrSrcAttr", 1, channels=ch(src_attr=attr, src_comp=0))
    for attr, comp in ((A.LIFETIME.id, 1), (A.POSITION.id, 3), (ONE, 1), (A.SIZE2.id, 0xFFFFFFFF)):
        refused("ErrSrcComp", 1, channels=ch(src_attr=attr, src_comp=comp, flags=0))
    for flags in (2, 3, 0x80000000):
        refused("ErrChannelFlags", 1, channels=ch(flags=flags))
    refused("ErrDiffOne", 1, channels=ch(src_attr=ONE, src_comp=0))
    for frac in (33, 0xFFFFFFFF):
        refused("ErrFracBits", 1, channels=ch(frac_bits=frac))
    for attr in (A.AGE.id, A.COLOR.id, A.SIZE3.id, A.ID.id, ONE, 9999):
        refused("ErrDstAttr", 1, channels=ch(dst_attr=attr, dst_comp=0))
    for attr, comp in ((A.LIFETIME.id, 1), (A.POSITION.id, 3), (A.HDR_COLOR.id, 4)):
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
    refused("ErrNoPosition", layout_first=1, channels=((ONE, 0, 0, 0, A.LIFETIME.id, 0, SET, 0),), n_channels=1)
    for cap in (0xFFFFFF01, 0xFFFFFFFF):
        refused("ErrCapacity", cap=cap)
    assert hit == set(ERRORS[1:]), set(ERRORS[1:]) - hit                   # every error class at least once


def test_scratch_layout_and_launch_plan_are_their_restatements(host_exe):
    assert _ask(host_exe, ["names"])[0].split() == [f"{i}:{n}" for i, n in enumerate(NEIGHBOUR_KERNELS)]
    caps = [1, 4096, 4097, 10_000, 16_777_216]
    for cap in caps:
        for n_cells, nch in ((1, 1), (512, 3), (68_921, 4), (1 << 24, 2)):
            lay, plan = _ask(host_exe, ["layout %d %d %d" % (cap, nch, n_cells), "plan %d %d" % (cap, n_cells)])
            lay = [int(x) for x in lay.split()]
            want = neighbour_layout(cap, nch, n_cells)
            sl = sort_layout(1, cap, INSTANCE)
            assert tuple(lay[:7]) == want and lay[7] == sl[10] and lay[8] == sl[2], (cap, n_cells, nch, lay, want)
            offs = [lay[0], lay[2], lay[4], lay[6]]
            assert all(o % 256 == 0 for o in offs) and lay[7] <= lay[0] and lay[0] + lay[1] <= lay[2] and lay[2] + lay[3] <= lay[4] and lay[4] + lay[5] <= lay[6]
            assert lay[1] >= 16 * cap and lay[3] >= 4 * nch * cap and lay[5] == 4 * (n_cells + 2)
            w = plan.split()
            L, memset, pack, gather = neighbour_plan(cap, n_cells)
            assert (int(w[0]), int(w[1]), int(w[2]), int(w[3])) == (-1 if memset is None else memset, pack, gather, 32), (cap, w)
            got = [(x.split(":")[0], int(x.split(":")[1])) for x in w[4:]]
            assert got == L, (cap, n_cells, got, L)
            passes = [int(x.split(":")[2]) for x in w[4:] if x.startswith("sort_scatter")]
            assert passes == ([] if cap <= 4096 else [0, 1, 2, 3])
            assert (pack - 1) * 256 < cap <= pack * 256 and len(L) + 2 <= (4 if cap <= 4096 else 11)      # every row has a lane; few launches at small capacities


# ---- the rule, through the kernels' own functions -----------------------------------------------------------------------------------------------------
def _np_pair(w, diff, frac, pi, pj, vi, vj, r2, inv_r2):
    d2 = np_d2(np.array([pi], F32), np.array([pj], F32))
    W = np_weight(w, d2, inv_r2)
    ok, q = np_contribution(np.array([vj], U32), np.array([vi], U32), diff, w, W, frac)
    return "%d %x %x %d %d" % (int(d2[0] < r2), int(d2.view(U32)[0]), int(W.view(U32)[0]), int(ok[0]), int(q[0]))


def test_pair_rule_and_store_at_the_edge_operands(host_exe):
    up, down = (lambda x: np.nextafter(F32(x), F32(np.inf))), (lambda x: np.nextafter(F32(x), F32(-np.inf)))
    bits = lambda f: int(np.array([f], F32).view(U32)[0])
    cases, seen = [], dict(eq=0, below=0, above=0, coincident=0, u_zero=0, u_negative=0, at_threshold=0, below_threshold=0)
    r2 = F32(0.5) * F32(0.5)
    inv = F32(1) / r2
    one = 0x3F800000
    for dx, tag in ((F32(0.5), "eq"), (down(0.5), "below"), (up(0.5), "above"), (F32(0.0), "coincident")):      # d2 == r2 is no neighbour; one ulp of dx either side; the same point
        for w in (W_ONE, W_U1, W_U2, W_U3):
            cases.append((w, 0, 20, (0.0, 2.0, 3.0), (float(dx), 2.0, 3.0), one, one, r2, inv))
        seen[tag] += 1
    # u rounding to 0: a neighbour one ulp of d2 below r2 whose q rounds to 1. u rounding to a negative number: with d2 < r2 the product q stays
    # below 1 + 2^-48 and rounds to at most 1, so a negative u is met only at d2 >= r2 - no neighbour, but the weight function still follows the formula
    rng = np.random.default_rng(5)

    def pair_with_d2(target, radius):
        """(dx, dy) with fl(fl(dx * dx) + fl(dy * dy)) == target, dx one ulp below the radius; None when the scan finds none"""
        dx = down(radius)
        rest = np.float64(target) - np.float64(dx * dx)
        if rest <= 0:
            return None
        dy = F32(np.sqrt(rest))
        for _ in range(40):
            dy = down(dy)
        for _ in range(80):
            if dx * dx + dy * dy == target:
                return float(dx), float(dy)
            dy = up(dy)
        return None

    for radius in rng.uniform(0.1, 2.0, 3000).astype(F32):
        rr = F32(radius) * F32(radius)
        ir = F32(1) / rr
        for d2, tag in ((down(rr), "u_zero"), (rr, "u_negative"), (up(rr), "u_negative")):
            u = F32(1) - d2 * ir
            if seen[tag] < 4 and ((u == 0) if tag == "u_zero" else (u < 0)):
                d = pair_with_d2(d2, radius)
                if d is not None:
                    for w in (W_U1, W_U2, W_U3):
                        cases.append((w, 0, 30, (0.0, 0.0, 0.0), (d[0], d[1], 0.0), one, one, rr, ir))
                    seen[tag] += 1
    # a contribution at the rejection threshold: 2^30 at frac_bits 32 is 2^62 units (rejected), the value below it is accepted; NaN and inf sources
    for vj, tag in ((F32(2.0 ** 30), "at_threshold"), (down(2.0 ** 30), "below_threshold"), (F32(-2.0 ** 30), "at_threshold"), (F32(np.nan), None), (F32(np.inf), None), (F32(1e30), None)):
        cases.append((W_ONE, 0, 32, (0.0, 0.0, 0.0), (0.25, 0.0, 0.0), one, bits(vj), r2, inv))
        cases.append((W_U1, 1, 32, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), bits(F32(0.0)), bits(vj), r2, inv))      # W = 1 at d2 = 0, v - 0
        if tag:
            seen[tag] += 1
    for _ in range(1500):                                                  # and a random sweep: denormal and signed-zero sources, every weight, DIFF or not
        pi = rng.normal(0, 1, 3).astype(F32)
        pj = (pi + rng.normal(0, 0.4, 3)).astype(F32)
        v = rng.choice([rng.normal(0, 100), 1e-41, -0.0, 3e38, -1e-45, rng.normal(0, 1e-3)], 2).astype(F32)
        radius = F32(rng.uniform(0.2, 1.0))
        rr = radius * radius
        cases.append((int(rng.integers(4)), int(rng.integers(2)), int(rng.integers(33)), tuple(pi.tolist()), tuple(pj.tolist()), bits(v[0]), bits(v[1]), rr, F32(1) / rr))
    lines = ["pair %d %d %d " % c[:3] + " ".join("%x" % bits(x) for x in c[3] + c[4]) + " %x %x %x %x" % (c[5], c[6], bits(c[7]), bits(c[8])) for c in cases]
    got = _ask(host_exe, lines)
    want = [_np_pair(*c) for c in cases]
    bad = [(l, g, w) for l, g, w in zip(lines, got, want) if g != w]
    assert not bad, (len(bad), bad[:5])
    assert all(v > 0 for v in seen.values()), seen
    flags = [int(g.split()[0]) for g in got[:16]]
    assert flags == [0] * 4 + [1] * 4 + [0] * 4 + [1] * 4                  # d2 == r2: no; below: yes; above: no; coincident: yes
    k = next(i for i, c in enumerate(cases) if c[2] == 32 and c[6] == bits(F32(2.0 ** 30)))
    assert got[k].split()[3:] == ["0", "0"] and got[k + 2].split()[3:] == ["1", str((2 ** 30 - 64) << 32)]
    # the store: the int64 -> f32 rounding at +-(2^24 + 1) (ties to even), larger sums, every frac_bits edge, SET and ADD
    sums = [0, 1, -1, (1 << 24) + 1, -(1 << 24) - 1, (1 << 24) + 3, -(1 << 24) - 3, (1 << 25) + 2, (1 << 25) + 6, (1 << 62) - 1, -(1 << 62), (1 << 63) - 1, -(1 << 63), 123456789012345]
    st = [(op, S, frac, scale, v) for op in (SET, ADD) for S in sums for frac in (0, 1, 30, 32) for scale, v in ((1.0, 0.5), (-0.25, -3.0), (2.0 ** -120, 1e-40))]
    got = _ask(host_exe, ["store %d %d %d %x %x" % (op, S, frac, bits(scale), bits(v)) for op, S, frac, scale, v in st])
    want = ["%x" % int(np_store(op, np.array([v], F32), np.array([S], np.int64), frac, scale).view(U32)[0]) for op, S, frac, scale, v in st]
    assert got == want, [(s, g, w) for s, g, w in zip(st, got, want) if g != w][:5]
    assert np_store(SET, [F32(0)], [(1 << 24) + 1], 0, 1.0).view(U32)[0] == bits(F32(2.0 ** 24)) and np_store(SET, [F32(0)], [-(1 << 24) - 3], 0, 1.0)[0] == -F32(2.0 ** 24 + 4)


# ---- whole states: the header's walk against the brute-force restatement ------------------------------------------------------------------------------
def _run_line(pos, src, dstv, grid, radius, scale, weight, limit, channels):
    dims, origin, inv_cell = grid
    head = "run %d %d %d " % tuple(dims) + " ".join("%x" % _f32(x) for x in tuple(origin) + tuple(inv_cell) + (radius, scale)) + " %d %d %d %d " % (weight, limit, len(channels), len(pos))
    head += " ".join("%d %d %d %d" % (int(c[0] == ONE), c[2] & DIFF, c[3], c[6]) for c in channels)
    rows = np.concatenate([np.asarray(pos, F32).view(U32).reshape(-1, 3)] + [np.stack([s, d], axis=1) for s, d in zip(src, dstv)], axis=1)
    return head + " " + " ".join("%x" % w for w in rows.reshape(-1))


STATES = [((3, 3, 3), 0.3, 400, 4096), ((5, 4, 3), 0.25, 700, 4096), ((1, 1, 1), 1.0, 60, 4096), ((2, 1, 7), 0.14, 300, 110), ((4, 4, 4), 0.25, 500, 30)]


@pytest.mark.parametrize("dims,radius,n,limit", STATES, ids=["x".join(map(str, s[0])) + f"-limit{s[3]}" for s in STATES])
def test_whole_states_through_the_header_are_the_brute_force_restatement_bit_for_bit(host_exe, dims, radius, n, limit):
    """positions uniform in and a little around the unit cube - part of them outside -, a cluster in one cell (crowding under the small limits),
    coincident pairs, a NaN and an infinite position; sources with denormals, zeros and values that are rejected at frac_bits 32"""
    rng = np.random.default_rng(n)
    pos = rng.uniform(-0.05, 1.05, (n, 3)).astype(F32)
    pos[: n // 6] = (F32(0.4) + rng.uniform(0, 0.05, (n // 6, 3))).astype(F32)
    pos[n // 6: n // 6 + 5] = pos[n // 6 + 5: n // 6 + 10]                  # coincident pairs
    pos[-1] = (np.nan, 0.5, 0.5); pos[-2] = (0.5, np.inf, 0.5)
    grid = (dims, (0.0, 0.0, 0.0), tuple(float(d) for d in dims))
    vel = rng.normal(0, 3, n).astype(F32)
    vel[::9] = F32(1e-41); vel[4::13] = F32(-0.0); vel[5::37] = F32(1e30); vel[7::41] = F32(np.nan)
    channels = [(ONE, 0, 0, 0, A.LIFETIME.id, 0, SET), (ONE, 0, 0, 30, A.VELOCITY.id, 0, ADD), (A.POSITION.id, 0, DIFF, 20, A.POSITION.id, 0, ADD), (A.VELOCITY.id, 1, 0, 32, A.VELOCITY.id, 2, SET)]
    src = [one_source(n), one_source(n), pos[:, 0].copy().view(U32), vel.view(U32)]
    dstv = [rng.normal(0, 1, n).astype(F32).view(U32), rng.normal(0, 1, n).astype(F32).view(U32), src[2], rng.normal(0, 1, n).astype(F32).view(U32)]
    total = dict(gathered=0, crowded=0, outside=0, rejected=0, nb=0)
    for weight, scale in ((W_ONE, 1.0), (W_U1, -0.5), (W_U2, 2.0), (W_U3, 2.0 ** -100)):
        want = np_neighbours(pos, rng.permutation(n), src, grid, radius, weight, channels, limit)
        out = _ask(host_exe, [_run_line(pos, src, dstv, grid, radius, scale, weight, limit, channels)])[0].split(" | ")
        assert int(out[0]) == want["rejected"]
        for i, item in enumerate(out[1:]):
            w = [int(x) for x in item.split()]
            state = 2 if want["gathered"][i] else 1 if want["crowded"][i] else 0
            assert w[0] == state and (state == 0 or w[1] == want["cand"][i]), (i, w, state, want["cand"][i])
            if state == 2:
                for k, ch in enumerate(channels):
                    stored = np_store(ch[6], dstv[k][i: i + 1].view(F32), want["S"][i: i + 1, k], ch[3], scale).view(U32)[0]
                    assert w[2 + 2 * k] == want["S"][i, k], (i, k, w, want["S"][i])
                    assert w[3 + 2 * k] == stored or (np.isnan(np.array([stored], U32).view(F32)[0]) and np.isnan(np.array([w[3 + 2 * k]], U32).view(F32)[0])), (i, k, w)
        total["gathered"] += int(want["gathered"].sum()); total["crowded"] += int(want["crowded"].sum()); total["outside"] += n - int(want["inside"].sum())
        total["rejected"] += want["rejected"]; total["nb"] += int(want["nnb"].sum())
    assert total["gathered"] > 0 and total["outside"] > 0 and total["rejected"] > 0 and total["nb"] > total["gathered"], total
    assert (total["crowded"] > 0) == (limit < 4096), total
    if dims == (3, 3, 3):
        assert len(want["offsets"]) == 27                                  # every one of the 26 directions, and the own cell
