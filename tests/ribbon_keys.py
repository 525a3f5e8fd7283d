"""Chosen keys for the ribbon sort (hnb_sort.hip.h) and the numpy model of what the sort must produce.

The sort orders an effect's alive list by the 64-bit key (RIBBON_ID << 32 | AGE bits), ascending and stable with respect to
the list order. Every generator here returns the two halves of `n` such keys IN LIST ORDER, `(rid: uint32[n],
age_bits: uint32[n])`; a test scatters them into the attribute planes along the list (`planes`), runs one frame and compares
the list with `expected_list`, keyed on the planes AFTER the frame (the update has ticked the ages).

Every age any generator makes stays below LIFETIME under the ticks the tests use, except the NaNs of `nan_ages`: NaN < lifetime
is false, so those particles die in the frame (`survivors`) and the sort sees the compacted rest.
"""
import numpy as np

LIFETIME = np.float32(3e38)          # nothing a generator makes dies of old age; its bits are 0x7F61B1E6
_AGE_MAX_BITS = 0x7EFFFFFF           # the largest age bits used: about 1.7e38, finite and below LIFETIME


def _perm256(i, mul=167, add=13):
    """All 256 byte values, never in ascending order over two consecutive rows for long (167 is odd: a permutation of 0..255)."""
    return ((i.astype(np.uint64) * mul + add) % 256).astype(np.uint32)


def _idx(n):
    return np.arange(n, dtype=np.uint64)


def all_equal(n, seed):
    return np.full(n, 2, np.uint32), np.full(n, np.float32(0.75).view(np.uint32), np.uint32)


def one_byte(b):
    """Only byte `b` of the key varies and takes all 256 values: one active radix pass, the result in the buffer the pass wrote.
    The constant bytes of the age keep bit 23 clear, so that byte 3 = 0x7F / 0xFF is a large finite age (below LIFETIME), not inf / NaN."""
    def gen(n, seed):
        v = _perm256(_idx(n) + np.uint64(seed % 251))
        rid = np.full(n, 0x00010203, np.uint32)
        age = np.full(n, 0x3E123456 if b != 3 else 0x00123456, np.uint32)
        if b < 4:
            age = (age & np.uint32(~(0xFF << (8 * b)) & 0xFFFFFFFF)) | (v << np.uint32(8 * b))
        else:
            rid = (rid & np.uint32(~(0xFF << (8 * (b - 4))) & 0xFFFFFFFF)) | (v << np.uint32(8 * (b - 4)))
        return rid.astype(np.uint32), age.astype(np.uint32)
    gen.__name__ = f"one_byte{b}"
    return gen


def bytes_0_7(n, seed):
    """Bytes 0 and 7 vary: two active passes. RIBBON_ID takes 0x00000000, 0x80000000, 0xFF000000, ..."""
    i = _idx(n) + np.uint64(seed % 251)
    age = np.uint32(0x3F000000) | _perm256(i)
    rid = _perm256(i // np.uint64(3), mul=201, add=128) << np.uint32(24)
    return rid.astype(np.uint32), age.astype(np.uint32)


def bytes_1_2_4(n, seed):
    """Bytes 1, 2 and 4 vary: three active passes (an odd count: the result is in the other ping-pong buffer)."""
    i = _idx(n) + np.uint64(seed % 251)
    age = np.uint32(0x3F000011) | (_perm256(i) << np.uint32(8)) | ((_perm256(i // np.uint64(5), mul=91, add=7) & np.uint32(0x7F)) << np.uint32(16))
    rid = np.uint32(0x0A0B0C00) | _perm256(i // np.uint64(2), mul=77, add=255)
    return rid.astype(np.uint32), age.astype(np.uint32)


def all_bytes(n, seed):
    """Every byte varies: eight active passes. Ages of both signs, finite; RIBBON_ID includes 0, 0x80000000 and 0xFFFFFFFF."""
    rng = np.random.default_rng(seed)
    rid = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    age = (rng.integers(0, _AGE_MAX_BITS + 1, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(31))).astype(np.uint32)
    for j, v in enumerate((0x00000000, 0x80000000, 0xFFFFFFFF)):
        rid[(np.arange(n) % 11) == 2 + 3 * j] = v       # (rows 2, 5, 8 of every 11: present from n = 9 on, and many times: ties on the upper half)
    return rid, age


def few_distinct(n, seed):
    """Three distinct keys, interleaved: long runs of equal keys across every wave, round, tile and group boundary (stability)."""
    which = (_idx(n) * np.uint64(7919) % np.uint64(3)).astype(np.int64)
    rid = np.array([0, 0, 7], np.uint32)[which]
    age = np.array([1.0, 2.0, 0.5], np.float32).view(np.uint32)[which]
    return rid, age


def reversed_keys(n, seed):
    """Strictly descending keys: every element moves, every digit bucket is written back to front."""
    m = np.uint64(n - 1) - _idx(n) if n else _idx(0)
    rid = (m >> np.uint64(9)).astype(np.uint32)
    age = (np.uint64(0x3F000000) + (m & np.uint64(511)) * np.uint64(8)).astype(np.uint32)
    return rid, age


AGE_EDGES = np.array([0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x00800001, 0x3F800000, 0x3F7FFFFF, 0x7E800000, _AGE_MAX_BITS], np.uint32)


def age_bit_edges(n, seed):
    """+0, the smallest denormal, the largest denormal, the smallest normal, 1.0 and its neighbour, up to 0x7EFFFFFF; for a tick of 0."""
    rng = np.random.default_rng(seed)
    age = rng.integers(0, _AGE_MAX_BITS + 1, n, dtype=np.uint64).astype(np.uint32)
    edge = np.arange(n) % 3 != 0
    age[edge] = AGE_EDGES[(np.arange(int(edge.sum())) * 5 + seed) % len(AGE_EDGES)]     # (5 and 9 are coprime: every edge, none next to itself)
    rid = ((_idx(n) * np.uint64(31)) % np.uint64(2)).astype(np.uint32)
    return rid, age


def signed_ages(n, seed):
    """Ages of both signs around zero, -0.0 included; for a tick of 1/60: those in (-1/60, 0) cross zero in the frame. Keys are age BITS:
    negative ages sort behind positive ones, in reverse magnitude order."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.05, 0.05, n).astype(np.float32)
    a[np.arange(n) % 7 == 3] = np.float32(-0.0)
    a[np.arange(n) % 7 == 5] = np.float32(0.0)
    rid = ((_idx(n) * np.uint64(7919)) % np.uint64(3)).astype(np.uint32)
    return rid, a.view(np.uint32).copy()


def nan_ages(n, seed):
    """A tenth of the ages are quiet NaNs of both signs (0x7FC00000 | payload); the rest are ordinary positive ages."""
    rng = np.random.default_rng(seed)
    age = rng.uniform(0.0, 4.0, n).astype(np.float32).view(np.uint32).copy()
    nan = np.arange(n) % 10 == 4
    payload = rng.integers(0, 1 << 22, n, dtype=np.uint64).astype(np.uint32)
    sign = (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(31)).astype(np.uint32)
    age[nan] = (np.uint32(0x7FC00000) | payload | sign)[nan]
    rid = ((_idx(n) * np.uint64(13)) % np.uint64(4)).astype(np.uint32)
    return rid, age


# name -> (generator, tick of the frame that sorts)
PATTERNS = {"all_equal": (all_equal, 0.0)}
PATTERNS.update({f"one_byte{b}": (one_byte(b), 0.0) for b in range(8)})
PATTERNS.update({
    "bytes_0_7": (bytes_0_7, 0.0),
    "bytes_1_2_4": (bytes_1_2_4, 0.0),
    "all_bytes": (all_bytes, 0.0),
    "few_distinct": (few_distinct, 0.0),
    "reversed": (reversed_keys, 0.0),
    "age_bit_edges": (age_bit_edges, 0.0),
    "signed_ages": (signed_ages, 1.0 / 60.0),
    "nan_ages": (nan_ages, 0.0),
})


def key64(rid, age_bits):
    return (np.asarray(rid).astype(np.uint64) << np.uint64(32)) | np.asarray(age_bits).astype(np.uint64)


def varying_bytes(rid, age_bits):
    """Which of the key's 8 bytes differ among the given keys (what sort_pass_info turns into active passes)."""
    k = key64(rid, age_bits)
    if len(k) == 0:
        return []
    v = int(np.bitwise_or.reduce(k) ^ np.bitwise_and.reduce(k))
    return [b for b in range(8) if (v >> (8 * b)) & 0xFF]


def planes(capacity, list_before, rid, age_bits):
    """The RIBBON_ID, AGE and LIFETIME planes (uint32 [capacity, 1] each) that put key i on the particle in row i of the list."""
    rp, ap = np.zeros((capacity, 1), np.uint32), np.zeros((capacity, 1), np.uint32)
    rp[list_before, 0] = rid
    ap[list_before, 0] = age_bits
    lp = np.full((capacity, 1), LIFETIME.view(np.uint32), np.uint32)
    return rp, ap, lp


def survivors(list_before, age_bits_after, lifetime_bits):
    """The rows of the list whose particle is alive after the update (age < lifetime; false for a NaN), in list order: what compaction keeps."""
    a = np.asarray(age_bits_after, np.uint32).reshape(-1).view(np.float32)[list_before]
    life = np.asarray(lifetime_bits, np.uint32).reshape(-1).view(np.float32)[list_before]
    with np.errstate(invalid="ignore"):
        return list_before[a < life]


def expected_list(list_before, rid, age_bits_after):
    """The list the sort must leave: `list_before` (the alive rows in list order) by (RIBBON_ID, AGE bits) of the planes after the frame, stable."""
    key = key64(np.asarray(rid).reshape(-1), np.asarray(age_bits_after).reshape(-1))
    return list_before[np.argsort(key[list_before], kind="stable")]


def in_key_order(list_rows, rid, age_bits):
    key = key64(np.asarray(rid).reshape(-1), np.asarray(age_bits).reshape(-1))[list_rows]
    return bool((key[1:] >= key[:-1]).all())


def sort_asset(capacity):
    """A ribbon effect whose keys are whatever the host writes: no motion, no update modifier (the update only ticks AGE), AGE initialised from the
    property `a0`, RIBBON_ID = PARTICLE_COUNTER % property `k`, a lifetime nothing reaches."""
    import bevy_hanabi_amd as bh
    A = bh.Attribute
    w = bh.ExprWriter()
    a0 = w.prop(w.add_property("a0", bh.Value.f32(0.0)))
    k = w.prop(w.add_property("k", bh.Value.u32(1)))
    mods = [bh.SetAttributeModifier(A.POSITION, w.lit((0.0, 0.0, 0.0)).expr()),
            bh.SetAttributeModifier(A.AGE, a0.expr()),
            bh.SetAttributeModifier(A.LIFETIME, w.lit(float(LIFETIME)).expr()),
            bh.SetAttributeModifier(A.RIBBON_ID, (w.attr(A.PARTICLE_COUNTER) % k).expr())]
    asset = bh.EffectAsset(capacity, bh.SpawnerSettings.once(float(capacity)), w.finish()).with_motion_integration(bh.MotionIntegration.None_)
    for m in mods:
        asset = asset.init(m)
    return asset
