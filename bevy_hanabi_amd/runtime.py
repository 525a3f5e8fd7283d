"""ctypes binding of the C ABI (include/hanabi_amd.h): the only way Python reaches the GPU path.

There is no CPU fallback here: if libhanabi_amd.so is missing or no HIP device exists the
calls raise HanabiError.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

HNB_OK = 0
HNB_ERR_NO_DEVICE = -4
HNB_ERR_NOT_FOUND = -6

ATTR_COMPONENTS = [1, 1, 3, 3, 1, 1, 1, 4, 1, 1, 2, 3, 1, 1, 3, 3, 3, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 1, 1, 1, 1, 1]
ATTR_IS_FLOAT = [0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0] + [1] * 16 + [0] * 5

# every entry point include/hanabi_amd.h declares
ABI_SYMBOLS = [
    "hnb_last_error", "hnb_version", "hnb_ctx_create", "hnb_ctx_destroy", "hnb_ctx_set_stream", "hnb_ctx_synchronize",
    "hnb_program_create", "hnb_program_destroy", "hnb_program_validate", "hnb_effect_create", "hnb_effect_destroy",
    "hnb_effect_set_parent", "hnb_frame_begin", "hnb_effect_set_frame", "hnb_effect_set_property", "hnb_simulate",
    "hnb_effect_metadata", "hnb_effect_alive_count", "hnb_effect_read_attr", "hnb_effect_read_alive_list",
    "hnb_effect_read_dead_list", "hnb_effect_write_attr", "hnb_effect_sort_ribbons", "hnb_ctx_enable_kernel_timing",
    "hnb_ctx_kernel_timing", "hnb_program_kernel_info", "hnb_jit_precompile", "hnb_effect_set_simulated", "hnb_ctx_set_option", "hnb_program_set_frames", "hnb_effect_index",
    "hnb_ctx_profile_marker", "hnb_program_kernel_timing",
    "hnb_comm_create_local", "hnb_comm_unique_id", "hnb_comm_create_rank", "hnb_comm_allreduce_alive", "hnb_comm_destroy", "hnb_comm_set_library",
    "hnb_effect_device_view", "hnb_effect_materialise", "hnb_jit_precompile_set", "hnb_effect_check", "hnb_effect_compare", "hnb_comm_describe", "hnb_program_device_view",
    "hnb_simulate_steps", "hnb_effect_set_frames_ahead", "hnb_program_set_frames_ahead", "hnb_ctx_step_stats",
    "hnb_program_prepare_steps", "hnb_jit_precompile_steps",
    "hnb_effect_export", "hnb_program_export", "hnb_effect_export_sorted", "hnb_program_export_sorted",
    "hnb_effect_export_filtered", "hnb_effect_export_filtered_sorted", "hnb_program_export_filtered",
    "hnb_effect_bounds", "hnb_program_bounds",
]
# ... and the entry point include/hanabi_amd_binned.h declares
ABI_BINNED_SYMBOLS = ["hnb_effect_export_binned"]
# ... and the one include/hanabi_amd_import.h declares
ABI_IMPORT_SYMBOLS = ["hnb_effect_import"]
# ... and the two include/hanabi_amd_deposit.h declares
ABI_DEPOSIT_SYMBOLS = ["hnb_effect_deposit", "hnb_program_deposit"]
# ... and the one include/hanabi_amd_sample.h declares
ABI_SAMPLE_SYMBOLS = ["hnb_effect_sample"]
# ... and the two include/hanabi_amd_splat.h declares
ABI_SPLAT_SYMBOLS = ["hnb_effect_splat", "hnb_program_splat"]
# ... and the one include/hanabi_amd_sample_program.h declares
ABI_SAMPLE_PROGRAM_SYMBOLS = ["hnb_program_sample"]
# ... and the one include/hanabi_amd_neighbours.h declares
ABI_NEIGHBOUR_SYMBOLS = ["hnb_effect_neighbours"]
# ... and the one include/hanabi_amd_pairs.h declares
ABI_PAIRS_SYMBOLS = ["hnb_effect_pairs"]
# ... and the one include/hanabi_amd_neighbours_from.h declares
ABI_NEIGHBOURS_FROM_SYMBOLS = ["hnb_effect_neighbours_from"]
# ... and the one include/hanabi_amd_pairs_from.h declares
ABI_PAIRS_FROM_SYMBOLS = ["hnb_effect_pairs_from"]

# hnb_ctx_set_option (include/hanabi_amd.h): name -> option id
OPTIONS = {"list_order": 1, "alternate": 2, "skip_lists": 3, "age_cohort": 4, "cull_lifetime": 5, "horizon": 6, "transpose": 7, "scene_merge": 8,
           "suffix_proof": 9, "overlap_updates": 10, "stream_hints": 11, "set_module": 12, "jit_async": 13, "test_break_proof": 15, "ring_lists": 16, "slot_init": 17, "direct_upload": 18, "fuse_steps": 19}
MAX_FUSED_STEPS = 8   # HNB_MAX_FUSED_STEPS
SET_MODULE_OFF, SET_MODULE_CACHED, SET_MODULE_COMPILE, SET_MODULE_BACKGROUND = 0, 1, 2, 3


class HanabiError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"[{code}] {message}")
        self.code = code


class SimParams(C.Structure):
    _fields_ = [("delta_time", C.c_float), ("time", C.c_float), ("virtual_delta_time", C.c_float), ("virtual_time", C.c_float),
                ("real_delta_time", C.c_float), ("real_time", C.c_float)]


class EffectMetadata(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("capacity", "alive_count", "max_update", "max_spawn", "indirect_write_index",
                                          "particle_counter", "instance_count", "dispatch_x", "dead_count", "spawned", "fault",
                                          "reserved")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class StepStats(C.Structure):
    """HnbStepStats (hnb_ctx_step_stats): what the context has submitted since it was created."""
    _fields_ = [(n, C.c_uint64) for n in ("frames", "fused_frames", "fused_launches", "update_launches", "list_launches")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class DeviceMeta(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("alive_count", "particle_counter", "list_column", "max_update", "dead_count", "spawned",
                                          "indirect_write_index", "instance_count")]


class EffectCheck(C.Structure):
    """HnbEffectCheck (hnb_effect_check): the list / alive-byte / lifetime invariants of one effect, evaluated on the device."""
    _fields_ = [(n, C.c_uint32) for n in ("ok", "capacity", "alive_count", "bad_slots", "duplicate_slots", "alive_byte_mismatches", "alive_past_lifetime", "fault")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class EffectDiff(C.Structure):
    """HnbEffectDiff (hnb_effect_compare): two effects of one layout compared bit for bit on the device."""
    _fields_ = [("equal", C.c_uint32), ("counter_diffs", C.c_uint32), ("alive_list_diffs", C.c_uint64), ("dead_list_diffs", C.c_uint64), ("attr_diffs", C.c_uint64),
                ("first_section", C.c_int32), ("reserved", C.c_uint32), ("first_index", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class DeviceAttr(C.Structure):
    _fields_ = [("attr", C.c_uint16), ("ncomp", C.c_uint8), ("scalar_type", C.c_uint8), ("stride_bytes", C.c_uint16), ("reserved", C.c_uint16),
                ("plane", C.c_void_p)]


class DeviceView(C.Structure):
    """HnbDeviceView: device pointers of an effect's planes, lists and metadata row (hnb_effect_device_view)."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("stream", C.c_void_p),
                ("capacity", C.c_uint32), ("slot_base", C.c_uint32), ("n_attrs", C.c_uint32), ("reserved", C.c_uint32),
                ("stale_attr_mask", C.c_uint64), ("alive_list", C.c_void_p * 2), ("dead_list", C.c_void_p),
                ("meta", C.c_void_p), ("meta_next", C.c_void_p), ("attrs", DeviceAttr * 40)]

    def plane(self, attr_id):
        for i in range(self.n_attrs):
            if self.attrs[i].attr == int(attr_id):
                return self.attrs[i]
        raise KeyError(attr_id)


class ProgramAttr(C.Structure):
    _fields_ = [("attr", C.c_uint16), ("ncomp", C.c_uint8), ("scalar_type", C.c_uint8), ("stride_bytes", C.c_uint16), ("reserved", C.c_uint16),
                ("plane_off", C.c_uint64)]


class ProgramView(C.Structure):
    """HnbProgramView: every instance of a program behind one device-resident table (hnb_program_device_view)."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("stream", C.c_void_p),
                ("capacity", C.c_uint32), ("n_instances", C.c_uint32), ("n_attrs", C.c_uint32), ("reserved", C.c_uint32),
                ("stale_attr_mask", C.c_uint64), ("slabs", C.c_void_p), ("meta", C.c_void_p), ("meta_next", C.c_void_p),
                ("alive_list_off", C.c_uint64 * 2), ("dead_list_off", C.c_uint64), ("attrs", ProgramAttr * 40)]


EXPORT_MAX_FIELDS = 16   # HNB_EXPORT_MAX_FIELDS


class ExportField(C.Structure):
    """HnbExportField: attribute `attr` goes to byte `dst_offset` of every record."""
    _fields_ = [("attr", C.c_uint16), ("reserved", C.c_uint16), ("dst_offset", C.c_uint32)]


class ExportDesc(C.Structure):
    """HnbExportDesc (hnb_effect_export / hnb_program_export): the record layout and the device buffers of a packed export."""
    _fields_ = [("struct_size", C.c_uint32), ("n_fields", C.c_uint32), ("record_stride", C.c_uint32), ("flags", C.c_uint32),
                ("dst", C.c_void_p), ("dst_capacity_records", C.c_uint64), ("out_count", C.c_void_p), ("fields", ExportField * EXPORT_MAX_FIELDS)]


def export_desc(fields, dst_ptr, stride, capacity_records, count_ptr=None):
    """fields: (attribute id, byte offset) pairs, or ExportField objects -> ExportDesc. More than EXPORT_MAX_FIELDS fields keep their count:
    the library refuses them."""
    d = ExportDesc()
    d.struct_size = C.sizeof(ExportDesc)
    fields = list(fields)
    d.n_fields = len(fields)
    for i, f in enumerate(fields[:EXPORT_MAX_FIELDS]):
        d.fields[i] = f if isinstance(f, ExportField) else ExportField(int(f[0]), 0, int(f[1]))
    d.record_stride = int(stride)
    d.dst = C.c_void_p(int(dst_ptr))
    d.dst_capacity_records = int(capacity_records)
    d.out_count = C.c_void_p(int(count_ptr)) if count_ptr else None
    return d


IMPORT_ROWS, IMPORT_IDS = 0, 1   # HNB_IMPORT_*
IMPORT_MODES = {"rows": IMPORT_ROWS, "ids": IMPORT_IDS}


class ImportDesc(C.Structure):
    """HnbImportDesc (hnb_effect_import): the record layout and the device buffers of a packed input. `fields` are the exports' ExportField: a
    field's dst_offset is its byte offset in the source record."""
    _fields_ = [("struct_size", C.c_uint32), ("n_fields", C.c_uint32), ("record_stride", C.c_uint32), ("mode", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32), ("src", C.c_void_p), ("src_capacity_records", C.c_uint64), ("src_count", C.c_void_p), ("out_count", C.c_void_p),
                ("fields", ExportField * EXPORT_MAX_FIELDS)]


def import_desc(fields, src_ptr, stride, capacity_records, mode=IMPORT_ROWS, src_count_ptr=None, out_count_ptr=None):
    """fields: (attribute id, byte offset) pairs, or ExportField objects; mode: IMPORT_ROWS / IMPORT_IDS or "rows" / "ids" -> ImportDesc. More than
    EXPORT_MAX_FIELDS fields keep their count: the library refuses them."""
    d = ImportDesc()
    d.struct_size = C.sizeof(ImportDesc)
    fields = list(fields)
    d.n_fields = len(fields)
    for i, f in enumerate(fields[:EXPORT_MAX_FIELDS]):
        d.fields[i] = f if isinstance(f, ExportField) else ExportField(int(f[0]), 0, int(f[1]))
    d.record_stride = int(stride)
    d.mode = IMPORT_MODES[mode] if isinstance(mode, str) else int(mode)
    d.src = C.c_void_p(int(src_ptr)) if src_ptr else None
    d.src_capacity_records = int(capacity_records)
    d.src_count = C.c_void_p(int(src_count_ptr)) if src_count_ptr else None
    d.out_count = C.c_void_p(int(out_count_ptr)) if out_count_ptr else None
    return d


SORT_KEY_DEPTH, SORT_KEY_DISTANCE, SORT_KEY_ATTR = 0, 1, 2   # HNB_SORT_KEY_*
SORT_SCOPE_INSTANCE, SORT_SCOPE_PROGRAM = 0, 1              # HNB_SORT_SCOPE_*
SORT_SCOPES = {"instance": SORT_SCOPE_INSTANCE, "program": SORT_SCOPE_PROGRAM}
SORT_KEYS = {"depth": SORT_KEY_DEPTH, "distance": SORT_KEY_DISTANCE, "attr": SORT_KEY_ATTR}


class ExportSort(C.Structure):
    """HnbExportSort (hnb_effect_export_sorted): the key the records are ordered by."""
    _fields_ = [("struct_size", C.c_uint32), ("key", C.c_uint32), ("attr", C.c_uint32), ("descending", C.c_uint32), ("v", C.c_float * 3), ("reserved", C.c_uint32)]


def export_sort(key, v=(0, 0, 0), attr=0, descending=False):
    """key: "depth" | "distance" | "attr" or a HNB_SORT_KEY_* value -> ExportSort."""
    s = ExportSort()
    s.struct_size = C.sizeof(ExportSort)
    s.key = SORT_KEYS[key] if isinstance(key, str) else int(key)
    s.attr = int(attr)
    s.descending = int(descending)
    s.v = (C.c_float * 3)(*[float(x) for x in v])
    return s


FILTER_PLANES, FILTER_SPHERE, FILTER_ATTR_RANGE = 0, 1, 2   # HNB_FILTER_*
FILTER_MAX_PLANES = 6                                        # HNB_FILTER_MAX_PLANES
FILTER_KINDS = {"planes": FILTER_PLANES, "sphere": FILTER_SPHERE, "attr_range": FILTER_ATTR_RANGE}


class ExportFilter(C.Structure):
    """HnbExportFilter (hnb_effect_export_filtered): the predicate in front of the export."""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_uint32), ("n_planes", C.c_uint32), ("attr", C.c_uint32), ("invert", C.c_uint32),
                ("lo_bits", C.c_uint32), ("hi_bits", C.c_uint32), ("reserved", C.c_uint32), ("P", (C.c_float * 4) * FILTER_MAX_PLANES)]


def _scalar_bits(x):
    """A bound of an attribute range as the 32 bits the library compares: a Python float as binary32, an int as it is."""
    if isinstance(x, (float, np.floating)):
        return int(np.array([x], np.float32).view(np.uint32)[0])
    return int(x) & 0xFFFFFFFF


def export_filter(kind, planes=(), sphere=None, attr=0, lo=0, hi=0, invert=False):
    """kind: "planes" | "sphere" | "attr_range" or a HNB_FILTER_* value -> ExportFilter. planes: up to six (a, b, c, d); sphere: (cx, cy, cz, squared
    radius); lo / hi: floats (taken as binary32) or ints (taken as bit patterns). More than six planes keep their count: the library refuses them."""
    f = ExportFilter()
    f.struct_size = C.sizeof(ExportFilter)
    f.kind = FILTER_KINDS[kind] if isinstance(kind, str) else int(kind)
    rows = [tuple(r) for r in planes]
    f.n_planes = len(rows)
    if sphere is not None:
        rows = [tuple(sphere)] + rows[1:]
    for i, r in enumerate(rows[:FILTER_MAX_PLANES]):
        f.P[i] = (C.c_float * 4)(*[float(x) for x in r])
    f.attr = int(attr)
    f.lo_bits, f.hi_bits = _scalar_bits(lo), _scalar_bits(hi)
    f.invert = int(invert)
    return f


class ExportSortFiltered(C.Structure):
    """HnbExportSortFiltered: the 48-byte form of the sort descriptor - an ExportSort whose struct_size is this struct's, and the host array of
    filters in front of the sort. Passed where an ExportSort is (export_sort_filtered)."""
    _fields_ = [("sort", ExportSort), ("filters", C.c_void_p), ("n_filters", C.c_uint32), ("reserved2", C.c_uint32)]


def export_sort_filtered(sort, filters):
    """sort: an ExportSort or a dict of export_sort's keywords; filters: a sequence of ExportFilter or dicts of export_filter's keywords
    -> (ExportSortFiltered, the ctypes array it points to: keep it alive for as long as the descriptor is used)."""
    arr = (ExportFilter * max(len(filters), 1))(*[f if isinstance(f, ExportFilter) else export_filter(**f) for f in filters])
    sf = ExportSortFiltered()
    s = sort if isinstance(sort, ExportSort) else export_sort(**sort)
    C.memmove(C.byref(sf.sort), C.byref(s), C.sizeof(ExportSort))
    sf.sort.struct_size = C.sizeof(ExportSortFiltered)
    sf.filters = C.cast(arr, C.c_void_p)
    sf.n_filters = len(filters)
    return sf, arr


BIN_MAX_CELLS = 1 << 24   # HNB_BIN_MAX_CELLS


class ExportBins(C.Structure):
    """HnbExportBins (hnb_effect_export_binned): the uniform grid the records are ordered by, and the device table of the cells' first records."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("dims", C.c_uint32 * 3), ("reserved", C.c_uint32), ("origin", C.c_float * 3),
                ("inv_cell", C.c_float * 3), ("cell_start", C.c_void_p)]


def export_bins(dims, origin, inv_cell, cell_start_ptr):
    """dims: cells along x, y, z; origin: the grid's lowest corner; inv_cell: 1 / cell edge per axis (floats, taken as binary32); cell_start_ptr:
    the device address of dims[0] * dims[1] * dims[2] + 2 words -> ExportBins."""
    g = ExportBins()
    g.struct_size = C.sizeof(ExportBins)
    g.dims = (C.c_uint32 * 3)(*[int(x) for x in dims])
    g.origin = (C.c_float * 3)(*[float(x) for x in origin])
    g.inv_cell = (C.c_float * 3)(*[float(x) for x in inv_cell])
    g.cell_start = C.c_void_p(int(cell_start_ptr)) if cell_start_ptr else None
    return g


class Bounds(C.Structure):
    """HnbBounds (hnb_effect_bounds / hnb_program_bounds): one 48-byte record as the device writes it."""
    _fields_ = [("lo", C.c_float * 4), ("hi", C.c_float * 4), ("alive", C.c_uint32), ("nan", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class BoundsDesc(C.Structure):
    """HnbBoundsDesc: the attribute whose bounds are taken and the device buffer of the records."""
    _fields_ = [("struct_size", C.c_uint32), ("attr", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32), ("dst", C.c_void_p),
                ("dst_capacity_records", C.c_uint64)]


def bounds_desc(attr, dst_ptr, capacity_records):
    d = BoundsDesc()
    d.struct_size = C.sizeof(BoundsDesc)
    d.attr = int(attr)
    d.dst = int(dst_ptr) if dst_ptr else None
    d.dst_capacity_records = int(capacity_records)
    return d


DEPOSIT_MAX_CHANNELS = 4     # HNB_DEPOSIT_MAX_CHANNELS
DEPOSIT_ACCUMULATE = 0x1     # HNB_DEPOSIT_ACCUMULATE
SPLAT_ATTR_ONE = 0xFFFFFFFF  # HNB_SPLAT_ATTR_ONE: a channel of hnb_effect_splat / hnb_program_splat whose value is 1.0f for every particle


class DepositChannel(C.Structure):
    """HnbDepositChannel: component `comp` of the f32 attribute `attr`, summed in units of 2^-frac_bits."""
    _fields_ = [("attr", C.c_uint32), ("comp", C.c_uint32), ("frac_bits", C.c_uint32), ("reserved", C.c_uint32)]


class DepositDesc(C.Structure):
    """HnbDepositDesc (hnb_effect_deposit / hnb_program_deposit): the uniform grid, the channels and the device buffers of a deposit."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("dims", C.c_uint32 * 3), ("n_channels", C.c_uint32), ("origin", C.c_float * 3),
                ("inv_cell", C.c_float * 3), ("channels", DepositChannel * DEPOSIT_MAX_CHANNELS), ("count", C.c_void_p), ("sums", C.c_void_p), ("out_stats", C.c_void_p)]


def deposit_desc(dims, origin, inv_cell, count_ptr, channels=(), sums_ptr=None, stats_ptr=None, accumulate=False):
    """dims, origin, inv_cell: export_bins' grid; channels: (attribute id, component, frac_bits) triples or DepositChannel objects; count_ptr:
    the device address of n_cells + 1 u32; sums_ptr: of (n_cells + 1) * len(channels) i64 (None without channels); stats_ptr: of 4 u32 or None
    -> DepositDesc. More than DEPOSIT_MAX_CHANNELS channels keep their count: the library refuses them."""
    d = DepositDesc()
    d.struct_size = C.sizeof(DepositDesc)
    d.flags = DEPOSIT_ACCUMULATE if accumulate else 0
    d.dims = (C.c_uint32 * 3)(*[int(x) for x in dims])
    d.origin = (C.c_float * 3)(*[float(x) for x in origin])
    d.inv_cell = (C.c_float * 3)(*[float(x) for x in inv_cell])
    channels = list(channels)
    d.n_channels = len(channels)
    for i, ch in enumerate(channels[:DEPOSIT_MAX_CHANNELS]):
        d.channels[i] = ch if isinstance(ch, DepositChannel) else DepositChannel(int(ch[0]), int(ch[1]), int(ch[2]), 0)
    d.count = C.c_void_p(int(count_ptr)) if count_ptr else None
    d.sums = C.c_void_p(int(sums_ptr)) if sums_ptr else None
    d.out_stats = C.c_void_p(int(stats_ptr)) if stats_ptr else None
    return d


SAMPLE_MAX_CHANNELS = 4               # HNB_SAMPLE_MAX_CHANNELS
SAMPLE_NEAREST, SAMPLE_TRILINEAR = 0, 1   # HNB_SAMPLE_NEAREST, HNB_SAMPLE_TRILINEAR
SAMPLE_SET, SAMPLE_ADD = 0, 1         # HNB_SAMPLE_SET, HNB_SAMPLE_ADD


class SampleChannel(C.Structure):
    """HnbSampleChannel: a channel of the field goes into component `comp` of the f32 attribute `attr`, stored (SAMPLE_SET) or added (SAMPLE_ADD)."""
    _fields_ = [("attr", C.c_uint32), ("comp", C.c_uint32), ("op", C.c_uint32), ("reserved", C.c_uint32)]


class SampleDesc(C.Structure):
    """HnbSampleDesc (hnb_effect_sample): the uniform grid, the mode, the scale, the destinations and the device field of a sample."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("dims", C.c_uint32 * 3), ("n_channels", C.c_uint32), ("origin", C.c_float * 3),
                ("inv_cell", C.c_float * 3), ("mode", C.c_uint32), ("scale", C.c_float), ("channels", SampleChannel * SAMPLE_MAX_CHANNELS), ("field", C.c_void_p),
                ("out_stats", C.c_void_p)]


def sample_desc(dims, origin, inv_cell, field_ptr, channels, mode=SAMPLE_TRILINEAR, scale=1.0, stats_ptr=None):
    """dims, origin, inv_cell: export_bins' grid; field_ptr: the device address of n_cells * len(channels) f32, channel-minor; channels: per channel
    of the field an (attribute id, component, op) triple or a SampleChannel; stats_ptr: the device address of 4 u32 or None -> SampleDesc. More than
    SAMPLE_MAX_CHANNELS channels keep their count: the library refuses them."""
    d = SampleDesc()
    d.struct_size = C.sizeof(SampleDesc)
    d.flags = 0
    d.dims = (C.c_uint32 * 3)(*[int(x) for x in dims])
    d.origin = (C.c_float * 3)(*[float(x) for x in origin])
    d.inv_cell = (C.c_float * 3)(*[float(x) for x in inv_cell])
    d.mode = int(mode)
    d.scale = float(scale)
    channels = list(channels)
    d.n_channels = len(channels)
    for i, ch in enumerate(channels[:SAMPLE_MAX_CHANNELS]):
        d.channels[i] = ch if isinstance(ch, SampleChannel) else SampleChannel(int(ch[0]), int(ch[1]), int(ch[2]), 0)
    d.field = C.c_void_p(int(field_ptr)) if field_ptr else None
    d.out_stats = C.c_void_p(int(stats_ptr)) if stats_ptr else None
    return d


PROGRAM_SAMPLE_MAX_INSTANCES = 65535   # HNB_PROGRAM_SAMPLE_MAX_INSTANCES


class ProgramSampleDesc(C.Structure):
    """HnbProgramSampleDesc (hnb_program_sample): hnb_effect_sample's description, the stride from an instance's field to the next one's and the
    per-instance stats."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("sample", SampleDesc), ("field_instance_stride", C.c_uint64), ("out_instance_stats", C.c_void_p),
                ("reserved", C.c_uint64)]


def program_sample_desc(dims, origin, inv_cell, field_ptr, channels, mode=SAMPLE_TRILINEAR, scale=1.0, stats_ptr=None, field_instance_stride=0, instance_stats_ptr=None):
    """sample_desc's arguments - field_ptr: instance 0's field; stats_ptr: the totals - and field_instance_stride: f32 elements from an instance's field
    to the next one's (0: one field for all); instance_stats_ptr: the device address of n_instances * 4 u32 or None -> ProgramSampleDesc"""
    d = ProgramSampleDesc()
    d.struct_size = C.sizeof(ProgramSampleDesc)
    d.flags = 0
    d.sample = sample_desc(dims, origin, inv_cell, field_ptr, channels, mode, scale, stats_ptr)
    d.field_instance_stride = int(field_instance_stride)
    d.out_instance_stats = C.c_void_p(int(instance_stats_ptr)) if instance_stats_ptr else None
    d.reserved = 0
    return d


NEIGHBOUR_MAX_CHANNELS = 4            # HNB_NEIGHBOUR_MAX_CHANNELS
NEIGHBOUR_MAX_CANDIDATES = 65536      # HNB_NEIGHBOUR_MAX_CANDIDATES
NEIGHBOUR_W_ONE, NEIGHBOUR_W_U1, NEIGHBOUR_W_U2, NEIGHBOUR_W_U3 = 0, 1, 2, 3   # HNB_NEIGHBOUR_W_*
NEIGHBOUR_DIFF = 0x1                  # HNB_NEIGHBOUR_DIFF


class NeighbourChannel(C.Structure):
    """HnbNeighbourChannel: the neighbours' `src_comp` of the f32 attribute `src_attr` (or SPLAT_ATTR_ONE), minus the particle's own with
    NEIGHBOUR_DIFF, weighted and summed in units of 2^-frac_bits, goes into component `dst_comp` of `dst_attr`, stored (SAMPLE_SET) or added."""
    _fields_ = [("src_attr", C.c_uint32), ("src_comp", C.c_uint32), ("flags", C.c_uint32), ("frac_bits", C.c_uint32), ("dst_attr", C.c_uint32), ("dst_comp", C.c_uint32),
                ("op", C.c_uint32), ("reserved", C.c_uint32)]


class NeighbourDesc(C.Structure):
    """HnbNeighbourDesc (hnb_effect_neighbours): the uniform grid, the radius, the weight, the crowding limit, the scale and the channels."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("dims", C.c_uint32 * 3), ("n_channels", C.c_uint32), ("origin", C.c_float * 3),
                ("inv_cell", C.c_float * 3), ("radius", C.c_float), ("scale", C.c_float), ("weight", C.c_uint32), ("candidate_limit", C.c_uint32),
                ("channels", NeighbourChannel * NEIGHBOUR_MAX_CHANNELS), ("out_stats", C.c_void_p)]


def neighbour_desc(dims, origin, inv_cell, radius, channels, weight=NEIGHBOUR_W_ONE, candidate_limit=4096, scale=1.0, stats_ptr=None):
    """dims, origin, inv_cell: export_bins' grid; channels: per channel a (src attribute id, src component, flags, frac_bits, dst attribute id, dst
    component, op) tuple or a NeighbourChannel; stats_ptr: the device address of 8 u32 or None -> NeighbourDesc. More than NEIGHBOUR_MAX_CHANNELS
    channels keep their count: the library refuses them."""
    d = NeighbourDesc()
    d.struct_size = C.sizeof(NeighbourDesc)
    d.flags = 0
    d.dims = (C.c_uint32 * 3)(*[int(x) for x in dims])
    d.origin = (C.c_float * 3)(*[float(x) for x in origin])
    d.inv_cell = (C.c_float * 3)(*[float(x) for x in inv_cell])
    d.radius = float(radius)
    d.scale = float(scale)
    d.weight = int(weight)
    d.candidate_limit = int(candidate_limit)
    channels = list(channels)
    d.n_channels = len(channels)
    for i, ch in enumerate(channels[:NEIGHBOUR_MAX_CHANNELS]):
        d.channels[i] = ch if isinstance(ch, NeighbourChannel) else NeighbourChannel(*[int(x) for x in ch], 0)
    d.out_stats = C.c_void_p(int(stats_ptr)) if stats_ptr else None
    return d


PAIRS_HALF = 0x1                      # HNB_PAIRS_HALF
PAIRS_NO_ROW = 0xFFFFFFFF             # HNB_PAIRS_NO_ROW


class PairsDesc(C.Structure):
    """HnbPairsDesc (hnb_effect_pairs): the uniform grid, the radius, the crowding limit and the CSR destinations."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("dims", C.c_uint32 * 3), ("candidate_limit", C.c_uint32), ("origin", C.c_float * 3),
                ("inv_cell", C.c_float * 3), ("radius", C.c_float), ("pair_capacity", C.c_uint32), ("out_rows", C.c_void_p), ("out_start", C.c_void_p),
                ("out_pairs", C.c_void_p), ("out_d2", C.c_void_p), ("out_stats", C.c_void_p)]


def pairs_desc(dims, origin, inv_cell, radius, rows_ptr, start_ptr, pairs_ptr=None, pair_capacity=0, d2_ptr=None, stats_ptr=None, candidate_limit=4096, half=False):
    """dims, origin, inv_cell: export_bins' grid; rows_ptr: the device address of capacity u32, start_ptr: of capacity + 1 u32, pairs_ptr / d2_ptr:
    of pair_capacity u32 / f32 or None, stats_ptr: of 8 u32 or None -> PairsDesc"""
    d = PairsDesc()
    d.struct_size = C.sizeof(PairsDesc)
    d.flags = PAIRS_HALF if half else 0
    d.dims = (C.c_uint32 * 3)(*[int(x) for x in dims])
    d.candidate_limit = int(candidate_limit)
    d.origin = (C.c_float * 3)(*[float(x) for x in origin])
    d.inv_cell = (C.c_float * 3)(*[float(x) for x in inv_cell])
    d.radius = float(radius)
    d.pair_capacity = int(pair_capacity)
    for name, ptr in (("out_rows", rows_ptr), ("out_start", start_ptr), ("out_pairs", pairs_ptr), ("out_d2", d2_ptr), ("out_stats", stats_ptr)):
        setattr(d, name, C.c_void_p(int(ptr)) if ptr else None)
    return d


_lib = None


def load_library():
    """Load libhanabi_amd.so (in-tree). Raises if it has not been built."""
    global _lib
    if _lib is None:
        path = os.environ.get("HNB_LIB") or _build.runtime_lib_path()  # HNB_LIB: kernel-variant A/B runs
        if not os.path.exists(path):
            raise HanabiError(-1, f"{path} not found: run `python -m bevy_hanabi_amd.build` (needs hipcc)")
        lib = C.CDLL(path)
        lib.hnb_last_error.restype = C.c_char_p
        lib.hnb_version.restype = C.c_char_p
        lib.hnb_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.hnb_ctx_destroy.argtypes = [C.c_void_p]
        lib.hnb_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        lib.hnb_ctx_synchronize.argtypes = [C.c_void_p]
        lib.hnb_program_create.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
        lib.hnb_program_destroy.argtypes = [C.c_void_p]
        lib.hnb_program_validate.argtypes = [C.c_char_p, C.c_size_t]
        lib.hnb_effect_create.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        lib.hnb_effect_destroy.argtypes = [C.c_void_p]
        lib.hnb_effect_set_parent.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.hnb_frame_begin.argtypes = [C.c_void_p, C.POINTER(SimParams)]
        lib.hnb_effect_set_frame.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.hnb_effect_set_property.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint32]
        lib.hnb_simulate.argtypes = [C.c_void_p]
        lib.hnb_effect_metadata.argtypes = [C.c_void_p, C.POINTER(EffectMetadata)]
        lib.hnb_effect_alive_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        lib.hnb_effect_read_attr.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
        lib.hnb_effect_write_attr.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
        lib.hnb_effect_read_alive_list.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.hnb_effect_read_dead_list.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.hnb_effect_sort_ribbons.argtypes = [C.c_void_p]
        lib.hnb_ctx_enable_kernel_timing.argtypes = [C.c_void_p, C.c_int]
        lib.hnb_ctx_kernel_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        lib.hnb_effect_set_simulated.argtypes = [C.c_void_p, C.c_int]
        lib.hnb_ctx_set_option.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        lib.hnb_program_set_frames.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hnb_effect_index.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        lib.hnb_ctx_profile_marker.argtypes = [C.c_void_p, C.c_uint32]
        lib.hnb_program_kernel_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        lib.hnb_comm_create_local.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p)]
        lib.hnb_comm_unique_id.argtypes = [C.c_void_p]
        lib.hnb_comm_create_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        lib.hnb_comm_allreduce_alive.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_uint64)]
        lib.hnb_comm_destroy.argtypes = [C.c_void_p]
        lib.hnb_comm_set_library.argtypes = [C.c_char_p, C.c_uint32]
        lib.hnb_program_device_view.argtypes = [C.c_void_p, C.POINTER(ProgramView)]
        lib.hnb_comm_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        lib.hnb_effect_check.argtypes = [C.c_void_p, C.POINTER(EffectCheck)]
        lib.hnb_effect_compare.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(EffectDiff)]
        lib.hnb_effect_device_view.argtypes = [C.c_void_p, C.POINTER(DeviceView)]
        lib.hnb_effect_materialise.argtypes = [C.c_void_p, C.c_uint64]
        lib.hnb_program_kernel_info.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        lib.hnb_jit_precompile.argtypes = [C.c_char_p, C.c_size_t]
        lib.hnb_jit_precompile_set.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_uint32]
        lib.hnb_simulate_steps.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(SimParams)]
        lib.hnb_effect_set_frames_ahead.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hnb_program_set_frames_ahead.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hnb_ctx_step_stats.argtypes = [C.c_void_p, C.POINTER(StepStats)]
        lib.hnb_program_prepare_steps.argtypes = [C.c_void_p]
        lib.hnb_jit_precompile_steps.argtypes = [C.c_char_p, C.c_size_t]
        lib.hnb_effect_export.argtypes = [C.c_void_p, C.POINTER(ExportDesc)]
        lib.hnb_program_export.argtypes = [C.c_void_p, C.POINTER(ExportDesc), C.c_void_p]
        lib.hnb_effect_export_sorted.argtypes = [C.c_void_p, C.POINTER(ExportDesc), C.POINTER(ExportSort)]
        lib.hnb_program_export_sorted.argtypes = [C.c_void_p, C.POINTER(ExportDesc), C.POINTER(ExportSort), C.c_uint32, C.c_void_p]
        lib.hnb_effect_export_filtered.argtypes = [C.c_void_p, C.POINTER(ExportDesc), C.POINTER(ExportFilter)]
        lib.hnb_effect_export_filtered_sorted.argtypes = [C.c_void_p, C.POINTER(ExportDesc), C.POINTER(ExportFilter), C.POINTER(ExportSort)]
        lib.hnb_program_export_filtered.argtypes = [C.c_void_p, C.POINTER(ExportDesc), C.POINTER(ExportFilter), C.c_uint32, C.c_void_p]
        lib.hnb_effect_bounds.argtypes = [C.c_void_p, C.POINTER(BoundsDesc)]
        lib.hnb_program_bounds.argtypes = [C.c_void_p, C.POINTER(BoundsDesc)]
        lib.hnb_effect_export_binned.argtypes = [C.c_void_p, C.POINTER(ExportDesc), C.POINTER(ExportBins)]
        lib.hnb_effect_import.argtypes = [C.c_void_p, C.POINTER(ImportDesc)]
        lib.hnb_effect_deposit.argtypes = [C.c_void_p, C.POINTER(DepositDesc)]
        lib.hnb_program_deposit.argtypes = [C.c_void_p, C.POINTER(DepositDesc)]
        lib.hnb_effect_sample.argtypes = [C.c_void_p, C.POINTER(SampleDesc)]
        lib.hnb_effect_splat.argtypes = [C.c_void_p, C.POINTER(DepositDesc)]
        lib.hnb_program_splat.argtypes = [C.c_void_p, C.POINTER(DepositDesc)]
        lib.hnb_program_sample.argtypes = [C.c_void_p, C.POINTER(ProgramSampleDesc)]
        lib.hnb_effect_neighbours.argtypes = [C.c_void_p, C.POINTER(NeighbourDesc)]
        lib.hnb_effect_pairs.argtypes = [C.c_void_p, C.POINTER(PairsDesc)]
        lib.hnb_effect_neighbours_from.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(NeighbourDesc)]
        lib.hnb_effect_pairs_from.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PairsDesc)]
        _lib = lib
    return _lib


def _check(rc):
    if rc != HNB_OK:
        raise HanabiError(rc, load_library().hnb_last_error().decode())


def validate_program(blob: bytes):
    """Structural validation of a program blob; works without a GPU."""
    _check(load_library().hnb_program_validate(blob, len(blob)))


def jit_precompile(blob: bytes):
    """Compile and cache the kernels specialised for this program (hiprtc; needs no GPU)."""
    _check(load_library().hnb_jit_precompile(blob, len(blob)))


def jit_precompile_steps(blob: bytes):
    """Compile and cache the steps kernel of this program (the several-frames form of a streaming update specialised at run time:
    Program.prepare_steps; needs no GPU). Writes nothing for a program without such an update."""
    _check(load_library().hnb_jit_precompile_steps(blob, len(blob)))


def jit_precompile_set(blobs):
    """Compile and cache the set module of these programs (HNB_OPT_SET_MODULE: the specialised code of the small programs of a context behind
    their shared launches; needs no GPU). Order and duplicates do not matter."""
    blobs = list(blobs)
    arr = (C.c_char_p * len(blobs))(*blobs)
    sizes = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
    _check(load_library().hnb_jit_precompile_set(arr, sizes, len(blobs)))


class Context:
    """One simulation context per GPU (`hnb_ctx_*`)."""

    def __init__(self, device_id=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        _check(self._lib.hnb_ctx_create(device_id, C.byref(self._h)))
        self._programs = []
        # A/B harness convenience (tools/, bench.py): HNB_CTX_OPTIONS="age_cohort=0,horizon=0" is applied to every context THIS BINDING creates.
        # The library itself reads no environment variable for its options (include/hanabi_amd.h, hnb_ctx_set_option).
        for kv in filter(None, os.environ.get("HNB_CTX_OPTIONS", "").split(",")):
            k, v = kv.split("=")
            self.set_option(k.strip(), int(v))

    def close(self):
        if self._h:
            for p in list(self._programs):
                p._h = None
                for e in p._effects:
                    e._h = None
            self._lib.hnb_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        _check(self._lib.hnb_ctx_set_stream(self._h, C.c_void_p(hip_stream)))

    def synchronize(self):
        _check(self._lib.hnb_ctx_synchronize(self._h))

    def set_list_order(self, order):
        """'spawn' (default: the serial-thread order) or 'slot' (lists kept in increasing slot order; programs created afterwards)."""
        _check(self._lib.hnb_ctx_set_option(self._h, 1, {"spawn": 0, "slot": 1}[order]))

    def set_option(self, option, value):
        """hnb_ctx_set_option by id or by name (OPTIONS): "age_cohort" (0 off / 1 lean stacks / 2 all; fixed in a program at creation; the one
        option that changes device-visible state: the AGE plane), "cull_lifetime", "horizon", "alternate", "skip_lists", "transpose",
        "scene_merge", "suffix_proof" (scheduling choices; results do not change)."""
        _check(self._lib.hnb_ctx_set_option(self._h, OPTIONS[option] if isinstance(option, str) else int(option), int(value)))

    def create_program(self, blob: bytes):
        return Program(self, blob)

    def frame_begin(self, dt, time=0.0, virtual_dt=None, virtual_time=None, real_dt=None, real_time=None):
        sp = SimParams(dt, time, dt if virtual_dt is None else virtual_dt, time if virtual_time is None else virtual_time,
                       dt if real_dt is None else real_dt, time if real_time is None else real_time)
        _check(self._lib.hnb_frame_begin(self._h, C.byref(sp)))

    def simulate(self):
        _check(self._lib.hnb_simulate(self._h))

    def simulate_steps(self, params_list):
        """hnb_simulate_steps: one frame per element, in one call. An element is a SimParams, a delta time, or a tuple of
        frame_begin's arguments (dt, time, ...). Per-effect inputs of the steps: Effect / Program.set_frames_ahead before the call."""
        steps = []
        for e in params_list:
            if isinstance(e, SimParams):
                steps.append(e)
                continue
            a = tuple(e) if isinstance(e, (tuple, list)) else (e,)
            dt, time = a[0], (a[1] if len(a) > 1 else 0.0)
            rest = list(a[2:]) + [None] * (6 - len(a))
            steps.append(SimParams(dt, time, dt if rest[0] is None else rest[0], time if rest[1] is None else rest[1],
                                   dt if rest[2] is None else rest[2], time if rest[3] is None else rest[3]))
        arr = (SimParams * max(len(steps), 1))(*steps)
        _check(self._lib.hnb_simulate_steps(self._h, len(steps), arr))

    def step_stats(self):
        """hnb_ctx_step_stats: frames, fused_frames, fused_launches, update_launches, list_launches since the context was created."""
        s = StepStats()
        _check(self._lib.hnb_ctx_step_stats(self._h, C.byref(s)))
        return s.as_dict()

    def enable_kernel_timing(self, every_n_frames=1):
        """0/False = off; n = bracket the kernels of every n-th simulated frame with HIP events."""
        _check(self._lib.hnb_ctx_enable_kernel_timing(self._h, int(every_n_frames)))

    def profile_marker(self, tag):
        """An empty kernel with `tag` workgroups on the simulation stream: a visible cut in rocprofv3's dispatch list."""
        _check(self._lib.hnb_ctx_profile_marker(self._h, int(tag)))

    def kernel_timing(self):
        u, c, i, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint32()
        _check(self._lib.hnb_ctx_kernel_timing(self._h, C.byref(u), C.byref(c), C.byref(i), C.byref(n)))
        return {"update_ms_avg": u.value, "compact_ms_avg": c.value, "init_ms_avg": i.value, "frames": n.value}


def comm_set_library(path, duplicate_devices=False, single_rank=False):
    """hnb_comm_set_library: which collective library hnb_comm_* binds; before the first Comm of the process.
    single_rank: a communicator of one context / one rank goes through the library too (HNB_COMM_LIB_SINGLE_RANK)."""
    _check(load_library().hnb_comm_set_library(None if path is None else os.fsencode(path), (1 if duplicate_devices else 0) | (2 if single_rank else 0)))


class Comm:
    """The alive-counter all-reduce over RCCL (`hnb_comm_*`): `Comm.local(contexts)` for one process with a context per GPU,
    `Comm.rank(ctx, unique_id, rank, n_ranks)` for one rank per process (`Comm.unique_id()` on rank 0)."""

    def __init__(self, handle, contexts):
        self._lib = load_library()
        self._h = handle
        self._contexts = list(contexts)

    @classmethod
    def local(cls, contexts):
        lib = load_library()
        arr = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
        h = C.c_void_p()
        _check(lib.hnb_comm_create_local(arr, len(contexts), C.byref(h)))
        return cls(h, contexts)

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _check(load_library().hnb_comm_unique_id(buf))
        return buf.raw

    @classmethod
    def rank(cls, ctx, unique_id, rank, n_ranks):
        lib = load_library()
        h = C.c_void_p()
        _check(lib.hnb_comm_create_rank(ctx._h, C.c_char_p(unique_id), int(rank), int(n_ranks), C.byref(h)))
        return cls(h, [ctx])

    def allreduce_alive(self, effects_per_context):
        """effects_per_context: one list of effects (or None) per local context, all of the same length -> totals per effect."""
        n = len(effects_per_context[0])
        assert len(effects_per_context) == len(self._contexts) and all(len(e) == n for e in effects_per_context)
        flat = [None if fx is None else fx._h for row in effects_per_context for fx in row]
        arr = (C.c_void_p * len(flat))(*flat)
        out = (C.c_uint64 * n)()
        _check(self._lib.hnb_comm_allreduce_alive(self._h, arr, n, out))
        return [int(v) for v in out]

    def describe(self):
        """hnb_comm_describe: 'rccl <resolved library path> ranks=N local=M' or 'host-sum ranks=N local=M'."""
        buf = C.create_string_buffer(1024)
        _check(self._lib.hnb_comm_describe(self._h, buf, len(buf)))
        return buf.value.decode()

    def destroy(self):
        if self._h:
            self._lib.hnb_comm_destroy(self._h)
            self._h = None


class Program:
    def __init__(self, ctx: Context, blob: bytes):
        self._ctx = ctx
        self._lib = ctx._lib
        self._h = C.c_void_p()
        _check(self._lib.hnb_program_create(ctx._h, blob, len(blob), C.byref(self._h)))
        self._effects = []
        ctx._programs.append(self)

    def create_effect(self, slot_base=0):
        return Effect(self, slot_base)

    def set_frames(self, spawn_counts, seeds, transforms=None, first=0):
        """Per-frame inputs of instances [first, first + n) in one call (creation order)."""
        sc = np.ascontiguousarray(spawn_counts, dtype=np.uint32)
        sd = np.ascontiguousarray(seeds, dtype=np.uint32)
        assert sc.shape == sd.shape
        xf = None if transforms is None else np.ascontiguousarray(transforms, dtype=np.float32).reshape(len(sc), 12)
        _check(self._lib.hnb_program_set_frames(self._h, int(first), len(sc), sc.ctypes.data, sd.ctypes.data, None if xf is None else xf.ctypes.data))

    def set_frames_ahead(self, spawn_counts, seeds, transforms=None, first=0):
        """Inputs of the next Context.simulate_steps for instances [first, first + count): arrays [n_steps][count] (transforms [n_steps][count][12])."""
        sc = np.ascontiguousarray(spawn_counts, dtype=np.uint32)
        sd = np.ascontiguousarray(seeds, dtype=np.uint32)
        assert sc.ndim == 2 and sc.shape == sd.shape
        n_steps, count = sc.shape
        xf = None if transforms is None else np.ascontiguousarray(transforms, dtype=np.float32).reshape(n_steps, count, 12)
        _check(self._lib.hnb_program_set_frames_ahead(self._h, int(first), count, n_steps, sc.ctypes.data, sd.ctypes.data, None if xf is None else xf.ctypes.data))

    def kernel_timing(self):
        """Context.kernel_timing() restricted to this program's kernels."""
        u, c, i, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint32()
        _check(self._lib.hnb_program_kernel_timing(self._h, C.byref(u), C.byref(c), C.byref(i), C.byref(n)))
        return {"update_ms_avg": u.value, "compact_ms_avg": c.value, "init_ms_avg": i.value, "frames": n.value}

    def device_view(self):
        """hnb_program_device_view: all instances behind one device-resident table (no synchronisation)."""
        v = ProgramView()
        _check(self._lib.hnb_program_device_view(self._h, C.byref(v)))
        return v

    def export(self, fields, dst_ptr, stride, capacity_records, count_ptr=None, offsets_ptr=None):
        """hnb_program_export: the alive particles of ALL instances, packed back to back in instance order, as records of `stride` bytes at the
        device address dst_ptr; offsets_ptr (device u32[n_instances + 1]) receives each instance's first record and the total, count_ptr (device
        u32[2]) the records written and the alive rows found. Raw device addresses; asynchronous on the simulation stream."""
        d = export_desc(fields, dst_ptr, stride, capacity_records, count_ptr)
        _check(self._lib.hnb_program_export(self._h, C.byref(d), C.c_void_p(int(offsets_ptr)) if offsets_ptr else None))

    def export_sorted(self, fields, dst_ptr, stride, capacity_records, count_ptr=None, offsets_ptr=None, *, scope="instance", key, v=(0, 0, 0), attr=0, descending=False):
        """hnb_program_export_sorted: the records of export(), ordered by a 32-bit key per particle (Effect.export_sorted's keys). scope "instance":
        the layout of export(), every instance's segment in its own sorted order; scope "program": one order over the particles of all instances
        (offsets_ptr must be None). Asynchronous."""
        d = export_desc(fields, dst_ptr, stride, capacity_records, count_ptr)
        s = export_sort(key, v, attr, descending)
        sc = SORT_SCOPES[scope] if isinstance(scope, str) else int(scope)
        _check(self._lib.hnb_program_export_sorted(self._h, C.byref(d), C.byref(s), sc, C.c_void_p(int(offsets_ptr)) if offsets_ptr else None))

    def export_filtered(self, fields, dst_ptr, stride, capacity_records, count_ptr=None, offsets_ptr=None, *, filter):
        """hnb_program_export_filtered: the records of export() for the rows a predicate keeps, every instance's segment in list order. `filter`:
        one filter for all instances or a list with one per instance (same kind and attr); each a dict of export_filter's keywords (kind, planes,
        sphere, attr, lo, hi, invert) or an ExportFilter. offsets_ptr / count_ptr as in export(), over the kept rows. Asynchronous."""
        d = export_desc(fields, dst_ptr, stride, capacity_records, count_ptr)
        fs = filter if isinstance(filter, (list, tuple)) else [filter]
        arr = (ExportFilter * max(len(fs), 1))(*[f if isinstance(f, ExportFilter) else export_filter(**f) for f in fs])
        _check(self._lib.hnb_program_export_filtered(self._h, C.byref(d), arr, len(fs), C.c_void_p(int(offsets_ptr)) if offsets_ptr else None))

    def export_filtered_sorted(self, fields, dst_ptr, stride, capacity_records, count_ptr=None, offsets_ptr=None, *, filter, sort):
        """hnb_program_export_sorted with an HnbExportSortFiltered, instance scope: of every instance the rows export_filtered() keeps, each
        segment in the order export_sorted(scope="instance") gives it. `filter`: one filter for all instances or a list with one per instance, as
        in export_filtered(); `sort`: a dict of export_sort's keywords (key, v, attr, descending) or an ExportSort. offsets_ptr / count_ptr over
        the kept rows. Asynchronous; the filter array lives until the call has returned."""
        d = export_desc(fields, dst_ptr, stride, capacity_records, count_ptr)
        fs = filter if isinstance(filter, (list, tuple)) else [filter]
        sf, arr = export_sort_filtered(sort, fs)
        rc = self._lib.hnb_program_export_sorted(self._h, C.byref(d), C.cast(C.byref(sf), C.POINTER(ExportSort)), SORT_SCOPES["instance"],
                                                 C.c_void_p(int(offsets_ptr)) if offsets_ptr else None)
        del arr   # (kept alive up to here: the library has read the host array)
        _check(rc)

    def bounds(self, attr, dst_ptr, capacity_records):
        """hnb_program_bounds: a Bounds record per instance at the device address dst_ptr (16-byte aligned), in instance order, and their union behind
        them: capacity_records >= n_instances + 1. Per component of the f32 attribute `attr` the smallest and the largest stored value among the
        alive particles, in the order of the sorted export's key. Asynchronous: enqueued on the simulation stream, nothing is read back."""
        d = bounds_desc(attr, dst_ptr, capacity_records)
        _check(self._lib.hnb_program_bounds(self._h, C.byref(d)))

    def deposit(self, dims, origin, inv_cell, count_ptr, channels=(), sums_ptr=None, stats_ptr=None, accumulate=False):
        """hnb_program_deposit: Effect.deposit over every instance of the program, all into the one grid; the stats are the totals."""
        d = deposit_desc(dims, origin, inv_cell, count_ptr, channels, sums_ptr, stats_ptr, accumulate)
        _check(self._lib.hnb_program_deposit(self._h, C.byref(d)))

    def splat(self, dims, origin, inv_cell, count_ptr, channels=(), sums_ptr=None, stats_ptr=None, accumulate=False):
        """hnb_program_splat: Effect.splat over every instance of the program, all into the one grid; the stats are the totals."""
        d = deposit_desc(dims, origin, inv_cell, count_ptr, channels, sums_ptr, stats_ptr, accumulate)
        _check(self._lib.hnb_program_splat(self._h, C.byref(d)))

    def sample_all(self, dims, origin, inv_cell, field_ptr, channels, mode=SAMPLE_TRILINEAR, scale=1.0, stats_ptr=None, field_instance_stride=0, instance_stats_ptr=None):
        """hnb_program_sample: Effect.sample over every instance of the program in one call. field_ptr is instance 0's field; with a
        field_instance_stride (f32 elements, a multiple of 4, at least n_cells * len(channels)) instance i reads field_ptr + 4 * i * stride bytes,
        with 0 every instance reads the one field. stats_ptr (device u32[4], optional): the totals; instance_stats_ptr (device u32[n_instances][4],
        optional): row i = what Effect.sample's stats would hold for instance i. Enqueued on the simulation stream, nothing is read back; the number
        of enqueues does not depend on the instance count."""
        d = program_sample_desc(dims, origin, inv_cell, field_ptr, channels, mode, scale, stats_ptr, field_instance_stride, instance_stats_ptr)
        _check(self._lib.hnb_program_sample(self._h, C.byref(d)))

    def kernel_info(self):
        """Which kernels run this program: 'init=jit|interp|none update=aot-stream:<name>|jit-stream|jit-generic|interp-*'."""
        buf = C.create_string_buffer(4096)
        _check(self._lib.hnb_program_kernel_info(self._h, buf, len(buf)))
        return buf.value.decode()

    def prepare_steps(self):
        """hnb_program_prepare_steps: build and install the steps kernel of a 'jit-stream' program now (Context.simulate_steps fuses its provable
        spans from the first call on). Does nothing for programs with a pre-built fused kernel or that can never fuse: see kernel_info()."""
        _check(self._lib.hnb_program_prepare_steps(self._h))

    def destroy(self):
        if self._h:
            for e in self._effects:
                e._h = None
            _check(self._lib.hnb_program_destroy(self._h))
            self._h = None
            self._ctx._programs.remove(self)


class Effect:
    def __init__(self, prog: Program, slot_base=0):
        self._prog = prog
        self._lib = prog._lib
        self._h = C.c_void_p()
        _check(self._lib.hnb_effect_create(prog._h, slot_base, C.byref(self._h)))
        prog._effects.append(self)
        self.capacity = self.metadata()["capacity"]

    def destroy(self):
        if self._h:
            _check(self._lib.hnb_effect_destroy(self._h))
            self._h = None
            self._prog._effects.remove(self)

    def index(self):
        """Current position of this instance in its program's tables (hnb_effect_index): destroying an instance moves the
        last one into its place."""
        out = C.c_uint32()
        _check(self._lib.hnb_effect_index(self._h, C.byref(out)))
        return out.value

    def set_simulated(self, simulated=True):
        """False freezes the instance (SimulationCondition::WhenVisible while not visible)."""
        _check(self._lib.hnb_effect_set_simulated(self._h, int(bool(simulated))))

    def set_parent(self, parent, channel, event_capacity=256):
        """EffectParent: this effect's init consumes the spawn events `parent` appends on `channel`
        (EmitSpawnEventModifier.child_index). 256 events per frame is the reference's hard-coded capacity."""
        _check(self._lib.hnb_effect_set_parent(self._h, parent._h, int(channel), int(event_capacity)))
        self._parent = parent

    def set_frame(self, spawn_count, seed, transform=None):
        xf = None
        if transform is not None:
            xf = np.ascontiguousarray(np.asarray(transform, dtype=np.float32).reshape(12))
        _check(self._lib.hnb_effect_set_frame(self._h, int(spawn_count), int(seed) & 0xFFFFFFFF, None if xf is None else xf.ctypes.data))

    def set_frames_ahead(self, spawn_counts, seeds, transforms=None):
        """Inputs of the steps of the next Context.simulate_steps: one spawn count and seed (and 3x4 transform) per step."""
        sc = np.ascontiguousarray(spawn_counts, dtype=np.uint32)
        sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64) & 0xFFFFFFFF, dtype=np.uint32)
        assert sc.ndim == 1 and sc.shape == sd.shape
        xf = None if transforms is None else np.ascontiguousarray(transforms, dtype=np.float32).reshape(len(sc), 12)
        _check(self._lib.hnb_effect_set_frames_ahead(self._h, len(sc), sc.ctypes.data, sd.ctypes.data, None if xf is None else xf.ctypes.data))

    def set_property(self, name, values):
        v = np.atleast_1d(np.asarray(values))
        words = v.astype(np.float32).view(np.uint32) if v.dtype.kind == "f" else v.astype(np.uint32)
        words = np.ascontiguousarray(words)
        _check(self._lib.hnb_effect_set_property(self._h, name.encode(), words.ctypes.data, len(words)))

    def apply_properties(self, effect_properties):
        """Push every value of an `EffectProperties` the program declares (the reference uploads the component's values
        every frame they changed, src/render/mod.rs property upload)."""
        for name, _default, value in effect_properties.properties():
            try:
                self.set_property(name, value)
            except HanabiError as e:
                if e.code != HNB_ERR_NOT_FOUND:   # a value for a property this effect's asset does not declare is not an error
                    raise

    def device_view(self):
        """hnb_effect_device_view: the effect's device pointers after the frames enqueued so far (no synchronisation)."""
        v = DeviceView()
        _check(self._lib.hnb_effect_device_view(self._h, C.byref(v)))
        return v

    def materialise(self, attr_ids):
        """hnb_effect_materialise: make these attributes' planes current for device-side readers (enqueued on the simulation stream)."""
        mask = 0
        for a in attr_ids:
            mask |= 1 << int(a)
        _check(self._lib.hnb_effect_materialise(self._h, mask))

    def export(self, fields, dst_ptr, stride, capacity_records, count_ptr=None):
        """hnb_effect_export: record r of the buffer at the device address dst_ptr = the particle in row r of the alive list; fields are
        (attribute id, byte offset) pairs, `stride` the bytes per record, count_ptr (device u32[2], optional) receives the records written and
        the alive rows found. Raw device addresses; enqueued on the simulation stream behind the frames so far, nothing synchronises."""
        d = export_desc(fields, dst_ptr, stride, capacity_records, count_ptr)
        _check(self._lib.hnb_effect_export(self._h, C.byref(d)))

    def export_sorted(self, fields, dst_ptr, stride, capacity_records, count_ptr=None, *, key, v=(0, 0, 0), attr=0, descending=False):
        """hnb_effect_export_sorted: the records of export(), ordered by a 32-bit key per particle - key "depth" (along the direction v), "distance"
        (squared, from the point v) or "attr" (the scalar attribute `attr`); ties keep list order, ascending and descending alike. A destination of
        K records receives the first K of that order."""
        d = export_desc(fields, dst_ptr, stride, capacity_records, count_ptr)
        s = export_sort(key, v, attr, descending)
        _check(self._lib.hnb_effect_export_sorted(self._h, C.byref(d), C.byref(s)))

    def export_filtered(self, fields, dst_ptr, stride, capacity_records, count_ptr=None, *, kind, planes=(), sphere=None, attr=0, lo=0, hi=0, invert=False):
        """hnb_effect_export_filtered: the records of export() for the rows a predicate keeps, in list order - kind "planes" (inside every half-space
        a*x + b*y + c*z + d >= 0 of `planes`), "sphere" ((cx, cy, cz, squared radius)) or "attr_range" (lo <= the scalar attribute `attr` <= hi,
        floats as binary32, ints as bit patterns); invert keeps the other rows. count_ptr: [0] = records written, [1] = rows kept."""
        d = export_desc(fields, dst_ptr, stride, capacity_records, count_ptr)
        f = export_filter(kind, planes, sphere, attr, lo, hi, invert)
        _check(self._lib.hnb_effect_export_filtered(self._h, C.byref(d), C.byref(f)))

    def export_filtered_sorted(self, fields, dst_ptr, stride, capacity_records, count_ptr=None, *, filter, sort):
        """hnb_effect_export_filtered_sorted: the rows export_filtered() keeps, in the order export_sorted() gives them. `filter`: a dict of
        export_filter's keywords (kind, planes, sphere, attr, lo, hi, invert); `sort`: a dict of export_sort's (key, v, attr, descending). A
        destination of K records receives the first K kept rows of that order. count_ptr: [0] = records written, [1] = rows kept."""
        d = export_desc(fields, dst_ptr, stride, capacity_records, count_ptr)
        f = export_filter(**filter)
        s = export_sort(**sort)
        _check(self._lib.hnb_effect_export_filtered_sorted(self._h, C.byref(d), C.byref(f), C.byref(s)))

    def export_binned(self, fields, dst_ptr, stride, capacity_records, count_ptr=None, *, dims, origin, inv_cell, cell_start_ptr):
        """hnb_effect_export_binned: the records of export(), ordered by the cell of a uniform grid of dims[0] x dims[1] x dims[2] cells that holds
        their POSITION - lowest corner `origin`, 1 / cell edge `inv_cell` per axis; particles outside the grid come last, particles of one cell
        keep list order. cell_start_ptr (device u32[n_cells + 2], 16-byte aligned): entry c = the records in cells below c, so cell c's records
        are [entry c, entry c + 1), entry n_cells the first outside record and entry n_cells + 1 the alive count. A destination of K records
        receives the first K of the order; the table is not clamped."""
        d = export_desc(fields, dst_ptr, stride, capacity_records, count_ptr)
        g = export_bins(dims, origin, inv_cell, cell_start_ptr)
        _check(self._lib.hnb_effect_export_binned(self._h, C.byref(d), C.byref(g)))

    def import_records(self, fields, src_ptr, stride, capacity_records, mode=IMPORT_ROWS, src_count_ptr=None, out_count_ptr=None):
        """hnb_effect_import, the inverse of export(): the records at the device address src_ptr are written into the planes of the particles they
        belong to - mode IMPORT_ROWS: record r belongs to row r of the alive list; IMPORT_IDS: to the particle its ID field (slot_base + slot)
        names, in any order and as any subset; records naming a dead slot or none of this effect are skipped. At most capacity_records records
        and, with src_count_ptr (device u32), at most that many are read; out_count_ptr (device u32[2], optional) receives the records applied
        and skipped. Raw device addresses; enqueued on the simulation stream behind everything so far, nothing synchronises; later frames see the
        planes as after write_attr of the same values."""
        d = import_desc(fields, src_ptr, stride, capacity_records, mode, src_count_ptr, out_count_ptr)
        _check(self._lib.hnb_effect_import(self._h, C.byref(d)))

    def bounds(self, attr, dst_ptr, capacity_records=1):
        """hnb_effect_bounds: one Bounds record at the device address dst_ptr (16-byte aligned) - per component of the f32 attribute `attr` the
        smallest and the largest stored value among the alive particles (POSITION: the effect's axis-aligned box), the alive particles and those
        with a NaN. Asynchronous: enqueued on the simulation stream, nothing is read back."""
        d = bounds_desc(attr, dst_ptr, capacity_records)
        _check(self._lib.hnb_effect_bounds(self._h, C.byref(d)))

    def deposit(self, dims, origin, inv_cell, count_ptr, channels=(), sums_ptr=None, stats_ptr=None, accumulate=False):
        """hnb_effect_deposit: the alive particles summed into the uniform grid of export_binned - count_ptr (device u32[n_cells + 1], 16-byte
        aligned): the particles per cell, entry n_cells the outside bin; sums_ptr (device i64[(n_cells + 1) * len(channels)], channel-minor):
        per channel (attribute id, component, frac_bits) the sum of round(v * 2^frac_bits) over the cell's particles, exact to the bit;
        stats_ptr (device u32[4], optional): deposited, outside, rejected contributions, 0. accumulate: add onto what is there instead of clearing
        first. Raw device addresses; enqueued on the simulation stream, nothing is read back. As f32: sums.to(torch.float32) * 2.0**-frac_bits."""
        d = deposit_desc(dims, origin, inv_cell, count_ptr, channels, sums_ptr, stats_ptr, accumulate)
        _check(self._lib.hnb_effect_deposit(self._h, C.byref(d)))

    def splat(self, dims, origin, inv_cell, count_ptr, channels=(), sums_ptr=None, stats_ptr=None, accumulate=False):
        """hnb_effect_splat: deposit through the stencil of sample(SAMPLE_TRILINEAR) - the same grid, destinations and fixed-point sums as deposit
        (and the two may accumulate into one grid); count_ptr takes the particles per OWN cell, unweighted; per channel an inside particle adds
        round(v * W * 2^frac_bits) to each of the eight cell centres around it, W the corner's trilinear weight, and an outside particle what
        deposit adds to row n_cells. A channel (SPLAT_ATTR_ONE, 0, frac_bits) has v = 1 for every particle: the weights themselves.
        stats_ptr (device u32[4], optional): visited, outside, rejected (particle, channel) pairs, 0. Exact to the bit whatever the grouping."""
        d = deposit_desc(dims, origin, inv_cell, count_ptr, channels, sums_ptr, stats_ptr, accumulate)
        _check(self._lib.hnb_effect_splat(self._h, C.byref(d)))

    def sample(self, dims, origin, inv_cell, field_ptr, channels, mode=SAMPLE_TRILINEAR, scale=1.0, stats_ptr=None):
        """hnb_effect_sample: the deposit's way back - for every alive particle inside the uniform grid of export_binned, channel k of the f32 field
        at field_ptr (device f32[n_cells * len(channels)], channel-minor, 16-byte aligned: a [D, H, W, k] tensor) - its cell's value (SAMPLE_NEAREST)
        or the trilinear blend of the eight cell centres around it, clamped to the edge (SAMPLE_TRILINEAR) - times `scale` is stored (SAMPLE_SET) or
        added (SAMPLE_ADD) into channels[k] = (attribute id, component, op). Particles outside the grid and dead slots keep every bit. stats_ptr
        (device u32[4], optional): visited, sampled, outside, 0. Raw device addresses; enqueued on the simulation stream, nothing is read back."""
        d = sample_desc(dims, origin, inv_cell, field_ptr, channels, mode, scale, stats_ptr)
        _check(self._lib.hnb_effect_sample(self._h, C.byref(d)))

    def neighbours(self, dims, origin, inv_cell, radius, channels, weight=NEIGHBOUR_W_ONE, candidate_limit=4096, scale=1.0, stats_ptr=None):
        """hnb_effect_neighbours: particle <-> particle - for every alive particle inside the uniform grid of export_binned, per channel (src attribute
        id or SPLAT_ATTR_ONE, src component, 0 or NEIGHBOUR_DIFF, frac_bits, dst attribute id, dst component, SAMPLE_SET or SAMPLE_ADD) the
        fixed-point sum of weight * source over the particles within `radius` (radius * inv_cell <= 1) and within one cell of it, times 2^-frac_bits
        times scale, stored or added into the destination component. Queries with more than candidate_limit candidates in their 27 cells are left
        alone and counted. stats_ptr (device u32[8], optional): visited, gathered, outside, crowded, rejected contributions, 0, 0, 0. Raw device
        addresses; enqueued on the simulation stream, nothing is read back."""
        d = neighbour_desc(dims, origin, inv_cell, radius, channels, weight, candidate_limit, scale, stats_ptr)
        _check(self._lib.hnb_effect_neighbours(self._h, C.byref(d)))

    def pairs(self, dims, origin, inv_cell, radius, rows_ptr, start_ptr, pairs_ptr=None, pair_capacity=0, d2_ptr=None, stats_ptr=None, candidate_limit=4096, half=False):
        """hnb_effect_pairs: the fixed-radius neighbour list as CSR - for the alive particles inside the uniform grid of export_binned, in its row
        order: rows_ptr (device u32[capacity]) takes the slot of every row (PAIRS_NO_ROW past the inside rows), start_ptr (device
        u32[capacity + 1]) the offsets of the runs, pairs_ptr (device u32[pair_capacity]) the slots of the particles within `radius` (radius *
        inv_cell <= 1) and within one cell of the row's, in ascending row order, d2_ptr (device f32[pair_capacity], optional) their squared
        distances. half: each pair once, under the lower slot. Only the pairs below pair_capacity are written and the offsets are clamped to it;
        pair_capacity 0 counts only. Queries with more than candidate_limit candidates list nothing and are counted. stats_ptr (device u32[8],
        optional): visited, inside, outside, crowded, the true total (low, high word), pairs written, 0. Raw device addresses; enqueued on the
        simulation stream, nothing is read back and nothing of the effect is written."""
        d = pairs_desc(dims, origin, inv_cell, radius, rows_ptr, start_ptr, pairs_ptr, pair_capacity, d2_ptr, stats_ptr, candidate_limit, half)
        _check(self._lib.hnb_effect_pairs(self._h, C.byref(d)))

    def neighbours_from(self, source, dims, origin, inv_cell, radius, channels, weight=NEIGHBOUR_W_ONE, candidate_limit=4096, scale=1.0, stats_ptr=None):
        """hnb_effect_neighbours_from: neighbours() across two effects of one context - the queries are this effect's alive particles, the sources
        those of the Effect `source`, the destinations planes of this effect. A channel's source attribute is looked up in source's layout (with
        NEIGHBOUR_DIFF in this effect's as well: v_i is the query's own), its destination in this effect's. There is no self-exclusion; the
        candidates of a query are sources only. stats_ptr (device u32[8], optional): queries visited, gathered, outside, crowded, rejected
        contributions, inside sources, alive sources visited, 0. `source` is only read. Raw device addresses; enqueued on the simulation stream,
        nothing is read back."""
        d = neighbour_desc(dims, origin, inv_cell, radius, channels, weight, candidate_limit, scale, stats_ptr)
        _check(self._lib.hnb_effect_neighbours_from(self._h, source._h if source is not None else None, C.byref(d)))

    def pairs_from(self, source, dims, origin, inv_cell, radius, rows_ptr, start_ptr, pairs_ptr=None, pair_capacity=0, d2_ptr=None, stats_ptr=None, candidate_limit=4096):
        """hnb_effect_pairs_from: pairs() across two effects of one context - the rows are this effect's alive particles inside the grid, in its
        export_binned order; the runs hold slots of the Effect `source`, in source's export_binned order. rows_ptr (device u32[capacity]) and
        start_ptr (device u32[capacity + 1]) are sized from THIS effect's capacity; pairs_ptr / d2_ptr (device u32 / f32 [pair_capacity]) take the
        source slots within `radius` and their squared distances. There is no self-exclusion and no half form; the candidates of a query are
        sources only. Truncation and pair_capacity 0 as in pairs(). stats_ptr (device u32[8], optional): queries visited, inside, outside,
        crowded, the true total (low, high word), pairs written, inside sources. Neither effect is written. Raw device addresses; enqueued on
        the simulation stream, nothing is read back."""
        d = pairs_desc(dims, origin, inv_cell, radius, rows_ptr, start_ptr, pairs_ptr, pair_capacity, d2_ptr, stats_ptr, candidate_limit, False)
        _check(self._lib.hnb_effect_pairs_from(self._h, source._h if source is not None else None, C.byref(d)))

    def check(self):
        """hnb_effect_check: list permutation, alive bytes, age < lifetime, fault flag - on the device; a dict with "ok"."""
        c = EffectCheck()
        _check(self._lib.hnb_effect_check(self._h, C.byref(c)))
        return c.as_dict()

    def compare(self, other):
        """hnb_effect_compare: this effect against another of the same layout on the same device, bit for bit; a dict with "equal"."""
        d = EffectDiff()
        _check(self._lib.hnb_effect_compare(self._h, other._h, C.byref(d)))
        return d.as_dict()

    def metadata(self):
        m = EffectMetadata()
        _check(self._lib.hnb_effect_metadata(self._h, C.byref(m)))
        return m.as_dict()

    def alive_count(self):
        n = C.c_uint32()
        _check(self._lib.hnb_effect_alive_count(self._h, C.byref(n)))
        return int(n.value)

    def read_attr(self, attr_id):
        attr_id = int(attr_id)
        out = np.zeros((self.capacity, ATTR_COMPONENTS[attr_id]), dtype=np.uint32)
        _check(self._lib.hnb_effect_read_attr(self._h, attr_id, out.ctypes.data, out.nbytes))
        return out.view(np.float32) if ATTR_IS_FLOAT[attr_id] else out

    def write_attr(self, attr_id, array):
        a = np.ascontiguousarray(array)
        _check(self._lib.hnb_effect_write_attr(self._h, int(attr_id), a.ctypes.data, a.nbytes))

    def alive_list(self):
        out = np.zeros(max(self.alive_count(), 1), dtype=np.uint32)
        _check(self._lib.hnb_effect_read_alive_list(self._h, out.ctypes.data, len(out)))
        return out[: self.alive_count()]

    def dead_list(self):
        n = self.capacity - self.alive_count()
        out = np.zeros(max(n, 1), dtype=np.uint32)
        _check(self._lib.hnb_effect_read_dead_list(self._h, out.ctypes.data, len(out)))
        return out[:n]
