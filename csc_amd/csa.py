"""csc_amd.csa -- Python mirror of the `.csa` container entry points (include/csa_mi355x.h).

The four operations of the reference's `csarc` (`class CSArc`, archiver/csarc.cpp:37-70) with its
options (ParseArg, csarc.cpp:137-208), served by `libcsc_mi355x.so`: streams and adler32 on the
GPU, container logic in C++.  Nothing here computes anything; it marshals arguments.
"""
import ctypes as C
from typing import Iterable, List, Optional, Sequence

from . import load


class CSAOptions(C.Structure):
    _fields_ = [
        ("level", C.c_int), ("dict_size", C.c_uint32), ("recurse", C.c_int), ("overwrite", C.c_int),
        ("verbose", C.c_int), ("mt_count", C.c_int), ("split_count", C.c_int), ("to_dir", C.c_char_p),
        ("device_streams", C.c_int), ("hbm_budget", C.c_uint64), ("task_bytes", C.c_uint64),
    ]


class CSAStats(C.Structure):
    _fields_ = [
        ("raw_bytes", C.c_uint64), ("archive_bytes", C.c_uint64), ("index_raw_size", C.c_uint64),
        ("index_compressed_size", C.c_uint64), ("n_entries", C.c_uint32), ("n_tasks", C.c_uint32),
        ("n_blocks", C.c_uint32), ("verify_failures", C.c_uint32), ("seconds_total", C.c_double),
        ("seconds_encode", C.c_double), ("peak_streams", C.c_uint32), ("reserved", C.c_uint32),
        ("seconds_io", C.c_double), ("seconds_setup", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class CSAFrag(C.Structure):
    _fields_ = [("bid", C.c_uint32), ("checksum", C.c_uint32), ("posblock", C.c_uint64),
                ("size", C.c_uint64), ("posfile", C.c_uint64)]


class CSADevFile(C.Structure):
    """CSADevFile of include/csa_mi355x.h.  `name` is kept as an address: CSAMI_PlanDeviceLayout's names are not NUL-terminated."""
    _fields_ = [("name", C.c_void_p), ("esize", C.c_int64), ("edate", C.c_int64), ("eattr", C.c_int64),
                ("offset", C.c_uint64), ("size", C.c_uint64), ("nfrags", C.c_uint32), ("failed_frags", C.c_uint32)]


class CSADevReadStats(C.Structure):
    _fields_ = [("tasks", C.c_uint64), ("frags", C.c_uint64), ("waves", C.c_uint64), ("launches", C.c_uint64),
                ("decode_launches", C.c_uint64), ("readback_bytes", C.c_uint64), ("raw_bytes", C.c_uint64),
                ("verify_failures", C.c_uint32), ("reserved", C.c_uint32), ("kernel_ms", C.c_double), ("seconds_total", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class CSADevStopStats(C.Structure):
    _fields_ = [("decoded_bytes", C.c_uint64), ("task_raw_bytes", C.c_uint64), ("scratch_bytes", C.c_uint64), ("stopped_tasks", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CSADevWriteStats(C.Structure):
    _fields_ = [("tasks", C.c_uint64), ("frags", C.c_uint64), ("waves", C.c_uint64), ("blocks", C.c_uint64), ("launches", C.c_uint64),
                ("encode_launches", C.c_uint64), ("readback_bytes", C.c_uint64), ("upload_bytes", C.c_uint64), ("raw_bytes", C.c_uint64),
                ("archive_bytes", C.c_uint64), ("index_raw_size", C.c_uint64), ("index_compressed_size", C.c_uint64),
                ("n_entries", C.c_uint32), ("retries", C.c_uint32), ("kernel_ms", C.c_double), ("seconds_encode", C.c_double),
                ("seconds_total", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CSADevDiff(C.Structure):
    _fields_ = [("first_diff", C.c_uint64), ("status", C.c_uint32), ("failed_frags", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CSADevSlice(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("run", C.c_uint64), ("stride", C.c_uint64), ("count", C.c_uint64)]


class CSADevSliceStats(C.Structure):
    _fields_ = [("selected_bytes", C.c_uint64), ("touched_bytes", C.c_uint64), ("periodic_pieces", C.c_uint64), ("plain_pieces", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CSADevGatherStats(C.Structure):
    _fields_ = [("selected_bytes", C.c_uint64), ("hull_bytes", C.c_uint64), ("periodic_pieces", C.c_uint64), ("plain_pieces", C.c_uint64),
                ("gathered_tasks", C.c_uint64), ("inplace_tasks", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CSADevSpreadStats(C.Structure):
    _fields_ = [("selected_bytes", C.c_uint64), ("hull_bytes", C.c_uint64), ("periodic_pieces", C.c_uint64), ("plain_pieces", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CSADevUpdateTask(C.Structure):
    _fields_ = [("base_bid", C.c_uint64), ("status", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {"base_bid": int(self.base_bid), "status": int(self.status)}


class CSADevUpdateStats(C.Structure):
    _fields_ = [("candidates", C.c_uint64), ("reused_tasks", C.c_uint64), ("encoded_tasks", C.c_uint64), ("reused_raw_bytes", C.c_uint64),
                ("reused_stream_bytes", C.c_uint64), ("encoded_raw_bytes", C.c_uint64), ("checked_bytes", C.c_uint64),
                ("decoded_bytes", C.c_uint64), ("check_waves", C.c_uint64), ("check_launches", C.c_uint64), ("decode_launches", C.c_uint64),
                ("check_kernel_ms", C.c_double), ("seconds_check", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CSADevDigest(C.Structure):
    _fields_ = [("b", C.c_uint8 * 32)]


class CSADevDigestStats(C.Structure):
    _fields_ = [("frags", C.c_uint64), ("leaves", C.c_uint64), ("digested_bytes", C.c_uint64), ("launches", C.c_uint64),
                ("mismatches", C.c_uint64), ("first_mismatch", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        """(the names the write's and the read's statistics also have get a prefix: the dicts are merged)"""
        return {"digest_frags": self.frags, "digest_leaves": self.leaves, "digested_bytes": self.digested_bytes, "digest_launches": self.launches,
                "mismatches": self.mismatches, "first_mismatch": self.first_mismatch, "digest_kernel_ms": self.kernel_ms}


class CSADevMoveStats(C.Structure):
    _fields_ = [("moves", C.c_uint64), ("moved_bytes", C.c_uint64), ("parked_moves", C.c_uint64), ("parked_bytes", C.c_uint64),
                ("held_stream_bytes", C.c_uint64), ("launches", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        """(the names the write's statistics also have get a prefix: the dicts are merged)"""
        return {"moves": self.moves, "moved_bytes": self.moved_bytes, "parked_moves": self.parked_moves, "parked_bytes": self.parked_bytes,
                "held_stream_bytes": self.held_stream_bytes, "move_launches": self.launches, "move_kernel_ms": self.kernel_ms}


LIST_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(CSAFrag))

SYMBOLS = ["CSA_OptionsInit", "CSA_Add", "CSA_Extract", "CSA_Test", "CSA_List", "CSA_ReadIndex",
           "CSA_Adler32", "CSAMI_Adler32Device", "CSA_DecimalTime", "CSA_UnixTime",
           "CSAMI_AddShardEncode", "CSAMI_FreeBlob", "CSAMI_AddShardAssemble", "CSAMI_PlanInfo", "CSAMI_PlanShards", "CSA_IndexRoundTrip",
           "CSAMI_DeviceOpen", "CSAMI_DevicePlan", "CSAMI_DeviceRead", "CSAMI_DeviceClose", "CSAMI_PlanDeviceLayout", "CSAMI_DeviceKernelMs",
           "CSAMI_DeviceReadStop", "CSAMI_PlanDeviceStops",
           "CSAMI_DeviceWritePlan", "CSAMI_DeviceWrite", "CSAMI_DeviceWriteKernelMs",
           "CSAMI_CheckBuffers", "CSAMI_DeviceWriteFrom", "CSAMI_DeviceReadInto", "CSAMI_DeviceCompare",
           "CSAMI_DeviceReadSlices", "CSAMI_PlanDeviceSlices", "CSAMI_DeviceWriteSlices",
           "CSAMI_CheckSlices", "CSAMI_DeviceReadIntoSlices", "CSAMI_DeviceCompareSlices",
           "CSAMI_DeviceUpdate", "CSAMI_PlanDeviceUpdate",
           "CSAMI_DeviceWriteFragCount", "CSAMI_DeviceDigestSlices", "CSAMI_DeviceUpdateDigests", "CSAMI_DeviceReadDigests",
           "CSAMI_DeviceDigestKernelMs", "CSAMI_DeviceUpdateInPlace", "CSAMI_DeviceMoveKernelMs"]

CSA_MAX_FRAGMENTS = 127
CSA_TOO_MANY_FRAGMENTS = -94
CSA_UNSAFE_NAME = -93
CSCMI_DEVICE_ERROR = -95
WRITE_ERROR = -97
CSAMI_DEV_STOP_EARLY = 1
CSA_DIFF_BYTES, CSA_DIFF_SIZE, CSA_DIFF_SKIPPED, CSA_DIFF_SHORT = 1, 2, 4, 8
CSAMI_UPDATE_TRUST_SUMS = 1
CSAMI_UPDATE_TRUST_DIGESTS = 2
DIGEST_BYTES, DIGEST_LEAF = 32, 16384
NO_MISMATCH = (1 << 64) - 1                # CSADevDigestStats.first_mismatch where nothing differs
CSA_UPD_REUSED, CSA_UPD_NEW, CSA_UPD_PROPS, CSA_UPD_CHANGED, CSA_UPD_BASE_BAD = 0, 1, 2, 3, 4
NO_BID = (1 << 64) - 1                     # CSADevUpdateTask.base_bid of a task that is no candidate
NO_DIFF = (1 << 64) - 1                    # CSADevDiff.first_diff without CSA_DIFF_BYTES

_lib = None


def lib():
    """the product library with the CSA_* prototypes bound"""
    global _lib
    if _lib is None:
        L = load().lib
        names = C.POINTER(C.c_char_p)
        L.CSA_OptionsInit.argtypes = [C.POINTER(CSAOptions)]
        L.CSA_OptionsInit.restype = None
        for fn in (L.CSA_Add, L.CSA_Extract, L.CSA_Test):
            fn.argtypes = [C.c_char_p, names, C.c_int, C.POINTER(CSAOptions), C.POINTER(CSAStats)]
            fn.restype = C.c_int
        L.CSA_List.argtypes = [C.c_char_p, names, C.c_int, LIST_FN, C.c_void_p]
        L.CSA_List.restype = C.c_int
        L.CSA_ReadIndex.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64]
        L.CSA_ReadIndex.restype = C.c_int64
        L.CSA_Adler32.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64]
        L.CSA_Adler32.restype = C.c_uint32
        L.CSAMI_Adler32Device.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]
        L.CSAMI_Adler32Device.restype = C.c_int
        L.CSA_DecimalTime.argtypes = [C.c_int64]
        L.CSA_DecimalTime.restype = C.c_int64
        L.CSA_UnixTime.argtypes = [C.c_int64]
        L.CSA_UnixTime.restype = C.c_int64
        L.CSAMI_AddShardEncode.argtypes = [names, C.c_int, C.POINTER(CSAOptions), C.c_int, C.c_int,
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(CSAStats)]
        L.CSAMI_AddShardEncode.restype = C.c_int
        L.CSAMI_FreeBlob.argtypes = [C.c_void_p]
        L.CSAMI_FreeBlob.restype = None
        L.CSAMI_AddShardAssemble.argtypes = [C.c_char_p, names, C.c_int, C.POINTER(CSAOptions), C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_uint64), C.c_int, C.POINTER(CSAStats)]
        L.CSAMI_AddShardAssemble.restype = C.c_int
        L.CSAMI_PlanInfo.argtypes = [names, C.c_int, C.POINTER(CSAOptions), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.CSAMI_PlanInfo.restype = C.c_int
        L.CSA_IndexRoundTrip.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        L.CSA_IndexRoundTrip.restype = C.c_int64
        files = C.POINTER(CSADevFile)
        L.CSAMI_DeviceOpen.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        L.CSAMI_DeviceOpen.restype = C.c_int
        L.CSAMI_DevicePlan.argtypes = [C.c_void_p, names, C.c_int, files, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        L.CSAMI_DevicePlan.restype = C.c_int
        L.CSAMI_DeviceRead.argtypes = [C.c_void_p, names, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(CSAOptions), files, C.c_uint32,
                                       C.POINTER(CSADevReadStats)]
        L.CSAMI_DeviceRead.restype = C.c_int
        L.CSAMI_DeviceReadStop.argtypes = L.CSAMI_DeviceRead.argtypes + [C.POINTER(CSADevStopStats)]
        L.CSAMI_DeviceReadStop.restype = C.c_int
        u64s = C.POINTER(C.c_uint64)
        L.CSAMI_PlanDeviceStops.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, names, C.c_int, u64s, u64s, u64s, C.c_uint32, C.POINTER(C.c_uint32)]
        L.CSAMI_PlanDeviceStops.restype = C.c_int
        L.CSAMI_DeviceKernelMs.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.CSAMI_DeviceKernelMs.restype = None
        L.CSAMI_DeviceClose.argtypes = [C.c_void_p]
        L.CSAMI_DeviceClose.restype = None
        L.CSAMI_PlanDeviceLayout.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, names, C.c_int, files, C.c_uint32, C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]
        L.CSAMI_PlanDeviceLayout.restype = C.c_int
        L.CSAMI_DeviceWritePlan.argtypes = [files, C.c_uint32, C.c_char_p, C.POINTER(CSAOptions), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint64)]
        L.CSAMI_DeviceWritePlan.restype = C.c_int
        L.CSAMI_DeviceWrite.argtypes = [C.c_void_p, C.c_uint64, files, C.c_uint32, C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(CSAOptions),
                                        C.POINTER(CSADevWriteStats)]
        L.CSAMI_DeviceWrite.restype = C.c_int
        L.CSAMI_DeviceWriteKernelMs.argtypes = [C.POINTER(C.c_double)]
        L.CSAMI_DeviceWriteKernelMs.restype = None
        ptrs = C.POINTER(C.c_void_p)
        L.CSAMI_CheckBuffers.argtypes = [ptrs, u64s, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
        L.CSAMI_CheckBuffers.restype = C.c_int
        L.CSAMI_DeviceWriteFrom.argtypes = [ptrs] + L.CSAMI_DeviceWrite.argtypes[2:]
        L.CSAMI_DeviceWriteFrom.restype = C.c_int
        L.CSAMI_DeviceReadInto.argtypes = [C.c_void_p, names, C.c_int, ptrs, u64s, C.c_uint32, C.c_uint32, C.POINTER(CSAOptions), files,
                                           C.POINTER(CSADevReadStats), C.POINTER(CSADevStopStats)]
        L.CSAMI_DeviceReadInto.restype = C.c_int
        L.CSAMI_DeviceCompare.argtypes = [C.c_void_p, names, C.c_int, ptrs, u64s, C.c_uint32, C.c_uint32, C.POINTER(CSAOptions), files,
                                          C.POINTER(CSADevDiff), C.POINTER(CSADevReadStats), C.POINTER(CSADevStopStats)]
        L.CSAMI_DeviceCompare.restype = C.c_int
        slices = C.POINTER(CSADevSlice)
        L.CSAMI_DeviceReadSlices.argtypes = [C.c_void_p, names, C.c_int, slices, ptrs, u64s, C.c_uint32, C.c_uint32, C.POINTER(CSAOptions), files,
                                             C.POINTER(CSADevReadStats), C.POINTER(CSADevStopStats), C.POINTER(CSADevSliceStats)]
        L.CSAMI_DeviceReadSlices.restype = C.c_int
        L.CSAMI_PlanDeviceSlices.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, names, C.c_int, slices, C.c_uint32, u64s, u64s, u64s, C.c_uint32,
                                             C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.CSAMI_PlanDeviceSlices.restype = C.c_int
        L.CSAMI_DeviceWriteSlices.argtypes = [ptrs, u64s, slices] + L.CSAMI_DeviceWrite.argtypes[2:] + [C.POINTER(CSADevGatherStats)]
        L.CSAMI_DeviceWriteSlices.restype = C.c_int
        L.CSAMI_CheckSlices.argtypes = [ptrs, u64s, slices, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
        L.CSAMI_CheckSlices.restype = C.c_int
        L.CSAMI_DeviceReadIntoSlices.argtypes = [C.c_void_p, names, C.c_int, ptrs, u64s, slices, C.c_uint32, C.c_uint32, C.POINTER(CSAOptions), files,
                                                 C.POINTER(CSADevReadStats), C.POINTER(CSADevStopStats), C.POINTER(CSADevSpreadStats)]
        L.CSAMI_DeviceReadIntoSlices.restype = C.c_int
        L.CSAMI_DeviceCompareSlices.argtypes = [C.c_void_p, names, C.c_int, ptrs, u64s, slices, C.c_uint32, C.c_uint32, C.POINTER(CSAOptions), files,
                                                C.POINTER(CSADevDiff), C.POINTER(CSADevReadStats), C.POINTER(CSADevStopStats),
                                                C.POINTER(CSADevSpreadStats)]
        L.CSAMI_DeviceCompareSlices.restype = C.c_int
        L.CSAMI_DeviceUpdate.argtypes = [C.c_void_p, ptrs, u64s, slices, files, C.c_uint32, C.c_char_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                         C.POINTER(CSAOptions), C.POINTER(CSADevWriteStats), C.POINTER(CSADevGatherStats),
                                         C.POINTER(CSADevUpdateStats), C.POINTER(CSADevUpdateTask), C.c_uint32]
        L.CSAMI_DeviceUpdate.restype = C.c_int
        L.CSAMI_PlanDeviceUpdate.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, files, C.c_uint32, C.POINTER(CSAOptions), u64s, C.c_uint32,
                                             C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.CSAMI_PlanDeviceUpdate.restype = C.c_int
        L.CSAMI_DeviceWriteFragCount.argtypes = [files, C.c_uint32, C.c_char_p, C.POINTER(CSAOptions), u64s]
        L.CSAMI_DeviceWriteFragCount.restype = C.c_int
        L.CSAMI_DeviceDigestSlices.argtypes = [ptrs, u64s, slices, files, C.c_uint32, C.c_char_p, C.POINTER(CSAOptions), C.c_void_p, C.c_uint64,
                                               C.POINTER(CSADevDigestStats)]
        L.CSAMI_DeviceDigestSlices.restype = C.c_int
        L.CSAMI_DeviceUpdateDigests.argtypes = ([C.c_void_p, C.c_void_p, C.c_uint64] + L.CSAMI_DeviceUpdate.argtypes[1:]
                                                + [C.c_void_p, C.c_uint64, C.POINTER(CSADevDigestStats)])
        L.CSAMI_DeviceUpdateDigests.restype = C.c_int
        L.CSAMI_DeviceReadDigests.argtypes = [C.c_void_p, C.POINTER(CSAOptions), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(CSADevReadStats),
                                              C.POINTER(CSADevDigestStats)]
        L.CSAMI_DeviceReadDigests.restype = C.c_int
        L.CSAMI_DeviceDigestKernelMs.argtypes = [C.POINTER(C.c_double)]
        L.CSAMI_DeviceDigestKernelMs.restype = None
        # (CSAMI_DeviceUpdateDigests's arguments with buf_cap behind the handle, no arc, and the move statistics at the end)
        L.CSAMI_DeviceUpdateInPlace.argtypes = ([C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + L.CSAMI_DeviceUpdate.argtypes[1:7]
                                                + L.CSAMI_DeviceUpdate.argtypes[9:]
                                                + [C.c_void_p, C.c_uint64, C.POINTER(CSADevDigestStats), C.POINTER(CSADevMoveStats)])
        L.CSAMI_DeviceUpdateInPlace.restype = C.c_int
        L.CSAMI_DeviceMoveKernelMs.argtypes = [C.POINTER(C.c_double)]
        L.CSAMI_DeviceMoveKernelMs.restype = None
        _lib = L
    return _lib


def _names(filenames: Iterable[str]):
    enc = [f.encode() if isinstance(f, str) else bytes(f) for f in filenames]
    arr = (C.c_char_p * max(len(enc), 1))(*enc)
    return arr, len(enc)


def options(level: int = 2, dict_size: int = 32000000, recurse: bool = False, overwrite: bool = False,
            verbose: bool = False, mt_count: int = 1, split_count: int = 1, to_dir: Optional[str] = None,
            device_streams: int = 0, hbm_budget: int = 0, task_bytes: int = 0) -> CSAOptions:
    o = CSAOptions()
    lib().CSA_OptionsInit(C.byref(o))
    o.level, o.dict_size, o.recurse, o.overwrite = level, dict_size, int(recurse), int(overwrite)
    o.verbose, o.mt_count, o.split_count = int(verbose), mt_count, split_count
    if to_dir is not None:
        o.to_dir = to_dir.encode()
    o.device_streams, o.hbm_budget, o.task_bytes = device_streams, hbm_budget, task_bytes
    return o


def add(arcname: str, filenames: Sequence[str], **opts):
    """`csarc a [opts] arcname filenames...` -> (rc, stats dict)"""
    o, st = options(**opts), CSAStats()
    arr, n = _names(filenames)
    rc = lib().CSA_Add(arcname.encode(), arr, n, C.byref(o), C.byref(st))
    return rc, st.as_dict()


def plan_info(filenames: Sequence[str], **opts):
    """the plan `add` would execute (host only) -> (rc, number of task streams, largest fragment count of any file)"""
    o = options(**opts)
    arr, n = _names(filenames)
    nt, mf = C.c_uint32(), C.c_uint32()
    rc = lib().CSAMI_PlanInfo(arr, n, C.byref(o), C.byref(nt), C.byref(mf))
    return rc, int(nt.value), int(mf.value)


def index_round_trip(raw: bytes):
    """bounds-checked parse + re-pack of a raw index buffer -> (rc, bytes): rc = re-packed size, -1 unparsable, CSA_UNSAFE_NAME"""
    buf = (C.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
    n = lib().CSA_IndexRoundTrip(buf, len(raw), None, 0)
    if n < 0:
        return int(n), b""
    out = (C.c_uint8 * max(n, 1))()
    lib().CSA_IndexRoundTrip(buf, len(raw), out, n)
    return int(n), bytes(out[:n])


def add_shard_encode(filenames: Sequence[str], rank: int, world: int, **opts):
    """this rank's tasks of `csarc a [opts] arc filenames...` encoded on its GPU -> (rc, blob bytes, stats dict)"""
    o, st = options(**opts), CSAStats()
    arr, n = _names(filenames)
    ptr, ln = C.c_void_p(), C.c_uint64()
    rc = lib().CSAMI_AddShardEncode(arr, n, C.byref(o), rank, world, C.byref(ptr), C.byref(ln), C.byref(st))
    blob = b""
    if rc == 0:
        blob = C.string_at(ptr, ln.value)
        lib().CSAMI_FreeBlob(ptr)
    return rc, blob, st.as_dict()


def plan_shards(filenames: Sequence[str], world: int, **opts):
    """the deal add_shard_encode uses, without encoding anything (host only): -> (rank of every task, cost estimate of every task)"""
    o = options(**opts)
    arr, n = _names(filenames)
    L = lib()
    L.CSAMI_PlanShards.restype = C.c_int
    nt = L.CSAMI_PlanShards(arr, n, C.byref(o), world, None, None, 0)
    if nt < 0:
        raise RuntimeError(f"CSAMI_PlanShards failed rc={nt}")
    ro, co = (C.c_uint32 * max(nt, 1))(), (C.c_double * max(nt, 1))()
    L.CSAMI_PlanShards(arr, n, C.byref(o), world, ro, co, nt)
    return list(ro[:nt]), list(co[:nt])


def add_shard_assemble(arcname: str, filenames: Sequence[str], blobs: Sequence[bytes], **opts):
    """every rank's blob -> the archive `csarc a -t1` writes; -> (rc, stats dict)"""
    o, st = options(**opts), CSAStats()
    arr, n = _names(filenames)
    keep = [C.create_string_buffer(b, len(b)) if len(b) else C.create_string_buffer(1) for b in blobs]
    ptrs = (C.c_void_p * max(len(keep), 1))(*[C.cast(k, C.c_void_p) for k in keep])
    lens = (C.c_uint64 * max(len(keep), 1))(*[len(b) for b in blobs])
    rc = lib().CSAMI_AddShardAssemble(arcname.encode(), arr, n, C.byref(o), ptrs, lens, len(blobs), C.byref(st))
    return rc, st.as_dict()


def extract(arcname: str, filenames: Sequence[str] = (), **opts):
    """`csarc x [opts] arcname [names...]` -> (rc, stats dict)"""
    o, st = options(**opts), CSAStats()
    arr, n = _names(filenames)
    rc = lib().CSA_Extract(arcname.encode(), arr, n, C.byref(o), C.byref(st))
    return rc, st.as_dict()


def test(arcname: str, filenames: Sequence[str] = (), **opts):
    """`csarc t [opts] arcname [names...]` -> (rc, stats dict)"""
    o, st = options(**opts), CSAStats()
    arr, n = _names(filenames)
    rc = lib().CSA_Test(arcname.encode(), arr, n, C.byref(o), C.byref(st))
    return rc, st.as_dict()


def list_entries(arcname: str, filenames: Sequence[str] = ()) -> Optional[List[dict]]:
    """`csarc l -v arcname [names...]` -> entries in name order, or None on a bad archive"""
    out = []

    def cb(ctx, name, esize, edate, eattr, nfrags, frags):
        out.append({"name": name.decode("latin-1"), "esize": esize, "edate": edate, "eattr": eattr,
                    "frags": [{"bid": frags[i].bid, "checksum": frags[i].checksum, "posblock": frags[i].posblock,
                               "size": frags[i].size, "posfile": frags[i].posfile} for i in range(nfrags)]})

    fn = LIST_FN(cb)
    arr, n = _names(filenames)
    rc = lib().CSA_List(arcname.encode(), arr, n, fn, None)
    return out if rc == 0 else None


def read_index(arcname: str) -> Optional[bytes]:
    n = lib().CSA_ReadIndex(arcname.encode(), None, 0)
    if n < 0:
        return None
    buf = (C.c_uint8 * max(n, 1))()
    lib().CSA_ReadIndex(arcname.encode(), buf, n)
    return bytes(buf[:n])


def adler32(data, adler: int = 0) -> int:
    b = bytes(data)
    return int(lib().CSA_Adler32(adler, b, len(b)))


def adler32_device(device_ptr: int, nbytes: int, adler: int = 0) -> int:
    out = C.c_uint32()
    rc = lib().CSAMI_Adler32Device(adler, C.c_void_p(device_ptr), nbytes, C.byref(out))
    if rc != 0:
        raise RuntimeError(f"CSAMI_Adler32Device failed: {rc}")
    return int(out.value)


# ---- device-resident read ----------------------------------------------------------------------------------------------

def _file_dict(f: CSADevFile, name: str) -> dict:
    return {"name": name, "esize": f.esize, "edate": f.edate, "eattr": f.eattr, "offset": f.offset, "size": f.size,
            "nfrags": f.nfrags, "failed_frags": f.failed_frags}


def plan_device_layout(raw_index: bytes, arc_size: int, names: Sequence[str] = ()):
    """CSAMI_PlanDeviceLayout (host only): the layout DeviceArchive.extract gives these raw index bytes ->
    (rc, [file dicts], dst_bytes, [raw size of every task that would be decoded, in decode order])"""
    buf = (C.c_uint8 * max(len(raw_index), 1)).from_buffer_copy(raw_index or b"\0")
    arr, n = _names(names)
    nf, nt, total = C.c_uint32(), C.c_uint32(), C.c_uint64()
    rc = lib().CSAMI_PlanDeviceLayout(buf, len(raw_index), arc_size, arr, n, None, 0, C.byref(nf), C.byref(total), None, 0, C.byref(nt))
    if rc != 0:
        return rc, [], 0, []
    files, tasks = (CSADevFile * max(nf.value, 1))(), (C.c_uint64 * max(nt.value, 1))()
    rc = lib().CSAMI_PlanDeviceLayout(buf, len(raw_index), arc_size, arr, n, files, nf.value, C.byref(nf), C.byref(total), tasks, nt.value, C.byref(nt))
    out = []
    for f in files[:nf.value]:
        ln = int.from_bytes(C.string_at(f.name - 4, 4), "little")          # the name lies in `buf`, its length in front of it
        out.append(_file_dict(f, C.string_at(f.name, ln).decode("latin-1")))
    return rc, out, int(total.value), list(tasks[:nt.value])


def plan_device_stops(raw_index: bytes, arc_size: int, names: Sequence[str] = ()):
    """CSAMI_PlanDeviceStops (host only): the tasks DeviceArchive.extract(names, stop_early=True) decodes for these raw index
    bytes, in decode order -> (rc, [{"bid", "stop", "raw"}])"""
    buf = (C.c_uint8 * max(len(raw_index), 1)).from_buffer_copy(raw_index or b"\0")
    arr, n = _names(names)
    nt = C.c_uint32()
    rc = lib().CSAMI_PlanDeviceStops(buf, len(raw_index), arc_size, arr, n, None, None, None, 0, C.byref(nt))
    if rc != 0:
        return rc, []
    k = nt.value
    bids, stops, raws = ((C.c_uint64 * max(k, 1))() for _ in range(3))
    rc = lib().CSAMI_PlanDeviceStops(buf, len(raw_index), arc_size, arr, n, bids, stops, raws, k, C.byref(nt))
    return rc, [{"bid": int(b), "stop": int(s), "raw": int(r)} for b, s, r in zip(bids[:k], stops[:k], raws[:k])]


def rows_slice(row_bytes: int, r0: int, r1: int, c0: int = 0, c1: Optional[int] = None):
    """the slice (offset, run, stride, count) for rows r0..r1 and byte columns c0..c1 (c1 None: the row's end) of a row-major matrix
    of row_bytes a row; a block of whole rows, or of one row, is one byte range (count == 1)"""
    c1 = row_bytes if c1 is None else c1
    if not (0 <= r0 < r1 and 0 <= c0 < c1 <= row_bytes):
        raise ValueError("an empty or inverted block")
    if (c0, c1) == (0, row_bytes) or r1 - r0 == 1:
        return (r0 * row_bytes + c0, (r1 - r0 - 1) * row_bytes + c1 - c0, (r1 - r0 - 1) * row_bytes + c1 - c0, 1)
    return (r0 * row_bytes + c0, c1 - c0, row_bytes, r1 - r0)


def tensor_slice(t):
    """a torch tensor of any dtype whose layout is count rows of run contiguous bytes a constant stride apart -- a contiguous tensor, a
    block of columns t2d[:, c0:c1], or more dimensions that collapse to that -- as (1-d uint8 view of its WHOLE storage, slice): the
    slice's packed bytes are t.contiguous()'s bytes.  ValueError for any other layout (a negative or zero stride with more than one
    element along it, rows that overlap, a third level of striding).  write_slices takes the pair as an entry's tensor and slice."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError("a torch tensor")
    item = t.element_size()
    base = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
    offset = t.storage_offset() * item
    if t.numel() == 0:
        return base, (offset, 0, 0, 0)
    # the dimensions that count, innermost first, in bytes; neighbours that continue each other collapse into one
    dims = [(item, 1)]                                             # (extent in bytes, stride in bytes): the element itself
    for n, st in zip(reversed(t.shape), reversed(t.stride())):
        if n == 1:
            continue
        if st <= 0:
            raise ValueError("a dimension with a stride that is not positive")
        ext, step = dims[-1]
        if st * item == ext * step:
            dims[-1] = (ext * n, step)
        else:
            dims.append((n, st * item))
    run = dims[0][0]                                               # (dims[0] has step 1: contiguous bytes)
    if len(dims) == 1:
        return base, (offset, run, run, 1)
    if len(dims) > 2 or dims[1][1] < run:
        raise ValueError("not rows of contiguous bytes a constant stride apart")
    return base, (offset, run, dims[1][1], dims[1][0])


def _slice_table(files, slices):
    """the CSADevSlice of every entry of a files table; slices: {stored name: (offset, length) | (offset, run, stride, count)}, an entry
    without a key gets count 0.  KeyError for a key that is no entry of the table."""
    slices = dict(slices)
    unknown = set(slices) - {f["name"] for f in files}
    if unknown:
        raise KeyError(sorted(unknown)[0])
    arr = (CSADevSlice * max(len(files), 1))()
    for a, f in zip(arr, files):
        s = slices.get(f["name"])
        if s is not None:
            a.offset, a.run, a.stride, a.count = (s[0], s[1], s[1], 1) if len(s) == 2 else s
    return arr


def plan_device_slices(raw_index: bytes, arc_size: int, slices_by_entry, names: Sequence[str] = ()):
    """CSAMI_PlanDeviceSlices (host only): the tasks DeviceArchive.extract_slices(slices_by_entry, names=names) decodes for these raw
    index bytes, in decode order, each with its stop under stop_early -> (rc, [{"bid", "stop", "raw"}], number of touched fragments)"""
    rc, files, _, _ = plan_device_layout(raw_index, arc_size, names)
    if rc != 0:
        return rc, [], 0
    table = _slice_table(files, slices_by_entry)
    buf = (C.c_uint8 * max(len(raw_index), 1)).from_buffer_copy(raw_index or b"\0")
    arr, n = _names(names)
    nt, touched = C.c_uint32(), C.c_uint32()
    rc = lib().CSAMI_PlanDeviceSlices(buf, len(raw_index), arc_size, arr, n, table, len(files), None, None, None, 0, C.byref(nt), C.byref(touched))
    if rc != 0:
        return rc, [], 0
    k = nt.value
    bids, stops, raws = ((C.c_uint64 * max(k, 1))() for _ in range(3))
    rc = lib().CSAMI_PlanDeviceSlices(buf, len(raw_index), arc_size, arr, n, table, len(files), bids, stops, raws, k, C.byref(nt), C.byref(touched))
    return rc, [{"bid": int(b), "stop": int(s), "raw": int(r)} for b, s, r in zip(bids[:k], stops[:k], raws[:k])], int(touched.value)


def _write_table(files):
    """[dicts with name, esize, edate, eattr, offset] -> (CSADevFile array, the name buffers it points into)"""
    keep = [C.create_string_buffer(f["name"].encode("latin-1") if isinstance(f["name"], str) else bytes(f["name"])) for f in files]
    arr = (CSADevFile * max(len(keep), 1))()
    for a, f, k in zip(arr, files, keep):
        a.name = C.cast(k, C.c_void_p)
        a.esize, a.edate, a.eattr, a.offset = f["esize"], f["edate"], f["eattr"], f.get("offset", 0)
    return arr, keep


def device_write_plan(files, arcname: str = "out.csa", **opts):
    """CSAMI_DeviceWritePlan (host only): the plan DeviceArchive.write would execute for this table ->
    (rc, number of task streams, largest fragment count of any entry, raw bytes of all tasks)"""
    arr, keep = _write_table(files)
    o = options(**opts)
    nt, mf, raw = C.c_uint32(), C.c_uint32(), C.c_uint64()
    rc = lib().CSAMI_DeviceWritePlan(arr, len(keep), arcname.encode(), C.byref(o), C.byref(nt), C.byref(mf), C.byref(raw))
    return rc, int(nt.value), int(mf.value), int(raw.value)


def device_write_frag_count(files, arcname: str = "out.csa", **opts):
    """CSAMI_DeviceWriteFragCount (host only): the fragments, and so the entries of the digest table, that DeviceArchive.write of this
    table makes -> (rc, number of fragments)"""
    arr, keep = _write_table(files)
    o = options(**opts)
    n = C.c_uint64()
    rc = lib().CSAMI_DeviceWriteFragCount(arr, len(keep), arcname.encode(), C.byref(o), C.byref(n))
    return rc, int(n.value)


def fragment_digest(data: bytes) -> bytes:
    """The digest of one fragment as the device computes it (include/csa_mi355x.h): BLAKE2s-256 in tree mode -- fan-out 0, maximal
    depth 2, leaf length 16384, inner length 32 -- with hashlib's stock parameters.  The host reference of the digest tables."""
    import hashlib
    data = bytes(data)
    n_leaves = max(1, -(-len(data) // DIGEST_LEAF))
    tree = dict(digest_size=DIGEST_BYTES, fanout=0, depth=2, leaf_size=DIGEST_LEAF, inner_size=DIGEST_BYTES)
    leaves = b"".join(hashlib.blake2s(data[DIGEST_LEAF * i:DIGEST_LEAF * (i + 1)], node_offset=i, node_depth=0, last_node=(i == n_leaves - 1),
                                      **tree).digest() for i in range(n_leaves))
    return hashlib.blake2s(leaves, node_offset=0, node_depth=1, last_node=True, **tree).digest()


def plan_device_update(raw_index: bytes, arc_size: int, files, **opts):
    """CSAMI_PlanDeviceUpdate (host only): the candidate step of DeviceArchive.update over these raw index bytes of the base and the
    new table (dicts with name, esize, edate, eattr) -> (rc, [base bid of every task of the new plan, NO_BID where it is no
    candidate], number of candidates)"""
    buf = (C.c_uint8 * max(len(raw_index), 1)).from_buffer_copy(raw_index or b"\0")
    arr, keep = _write_table(files)
    o = options(**opts)
    nt, nc = C.c_uint32(), C.c_uint32()
    rc = lib().CSAMI_PlanDeviceUpdate(buf, len(raw_index), arc_size, arr, len(keep), C.byref(o), None, 0, C.byref(nt), C.byref(nc))
    if rc != 0:
        return rc, [], 0
    bids = (C.c_uint64 * max(nt.value, 1))()
    rc = lib().CSAMI_PlanDeviceUpdate(buf, len(raw_index), arc_size, arr, len(keep), C.byref(o), bids, nt.value, C.byref(nt), C.byref(nc))
    return rc, [int(b) for b in bids[:nt.value]], int(nc.value)


def device_write_kernel_ms():
    """HIP-event milliseconds of this thread's last DeviceArchive.write by kernel: (k_frag_pieces -- k_frag_rows in a wave of write_slices
    with a piece across a run border --, k_frag_fold, k_block_table, k_gather_extents)"""
    ms = (C.c_double * 4)()
    lib().CSAMI_DeviceWriteKernelMs(ms)
    return tuple(ms)


def device_digest_kernel_ms():
    """HIP-event milliseconds of this thread's last digesting call by kernel: (k_digest_leaves, k_digest_roots)"""
    ms = (C.c_double * 2)()
    lib().CSAMI_DeviceDigestKernelMs(ms)
    return tuple(ms)


def device_move_kernel_ms():
    """HIP-event milliseconds of this thread's last DeviceArchive.update_in_place by launch: (the park copy, k_move_extents' left phase,
    its right phase)"""
    ms = (C.c_double * 3)()
    lib().CSAMI_DeviceMoveKernelMs(ms)
    return tuple(ms)


def check_buffers(ptrs: Sequence[int], sizes: Sequence[int], excl=(0, 0), disjoint: bool = False):
    """CSAMI_CheckBuffers (host only): the address checks write_tensors, extract_into and compare make before anything is launched.
    ptrs, sizes: addresses and byte counts; excl: (address, size) of the range none may overlap -> (rc, lowest refused index or None)"""
    n = len(ptrs)
    pa, sa = (C.c_void_p * max(n, 1))(*ptrs), (C.c_uint64 * max(n, 1))(*sizes)
    bad = C.c_uint32(0xFFFFFFFF)
    rc = lib().CSAMI_CheckBuffers(pa, sa, n, C.c_void_p(excl[0]), excl[1], int(disjoint), C.byref(bad))
    return rc, (int(bad.value) if rc != 0 else None)


def check_slices(ptrs: Sequence[int], sizes: Sequence[int], slices, excl=(0, 0), disjoint: bool = False):
    """CSAMI_CheckSlices (host only): the address checks extract_into_slices (disjoint) and compare_slices make before anything is
    launched.  ptrs, sizes: addresses and byte counts of the buffers; slices: (offset, run, stride, count) into each; excl: (address,
    size) of the range no hull may overlap -> (rc, lowest refused index or None)"""
    n = len(ptrs)
    pa, sa = (C.c_void_p * max(n, 1))(*ptrs), (C.c_uint64 * max(n, 1))(*sizes)
    sl = (CSADevSlice * max(n, 1))()
    for a, s in zip(sl, slices):
        a.offset, a.run, a.stride, a.count = s
    bad = C.c_uint32(0xFFFFFFFF)
    rc = lib().CSAMI_CheckSlices(pa, sa, sl, n, C.c_void_p(excl[0]), excl[1], int(disjoint), C.byref(bad))
    return rc, (int(bad.value) if rc != 0 else None)


def _is_bytes_tensor(t) -> bool:
    import torch
    return isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and t.dim() == 1


def _write_planned(files, arcname, arc, device, opts, call, plan=False):
    """The one write call below write, write_tensors, write_slices and update: the table, the two capacities, the call and the stats
    dict.  arc None: the archive tensor is allocated here on `device` with the plan's capacity, and once more with twice the room
    on WRITE_ERROR (`plan`: the plan is made even with an arc).  call(table, n, (arcname, arc address, arc bytes), options, number
    of planned tasks or None) makes the library call and returns (rc, [its statistics structs, the write's first]).
    -> (rc, uint8 CUDA view of the archive, stats dict)"""
    import torch
    o, nt, caps = options(**opts), None, [None]
    if arc is None or plan:
        rc, nt, _, raw = device_write_plan(files, arcname, **opts)
        if rc != 0:
            return rc, None, {"files": []}
    if arc is None:
        cap = 24 + raw + raw // 8 + (64 << 10) * (nt + 1) + (1 << 20)
        caps = [cap, 2 * cap]
    for cap in caps:
        if cap is not None:
            arc = torch.empty(cap, dtype=torch.uint8, device=device)
        arr, keep = _write_table(files)
        torch.cuda.synchronize()                   # the buffers were filled on torch's stream, the library launches on its own
        rc, stats = call(arr, len(keep), (arcname.encode(), C.c_void_p(arc.data_ptr()) if arc.numel() else None, int(arc.numel())), o, nt)
        if rc != WRITE_ERROR:
            break
    d = {}
    for st in stats:
        d.update(st.as_dict())
    d["files"] = [_file_dict(a, f["name"]) for a, f in zip(arr, files)]
    return rc, (arc[:stats[0].archive_bytes] if rc == 0 else None), d


def _is_digest_table(t) -> bool:
    import torch
    return isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and t.dim() == 2 and t.shape[1] == DIGEST_BYTES


def _digest_table(files, arcname, device, opts):
    """an empty digest table for a write of `files`: (rc, uint8 CUDA tensor [n_frags, 32] or None)"""
    import torch
    rc, n = device_write_frag_count(files, arcname, **opts)
    return rc, (torch.empty((n, DIGEST_BYTES), dtype=torch.uint8, device=device) if rc == 0 else None)


def _write_slices(base, entries, arcname, arc, flags, whole_default, opts, digests=False, base_digests=None, whole=False):
    """DeviceArchive.write_tensors (whole), DeviceArchive.write_slices (base None) and DeviceArchive.update: CSAMI_DeviceWriteSlices, or
    CSAMI_DeviceUpdate over the base; with digests or base_digests CSAMI_DeviceUpdateDigests, and stats["digests"] is the table.
    whole_default: an entry without "slice" is its whole tensor (else: no bytes); whole: no slices at all are handed in"""
    files, table = [], (CSADevSlice * max(len(entries), 1))()
    for a, e in zip(table, entries):
        t = e["tensor"]
        if not (t is None or _is_bytes_tensor(t)):
            raise TypeError("tensor: a contiguous 1-d torch.uint8 CUDA tensor, or None")
        s = e.get("slice") or ((0, int(t.numel())) if whole_default and t is not None else (0, 0, 0, 0))
        a.offset, a.run, a.stride, a.count = (s[0], s[1], s[1], 1 if s[1] else 0) if len(s) == 2 else s
        files.append({"name": e["name"], "esize": a.run * a.count if a.count else 0, "edate": e["edate"], "eattr": e["eattr"]})
    if not (arc is None or _is_bytes_tensor(arc)):
        raise TypeError("arc: a contiguous 1-d torch.uint8 CUDA tensor")
    live = [e["tensor"] for e in entries]                      # alive across the call
    ptrs = (C.c_void_p * max(len(live), 1))(*[t.data_ptr() if t is not None and t.numel() else None for t in live])
    sizes = (C.c_uint64 * max(len(live), 1))(*[0 if t is None else int(t.numel()) for t in live])
    device = arc.device if arc is not None else next((t.device for t in live if t is not None), "cuda")
    last = []
    if base_digests is not None and not _is_digest_table(base_digests):
        raise TypeError("base_digests: a contiguous torch.uint8 CUDA tensor [n, 32]")
    out = None
    if _is_digest_table(digests):
        out = digests
    elif digests is not False and digests is not None:
        if digests is not True:
            raise TypeError("digests: True, or a contiguous torch.uint8 CUDA tensor [n, 32] to write the table into")
        rc, out = _digest_table(files, arcname, device, opts)
        if rc != 0:
            return rc, None, {"files": []}

    def call(arr, n, where, o, nt):
        st, gs, us, ds = CSADevWriteStats(), CSADevGatherStats(), CSADevUpdateStats(), CSADevDigestStats()
        plain = out is None and base_digests is None and not flags & CSAMI_UPDATE_TRUST_DIGESTS
        if plain:
            if whole:
                return lib().CSAMI_DeviceWriteFrom(ptrs, arr, n, *where, C.byref(o), C.byref(st)), [st]
            if base is None:
                return lib().CSAMI_DeviceWriteSlices(ptrs, sizes, table, arr, n, *where, C.byref(o), C.byref(st), C.byref(gs)), [st, gs]
        tasks = (CSADevUpdateTask * max(nt or 0, 1))()
        if base is not None:
            last[:] = [tasks, nt, st]
        if plain:
            return lib().CSAMI_DeviceUpdate(base._h, ptrs, sizes, table, arr, n, *where, flags, C.byref(o), C.byref(st), C.byref(gs),
                                            C.byref(us), tasks, nt), [st, gs, us]
        rc = lib().CSAMI_DeviceUpdateDigests(
            None if base is None else base._h, None if base_digests is None else C.c_void_p(base_digests.data_ptr() or 0),
            0 if base_digests is None else int(base_digests.shape[0]), ptrs, None if whole else sizes, None if whole else table, arr, n, *where,
            flags, C.byref(o), C.byref(st), C.byref(gs), C.byref(us), tasks, nt or 0,
            None if out is None else C.c_void_p(out.data_ptr() or 0), 0 if out is None else int(out.shape[0]), C.byref(ds))
        return rc, ([st] if whole else [st, gs]) + ([us] if base is not None else []) + [ds]
    rc, arc, d = _write_planned(files, arcname, arc, device, opts, call, plan=base is not None)
    if last:
        d["tasks"] = [t.as_dict() for t in last[0][:min(last[1], int(last[2].tasks))]]
    if out is not None:
        d["digests"] = out
    return rc, arc, d


class DeviceArchive:
    """A `.csa` that lies in device memory (CSAMI_DeviceOpen ... CSAMI_DeviceClose): `csarc x` / `csarc t` without the archive,
    the decoded tasks or the files crossing the bus.  torch is the plumbing: it owns the buffers and hands out views."""

    def __init__(self, handle, tensor):
        self._h, self._arc = handle, tensor           # the archive tensor must outlive the handle

    @classmethod
    def open(cls, tensor) -> "DeviceArchive":
        """tensor: 1-d contiguous torch.uint8 CUDA tensor of any alignment.  Raises ValueError(rc) where CSAMI_DeviceOpen refuses it."""
        import torch
        if not _is_bytes_tensor(tensor):
            raise TypeError("a contiguous 1-d torch.uint8 CUDA tensor")
        torch.cuda.synchronize()                       # the tensor was filled on torch's stream, the library launches on its own
        h = C.c_void_p()
        rc = lib().CSAMI_DeviceOpen(C.c_void_p(tensor.data_ptr()), int(tensor.numel()), C.byref(h))
        if rc != 0:
            err = ValueError(f"CSAMI_DeviceOpen: {rc}")
            err.rc = rc
            raise err
        return cls(h, tensor)

    def _plan(self, names):
        arr, n = _names(names)
        nf, total = C.c_uint32(), C.c_uint64()
        rc = lib().CSAMI_DevicePlan(self._h, arr, n, None, 0, C.byref(nf), C.byref(total))
        if rc != 0:
            raise ValueError(f"CSAMI_DevicePlan: {rc}")
        return arr, n, int(nf.value), int(total.value)

    def plan(self, names: Sequence[str] = ()):
        """-> ([file dicts in index order], dst_bytes)"""
        arr, n, nf, total = self._plan(names)
        files = (CSADevFile * max(nf, 1))()
        lib().CSAMI_DevicePlan(self._h, arr, n, files, nf, None, None)
        return [_file_dict(f, C.string_at(f.name).decode("latin-1")) for f in files[:nf]], total

    def _read(self, names, dst, opts, stop_early=False):
        import torch
        arr, n, nf, total = self._plan(names)
        files, st, o = (CSADevFile * max(nf, 1))(), CSADevReadStats(), options(**opts)
        torch.cuda.synchronize()
        args = (self._h, arr, n, C.c_void_p(dst.data_ptr()) if dst is not None else None,
                int(dst.numel()) if dst is not None else 0, C.byref(o), files, nf, C.byref(st))
        if stop_early:
            ss = CSADevStopStats()
            rc = lib().CSAMI_DeviceReadStop(*args, C.byref(ss))
        else:
            rc = lib().CSAMI_DeviceRead(*args)
        out = st.as_dict()
        if stop_early:
            out.update(ss.as_dict())
        return rc, [_file_dict(f, C.string_at(f.name).decode("latin-1")) for f in files[:nf]], out

    def extract(self, names: Sequence[str] = (), dst=None, stop_early=False, **opts):
        """`csarc x` -> (rc, {name: uint8 CUDA view of dst}, stats dict).  dst: a 1-d contiguous torch.uint8 CUDA tensor of any
        alignment with at least plan(names)[1] bytes (allocated here when None); stats["files"] is the files table.
        stop_early: CSAMI_DeviceReadStop -- every task is decoded only up to its last selected byte, and the stats dict also holds
        decoded_bytes, task_raw_bytes, scratch_bytes and stopped_tasks."""
        import torch
        if dst is None:
            dst = torch.empty(max(self._plan(names)[3], 1), dtype=torch.uint8, device=self._arc.device)
        elif not _is_bytes_tensor(dst):
            raise TypeError("dst: a contiguous 1-d torch.uint8 CUDA tensor")
        rc, files, st = self._read(names, dst, opts, stop_early)
        st["files"] = files
        views = {} if rc == WRITE_ERROR else {f["name"]: dst[f["offset"]:f["offset"] + f["size"]] for f in files}
        return rc, views, st

    def test(self, names: Sequence[str] = (), stop_early=False, **opts):
        """`csarc t` -> (rc, stats dict); stop_early as in extract"""
        rc, files, st = self._read(names, None, opts, stop_early)
        st["files"] = files
        return rc, st

    @staticmethod
    def write(files, src, arcname: str = "out.csa", arc=None, **opts):
        """`csarc a -t1` -> (rc, uint8 CUDA view of the archive, stats dict).  files: the dicts plan() and extract() return (name,
        esize, edate, eattr and offset are read); src: the 1-d contiguous torch.uint8 CUDA tensor they lie in, any alignment; arc: the
        tensor to write into (allocated here when None, and once more with twice the room on WRITE_ERROR).  stats["files"] is the
        table as returned: size = esize, nfrags = the fragments the entry got."""
        if not _is_bytes_tensor(src) or not (arc is None or _is_bytes_tensor(arc)):
            raise TypeError("src, arc: contiguous 1-d torch.uint8 CUDA tensors")

        def call(arr, n, where, o, nt):
            st = CSADevWriteStats()
            return lib().CSAMI_DeviceWrite(C.c_void_p(src.data_ptr()) if src.numel() else None, int(src.numel()), arr, n, *where,
                                           C.byref(o), C.byref(st)), [st]
        return _write_planned(files, arcname, arc, src.device, opts, call)

    @staticmethod
    def write_tensors(entries, arcname: str = "out.csa", arc=None, digests=False, **opts):
        """`csarc a -t1` of entries that lie in tensors of their own (CSAMI_DeviceWriteFrom) -> (rc, uint8 CUDA view of the archive,
        stats dict), as write.  entries: dicts with name, tensor, edate, eattr; tensor: a 1-d contiguous torch.uint8 CUDA tensor of any
        alignment, its numel the entry's size, or None for directories and empty files.  The tensors may alias each other, not arc.
        digests (True, or a contiguous uint8 CUDA tensor [n, 32] to write into): stats["digests"] is the archive's digest table, a uint8
        CUDA tensor [n_frags, 32] in index order, and the digest statistics are merged in (CSAMI_DeviceUpdateDigests)."""
        files = []
        for e in entries:
            t = e["tensor"]
            if not (t is None or _is_bytes_tensor(t)):
                raise TypeError("tensor: a contiguous 1-d torch.uint8 CUDA tensor, or None")
            files.append({"name": e["name"], "esize": 0 if t is None else int(t.numel()), "edate": e["edate"], "eattr": e["eattr"]})
        if not (arc is None or _is_bytes_tensor(arc)):
            raise TypeError("arc: a contiguous 1-d torch.uint8 CUDA tensor")
        live = [e["tensor"] for e in entries]                      # alive across the call
        ptrs = (C.c_void_p * max(len(live), 1))(*[t.data_ptr() if t is not None and t.numel() else None for t in live])
        device = arc.device if arc is not None else next((t.device for t in live if t is not None), "cuda")
        if digests is not False and digests is not None:
            return _write_slices(None, entries, arcname, arc, 0, True, opts, digests=digests, whole=True)

        def call(arr, n, where, o, nt):
            st = CSADevWriteStats()
            return lib().CSAMI_DeviceWriteFrom(ptrs, arr, n, *where, C.byref(o), C.byref(st)), [st]
        return _write_planned(files, arcname, arc, device, opts, call)

    @staticmethod
    def write_slices(entries, arcname: str = "out.csa", arc=None, digests=False, **opts):
        """`csarc a -t1` of entries gathered from strided slices of buffers (CSAMI_DeviceWriteSlices) -> (rc, uint8 CUDA view of the
        archive, stats dict), as write_tensors, with the gather statistics beside the write's.  entries: dicts with name, tensor,
        slice, edate, eattr; tensor: the 1-d contiguous torch.uint8 CUDA base buffer (None for directories and empty files); slice:
        (offset, length) | (offset, run, stride, count) into it -- rows_slice makes one for a block of a row-major matrix,
        tensor_slice both for a strided view.  The entry's bytes are the selected ones, packed: esize = run * count.  The buffers
        are only read and may alias each other, not arc.  digests: as in write_tensors."""
        return _write_slices(None, entries, arcname, arc, 0, False, opts, digests=digests)

    @staticmethod
    def digest_slices(entries, arcname: str = "out.csa", **opts):
        """the digest table write_slices(entries, digests=True) would hand out, with nothing written and nothing encoded
        (CSAMI_DeviceDigestSlices) -> (rc, uint8 CUDA tensor [n_frags, 32], stats dict).  An entry without "slice" is its whole tensor.
        Row i is fragment_digest of fragment i of the index: the entries in byte-wise name order, an entry's fragments in offset order."""
        import torch
        files, table = [], (CSADevSlice * max(len(entries), 1))()
        for a, e in zip(table, entries):
            t = e["tensor"]
            if not (t is None or _is_bytes_tensor(t)):
                raise TypeError("tensor: a contiguous 1-d torch.uint8 CUDA tensor, or None")
            s = e.get("slice") or ((0, int(t.numel())) if t is not None else (0, 0, 0, 0))
            a.offset, a.run, a.stride, a.count = (s[0], s[1], s[1], 1 if s[1] else 0) if len(s) == 2 else s
            files.append({"name": e["name"], "esize": a.run * a.count if a.count else 0, "edate": e["edate"], "eattr": e["eattr"]})
        live = [e["tensor"] for e in entries]
        ptrs = (C.c_void_p * max(len(live), 1))(*[t.data_ptr() if t is not None and t.numel() else None for t in live])
        sizes = (C.c_uint64 * max(len(live), 1))(*[0 if t is None else int(t.numel()) for t in live])
        device = next((t.device for t in live if t is not None), "cuda")
        rc, out = _digest_table(files, arcname, device, opts)
        if rc != 0:
            return rc, None, {}
        arr, keep = _write_table(files)
        o, ds = options(**opts), CSADevDigestStats()
        torch.cuda.synchronize()
        rc = lib().CSAMI_DeviceDigestSlices(ptrs, sizes, table, arr, len(keep), arcname.encode(), C.byref(o), C.c_void_p(out.data_ptr() or 0),
                                            int(out.shape[0]), C.byref(ds))
        return rc, (out if rc == 0 else None), ds.as_dict()

    def digests(self, expect=None, **opts):
        """`csarc t` of the whole archive that also hands out its digest table (CSAMI_DeviceReadDigests) -> (rc, uint8 CUDA tensor
        [n_frags, 32], stats dict: the read's and the digest statistics).  expect: a table to compare every fragment with on the
        device; a mismatch counts as a failed checksum of that fragment does, and in stats["mismatches"] / ["first_mismatch"]."""
        import torch
        if expect is not None and not _is_digest_table(expect):
            raise TypeError("expect: a contiguous torch.uint8 CUDA tensor [n, 32]")
        n = sum(f["nfrags"] for f in self.plan()[0])
        if expect is not None and int(expect.shape[0]) != n:
            raise ValueError(f"expect: {n} rows, one per fragment of the archive")
        out = torch.empty((n, DIGEST_BYTES), dtype=torch.uint8, device=self._arc.device)
        o, st, ds = options(**opts), CSADevReadStats(), CSADevDigestStats()
        torch.cuda.synchronize()
        rc = lib().CSAMI_DeviceReadDigests(self._h, C.byref(o), C.c_void_p(out.data_ptr() or 0), n,
                                           None if expect is None else C.c_void_p(expect.data_ptr() or 0), C.byref(st), C.byref(ds))
        d = st.as_dict()
        d.update(ds.as_dict())
        return rc, out, d

    def update(self, entries, arcname: str = "out.csa", arc=None, trust_sums=False, digests=False, base_digests=None, trust_digests=False,
               **opts):
        """write_slices of `entries` with this archive as the base (CSAMI_DeviceUpdate): a task of the new plan that has the
        composition and the bytes of a task of this archive gets that task's stream copied, not encoded -> (rc, uint8 CUDA view of
        the new archive, stats dict) as write_slices, with the update statistics merged in and stats["tasks"] = [{"base_bid",
        "status"}] per task of the new plan.  entries: write_slices's; an entry without "slice" is its whole tensor.  The new
        archive is byte for byte write_slices's as long as this archive was written at the same level.  trust_sums: nothing is
        decoded -- a task is taken for unchanged when every fragment's adler32 equals this archive's index's, a 32-bit test that two
        different contents can pass.  arc must not overlap this archive's tensor (update_in_place is the call for that).
        digests: as in write_tensors -- the new archive's table, computed in this call from the entries' bytes.  base_digests: this
        archive's table, as the call that wrote it (or digests()) handed it out.  trust_digests: nothing is decoded -- a task is taken
        for unchanged when every fragment's BLAKE2s digest equals base_digests's at that fragment's place in this archive's index."""
        flags = (CSAMI_UPDATE_TRUST_SUMS if trust_sums else 0) | (CSAMI_UPDATE_TRUST_DIGESTS if trust_digests else 0)
        return _write_slices(self, entries, arcname, arc, flags, True, opts, digests=digests, base_digests=base_digests)

    def update_in_place(self, entries, buf=None, arcname: str = "out.csa", trust_sums=False, digests=False, base_digests=None,
                        trust_digests=False, **opts):
        """update with the new archive in the place of this one (CSAMI_DeviceUpdateInPlace) -> (rc, uint8 CUDA view buf[:archive_bytes],
        stats dict): update's, with the move statistics merged in.  buf: the 1-d uint8 CUDA tensor whose first bytes are this archive
        -- the same data_ptr() as the opened tensor and at least its numel(), else ValueError; default: the opened tensor itself.
        The new archive may grow into the room behind the old one, up to buf.numel().  On success this object stays open on the
        view and describes the new archive: no reopen.  Every refusal (rc != 0 other than CSCMI_DEVICE_ERROR) leaves buf and this
        object as they were; there is nothing to reallocate, so nothing is tried twice."""
        import torch
        if buf is None:
            buf = self._arc
        if not _is_bytes_tensor(buf):
            raise TypeError("buf: a contiguous 1-d torch.uint8 CUDA tensor")
        if buf.data_ptr() != self._arc.data_ptr() or buf.numel() < self._arc.numel():
            raise ValueError("buf: it begins at the opened archive's first byte and is at least as large")
        files, table = [], (CSADevSlice * max(len(entries), 1))()
        for a, e in zip(table, entries):
            t = e["tensor"]
            if not (t is None or _is_bytes_tensor(t)):
                raise TypeError("tensor: a contiguous 1-d torch.uint8 CUDA tensor, or None")
            s = e.get("slice") or ((0, int(t.numel())) if t is not None else (0, 0, 0, 0))
            a.offset, a.run, a.stride, a.count = (s[0], s[1], s[1], 1 if s[1] else 0) if len(s) == 2 else s
            files.append({"name": e["name"], "esize": a.run * a.count if a.count else 0, "edate": e["edate"], "eattr": e["eattr"]})
        if base_digests is not None and not _is_digest_table(base_digests):
            raise TypeError("base_digests: a contiguous torch.uint8 CUDA tensor [n, 32]")
        live = [e["tensor"] for e in entries]                      # alive across the call
        ptrs = (C.c_void_p * max(len(live), 1))(*[t.data_ptr() if t is not None and t.numel() else None for t in live])
        sizes = (C.c_uint64 * max(len(live), 1))(*[0 if t is None else int(t.numel()) for t in live])
        out = None
        if _is_digest_table(digests):
            out = digests
        elif digests is not False and digests is not None:
            if digests is not True:
                raise TypeError("digests: True, or a contiguous torch.uint8 CUDA tensor [n, 32] to write the table into")
            rc, out = _digest_table(files, arcname, buf.device, opts)
            if rc != 0:
                return rc, None, {"files": []}
        rc, nt, _, _ = device_write_plan(files, arcname, **opts)
        if rc != 0:
            return rc, None, {"files": []}
        flags = (CSAMI_UPDATE_TRUST_SUMS if trust_sums else 0) | (CSAMI_UPDATE_TRUST_DIGESTS if trust_digests else 0)
        o = options(**opts)
        st, gs, us, ds, ms = CSADevWriteStats(), CSADevGatherStats(), CSADevUpdateStats(), CSADevDigestStats(), CSADevMoveStats()
        tasks = (CSADevUpdateTask * max(nt, 1))()
        arr, keep = _write_table(files)
        torch.cuda.synchronize()                   # the buffers were filled on torch's stream, the library launches on its own
        rc = lib().CSAMI_DeviceUpdateInPlace(
            self._h, int(buf.numel()), None if base_digests is None else C.c_void_p(base_digests.data_ptr() or 0),
            0 if base_digests is None else int(base_digests.shape[0]), ptrs, sizes, table, arr, len(keep), arcname.encode(), flags, C.byref(o),
            C.byref(st), C.byref(gs), C.byref(us), tasks, nt, None if out is None else C.c_void_p(out.data_ptr() or 0),
            0 if out is None else int(out.shape[0]), C.byref(ds), C.byref(ms))
        d = {}
        for x in (st, gs, us, ds, ms):
            d.update(x.as_dict())
        d["files"] = [_file_dict(a, f["name"]) for a, f in zip(arr, files)]
        d["tasks"] = [t.as_dict() for t in tasks[:min(nt, int(st.tasks))]]
        if out is not None:
            d["digests"] = out
        if rc != 0:
            return rc, None, d
        self._buf = buf                                # (the view's storage)
        self._arc = buf[:st.archive_bytes]
        return rc, self._arc, d

    def _by(self, bufs, names, take):
        """the selection's files table and, per entry of it, the caller's base buffer, its address and size, and the slice of it (None,
        count 0: verified only).  take(b) -> (base tensor, slice or None: none is set) for a value of bufs that is not None.
        KeyError for a key that is no selected entry."""
        files = self.plan(names)[0]
        bufs = dict(bufs)
        unknown = set(bufs) - {f["name"] for f in files}
        if unknown:
            raise KeyError(sorted(unknown)[0])
        live, table = [], (CSADevSlice * max(len(files), 1))()
        for a, f in zip(table, files):
            b = bufs.get(f["name"])
            if b is not None:
                b, s = take(b)
                if s is not None:
                    a.offset, a.run, a.stride, a.count = (s[0], s[1], s[1], 1 if s[1] else 0) if len(s) == 2 else s
            live.append(b)
        # (an empty tensor may have no address: it stands for itself with the archive's, which a range of size 0 never overlaps)
        ptrs = (C.c_void_p * max(len(live), 1))(*[None if t is None else (t.data_ptr() or self._arc.data_ptr()) for t in live])
        sizes = (C.c_uint64 * max(len(live), 1))(*[0 if t is None else int(t.numel()) for t in live])
        return files, live, ptrs, sizes, table

    def _by_name(self, bufs, names):
        """the selection's files table and, per entry of it, the caller's tensor (None: verified only).  KeyError for a key that is
        no selected entry."""
        def take(t):
            if not _is_bytes_tensor(t):
                raise TypeError("a contiguous 1-d torch.uint8 CUDA tensor, or None")
            return t, None
        return self._by(bufs, names, take)[:4]

    def _by_slice(self, bufs, names):
        """the selection's files table and, per entry of it, the caller's base buffer and the slice of it (None, count 0: verified
        only).  bufs: {stored name: (1-d contiguous torch.uint8 CUDA base tensor, (offset, length) | (offset, run, stride, count)) |
        any CUDA tensor tensor_slice takes | None}.  KeyError for a key that is no selected entry."""
        import torch

        def take(b):
            t, s = tensor_slice(b) if isinstance(b, torch.Tensor) else b
            if not _is_bytes_tensor(t):
                raise TypeError("a CUDA tensor, or (a contiguous 1-d torch.uint8 CUDA tensor, slice), or None")
            return t, s
        return self._by(bufs, names, take)

    def _call(self, fn, names, files, args, stop_early, opts, extra=(), compare=False):
        """One read call over buffers of the caller's: fn(handle, names, *args, number of entries, flags, options, files table[, diffs],
        read statistics, stop statistics, *extra) -> (rc, stats dict with `extra`'s merged in and the files table, {name: diff} or None)"""
        import torch
        arr, n = _names(names)
        table, st, ss, o = (CSADevFile * max(len(files), 1))(), CSADevReadStats(), CSADevStopStats(), options(**opts)
        diffs = (CSADevDiff * max(len(files), 1))() if compare else None
        torch.cuda.synchronize()
        rc = fn(self._h, arr, n, *args, len(files), CSAMI_DEV_STOP_EARLY if stop_early else 0, C.byref(o), table,
                *([diffs] if compare else []), C.byref(st), C.byref(ss), *[C.byref(x) for x in extra])
        out = st.as_dict()
        if stop_early:
            out.update(ss.as_dict())
        for x in extra:
            out.update(x.as_dict())
        out["files"] = [_file_dict(f, C.string_at(f.name).decode("latin-1")) if f.name else g for f, g in zip(table, files)]
        return rc, out, ({f["name"]: d.as_dict() for f, d in zip(files, diffs)} if compare else None)

    def extract_into(self, dsts, names: Sequence[str] = (), stop_early=False, **opts):
        """`csarc x` into tensors of the caller's (CSAMI_DeviceReadInto) -> (rc, stats dict); stats["files"] as in extract.
        dsts: {stored name: 1-d contiguous torch.uint8 CUDA tensor of at least the entry's size, or None}; a selected entry that is
        absent or None is verified only.  The tensors must not overlap each other or the archive."""
        files, live, ptrs, caps = self._by_name(dsts, names)
        return self._call(lib().CSAMI_DeviceReadInto, names, files, (ptrs, caps), stop_early, opts)[:2]

    def extract_slices(self, slices, dsts=None, names: Sequence[str] = (), stop_early=True, **opts):
        """byte ranges and strided slices of entries (CSAMI_DeviceReadSlices) -> (rc, {name: uint8 CUDA tensor of the packed slice},
        stats dict); stats["files"] as in extract, and the slice statistics beside the read's.  slices: {stored name: (offset,
        length) | (offset, run, stride, count)} -- rows_slice makes them for a matrix; a selected entry without a key is not read at
        all.  dsts: as in extract_into, except that a sliced entry that is absent gets a tensor allocated here; None: its touched
        fragments are verified only.  A tensor needs at least run * count bytes and the result is its front of that size."""
        import torch
        files = self.plan(names)[0]
        table = _slice_table(files, slices)
        given = dict(dsts or {})
        for f, s in zip(files, table):
            if f["name"] not in given and s.count:
                given[f["name"]] = torch.empty(s.run * s.count, dtype=torch.uint8, device=self._arc.device)
        files, live, ptrs, caps = self._by_name(given, names)
        rc, out, _ = self._call(lib().CSAMI_DeviceReadSlices, names, files, (table, ptrs, caps), stop_early, opts, (CSADevSliceStats(),))
        got = {f["name"]: t[:s.run * s.count] for f, t, s in zip(files, live, table) if t is not None and s.count and rc != WRITE_ERROR}
        return rc, got, out

    def compare(self, srcs, names: Sequence[str] = (), stop_early=False, **opts):
        """`csarc t` and a byte-for-byte comparison with tensors of the caller's in one pass (CSAMI_DeviceCompare) ->
        (rc, {name: {"status", "first_diff", "failed_frags"}}, stats dict).  srcs: as dsts of extract_into; the tensors are only read
        and may alias each other.  status: 0 or a sum of CSA_DIFF_*; first_diff: NO_DIFF without CSA_DIFF_BYTES.  rc is the
        archive's health, as test returns it."""
        files, live, ptrs, sizes = self._by_name(srcs, names)
        rc, out, diffs = self._call(lib().CSAMI_DeviceCompare, names, files, (ptrs, sizes), stop_early, opts, compare=True)
        return rc, diffs, out

    def extract_into_slices(self, dsts, names: Sequence[str] = (), stop_early=False, **opts):
        """`csarc x` into strided slices of buffers of the caller's (CSAMI_DeviceReadIntoSlices), the way back of write_slices ->
        (rc, stats dict); stats["files"] as in extract, and the spread statistics beside the read's.  dsts: {stored name: (base
        tensor, slice) as write_slices takes them | a CUDA tensor of any dtype that tensor_slice takes -- contiguous, or a view such
        as t2d[:, c0:c1] | None}; a selected entry that is absent or None is verified only.  The entry's packed bytes go to the bytes
        the slice selects, which must be at least the entry's size; nothing else of the buffer is stored to.  The selections must not
        meet each other -- their hulls may interleave, as the column blocks of one matrix do -- and no hull may overlap the archive."""
        files, live, ptrs, sizes, slices = self._by_slice(dsts, names)
        return self._call(lib().CSAMI_DeviceReadIntoSlices, names, files, (ptrs, sizes, slices), stop_early, opts, (CSADevSpreadStats(),))[:2]

    def compare_slices(self, srcs, names: Sequence[str] = (), stop_early=False, **opts):
        """compare against strided slices of buffers of the caller's (CSAMI_DeviceCompareSlices) -> (rc, diffs, stats dict), shaped as
        compare returns them, with the spread statistics beside the read's.  srcs: as dsts of extract_into_slices; the buffers are only
        read and may alias each other.  CSA_DIFF_SIZE: the slice does not select exactly the entry's size; first_diff is a packed
        offset in the entry."""
        files, live, ptrs, sizes, slices = self._by_slice(srcs, names)
        rc, out, diffs = self._call(lib().CSAMI_DeviceCompareSlices, names, files, (ptrs, sizes, slices), stop_early, opts,
                                    (CSADevSpreadStats(),), compare=True)
        return rc, diffs, out

    def kernel_ms(self):
        """HIP-event milliseconds of the last extract / test by kernel: (k_gather_extents, k_frag_pieces, k_frag_fold); after compare:
        (k_gather_extents, k_frag_compare, k_frag_fold_diff); k_frag_spread / k_frag_compare_rows in slot [1] where a wave of
        extract_into_slices / compare_slices ran them"""
        ms = (C.c_double * 3)()
        lib().CSAMI_DeviceKernelMs(self._h, ms)
        return tuple(ms)

    def close(self):
        if self._h:
            lib().CSAMI_DeviceClose(self._h)
            self._h = None
        self._arc = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
