"""Device-resident decode: ctypes mirror of CSCMI_DecodeDeviceBatch (include/csc_mi355x.h) and a torch front end.

The streams lie in device memory and the raw bytes stay there: torch is the plumbing (allocation, upload of `bytes`
inputs), the decoding is the library's k_decode_dev* kernels.  Nothing here decodes, and nothing falls back to the
callback path."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple, Union

from .capi import CSC_PROP_SIZE, CSCProps, CscLib

CSCMI_DEVICE_ERROR = -95
CSCMI_NO_DECODER = -92


class CSCMIDevDecode(C.Structure):
    _fields_ = [("props", CSCProps), ("src", C.c_void_p), ("src_size", C.c_size_t), ("dst", C.c_void_p),
                ("dst_cap", C.c_size_t), ("produced", C.c_size_t), ("consumed", C.c_size_t), ("rc", C.c_int)]


class CSCMIDevDecodeOpts(C.Structure):
    _fields_ = [("launch_bytes", C.c_uint64)]


class CSCMIDevDecodeStats(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("rounds", C.c_uint64), ("kernel_ms", C.c_double)]


def bind(lib: CscLib):
    fn = lib.lib.CSCMI_DecodeDeviceBatch
    fn.argtypes = [C.c_int, C.POINTER(CSCMIDevDecode), C.POINTER(CSCMIDevDecodeOpts), C.POINTER(CSCMIDevDecodeStats)]
    fn.restype = C.c_int
    return fn


def default_cap(stream_len: int) -> int:
    """the destination size decode_device gives a stream when the caller names none: 64 bytes per stream byte, 1 MiB at least"""
    return max(1 << 20, 64 * stream_len)


def decode_device(lib: CscLib, streams: Sequence, *, caps: Union[None, int, Sequence[int]] = None, launch_bytes: int = 0,
                  dsts: Optional[Sequence] = None) -> Tuple[List[tuple], CSCMIDevDecodeStats]:
    """Decode whole streams (each with its 10 property bytes) on the current device, all in ONE CSCMI_DecodeDeviceBatch call.

    streams       a list of `bytes` (uploaded here, in one copy) or of contiguous torch.uint8 CUDA tensors (used in place)
    caps          destination bytes per stream: one int for all, or one per stream.  A stream does not say how long its raw
                  bytes are, and a first pass that asks for nothing would decode everything twice, so the size is the
                  CALLER's: with caps=None each destination gets default_cap(len(stream)), and a stream that needs more ends
                  with WRITE_ERROR and the runs that fitted -- call again with a larger cap.
    dsts          instead of caps: the torch.uint8 CUDA tensors to decode into (cap = their size); any alignment
    launch_bytes  output per stream after which a launch returns (0 = the library's default)

    Returns ([(rc, tensor_view_of_the_produced_bytes, consumed)], stats); rc is CSCDec_Decode's code for that stream, or
    CSCMI_NO_DECODER where CSCDec_Create would have refused it.  Raises RuntimeError if the call itself fails."""
    import torch
    fn = bind(lib)
    n = len(streams)
    stats = CSCMIDevDecodeStats()
    if n == 0:
        rc = fn(0, None, None, C.byref(stats))
        if rc != 0:
            raise RuntimeError(f"CSCMI_DecodeDeviceBatch: {rc}")
        return [], stats
    dev = torch.device("cuda", torch.cuda.current_device())
    lens = [len(s) if isinstance(s, (bytes, bytearray, memoryview)) else int(s.numel()) for s in streams]
    heads, srcs, keep = [], [], []
    if all(isinstance(s, (bytes, bytearray, memoryview)) for s in streams):
        flat = torch.frombuffer(bytearray(b"".join(bytes(s) for s in streams)) or bytearray(1), dtype=torch.uint8).to(dev)
        keep.append(flat)
        off = 0
        for s, ln in zip(streams, lens):
            heads.append(bytes(s[:CSC_PROP_SIZE]))
            srcs.append(flat.data_ptr() + off + CSC_PROP_SIZE)
            off += ln
    else:
        for s in streams:
            if not (isinstance(s, torch.Tensor) and s.dtype == torch.uint8 and s.is_cuda and s.is_contiguous() and s.dim() == 1):
                raise TypeError("streams: all bytes, or all contiguous 1-d torch.uint8 CUDA tensors")
            heads.append(bytes(s[:CSC_PROP_SIZE].cpu().numpy().tobytes()))
            srcs.append(s.data_ptr() + CSC_PROP_SIZE)
    if dsts is None:
        if caps is None:
            caps = [default_cap(ln) for ln in lens]
        elif isinstance(caps, int):
            caps = [caps] * n
        dsts = [torch.empty(max(int(c), 1), dtype=torch.uint8, device=dev)[:int(c)] for c in caps]
    if len(dsts) != n:
        raise ValueError("one destination per stream")
    jobs = (CSCMIDevDecode * n)()
    for j, head, src, ln, d in zip(jobs, heads, srcs, lens, dsts):
        # (a stream shorter than its property bytes: CSCDec_ReadProperties has nothing to read; the caller's Create sees an empty source)
        j.props = lib.read_properties(head.ljust(CSC_PROP_SIZE, b"\0"))
        j.src = src
        j.src_size = max(0, ln - CSC_PROP_SIZE)
        j.dst = d.data_ptr()
        j.dst_cap = int(d.numel())
        j.rc = 0
    torch.cuda.synchronize()                  # the uploads ran on torch's stream, the library launches on its own
    opts = CSCMIDevDecodeOpts(int(launch_bytes))
    rc = fn(n, jobs, C.byref(opts), C.byref(stats))
    if rc != 0:
        raise RuntimeError(f"CSCMI_DecodeDeviceBatch: {rc}")
    del keep
    return [(int(j.rc), d[:int(j.produced)], int(j.consumed)) for j, d in zip(jobs, dsts)], stats
