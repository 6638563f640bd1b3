"""Device-resident decode and encode: ctypes mirrors of CSCMI_DecodeDeviceBatch(Stop) / CSCMI_EncodeDeviceBatch
(include/csc_mi355x.h) and a torch front end for each.

The streams lie in device memory and the raw bytes stay there: torch is the plumbing (allocation, upload of `bytes`
inputs), the decoding is the library's k_decode_dev* kernels, the encoding its encode kernels and k_frame_blocks.  Nothing
here decodes or encodes, and nothing falls back to the callback paths."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple, Union

from .capi import CSC_PROP_SIZE, CSCProps, CscLib

CSCMI_DEVICE_ERROR = -95
CSCMI_NO_DECODER = -92
CSCMI_NO_ENCODER = -91


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


def bind_stop(lib: CscLib):
    fn = lib.lib.CSCMI_DecodeDeviceBatchStop
    fn.argtypes = [C.c_int, C.POINTER(CSCMIDevDecode), C.POINTER(C.c_uint64), C.POINTER(CSCMIDevDecodeOpts),
                   C.POINTER(CSCMIDevDecodeStats)]
    fn.restype = C.c_int
    return fn


NO_STOP = (1 << 64) - 1     # stop_at[i] of a stream that is decoded to its end


def default_cap(stream_len: int) -> int:
    """the destination size decode_device gives a stream when the caller names none: 64 bytes per stream byte, 1 MiB at least"""
    return max(1 << 20, 64 * stream_len)


def decode_device(lib: CscLib, streams: Sequence, *, caps: Union[None, int, Sequence[int]] = None, launch_bytes: int = 0,
                  dsts: Optional[Sequence] = None,
                  stop_at: Union[None, int, Sequence[Optional[int]]] = None) -> Tuple[List[tuple], CSCMIDevDecodeStats]:
    """Decode whole streams (each with its 10 property bytes) on the current device, all in ONE CSCMI_DecodeDeviceBatch call
    (CSCMI_DecodeDeviceBatchStop where stop_at is given).

    streams       a list of `bytes` (uploaded here, in one copy) or of contiguous torch.uint8 CUDA tensors (used in place)
    caps          destination bytes per stream: one int for all, or one per stream.  A stream does not say how long its raw
                  bytes are, and a first pass that asks for nothing would decode everything twice, so the size is the
                  CALLER's: with caps=None each destination gets default_cap(len(stream)), and a stream that needs more ends
                  with WRITE_ERROR and the runs that fitted -- call again with a larger cap.
    dsts          instead of caps: the torch.uint8 CUDA tensors to decode into (cap = their size); any alignment
    launch_bytes  output per stream after which a launch returns (0 = the library's default)
    stop_at       raw bytes wanted per stream: one int for all, or one per stream (None: to its end).  The decoder stops once
                  they are delivered -- rc 0, the view is dst[:produced], nothing behind the position is decoded, `consumed` is
                  informative.  With caps=None a stopped stream's destination is min(default_cap(len(stream)), its stop).

    Returns ([(rc, tensor_view_of_the_produced_bytes, consumed)], stats); rc is CSCDec_Decode's code for that stream, or
    CSCMI_NO_DECODER where CSCDec_Create would have refused it.  Raises RuntimeError if the call itself fails."""
    import torch
    n = len(streams)
    stops = None
    if stop_at is not None:
        stop_at = [stop_at] * n if isinstance(stop_at, int) else list(stop_at)
        if len(stop_at) != n:
            raise ValueError("one stop per stream")
        stops = (C.c_uint64 * max(n, 1))(*[NO_STOP if s is None else int(s) for s in stop_at])
        call, what = bind_stop(lib), "CSCMI_DecodeDeviceBatchStop"

        def fn(k, jobs, opts, st):
            return call(k, jobs, stops, opts, st)
    else:
        fn, what = bind(lib), "CSCMI_DecodeDeviceBatch"
    stats = CSCMIDevDecodeStats()
    if n == 0:
        rc = fn(0, None, None, C.byref(stats))
        if rc != 0:
            raise RuntimeError(f"{what}: {rc}")
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
            if stops is not None:
                caps = [min(c, int(s)) for c, s in zip(caps, stops)]
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
        raise RuntimeError(f"{what}: {rc}")
    del keep
    return [(int(j.rc), d[:int(j.produced)], int(j.consumed)) for j, d in zip(jobs, dsts)], stats


# ---- encode ----------------------------------------------------------------------------------------------------------

class CSCMIDevEncode(C.Structure):
    _fields_ = [("props", CSCProps), ("src", C.c_void_p), ("src_size", C.c_size_t), ("dst", C.c_void_p),
                ("dst_cap", C.c_size_t), ("produced", C.c_size_t), ("rc", C.c_int)]


class CSCMIDevEncodeStats(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("rounds", C.c_uint64), ("readback_bytes", C.c_uint64), ("kernel_ms", C.c_double)]


def bind_encode(lib: CscLib):
    fn = lib.lib.CSCMI_EncodeDeviceBatch
    fn.argtypes = [C.c_int, C.POINTER(CSCMIDevEncode), C.POINTER(CSCMIDevEncodeStats)]
    fn.restype = C.c_int
    return fn


def default_enc_cap(n: int) -> int:
    """the room encode_device gives the stream of an n-byte input behind its property bytes when the caller names none.  A
    convenience, not a bound: a stream that needs more ends with WRITE_ERROR -- call again with a larger cap."""
    return n + n // 4 + (1 << 20)


def encode_device(lib: CscLib, inputs: Sequence, *, props=None, level: int = 2, dict_size: int = 64000000,
                  caps: Union[None, int, Sequence[int]] = None, dsts: Optional[Sequence] = None) -> Tuple[List[tuple], CSCMIDevEncodeStats]:
    """Encode whole inputs on the current device, all in ONE CSCMI_EncodeDeviceBatch call; the streams stay in device memory.

    inputs     a list of `bytes` (uploaded here, in one copy) or of contiguous 1-d torch.uint8 CUDA tensors (used in place)
    props      one CSCProps for all, or one per input; without it props_init(min(dict_size, len), level), as capi.encode does
    caps       bytes per stream BEHIND its 10 property bytes: one int for all, or one per input (None: default_enc_cap(len)).
               Each destination is allocated with the 10 bytes in front, and the property bytes are copied there.
    dsts       instead of caps: the torch.uint8 CUDA tensors that receive the streams behind their property bytes (cap = their
               size, any alignment); the caller writes the property bytes itself

    Returns ([(rc, stream_tensor)], stats).  With caps, stream_tensor is the whole stream -- property bytes and the `produced`
    bytes -- in device memory, which decode_device accepts in place; with dsts it is the view dst[:produced].  rc is what
    CSCEnc_Encode + CSCEnc_Encode_Flush give (0 or WRITE_ERROR), or CSCMI_NO_ENCODER where CSCEnc_Create would have refused the
    props.  Raises RuntimeError if the call itself fails."""
    import torch
    fn = bind_encode(lib)
    n = len(inputs)
    stats = CSCMIDevEncodeStats()
    if n == 0:
        rc = fn(0, None, C.byref(stats))
        if rc != 0:
            raise RuntimeError(f"CSCMI_EncodeDeviceBatch: {rc}")
        return [], stats
    dev = torch.device("cuda", torch.cuda.current_device())
    lens = [len(s) if isinstance(s, (bytes, bytearray, memoryview)) else int(s.numel()) for s in inputs]
    srcs, keep = [], []
    if all(isinstance(s, (bytes, bytearray, memoryview)) for s in inputs):
        flat = torch.frombuffer(bytearray(b"".join(bytes(s) for s in inputs)) or bytearray(1), dtype=torch.uint8).to(dev)
        keep.append(flat)
        off = 0
        for ln in lens:
            srcs.append(flat.data_ptr() + off)
            off += ln
    else:
        for s in inputs:
            if not (isinstance(s, torch.Tensor) and s.dtype == torch.uint8 and s.is_cuda and s.is_contiguous() and s.dim() == 1):
                raise TypeError("inputs: all bytes, or all contiguous 1-d torch.uint8 CUDA tensors")
            srcs.append(s.data_ptr())
    if props is None:
        props = [lib.props_init(min(dict_size, ln), level) for ln in lens]
    elif isinstance(props, CSCProps):
        props = [props] * n
    if len(props) != n:
        raise ValueError("one CSCProps per input")
    whole = None
    if dsts is None:
        if caps is None:
            caps = [default_enc_cap(ln) for ln in lens]
        elif isinstance(caps, int):
            caps = [caps] * n
        if len(caps) != n:
            raise ValueError("one cap per input")
        # every stream in one allocation, its property bytes in front (one upload for all of them)
        offs, total = [], 0
        for c in caps:
            offs.append(total)
            total += CSC_PROP_SIZE + int(c)
        pool = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        heads = torch.frombuffer(bytearray(b"".join(lib.write_properties(p) for p in props)), dtype=torch.uint8).to(dev)
        where = (torch.tensor(offs, dtype=torch.int64).unsqueeze(1) + torch.arange(CSC_PROP_SIZE, dtype=torch.int64)).reshape(-1)
        pool[where.to(dev)] = heads
        whole = [pool[o:o + CSC_PROP_SIZE + int(c)] for o, c in zip(offs, caps)]
        dsts = [w[CSC_PROP_SIZE:] for w in whole]
    if len(dsts) != n:
        raise ValueError("one destination per input")
    jobs = (CSCMIDevEncode * n)()
    for j, p, src, ln, d in zip(jobs, props, srcs, lens, dsts):
        j.props = p
        j.src = src
        j.src_size = ln
        j.dst = d.data_ptr()
        j.dst_cap = int(d.numel())
        j.rc = 0
    torch.cuda.synchronize()                  # the uploads ran on torch's stream, the library launches on its own
    rc = fn(n, jobs, C.byref(stats))
    if rc != 0:
        raise RuntimeError(f"CSCMI_EncodeDeviceBatch: {rc}")
    del keep
    if whole is not None:
        return [(int(j.rc), w[:CSC_PROP_SIZE + int(j.produced)]) for j, w in zip(jobs, whole)], stats
    return [(int(j.rc), d[:int(j.produced)]) for j, d in zip(jobs, dsts)], stats
