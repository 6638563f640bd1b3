"""GPU tier for the stop position of the device-resident decode (CSCMI_DecodeDeviceBatchStop, csc_amd.device.decode_device(stop_at=)):
a stream is wanted only its first stop_at raw bytes of; the run that reaches the position is delivered clipped to it and nothing
behind it is decoded.

The checker (soak_gen.checker(): the reference build where oracle/_ref has it, the oracle otherwise) decodes the intact stream
once per module with a writer that records its Write sizes -- those are the run boundaries -- and the wanted answer for every stop
is the prefix of those bytes.  Every case is one stream of at most 600 KB; the stops of a case share ONE batch call."""
import ctypes as C

import pytest

import cases
import soak_gen
from csc_amd.capi import CSC_WRITE_ABORT, BytesWriter, WRITE_ERROR
from csc_amd.device import CSCMI_NO_DECODER, NO_STOP, decode_device

pytestmark = pytest.mark.gpu

# every block type the generators reach: RLE zeros, text through the dictionary filter, exe, delta, normal, entropy, bad; the
# incompressible kinds last, so that the first runs lie in the first third of the coded stream
MIX = [["zeros", 60000], ["text", 21, 0, 120000], ["exe", 22, 0, 90000], ["delta", 23, 0, 80000], ["pattern", "00", 40000],
       ["text", 26, 0, 70000], ["entropy8", 25, 0, 50000], ["random", 24, 0, 30000]]
# the window_wrap_32k geometry: a dictionary smaller than the input, so that a clipped delivery meets a window that has wrapped
WRAP = [["text", 7, 0, 300000], ["exe", 8, 0, 150000]]
OFFSETS = (0, 1, 15)
GUARD = 64
_memo = {}


def _chk():
    if "chk" not in _memo:
        _memo["chk"] = soak_gen.checker()
    return _memo["chk"][:2]


class WantFirst(BytesWriter):
    """the writer the call is specified against: wants the first `stop` bytes, answers CSC_WRITE_ABORT once it has them"""

    def __init__(self, stop):
        super().__init__()
        self.stop = stop

    def _write(self, p, buf, size):
        self.sizes.append(size)
        self.out += C.string_at(buf, min(size, self.stop - len(self.out)))
        return CSC_WRITE_ABORT if len(self.out) >= self.stop else size


class AbortLate(BytesWriter):
    """the callback path's writer (csa_archive.cpp, FragSink): takes the run that reaches `stop` whole and aborts the Write after it"""

    def __init__(self, stop):
        super().__init__()
        self.stop = stop

    def _write(self, p, buf, size):
        self.sizes.append(size)
        if len(self.out) >= self.stop:
            return CSC_WRITE_ABORT
        self.out += C.string_at(buf, size)
        return size


def _case(name):
    """-> (stream, raw bytes, run boundaries b0 < b1 < ... < T), built and decoded by the checker once"""
    if name not in _memo:
        chk, za = _chk()
        if name == "mix":
            data, p = cases.build(MIX), chk.props_init(1 << 20, 2)
        else:
            data, p = cases.build(WRAP), chk.props_init(32768, 2)
            p.dict_size = 32768
            p.raw_blocksize = 65536
        p.csc_blocksize = 4096
        rc, s = chk.encode(data, props=p, alloc=za)
        w = BytesWriter()
        rcd, out = chk.decode(s, alloc=za, writer=w)
        assert rc == 0 and rcd == 0 and out == data and len(data) <= 600000 and len(w.sizes) >= 5
        bounds, acc = [], 0
        for n in w.sizes:
            acc += n
            bounds.append(acc)
        _memo[name] = (s, data, bounds)
    return _memo[name]


def _run(prod, streams, stops, caps, offsets=None, launch_bytes=0):
    """one batch call; job i decodes into a canary-filled allocation of its own, offsets[i] bytes in.
    -> ([(rc, bytes, consumed)], stats); the canaries in front, behind `produced` and behind the cap are checked here"""
    import torch
    offsets = offsets or [0] * len(streams)
    bufs = [torch.full((GUARD + o + c + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for o, c in zip(offsets, caps)]
    dsts = [b[GUARD + o:GUARD + o + c] for b, o, c in zip(bufs, offsets, caps)]
    res, stats = decode_device(prod, streams, dsts=dsts, stop_at=stops, launch_bytes=launch_bytes)
    out = []
    for (rc, view, consumed), b, o in zip(res, bufs, offsets):
        host = b.cpu().numpy().tobytes()
        n = int(view.numel())
        assert host[:GUARD + o] == b"\xa5" * (GUARD + o), "a byte in front of dst was written"
        assert host[GUARD + o + n:] == b"\xa5" * (len(host) - GUARD - o - n), "a byte behind `produced` was written"
        out.append((rc, host[GUARD + o:GUARD + o + n], consumed))
    return out, stats


def _stops(bounds):
    T = bounds[-1]
    inside = [(a + b) // 2 for a, b in zip([0] + bounds[:-1], bounds)]              # a position inside every run
    b0, b1 = bounds[0], bounds[1]
    return sorted(set([0, 1, b0 - 1, b0, b0 + 1, b1, T - 1, T, T + 1, NO_STOP] + inside + bounds))


# ---- 1. every stop position, three destination alignments ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["mix", "wrap"])
def test_stop_positions(prod, name):
    s, data, bounds = _case(name)
    T = bounds[-1]
    jobs = [(stop, off) for stop in _stops(bounds) for off in OFFSETS]
    got, _ = _run(prod, [s] * len(jobs), [j[0] for j in jobs], [T + 33] * len(jobs), [j[1] for j in jobs])
    for (stop, off), (rc, out, consumed) in zip(jobs, got):
        want = data[:min(stop, T)]
        assert rc == 0 and len(out) == len(want) and out == want, (name, stop, off, rc, len(out))
        assert consumed <= len(s) - 10
    if name == "wrap":
        assert T > 32768 * 4 and any(32768 < stop < T and stop not in bounds for stop, _ in jobs)


# ---- 2. no stop is the plain call -----------------------------------------------------------------------------------------

def test_no_stop_equals_the_plain_call(prod):
    s, data, bounds = _case("mix")
    T = bounds[-1]
    streams = [s, s, s[:len(s) // 2], s[:len(s) - 1], s]
    caps = [T, T + 7, T, T, bounds[2] + 5]
    plain, _ = _run(prod, streams, None, caps)                                       # stop_at == NULL: CSCMI_DecodeDeviceBatch
    assert plain[0] == (0, data, len(s) - 10) and plain[2][0] != 0 and plain[3][0] != 0 and plain[4] == (WRITE_ERROR, data[:bounds[2]], plain[4][2])
    for stop in (NO_STOP, T + 1, T):
        got, _ = _run(prod, streams, [stop] * len(streams), caps)
        # (a stream cut behind its last run reaches T and stops there with 0, where the plain call goes on into the damage:
        # at stop == T the two cut streams are left to test_damage_behind_the_stop_is_not_decoded)
        same = range(len(streams)) if stop > T else (0, 1, 4)
        assert [got[i] for i in same] == [plain[i] for i in same], stop
    none, _ = _run(prod, streams, [None] * len(streams), caps)
    assert none == plain


# ---- 3. capacities ------------------------------------------------------------------------------------------------------

def test_capacity_against_stop(prod):
    s, data, bounds = _case("mix")
    T = bounds[-1]
    chk, za = _chk()
    k = 3
    mid = (bounds[k - 1] + bounds[k]) // 2                                            # inside run 3
    rows = [(mid, mid), (mid, mid - 1), (bounds[k], bounds[k]), (bounds[k], bounds[k] - 1), (1, 1), (1, 0), (T, T), (T, T - 1),
            (mid + 10, mid), (T + 1, bounds[1] + 1), (NO_STOP, bounds[0])]           # (stop_at, dst_cap)
    got, _ = _run(prod, [s] * len(rows), [r[0] for r in rows], [r[1] for r in rows])
    for (stop, cap), (rc, out, _) in zip(rows, got):
        if cap >= min(stop, T):                                                       # dst_cap == stop_at succeeds
            assert (rc, out) == (0, data[:min(stop, T)]), (stop, cap)
        elif stop > cap + 1 or stop > T:                                              # stop_at > dst_cap: the plain call with that cap
            rcw, want = chk.decode(s, alloc=za, writer=BytesWriter(fail_after=cap))
            assert rcw == WRITE_ERROR and (rc, out) == (rcw, bytes(want)), (stop, cap)
        else:                                                                         # dst_cap == stop_at - 1: exactly the earlier runs
            earlier = max([b for b in bounds if b < stop], default=0)
            assert (rc, out) == (WRITE_ERROR, data[:earlier]), (stop, cap)


# ---- 4. the stop holds across launches -------------------------------------------------------------------------------------

def test_one_run_per_launch(prod):
    s, data, bounds = _case("mix")
    stop = (bounds[1] + bounds[2]) // 2                                               # in the third run
    (whole,), st_all = _run(prod, [s], [NO_STOP], [bounds[-1]], launch_bytes=1)
    (got,), st = _run(prod, [s], [stop], [stop], launch_bytes=1)
    (one,), st_one = _run(prod, [s], [stop], [stop], launch_bytes=1 << 30)
    assert whole[:2] == (0, data) and st_all.launches == len(bounds) + 1               # a launch per run, and one that finds the end
    assert got[:2] == one[:2] == (0, data[:stop])
    assert st.launches == 3 < st_all.launches and st_one.launches == 1                 # a stopped stream is not launched again
    (edge,), st_edge = _run(prod, [s], [bounds[1]], [bounds[1]], launch_bytes=1)
    assert edge[:2] == (0, data[:bounds[1]]) and st_edge.launches == 2                 # ... nor one that stopped at a run's end


def test_default_destination_is_no_larger_than_the_stop(prod):
    s, data, bounds = _case("mix")
    res, _ = decode_device(prod, [s, s, s], stop_at=[100, None, 0])                   # caps=None: min(default_cap, stop) bytes each
    assert [(rc, int(t.numel())) for rc, t, _ in res] == [(0, 100), (0, len(data)), (0, 0)]
    assert bytes(res[0][1].cpu().numpy().tobytes()) == data[:100]
    assert res[0][1].untyped_storage().nbytes() <= 512 and res[1][1].untyped_storage().nbytes() >= len(data)
    res, _ = decode_device(prod, [s], stop_at=bounds[0] + 3, launch_bytes=1)           # one int for all
    assert (res[0][0], bytes(res[0][1].cpu().numpy().tobytes())) == (0, data[:bounds[0] + 3])


# ---- 5. it really stops -------------------------------------------------------------------------------------------------

def test_damage_behind_the_stop_is_not_decoded(prod):
    s, data, bounds = _case("mix")
    chk, za = _chk()
    b0 = bounds[0]
    damaged = {"tail overwritten": s[:-64] + b"\x5a" * 64, "last third cut off": s[:len(s) * 2 // 3]}
    for what, bad in damaged.items():
        # the input is honest: decoded to its end the stream fails, and the checker -- with the writer the call is specified
        # against, and with one that aborts a Write later, so one run more -- returns 0 for these stops
        assert chk.decode(bad, alloc=za, writer=BytesWriter())[0] != 0, what
        for stop in (b0, b0 + 1):
            w = WantFirst(stop)
            rc, out = chk.decode(bad, alloc=za, writer=w)
            assert rc == 0 and bytes(out) == data[:stop], (what, stop)
            w = AbortLate(stop)
            assert chk.decode(bad, alloc=za, writer=w)[0] == 0 and len(w.sizes) == (2 if stop == b0 else 3), (what, stop)
        got, _ = _run(prod, [bad] * 3, [None, b0, b0 + 1], [len(data)] * 3)
        assert got[0][0] != 0, what                                                    # the plain call fails
        assert got[1][:2] == (0, data[:b0]) and got[2][:2] == (0, data[:b0 + 1]), what


# ---- 6. one batch of everything -------------------------------------------------------------------------------------------

def test_mixed_batch_answers_as_each_job_alone(prod):
    s, data, bounds = _case("mix")
    w, wdata, wb = _case("wrap")
    mid = (bounds[2] + bounds[3]) // 2
    illegal = bytes(4) + s[4:]                                                         # dict_size 0
    rows = [(s, mid, mid), (s, None, bounds[-1]), (s, 0, 16), (illegal, 100, 1000), (s, NO_STOP, bounds[1] + 1), (illegal, 0, 16),
            (s[:12], 0, 16), (w, wb[2] + 5, wb[2] + 5), (s, mid, mid - 1)]            # (stream, stop_at, dst_cap)
    alone = [_run(prod, [r[0]], [r[1]], [r[2]])[0][0] for r in rows]
    got, _ = _run(prod, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], offsets=[i % 3 for i in range(len(rows))])
    assert got == alone
    assert [g[0] for g in got] == [0, 0, 0, CSCMI_NO_DECODER, WRITE_ERROR, CSCMI_NO_DECODER, CSCMI_NO_DECODER, 0, WRITE_ERROR]
    assert got[0][1] == data[:mid] and got[1][1] == data and got[2][1] == b"" and got[4][1] == data[:bounds[1]]
    assert got[7][1] == wdata[:wb[2] + 5] and got[8][1] == data[:bounds[2]]
