"""GPU tier for byte ranges and strided slices of entries (include/csa_mi355x.h: CSAMI_DeviceReadSlices;
csc_amd.csa.DeviceArchive.extract_slices): what a slice delivers must be what `extract` delivers of the whole entry, sliced with
numpy on the host -- never the call under test -- and nothing else may be stored; what it costs under stop_early must be what the
host planner (CSAMI_PlanDeviceSlices) says over the archive's index.

Archive "fragmented" is written with task_bytes=20000, so the entries are cut across many tasks; archive "one_task" holds the
same entries in one task of several fragments."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import csa_cases
import csa_write_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

CSARC_REF = os.path.join(ROOT, "oracle", "_ref", "csarc_ref")
SIZES = [1, 17, 16385, 70001]
MATRIX, ROWS, ROW = "s/matrix.bin", 200, 1000
SLACK = 32
ALIGN = [0, 1, 15]                              # where a destination begins, in rotation
M64 = 1 << 64


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


def _upload(data):
    import torch
    t = torch.empty(max(len(data), 1), dtype=torch.uint8, device="cuda")[:len(data)]
    if len(data):
        t.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def _content():
    c = {f"s/f{n:05d}.bin": cases.build([["text", 70 + i, 0, n]]) for i, n in enumerate(SIZES)}
    c[MATRIX] = cases.build([["text", 81, 0, 50000], ["exe", 82, 0, 50000], ["delta", 83, 0, 50000], ["random", 84, 0, 50000]])
    c["s/empty.bin"] = b""
    assert len(c[MATRIX]) == ROWS * ROW
    return c


@pytest.fixture(scope="module")
def arcs(csa, tmp_path_factory):
    """name -> dict(a: the open handle, data: the archive's bytes, raw_index, truth: {name: numpy bytes of the whole entry, by
    extract() on the same handle}, listed: list_entries by name)"""
    content = _content()
    edate = int(csa.lib().CSA_DecimalTime(int(csa_cases.MTIME)))
    entries = [{"name": n, "tensor": _upload(d) if d else None, "edate": edate, "eattr": csa_write_cases.FILE_ATTR} for n, d in content.items()]
    entries.append({"name": "s/", "tensor": None, "edate": edate, "eattr": csa_write_cases.DIR_ATTR})
    out = {}
    d = tmp_path_factory.mktemp("slices")
    for name, extra in (("fragmented", dict(task_bytes=20000)), ("one_task", {})):
        rc, arc, st = csa.DeviceArchive.write_tensors(entries, level=1, dict_size=64 << 10, **extra)
        assert rc == 0
        data = arc.cpu().numpy().tobytes()
        path = d / f"{name}.csa"
        path.write_bytes(data)
        a = csa.DeviceArchive.open(arc)
        rc, views, st = a.extract()
        assert rc == 0 and st["verify_failures"] == 0
        truth = {n: v.cpu().numpy().copy() for n, v in views.items()}
        assert {n: t.tobytes() for n, t in truth.items() if not n.endswith("/")} == content
        out[name] = dict(a=a, data=data, raw_index=csa.read_index(str(path)), truth=truth,
                         listed={e["name"]: e for e in csa.list_entries(str(path))}, tasks=st["tasks"])
    assert out["fragmented"]["tasks"] >= 10 and out["one_task"]["tasks"] == 1
    assert max(len(e["frags"]) for e in out["one_task"]["listed"].values()) == 1
    yield out
    for p in out.values():
        p["a"].close()


def _norm(s):
    return (s[0], s[1], s[1], 1) if len(s) == 2 else tuple(s)


def _take(whole, s):
    """the slice of an entry's bytes by the definition, with numpy"""
    off, run, stride, count = _norm(s)
    idx = (off + stride * np.arange(count, dtype=np.int64))[:, None] + np.arange(run, dtype=np.int64)[None, :]
    return whole[idx.ravel()].tobytes()


class Guarded:
    """n bytes, `off` bytes behind a 16-byte line, between 32 bytes of 0xA5 on either side, in an allocation of their own"""

    def __init__(self, n, off=0):
        import torch
        self.buf = torch.full((SLACK + off + n + SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.n = SLACK + off, n
        self.view = self.buf[self.lo:self.lo + n]

    def bytes(self):
        return self.view.cpu().numpy().tobytes()

    def guards_intact(self):
        return bool((self.buf[:self.lo] == 0xA5).all()) and bool((self.buf[self.lo + self.n:] == 0xA5).all())

    def untouched(self):
        return bool((self.buf == 0xA5).all())


def _read(p, slices, k=0, **kw):
    """extract_slices into guarded destinations -> (rc, {name: Guarded}, stats); the destinations' alignments rotate from k"""
    dsts = {n: Guarded(_norm(s)[1] * _norm(s)[3], ALIGN[(k + i) % 3]) for i, (n, s) in enumerate(slices.items())}
    rc, got, st = p["a"].extract_slices(slices, {n: g.view for n, g in dsts.items()}, **kw)
    assert set(got) == {n for n, s in slices.items() if _norm(s)[3]}
    return rc, dsts, st


def _check(p, slices, k=0, **kw):
    rc, dsts, st = _read(p, slices, k, **kw)
    assert rc == 0 and st["verify_failures"] == 0 and st["launches"] == 3 * st["waves"], slices
    assert st["selected_bytes"] == sum(g.n for g in dsts.values())
    for n, g in dsts.items():
        assert g.bytes() == _take(p["truth"][n], slices[n]), (n, slices[n])
        assert g.guards_intact(), (n, slices[n])
    return st


BOTH = ["fragmented", "one_task"]


# ---- 1. ranges --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BOTH)
def test_ranges_of_every_entry(arcs, name):
    p = arcs[name]
    sizes = {n: len(t) for n, t in p["truth"].items() if len(t)}
    assert len(sizes) == 5
    for k, rng in enumerate([lambda z: (0, z), lambda z: (0, 1), lambda z: (z - 1, 1), lambda z: (19999, 2), lambda z: (20000, 1),
                             lambda z: (16383, 2)]):
        slices = {n: rng(z) for n, z in sizes.items() if sum(rng(z)) <= z}
        assert len(slices) >= 2
        for stop in (True, False):
            _check(p, slices, k, stop_early=stop)


@pytest.mark.parametrize("name", BOTH)
def test_the_whole_entry_as_a_slice_is_extract_into(arcs, name):
    p = arcs[name]
    a = p["a"]
    files = a.plan()[0]
    whole = {f["name"]: (0, f["size"]) for f in files if f["size"]}
    for stop in (False, True):
        into = {f["name"]: Guarded(f["size"], ALIGN[i % 3]) for i, f in enumerate(files)}
        rc0, st0 = a.extract_into({n: g.view for n, g in into.items()}, stop_early=stop)
        rc1, dsts, st1 = _read(p, whole, stop_early=stop)
        assert rc0 == rc1 == 0
        assert all(dsts[n].bytes() == into[n].bytes() and dsts[n].guards_intact() for n in whole)
        keys = ["tasks", "frags", "waves", "launches", "raw_bytes", "verify_failures", "readback_bytes"] + (["decoded_bytes", "scratch_bytes"] if stop else [])
        assert {k: st1[k] for k in keys} == {k: st0[k] for k in keys}
        assert [(f["name"], f["nfrags"], f["failed_frags"], f["size"]) for f in st1["files"]] == \
               [(f["name"], f["nfrags"], f["failed_frags"], f["size"]) for f in st0["files"]]
        assert st1["periodic_pieces"] == 0 and st1["touched_bytes"] == st1["raw_bytes"] == st1["selected_bytes"]


# ---- 2. strided slices on the matrix ------------------------------------------------------------------------------------------

def _raw_slices():
    out = []
    for run, stride in ((1, 2), (3, 5), (16, 17), (100, 16384), (100, 20000), (1, 40000)):
        for off in (0, 1, 15):
            out.append((off, run, stride, (ROWS * ROW - off - run) // stride + 1))
    return out


@pytest.mark.parametrize("name", BOTH)
def test_column_blocks_of_the_matrix(csa, arcs, name):
    p = arcs[name]
    k = 0
    for c0, c1 in ((0, 1), (999, 1000), (0, 500), (496, 512), (3, 20)):
        for r0, r1 in ((0, 200), (19, 21), (199, 200)):
            s = csa.rows_slice(ROW, r0, r1, c0, c1)
            want = np.ascontiguousarray(p["truth"][MATRIX].reshape(ROWS, ROW)[r0:r1, c0:c1]).tobytes()
            assert _take(p["truth"][MATRIX], s) == want, "rows_slice means what numpy means"
            _check(p, {MATRIX: s}, k)
            k += 1


@pytest.mark.parametrize("name", BOTH)
def test_raw_strided_slices_of_the_matrix(arcs, name):
    p = arcs[name]
    periodic = 0
    for k, s in enumerate(_raw_slices()):
        st = _check(p, {MATRIX: s}, k, stop_early=bool(k % 2))
        periodic += st["periodic_pieces"]
        if s[2] <= 17:
            assert st["periodic_pieces"] == -(-ROWS * ROW // 16384) if name == "one_task" else st["periodic_pieces"] >= 13
    assert periodic > 0


def test_slices_of_several_entries_at_once(csa, arcs):
    p = arcs["fragmented"]
    slices = {MATRIX: csa.rows_slice(ROW, 10, 190, 250, 375), "s/f70001.bin": (1, 7, 11, 6363), "s/f16385.bin": (16384, 1), "s/f00017.bin": (0, 0, 0, 0)}
    st = _check(p, slices)
    assert st["tasks"] < p["tasks"]


# ---- 3. cost ------------------------------------------------------------------------------------------------------------------

def test_cost_is_what_the_planner_says(csa, arcs):
    p = arcs["fragmented"]
    for k, slices in enumerate([{MATRIX: csa.rows_slice(ROW, 19, 21)}, {MATRIX: csa.rows_slice(ROW, 0, 200, 496, 512)}, {MATRIX: (15, 100, 20000, 10)},
                                {MATRIX: (1, 1, 40000, 5), "s/f70001.bin": (20000, 1)}, {"s/f16385.bin": (16383, 2), "s/f00001.bin": (0, 1)}]):
        rcp, plan, touched = csa.plan_device_slices(p["raw_index"], len(p["data"]), slices)
        assert rcp == 0 and plan
        st = _check(p, slices, k, stop_early=True)
        assert st["tasks"] == len(plan) and st["frags"] == touched
        assert st["decoded_bytes"] == sum(t["stop"] for t in plan)
        assert st["scratch_bytes"] == sum((t["stop"] + 255) // 256 * 256 for t in plan)
        assert st["task_raw_bytes"] == sum(t["raw"] for t in plan)
        st0 = _check(p, slices, k, stop_early=False)
        assert st0["tasks"] == len(plan) and "decoded_bytes" not in st0


def test_the_tail_of_an_entry_decodes_the_tasks_of_its_last_fragments(csa, arcs):
    p = arcs["fragmented"]
    name, size = "s/f70001.bin", 70001
    frags = p["listed"][name]["frags"]
    assert len(frags) >= 3
    bids = {f["bid"] for f in frags if f["size"] and f["posfile"] + f["size"] > size - 100}
    st = _check(p, {name: (size - 100, 100)})
    rcp, plan, touched = csa.plan_device_slices(p["raw_index"], len(p["data"]), {name: (size - 100, 100)})
    assert st["tasks"] == len(bids) < len({f["bid"] for f in frags}) and {t["bid"] for t in plan} == bids


def test_a_stride_that_steps_over_a_task_leaves_it_undecoded(arcs):
    p = arcs["fragmented"]
    s = (0, 100, 40000, 5)
    st = _check(p, {MATRIX: s})
    hull = _check(p, {MATRIX: (0, 4 * 40000 + 100)})
    assert st["tasks"] < hull["tasks"] and st["decoded_bytes"] < hull["decoded_bytes"] and st["touched_bytes"] < hull["touched_bytes"]


def test_three_launches_a_wave_in_several_waves(csa, arcs):
    p = arcs["fragmented"]
    s = {MATRIX: csa.rows_slice(ROW, 0, 200, 3, 20)}
    st = _check(p, s, device_streams=2)
    assert st["waves"] == (st["tasks"] + 1) // 2 > 1 and st["launches"] == 3 * st["waves"]
    ms = p["a"].kernel_ms()
    assert ms[1] > 0 and ms[2] > 0


# ---- 4. verify only -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BOTH)
def test_verify_only(csa, arcs, name):
    p = arcs[name]
    slices = {MATRIX: csa.rows_slice(ROW, 0, 200, 496, 512), "s/f70001.bin": (19999, 2)}
    st = _check(p, slices)
    rc, got, st0 = p["a"].extract_slices(slices, {n: None for n in slices})
    assert rc == 0 and got == {}
    for k in ("tasks", "frags", "verify_failures", "raw_bytes", "touched_bytes", "selected_bytes", "decoded_bytes", "launches"):
        assert st0[k] == st[k], k
    assert st0["periodic_pieces"] == 0 and st0["plain_pieces"] == st["plain_pieces"] + st["periodic_pieces"]
    # one given, one verified only: the given one is delivered, nothing else is written
    g = Guarded(2, 1)
    rc, got, st1 = p["a"].extract_slices(slices, {MATRIX: None, "s/f70001.bin": g.view})
    assert rc == 0 and list(got) == ["s/f70001.bin"] and g.bytes() == _take(p["truth"]["s/f70001.bin"], (19999, 2)) and g.guards_intact()


# ---- 5. damage --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dec(orc, zalloc):
    def d(stream):
        rc, raw = orc.decode(stream, alloc=zalloc)
        assert rc == 0
        return raw
    return d


def test_damage_in_a_touched_task_and_in_an_untouched_one(csa, arcs, dec):
    p = arcs["fragmented"]
    info = orc_csa.parse(p["data"], dec)
    frags = sorted(p["listed"][MATRIX]["frags"], key=lambda f: f["posfile"])
    mid = next(f for f in frags if f["posfile"] <= 100000 < f["posfile"] + f["size"])
    bid = mid["bid"]
    hit = [f for f in frags if f["bid"] == bid and f["size"]]
    lo, hi = min(f["posfile"] for f in hit), max(f["posfile"] + f["size"] for f in hit)
    assert hi - lo == sum(f["size"] for f in hit) and 0 < lo and hi < ROWS * ROW, "the task's fragments of the entry lie back to back"
    off, size = info["abindex"][bid][0]
    bad = bytearray(p["data"])
    bad[off + size // 2] ^= 0x40
    truth = p["truth"][MATRIX]
    with csa.DeviceArchive.open(_upload(bytes(bad))) as a:
        q = dict(p, a=a)
        rc_t, st_t = a.test([MATRIX])
        failed_t = [f["failed_frags"] for f in st_t["files"]]
        assert rc_t == -1 or failed_t[0] > 0
        # touched: every fragment of the damaged task, and one byte of either neighbour
        s = (lo - 1, hi - lo + 2)
        rc, dsts, st = _read(q, {MATRIX: s}, names=[MATRIX], stop_early=False)
        assert rc == rc_t and [f["failed_frags"] for f in st["files"]] == failed_t and st["verify_failures"] == st_t["verify_failures"]
        g = dsts[MATRIX]
        got = g.bytes()
        assert g.guards_intact()
        assert got[0] == truth[lo - 1] and got[-1] == truth[hi], "the neighbours' tasks are intact"
        if failed_t[0] == 0:                             # the stream failed before it delivered a byte of them: nothing of them is stored
            assert got[1:-1] == b"\xa5" * (hi - lo)
        # not touched: the bytes around the damaged task's, the task itself stepped over
        s = (lo - 100, 100, hi - lo + 100, 2)
        rc, dsts, st = _read(q, {MATRIX: s}, names=[MATRIX])
        assert rc == 0 and st["verify_failures"] == 0 and [f["failed_frags"] for f in st["files"]] == [0]
        assert dsts[MATRIX].bytes() == _take(truth, s) and dsts[MATRIX].guards_intact()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(csa, arcs):
    import torch
    p = arcs["one_task"]
    n_arc = len(p["data"])
    big = torch.full((n_arc + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    big[:n_arc].copy_(_upload(p["data"]))
    zero = ["launches", "decode_launches", "tasks", "frags", "waves", "readback_bytes", "selected_bytes", "touched_bytes", "periodic_pieces",
            "plain_pieces", "decoded_bytes", "scratch_bytes"]
    with csa.DeviceArchive.open(big[:n_arc]) as a:
        def refused(slices, dsts, want, guarded):
            rc, got, st = a.extract_slices(slices, dsts)
            assert rc == want, (slices, rc)
            assert [st[k] for k in zero] == [0] * len(zero), st
            assert all(g.untouched() for g in guarded)
        s = csa.rows_slice(ROW, 0, 200, 3, 20)
        nbytes = 17 * 200
        g = Guarded(nbytes - 1, 1)
        refused({MATRIX: s}, {MATRIX: g.view}, csa.WRITE_ERROR, [g])                 # a capacity one byte short
        g = Guarded(nbytes + 100, 15)
        refused({MATRIX: s, "s/f70001.bin": (5, 100)}, {MATRIX: g.view[:nbytes], "s/f70001.bin": g.view[nbytes - 1:]}, -1, [g])   # one byte of overlap
        rc, got, st = a.extract_slices({MATRIX: s, "s/f70001.bin": (5, 100)}, {MATRIX: g.view[:nbytes], "s/f70001.bin": g.view[nbytes:]})
        assert rc == 0 and g.guards_intact(), "touching is fine"
        refused({MATRIX: s}, {MATRIX: big[n_arc - 1:n_arc - 1 + nbytes]}, -1, [])     # a destination on the archive's last byte
        assert big[:n_arc].cpu().numpy().tobytes() == p["data"] and bool((big[n_arc:] == 0xA5).all())
        z = ROWS * ROW
        for bad in ((0, 0, 1, 1), (0, 4, 3, 2), (M64 - 1, 2, 2, 1), (0, 1, 1 << 62, 5), (0, 2, M64 - 1, 2), (M64 - 8, 1, 8, 2),
                    (z - 1, 2), (z, 1), (1, 1000, 1000, 200)):
            g = Guarded(4096)
            refused({MATRIX: bad}, {MATRIX: g.view}, -1, [g])
        # n off by one, and no slices at all
        files = a.plan()[0]
        ptrs, caps, sl = (C.c_void_p * 8)(), (C.c_uint64 * 8)(), (csa.CSADevSlice * 8)()
        st, ss, ls = csa.CSADevReadStats(), csa.CSADevStopStats(), csa.CSADevSliceStats()
        L = csa.lib()
        for n, table, want in ((len(files) - 1, sl, -1), (len(files) + 1, sl, -1), (len(files), None, -1), (len(files), sl, 0)):
            assert L.CSAMI_DeviceReadSlices(a._h, None, 0, table, ptrs, caps, n, 1, None, None, C.byref(st), C.byref(ss), C.byref(ls)) == want
            assert st.launches == 0 and st.decode_launches == 0 and st.tasks == 0, "and count == 0 everywhere reads nothing"
        g = Guarded(16)
        with pytest.raises(KeyError):
            a.extract_slices({"s/nothing.bin": (0, 1)})
        with pytest.raises(KeyError):
            a.extract_slices({MATRIX: (0, 1)}, {"s/f00001.bin": g.view}, names=[MATRIX])
        assert g.untouched()


# ---- 7. an archive the reference wrote ----------------------------------------------------------------------------------------------

def test_slices_of_an_archive_the_reference_wrote(csa, arcs, tmp_path):
    if not os.path.exists(CSARC_REF):
        pytest.skip("oracle/_ref/csarc_ref not in this snapshot")
    truth = arcs["one_task"]["truth"][MATRIX]
    (tmp_path / "m").mkdir()
    (tmp_path / "m" / "matrix.bin").write_bytes(truth.tobytes())
    subprocess.run([CSARC_REF, "a", "-m1", "-d64k", "-p4", "-f", "ref.csa", "m/matrix.bin"], cwd=tmp_path, check=True, capture_output=True)
    with csa.DeviceArchive.open(_upload((tmp_path / "ref.csa").read_bytes())) as a:
        rc, views, st = a.extract()
        (stored, view), = [(n, v) for n, v in views.items() if v.numel()]
        assert rc == 0 and view.cpu().numpy().tobytes() == truth.tobytes()
        p = dict(a=a, truth={stored: truth})
        _check(p, {stored: csa.rows_slice(ROW, 19, 21, 496, 512)})
        _check(p, {stored: (15, 16, 17, 11763)}, 1)
