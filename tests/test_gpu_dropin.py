"""GPU tier of the drop-in rows: the reference's own archiver and command-line tool, compiled from their sources and linked against
libcsc_mi355x.so (oracle/_ref/csarc_on_product, csc_on_product: oracle/Makefile), run as a user would run them.  What only these two
callers exercise is held here: the ICompressProgress values and the memory estimate the tool prints, the Write sequence as the
archiver's coalescing writer turns it into the archive's block table, the index packed through CSCEnc_* with a NULL ISzAlloc and read
back through CSCDec_*, eight worker threads with handles alive at once, and the decoder fed by the archiver's reader thread.

The checkers: what the tool prints and writes on the REFERENCE's libcsc (tests/golden/dropin_cli.json, held against both checkers by
tests/test_dropin_host.py), the archives the reference archiver writes (tests/golden/csa.json), and both reference binaries run live
when oracle/_ref holds them.  Every child is one fresh process at a time; after one that hung or died nothing more is started."""
import json
import os
import stat
import subprocess
import sys

import pytest

import cases
import csa_cases
import dropin_cases as dc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

REFDIR = os.path.join(ROOT, "oracle", "_ref")
CSARC, CSC = os.path.join(REFDIR, "csarc_on_product"), os.path.join(REFDIR, "csc_on_product")
CSARC_REF, CSC_REF = os.path.join(REFDIR, "csarc_ref"), os.path.join(REFDIR, "csc_ref")
HAVE_CSARC_REF, HAVE_CSC_REF = os.path.exists(CSARC_REF), os.path.exists(CSC_REF)
if not os.path.exists(CSARC):
    pytest.skip("oracle/_ref/csarc_on_product not built (the recipe needs the reference tree)", allow_module_level=True)

GOLD_CLI = json.load(open(os.path.join(ROOT, "tests", "golden", "dropin_cli.json")))
GOLD_CSA = json.load(open(os.path.join(ROOT, "tests", "golden", "csa.json")))

_stop = {"why": None}          # set by the first child that hung or died: every later test of the file skips


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _stop["why"]:
        pytest.skip("not started: " + _stop["why"])


def child(argv, cwd):
    """one fresh process, run to its end before anything else starts; the environment as inherited plus TZ=UTC (`l` prints dates)"""
    assert not _stop["why"]
    what = " ".join([os.path.basename(argv[0])] + list(argv[1:]))
    try:
        p = subprocess.run(argv, cwd=cwd, env=dict(os.environ, TZ="UTC"), capture_output=True, timeout=120)
    except subprocess.TimeoutExpired:
        _stop["why"] = f"`{what}` did not end within 120 s"
        pytest.fail(_stop["why"])
    if p.returncode < 0 or p.returncode in (134, 137, 139):
        _stop["why"] = f"`{what}` died with status {p.returncode}"
        pytest.fail(_stop["why"] + ": " + p.stderr[-1500:].decode("latin-1"))
    return p


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def orc_dec(orc, zalloc):
    def dec(stream):
        rc, raw = orc.decode(stream, alloc=zalloc)
        assert rc == 0
        return raw
    return dec


# ---------------------------------------------------------------------------------------------
# the command-line tool
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(dc.CLI_CASES))
def test_cli_encode_writes_and_prints_what_the_reference_does(case, tmp_path):
    g = GOLD_CLI[case]
    (tmp_path / dc.IN_NAME).write_bytes(cases.build(g["spec"]))
    p = child([CSC] + dc.encode_argv(case), tmp_path)
    assert p.returncode == 0 and p.stdout == b"\n"
    stream = (tmp_path / dc.OUT_NAME).read_bytes()
    print(case, "stderr:", repr(p.stderr.decode("latin-1")))
    assert (len(stream), cases.digest(stream)) == (g["stream_size"], g["stream_sha256"])
    assert p.stderr.decode("latin-1") == g["encode_stderr"]        # the memory estimate and every Progress record, byte for byte
    if HAVE_CSC_REF:
        os.rename(tmp_path / dc.OUT_NAME, tmp_path / "mine.csc")
        r = child([CSC_REF] + dc.encode_argv(case), tmp_path)
        assert r.returncode == 0 and (tmp_path / dc.OUT_NAME).read_bytes() == stream and r.stderr == p.stderr


@pytest.mark.parametrize("case", list(dc.CLI_CASES))
def test_cli_decode_writes_and_prints_what_the_reference_does(case, tmp_path, orc, zalloc):
    g = GOLD_CLI[case]
    data = cases.build(g["spec"])
    rc, stream = orc.encode(data, props=dc.props_of(orc, case, len(data)), alloc=zalloc)       # the recorded stream, re-made by the checker
    assert rc == 0 and (len(stream), cases.digest(stream)) == (g["stream_size"], g["stream_sha256"])
    (tmp_path / dc.OUT_NAME).write_bytes(stream)
    p = child([CSC] + dc.decode_argv(), tmp_path)
    assert p.returncode == 0 and p.stdout == b"\n"
    back = (tmp_path / dc.BACK_NAME).read_bytes()
    print(case, "stderr:", repr(p.stderr.decode("latin-1")))
    assert (len(back), cases.digest(back)) == (g["decoded_size"], g["decoded_sha256"]) and back == data
    assert p.stderr.decode("latin-1") == g["decode_stderr"]


# ---------------------------------------------------------------------------------------------
# the archiver: a
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", csa_cases.CPU_CASES)
def test_archiver_add_writes_the_reference_archive(case, tmp_path):
    """`a` with one worker: the archive is a function of the sizes and the order of the library's Write calls (the writer coalesces them
    into blocks of at most 1 MiB, csa_io.h:174-200) and of the index packed through CSCEnc_* with a NULL ISzAlloc (csarc.cpp:252-262)"""
    csa_cases.make_tree(str(tmp_path), case)
    p = child([CSARC] + csa_cases.csarc_argv(case), tmp_path)
    assert p.returncode == 0, p.stderr[-1500:]
    arc = (tmp_path / csa_cases.ARCNAME).read_bytes()
    g = GOLD_CSA[case]
    assert (len(arc), cases.digest(arc)) == (g["archive_size"], g["archive_sha256"])
    if HAVE_CSARC_REF:
        os.rename(tmp_path / csa_cases.ARCNAME, tmp_path / "mine.csa")
        r = child([CSARC_REF] + csa_cases.csarc_argv(case), tmp_path)
        assert r.returncode == 0 and (tmp_path / csa_cases.ARCNAME).read_bytes() == arc


def same_but_for_block_offsets(a, b):
    """two parsed archives (orc_csa.parse) of one tree and one option set, written by different numbers of workers: the same files,
    fragments and tasks, every task's blocks of the same sizes in the same order.  Where the blocks lie may differ, and so may the
    order of one file's fragments in its entry: workers append them as they finish (the reference's own `-t8` archive of
    single_split_many lists them in another order than its `-t1` archive does)"""
    def entries(info):
        return {n: dict(e, frags=sorted(e["frags"], key=lambda f: f["posfile"])) for n, e in info["index"].items()}
    assert list(a["index"]) == list(b["index"]) and entries(a) == entries(b)
    assert sorted(a["abindex"]) == sorted(b["abindex"])
    for tid in a["abindex"]:
        assert [s for _, s in a["abindex"][tid]] == [s for _, s in b["abindex"][tid]], tid
    assert (a["index_rsize"], a["index_used"], a["index_pos"]) == (b["index_rsize"], b["index_used"], b["index_pos"])
    assert a["index_raw"][a["index_used"]:] == b["index_raw"][b["index_used"]:]


def blocks_tile_the_body(info):
    """the blocks of all tasks lie back to back between the header and the index: none lost, none overlapping"""
    pos = 24
    for off, size in sorted(b for blocks in info["abindex"].values() for b in blocks):
        assert off == pos
        pos += size
    assert pos == info["index_pos"]


def task_stream(arc, info, tid):
    return b"".join(arc[o:o + s] for o, s in info["abindex"][tid])


@pytest.mark.parametrize("case", ["many_files", "single_split_many"])
def test_archiver_add_with_eight_workers(case, tmp_path, csa, orc_dec, monkeypatch):
    """`a -t8`: eight worker threads create, drive and destroy handles at once while their I/O threads block in semaphores.  Where a
    task's blocks land depends on timing (in the reference too); everything else must be the one-worker archive's"""
    content = csa_cases.make_tree(str(tmp_path), case)
    argv = csa_cases.csarc_argv(case)
    p = child([CSARC, argv[0], "-t8"] + argv[1:], tmp_path)
    assert p.returncode == 0, p.stderr[-1500:]
    arc8 = (tmp_path / csa_cases.ARCNAME).read_bytes()
    os.rename(tmp_path / csa_cases.ARCNAME, tmp_path / "t8.csa")
    if HAVE_CSARC_REF:
        assert child([CSARC_REF] + argv, tmp_path).returncode == 0
    else:
        monkeypatch.chdir(tmp_path)
        spec = csa_cases.CSA_CASES[case]
        assert csa.add(csa_cases.ARCNAME, spec["args"], overwrite=True, **spec["opts"])[0] == 0
    arc1 = (tmp_path / csa_cases.ARCNAME).read_bytes()
    assert cases.digest(arc1) == GOLD_CSA[case]["archive_sha256"]
    i8, i1 = orc_csa.parse(arc8, orc_dec), orc_csa.parse(arc1, orc_dec)
    assert len(i1["abindex"]) > 8          # (the archives' lengths may differ: the block offsets are compressed into the index)
    same_but_for_block_offsets(i8, i1)
    blocks_tile_the_body(i8)
    for tid in i1["abindex"]:
        assert task_stream(arc8, i8, tid) == task_stream(arc1, i1, tid), tid
    if HAVE_CSARC_REF:
        t = child([CSARC_REF, "t", "t8.csa"], tmp_path)
        assert t.returncode == 0 and b"failed" not in t.stderr
    monkeypatch.chdir(tmp_path)
    rc, st = csa.extract("t8.csa", to_dir=str(tmp_path / "out"), mt_count=8)
    assert rc == 0 and st["verify_failures"] == 0
    for rel, data in content.items():
        assert (tmp_path / "out" / rel).read_bytes() == data, rel


# ---------------------------------------------------------------------------------------------
# the archiver: t, x, l
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def archives(csa, tmp_path_factory):
    """name -> (directory holding the tree and the archive `in.csa`, the tree's content); made once, read by every test below"""
    made = {}

    def get(name):
        if name in made:
            return made[name]
        if name == "ref_t4_many_files" and not HAVE_CSARC_REF:
            pytest.skip("oracle/_ref/csarc_ref not in this snapshot")
        root = tmp_path_factory.mktemp(name)
        if name == "product_mixed_tree":
            content = csa_cases.make_tree(str(root), "mixed_tree")
            spec = csa_cases.CSA_CASES["mixed_tree"]
            cwd = os.getcwd()
            os.chdir(root)
            try:
                assert csa.add("in.csa", spec["args"], overwrite=True, **spec["opts"])[0] == 0
            finally:
                os.chdir(cwd)
        else:
            content = csa_cases.make_tree(str(root), "many_files")
            argv = ["in.csa" if a == csa_cases.ARCNAME else a for a in csa_cases.csarc_argv("many_files")]
            assert child([CSARC_REF, argv[0], "-t4"] + argv[1:], root).returncode == 0       # four workers: blocks of different tasks interleave
        made[name] = (root, content)
        return made[name]
    return get


@pytest.mark.parametrize("threads", [1, 8])
@pytest.mark.parametrize("name", ["product_mixed_tree", "ref_t4_many_files"])
def test_archiver_test_extract_list(name, threads, archives):
    """`t`, `x` and `l` over an archive the product's container wrote and one the reference archiver wrote with four workers: the
    index through CSCDec_* with a NULL ISzAlloc and a memory reader (csarc.cpp:322-325), the task streams through decoders fed by
    the archiver's reader thread, `threads` of them at once"""
    root, content = archives(name)
    t = child([CSARC, "t", f"-t{threads}", "in.csa"], root)
    assert t.returncode == 0 and b"failed" not in t.stderr, t.stderr[-1500:]
    out = f"x{threads}"
    x = child([CSARC, "x", f"-t{threads}", "-o", out, "in.csa"], root)
    assert x.returncode == 0 and b"failed" not in x.stderr, x.stderr[-1500:]
    for rel, data in content.items():
        p = root / out / rel
        assert p.read_bytes() == data, rel
        s = p.stat()
        assert int(s.st_mtime) == csa_cases.MTIME and stat.S_IMODE(s.st_mode) == 0o644, rel
    for d in {os.path.dirname(rel) for rel in content}:
        while d:
            assert stat.S_IMODE((root / out / d).stat().st_mode) == 0o755, d
            d = os.path.dirname(d)
    ls = child([CSARC, "l", f"-t{threads}", "in.csa"], root)
    assert ls.returncode == 0 and all(os.path.basename(rel).encode() in ls.stdout for rel in content)
    if HAVE_CSARC_REF:
        want = child([CSARC_REF, "l", f"-t{threads}", "in.csa"], root)
        assert want.returncode == 0 and ls.stdout == want.stdout
