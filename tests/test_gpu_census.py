"""GPU tier (-m gpu): the census cases (tests/census_cases.py, tests/golden/census_cases.json) -- small inputs that provably reach
each named rare branch of the reference's coder, model, match finder and parsers (tests/test_census_host.py holds that claim on
the CPU) -- through every kernel form of their dispatch row: alone (the row's single-stream kernel), all of a row's cases in one
batch call (its batch kernel) and, for rows with a threshold, together with tiny fillers one stream above it (its over-threshold
kernel).  The block-size family (csc_blocksize 16 / 17 / 255 / 4096, twelve chunks a stream, and 1 / 3 below the decoder's floor)
runs alone and batched in every row, one member through CSCMI_EncodeDeviceBatch as well.

Every stream must equal the checker's byte for byte.  Where the checker's decoder reads the checker's stream, the device decodes
it too and (rc, bytes) must be the checker's; where it does not -- csc_blocksize below the floor, a Flush that left an empty BC
block -- only the encode is compared, and the test id says encode-only."""
import pytest

import census_cases as cc
import soak_gen
import test_gpu_forms as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chk():
    return soak_gen.checker()[:2]


_memo = {}


def _want(chk, name, spec):
    """(data, (rc, stream, decoder rc, decoded)) of the checker, once per case"""
    if name not in _memo:
        data = soak_gen.build_input(spec)
        _memo[name] = (data, soak_gen.check_one(*chk, spec, data))
    return _memo[name]


def _single(prod, chk, name, spec, decodes):
    data, (rc2, want, rcd2, back2) = _want(chk, name, spec)
    rc, s = prod.encode(data, props=soak_gen.props_of(prod, spec), max_read=spec.get("max_read"))
    assert rc == 0 and rc2 == 0
    assert s == want, f"{name}: HIP stream differs from the checker's ({len(s)} vs {len(want)} bytes) {soak_gen.describe(None, 0, spec)}"
    assert (rcd2 == 0 and back2 == data) == decodes, f"{name}: the checker's decoder answers {rcd2}"
    if rcd2 == 0:
        assert prod.decode(s) == (rcd2, back2), f"{name}: device decoder differs from the checker's decoder"


def _batch(prod, chk, named, rounds, fillers=()):
    """`named` [(name, spec)] and `fillers` [spec] in one batch call, the streams with a Read size of their own in chunks of that
    size; one launch a chunk round on the lead handle, as tests/test_gpu_forms.py counts them"""
    specs = [s for _, s in named] + list(fillers)
    wants = [_want(chk, n, s) for n, s in named]
    datas = [w[0] for w in wants] + [soak_gen.build_input(s) for s in fillers]
    checked = [w[1] for w in wants] + (F._check_many(chk, list(fillers), datas[len(named):]) if fillers else [])
    stats = []
    got, k = soak_gen.encode_batch(prod, [soak_gen.props_of(prod, s) for s in specs], datas,
                                   chunk=[s.get("max_read") or soak_gen.CHUNK for s in specs], stats=stats)
    bad = [i for i in range(len(specs)) if checked[i][0] != 0 or got[i] != checked[i][1]]
    assert not bad, f"{len(bad)} of {len(specs)} streams differ from the checker's; first: stream {bad[0]} {soak_gen.describe(None, bad[0], specs[bad[0]])}"
    assert k == rounds and stats[0].encode_launches == rounds, (k, stats[0].encode_launches)
    readable = [i for i in range(len(specs)) if checked[i][2] == 0]
    dec = soak_gen.decode_batch(prod, [got[i] for i in readable])
    bad = [i for j, i in enumerate(readable) if dec[j] != (checked[i][2], checked[i][3])]
    assert not bad, f"{len(bad)} batch decodes differ from the checker's decoder; first: stream {bad[0]} {soak_gen.describe(None, bad[0], specs[bad[0]])}"


CASES = cc.load()["cases"]


@pytest.mark.parametrize("case", CASES, ids=[f"{c['name']}-{F.FORMS[c['row']]['single']}" + ("" if c["decodes"] else "-encode-only") for c in CASES])
def test_single(prod, chk, case):
    _single(prod, chk, case["name"], case["spec"], case["decodes"])


@pytest.mark.parametrize("row", list(F.FORMS), ids=F._ids("multi"))
def test_multi(prod, chk, row):
    named = sorted(((c["name"], c["spec"]) for c in cc.cases_of(row)), key=lambda ns: -len(soak_gen.build_input(ns[1])))
    _batch(prod, chk, named, 1)


def _fillers(row, count):
    """1 .. 300 bytes each, the row's props variants in turn"""
    out = []
    for i in range(count):
        n = 1 + (i * 2654435761 + 17) % 300
        out.append(F._spec(row, i, n, [[F._kind(i), 720 + i % 13, (i * 104729) % 5000000, n]]))
    return out


OVER_ROWS = [row for row, f in F.FORMS.items() if f["threshold"]]


@pytest.mark.parametrize("row", OVER_ROWS, ids=[f"{row}-{F.FORMS[row]['over']}" for row in OVER_ROWS])
def test_over(prod, chk, row):
    named = sorted(((c["name"], c["spec"]) for c in cc.cases_of(row)), key=lambda ns: -len(soak_gen.build_input(ns[1])))
    count = F.THRESHOLDS[F.FORMS[row]["threshold"]] + 1
    _batch(prod, chk, named, 1, _fillers(row, count - len(named)))


FAMILY = [(row, member, spec, decodes) for row in F.FORMS for member, spec, decodes in cc.family_specs(row)]


@pytest.mark.parametrize("row,member,spec,decodes", FAMILY, ids=[f"{row}-{F.FORMS[row]['single']}-{member}" for row, member, _, _ in FAMILY])
def test_family_single(prod, chk, row, member, spec, decodes):
    _single(prod, chk, f"family-{row}-{member}", spec, decodes)


@pytest.mark.parametrize("row", list(F.FORMS), ids=F._ids("multi"))
def test_family_multi(prod, chk, row):
    named = [(f"family-{row}-{member}", spec) for member, spec, _ in cc.family_specs(row)]
    assert named[0][1].get("max_read") == cc.FAMILY_READ          # the lead stream is live in every round
    _batch(prod, chk, named, -(-len(soak_gen.build_input(named[0][1])) // cc.FAMILY_READ))


@pytest.mark.parametrize("row", list(F.FORMS))
def test_family_device_batch(prod, chk, row):
    """csc_blocksize 17 through CSCMI_EncodeDeviceBatch: the same twelve chunks, cut by raw_blocksize (the device-resident encode
    has no Read); the blocks framed on the device"""
    from csc_amd.device import encode_device
    level, over = cc.row_variant(row)
    spec = {"parts": cc.FAMILY_PARTS, "level": level, "dict": 32768, "row": row,
            "props": dict(over, csc_blocksize=cc.FAMILY_DEVICE_BATCH_BSIZE, raw_blocksize=cc.FAMILY_READ)}
    data, (rc2, want, _, _) = _want(chk, f"family-device-{row}", spec)
    p = soak_gen.props_of(prod, spec)
    res, stats = encode_device(prod, [data], props=p, caps=len(want))
    (rc, t), = res
    got = bytes(t.cpu().numpy().tobytes())
    assert rc == 0 and rc2 == 0 and got == want, f"{row}: rc {rc}, {len(got)} vs {len(want)} bytes"
    assert stats.rounds == -(-len(data) // cc.FAMILY_READ) + 1


def test_arena_holds_one_byte_blocks(prod, chk):
    """256 KiB of random at level 2 with csc_blocksize 1: 262 208 coder blocks of 32 arena bytes each, more than an arena sized from
    raw_blocksize alone held (3 x 2 MiB + 1 MiB).  CSCEnc_Create accepts the props and the reference writes the stream, so the
    product must.  (Encode only: below the floor.  Three Write calls a block on both sides: collected in C, census_cases.CSink.)"""
    spec = {"parts": [["random", 31, 0, 256 << 10]], "level": 2, "dict": 256 << 10, "props": {"csc_blocksize": 1}}
    data = soak_gen.build_input(spec)
    lib, za = chk
    sink = cc.CSink()
    rc2, _ = lib.encode(data, props=soak_gen.props_of(lib, spec), alloc=za, writer=sink)
    want = sink.take()
    assert rc2 == 0
    blocks = (len(want) - 10) // 2                  # a full one-byte block is its flag byte and its byte
    assert 32 * blocks > 3 * soak_gen.RAW_BLOCKSIZE + (1 << 20)
    sink = cc.CSink()
    rc, _ = prod.encode(data, props=soak_gen.props_of(prod, spec), writer=sink)
    s = sink.take()
    assert rc == 0, rc
    assert s == want, f"HIP stream differs from the checker's ({len(s)} vs {len(want)} bytes)"
