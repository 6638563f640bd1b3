"""GPU tier (-m gpu): every entry-point kernel form of the encoder against the checker (the reference build oracle/_ref when it
is there, the oracle otherwise).  The form a stream runs in depends on its props (the parser bits of CSCEnc_Create) and, in a
batch call, on how many streams of that flavour the call carries (thresholds kBtMultiMax, kD4MultiMax, kHpMultiMax).  FORMS
is the dispatch table of the launchers (csc_kernels_blocks.inc); tests/test_product_host.py fails when a launcher names a
kernel FORMS lacks or a threshold moves.  Every stream is decoded again on the device -- CSCDec_Decode for single streams,
CSCMI_DecodeBatch for batches -- and (rc, bytes) must equal the checker's decoder (not the input: the reference has a known
round-trip hazard, tests/golden/ref_roundtrip_hazard.json)."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import soak_gen

pytestmark = pytest.mark.gpu

THRESHOLDS = {"kBtMultiMax": 256, "kD4MultiMax": 768, "kHpMultiMax": 768}

# row -> the kernel of a single stream, of a batch flavour at or below the row's threshold, and above it; the threshold; the
# props variants (level, overrides) the row's tests use (variant 0 for the single stream; every variant selects the row)
FORMS = {
    "level3": dict(single="k_encode_runs_dp4", multi="k_encode_runs_multi_dp4", over="k_encode_runs_multi_one",
                   threshold="kD4MultiMax", variants=[(3, {}), (3, {"hash_width": 1, "hash_bits": 16, "good_len": 8})]),
    "level4": dict(single="k_encode_runs<3,true>", multi="k_encode_runs_multi_one", over="k_encode_runs_multi_one",
                   threshold="kD4MultiMax", variants=[(4, {}), (3, {"good_len": 65}), (3, {"hash_width": 9, "hash_bits": 15})]),
    "level5": dict(single="k_encode_runs_bt", multi="k_encode_runs_multi_bt", over="k_encode_runs_multi<3,false>",
                   threshold="kBtMultiMax", variants=[(5, {}), (5, {"bt_cyc": 16, "bt_size": 100000, "good_len": 200})]),
    "level12": dict(single="k_encode_runs_hp", multi="k_encode_runs_multi_hp", over="k_encode_runs_multi<2,true>",
                    threshold="kHpMultiMax", variants=[(2, {}), (1, {}), (2, {"lz_mode": 1, "hash_width": 4})]),
    "lazy_w9": dict(single="k_encode_runs<2,true>", multi="k_encode_runs_multi<2,true>", over="k_encode_runs_multi<2,true>",
                    threshold=None, variants=[(1, {"hash_width": 9, "lz_mode": 1}), (2, {"hash_width": 9}),
                                              (2, {"hash_width": 9, "lz_mode": 1, "good_len": 200})]),
    "adv_generic": dict(single="k_encode_runs<3,false>", multi="k_encode_runs_multi<3,false>", over="k_encode_runs_multi<3,false>",
                        threshold=None, variants=[(5, {"hash_width": 4, "hash_bits": 16}), (5, {"bt_cyc": 48}),
                                                  (3, {"hash_width": 12, "hash_bits": 16})]),
    "lazy_generic": dict(single="k_encode_runs<2,false>", multi="k_encode_runs_multi<2,false>", over="k_encode_runs_multi<2,false>",
                         threshold=None, variants=[(5, {"lz_mode": 2}), (2, {"hash_width": 16, "lz_mode": 1}),
                                                   (5, {"lz_mode": 1, "hash_width": 4, "hash_bits": 16})]),
}


def _spec(row, k, dict_size, parts):
    level, over = FORMS[row]["variants"][k % len(FORMS[row]["variants"])]
    return {"parts": parts, "level": level, "dict": dict_size, "props": dict(over), "row": row}


def _kind(i):
    return ("text", "exe", "delta", "entropy8", "random", "silesia")[i % 6]


@pytest.fixture(scope="module")
def chk():
    return soak_gen.checker()[:2]


def _check_many(chk, specs, datas):
    lib, za = chk
    first = soak_gen.check_one(lib, za, specs[0], datas[0])      # (alone: whatever the checker sets up on first use, one thread sets up)
    with ThreadPoolExecutor(8) as ex:
        return [first] + list(ex.map(lambda i: soak_gen.check_one(lib, za, specs[i], datas[i]), range(1, len(specs))))


def _run_batch(prod, chk, specs, stats=None):
    datas = [soak_gen.build_input(s) for s in specs]
    got, rounds = soak_gen.encode_batch(prod, [soak_gen.props_of(prod, s) for s in specs], datas, stats=stats)
    want = _check_many(chk, specs, datas)
    bad = [i for i in range(len(specs)) if want[i][0] != 0 or got[i] != want[i][1]]
    assert not bad, f"{len(bad)} of {len(specs)} streams differ from the checker's; first: stream {bad[0]} {soak_gen.describe(None, bad[0], specs[bad[0]])}"
    dec = soak_gen.decode_batch(prod, got)
    bad = [i for i in range(len(specs)) if dec[i] != (want[i][2], want[i][3])]
    assert not bad, f"{len(bad)} batch decodes differ from the checker's decoder; first: stream {bad[0]} rc {dec[bad[0]][0]} vs {want[bad[0]][2]} " \
                    f"{soak_gen.describe(None, bad[0], specs[bad[0]])}"
    return rounds


def _ids(kind):
    return [f"{row}-{f[kind]}" for row, f in FORMS.items()]


# an input of a little over one 2 MiB chunk that mixes text, exe, delta, random and zeros
SINGLE_PARTS = [["text", 501, 0, 700000], ["exe", 502, 0, 400000], ["delta", 503, 0, 300000], ["random", 504, 0, 60000],
                ["zeros", 200000], ["text", 501, 100000, 250000], ["entropy8", 505, 0, 200000]]


@pytest.mark.parametrize("row", list(FORMS), ids=_ids("single"))
def test_single(prod, chk, row):
    spec = _spec(row, 0, 1 << 20, SINGLE_PARTS)
    data = soak_gen.build_input(spec)
    assert len(data) > soak_gen.CHUNK
    rc, s = prod.encode(data, props=soak_gen.props_of(prod, spec))
    rc2, want, rcd2, back2 = soak_gen.check_one(*chk, spec, data)
    assert rc == 0 and rc2 == 0
    assert s == want, f"{row}: HIP stream differs from the checker's ({len(s)} vs {len(want)} bytes)"
    assert prod.decode(s) == (rcd2, back2), f"{row}: device decoder differs from the checker's decoder"


# 1 byte .. 24 KiB (power-of-two edges) and two streams that cross a chunk
BATCH_SIZES = [1, 2, 3, 7, 64, 255, 256, 257, 511, 1000, 4095, 4096, 4097, 8191, 8192, 8193, 12000, 16383, 16384, 16385, 20000, 24576,
               soak_gen.CHUNK + 1, soak_gen.CHUNK + 300000]


@pytest.mark.parametrize("row", list(FORMS), ids=_ids("multi"))
def test_batch(prod, chk, row):
    specs = []
    for i, n in enumerate(BATCH_SIZES):
        parts = [[_kind(i), 600 + i, i * 7919, n]]
        specs.append(_spec(row, i, 1 << 20 if n > soak_gen.CHUNK else max(n, 1), parts))
    assert _run_batch(prod, chk, specs) == 2


def _small_streams(row, count, salt):
    specs = []
    for i in range(count):
        n = 1 + (i * 2654435761 + salt) % 3000
        specs.append(_spec(row, i, n, [[_kind(i + salt), 700 + i % 17, (i * 104729) % 5000000, n]]))
    return specs


THRESHOLD_CASES = [("level5", 256), ("level5", 257), ("level3", 768), ("level3", 769), ("level12", 768), ("level12", 769), ("level4", 769)]


def _threshold_id(case):
    row, count = case
    f = FORMS[row]
    kernel = f["over"] if f["threshold"] and count > THRESHOLDS[f["threshold"]] else f["multi"]
    return f"{row}-{count}-{kernel}"


@pytest.mark.parametrize("case", THRESHOLD_CASES, ids=[_threshold_id(c) for c in THRESHOLD_CASES])
def test_batch_threshold(prod, chk, case):
    row, count = case
    assert _run_batch(prod, chk, _small_streams(row, count, count)) == 1


def test_batch_mixed_flavours_one_launch_each(prod, chk):
    """800 streams in one call -- above every threshold in total -- but 200 of each of four flavours: each flavour stays in
    its at-or-below-threshold form, one launch per flavour per chunk round, counted on the lead handle"""
    rows = ["level3", "level12", "level5", "level4"]
    per = {r: _small_streams(r, 200, 11 + k) for k, r in enumerate(rows)}
    specs = [per[rows[i % 4]][i // 4] for i in range(800)]
    stats = []
    assert _run_batch(prod, chk, specs, stats=stats) == 1
    assert stats[0].encode_launches == len(rows), stats[0].encode_launches

