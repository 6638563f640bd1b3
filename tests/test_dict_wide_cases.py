"""CPU tier: the cases of tests/dict_wide_cases.py against what the REFERENCE recorded for them (tests/golden/dict_wide.json,
tools/make_golden_dict_wide.py), through the oracle's restatement of Foward_Dict -- and the cases shown sensitive to what they
are there for: a filter that forgets the token chain where two steps of 64 positions meet, or where two passes meet (of 128
positions, the kernel's two steps a pass, and of 256, four steps a pass), and one that counts an escaped byte as one output byte."""
import json
import os

import pytest

import dict_wide_cases as W
import filter_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the generator makes: 9 seams x 3 word lengths x 5 starts x 4 arrivals; 5 seams x 5 run lengths; 27 sizes x 3 word lengths
# x 5 starts; one pair at the 82 % boundary; two stretches of text
N_SEAM, N_ESC, N_END, N_REJECT, N_TEXT = 540, 25, 405, 2, 2
# seam cases whose word has letters on both sides of its seam (start 1 .. len - 1 bytes below it): 9 seams x (1 + 2 + 3) starts x 4
# arrivals; of them at the multiples of 128 (128, 256, 384, 512: the kernel's pass seams): 4 x 6 x 4; at 256 and 512: 2 x 6 x 4
N_STRADDLE_64, N_STRADDLE_128, N_STRADDLE_256 = 216, 96, 48


@pytest.fixture(scope="module")
def words(orc):
    return F.words(orc.lib)


@pytest.fixture(scope="module")
def wide(words):
    return W.cases(words)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "dict_wide.json")) as f:
        return json.load(f)


def _group(cases, prefix):
    return {n: d for n, d in cases.items() if n.startswith(prefix + "/")}


def test_the_generator_makes_the_cases_the_golden_file_has(wide, golden):
    assert sorted(wide) == sorted(golden)
    assert [len(_group(wide, p)) for p in ("seam", "esc", "end", "reject", "text")] == [N_SEAM, N_ESC, N_END, N_REJECT, N_TEXT]
    assert all(16384 <= len(d) <= 17000 for n, d in wide.items() if not n.startswith("text/"))
    sizes = sorted({len(d) - 5 - 16384 for d in _group(wide, "end").values()})
    assert sizes == sorted(64 * g + r for g in range(9) for r in (-1, 0, 1))
    assert (len(wide[f"reject/{W.REJECT_SIZE}/at"]) - 5) % W.PASS not in (0, W.PASS - 1)      # the last pass is partial


def test_oracle_reproduces_the_reference_on_every_case(orc, wide, golden):
    probes = F.Probes(orc.lib, "orc")
    bad = []
    for name, data in wide.items():
        ok, out = probes.run("forward_dict", data)
        if (int(ok), F.digest(out)) != (golden[name]["dict_ok"], golden[name]["sha256"]):
            bad.append(name)
    assert not bad, f"{len(bad)} cases differ from the reference, first {bad[:5]}"


def test_reject_leaves_the_buffer_untouched(orc, wide, golden):
    at, above = f"reject/{W.REJECT_SIZE}/at", f"reject/{W.REJECT_SIZE}/above"
    assert (golden[at]["dict_ok"], golden[above]["dict_ok"]) == (1, 0)
    assert golden[above]["sha256"] == F.digest(wide[above]) and golden[at]["sha256"] != F.digest(wide[at])


def test_the_restatement_is_the_filter(words, wide, golden):
    """forward_dict_w without a planted mistake, padded as the filter pads, is what the reference recorded (on a sample: it is slow)"""
    names = sorted(wide)[::37] + [f"reject/{W.REJECT_SIZE}/at"]
    for name in names:
        data = wide[name]
        out = W.forward_dict_w(data, words)
        assert golden[name]["dict_ok"] == 1 and len(out) <= len(data)
        assert F.digest(out + b"\x20" * (len(data) - len(out))) == golden[name]["sha256"], name


def test_seam_cases_notice_a_chain_forgotten_between_steps_and_between_passes(words, wide):
    """every seam case whose word lies across its seam changes when the chain is forgotten at the multiples of 64, those at a
    multiple of 128 (the kernel's pass seams) or of 256 also when it is forgotten at those multiples only; the cases whose word
    ends at or starts on the seam are the controls and do not change.  (Forgotten inside the adversarial head only: the four-letter words behind it lie across
    multiples of 64 as well and would make every case change.)"""
    n64 = n128 = n256 = 0
    for name, data in _group(wide, "seam").items():
        s, wl, back, gap = (int(x) for x in name.split("/")[1:])
        right = W.forward_dict_w(data, words)
        across = W.seam_straddles(s, wl, back)
        assert (W.forward_dict_w(data, words, forget=64, upto=s + W.SEAM_HEAD) != right) == across, name
        for width in (W.PASS, W.PASS4):
            assert (W.forward_dict_w(data, words, forget=width, upto=s + W.SEAM_HEAD) != right) == (across and s % width == 0), (name, width)
        n64 += across
        n128 += across and s % W.PASS == 0
        n256 += across and s % W.PASS4 == 0
    assert (n64, n128, n256) == (N_STRADDLE_64, N_STRADDLE_128, N_STRADDLE_256)


def test_escape_cases_notice_an_escape_counted_as_one_byte(words, wide):
    esc = _group(wide, "esc")
    assert len(esc) == N_ESC
    for name, data in esc.items():
        assert W.forward_dict_w(data, words, esc_len=1) != W.forward_dict_w(data, words), name
