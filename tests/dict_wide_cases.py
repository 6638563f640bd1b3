"""Inputs for the dictionary filter that walks several steps of 64 positions a pass (two, as built: kDictW) (flt_forward_dict, csc_kernels_blocks.inc):
everything that can go wrong where two steps, or two passes, meet.  Shared by tools/make_golden_dict_wide.py (which records
what the REFERENCE makes of them in tests/golden/dict_wide.json), tests/test_dict_wide_cases.py (oracle, CPU) and
tests/test_gpu_dict_wide.py (the HIP kernels).  A plain module like filter_cases.py, whose parts it is built from.

  cases(words) -> name -> bytes        every run is 16 384 .. 17 000 bytes long except the two whole-text stretches
    seam/<s>/<len>/<back>/<gap>        a <len>-letter word starting <back> = 4 .. 0 bytes below the seam s = 64 k, k = 1 .. 9, behind a
                                       `with` that ends <gap> = 0 .. 3 bytes before it: the chain reaches the word, and with it the
                                       seam, from every phase.  With two steps a pass (what the kernel does) every multiple of 128
                                       is a pass seam and the odd multiples of 64 lie inside a pass; with four, 256 and 512 are the
                                       pass seams: the seams serve any number of steps a pass up to eight
    esc/<s>/<n>                        n = 1, 2, 63, 64, 65 bytes >= 0x82 ending at seam s = 64 .. 320: [s - n, s) (the one run that
                                       does not fit below its seam, 65 bytes at 64, is [0, 65)).  Two output bytes each, so every
                                       later offset moves; four-letter words behind them pay for the 82 % test
    end/<size>/<len>/<back>            size - 5 = 16 384 + 64 g + r, g = 0 .. 8, r = -1, 0, 1: the walked range ends in every group of
                                       the last pass; text, with a word starting 9 .. 5 bytes before the end
    reject/<size>/at|above             dstSize == floor(0.82 * size) and one more, for a size whose last pass is partial
    text/65536, text/200000            stretches of the text corpus

forward_dict_w() is filter_cases.forward_dict with two more places for a planted mistake: the chain forgotten at every multiple
of `forget` (below `upto`: the words that fill a buffer behind its adversarial head lie across such multiples too, and would
make every case "notice"), and an escape counted as `esc_len` bytes."""
from filter_cases import DICT_MIN, FILLER, _counted, _dict_buf, _put, _text, forward_dict  # noqa: F401

SEAMS = tuple(64 * k for k in range(1, 10))
PASS = 128                                                  # positions a pass of the kernel covers: kDictW = 2 steps of 64
PASS4 = 256                                                 # ... and a pass of four steps, the width the cases were first laid out for
WORDS_BY_LEN = {2: b"at", 3: b"the", 4: b"that"}
ESC_SEAMS = (64, 128, 192, 256, 320)
ESC_RUNS = (1, 2, 63, 64, 65)
END_GROUPS = tuple(range(9))
END_REST = (-1, 0, 1)
REJECT_SIZE = 16384 + 64 + 7 + 5                            # the last pass: one full step and seven positions of the second


SEAM_HEAD = 64                                              # filler behind a seam before the words that pay for the 82 % test


def seam_straddles(s, wl, back):
    """does the word starting `back` bytes below seam s lie across it (letters on both sides)?"""
    return 0 < back < wl


def seam_cases():
    out = {}
    for s in SEAMS:
        for wl, w in WORDS_BY_LEN.items():
            for back in range(4, -1, -1):
                for gap in range(4):
                    head = bytearray(FILLER * (s + SEAM_HEAD))
                    at = s - back
                    _put(head, at - gap - 4, b"with")
                    _put(head, at, w)
                    out[f"seam/{s}/{wl}/{back}/{gap}"] = _dict_buf(16400, bytes(head))
    return out


def esc_cases():
    out = {}
    for s in ESC_SEAMS:
        for n in ESC_RUNS:
            lo = max(0, s - n)
            head = bytearray(FILLER * (lo + n + 8))
            _put(head, lo, bytes(0x82 + (7 * k) % 0x7E for k in range(n)))
            out[f"esc/{s}/{n}"] = _dict_buf(16400, bytes(head))
    return out


def end_cases():
    out = {}
    for g in END_GROUPS:
        for r in END_REST:
            size = DICT_MIN + 64 * g + r + 5
            for wl, w in WORDS_BY_LEN.items():
                for back in range(9, 4, -1):
                    b = bytearray(_text(size, 1000 * g))
                    _put(b, size - 12, FILLER * 12)
                    _put(b, size - back, w)
                    out[f"end/{size}/{wl}/{back}"] = bytes(b)
    return out


def reject_cases():
    lim = int(float(REJECT_SIZE) * 0.82)
    return {f"reject/{REJECT_SIZE}/at": _counted(REJECT_SIZE, lim, 3), f"reject/{REJECT_SIZE}/above": _counted(REJECT_SIZE, lim + 1, 3)}


def text_cases():
    return {"text/65536": _text(65536, 12345), "text/200000": _text(200000, 777)}


def cases(words):
    assert all(w in words for w in WORDS_BY_LEN.values()) and b"with" in words
    out = {}
    for part in (seam_cases(), esc_cases(), end_cases(), reject_cases(), text_cases()):
        assert not set(part) & set(out)
        out.update(part)
    lim = int(float(REJECT_SIZE) * 0.82)                    # what the generator intended, counted in plain Python
    assert forward_dict(out[f"reject/{REJECT_SIZE}/at"], words)[2] == lim
    assert forward_dict(out[f"reject/{REJECT_SIZE}/above"], words)[2] == lim + 1
    return out


def forward_dict_w(buf, words, forget=None, upto=None, esc_len=2):
    """Filters::Foward_Dict's output bytes before the 82 % test (no padding).  forget=N: a token starts at every multiple of N
    (below `upto`, if given) whatever the chain says; esc_len=1: an escaped byte counted as one output byte."""
    size = len(buf)
    trie = {w: 0x82 + k for k, w in enumerate(words)}
    prefixes = {w[:k] for w in words for k in range(1, len(w) + 1)}
    esc = (lambda c: bytes([254, c])) if esc_len == 2 else (lambda c: bytes([c]))
    dst = bytearray()
    i = 0
    while i < size - 5:
        c = buf[i]
        adv = 1
        if 0x61 <= c <= 0x7A:
            sym, j = 0, 0
            while bytes(buf[i:i + j + 1]) in prefixes and i + j < size:
                j += 1
                if bytes(buf[i:i + j]) in trie:
                    sym, adv = trie[bytes(buf[i:i + j])], j
            dst.append(sym if sym else c)
        elif c >= 0x82:
            dst += esc(c)
        else:
            dst.append(c)
        nxt = i + adv
        if forget and nxt // forget != i // forget and (upto is None or nxt // forget * forget < upto):
            nxt = nxt // forget * forget
        i = nxt
    for c in buf[i:]:
        dst += esc(c) if c >= 0x82 else bytes([c])
    return bytes(dst)
