"""CPU tier: the soak generator's single-stream and renormalisation cases through the oracle (the C restatement the GPU
tests fall back to) against the reference build (oracle/_ref), encode and decode: it keeps the checker honest wherever
the GPU tier runs without oracle/_ref.  Skips when oracle/_ref is not built."""
import ctypes as C
import random

import pytest

import soak_gen

SEEDS, CASES, CAP = (20261501, 20261502, 20261503), 30, 1 << 20
RENORM_SEEDS = (20261601, 20261602)


def _pair(orc, zalloc, ref, spec, data, set_pos=None):
    out = []
    for lib, hook in ((orc, "orc_debug_set_pos"), (ref, "ref_debug_set_pos")):
        sp = None
        if set_pos:
            sp = getattr(lib.lib, hook)
            sp.argtypes = [C.c_void_p, C.c_uint32]
            sp.restype = None
        out.append(soak_gen.check_one(lib, zalloc, spec, data, set_pos=sp))
    return out


@pytest.mark.parametrize("seed", soak_gen.seeds(SEEDS))
def test_oracle_equals_reference_on_soak_cases(orc, zalloc, ref, seed):
    rng = random.Random(seed)
    for idx in range(CASES):
        spec = soak_gen.single_case(rng, CAP)
        data = soak_gen.build_input(spec)
        a, b = _pair(orc, zalloc, ref, spec, data)
        assert a[:2] == b[:2], f"oracle stream differs from the reference's: {soak_gen.describe(seed, idx, spec)}"
        assert a[2:] == b[2:], f"oracle decoder differs from the reference's: {soak_gen.describe(seed, idx, spec)}"


@pytest.mark.parametrize("seed", soak_gen.seeds(RENORM_SEEDS))
def test_oracle_equals_reference_across_renormalisation(orc, zalloc, ref, seed):
    rng = random.Random(seed)
    for idx in range(3):
        spec = soak_gen.renorm_case(rng)
        data = soak_gen.build_input(spec)
        a, b = _pair(orc, zalloc, ref, spec, data, set_pos=True)
        assert a == b, f"oracle differs from the reference across pos_ renormalisation: {soak_gen.describe(seed, idx, spec)}"
