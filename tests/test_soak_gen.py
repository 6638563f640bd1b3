"""CPU tier: tests/soak_gen.py, the seeded case generator of the soaks -- deterministic per seed, and the default seeds of the
GPU soak tests reach what the generator is meant to reach."""
import json
import random

import soak_gen
import test_gpu_forms
import test_gpu_soak


def test_same_seed_same_specs():
    for seed in (1, 77, 20261101):
        a, b = random.Random(seed), random.Random(seed)
        assert [soak_gen.single_case(a) for _ in range(40)] == [soak_gen.single_case(b) for _ in range(40)]
        assert [soak_gen.batch_round(a, 900, 6_000_000) for _ in range(4)] == [soak_gen.batch_round(b, 900, 6_000_000) for _ in range(4)]
        assert [soak_gen.renorm_case(a) for _ in range(5)] == [soak_gen.renorm_case(b) for _ in range(5)]
    assert test_gpu_soak.single_specs(5) == test_gpu_soak.single_specs(5)
    assert soak_gen.single_case(random.Random(1)) != soak_gen.single_case(random.Random(2))


def test_specs_are_one_json_line():
    spec = soak_gen.single_case(random.Random(3))
    line = soak_gen.describe(3, 0, spec)
    assert "\n" not in line and json.loads(line.split(" spec ", 1)[1]) == spec


def test_restated_props_init_gives_the_oracles_rows(orc):
    """spec_row (no library) against the parser bits of the oracle's own CSCEncProps_Init + overrides, for generated specs"""
    for seed in (1, 2, 3):
        rng = random.Random(seed)
        specs = [soak_gen.single_case(rng) for _ in range(150)] + [soak_gen.renorm_case(rng) for _ in range(20)]
        specs += [s for _ in range(3) for s in soak_gen.batch_round(rng, 300, 6_000_000)]
        for s in specs:
            assert soak_gen.row_of(soak_gen.props_of(orc, s)) == s["row"] == soak_gen.spec_row(s), s
    for level in (1, 2, 3, 4, 5):
        for d in (1, 30000, 1 << 20, 5 << 20, 20 << 20, 100 << 20, 300 << 20):
            spec = {"level": level, "dict": d, "props": {}}
            assert soak_gen.row_of(soak_gen.props_of(orc, spec)) == soak_gen.spec_row(spec), (level, d)


def test_form_variants_select_their_rows(orc):
    for row, f in test_gpu_forms.FORMS.items():
        for k in range(len(f["variants"])):
            spec = test_gpu_forms._spec(row, k, 1 << 20, [])
            assert soak_gen.spec_row(spec) == row == soak_gen.row_of(soak_gen.props_of(orc, spec)), (row, k)
    for row, count in test_gpu_forms.THRESHOLD_CASES:
        assert {soak_gen.spec_row(s) for s in test_gpu_forms._small_streams(row, count, count)} == {row}


def test_default_seeds_reach_every_row_and_shape():
    single = [s for seed in test_gpu_soak.SINGLE_SEEDS for s in test_gpu_soak.single_specs(seed)]
    rounds = [r for seed in test_gpu_soak.BATCH_SEEDS for r in test_gpu_soak.batch_specs(seed)]
    renorm = [s for seed in test_gpu_soak.RENORM_SEEDS for s in test_gpu_soak.renorm_specs(seed)]
    batch = [s for r in rounds for s in r]
    allspecs = single + batch + renorm

    def n_of(s):
        return sum(p[1] if p[0] == "zeros" else p[3] for p in s["parts"])

    assert {s["row"] for s in allspecs} == set(test_gpu_forms.FORMS)
    assert any(s["dict"] + (10 << 10) < n_of(s) for s in single)             # window wrap (CSCEncProps_Init adds 10 KiB)
    assert any(s["nofilters"] for s in single) and any(s["nofilters"] for s in batch)
    assert any(s["max_read"] for s in single) and any(s["dec_max_read"] for s in single)
    assert all(s["max_read"] is None or s["max_read"] >= 257 for s in single)
    assert all(soak_gen.RENORM_LINE - n_of(s) <= s["pos"] <= soak_gen.RENORM_LINE for s in renorm)
    assert any(n_of(s) <= 2 for s in single + batch)
    assert any(len(s["parts"]) > 1 for s in single)                          # splices
    assert max(len(r) for r in rounds) > test_gpu_forms.THRESHOLDS["kD4MultiMax"] and min(len(r) for r in rounds) <= 40
