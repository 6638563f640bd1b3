#!/usr/bin/env python3
"""Evidence run (python tools/gpu_soak_batch.py [seconds] [seed]): the BATCH entry points -- CSCMI_EncodeDeviceChunkBatch / CSCMI_FlushBatch / CSCMI_DecodeBatch,
i.e. the k_encode_runs_multi_* kernels and k_decode_run_multi that the -pN split and the archiver use -- on random batches from tests/soak_gen.py (batch_round: 2 .. 900
streams a round, rounds beyond 768 streams of one dispatch row, every stream its own corpus kind / offset / size, level or custom props and dictionary size; mixed in one
batch call: one launch per kernel flavour), inputs resident in device memory, 2 MiB chunk rounds.  Every stream is compared byte for byte with the reference build's
(oracle/_ref/libcsc_ref.so, zeroing allocator; the oracle where that is absent), every batch-decoded stream with the reference DECODER's bytes.  tests/test_gpu_soak.py
runs the same generator on fixed seeds and round counts.  Exit code 1 on the first difference."""
import hashlib, os, random, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa
import csc_amd
import soak_gen

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 600.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 20261005
rng = random.Random(seed)
prod = csc_amd.load()
chk, za, is_ref = soak_gen.checker()
print(f"checker: {'reference build (oracle/_ref)' if is_ref else 'oracle'}; seed {seed}; budget {budget:.0f} s", flush=True)

t_start = time.time()
rounds = n_streams = n_bytes = n_ref_rt = 0
while time.time() - t_start < budget:
    specs = soak_gen.batch_round(rng, 900, 30_000_000)      # (byte cap per round: the checker encodes all of it on the host)
    S = len(specs)
    datas = [soak_gen.build_input(s) for s in specs]
    total = sum(len(d) for d in datas)
    # ---- the HIP path: one batch call per chunk round, one flush for all ----
    torch.cuda.synchronize()
    t0 = time.time()
    got, k = soak_gen.encode_batch(prod, [soak_gen.props_of(prod, s) for s in specs], datas)
    t_gpu = time.time() - t0
    # ---- the checker, eight host threads (ctypes releases the GIL) ----
    first = soak_gen.check_one(chk, za, specs[0], datas[0])      # (alone: whatever the checker sets up on first use is set up by one thread)
    with ThreadPoolExecutor(8) as ex:
        want = [first] + list(ex.map(lambda i: soak_gen.check_one(chk, za, specs[i], datas[i]), range(1, S)))
    bad = [i for i in range(S) if want[i][0] != 0 or got[i] != want[i][1]]
    # ---- batch decode of the HIP streams, 256 handles a call ----
    dec = soak_gen.decode_batch(prod, got)
    dec_bad = [i for i in range(S) if dec[i] != (want[i][2], want[i][3])]
    n_ref_rt += sum(1 for i in range(S) if i not in dec_bad and want[i][3] != datas[i])
    rounds += 1; n_streams += S; n_bytes += total
    rows = sorted(set(s["row"] for s in specs))
    print(f"round {rounds:3d}: {S:4d} streams, {total:10d} B, rows {rows}, {k} chunk rounds, HIP encode {total / 1e6 / t_gpu:8.2f} MB/s -> "
          f"{'all streams == reference, all batch decodes == reference decoder' if not bad and not dec_bad else 'DIFFERS: encode %s decode %s' % ([soak_gen.describe(seed, rounds - 1, specs[i]) for i in bad[:2]], [soak_gen.describe(seed, rounds - 1, specs[i]) for i in dec_bad[:2]])}", flush=True)
    if bad or dec_bad:
        print("FAILED", flush=True)
        sys.exit(1)
print(f"ALL OK: {rounds} rounds, {n_streams} streams ({n_ref_rt} of them streams the reference's own decoder does not turn back into the input: reproduced), {n_bytes} input bytes, "
      f"{time.time() - t_start:.0f} s; library sha256[:16] {hashlib.sha256(open(os.path.join(ROOT, 'csc_amd', 'libcsc_mi355x.so'), 'rb').read()).hexdigest()[:16]}")
