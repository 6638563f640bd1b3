# the round's bench lines once more on the frozen library, with roofline.traffic from profiles/pmc_traffic.json
#   bash tools/bench_lines.sh <tag> [out_dir]      (from the repository root; the lines land in out_dir, default bench_out/)
T=${1:-r05}
O=${2:-bench_out}
mkdir -p $O
python bench.py --full > $O/${T}_a_bench.json 2> $O/${T}_a_bench.err
python bench.py --full --config silesia --steps 4 --warmup 1 > $O/${T}_m5_bench.json 2> $O/${T}_m5_bench.err
python bench.py --full --config mix5 --steps 4 --warmup 1 > $O/${T}_m2_bench.json 2> $O/${T}_m2_bench.err
python bench.py --full --split 127 --steps 4 --warmup 1 > $O/${T}_p127_bench.json 2> $O/${T}_p127_bench.err
python -c "
import json
for t in ('a','m5','m2','p127'):
    d=json.load(open('$O/${T}_%s_bench.json'%t)); r=d['roofline']; print(t, d['value'], r['frac'], r['traffic'], (d.get('cpu_baseline') or {}).get('value'))
"
