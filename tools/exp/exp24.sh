set -e
O=${1:?usage: bash tools/exp/exp24.sh <output dir>}; mkdir -p $O
timeout -k 10 300 python -m pytest tests/test_gpu_round4.py -x -q -m gpu -k "half_empty" > $O/exp24_t0.txt 2>&1 || { tail -30 $O/exp24_t0.txt; exit 1; }
tail -3 $O/exp24_t0.txt
timeout -k 10 300 python -u bench.py --full --variant base --lcm_steps 8 --batch 32 --no-cpu-baseline > $O/exp24_base.json 2> $O/exp24_base.err
python - $O/exp24_base.json <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'])
for k,v in list(d['roofline']['step_breakdown'].items())[:12]: print('  ',k,v)
PY
timeout -k 10 900 python -m pytest tests/test_gpu_parity.py tests/test_gpu_round2.py tests/test_gpu_round3.py -x -q -m gpu > $O/exp24_tests.txt 2>&1 || { tail -30 $O/exp24_tests.txt; exit 1; }
tail -3 $O/exp24_tests.txt
