O=${1:?usage: bash tools/exp/exp31.sh <output dir>}; mkdir -p $O
for i in 1 2 3; do timeout -k 10 300 python -u bench.py --full --no-cpu-baseline 2>/dev/null > $O/exp31_$i.json; python -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'], d['roofline']['peak_measured'])" $O/exp31_$i.json; done
