# training-step artefacts for profiles/: bench lines of both paths, rocprofv3 kernel stats + last-step breakdown of the chain path
# usage, from the repository root: bash scripts/gpu_train_profile.sh OUT_DIR
R=$PWD; O=$(realpath -m "${1:?usage: bash scripts/gpu_train_profile.sh OUT_DIR}"); mkdir -p $O
python bench.py --full --mode train --steps 20 --warmup 5 > $O/train_bench.json 2>$O/train_bench.err
python bench.py --mode train --train-precision f16x3_gemm --steps 20 --warmup 5 --no-cpu-baseline > $O/train_bench_gemm_path.json 2>/dev/null
python bench.py --mode train --train-precision fp32 --steps 20 --warmup 5 --no-cpu-baseline > $O/train_bench_fp32.json 2>/dev/null
cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/prof && timeout 300 rocprofv3 --kernel-trace --stats -d /tmp/prof -o run --output-format csv -- python $R/bench.py --mode train --steps 10 --warmup 3 --no-cpu-baseline > /dev/null 2>&1
cd $R; f=$(find /tmp/prof -name "*kernel_trace.csv" | head -1); python scripts/train_breakdown.py $f > $O/train_breakdown.txt 2>&1; cp $(find /tmp/prof -name "*kernel_stats.csv" | head -1) $O/train_kernel_stats.csv
for f in $O/train_bench*.json; do python -c "import json,sys; d=json.load(open('$f')); print('$f', d['ms_per_step'], d['value'], d['roofline']['frac'])"; done
head -20 $O/train_breakdown.txt
