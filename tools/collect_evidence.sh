set -x
O=${1:?usage: bash tools/collect_evidence.sh OUTPUT_DIR}
mkdir -p $O
export TMPDIR=/tmp
if [ -z "$VX_EVIDENCE_PROFILES_ONLY" ]; then
timeout 600 python bench.py --full > $O/bench_line.json 2> $O/bench_line.err
timeout 300 python bench.py --full --no-eager-baseline --no-cpu-baseline --dtype bf16 > $O/bench_autopet128_bf16.json 2>/dev/null
timeout 300 python bench.py --full --no-eager-baseline --no-cpu-baseline --workload brats128 > $O/bench_brats128_f32.json 2>/dev/null
timeout 300 python bench.py --full --no-eager-baseline --no-cpu-baseline --workload brats128 --dtype bf16 > $O/bench_brats128_bf16.json 2>/dev/null
timeout 300 python bench.py --full --no-eager-baseline --no-cpu-baseline --workload brats128 --batch 4 > $O/bench_brats128_b4_f32.json 2>/dev/null
timeout 300 python bench.py --full --no-eager-baseline --no-cpu-baseline --workload autopet96 > $O/bench_autopet96.json 2>/dev/null
timeout 300 python bench.py --full --no-eager-baseline --no-cpu-baseline --workload brats96 > $O/bench_brats96.json 2>/dev/null
fi
timeout 600 rocprofv3 --kernel-trace --stats -d $O/stats96 -o st --output-format csv -- python3 bench.py --workload autopet96 --steps 100 --warmup 10 --no-eager-baseline --no-cpu-baseline --no-kernel-pass --dispersion-steps 0 > $O/stats96.log 2>&1
timeout 600 rocprofv3 --kernel-trace --stats -d $O/stats -o st --output-format csv -- python3 bench.py --steps 100 --warmup 10 --no-eager-baseline --no-cpu-baseline --no-kernel-pass --dispersion-steps 0 > $O/stats.log 2>&1
# (flag kernels off: under --pmc kernels run one at a time, a polling kernel would never see its flag set)
VELOXSEG_TAPE_FLAGS=0 timeout 600 rocprofv3 --pmc FETCH_SIZE -d $O/fetch -o f --output-format csv -- python3 bench.py --full --steps 3 --warmup 2 --no-eager-baseline --no-cpu-baseline --dispersion-steps 0 > $O/fetch.log 2>&1
VELOXSEG_TAPE_FLAGS=0 timeout 600 rocprofv3 --pmc WRITE_SIZE -d $O/write -o w --output-format csv -- python3 bench.py --full --steps 3 --warmup 2 --no-eager-baseline --no-cpu-baseline --dispersion-steps 0 > $O/write.log 2>&1
python tools/pmc_traffic.py $(find $O/fetch -name '*counter_collection.csv') $(find $O/write -name '*counter_collection.csv') $O/pmc_traffic.json
find $O -name '*counter_collection.csv' -delete
find $O -name '*kernel_trace.csv' -delete
ls -la $O $O/stats
tail -1 $O/bench_line.json | cut -c1-300
