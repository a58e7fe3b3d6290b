export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${O:-$(mktemp -d)}   # traces, counter passes and bench lines go here; the summaries are copied to profiles/
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/r01_trace -o run -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --c4-batches 0 --c5-steps 0 > $O/r01_bench_traced.json 2> $O/r01_trace.log && \
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/r01_fetch -o run -- python3 $R/bench.py --steps 3 --warmup 1 > $O/r01_fetch.log 2>&1 && \
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/r01_write -o run -- python3 $R/bench.py --steps 3 --warmup 1 > $O/r01_write.log 2>&1 && \
python3 $R/tools/pmc_traffic.py --trace $O/r01_trace --fetch $O/r01_fetch --write $O/r01_write --steps 25 --out $O/pmc_traffic.json > /dev/null && \
cp $O/pmc_traffic.json $R/profiles/pmc_traffic.json && \
timeout -k 10 300 python3 $R/bench.py --full > $O/r01_bench.json 2> $O/r01_bench.err
rc=$?
cp $O/r01_trace/run_kernel_stats.csv $R/profiles/r01_kernel_stats.csv
cp $O/r01_bench_traced.json $O/r01_bench.json $R/profiles/
echo rc=$rc
cat $O/r01_bench_traced.json; cat $O/r01_bench.json
