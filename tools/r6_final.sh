# Round 6 on the final code: smoke, the full GPU suite and the --full bench line.   bash tools/r6_final.sh <output folder>
out=${1:?usage: bash tools/r6_final.sh <output folder>}
mkdir -p $out
python -c "import __graft_entry__ as g; g.smoke()" > $out/smoke.txt 2>&1; tail -2 $out/smoke.txt
timeout 2400 python -m pytest tests/ -q -m gpu > $out/r6_pytest_gpu.log 2>&1; tail -4 $out/r6_pytest_gpu.log
t0=$(date +%s)
timeout 900 python bench.py --full > $out/r6_bench_default.json 2> $out/default.err
echo "default bench.py run: $(( $(date +%s) - t0 )) s wall" > $out/r6_bench_default_wall.txt
tail -c 900 $out/r6_bench_default.json; cat $out/r6_bench_default_wall.txt
