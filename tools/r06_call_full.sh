OUT=${OUT:-bench_runs/full}
mkdir -p $OUT
timeout 2400 python -m pytest tests -x -q -m gpu > $OUT/pytest.log 2>&1; echo "rc $?" >> $OUT/pytest.log
tail -8 $OUT/pytest.log
timeout 600 python bench.py --steps 20 --warmup 5 --full > $OUT/bench_default.json 2> $OUT/bench_default.err; tail -c 600 $OUT/bench_default.err
python tools/show_bench.py $OUT/bench_default.json 2>/dev/null | head -40
