# GPU machine: the whole -m gpu suite (one process), then the benchmark with --full.  Logs go to DIR (default: gpu_results/<OUT>).
OUT=${OUT:-r3a}
DIR=${DIR:-gpu_results/$OUT}
mkdir -p $DIR
timeout -k 10 1000 python -m pytest tests -m gpu -q -s --durations=15 > $DIR/tests.log 2>&1; echo "pytest rc=$?" >> $DIR/tests.log
grep -E "passed|failed|FAILED|Error|worst|fullsize|rc=" $DIR/tests.log | cut -c1-600 | tail -40
timeout -k 10 500 python bench.py --full --steps 20 --warmup 5 > $DIR/bench.json 2> $DIR/bench.err; tail -c 1500 $DIR/bench.json; tail -8 $DIR/bench.err
