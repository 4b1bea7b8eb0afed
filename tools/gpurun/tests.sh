#!/bin/bash
# GPU parity suite (+ optional full bench line), each step under its own time limit.
# Results go to $O (default: out/tests under the repository root).
O=${O:-out/tests}
mkdir -p $O
timeout -k 10 400 python -u -m pytest tests -m gpu -x -v --timeout 180 --timeout-method thread \
  > $O/pytest_gpu.log 2>&1 || { tail -40 $O/pytest_gpu.log; exit 1; }
tail -3 $O/pytest_gpu.log
grep -h "latches:\|device batches" $O/pytest_gpu.log | head -5
if [ -n "$BENCH_DEFAULT" ]; then
  timeout -k 10 400 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err \
    || { tail -20 $O/bench_default.err; exit 1; }
  cat $O/bench_default.json
fi
for w in ${BENCH_WORKLOADS:-}; do
  timeout -k 10 300 python bench.py --steps 10 --warmup 2 --workload $w \
    > $O/bench_$w.json 2> $O/bench_$w.err || { tail -20 $O/bench_$w.err; exit 1; }
  python -c "import json;d=json.load(open('$O/bench_$w.json'));print('$w', d['ms_per_step'], d['value'])"
done
