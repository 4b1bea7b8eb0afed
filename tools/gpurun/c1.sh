#!/bin/bash
# GPU tests + the full C1 echo line (every codec mode and the reference's Snappy).
# Results go to $O (default: out/c1 under the repository root).
O=${O:-out/c1}
mkdir -p $O
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 180 --timeout-method thread \
  > $O/pytest_gpu.log 2>&1 || { tail -40 $O/pytest_gpu.log; exit 1; }
tail -2 $O/pytest_gpu.log
timeout -k 10 300 python bench.py --full --workload c1-echo --steps 20 > $O/bench_c1.json 2> $O/bench_c1.err \
  || { tail -20 $O/bench_c1.err; exit 1; }
cat $O/bench_c1.json
