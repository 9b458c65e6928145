#!/bin/bash
# round 3 evidence set, one GPU call: the whole GPU suite, the judged measurement set (bench line, rocprofv3
# kernel stats, FETCH_SIZE / WRITE_SIZE passes), the per-GPU block counts of configs[3] (512 / 1024 / 2048 /
# 4096) with the 2-rank gloo rehearsal, the corpus table and the R-era line.
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p "$OUT"
PYTHONUNBUFFERED=1 timeout -k 10 900 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider 2>&1 | tail -6 | tee $OUT/r03_tests.txt
grep -q " passed" $OUT/r03_tests.txt && ! grep -q "failed" $OUT/r03_tests.txt || exit 1
PROF_TAG=r03 bash tools/profile_round.sh > $OUT/r03_profile.log 2>&1 || { tail -20 $OUT/r03_profile.log; exit 1; }
tail -3 $OUT/r03_profile.log | cut -c1-300
TAG=r03 bash tools/scaling_lines.sh > $OUT/r03_scaling.log 2>&1 || { tail -20 $OUT/r03_scaling.log; exit 1; }
tail -8 $OUT/r03_scaling.log | cut -c1-400
timeout -k 10 300 python tools/microbench/corpus_batch.py > $OUT/r03_corpus_batch.txt 2>&1 || tail -5 $OUT/r03_corpus_batch.txt
tail -9 $OUT/r03_corpus_batch.txt | cut -c1-200
timeout -k 10 300 python bench.py --full --steps 2 --warmup 1 --codec rc > $OUT/r03_rc.log 2>&1 && grep '^{' $OUT/r03_rc.log > $OUT/r03_rc_bench_line.json
