#!/bin/bash
# Round 5 end, part B: rocprofv3 kernel-trace stats (CSV) of the bench lines, then the HBM PMC
# passes (FETCH_SIZE / WRITE_SIZE, one counter group a run, no tracing) of C2 and C3.
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=gpurun_out/round_end_b
mkdir -p $O
prof() {  # name, bench args
  local n=$1; shift
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$n -o run -- \
      python3 bench.py "$@" > $O/prof_$n.json 2> $O/prof_$n.err
}
prof c2 --steps 60 --warmup 10 --full --no-cpu-baseline &&
prof c2s1 --steps 60 --warmup 10 --full --no-cpu-baseline --streams 1 &&
prof c3 --config c3 --steps 6 --warmup 2 --streams 1 --iso-steps 2 --full --no-cpu-baseline &&
prof c4s1 --config c4 --steps 60 --warmup 10 --streams 1 --full --no-cpu-baseline &&
prof c5 --config c5 --steps 6 --warmup 2 --streams 1 --iso-steps 2 --full --no-cpu-baseline &&
for grp in FETCH_SIZE WRITE_SIZE; do
  timeout -s KILL 240 rocprofv3 --pmc $grp --output-format csv -d $O/pmc_c3_$grp -o run -- \
      python3 bench.py --config c3 --steps 3 --warmup 1 --streams 1 --iso-steps 1 --no-cpu-baseline \
      --no-kernel-timing --no-stream-probe > $O/pmc_c3_$grp.log 2>&1 || exit 1
  timeout -s KILL 240 rocprofv3 --pmc $grp --output-format csv -d $O/pmc_c2_$grp -o run -- \
      python3 bench.py --steps 6 --warmup 2 --streams 1 --no-cpu-baseline --no-kernel-timing \
      --no-stream-probe > $O/pmc_c2_$grp.log 2>&1 || exit 1
done
echo finB-done
