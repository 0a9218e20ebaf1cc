#!/bin/bash
# sample clocks / power while the B=64 step runs (the complete 1000-step loop of `bench.py --full` is ~20 s of steady load)
# usage (from the repo root): tools/power_probe.sh <output dir>
out=${1:?usage: tools/power_probe.sh <output dir>}
mkdir -p $out
(python bench.py --full --no-cpu-baseline --no-extras --steps 100 --warmup 5 > $out/bench.json 2>/dev/null) &
BP=$!
: > $out/smi.txt
while kill -0 $BP 2>/dev/null; do
  rocm-smi --showpower --showclocks --showtemp 2>/dev/null | grep -E "sclk|fclk|Power|junction" | sed -e 's/.*: //' | tr '\n' ' ' >> $out/smi.txt; echo >> $out/smi.txt
  sleep 0.7
done
grep -v "(9[0-9]Mhz)\|(1[0-9][0-9]Mhz)" $out/smi.txt | tail -40
