#!/bin/bash
# Same-box A/B of library variants (tools/ab_variant.sh): tools/ab_bench.sh <out.txt> <tag|base> [<tag> ...] [-- bench flags]
# Every variant runs the default bench workload (no CPU baseline, no PMC child passes), the whole list REPS times (default 2:
# A B A B) so that drift of the box shows.  One line per run: tag, particle-updates/s, ms/step, force-pass ms, rebin ms/step.
# Every run has its own time limit (RUN_TIMEOUT seconds, default 600); a run that fails or is killed ends the series.
out=$1; shift
tags=(); while [ $# -gt 0 ] && [ "$1" != "--" ]; do tags+=("$1"); shift; done
[ "$1" == "--" ] && shift
flags="${@:---steps 60 --warmup 10}"
: > $out
for rep in $(seq 1 ${REPS:-2}); do
  for t in "${tags[@]}"; do
    lib=""; [ "$t" != "base" ] && lib="ls1-mardyn_amd/lib/variants/libls1hip_$t.so"
    LS1HIP_LIB=$lib timeout -k 10 ${RUN_TIMEOUT:-600} python bench.py --full --no-cpu-baseline --no-live-pmc $flags 2>/dev/null > $out.json
    st=$?
    if [ $st -ne 0 ]; then echo "$t FAILED (exit $st)" >> $out; tail -1 $out; rm -f $out.json; exit 1; fi
    python -c "
import sys, json
d = json.loads(open('$out.json').read().strip().splitlines()[-1])
m = d['device_ms_per_step']
print('%-12s %.4g upd/s  %.3f ms/step  force %.4f  rebin %.3f  integrate %.3f  builds %s' % ('$t', d['value'], d['ms_per_step'], m['force'], m['rebin'], m['integrate'], d['config'].get('neighbour_lists', {}).get('list_builds')))
" >> $out || { echo "$t: no result line" >> $out; rm -f $out.json; exit 1; }
    tail -1 $out
  done
done
rm -f $out.json
