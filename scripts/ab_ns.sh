#!/bin/bash
# Interleaved A/B of the NS training step: bench.py --config ns with the in-tree library
# ("cur") and abl/abl_<name>.so variants. usage: scripts/ab_ns.sh name1 [name2 ...]
# (results under $MMRE_OUT, default bench_out/)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
out=${MMRE_OUT:-bench_out}/ab_ns
mkdir -p $out
for rep in 1 2; do
  for v in cur "$@"; do
    if [ "$v" = cur ]; then L=; else L=abl/abl_$v.so; fi
    MMRE_LIB=$L timeout -k 10 200 python -u bench.py --config ns --full --no-cpu-baseline \
        > $out/$v.$rep.json 2> $out/$v.$rep.err || exit 1
    python - "$v" $out/$v.$rep.json <<'PY'
import json, sys
d = [json.loads(l) for l in open(sys.argv[2]) if l.startswith("{")][0]
print(sys.argv[1], "step_ms %.4f" % d["ms_per_step"], "fused_ms %.4f" % d["roofline"]["kernel_ms"], d["build"]["sha256"])
PY
  done
done
