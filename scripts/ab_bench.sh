#!/bin/bash
# Same-box A/B of whole-rollout rates: scripts/ab_bench.sh <workload> <steps> <leg>...   (interleaved rounds, ROUNDS=3 by default)
# A leg is "shipped" (this tree's library), a library name (graphs4cfd_amd/lib/libg4c_ws_<name>.so, this tree's python) or
# "<label>=<dir>": another tree (the parent commit's checkout, built there) running its own bench.py on its own library.
cd "$GRAFT_REPO_ROOT"
W=$1; S=$2; shift 2
for r in $(seq 1 ${ROUNDS:-3}); do for v in "$@"; do
  D=$PWD; N=$v
  case "$v" in
    shipped) L=$PWD/graphs4cfd_amd/lib/libg4c.so;;
    *=*) N=${v%%=*}; D=$(cd "${v#*=}" && pwd); L=$D/graphs4cfd_amd/lib/libg4c.so;;
    *) L=$PWD/graphs4cfd_amd/lib/libg4c_ws_$v.so;;
  esac
  ( cd "$D" && G4C_LIB_PATH=$L timeout -k 10 600 python bench.py --workload $W --steps $S --no-cpu-baseline --no-side-configs --no-roofline --no-strict-range 2>&1 | tail -1 | \
    python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$W', '$N', round(d['value'],2), 'steps/s', round(d['ms_per_step'],4), 'ms')" ) || exit 1
done; done
