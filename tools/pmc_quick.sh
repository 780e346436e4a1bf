#!/bin/bash
# One counter pass of its own (no tracing) over bench.py's headline launches: SQ_INSTS_VALU, SQ_INSTS_SALU, SQ_WAIT_ANY, SQ_ACTIVE_INST_VALU, SQ_WAVES
# of kmpc_solve_fast_kernel<double,20> at 4096 problems, averaged over its dispatches and divided by the batch.  Run on the GPU box from the repo root:
#   bash tools/pmc_quick.sh <label> <out.json>     appends runs[<label>] to out.json (the format of profiles/r5_pmc_counters.json)
set -eo pipefail
export TMPDIR=/tmp
LABEL=${1:?label}; JSON=${2:?out.json}
DIR=$(mktemp -d /tmp/pmc_quick.XXXXXX)
CMD="python3 bench.py --gpus 1 --steps 4 --warmup 2 --no-cpu-baseline"
rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_WAVES -d $DIR -o c -- $CMD > $DIR/out.txt 2> $DIR/err.txt
python3 - "$LABEL" "$JSON" "$DIR" "$CMD" <<'EOF'
import glob, json, os, sqlite3, sys
label, path, d, cmd = sys.argv[1:5]
B = 4096
out = json.load(open(path)) if os.path.exists(path) else {
    "note": "rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_WAVES (one pass, no tracing), averaged over the dispatches of "
            "kmpc_solve_fast_kernel<double,20> at 4096 problems; SQ_* summed over the chip; SQ_WAIT_ANY / SQ_ACTIVE_INST_VALU in quad-cycles", "runs": {}}
k = {}
c = sqlite3.connect(glob.glob(d + "/**/*_results.db", recursive=True)[0])
for name, val, n in c.execute("select counter_name, avg(value), count(*) from counters_collection where kernel_name like ? and grid_size=? group by counter_name",
                              ("%kmpc_solve_fast_kernel<double, 20>%", B * 64)):
    k[name] = val; k["dispatches_averaged"] = n
k["command"] = cmd
k["per_solve"] = {x: k[x] / B for x in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_WAIT_ANY", "SQ_ACTIVE_INST_VALU") if x in k}
out["runs"][label] = k
json.dump(out, open(path, "w"), indent=1)
print(label, json.dumps(k["per_solve"]))
EOF
rm -rf $DIR
