#!/bin/bash
# Round-3 measurement pass (run on the GPU box from the repo root) -> gpurun_out/r3/: bench lines of every workload, the config-3 kernel
# trace with the FETCH_SIZE / WRITE_SIZE counters of EVERY kernel (per-frame traffic table), counter summaries of the dominant kernels
# (stamped with the digest of their sources: bench.py's `traffic_stale`), kernel traces of configs 4 and 5.
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$PWD}
O=$R/gpurun_out/r3; mkdir -p $O
B="timeout 300 python $R/bench.py --full"
Q="--no-cpu-baseline --sustained-seconds 0"
$B > $O/bench_c3_n1.json 2> $O/err.txt
$B --workload amaze $Q > $O/bench_amaze_n1.json 2>> $O/err.txt
$B --workload amaze --width 8256 --height 5504 $Q > $O/bench_amaze_8256x5504.json 2>> $O/err.txt
$B --workload amaze --width 4000 --height 3000 $Q > $O/bench_amaze_4000x3000.json 2>> $O/err.txt
$B --workload rcd $Q > $O/bench_rcd_n1.json 2>> $O/err.txt
$B --workload c4 $Q > $O/bench_c4_n1.json 2>> $O/err.txt
$B --workload c5 $Q --steps 5 > $O/bench_c5_n1.json 2>> $O/err.txt
$B --lanes 2 $Q > $O/bench_c3_lanes2.json 2>> $O/err.txt
# config 3, one kernel after the other (dn_streams=0: per-kernel durations and counters that do not overlap)
bash $R/scripts/dn_profile.sh r3 c3 > /dev/null 2>&1
# dominant kernels: instruction and traffic counters
prof() {  # workload kernel tag [bench args]
  W=$1; K=$2; T=$3; shift; shift; shift
  (cd /tmp && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_$T -- python $R/bench.py --workload $W $Q --steps 4 --warmup 1 "$@" > /dev/null 2>&1) || true
  find $O/trace_$T -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/${T}_kernel_stats.csv
  for c in FETCH_SIZE WRITE_SIZE "SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_BUSY_CYCLES" "SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_VALU" "SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_SALU SQ_ACTIVE_INST_LDS"; do
    n=$(echo $c | cut -d' ' -f1)
    (cd /tmp && timeout 300 rocprofv3 --pmc $c --output-format csv -d $O/pmc_${T}_$n -- python $R/bench.py --workload $W $Q --steps 2 --warmup 1 "$@" > /dev/null 2>&1) || true
  done
  python $R/scripts/pmc_summary.py $K $O/${K}_pmc_summary.json $O/pmc_${T}_FETCH_SIZE $O/pmc_${T}_WRITE_SIZE $O/pmc_${T}_SQ_INSTS_VALU $O/pmc_${T}_SQ_INSTS_LDS $O/pmc_${T}_SQ_WAIT_INST_ANY > /dev/null
  rm -rf $O/trace_$T $O/pmc_${T}_*
}
prof amaze amaze_stream_kernel amaze
prof rcd rcd_stream_kernel rcd
prof c4 nlm_group_kernel c4
prof c5 xtrans_tiles_kernel c5
nfr=$(python3 -c "
import csv
for r in csv.DictReader(open('$O/c3_kernel_stats.csv')):
    if 'amaze_stream' in r['Name']: print(r['Calls'])")
python $R/scripts/dn_table.py $O/c3_kernel_stats.csv $O/c3_pmc_all.json $nfr $O/c3_per_frame_table.md > /dev/null
ls $O
