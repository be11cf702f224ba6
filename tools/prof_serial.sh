# plain kernel trace (no counters) of the bench with the alignment kernels one at a time: the per-kernel durations that
# bench.py's roofline.avg_launch_ms (HIP events in the same mode, a leg of --full) has to agree with
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
TAG=${1:-r02}
OUT=${OUT:-$R/profile_out}          # where the trace and the bench line go
mkdir -p $OUT
export MNC_DP_SERIAL=1
rm -rf $OUT/serial_$TAG
timeout 200 rocprofv3 --kernel-trace --stats -d $OUT/serial_$TAG -o out --output-format csv -- python3 $R/bench.py --steps 2 --warmup 1 --cpu-sample 0 --full > $OUT/serial_$TAG.json 2> $OUT/serial_$TAG.err
head -8 $(find $OUT/serial_$TAG -name "out_kernel_stats.csv" | head -1)
