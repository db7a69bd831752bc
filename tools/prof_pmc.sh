#!/bin/bash
# PMC counters and a kernel trace for one conv layer; separate passes.
set -u
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=$R/gpurun_out/pmc
mkdir -p $OUT
SHAPE=${SHAPE:-"96 128 512 512 3 16"}
timeout -k 10 120 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_VALU --output-format csv -d $OUT/p -o run -- python3 $R/tools/prof_conv_one.py $SHAPE fwd,wgrad > $OUT/log.txt 2>&1 || exit 1
timeout -k 10 120 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/t -o run -- python3 $R/tools/prof_conv_one.py $SHAPE fwd,wgrad >> $OUT/log.txt 2>&1 || exit 1
