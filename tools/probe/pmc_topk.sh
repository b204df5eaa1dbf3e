#!/bin/bash
# PMC passes over the top-k pre-selection kernel (c2 bench, 262144-user top-30), one rocprofv3 run per pass.
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=gpurun_out/pmc_topk_${1:-a}
mkdir -p $OUT
i=0
for P in "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES" \
         "SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_VALU SQ_INSTS_SALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VALU SQ_INSTS_VMEM_RD SQ_WAIT_INST_LDS"; do
  i=$((i+1))
  timeout -s KILL 120 rocprofv3 --pmc $P --kernel-include-regex topk_kernel --output-format csv -d $OUT/p$i -o run -- python3 -u bench.py --full --config c2 --steps 1 --warmup 0 --no-cpu --topk-users 262144 > $OUT/p$i.txt 2>&1
done
echo pmc done
