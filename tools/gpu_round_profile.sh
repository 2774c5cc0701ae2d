#!/bin/bash
# tools/gpu_round_profile.sh [quick] — run on an MI355X: tests, the full bench line, rocprofv3 kernel stats, the two HBM PMC passes and the FP64
# instruction-count passes.  Everything lands under $QM_PROFILE_OUT (default profile_out/); the summaries worth keeping are copied into profiles/ by
# tools/digest_round_profile.sh (run with the same QM_PROFILE_OUT).
set -x
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
OUT=${QM_PROFILE_OUT:-profile_out}
mkdir -p "$OUT"
python qm_control_amd/record_model.py > $OUT/kernel_source_hash.txt      # the sources these counters belong to (bench.py: roofline `stale` on mismatch)
if [ "$1" != "noprof" ]; then
python -m pytest tests -m gpu -x -q > $OUT/pytest_gpu.log 2>&1; tail -5 $OUT/pytest_gpu.log
fi
python bench.py --full --steps 20 --warmup 3 > $OUT/bench.json 2> $OUT/bench.err; tail -c 1500 $OUT/bench.json; tail -5 $OUT/bench.err
if [ "$1" == "quick" ]; then rocprofv3 -L > $OUT/counters.txt 2>&1; grep -i "F64\|MFMA" $OUT/counters.txt | head -40; exit 0; fi
rm -rf $OUT/prof_stats $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_flops_a $OUT/pmc_flops_b
B="python bench.py --full --no-cpu-baseline --no-secondary"
rocprofv3 --kernel-trace --stats -d $OUT/prof_stats -- $B --steps 5 --warmup 2 > $OUT/prof_stats.log 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/pmc_fetch -- $B --steps 3 --warmup 1 > $OUT/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/pmc_write -- $B --steps 3 --warmup 1 > $OUT/pmc_write.log 2>&1
# FP64 instructions the kernels issue (wave-level counts): matrix-core ops in 512-flop units, vector FMA / MUL / ADD / transcendental
rocprofv3 --pmc SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_ADD_F64 --kernel-trace -d $OUT/pmc_flops_a -- $B --steps 3 --warmup 1 > $OUT/pmc_flops_a.log 2>&1
rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_VALU_TRANS_F64 SQ_INSTS_MFMA SQ_WAVES --kernel-trace -d $OUT/pmc_flops_b -- $B --steps 3 --warmup 1 > $OUT/pmc_flops_b.log 2>&1
ls -R $OUT | head -60
rm -rf $OUT/pmc_sq
rocprofv3 --pmc SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS --kernel-trace -d $OUT/pmc_sq -- $B --steps 3 --warmup 1 > $OUT/pmc_sq.log 2>&1
tail -3 $OUT/pmc_sq.log
# LDS pipe and instruction mix (round 6: K1b turned out to be sensitive to LDS instructions and vector instructions, not to scalar ones — profiles/r06_ab_lq_regions.log)
rm -rf $OUT/pmc_lds
rocprofv3 --pmc SQ_INSTS_LDS SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS SQ_INSTS_SALU SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES --kernel-trace -d $OUT/pmc_lds -- $B --steps 3 --warmup 1 > $OUT/pmc_lds.log 2>&1
tail -3 $OUT/pmc_lds.log
