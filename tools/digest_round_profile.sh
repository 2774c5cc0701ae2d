#!/bin/bash
# tools/digest_round_profile.sh <round> <tag> — after `bash tools/gpu_round_profile.sh` on the GPU: turn the NEWEST rocprofv3 databases under $QM_PROFILE_OUT
# (default profile_out/, the folder that script wrote) into the
# summaries kept in profiles/ (kernel stats, FETCH_SIZE / WRITE_SIZE per kernel, HBM traffic digest, issued-flops digest, SQ activity, bench line).
# Usage: bash tools/digest_round_profile.sh r02 v19
set -e
cd "$(dirname "$0")/.."
rnd=${1:?round like r02}; tag=${2:?tag like v19}
OUT=${QM_PROFILE_OUT:-profile_out}
newest() { ls -t "$1"/runc/*_results.db | head -1; }
python tools/rocpd_kernel_stats.py "$(newest $OUT/prof_stats)" profiles/${rnd}_rocprofv3_kernel_stats_${tag}.csv | head -12
python tools/rocpd_pmc_summary.py "$(newest $OUT/pmc_fetch)" profiles/${rnd}_pmc_fetch_size_${tag}.csv > /dev/null
python tools/rocpd_pmc_summary.py "$(newest $OUT/pmc_write)" profiles/${rnd}_pmc_write_size_${tag}.csv > /dev/null
python tools/hbm_traffic_digest.py profiles/${rnd}_pmc_fetch_size_${tag}.csv profiles/${rnd}_pmc_write_size_${tag}.csv "${rnd} ${tag}" profiles/hbm_traffic.json | head -6
if [ -d $OUT/pmc_flops_a ]; then
  python tools/rocpd_pmc_summary.py "$(newest $OUT/pmc_flops_a)" profiles/${rnd}_pmc_flops_a_${tag}.csv > /dev/null
  python tools/rocpd_pmc_summary.py "$(newest $OUT/pmc_flops_b)" profiles/${rnd}_pmc_flops_b_${tag}.csv > /dev/null
  python tools/flops_pmc_digest.py profiles/${rnd}_pmc_flops_a_${tag}.csv profiles/${rnd}_pmc_flops_b_${tag}.csv "${rnd} ${tag}" 32 profiles/flops_pmc.json
fi
if [ -d $OUT/pmc_sq ]; then python tools/rocpd_pmc_summary.py "$(newest $OUT/pmc_sq)" profiles/${rnd}_pmc_sq_activity_${tag}.csv > /dev/null; fi
if [ -d $OUT/pmc_lds ]; then python tools/rocpd_pmc_summary.py "$(newest $OUT/pmc_lds)" profiles/${rnd}_pmc_lds_mix_${tag}.csv > /dev/null; fi
cp $OUT/bench.json profiles/${rnd}_bench_${tag}.json
