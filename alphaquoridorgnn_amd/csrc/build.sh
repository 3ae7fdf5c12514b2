#!/usr/bin/env bash
# Build libaqgnn_hip.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=${OUT:-../libaqgnn_hip.so}
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function ${AQG_EXTRA_FLAGS:-}"
# objects go into a directory of this build's own: a caller-supplied OBJDIR must be empty (a stale object from another build
# would otherwise be linked silently when its compile fails)
if [ -n "${OBJDIR:-}" ]; then
  mkdir -p "$OBJDIR"
  if [ -n "$(ls -A "$OBJDIR")" ]; then echo "build.sh: OBJDIR=$OBJDIR is not empty" >&2; exit 2; fi
else
  OBJDIR=$(mktemp -d)
  trap 'rm -rf "$OBJDIR"' EXIT
fi
# The one list of translation units: every diagnostic and A/B build goes through this script (AQG_EXTRA_FLAGS, OUT, OBJDIR).
# AQG_REPLACE="unit=path ..." compiles another version of a unit in its place (absolute paths; e.g. an older gcn_trunk_split.hip).
objs=()
pids=()
replaced=0
for f in legal_mask state_check board_featuriser gcn_pack gcn_trunk_split gcn_trunk_exact gcn_boards_plain gcn_forward gcn_general gcn_boards_general gcn_train gcn_train_exact gcn_train_split gcn_train_final gcn_train_general grad_norm weight_average cnn_forward cnn_train mcts mcts_step mcts_eval mcts_move mcts_gumbel mcts_reuse mcts_improve mcts_record agents augment replay replay_refresh replay_merge replay_surprise row_metrics value_targets capi; do
  src=$f.hip
  for pair in ${AQG_REPLACE:-}; do
    if [ "${pair%%=*}" = "$f" ]; then src=${pair#*=}; replaced=$((replaced + 1)); fi
  done
  if [ "$f" = mcts_step ] || [ "$f" = mcts_eval ] || [ "$f" = replay_surprise ] || [ "$f" = row_metrics ] || [ "$f" = state_check ] || [ "$f" = value_targets ] || [ "$f" = weight_average ]; then
    # the resource lines of the step kernels, of the evaluation launch, of the surprise kernels, of the row-metrics kernels, of the record checker, of the lambda-return kernel and of the averaging kernel are kept: the budget checks below read them
    $HIPCC $FLAGS -Rpass-analysis=kernel-resource-usage -I. -c "$src" -o "${OBJDIR}/aqg_$f.o" 2> "${OBJDIR}/aqg_$f.remarks" &
  else
    $HIPCC $FLAGS -I. -c "$src" -o "${OBJDIR}/aqg_$f.o" &
  fi
  pids+=($!)
  objs+=("${OBJDIR}/aqg_$f.o")
done
if [ "$replaced" -ne "$(echo ${AQG_REPLACE:-} | wc -w)" ]; then echo "build.sh: AQG_REPLACE names a unit that is not built: ${AQG_REPLACE}" >&2; exit 2; fi
# host-only code (CPU baseline agents over the same rule header): plain C++, no device pass
${CXX:-g++} -O2 -std=c++17 -fPIC -Wall -Wno-unknown-pragmas -c host_agents.cpp -o "${OBJDIR}/aqg_host_agents.o" &
pids+=($!)
objs+=("${OBJDIR}/aqg_host_agents.o")
# every compile job is waited for by PID: a bare `wait` returns 0 whatever the jobs did
failed=0
for pid in "${pids[@]}"; do
  wait "$pid" || failed=1
done
if [ "$failed" -ne 0 ]; then
  grep -v "remark:" "${OBJDIR}/aqg_mcts_step.remarks" >&2 || true      # whatever mcts_step.hip's compile said besides the remarks
  grep -v "remark:" "${OBJDIR}/aqg_mcts_eval.remarks" >&2 || true
  grep -v "remark:" "${OBJDIR}/aqg_replay_surprise.remarks" >&2 || true
  grep -v "remark:" "${OBJDIR}/aqg_row_metrics.remarks" >&2 || true
  grep -v "remark:" "${OBJDIR}/aqg_state_check.remarks" >&2 || true
  grep -v "remark:" "${OBJDIR}/aqg_value_targets.remarks" >&2 || true
  grep -v "remark:" "${OBJDIR}/aqg_weight_average.remarks" >&2 || true
  echo "build.sh: a compile job failed" >&2; exit 1
fi
grep -A3 "warning:" "${OBJDIR}/aqg_mcts_step.remarks" "${OBJDIR}/aqg_mcts_eval.remarks" "${OBJDIR}/aqg_replay_surprise.remarks" "${OBJDIR}/aqg_row_metrics.remarks" "${OBJDIR}/aqg_state_check.remarks" "${OBJDIR}/aqg_value_targets.remarks" "${OBJDIR}/aqg_weight_average.remarks" >&2 || true
# Register budget of the step kernels with the heads inside (engine_step_fast_kernel<9, CACHE, true, ..>, the form with policy workgroups
# included: both kinds of its workgroups take step-sized slots): at most
# 128 VGPRs and no scratch, or a step workgroup no longer fits beside a trunk workgroup.  The order of their load rounds is steered
# by scheduling barriers that a compiler update may treat differently: such a build fails here instead of running slower.
# (The kernels' launch bound already caps them at 128 registers -- the compiler spills rather than exceed it -- so the scratch
#  test is the one that fires; the register test guards the day the launch bound is changed.)
awk '/Function Name:/ { k = ($0 ~ /engine_step_fast_kernelILi9ELb[01]ELb1E/) ? $0 : "" }
     k != "" && / VGPRs: / { n++; v = $0; sub(/.* VGPRs: /, "", v); if (v + 0 > 128) { print "build.sh: over 128 VGPRs: " k > "/dev/stderr"; bad = 1 } }
     k != "" && /ScratchSize/ { v = $0; sub(/.*: /, "", v); if (v + 0 != 0) { print "build.sh: scratch in use: " k > "/dev/stderr"; bad = 1 } }
     END { if (n != 4) { print "build.sh: expected four fused step kernels in the resource remarks, found " n + 0 > "/dev/stderr"; bad = 1 } exit bad }' \
  "${OBJDIR}/aqg_mcts_step.remarks" || exit 1
# The Gumbel instantiations of the plain step kernel (engine_step_fast_kernel<N, CACHE, false, false, false, GumbelStep>, four boards with and
# without the evaluation cache): the score of rule 3 adds three logits, three q and a wave maximum to level 0's registers -- no scratch.
awk '/Function Name:/ { k = ($0 ~ /engine_step_fast_kernelILi[3579]ELb[01]ELb0ELb0ELb0EJNS_10GumbelStepE/) ? $0 : "" }
     k != "" && /ScratchSize/ { n++; v = $0; sub(/.*: /, "", v); if (v + 0 != 0) { print "build.sh: scratch in use: " k > "/dev/stderr"; bad = 1 } }
     END { if (n != 8) { print "build.sh: expected eight Gumbel step kernels in the resource remarks, found " n + 0 > "/dev/stderr"; bad = 1 } exit bad }' \
  "${OBJDIR}/aqg_mcts_step.remarks" || exit 1
# The same budget for the evaluation launch (engine_eval_kernel<TRACK>, mcts_eval.hip): its board workgroups are the trunk's, two per CU.
awk '/Function Name:/ { k = ($0 ~ /engine_eval_kernelILi[02]E/) ? $0 : "" }
     k != "" && / VGPRs: / { n++; v = $0; sub(/.* VGPRs: /, "", v); if (v + 0 > 128) { print "build.sh: over 128 VGPRs: " k > "/dev/stderr"; bad = 1 } }
     k != "" && /ScratchSize/ { v = $0; sub(/.*: /, "", v); if (v + 0 != 0) { print "build.sh: scratch in use: " k > "/dev/stderr"; bad = 1 } }
     END { if (n != 2) { print "build.sh: expected two evaluation kernels in the resource remarks, found " n + 0 > "/dev/stderr"; bad = 1 } exit bad }' \
  "${OBJDIR}/aqg_mcts_eval.remarks" || exit 1
# The surprise kernels (replay_surprise.hip: four board sizes of the rows kernel and the counts kernel) carry float64 logarithms in
# fully unrolled register arrays: no scratch, or the arrays have gone to memory.
awk '/Function Name:/ { k = ($0 ~ /replay_surprise_(rows|counts)_kernel/) ? $0 : "" }
     k != "" && /ScratchSize/ { n++; v = $0; sub(/.*: /, "", v); if (v + 0 != 0) { print "build.sh: scratch in use: " k > "/dev/stderr"; bad = 1 } }
     END { if (n != 5) { print "build.sh: expected five surprise kernels in the resource remarks, found " n + 0 > "/dev/stderr"; bad = 1 } exit bad }' \
  "${OBJDIR}/aqg_replay_surprise.remarks" || exit 1
# The row-metrics kernels (row_metrics.hip: four board sizes of the rows kernel, the two launches of the reduction and the hold-out
# mask) carry float64 logarithms and exponentials in fully unrolled register arrays: no scratch, or the arrays have gone to memory.
awk '/Function Name:/ { k = ($0 ~ /replay_row_metrics_kernel|row_metrics_(partial|total)_kernel|replay_holdout_mask_kernel/) ? $0 : "" }
     k != "" && /ScratchSize/ { n++; v = $0; sub(/.*: /, "", v); if (v + 0 != 0) { print "build.sh: scratch in use: " k > "/dev/stderr"; bad = 1 } }
     END { if (n != 7) { print "build.sh: expected seven row-metrics kernels in the resource remarks, found " n + 0 > "/dev/stderr"; bad = 1 } exit bad }' \
  "${OBJDIR}/aqg_row_metrics.remarks" || exit 1
# The record checker (state_check.hip, four board sizes): its wall masks and fill boards live in registers, no scratch.
awk '/Function Name:/ { k = ($0 ~ /states72_check_kernel/) ? $0 : "" }
     k != "" && /ScratchSize/ { n++; v = $0; sub(/.*: /, "", v); if (v + 0 != 0) { print "build.sh: scratch in use: " k > "/dev/stderr"; bad = 1 } }
     END { if (n != 4) { print "build.sh: expected four checker kernels in the resource remarks, found " n + 0 > "/dev/stderr"; bad = 1 } exit bad }' \
  "${OBJDIR}/aqg_state_check.remarks" || exit 1
# The lambda-return kernel (value_targets.hip) holds four rounds of a game's row and of its results in registers: no scratch.
awk '/Function Name:/ { k = ($0 ~ /lambda_values_kernel/) ? $0 : "" }
     k != "" && /ScratchSize/ { n++; v = $0; sub(/.*: /, "", v); if (v + 0 != 0) { print "build.sh: scratch in use: " k > "/dev/stderr"; bad = 1 } }
     END { if (n != 1) { print "build.sh: expected one lambda-return kernel in the resource remarks, found " n + 0 > "/dev/stderr"; bad = 1 } exit bad }' \
  "${OBJDIR}/aqg_value_targets.remarks" || exit 1
# The averaging kernel (weight_average.hip) holds four 16-byte words of the average and of the source per lane in registers: no scratch.
awk '/Function Name:/ { k = ($0 ~ /weight_average_kernel/) ? $0 : "" }
     k != "" && /ScratchSize/ { n++; v = $0; sub(/.*: /, "", v); if (v + 0 != 0) { print "build.sh: scratch in use: " k > "/dev/stderr"; bad = 1 } }
     END { if (n != 1) { print "build.sh: expected one averaging kernel in the resource remarks, found " n + 0 > "/dev/stderr"; bad = 1 } exit bad }' \
  "${OBJDIR}/aqg_weight_average.remarks" || exit 1
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT" "${objs[@]}"
echo "built $(realpath "$OUT")"
