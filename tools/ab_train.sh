#!/usr/bin/env bash
# Developer A/B of training-step builds on one GPU box: every argument is a set of -D flags for the training units (gcn_train_*.hip;
# "-" = none); each is built into its own library and timed with tools/train_bench.py (run_epoch ms/step per form).
#   bash tools/ab_train.sh "-" "-DMY_SWITCH=2"      (the syntax only: the training units have no timing switch left)
set -euo pipefail
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
i=0
for fl in "$@"; do
  [ "$fl" = "-" ] && flags="" || flags="$fl"
  so=/tmp/libaqgnn_abtrain_$i.so
  AQG_EXTRA_FLAGS="$flags" OUT=$so OBJDIR= bash $ROOT/alphaquoridorgnn_amd/csrc/build.sh >/dev/null
  echo "[$i] $fl"
  AQG_LIB_PATH=$so timeout -k 10 200 python3 $ROOT/tools/train_bench.py 2>/dev/null | grep -E "train_fused=2|fallbacks"
  i=$((i+1))
done
