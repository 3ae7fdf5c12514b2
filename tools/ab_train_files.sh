#!/usr/bin/env bash
# A/B of two versions of gcn_train.hip on one box: bash tools/ab_train_files.sh <old file> (the in-tree file is the new one)
set -euo pipefail
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
old=$(realpath "$1")
for v in old new; do
  so=/tmp/libaqgnn_abtf_$v.so
  replace=""; [ $v = old ] && replace="gcn_train=$old"
  AQG_REPLACE="$replace" AQG_EXTRA_FLAGS= OUT=$so OBJDIR= bash $ROOT/alphaquoridorgnn_amd/csrc/build.sh >/dev/null
done
for v in old new old new; do
  echo "[$v]"; AQG_LIB_PATH=/tmp/libaqgnn_abtf_$v.so timeout -k 10 200 python3 $ROOT/tools/train_bench.py 2>/dev/null | grep -E "train_fused=2"
done
