#!/usr/bin/env bash
# A/B of two versions of the fused training step's units on one box: bash tools/ab_train_files.sh <directory of old units>
# Every gcn_train*.hip in that directory replaces the unit of its name (AQG_REPLACE; headers are found next to the old unit first);
# the in-tree files are the new side.  Applies from the commit that split gcn_train.hip into gcn_train_exact / _split / _final on:
# an older gcn_train.hip defines what those units define too and cannot stand in for any of them.
set -euo pipefail
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
if [ $# -ne 1 ] || [ ! -d "$1" ]; then echo "usage: ab_train_files.sh <directory that holds old gcn_train*.hip units>" >&2; exit 2; fi
old=$(realpath "$1")
if ! ls "$old"/gcn_train*.hip >/dev/null 2>&1; then echo "ab_train_files.sh: no gcn_train*.hip in $old" >&2; exit 2; fi
replace=""
for f in "$old"/gcn_train*.hip; do replace="$replace $(basename "$f" .hip)=$f"; done
for v in old new; do
  so=/tmp/libaqgnn_abtf_$v.so
  r=""; [ $v = old ] && r="$replace"
  AQG_REPLACE="$r" AQG_EXTRA_FLAGS= OUT=$so OBJDIR= bash $ROOT/alphaquoridorgnn_amd/csrc/build.sh >/dev/null
done
for v in old new old new; do
  echo "[$v]"; AQG_LIB_PATH=/tmp/libaqgnn_abtf_$v.so timeout -k 10 200 python3 $ROOT/tools/train_bench.py 2>/dev/null | grep -E "train_fused=2"
done
