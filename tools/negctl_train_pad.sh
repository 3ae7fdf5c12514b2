#!/usr/bin/env bash
# Negative control for the padding-row fix of the fused training kernel: rebuild with the OLD clearing loop (rows 81..95 only)
# and run the small-board gradient test, which poisons the LDS first -- it must FAIL on 3x3 / 5x5.
set -uo pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
mkdir -p /tmp/negctl
sed 's|for (int i = t; i < (96 - V) \* 32; i += 512) st4(Hs + (V + (i >> 5)) \* SA|for (int i = t; i < 15 * 32; i += 512) st4(Hs + (81 + (i >> 5)) * SA|' \
  $R/alphaquoridorgnn_amd/csrc/gcn_train.hip > /tmp/negctl/gcn_train_old.hip
grep -c "81 + (i >> 5)" /tmp/negctl/gcn_train_old.hip
AQG_REPLACE="gcn_train=/tmp/negctl/gcn_train_old.hip" AQG_EXTRA_FLAGS= OUT=/tmp/negctl/lib_old.so OBJDIR= bash $R/alphaquoridorgnn_amd/csrc/build.sh >/dev/null || exit 1
cd $R
AQG_LIB_PATH=/tmp/negctl/lib_old.so python -m pytest tests/test_gpu_parity.py -q -k "small_boards" 2>&1 | tail -4 | cut -c1-160
