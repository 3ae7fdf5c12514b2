#!/usr/bin/env bash
# Negative control for the padding-row fix of the fused training kernel: rebuild with the OLD clearing loop (rows 81..95 only)
# and run the small-board gradient test, which poisons the LDS first -- it must FAIL on 3x3 / 5x5.
# The loop lives in gcn_train_exact.hpp: the rewritten header and the two units that include it are copied into one directory (a
# quoted include finds the header next to the including file first) and replace those units.
set -uo pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
C=$R/alphaquoridorgnn_amd/csrc
mkdir -p /tmp/negctl
sed 's|for (int i = t; i < (96 - V) \* 32; i += 512) st4(Hs + (V + (i >> 5)) \* SA|for (int i = t; i < 15 * 32; i += 512) st4(Hs + (81 + (i >> 5)) * SA|' \
  $C/gcn_train_exact.hpp > /tmp/negctl/gcn_train_exact.hpp
grep -c "81 + (i >> 5)" /tmp/negctl/gcn_train_exact.hpp
cp $C/gcn_train_exact.hip $C/gcn_train_split.hip /tmp/negctl/
AQG_REPLACE="gcn_train_exact=/tmp/negctl/gcn_train_exact.hip gcn_train_split=/tmp/negctl/gcn_train_split.hip" AQG_EXTRA_FLAGS= OUT=/tmp/negctl/lib_old.so OBJDIR= bash $C/build.sh >/dev/null || exit 1
cd $R
AQG_LIB_PATH=/tmp/negctl/lib_old.so python -m pytest tests/test_gpu_parity.py -q -k "small_boards" 2>&1 | tail -4 | cut -c1-160
