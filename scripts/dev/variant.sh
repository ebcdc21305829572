#!/bin/bash
# variant.sh NAME FILE.hip "-DFLAG=1 ..."  -> scripts/dev/_NAME.so: the shipped objects with FILE.hip recompiled under the extra flags
# (for scripts/dev/ab.py; *.so is git-ignored).  Run from the repo root after `make -C flowgnn_amd/csrc`.
# The walks' timing variants (csrc/dev/walk_timing_variants.h: GR_CONFLICT_FREE_WALK, GR_ONE_CODE_WALK, GCN_CF_ROWS, GCN_CF_CODES) and the
# ping-pong kernel live behind -DFLOWGNN_DEV: pass it with them, e.g. variant.sh cf gcn.hip "-DFLOWGNN_DEV -DGCN_CF_ROWS".
# FILE.hip may be one of the files that compile a model's file once more under a macro (the instances of its resident kernel):
#   gin_split_f16 gin_split_pool gin_split_nlogit gin_split_poolsum gin_split_poolmax gin_split_eps (gin_split.hip), gcn_rows gcn_nlogit gcn_poolsum (gcn.hip),
#   gat_nlogit gat_attn gat_poolsum (gat.hip), pna_emb pna_rows pna_f16 pna_emb_f16 pna_rows_f16 (pna.hip), dgn_emb dgn_rows dgn_f16 dgn_emb_f16 dgn_rows_f16 (dgn.hip)
# -- a flag that changes the model's file changes them too, and each is recompiled by its own call: variant.sh sum gin_split_poolsum.hip "-D..."
set -e
name=$1; file=$2; flags=$3
src=flowgnn_amd/csrc
tmp=$(mktemp -d)
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall $flags -c $src/$file -o $tmp/v.o 2>$tmp/log || { grep -A5 "error" $tmp/log | head -60; exit 1; }
objs=""
for o in $src/*.o; do
  if [ "$(basename $o .o)" = "$(basename $file .hip)" ]; then objs="$objs $tmp/v.o"; else objs="$objs $o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o scripts/dev/_$name.so $objs -lpthread
rm -rf $tmp
echo scripts/dev/_$name.so
