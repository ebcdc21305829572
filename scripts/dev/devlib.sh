#!/bin/bash
# devlib.sh [NAME] ["extra flags"] -> scripts/dev/_NAME.so: the whole library built with -DFLOWGNN_DEV (ablation bits, *_ablate options) in a
# scratch object directory, so the shipped objects under flowgnn_amd/csrc stay as they are.  Run from the repo root.
set -e
name=${1:-dev}; flags=$2
src=flowgnn_amd/csrc
obj=${TMPDIR:-/tmp}/flowgnn_devobj_$name
mkdir -p $obj
pids=""
for f in engine engine_config group entry ingest graph_build gin gin_split gin_split_f16 gin_split_pool gin_split_nlogit ginq modelq gcn gcn_rows gcn_nlogit pna pna_emb pna_rows pna_f16 pna_emb_f16 pna_rows_f16 dgn dgn_emb dgn_rows dgn_f16 dgn_emb_f16 dgn_rows_f16 gat gat_nlogit gat_attn gin_split_poolsum gin_split_poolmax gcn_poolsum gat_poolsum gin_split_eps eigen gin_ogbvn gcn_ogbvn gin_wide gin_wide_f16 gin_wide_jk gcn_wide gcn_wide_f16 gcn_wide_jk wide_attn wide_s2s; do
  if [ ! -f $obj/$f.o ] || [ $src/$f.hip -nt $obj/$f.o ] || [ -n "$FORCE" ]; then
    ( /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -DFLOWGNN_DEV $flags -c $src/$f.hip -o $obj/$f.o 2>$obj/$f.log || { grep -A5 "error" $obj/$f.log | head -40; exit 1; } ) &
    pids="$pids $!"
  fi
done
for p in $pids; do wait $p; done
for f in h2d_pack tile_pack; do g++ -O3 -std=c++17 -fPIC -c $src/$f.cpp -o $obj/$f.o; done  # the host-side packer and tile planner: plain C++
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o scripts/dev/_$name.so $obj/*.o -lpthread
echo scripts/dev/_$name.so
