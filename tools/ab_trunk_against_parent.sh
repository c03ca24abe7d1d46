# A/B of the trunk kernel against another build of the tree (the parent commit), on one box in one session:
#   1. stamped k_tower1wa (tools/stamps_1wa.py), processes alternating;
#   2. bench.py step pairs, order P P C P C P C P C P C (the two leading P = the noise floor), the last pair with
#      --dump-outputs, compared array for array;
#   3. a counter pass of its own (no tracing) over the trunk kernel alone; 4. a kernel trace under the bench.
# usage: bash tools/ab_trunk_against_parent.sh PARENT_TREE [OUT_DIR]
#   PARENT_TREE: a second copy of the tree at the parent commit with its libxq_hip.so built
#   (git worktree add ../parent HEAD~1 && cd ../parent && python -c "import __graft_entry__ as g; g.build()")
# Every GPU step runs under its own time limit; the first one that fails ends the script.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
PAR=$(cd "${1:?parent tree}" && pwd)
O=${2:-$R/bench_out/ab_trunk}
mkdir -p $O
export TMPDIR=/tmp
step() { # name dir command...
  local name=$1 dir=$2; shift 2
  ( cd $dir && timeout -k 10 240 "$@" ) > $O/$name.txt 2> $O/$name.err; local rc=$?
  echo "$name rc=$rc"
  if [ $rc -ne 0 ]; then tail -5 $O/$name.err; exit 1; fi
}
sha16() { sha256sum $1/chinesechessai_amd/csrc/libxq_hip.so | cut -c1-16; }
echo "parent lib $(sha16 $PAR) change lib $(sha16 $R)" | tee $O/libs.txt
for k in 1 2; do
  step stamps_parent_$k $PAR python tools/stamps_1wa.py
  step stamps_change_$k $R python tools/stamps_1wa.py
done
grep -H "variant 60 stamped\|block 2:" $O/stamps_*.txt
i=0
for w in P P C P C P C P C P C; do
  i=$((i+1)); d=$PAR; [ $w = C ] && d=$R
  extra=""; [ $i -ge 10 ] && extra="--dump-outputs $TMPDIR/ab_dump_$w"
  n=bench_$(printf %02d $i)_$w
  step $n $d python bench.py --gpus 1 --steps 5 --warmup 1 $extra
  tail -1 $O/$n.txt | python -c "import json,sys; d=json.loads(sys.stdin.read()); r=d['roofline']; print('  value %.2f frac %.4f clock %.4f sha %s' % (d['value'], r['frac'], r['clock_ghz'] or 0, d.get('build_libxq_hip_sha16')))"
done
python $R/tools/compare_dumps.py $TMPDIR/ab_dump_P $TMPDIR/ab_dump_C | tee $O/dump_compare.txt | tail -1
for w in P C; do
  d=$PAR; [ $w = C ] && d=$R
  rm -rf $TMPDIR/ab_pmc_$w $TMPDIR/ab_kt_$w
  step pmc_$w $TMPDIR rocprofv3 --pmc SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_INSTS_MFMA SQ_LDS_BANK_CONFLICT SQ_INSTS_LDS --output-format csv -d $TMPDIR/ab_pmc_$w -- python3 $d/tools/tower_only.py 16384 6 60 5
  python $R/tools/pmc_kernel_mean.py $TMPDIR/ab_pmc_$w k_tower1wa | tee $O/pmc_${w}_summary.txt
  step kt_$w $TMPDIR rocprofv3 --kernel-trace --stats --output-format csv -d $TMPDIR/ab_kt_$w -- python3 $d/bench.py --gpus 1 --steps 1 --warmup 0 --profile-plies 4
  find $TMPDIR/ab_kt_$w -name "*kernel_stats.csv" -exec cp {} $O/kernel_stats_$w.csv \;
  grep k_tower1wa $O/kernel_stats_$w.csv | cut -c1-300
done
