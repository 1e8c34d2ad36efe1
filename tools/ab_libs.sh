# Same-box A/B of two builds of the library.  Build the other one elsewhere (e.g. `git worktree add /tmp/t <commit>;
# make -C /tmp/t/neural-flow-style_amd/csrc`), then on the GPU box: bash tools/ab_libs.sh /tmp/t/neural-flow-style_amd/libnfs_hip.so [pairs]
# The other build is selected through NFS_LIB_PATH (_lib.py); the product library is not touched.  Per run: the headline
# (iterations/s) and tools/advect_bench.py's three kernel times at 200^3.  Stops at the first run that fails.
# (boxes differ by ~2 % in what they sustain; only runs on one box compare)
OLD=${1:?path of the other libnfs_hip.so}; PAIRS=${2:-3}
cd "$(dirname "$0")/.." || exit 1
F="--steps 40 --warmup 5"
one() {   # one <label> <NFS_LIB_PATH or empty>
  NFS_LIB_PATH=$2 timeout -k 10 300 python bench.py $F > /tmp/ab_libs.$$ 2>&1 || { tail -5 /tmp/ab_libs.$$; return 1; }
  tail -1 /tmp/ab_libs.$$ | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$1 lib  headline', round(d['value'],2), d.get('unit',''))" || return 1
  NFS_LIB_PATH=$2 timeout -k 10 120 python tools/advect_bench.py > /tmp/ab_libs.$$ 2>&1 || { tail -5 /tmp/ab_libs.$$; return 1; }
  grep "^advect" /tmp/ab_libs.$$ | sed "s/^/$1 lib  /"
}
for i in $(seq "$PAIRS"); do
  one old "$OLD" && one HEAD "" || { rm -f /tmp/ab_libs.$$; exit 1; }
done
rm -f /tmp/ab_libs.$$
