# same-box A/B of two builds of the library: recommendersystem_amd/librsys_hip_{old,new}.so alternately copied over librsys_hip.so
# bash tools/dbg/ab_lib.sh [pairs, default 3]      (a run that fails or outlasts its time limit ends the script)
set -e -o pipefail
R=$GRAFT_REPO_ROOT; cd $R
for i in $(seq ${1:-3}); do for v in old new; do cp recommendersystem_amd/librsys_hip_$v.so recommendersystem_amd/librsys_hip.so; timeout -k 10 300 python bench.py --steps 60 --warmup 10 --no-cpu-baseline --no-train-loop --no-kernel-timing 2>/dev/null | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(sys.argv[1], d['ms_per_step'], d['ms_per_step_stats']['median'])" $v; done; done
cp recommendersystem_amd/librsys_hip_new.so recommendersystem_amd/librsys_hip.so
