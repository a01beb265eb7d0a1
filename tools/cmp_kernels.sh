# usage: [O=<dir>] tools/cmp_kernels.sh "VAR=a VAR2=b" "VAR=c" ...   (one bench.py --full run per argument, environment = the argument;
#   its JSON line and stderr are kept in <dir>, a fresh temporary directory by default)
O=${O:-$(mktemp -d)}; mkdir -p $O
i=0
for cfg in "$@"; do
  i=$((i+1))
  env $cfg python bench.py --full --no-cpu-baseline --steps 100 > $O/cmp_$i.json 2> $O/cmp_$i.err
  python - <<PY
import json
d=json.load(open("$O/cmp_$i.json"))
print("[$cfg]", "main: step/layer", d["attention_latency_us_per_layer"], "stage1", d["roofline"]["avg_launch_us"], "frac", d["roofline"]["frac"])
for n,v in d["other_workloads"].items():
    print("   ", n, v.get("us_per_layer"), v.get("stage1_us"), v.get("stage1_hbm_frac"), v.get("error"))
PY
done
