# the workload's own leg (bench.py --save-fixed-rois) against tools/probes/alter_leg_split.py on the set that run generated: are the leg's numbers the RoI set or the leg?
out=${1:-$(mktemp -d)}; mkdir -p $out; timeout -k 10 400 python bench.py --full --workload resnet50_alter --steps 6 --warmup 3 --no-cpu-baseline --save-fixed-rois $out/alter_rois_now.npy > $out/alter_bench_now.log 2>&1; python - <<EOF
import json,numpy as np
d=json.loads([l for l in open("$out/alter_bench_now.log") if l.startswith("{\"metric")][-1])
fs=d["roofline"]["fixed_set"]; print("bench leg:", {k:round(v["avg_ms"],4) for k,v in fs.items()})
for f in ("$out/alter_rois_now.npy","profiles/roofline_rois_resnet50_alter_weak_r4000.npy"):
    r=np.load(f); w=(r[:,3]-r[:,1]+1)/16; h=(r[:,4]-r[:,2]+1)/16
    print(f, r.shape, "mean w,h in cells %.1f %.1f"%(w.mean(),h.mean()), "images", np.bincount(r[:,0].astype(int)))
EOF
timeout -k 10 300 python tools/probes/alter_leg_split.py $out/alter_rois_now.npy 2>&1 | cut -c1-200 | head -6
