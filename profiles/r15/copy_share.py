"""argv = kernel-stats CSV files of `rocprofv3 --kernel-trace --stats` runs: per file, the traced GPU time, the share of the runtime's copy kernels
(names with copyBuffer) and the five kernels with the most time; a run is named by the directory its file lies in.  JSON lines."""
import csv, json, os, sys
for path in sys.argv[1:]:
    rows = list(csv.DictReader(open(path)))
    name = next(k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name"))
    dur = next(k for k in rows[0] if k.lower().startswith("totalduration") or k.lower() == "total_duration_ns")
    total = sum(float(r[dur]) for r in rows)
    copy = sum(float(r[dur]) for r in rows if "copyBuffer" in r[name])
    top = sorted(rows, key=lambda r: -float(r[dur]))[:5]
    print(json.dumps({"run": os.path.basename(os.path.dirname(os.path.abspath(path))), "traced_gpu_ms": round(total / 1e6, 2), "copyBuffer_ms": round(copy / 1e6, 2), "copyBuffer_share": round(copy / total, 4),
                      "top": [[r[name][:60], round(float(r[dur]) / 1e6, 2)] for r in top]}))
