"""One end-to-end run in a fresh process: argv = dir, mode (host | gpu).  Prints one JSON line."""
import io, json, os, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from mapper_amd import cli
d, mode = sys.argv[1], sys.argv[2]
log = io.StringIO()
t0 = time.perf_counter()
rc = cli.run(["--reference", os.path.join(d, "ref.fa"), "--queries", os.path.join(d, "reads.fq"), "--out-sam", os.path.join(d, mode + ".sam")] + (["--parse-on-gpu"] if mode == "gpu" else []), out=log)
t = cli.last_timing
print(json.dumps({"mode": mode, "rc": rc, "Mreads_s": round(t["queries"] / t["stream_seconds"] / 1e6, 4), "stream_seconds": round(t["stream_seconds"], 3), "wall": round(time.perf_counter() - t0, 2), "contexts": t["contexts"]}))
