"""One end-to-end run in a fresh process: argv = dir, mode, [tree].  mode is "host" (no flag), "parse", "format", "both", or "parent" (no flag, with the
package of another checkout, `tree`: the commit before this one).  Prints one JSON line."""
import io, json, os, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
d, mode = sys.argv[1], sys.argv[2]
ROOT = sys.argv[3] if len(sys.argv) > 3 else os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from mapper_amd import cli
flags = {"host": [], "parent": [], "parse": ["--parse-on-gpu"], "format": ["--format-on-gpu"], "both": ["--parse-on-gpu", "--format-on-gpu"]}[mode]
log = io.StringIO()
t0 = time.perf_counter()
rc = cli.run(["--reference", os.path.join(d, "ref.fa"), "--queries", os.path.join(d, "reads.fq"), "--out-sam", os.path.join(d, mode + ".sam")] + flags, out=log)
t = cli.last_timing
print(json.dumps({"mode": mode, "rc": rc, "Mreads_s": round(t["queries"] / t["stream_seconds"] / 1e6, 4), "stream_seconds": round(t["stream_seconds"], 3), "wall": round(time.perf_counter() - t0, 2),
                  "contexts": t["contexts"], "phases": {k: round(v, 3) for k, v in t.get("phases", {}).items()}}))
