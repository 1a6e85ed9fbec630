"""One end-to-end run in a fresh process: argv = dir, mode, [tree].  mode is "host" (no flag), "format", "results" (--format-on-gpu --results-on-gpu), "all"
(those plus --parse-on-gpu), "host3" / "all3" (the same with --contexts 3), or "parent" (no flag, with the package of another checkout, `tree`: the commit
before this one).  Prints one JSON line."""
import io, json, os, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
d, mode = sys.argv[1], sys.argv[2]
ROOT = sys.argv[3] if len(sys.argv) > 3 else os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from mapper_amd import cli
flags = {"host": [], "parent": [], "format": ["--format-on-gpu"], "results": ["--format-on-gpu", "--results-on-gpu"], "all": ["--parse-on-gpu", "--format-on-gpu", "--results-on-gpu"],
         "host3": ["--contexts", "3"], "all3": ["--parse-on-gpu", "--format-on-gpu", "--results-on-gpu", "--contexts", "3"]}[mode]
log = io.StringIO()
t0 = time.perf_counter()
rc = cli.run(["--reference", os.path.join(d, "ref.fa"), "--queries", os.path.join(d, "reads.fq"), "--out-sam", os.path.join(d, mode + ".sam"), "--batch-size", "500000"] + flags, out=log)
t = cli.last_timing
print(json.dumps({"mode": mode, "rc": rc, "Mreads_s": round(t["queries"] / t["stream_seconds"] / 1e6, 4), "stream_seconds": round(t["stream_seconds"], 3), "wall": round(time.perf_counter() - t0, 2),
                  "contexts": t["contexts"], "phases": {k: round(v, 3) for k, v in t.get("phases", {}).items()}, "statistics": log.getvalue()[log.getvalue().index("Statistics"):]}))
