"""One --out-mutations job of 100 000 configs[1]-shaped reads through the command line in this process: wall time of the streaming phase and peak RSS."""
import sys, io, os, resource, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mapper_amd import cli
d, mode = sys.argv[1], sys.argv[2]
extra = {"per_object": ["--per-object"], "streamed": [], "streamed_parse_on_gpu": ["--parse-on-gpu"]}[mode]
t0 = time.perf_counter()
cli.run(["--reference", d + "/ref.fasta", "--queries", d + "/reads.fastq", "--out-mutations", d + "/mut_%s.txt" % mode, "--out-sam", d + "/out_%s.sam" % mode] + extra, out=io.StringIO())
wall = time.perf_counter() - t0
t = cli.last_timing
print("%s: queries %d stream_seconds %.3f contexts %d whole run %.3f s peak RSS %.0f MiB phases %s" % (mode, t["queries"], t["stream_seconds"], t["contexts"], wall,
      resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024, {k: round(v, 3) for k, v in t["phases"].items()}))
