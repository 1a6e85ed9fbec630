"""One format-heavy command-line job for the kernel trace of round 22: single FASTQ reads parsed, aligned, formatted, summarised and counted on the GPU, so
that every offset scan of the align path's output stages runs (FASTQ stage 3, result stage, SAM, summary, unaligned file, reference counts).

    python format_job.py <root of the tree to run> <work directory> [<reads>]

The tree is named so that the same script runs the parent commit's checkout and this one's; the outputs' SHA-256 are printed so the two can be compared.
"""
import hashlib
import io
import os
import sys

ROOT = os.path.abspath(sys.argv[1])
WORK = sys.argv[2]
READS = int(sys.argv[3]) if len(sys.argv) > 3 else 200_000
sys.path.insert(0, ROOT)

from mapper_amd import api, cli, synth  # noqa: E402

os.makedirs(WORK, exist_ok=True)
a, b = synth.synthetic_reference(600_000, seed=81), synth.synthetic_reference(400_000, seed=82)
elsewhere = synth.synthetic_reference(50_000, seed=85)
reads = (list(synth.synthetic_single_end(a, READS * 6 // 10, seed=83)[0]) + list(synth.synthetic_single_end(b, READS * 3 // 10, seed=84)[0])
         + list(synth.synthetic_single_end(elsewhere, READS // 10, seed=86)[0]))
ref, fq = os.path.join(WORK, "ref.fasta"), os.path.join(WORK, "reads.fastq")
with open(ref, "w") as f:
    f.write(">chrA\n" + api.decode(a) + "\n>chrB\n" + api.decode(b) + "\n")
with open(fq, "w") as f:
    for i, r in enumerate(reads):
        f.write("@r%d\n%s\n+\n%s\n" % (i, api.decode(r), "I" * len(r)))
outs = {"--out-sam": "out.sam", "--out-unaligned": "out.un", "--out-refs-map-count": "counts.txt"}
argv = ["--reference", ref, "--queries", fq, "--batch-size", str(READS // 4 + 1), "--parse-on-gpu", "--format-on-gpu", "--results-on-gpu", "--count-refs-on-gpu"]
for flag, name in outs.items():
    argv += [flag, os.path.join(WORK, name)]
log = io.StringIO()
rc = cli.run(argv, out=log)
text = log.getvalue()
print(text[text.index("Statistics"):] if "Statistics" in text else text)
for name in outs.values():
    print(name, hashlib.sha256(open(os.path.join(WORK, name), "rb").read()).hexdigest()[:16], os.path.getsize(os.path.join(WORK, name)))
sys.exit(rc)
