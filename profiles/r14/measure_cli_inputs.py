import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mapper_amd import api, synth
d = sys.argv[1]
ref = synth.synthetic_reference(5_000_000, seed=0xEC011)
reads = synth.synthetic_single_end(ref, 100_000, seed=0x5EED0001)[0]
open(d + "/ref.fasta", "w").write(">ecoli_syn\n" + api.decode(ref) + "\n")
lut = "?ACMGRSVTWYHKDBN"
with open(d + "/reads.fastq", "w") as f:
    qual = "I" * reads.shape[1]
    for i, r in enumerate(reads):
        f.write("@r%d\n%s\n+\n%s\n" % (i, "".join(lut[c] for c in r), qual))
