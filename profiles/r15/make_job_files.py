"""argv = dir, reads: the configs[1] reference as ref.fa and that many 150-base reads as reads.fq in dir (the files end_to_end_one.py reads)."""
import os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import numpy as np
from mapper_amd import synth
d, N = sys.argv[1], int(sys.argv[2])
os.makedirs(d, exist_ok=True)
dec = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)
ref = synth.synthetic_reference(5_000_000, seed=0xEC011)
with open(os.path.join(d, "ref.fa"), "wb") as f:
    f.write(b">ecoli_syn\n" + dec[ref].tobytes() + b"\n")
reads = synth.synthetic_single_end(ref, N, read_len=150, seed=0x5EED0E2E)[0]
with open(os.path.join(d, "reads.fq"), "wb") as f:
    for lo in range(0, N, 100_000):
        f.write(b"".join(b"@r%09d\n" % (lo + i) + dec[r].tobytes() + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads[lo:lo + 100_000])))
