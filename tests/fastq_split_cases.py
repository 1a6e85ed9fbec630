"""FASTQ texts of reads that are cut into sections (--split-queries-past-size) for tests/test_fastq_split.py (the rule and the stages on the host) and
tests/test_gpu_fastq_split.py (the same on the GPU), and the host reader's arrays of a file with a split size, concatenated over its batches: the split branch
of xmio_next (hostio.read_batches(split=...)) is the definition of what the sections of a record are."""
import numpy as np

import fastq_cases as fc
from mapper_amd import hostio

SPLITS = (1, 3, 10, 1000)


def read_of(length, k=0):
    return bytes(b"ACGTTGCAN"[(k + i * i) % 9] for i in range(length))


def edge_lengths(split):
    """1, split - 1, split, split + 1, 2 split, 2 split + 1 and 10 split + 3 bases (a read has at least one)."""
    return [n for n in (1, split - 1, split, split + 1, 2 * split, 2 * split + 1, 10 * split + 3) if n >= 1]


def edge_text(split):
    """One record per edge length; every other one comes with blanks around its sequence (they are trimmed before the read is cut) and a CRLF line end."""
    out = []
    for k, n in enumerate(edge_lengths(split)):
        seq = read_of(n, k)
        if k % 2:
            out.append(b"@edge%d of %d bases\r\n \t" % (k, n) + seq + b"\t \r\n+\r\n" + b"I" * n + b"\r\n")
        else:
            out.append(b"@edge%d\n" % k + seq + b"\n+\n" + b"I" * n + b"\n")
    return b"".join(out)


def texts(split):
    """name -> text: fastq_cases.rule_texts() (blanks, tabs, CRLF, empty names, no final newline) and the edge lengths of this split size."""
    d = dict(fc.rule_texts())
    d["edge_lengths"] = edge_text(split)
    d["edge_lengths_no_final_newline"] = edge_text(split)[:-1]
    return d


def reader_arrays(path, split, keep_qualities=True, batch_size=1 << 30):
    """What the host reader makes of the file with this split size, its batches concatenated (a record's sections may straddle two of them)."""
    parts = []
    for b in hostio.read_batches(path, None, batch_size, split=split, keep_qualities=keep_qualities):
        parts.append(fc.batch_dict(b._ptr.contents))
        b.close()
    out = {"num_queries": sum(p["num_queries"] for p in parts)}
    for k in ("mate_count", "mate_length", "codes"):
        out[k] = np.concatenate([p[k] for p in parts])
    base = np.cumsum([0] + [len(p["codes"]) for p in parts])
    out["mate_offset"] = np.concatenate([np.where(p["mate_length"] > 0, p["mate_offset"] + base[i], 0) for i, p in enumerate(parts)])  # (a padding mate's offset is 0)
    out["names"] = b"".join(p["names"] for p in parts)
    base = np.cumsum([0] + [len(p["names"]) for p in parts])
    out["name_off"] = np.concatenate([p["name_off"][:-1] + base[i] for i, p in enumerate(parts)] + [base[-1:]])
    if keep_qualities:
        out["quals"] = b"".join(p["quals"] for p in parts)
        base = np.cumsum([0] + [len(p["quals"]) for p in parts])
        out["qual_off"] = np.concatenate([p["qual_off"][:-1] + base[i] for i, p in enumerate(parts)] + [base[-1:]])
        out["has_qual"] = np.concatenate([p["has_qual"] for p in parts])
    else:
        out["quals"] = out["qual_off"] = out["has_qual"] = None
    return out


def sequence_lengths(text):
    """The trimmed length of every record's sequence line, as the reader trims it."""
    lines = text.split(b"\n")
    return [len(lines[k].strip(b" \t\r")) for k in range(1, len(lines), 4)]
