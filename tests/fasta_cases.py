"""FASTA texts for tests/test_fasta_text.py (the rules of mapper_amd/csrc/xm_fasta_rules.h on the host) and tests/test_gpu_fasta.py (the same rules on the
GPU), and the host reader's arrays of a file, concatenated over its batches, which both compare with: the FASTA branch of hostio.read_batches is the
definition of what a '>' record of any number of lines means."""
import numpy as np

import fastq_cases as fc
from mapper_amd import hostio

SPLITS = (0, 1, 7, 100, 1000)
WIDTHS = (1, 59, 60, 63, 64, 65, 80)
LETTERS = b"ACGTTGCAN"


def bases(length, k=0):
    return bytes(LETTERS[(k + i * i) % 9] for i in range(length))


def wrap(seq, width, eol=b"\n"):
    return b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def record(name, seq, width, eol=b"\n"):
    return b">" + name + eol + wrap(seq, width, eol)


def wrapped(width, lengths, eol=b"\n", name=b"w%d_%d some description"):
    return b"".join(record(name % (width, k), bases(n, k), width, eol) for k, n in enumerate(lengths))


def width_lengths(width):
    """1 base, one short of a line, a line, one over, three lines and a bit, and 200 bases."""
    return [n for n in (1, width - 1, width, width + 1, 3 * width + 7, 200) if n >= 1]


def texts():
    """name -> text of a file the host reader takes."""
    d = {"width_%d" % w: wrapped(w, width_lengths(w)) for w in WIDTHS}
    d["one_line_per_record"] = b"".join(b">one%d\n" % k + bases(n, k) + b"\n" for k, n in enumerate((1, 2, 70, 333, 1001)))
    d["crlf"] = wrapped(60, width_lengths(60), eol=b"\r\n")
    d["padded_lines"] = b">pad desc\n \tACGT \n\t\tAC GT\t \nA\tC\n   \n>pad2\n  NNNN\r\r\n \t \nACGT \t\r\n"   # blanks and tabs at both ends go, those inside stay (code 15)
    d["empty_lines"] = b">e1\nACGT\n\nACGT\n\n\n>e2\n\nAC\n\r\n>e3\nGG\n\n\n"                              # inside a record, between records, at the end of the file
    d["no_final_newline"] = wrapped(7, [20, 15])[:-1]
    d["no_final_newline_crlf"] = wrapped(7, [20, 15], eol=b"\r\n")[:-2]
    d["odd_body_lines"] = b">odd\n@ACGT\n+\n >x\nACGT\n+ACGT\n@\n>odd2\n >ACGT\n"                           # '@', '+' and ' >' start body lines: the reader swallows them
    d["letters"] = b">letters\nacgtnACGTN\nUuTtRYSWKMBDHVN\nryswkmbdhvn\n\xc3\xa9\x80\xffX*.-\n"              # lower case, IUPAC, unknown bytes, bytes >= 128
    d["names"] = b">\nACGT\n> blank first\nAC\n>tab\tdescription\nGT\n>name with a description\r\nTT\n>x\r\nA\n"  # empty names; the name ends at the blank or tab
    d["fastq_behind_fasta"] = b">fa\nACGT\n@fq\nACGTACGT\n+\nIIIIIIII\n>fb\nGG\n@fq2\nAC\n+\nII\n"          # the four lines are bases of the record in front of them
    d["mixed_widths"] = b"".join(record(b"m%d" % k, bases(1 + (k * 37) % 211, k), 1 + (k * 7) % 83) for k in range(60))
    return d


def pair_texts():
    """Two files of equally many records whose records differ in length and width."""
    a = wrapped(60, [1, 60, 61, 150, 7]) + b">last1\nAC\nGT"
    b = wrapped(7, [33, 2, 90, 8, 61], eol=b"\r\n", name=b"p%d_%d") + b">last2 mate\n\nTTTT\n\n"
    return a, b


def record_lengths(text):
    """The bases of every record of a text that starts with a header, as the reader counts them."""
    out = []
    for line in text.split(b"\n"):
        if line.endswith(b"\r"):
            line = line[:-1]
        if line.startswith(b">"):
            out.append(0)
        else:
            out[-1] += len(line.strip(b" \t\r"))
    return out


def counts(text):
    """(records, lines) of a text as the cutter announces them: the lines that start with '>', and the lines (a last one without its newline is one)."""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return sum(1 for line in lines if line.startswith(b">")), len(lines)


def reader_arrays(path1, path2=None, split=0, keep_qualities=True, batch_size=1 << 30):
    """What the host reader makes of the file(s), its batches concatenated (with a split size a record's sections may straddle two of them)."""
    parts = []
    for b in hostio.read_batches(path1, path2, batch_size, split=split, keep_qualities=keep_qualities):
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
