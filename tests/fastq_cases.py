"""FASTQ texts for tests/test_fastq_text.py (the rules on the host) and tests/test_gpu_fastq.py (the same rules on the GPU), and the host reader's
arrays of a file, which both compare with: hostio.read_batches is the definition of what a FASTQ record means."""
import ctypes as C
import gzip
import os

import numpy as np

from mapper_amd import hostio

# Every rule of mapper_amd/csrc/xm_fastq_rules.h on a record of its own.
RULE_RECORDS = [
    b"@crlf comment\tmore\r\nACGTTGCA\r\n+\r\nIIIIIIII\r\n",                 # CRLF line ends; the name ends at the blank
    b"@tab\tcomment after a tab\nacgtnACGTN\n+tab\n@IIIIIIII!\n",             # a tab ends the name; lower case; a `+name` line; a quality line starting with '@'
    b"@\nUuTtRYSWKMBDHVN\n+\n+IIIIIIIIIIIIII\n",                              # an empty name; U; every IUPAC letter; a quality line starting with '+'
    b"@ blank first\n \t ACGT.-*\t \n+\n\t IIIIIII \t\n",                     # the name is empty when a blank follows '@'; blanks and tabs around sequence and quality
    b"@high\nryswkmbdhvn\xc3\xa9\x80\xffX@+\n+\n" + b"I" * 18 + b"\n",       # lower-case IUPAC; bytes >= 128; letters and signs that are no bases
    b"@cr_in_line\r\nAC GT\r\r\n+\r\nII\tII\r\r\n",                           # blanks inside stay; only one '\r' belongs to the line end, more are trimmed from sequence and quality
]
LAST_RECORD = b"@last and no newline\nGATTACA\n+\nIIIIIII"                    # the last block of a file may lack the final newline


def rule_texts():
    """name -> text of a file: all the rules with and without a final newline, and a file of CRLF records only."""
    body = b"".join(RULE_RECORDS)
    return {"rules_no_final_newline": body + LAST_RECORD, "rules_final_newline": body + LAST_RECORD + b"\n", "crlf_only": RULE_RECORDS[0] * 3 + RULE_RECORDS[5],
            "one_record": LAST_RECORD}


def pair_texts():
    """Two files of equally many records whose records differ in length."""
    a = b"".join(RULE_RECORDS) + LAST_RECORD
    b = b"".join(reversed(RULE_RECORDS)) + b"@mate2\r\nTTTTGGGGCCCCAAAA\r\n+\r\n" + b"#" * 16 + b"\r\n"
    return a, b


def random_fastq(n, seed, length=lambda k: 20 + k % 31, name=lambda k: "read%d" % k, crlf=False):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        seq = "".join("ACGT"[i] for i in rng.integers(0, 4, length(k)))
        out.append("@%s\n%s\n+\n%s\n" % (name(k), seq, "I" * len(seq)))
    text = "".join(out).encode()
    return text.replace(b"\n", b"\r\n") if crlf else text


def write(path, text, gz=False):
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(text)
    return path


def arr(ptr, n, dtype):
    return np.ctypeslib.as_array(ptr, shape=(max(int(n), 1),))[:int(n)].astype(dtype, copy=True)


def batch_dict(c):
    """The arrays of an XmioBatch or an xm_fastq_batch (same fields), copied."""
    n = int(c.num_queries)
    d = {"num_queries": n, "mate_count": arr(c.mate_count, n, np.int32), "mate_offset": arr(c.mate_offset, 2 * n, np.int64), "mate_length": arr(c.mate_length, 2 * n, np.int32),
         "codes": arr(c.codes, c.codes_length, np.uint8), "name_off": arr(c.name_off, 2 * n + 1, np.int64)}
    d["names"] = C.string_at(c.names, int(d["name_off"][-1]))
    if c.qual_off:
        d["qual_off"] = arr(c.qual_off, 2 * n + 1, np.int64)
        d["quals"] = C.string_at(c.quals, int(d["qual_off"][-1]))
        d["has_qual"] = arr(c.has_qual, 2 * n, np.uint8)
    else:
        assert not c.quals and not c.has_qual
        d["qual_off"] = d["quals"] = d["has_qual"] = None
    return d


def reader_arrays(path1, path2=None, keep_qualities=True):
    """What the host reader makes of the file(s), as one batch."""
    out = None
    for b in hostio.read_batches(path1, path2, 1 << 30, keep_qualities=keep_qualities):
        assert out is None
        out = batch_dict(b._ptr.contents)
        b.close()
    return out


def assert_same_arrays(got, want, what=""):
    assert got["num_queries"] == want["num_queries"], what
    for k in ("mate_count", "mate_offset", "mate_length", "codes", "name_off", "names", "qual_off", "quals", "has_qual"):
        if want[k] is None:
            assert got[k] is None, (what, k)
        elif isinstance(want[k], bytes):
            assert got[k] == want[k], (what, k, got[k][:80], want[k][:80])
        else:
            assert got[k] is not None and np.array_equal(got[k], want[k]), (what, k, got[k][:16], want[k][:16])


HERE = os.path.dirname(os.path.abspath(__file__))
