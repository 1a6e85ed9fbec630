"""ctypes binding of libxm_hostio.so (include/xmapper_hostio.h): FASTA / FASTQ files -> batch arrays, result streams -> SAM text, in native code.

Host-side plumbing of the standalone harness, not part of the alignment path and not part of the drop-in boundary: the
Java host keeps its own readers and writers (Mapper.java:699-732).  The per-object path of mapper_amd/cli.py (api.Query, sam.records) remains the
reference for the formats; tests/test_hostio.py holds the two equal byte for byte."""
import ctypes as C
import os
import time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_lib", "libxm_hostio.so")


class XmioBatch(C.Structure):
    _fields_ = [("num_queries", C.c_int64), ("mate_count", C.POINTER(C.c_int32)), ("mate_offset", C.POINTER(C.c_int64)), ("mate_length", C.POINTER(C.c_int32)),
                ("codes", C.POINTER(C.c_uint8)), ("codes_length", C.c_int64), ("names", C.c_void_p), ("name_off", C.POINTER(C.c_int64)),
                ("quals", C.c_void_p), ("qual_off", C.POINTER(C.c_int64)), ("has_qual", C.POINTER(C.c_uint8)), ("store", C.c_void_p)]


class XmioStats(C.Structure):
    _fields_ = [("num_queries", C.c_int64), ("num_aligned", C.c_int64), ("total_aligned_length", C.c_int64), ("num_indels", C.c_int64), ("total_penalty", C.c_double)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it first (make -C mapper_amd/hostio, or __graft_entry__.build())" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.xmio_last_error.restype = C.c_char_p
        L.xmio_open.restype = C.c_void_p
        L.xmio_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.c_int32]
        L.xmio_next.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.POINTER(XmioBatch))]
        L.xmio_batch_free.argtypes = [C.POINTER(XmioBatch)]
        L.xmio_close.argtypes = [C.c_void_p]
        L.xmio_write_batch.argtypes = [C.POINTER(XmioBatch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32,
                                       C.POINTER(XmioStats)]
        L.xmio_write_summary.argtypes = [C.POINTER(XmioBatch), C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(XmioStats)]
        L.xmio_java_double.argtypes = [C.c_double, C.c_char_p, C.c_int32]
        L.xmio_last_write_seconds.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.xmio_last_write_seconds.restype = None
        _lib = L
    return _lib


class Batch:
    """One batch of queries as read from the files: numpy views of the native arrays (valid while this object lives)."""

    def __init__(self, ptr, expected_inner, deviation):
        self._ptr = ptr
        b = ptr.contents
        n = int(b.num_queries)
        self.num_queries = n
        self.mate_count = np.ctypeslib.as_array(b.mate_count, shape=(n,))
        self.mate_offset = np.ctypeslib.as_array(b.mate_offset, shape=(2 * n,))
        self.mate_length = np.ctypeslib.as_array(b.mate_length, shape=(2 * n,))
        self.codes = np.ctypeslib.as_array(b.codes, shape=(max(int(b.codes_length), 1),))
        paired = self.mate_count > 1
        self.expected_inner = np.where(paired, float(expected_inner), 0.0)   # single-end Query: expected inner distance 0, deviation 1 (api.Query)
        self.deviation = np.where(paired, float(deviation), 1.0)

    def arrays(self):
        return self.mate_count, self.mate_offset, self.mate_length, self.codes, self.expected_inner, self.deviation

    def __len__(self):
        return self.num_queries

    def close(self):
        if self._ptr is not None:
            lib().xmio_batch_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_batches(path1, path2=None, batch_size=1_000_000, split=0, keep_qualities=False, expected_inner=0.0, deviation=1.0):
    """Generator of Batch objects over a FASTA / FASTQ file (or a pair of them, read in step)."""
    L = lib()
    r = L.xmio_open(os.fsencode(path1), os.fsencode(path2) if path2 else None, int(split), 1 if keep_qualities else 0)
    if not r:
        raise OSError(L.xmio_last_error().decode())
    r = C.c_void_p(r)
    try:
        while True:
            ptr = C.POINTER(XmioBatch)()
            if L.xmio_next(r, int(batch_size), C.byref(ptr)):
                raise ValueError(L.xmio_last_error().decode())
            if not ptr:
                return
            yield Batch(ptr, expected_inner, deviation)
    finally:
        L.xmio_close(r)


class StrictFormError(ValueError):
    """The query files are not what the device parser takes (four-line FASTQ records, '@' headers, 1 .. 30000 bases): the message names file and place."""


class XmioTextBlock(C.Structure):
    _fields_ = [("text1", C.c_void_p), ("bytes1", C.c_int64), ("records1", C.c_int64), ("longest1", C.c_int64),
                ("text2", C.c_void_p), ("bytes2", C.c_int64), ("records2", C.c_int64), ("longest2", C.c_int64), ("store", C.c_void_p),
                ("num_queries", C.c_int64), ("lines1", C.c_int64), ("lines2", C.c_int64), ("format", C.c_int32)]


TEXT_FASTQ, TEXT_FASTA = 0, 1  # XmioTextBlock.format (include/xmapper_hostio.h)


def _text_lib():
    L = lib()
    if not hasattr(L, "_xm_text_ready"):
        L.xmio_text_open.restype = C.c_void_p
        L.xmio_text_open.argtypes = [C.c_char_p, C.c_char_p]
        L.xmio_text_open_split.restype = C.c_void_p
        L.xmio_text_open_split.argtypes = [C.c_char_p, C.c_int32]
        L.xmio_text_open_fasta.restype = C.c_void_p
        L.xmio_text_open_fasta.argtypes = [C.c_char_p, C.c_char_p, C.c_int32]
        L.xmio_first_header_byte.argtypes = [C.c_char_p]
        L.xmio_text_next.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.POINTER(XmioTextBlock))]
        L.xmio_text_block_free.argtypes = [C.POINTER(XmioTextBlock)]
        L.xmio_text_block_free.restype = None
        L.xmio_text_close.argtypes = [C.c_void_p]
        L.xmio_text_close.restype = None
        L._xm_text_ready = True
    return L


class TextBlock:
    """A block of whole records as text (one file's, or a pair's in step) - four-line FASTQ records, or with fasta = True FASTA records of any number of
    lines, whose line counts lines(which) then go to the parser too - for api.ReferenceDatabase.stage_fastq: the GPU parses it.  Before it
    is staged it offers num_queries and longest_line (an upper bound of the longest mate); once staged - the text is released then - it offers what Batch
    does: the six arrays(), mate_count / mate_offset / mate_length / codes, and a _ptr that Writer.write takes (an XmioBatch over the arrays the library
    returned, store NULL).  block[k] is the mates of query k, as pileup.MatchDatabase.add_last(queries=block) reads them.  Staged by a context with
    set_batch_copy(False) the batch stays in HBM: codes is None, on_host False, block[k] raises a ValueError, and _ptr holds no names, codes or qualities.  split > 0: the block was cut
    for a parser that cuts every record into sections of at most that many bases (read_text_blocks(split=...)); num_queries counts the sections."""

    def __init__(self, ptr, keep_qualities, expected_inner, deviation, split=0):
        self._text = ptr
        t = ptr.contents
        self.split = int(split)
        self.fasta = int(t.format) == TEXT_FASTA
        self.num_queries = int(t.num_queries)
        self.paired = bool(t.text2)
        self.longest_line = int(max(t.longest1, t.longest2))
        self.keep_qualities = bool(keep_qualities)
        self.pair_spacing = (float(expected_inner), float(deviation))
        self._ptr = self._staged = self._free = None
        self.times_ms = None

    def text(self, which=0):
        """The bytes of file `which` in this block (before it is staged)."""
        t = self._text.contents
        return C.string_at(t.text2 if which else t.text1, t.bytes2 if which else t.bytes1)

    def records(self, which=0):
        t = self._text.contents
        return int(t.records2 if which else t.records1)

    def lines(self, which=0):
        t = self._text.contents
        return int(t.lines2 if which else t.lines1)

    def attach(self, staged, free):
        """stage_fastq's result: `staged` points to the library's xm_fastq_batch, free(staged) gives it back."""
        self._release_staged()
        f = staged.contents
        n = self.num_queries = int(f.num_queries)  # (with a split size: the sections the kernels cut; stage_fastq has held it against the cutter's count)
        self._staged, self._free = staged, free
        self._batch = XmioBatch(n, f.mate_count, f.mate_offset, f.mate_length, f.codes, f.codes_length, f.names, f.name_off, f.quals, f.qual_off, f.has_qual, None)
        self._ptr = C.pointer(self._batch)
        self.mate_count = np.ctypeslib.as_array(f.mate_count, shape=(n,))
        self.mate_offset = np.ctypeslib.as_array(f.mate_offset, shape=(2 * n,))
        self.mate_length = np.ctypeslib.as_array(f.mate_length, shape=(2 * n,))
        # (a context with set_batch_copy(False) leaves codes, names and qualities in HBM: the library returns NULL for them)
        self.codes = np.ctypeslib.as_array(f.codes, shape=(max(int(f.codes_length), 1),)) if f.codes else None
        self.on_host = bool(f.codes) and bool(f.names)
        paired = self.mate_count > 1
        self.expected_inner = np.where(paired, self.pair_spacing[0], 0.0)
        self.deviation = np.where(paired, self.pair_spacing[1], 1.0)
        self.times_ms = {"h2d": f.h2d_ms, "kernel": f.kernel_ms, "d2h": f.d2h_ms}
        self._release_text()

    def arrays(self):
        if self._ptr is None:
            raise ValueError("the block has not been staged (ReferenceDatabase.stage_fastq)")
        return self.mate_count, self.mate_offset, self.mate_length, self.codes, self.expected_inner, self.deviation

    def __len__(self):
        return self.num_queries

    def __getitem__(self, k):
        self.arrays()
        if self.codes is None:
            raise ValueError("the batch stayed in HBM (ReferenceDatabase.set_batch_copy(False)): its bases are not on the host")
        return [self.codes[self.mate_offset[2 * k + m]:self.mate_offset[2 * k + m] + self.mate_length[2 * k + m]] for m in range(int(self.mate_count[k]))]

    def _release_text(self):
        if self._text is not None:
            lib().xmio_text_block_free(self._text)
            self._text = None

    def _release_staged(self):
        if self._staged is not None:
            self._ptr = None
            self.mate_count = self.mate_offset = self.mate_length = self.codes = None
            self._free(self._staged)
            self._staged = None

    def close(self):
        self._release_text()
        self._release_staged()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def first_header_byte(path):
    """b">" or b"@": the first byte of the file's first line that is not empty (gzip is read through), i.e. which cutter of read_text_blocks the file is
    for; b"" for a file of nothing but empty lines.  Any other first byte is a StrictFormError in the host reader's words."""
    L = _text_lib()
    c = L.xmio_first_header_byte(os.fsencode(path))
    if c < 0:
        message = L.xmio_last_error().decode()
        raise OSError(message) if message.startswith("cannot open") else StrictFormError(message)
    return bytes([c]) if c else b""


def read_text_blocks(path1, path2=None, batch_size=1_000_000, keep_qualities=False, expected_inner=0.0, deviation=1.0, split=0, fasta=False):
    """Generator of TextBlock objects over a four-line FASTQ file (or a pair of them, cut in step): whole records as text, at most batch_size of them.
    split > 0 (a single file): the records will be cut into sections of at most `split` bases by the parser, batch_size counts the sections, and a record
    of more sections than that is a block of its own.  fasta = True: the files hold FASTA records of any number of lines ('>' headers); the blocks carry
    their line counts and block.fasta, and stage_fastq hands them to the FASTA parser."""
    L = _text_lib()
    if split and path2:
        raise ValueError("a split size is for single reads (--paired-queries is not supported with --split-queries-past-size)")
    if fasta:
        r = L.xmio_text_open_fasta(os.fsencode(path1), os.fsencode(path2) if path2 else None, int(split))
    elif split:
        r = L.xmio_text_open_split(os.fsencode(path1), int(split))
    else:
        r = L.xmio_text_open(os.fsencode(path1), os.fsencode(path2) if path2 else None)
    if not r:
        raise OSError(L.xmio_last_error().decode())
    r = C.c_void_p(r)
    try:
        while True:
            ptr = C.POINTER(XmioTextBlock)()
            if L.xmio_text_next(r, int(batch_size), C.byref(ptr)):
                raise StrictFormError(L.xmio_last_error().decode())
            if not ptr:
                return
            yield TextBlock(ptr, keep_qualities, expected_inner, deviation, split)
    finally:
        L.xmio_text_close(r)


class Writer:
    """SAM records (and the unaligned-query file) of the batches of a job, written in query order through file descriptors; keeps Mapper.run's statistics."""

    def __init__(self, contig_names, sam_file=None, unaligned_file=None, threads=None):
        self._names = (C.c_char_p * len(contig_names))(*[n.encode() for n in contig_names])
        self._n = len(contig_names)
        self._sam, self._un = sam_file, unaligned_file
        self.stats = XmioStats()
        self.threads = int(threads or min(32, os.cpu_count() or 1))
        self.seconds = {"format": 0.0, "write": 0.0}  # wall seconds of the write() calls so far: formatting on the host (and counting), and writing the files

    def write(self, batch, result, sam_text=None, summary=None, unaligned_text=None):
        """result: anything with ints / dbls / int_off / dbl_off (api.BatchResult).  sam_text: the batch's SAM records as the GPU formatted them
        (api.SamText, or any bytes-like object): they are written as they are, and the native call only counts the statistics and writes the unaligned queries.
        summary: what the GPU counted of the streams (api.BatchSummary, or anything with its fields): the statistics and the unaligned queries come from it
        (xmio_write_summary) and none of result's streams is read - a result whose streams stayed in HBM has none.  A writer with a SAM file then needs the
        text too, and one with an unaligned-query file a summary that was asked for the list.  unaligned_text: the batch's unaligned queries as the GPU wrote
        them (api.ReferenceDatabase.unaligned_format_last, or any bytes-like object): they are written as they are to the unaligned-query file, and the native
        call gets unaligned_fd = -1; it needs a summary, which the statistics come from (the list is not needed).  A batch that stayed in HBM
        (set_batch_copy(False)) has no arrays on the host to write its unaligned queries from: with an unaligned-query file it needs the text."""
        if unaligned_text is not None and summary is None:
            raise ValueError("the text of the unaligned queries comes with a summary, which the statistics are made of (summary=)")
        if self._un is not None and unaligned_text is None and not getattr(batch, "on_host", True):
            raise ValueError("the batch stayed in HBM (set_batch_copy(False)) and has no arrays on the host: with an unaligned-query file the text must be given (unaligned_text)")
        if summary is None and not getattr(batch, "on_host", True):
            raise ValueError("the batch stayed in HBM (set_batch_copy(False)) and has no arrays on the host for the host's formatter to read: give a summary (and the texts)")
        for f in (self._sam, self._un):
            if f is not None:
                f.flush()
        sam_fd = self._sam.fileno() if self._sam is not None else -1
        if sam_text is not None and sam_fd >= 0:
            t0 = time.perf_counter()
            view = sam_text.view() if hasattr(sam_text, "view") else memoryview(sam_text)
            done = 0
            while done < len(view):
                done += os.write(sam_fd, view[done:])
            self.seconds["write"] += time.perf_counter() - t0
            sam_fd = -1
        un_fd = self._un.fileno() if self._un is not None else -1
        if unaligned_text is not None and un_fd >= 0:
            t0 = time.perf_counter()
            view = unaligned_text.view() if hasattr(unaligned_text, "view") else memoryview(unaligned_text)
            done = 0
            while done < len(view):
                done += os.write(un_fd, view[done:])
            self.seconds["write"] += time.perf_counter() - t0
        if unaligned_text is not None:
            un_fd = -1
        if summary is not None:
            if sam_fd >= 0:
                raise ValueError("a summary holds no alignments to format: with a SAM file the text must be given as well (sam_text)")
            if summary.num_queries != batch.num_queries:
                raise ValueError("the summary of %d queries for a batch of %d" % (summary.num_queries, batch.num_queries))
            pen = np.ascontiguousarray(summary.penalties, dtype=np.float64)
            un = np.ascontiguousarray(summary.unaligned, dtype=np.int64)
            if len(pen) != summary.num_alignments:
                raise ValueError("%d penalties for %d alignments" % (len(pen), summary.num_alignments))
            if un_fd >= 0 and len(un) != batch.num_queries - summary.num_aligned:
                raise ValueError("the summary lists %d unaligned queries of %d (ask for the list: summary_last(want_unaligned=True))" % (len(un), batch.num_queries - summary.num_aligned))
            if lib().xmio_write_summary(batch._ptr, summary.num_aligned, summary.total_aligned_length, summary.num_indels, len(pen), pen.ctypes.data if len(pen) else None,
                                        len(un), un.ctypes.data if len(un) else None, un_fd, C.byref(self.stats)):
                raise RuntimeError(lib().xmio_last_error().decode())
            self._tick_native()
            return
        ints = np.ascontiguousarray(result.ints, dtype=np.int32)
        dbls = np.ascontiguousarray(result.dbls, dtype=np.float64)
        io = np.ascontiguousarray(result.int_off, dtype=np.int64)
        do = np.ascontiguousarray(result.dbl_off, dtype=np.int64)
        if len(io) != batch.num_queries + 1:
            raise ValueError("result streams of %d queries for a batch of %d" % (len(io) - 1, batch.num_queries))
        if lib().xmio_write_batch(batch._ptr, ints.ctypes.data, dbls.ctypes.data, io.ctypes.data, do.ctypes.data, self._n, self._names,
                                  sam_fd, un_fd, self.threads, C.byref(self.stats)):
            raise RuntimeError(lib().xmio_last_error().decode())
        self._tick_native()

    def _tick_native(self):
        """The seconds of this thread's last native write call into self.seconds."""
        fmt, wr = C.c_double(), C.c_double()
        lib().xmio_last_write_seconds(C.byref(fmt), C.byref(wr))
        self.seconds["format"] += fmt.value
        self.seconds["write"] += wr.value


def java_double(x):
    buf = C.create_string_buffer(64)
    n = lib().xmio_java_double(float(x), buf, 64)
    return buf.raw[:n].decode()
